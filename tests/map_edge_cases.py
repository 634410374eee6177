"""Edge shapes of the resampler, the blur (reni_tu_resample.hip) and the environment-map rotation (reni_tu_rotate.hip): the
case lists, the input builders, the float64 references and the fp32 restatements that tests/test_map_edges_cpu.py and
tests/test_gpu_map_edges.py share.

Plain data on the CPU; nothing here touches a device.  Every builder is deterministic (fixed seeds): treat what it returns as
read-only.  The oracles and bounds are those of tests/test_resample_cpu.py and tests/test_rotate_cpu.py; what is added here
is the table sum with the two tap counts separated (the generic instance takes any ty, tx), the blur's per-pixel bound, and
the rule for where a nearest tap may differ from the oracle's."""
import functools
import math

import numpy as np

from tests.test_resample_cpu import EPS32, np_gaussian_blur
from tests.test_rotate_cpu import (A_ROW, B_COL, CAP, FLIP_X, FLIP_Y, FLIP_Z, Rx, Ry, rotation_list, sky_maps, source_coordinates)

MODES = ("nearest", "bilinear", "bicubic", "lanczos4")
ROOM = 0.5  # an fp32 restatement of a case may use at most this share of the bound the GPU test applies


def fma32(a, b, c):
    """fmaf: the product and the sum exact in float64 (a 48-bit product), rounded to fp32 once"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def maps(n, c, h, w, seed):
    """[n, c, h, w] float32 of sky_maps (positive, one 2000.0 spot, map 1 shifted negative): its three channels, and further
    draws of it (seed + 1, ...) where c > 3"""
    blocks = [sky_maps(n, h, w, seed + k) for k in range((c + 2) // 3)]
    x = np.ascontiguousarray(np.concatenate(blocks, 1)[:, :c])
    x.setflags(write=False)
    return x


# ================================================================================================ 1. resampler
# (source H, W) -> (target H, W), all four modes at N = 2, C = 3.  Sources of size 1 and 2: every bicubic and Lanczos tap is a
# clamped border tap.  Targets of 255, 256 and 257 pixels: the tail guard of the 256-thread block.  9 x 9 -> 9 x 9: an identity.
RESAMPLE_PAIRS = (((1, 1), (1, 1)), ((1, 1), (5, 7)), ((1, 2), (3, 257)), ((2, 1), (255, 1)), ((3, 5), (1, 1)),
                  ((7, 3), (16, 16)), ((2, 2), (17, 15)), ((300, 5), (1, 256)), ((5, 300), (257, 1)), ((9, 9), (9, 9)),
                  ((8, 8), (7, 9)), ((1000, 3), (3, 1000)))
IDENTITY_PAIR = ((9, 9), (9, 9))
# (N, C, pair): the grid's y and z extents other than (3, 2)
RESAMPLE_NC = ((1, 1, ((8, 8), (7, 9))), (3, 5, ((2, 2), (17, 15))))
RESAMPLE_CASES = tuple((2, 3, p) for p in RESAMPLE_PAIRS) + RESAMPLE_NC
# real weights through the C entry point, (ty, tx): tx = 3, 5, 6, 7 take the generic instance k_resample<0> (dispatch is on tx
# alone), (8, 1) and (1, 8) the two outermost register instances with the other extreme of the shared row loop
GENERIC_TAPS = ((3, 3), (5, 5), (6, 7), (7, 6), (8, 1), (1, 8), (2, 5), (3, 4))
# each register instance with a row tap count other than its own
REGISTER_TAPS = ((3, 1), (5, 2), (7, 4), (2, 8))
TABLE_SIZES = (((37, 91), (50, 23)), ((1, 2), (3, 257)))
CARVED_TARGETS = ((15, 17), (16, 16), (1, 257))  # 255, 256 and 257 output pixels


def resample_input(N, C, pair):
    (hs, ws), _ = pair
    return maps(N, C, hs, ws, hs + ws)


def random_tables(n_in, n_out, taps, seed, wild=False):
    """(idx int32 [n_out, taps], w float32 [n_out, taps]): random in-range indices and signed weights of magnitude 0.1 .. 1,
    none zero.  wild: indices drawn from [-3, n_in + 4] instead, both ends present (the kernel clamps them)."""
    g = np.random.default_rng(seed)
    if wild:
        idx = g.integers(-3, n_in + 5, (n_out, taps))
        idx[0, 0], idx[-1, -1] = -3, n_in + 4
    else:
        idx = g.integers(0, n_in, (n_out, taps))
    w = g.uniform(0.1, 1.0, (n_out, taps)) * g.choice([-1.0, 1.0], (n_out, taps))
    return idx.astype(np.int32), w.astype(np.float32)


def table_sum(src, ri, rw, ci, cw, absolute=False):
    """float64: out[..., y, x] = sum_j rw[y, j] sum_k cw[x, k] src[..., ri[y, j], ci[x, k]]; absolute: sum |w| |w| |src|"""
    src, rw, cw = np.asarray(src, np.float64), np.asarray(rw, np.float64), np.asarray(cw, np.float64)
    if absolute:
        src, rw, cw = np.abs(src), np.abs(rw), np.abs(cw)
    rows = sum(src[..., ri[:, j], :] * rw[:, j][:, None] for j in range(ri.shape[1]))
    return sum(rows[..., :, ci[:, k]] * cw[:, k] for k in range(ci.shape[1]))


def table_bound(src, ri, rw, ci, cw):
    """resample_bound with the two tap counts separated: (ty + tx + 4) 2^-24 sum |w| |w| |src|"""
    return (ri.shape[1] + ci.shape[1] + 4) * EPS32 * table_sum(src, ri, rw, ci, cw, absolute=True)


def table_sum_fp32(src, ri, rw, ci, cw):
    """k_resample restated: fp32 weights, the inner fmaf chain over k ascending from 0, the outer over j ascending from 0"""
    src, rw, cw = np.asarray(src, np.float32), np.asarray(rw, np.float32), np.asarray(cw, np.float32)
    Hs, Ws = src.shape[-2:]
    ri, ci = np.clip(ri, 0, Hs - 1), np.clip(ci, 0, Ws - 1)
    acc = np.zeros(src.shape[:-2] + (ri.shape[0], ci.shape[0]), np.float32)
    for j in range(ri.shape[1]):
        rows = src[..., ri[:, j], :]
        s = np.zeros_like(acc)
        for k in range(ci.shape[1]):
            s = fma32(cw[:, k], rows[..., :, ci[:, k]], s)
        acc = fma32(rw[:, j][:, None], s, acc)
    return acc


def mode_tables(pair, mode):
    """(ri, rw, ci, cw) of reni_amd.resample.resample_tables, the weights float64"""
    from reni_amd.resample import resample_tables
    (hs, ws), (hd, wd) = pair
    return resample_tables(hs, hd, mode) + resample_tables(ws, wd, mode)


# ================================================================================================ 2. blur
BLUR_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (16, 16), (1, 257), (255, 1), (5, 52), (40, 40))
BLUR_SIGMAS = (0.1, 0.5, 1, 3, 5, 12.3)  # radius 0 (bit-identity), 2, 4, 12, 20, 49
BLUR_CHANNELS = (1, 3, 4)
BLUR_WORKSPACE_SHAPES = ((5, 52), (1, 257))


def blur_radius(sigma):
    return int(4.0 * sigma + 0.5)


def blur_image(C, H, W, n):
    """[H, W, C] float32: map n (0: positive, 1: with negatives) of the sky maps at this shape, channel-last"""
    return np.ascontiguousarray(maps(2, C, H, W, 3 * H + W)[n].transpose(1, 2, 0))


def blur_bound(img, sigma):
    """Per-pixel bound on |fp32 kernel - np_gaussian_blur(img, sigma, fp32_intermediate=False)|:

        2 (2 r + 3) 2^-24 blur_f64(|img|)

    Each axis is a chain of 2 r + 1 fmaf over weights rounded to fp32 once: a weight's rounding (u relative per term) and
    the chain's 2 r + 1 roundings of partial sums, each at most the absolute sum, cost (2 r + 2) u times the absolute sum of
    that axis.  The second axis carries the first's error through positive weights of sum 1, so the two add and both scale
    with the blur of |img|.  One more u per axis covers the second-order terms.  Unlike max|img| (blur_bound of
    tests/test_resample_cpu.py) this follows the image: away from the bright spot it is 10^4 times tighter."""
    r = blur_radius(sigma)
    return 2 * (2 * r + 3) * EPS32 * np_gaussian_blur(np.abs(np.asarray(img, np.float64)), sigma, fp32_intermediate=False)


def blur_fp32(img, sigma):
    """k_blur_axis twice, restated: fp32 weights, one fmaf chain per axis over t = -r .. r ascending, axis 0 first"""
    from reni_amd.resample import gaussian_weights, reflect_indices
    x = np.asarray(img, np.float32)
    w, r = gaussian_weights(sigma)
    w = w.astype(np.float32)
    H, W = x.shape[:2]
    iy, ix = reflect_indices(H, r), reflect_indices(W, r)
    mid = np.zeros_like(x)
    for t in range(2 * r + 1):
        mid = fma32(w[t], x[iy[:, t]], mid)
    out = np.zeros_like(x)
    for t in range(2 * r + 1):
        out = fma32(w[t], mid[:, ix[:, t]], out)
    return out


# ================================================================================================ 3. rotation
# (H, W): W = 2 (half = 1: both column wraps at once), H = 1, 2, 3 (both pole crossings on one pixel, the H == 1 clamp),
# W / 2 odd, H W no multiple of 256 except at 16 x 16 and 8 x 64
ROTATE_SHAPES = ((1, 2), (1, 8), (2, 2), (2, 6), (3, 10), (5, 6), (7, 36), (9, 30), (17, 30), (16, 16), (33, 8), (8, 64))
ROTATE_CHANNEL_SHAPE = (9, 30)  # C = 1 and C = 5 here; C = 3 everywhere
ROTATE_CARVED_SHAPE = (7, 36)
NONFINITE_SHAPES = ((5, 6), (16, 16))
GENERAL_MIN_H = 7  # from here on all of rotation_list(); below, the polar caps hold most of the sphere


def rotate_input(H, W, C=3):
    return maps(2, C, H, W, 5 * H + W)


def yaws(W):
    """a yaw keeps the polar angle: the oracle leaves out no pixel at any H"""
    return [("Ry(0.7)", Ry(0.7)), ("Ry(-2.9)", Ry(-2.9)), ("Ry(pi/W)", Ry(math.pi / W)), ("Ry(1e-4)", Ry(1e-4))]


def bilinear_rotations(H, W):
    """[(name, R float32, yaw?)]: the matrices as the kernel is given them"""
    out = [(n, R.astype(np.float32), True) for n, R in yaws(W)]
    if H >= GENERAL_MIN_H:
        out += [(n, R.astype(np.float32), False) for n, R in rotation_list()]
    return out


POLE_CAP = 0.25


def pole_pixels(H, W, R):
    """[H, W] bool: pixels whose bilinear cell reaches beyond a pole (row < 0 or row > H - 1: two of the four taps are read on
    the far side, W / 2 columns away) with sin phi_s >= POLE_CAP sin(pi / 2H).  rotate_bound's keep (CAP = 0.999) leaves out
    the whole half row round a pole, which is exactly where such a tap carries weight; the bound itself is first order in
    u / sin phi_s and stays valid much closer to the pole: at POLE_CAP and H <= 33 the direction error 8.2 u / sin phi_s is below
    4.1e-5 rad, so what the first order leaves out is 4e-5 of what it counts."""
    row, _, sin_s = source_coordinates(H, W, R)
    return (sin_s >= POLE_CAP * math.sin(math.pi / (2 * H))) & ((row < -1e-6) | (row > H - 1 + 1e-6))


def pixel_yaws(W):
    return [(k, Ry(k * 2 * math.pi / W)) for k in (1, -1, W // 2 - 1, W - 1)]


def nearest_exact_cases(x):
    """[(name, R, expected)] for x [..., H, W] (numpy): the identity, the half turns and the whole-pixel yaws"""
    W = x.shape[-1]
    flip = x[..., ::-1, ::-1]
    cases = [("identity", np.eye(3), x), ("FLIP_Y", FLIP_Y, np.roll(x, W // 2, -1)), ("FLIP_Z", FLIP_Z, flip),
             ("FLIP_X", FLIP_X, np.roll(flip, W // 2, -1))]
    return cases + [(f"Ry({k} 2 pi / W)", R, np.roll(x, -k, -1)) for k, R in pixel_yaws(W)]


def nearest_rotations():
    """rotation_list() for nearest against the oracle, with Rx(1.5) in place of Rx(pi/2): a quarter turn about x puts source
    coordinates of the 7 x 36 and 33 x 8 grids on exact half-integers, where the tap is a matter of the last bit"""
    return [(("Rx(1.5)", Rx(1.5)) if n == "Rx(pi/2)" else (n, R)) for n, R in rotation_list()]


def nearest_permitted(H, W, R):
    """(permitted [H, W] bool, keep [H, W] bool, margin): where a nearest tap may differ from the float64 oracle's -- the
    float64 source coordinate within A_ROW H u (rows) or B_COL W u / sin phi_s (columns) of a half-integer, outside the polar
    caps -- and the smallest distance / threshold over the pixels outside the caps"""
    row, col, sin_s = source_coordinates(H, W, R)
    keep = sin_s >= CAP * math.sin(math.pi / (2 * H))
    dr = np.abs(row - np.floor(row) - 0.5) / (A_ROW * H * EPS32)
    dc = np.abs(col - np.floor(col) - 0.5) / (B_COL * W * EPS32 / np.maximum(sin_s, 1e-300))
    near = (dr <= 1.0) | (dc <= 1.0)
    margin = float(np.minimum(dr, dc)[keep].min()) if keep.any() else math.inf
    return near & keep, keep, margin


NONFINITE = (("all NaN", np.full((3, 3), np.nan)), ("one +inf", np.where(np.arange(9).reshape(3, 3) == 5, np.inf, np.eye(3))),
             ("all 1e30", np.full((3, 3), 1e30)), ("all zero", np.zeros((3, 3))))
INDEX_B7 = (1, 0, 0, 1, 1, 0, 1)  # B = 7 images from N = 2, with repeats
