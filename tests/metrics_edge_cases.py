"""Edge shapes and edge values of the map scores (reni_tu_metrics.hip) and wide rows of the light tables (reni_tu_lights.hip):
the case lists, the input builders and the float64 references that tests/test_metrics_edges_cpu.py and
tests/test_gpu_metrics_edges.py share.

Plain data on the CPU; nothing here touches a device.  Every builder is cached and deterministic: treat what it returns as
read-only.  The oracles and the error budget are those of tests/test_metrics_cpu.py and tests/test_lighting_cpu.py; nothing
is restated here."""
import functools

import numpy as np

from oracle import reni_oracle as O
from tests.test_lighting_cpu import np_light_table, np_omega, sky_maps
from tests.test_metrics_cpu import (np_exposure, np_map, np_pair_stats, np_ssim_map, pair_maps, sin_rows, sphere_pad, ssim_budget,
                                    ssim_mean, stats_budget)

MM = O.MINMAX
SPACES = ("stored", "linear", "srgb")
B = 2
PS_CHUNK = 2048  # pixels per workgroup of k_pair_stats
SS_T = 32        # k_ssim's tile

# ---------------------------------------------------------------------------------------------- 1. shapes
# pair_stats alone (any H, W): the smallest images; 21 pixels (one chunk, mostly the clamped tail); the chunk boundary;
# nblk = 7, 8, 9 (fewer strands of k_finish than 8, exactly 8, a strand with two partials of which the last holds 2 pixels); 17
PAIR_SHAPES = ((1, 1), (1, 2), (3, 7), (1, 2047), (1, 2048), (1, 2049), (7, 2048), (4, 4096), (3, 5462), (17, 1928))
# sphere SSIM (W even, H >= 5): W < 11 (a window wraps the row, every window crosses a pole; both poles at H = 5); small partial
# tiles; the tile boundary in both axes; partial tiles in both axes with W / 2 odd; three tile rows and a last tile column 2
# wide; whole tile columns with partial tile rows
SPHERE_SHAPES = ((5, 2), (6, 4), (5, 10), (7, 12), (11, 12), (31, 64), (32, 64), (33, 66), (37, 50), (65, 34), (43, 96))
# planar SSIM (H, W >= 11): one window; a one-row and a one-column interior; interior 32 x 33; partial tiles
PLANAR_SHAPES = ((11, 11), (11, 12), (12, 11), (42, 43), (37, 50), (33, 66), (43, 96))
WEIGHT_KINDS = ("none", "sin", "random")
VALUE_SHAPE = (37, 50)  # the value cases: partial tiles in both axes, one chunk of k_pair_stats


def nblk(H, W):
    """workgroups (partials) of k_pair_stats per image"""
    return (H * W + PS_CHUNK - 1) // PS_CHUNK


def ssim_L(space, target):
    """tests/test_gpu_metrics.py's _ssim_L"""
    return {"stored": 2.0, "linear": float(np_map(target, "linear", MM, None).max()), "srgb": 1.0}[space]


@functools.lru_cache(maxsize=None)
def shape_inputs(H, W):
    """(pred, target [B, 3, H, W] float32 in stored space, exposure [B] float32)"""
    pred, target = pair_maps(B, H, W, H + W)
    return pred, target, np_exposure(target, MM)


@functools.lru_cache(maxsize=None)
def weight(kind, H, W):
    """None, sin(phi) per row as [H, 1], or a per-pixel random weight [B, H, W] in [0, 1] with about a quarter exactly 0"""
    if kind == "none":
        return None
    if kind == "sin":
        return sin_rows(H)[:, None].astype(np.float32)
    assert kind == "random"
    g = np.random.default_rng(7 * H + W)
    w = g.random((B, H, W)).astype(np.float32)
    w[g.random((B, H, W)) < 0.25] = 0.0
    if not (w > 0).reshape(B, -1).any(1).all():  # (1 x 1, 1 x 2: an image needs a live pixel for a score to exist)
        w[:, 0, 0] = 0.5
    return w


def stats_reference(pred, target, w, space, expo):
    """(float64 oracle [B, 8], budget [B, 8])"""
    return np_pair_stats(pred, target, w, space, MM, expo), stats_budget(pred, target, w, space, MM, expo)


def ssim_reference(pred, target, space, expo, L, sphere):
    """(float64 map [B, H, W], kappa [B, H, W])"""
    return np_ssim_map(pred, target, space, MM, expo, L, sphere, with_kappa=True)


def interior(H, W, sphere):
    """boolean [H, W]: the pixels that have a window"""
    m = np.ones((H, W), bool)
    if not sphere:
        m[:] = False
        m[5:H - 5, 5:W - 5] = True
    return m


def stats_ratio(got, ref, bud):
    """largest err / budget over the entries with a budget; asserts exact equality where the budget is 0"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    exact = bud == 0
    assert np.array_equal(got[exact], ref[exact]), (got, ref)
    return float((err[~exact] / bud[~exact]).max()) if (~exact).any() else 0.0


def map_ratio(gmap, smap, pix, sphere):
    """largest per-pixel err / budget over every pixel that has a window; asserts the planar border is exactly 0"""
    gmap = np.asarray(gmap, np.float64)
    H, W = gmap.shape[-2:]
    inn = interior(H, W, sphere)
    assert not gmap[:, ~inn].any()
    return float((np.abs(gmap - smap)[:, inn] / pix[:, inn]).max())


def mean_ratio(mean, smap, w, img, sphere):
    return float((np.abs(np.asarray(mean, np.float64) - ssim_mean(smap, w, sphere)) / img).max())


# ---------------------------------------------------------------------------------------------- 2. values
def window_hits(bad, sphere):
    """boolean [H, W]: the pixels whose 11 x 11 window holds a pixel of `bad` [H, W] -- on the sphere by sphere_pad's tap rule
    (a row beyond a pole is the row seen from the other side, W / 2 columns on; columns modulo W), in planar mode only the
    pixels that have a window at all"""
    H, W = bad.shape
    x = np.asarray(bad, np.float64)
    if sphere:
        x = sphere_pad(x)
        return sum(x[k:k + H, l:l + W] for k in range(11) for l in range(11)) > 0
    out = np.zeros((H, W), bool)
    out[5:H - 5, 5:W - 5] = sum(x[k:k + H - 10, l:l + W - 10] for k in range(11) for l in range(11)) > 0
    return out


# stored values that no score can digest: a NaN, the infinities, and a number whose radiance overflows (exp(0.5 x 101 x 29.5 - 18))
BAD_VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf"), "overflow": 100.0}


def mapped_is_finite(value, space):
    """whether the bad stored value is a finite number once mapped into `space`: exp(-inf) is 0, and the sRGB clamp turns an
    infinite radiance into 1"""
    if value != value:
        return False
    if space == "stored":
        return bool(np.isfinite(value))
    return value < 0 or space == "srgb"


def hidden_masks(H, W):
    """{name: boolean [H, W]}: where the bad pixels of the weight-0 cases lie"""
    first, last, tail, tile = (np.zeros((H, W), bool) for _ in range(4))
    first[0, 0] = True
    last[-1, -1] = True
    tail.reshape(-1)[[(nblk(H, W) - 1) * PS_CHUNK, H * W - 2]] = True  # the last chunk's first pixel and one next to the clamp
    tile[:SS_T, :SS_T] = True
    return {"first": first, "last": last, "tail": tail, "tile": tile}


@functools.lru_cache(maxsize=None)
def constant_pair(space):
    """(pred, target, exposure): two different constant images at VALUE_SHAPE.  In a mapped space the prediction is the darker
    one, so that kappa = 1 + 2 (a^2 + b^2) / C2 stays at or below 1 + 4 / 9e-4 (L is the target's value)"""
    H, W = VALUE_SHAPE
    a, b = ((0.3, 0.5), (-0.2, 0.7)) if space == "stored" else ((-0.1, 0.0), (0.1, 0.2))
    pred = np.stack([np.full((3, H, W), a[i], np.float32) for i in range(B)])
    target = np.stack([np.full((3, H, W), b[i], np.float32) for i in range(B)])
    return pred, target, np_exposure(target, MM)


def constant_ssim(pred, target, space, expo, L):
    """[B] float64: (2 a b + C1) / (a^2 + b^2 + C1) of the mapped constants (test_oracle_ssim_of_constant_images)"""
    a = np_map(pred, space, MM, expo)[:, 0, 0, 0]
    b = np_map(target, space, MM, expo)[:, 0, 0, 0]
    C1 = (0.01 * L) ** 2
    return (2 * a * b + C1) / (a * a + b * b + C1)


@functools.lru_cache(maxsize=None)
def black_pixel_pair():
    """shape_inputs(VALUE_SHAPE) with p = 0 at one pixel, t = 0 at another and both at a third (all three channels, in stored
    space): the norms of F.cosine_similarity's eps = 1e-20 rule are at their floor there"""
    pred, target, _ = shape_inputs(*VALUE_SHAPE)
    pred, target = pred.copy(), target.copy()
    pred[:, :, 3, 4] = 0.0
    target[:, :, 20, 33] = 0.0
    pred[:, :, 36, 49] = 0.0
    target[:, :, 36, 49] = 0.0
    return pred, target, np_exposure(target, MM)


@functools.lru_cache(maxsize=None)
def extreme_exposures():
    """(toe, clamp) [B] float32 for shape_inputs(VALUE_SHAPE): under the first every sRGB argument is below the curve's linear
    toe (0.0031308), under the second every one clamps to 1 (constant images: the largest kappa of this file)"""
    pred, target, _ = shape_inputs(*VALUE_SHAPE)
    lin = np.stack([np_map(pred, "linear", MM, None), np_map(target, "linear", MM, None)])
    hi, lo = lin.max((0, 2, 3, 4)), lin.min((0, 2, 3, 4))
    return (hi * 1e3).astype(np.float32), (lo * 0.5).astype(np.float32)


def value_pairs():
    """[(name, pred, target, {space: exposure})]: every pair of images whose SSIM budget the CPU test holds to the 5e-3 cap"""
    pred, target, expo = shape_inputs(*VALUE_SHAPE)
    toe, clamp = extreme_exposures()
    bp, bt, be = black_pixel_pair()
    zero = np.zeros_like(target)
    out = [("self", target, target, {s: expo for s in SPACES}),
           ("black pixels", bp, bt, {s: be for s in SPACES}),
           ("zero", zero, zero, {s: np_exposure(zero, MM) for s in SPACES}),
           ("toe", pred, target, {"srgb": toe}), ("clamp", pred, target, {"srgb": clamp})]
    out.append(("constant", None, None, {s: None for s in SPACES}))
    return out


def value_pair(name, space):
    """(pred, target, exposure) of one entry of value_pairs in one space"""
    if name == "constant":
        return constant_pair(space)
    for n, p, t, e in value_pairs():
        if n == name:
            return p, t, e[space]
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------- 4. light tables: wide rows
LT_TILE = 256                         # entries per tile of a row scan
LIGHT_WIDTHS = ((1024, 2), (4096, 1))  # (W, B): 4 row tiles and 2 marginal tiles; LT_MAX_W: 16 and 8
LIGHT_MIXES = (0.0, 0.25)
LIGHT_PMF_REL = 4 * 2.0 ** -24        # the budgets of tests/test_gpu_lighting.py::test_tables_match_float64_in_stored_space
LIGHT_CDF_ABS = 2.0 ** -22


@functools.lru_cache(maxsize=None)
def light_maps(W, Bn):
    """[Bn, W / 2, W, 3] float32 radiance; row 1 is black"""
    return sky_maps(Bn, W, 100 + W)


@functools.lru_cache(maxsize=None)
def light_reference(W, Bn, eps, mask_name=None):
    """float64 (pmf, cond, marg) of light_maps(W, Bn)"""
    mask = None if mask_name is None else light_masks(W)[mask_name]
    return np_light_table(light_maps(W, Bn).astype(np.float64), np_omega(W), mask=mask, eps=eps)


@functools.lru_cache(maxsize=None)
def light_masks(W):
    """{name: float32 [H, W] of 0 and 1}: mass placed so that one carry of the tiled scans is the only thing that can get the
    CDF right: texels in column 0 only, in column W - 1 only, inside the third tile only (columns 512..767); lit rows only in
    the marginal's second tile (i >= 256), only in its first"""
    H = W // 2
    assert W >= 4 * LT_TILE and H >= 2 * LT_TILE
    m = {k: np.zeros((H, W), np.float32) for k in ("column 0", "column W-1", "third tile", "rows >= 256", "rows < 256")}
    m["column 0"][:, 0] = 1
    m["column W-1"][:, W - 1] = 1
    m["third tile"][:, 2 * LT_TILE:3 * LT_TILE] = 1
    m["rows >= 256"][LT_TILE:] = 1
    m["rows < 256"][:LT_TILE] = 1
    return m
