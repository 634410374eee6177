"""CPU tests of the environment-map rotation (reni_amd/rotation.py, reni_tu_rotate.hip: reni_rotate_envmap).

Holds the float64 oracle tests/test_gpu_rotate.py compares the HIP kernel against (np_rotate_envmap, written from the
definition in include/reni_hip.h, not from the kernel) and the per-pixel error bound derived from the kernel's operation chain
(rotate_bound).  Here: the oracle's own identities (rolls, flips, the model's equivariance through oracle.reni_oracle), the
rotation helpers on CPU tensors, the bound against an fp32 emulation of the chain, the unit's ISA audit and the C ABI's
argument checks."""
import ctypes
import math
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

from oracle import reni_oracle as O
from tests import isa_audit
from tests.util import load_golden, sd_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------ rotations of the tests
def Rx(t):
    return np.array([[1, 0, 0], [0, math.cos(t), -math.sin(t)], [0, math.sin(t), math.cos(t)]], np.float64)


def Ry(t):
    return np.array([[math.cos(t), 0, math.sin(t)], [0, 1, 0], [-math.sin(t), 0, math.cos(t)]], np.float64)


FLIP_Y, FLIP_Z, FLIP_X = np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0]), np.diag([1.0, -1.0, -1.0])


def rotation_list():
    """[(name, R float64)]: Ry(0.7) and R3 of golden G10, Rx(0.01), Rx(0.03), Rx(pi/2) and eight draws Q from
    numpy.random.default_rng(1): QR of a 3 x 3 standard normal, first column negated where det Q < 0."""
    g = load_golden("g10_equivariance.npz")
    out = [("Ry(0.7)", g["Ry"].astype(np.float64)), ("R3", g["R3"].astype(np.float64)),
           ("Rx(0.01)", Rx(0.01)), ("Rx(0.03)", Rx(0.03)), ("Rx(pi/2)", Rx(math.pi / 2))]
    rng = np.random.default_rng(1)
    for k in range(8):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append((f"Q{k}", q))
    return out


# ------------------------------------------------------------------------------------------ float64 oracle
def grid_directions(H, W):
    """d [H, W, 3] of the grid: phi = pi (r + 1/2) / H, theta = pi ((c + 1/2) / (W / 2) - 1)"""
    phi = (np.pi * (np.arange(H) + 0.5) / H)[:, None]
    theta = (np.pi * ((np.arange(W) + 0.5) / (W / 2) - 1.0))[None, :]
    return np.stack((np.sin(phi) * np.sin(theta), np.cos(phi) * np.ones_like(theta), -np.sin(phi) * np.cos(theta)), -1)


def source_coordinates(H, W, R):
    """(row, col, sin phi_s), each [H, W] float64: where output pixel (r, c) of rotate(img, R) looks in img"""
    s = grid_directions(H, W) @ np.asarray(R, np.float64)  # s = R^T d, as rows: d^T R
    rho = np.sqrt(s[..., 0] ** 2 + s[..., 2] ** 2)
    phis = np.arctan2(rho, s[..., 1])
    thetas = np.arctan2(s[..., 0], -s[..., 2])
    return phis / np.pi * H - 0.5, (thetas / np.pi + 1.0) * (W / 2) - 0.5, rho / np.sqrt(rho ** 2 + s[..., 1] ** 2)


def fetch(img, i, j):
    """img [..., H, W] at integer taps i, j [h, w] of the sphere: a row beyond a pole is the same row seen from the other side"""
    H, W = img.shape[-2:]
    i, j = np.array(i), np.array(j)
    k = np.mod(i, 2 * H)  # (rows repeat with period 2 H: at H = 1 a tap two rows beyond a pole is back on the near side)
    far = k >= H
    j = np.where(far, j + W // 2, j)
    i = np.where(far, 2 * H - 1 - k, k)
    return img[..., i, np.mod(j, W)]


def np_rotate_envmap(img, R, mode="bilinear"):
    """img [..., H, W] (float64 arithmetic) turned by R: out(d) = img(R^T d)."""
    img = np.asarray(img, np.float64)
    H, W = img.shape[-2:]
    assert W % 2 == 0
    row, col, _ = source_coordinates(H, W, R)
    if mode == "nearest":
        return fetch(img, np.floor(row + 0.5).astype(np.int64), np.floor(col + 0.5).astype(np.int64))
    assert mode == "bilinear"
    i, j = np.floor(row).astype(np.int64), np.floor(col).astype(np.int64)
    fr, fc = row - i, col - j
    return ((1 - fr) * ((1 - fc) * fetch(img, i, j) + fc * fetch(img, i, j + 1))
            + fr * ((1 - fc) * fetch(img, i + 1, j) + fc * fetch(img, i + 1, j + 1)))


# What the kernel's chain can lose (reni_tu_rotate.hip's header writes the chain out), in units of u = 2^-24, to first order:
#   tables      sin / cos of the output grid, float64 rounded to fp32: relative u each
#   d           d.x = fl(sp st), d.z = -fl(sp ct): two table roundings and a product, |delta d.x| <= 3 u |d.x|; d.y: u |d.y|.
#               |delta d| <= 3 u.
#   s = R^T d   R is the caller's fp32 matrix (the oracle is given the same numbers: no rounding of R).  The propagated part
#               has norm |R^T delta d| = |delta d| <= 3 u.  Each s_j is a product and two fma, three roundings of partial sums
#               bounded by sum_i |R_ij| |d_i|: the rounding part is <= 3 u (|R|^T |d|)_j, of norm <= 3 u || |R| ||_2 <= 3 sqrt(3) u
#               (|| |R| ||_2^2 <= || |R| ||_1 || |R| ||_inf <= sqrt(3) sqrt(3) for orthogonal R).
#               |delta s| <= (3 + 3 sqrt 3) u = 8.2 u with |s| = 1: an error of 8.2 u radians on the sphere, which is at most
#               8.2 u in phi_s and at most 8.2 u / sin phi_s in theta_s.
#   rho         fl(s.x s.x), fma, sqrtf: relative 2 u on the sum of squares, halved by the root, plus sqrtf's own error, 1 ulp
#               <= 2 u relative (the HIP math API's documented accuracy): 3 u relative, which moves atan2(rho, s.y) by
#               3 u sin phi_s cos phi_s <= 1.5 u.
#   atan2f      2 ulp (documented accuracy) of a result below 4: 2 x 2^-22 = 8 u, for phi_s and for theta_s.
#   row         fma(phi_s, fp32(H / pi), -1/2): the constant's rounding u H, the fma's u H (|row| < H).
#   col         fma(theta_s, fp32(W / 2 pi), W/2 - 1/2): the constant's rounding u W / 2, the fma's u W (|col| < W).
# delta_r = (8.2 + 1.5 + 8) u H / pi + 2 u H = A_ROW H u;  delta_c = ((8.2 / sin phi_s + 8) / 2 pi + 1.5) u W <= B_COL W u / sin phi_s.
# An fp32 emulation of the chain with numpy's functions needs a third of these constants and stays below 0.15 of the bound
# (test_bound_covers_an_fp32_emulation_of_the_chain); the device, below 0.2 (tests/test_gpu_rotate.py).  The
# worst case takes every rounding at its limit at once and sqrtf, atan2f at their documented 1 and 2 ulp.
S_ERR = 3.0 + 3.0 * math.sqrt(3.0)
A_ROW = (S_ERR + 1.5 + 8.0) / math.pi + 2.0  # 7.63
B_COL = (S_ERR + 8.0) / (2.0 * math.pi) + 1.5  # 4.08
# the value: gc = fl(1 - fc), gc t00, the fma with t01, gr = fl(1 - fr), gr top, the fma with bot: six roundings on the longest
# path of a tap (fr = row - floor(row) is exact); two more cover the second-order terms, as resample_bound counts them
K_SUM = 8.0
CAP = 0.999  # pixels with sin phi_s < CAP sin(pi / 2H) (inside the last half row around a pole) are left out: col is ill-conditioned


def rotate_bound(img, R):
    """(bound [..., H, W], keep [H, W] bool): per-pixel bound on |fp32 kernel - float64 oracle| for bilinear,
    delta_r Sr + delta_c Sc + K_SUM 2^-24 sum w_i |t_i|, with Sr, Sc the largest absolute difference between row- resp.
    column-neighbours among the 4 x 4 taps at offsets -1 .. +2 around the oracle's cell (bilinear is continuous: a
    coordinate error may step into the next cell but cannot jump).  keep: outside the polar caps."""
    img = np.asarray(img, np.float64)
    H, W = img.shape[-2:]
    row, col, sin_s = source_coordinates(H, W, R)
    keep = sin_s >= CAP * math.sin(math.pi / (2 * H))
    i, j = np.floor(row).astype(np.int64), np.floor(col).astype(np.int64)
    taps = [[fetch(img, i + a, j + b) for b in range(-1, 3)] for a in range(-1, 3)]
    Sr = np.max([np.abs(taps[a + 1][b] - taps[a][b]) for a in range(3) for b in range(4)], axis=0)
    Sc = np.max([np.abs(taps[a][b + 1] - taps[a][b]) for a in range(4) for b in range(3)], axis=0)
    fr, fc = row - i, col - j
    mag = ((1 - fr) * ((1 - fc) * np.abs(taps[1][1]) + fc * np.abs(taps[1][2]))
           + fr * ((1 - fc) * np.abs(taps[2][1]) + fc * np.abs(taps[2][2])))
    dr = A_ROW * H * EPS32
    dc = B_COL * W * EPS32 / np.maximum(sin_s, 1e-300)
    return dr * Sr + dc * Sc + K_SUM * EPS32 * mag, keep


def _fma32(a, b, c):  # one rounding
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def emulate_coordinates_fp32(H, W, R):
    """(row, col) [H, W] float32: the source coordinate as the kernel's chain computes it, with numpy's fp32 functions"""
    from reni_amd.rotation import grid_trig
    f = np.float32
    rt, ct = (t.astype(f) for t in grid_trig(H, W))
    R = np.asarray(R, f)
    sp, cp, st, cth = rt[:, 0][:, None], rt[:, 1][:, None], ct[:, 0][None, :], ct[:, 1][None, :]
    dx, dy, dz = sp * st, cp * np.ones_like(st), -(sp * cth)
    s = [_fma32(R[2, k], dz, _fma32(R[1, k], dy, R[0, k] * dx)) for k in range(3)]
    phi = np.arctan2(np.sqrt(_fma32(s[2], s[2], s[0] * s[0])), s[1])
    theta = np.arctan2(s[0], -s[2])
    assert phi.dtype == f and theta.dtype == f
    return _fma32(phi, f(H / np.pi), f(-0.5)), _fma32(theta, f(W / (2 * np.pi)), f(W / 2 - 0.5))


def emulate_kernel_fp32(img, R):
    """the kernel's chain with numpy's fp32 functions (each operation rounded to fp32; numpy's sqrt is correctly rounded and
    its arctan2 within an ulp or so): what the derivation of rotate_bound is checked against without a GPU"""
    f, fma = np.float32, _fma32
    img = np.asarray(img, f)
    H, W = img.shape[-2:]
    row, col = emulate_coordinates_fp32(H, W, R)
    fi, fj = np.floor(row), np.floor(col)
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    fr, fc = row - fi, col - fj
    gr, gc = f(1) - fr, f(1) - fc
    top = fma(fc, fetch(img, i, j + 1), gc * fetch(img, i, j))
    bot = fma(fc, fetch(img, i + 1, j + 1), gc * fetch(img, i + 1, j))
    return fma(fr, bot, gr * top)


def sky_maps(n, hs, ws, seed):
    """the maps of tests/test_gpu_resample.py::_maps: positive sky-like maps with a bright spot (five decades of range) and, in
    map 1, negatives"""
    g = np.random.default_rng(seed)
    x = 0.05 + g.random((n, 3, hs, ws))
    x[:, :, hs // 3, (2 * ws) // 3] = 2000.0
    if n > 1:
        x[1] -= 0.5
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------ 1. the oracle's identities
def test_oracle_grid_is_get_directions():
    for W in (32, 64):
        assert np.abs(grid_directions(W // 2, W).reshape(-1, 3) - O.get_directions(W)[0].double().numpy()).max() <= 1e-6


@pytest.mark.parametrize("mode,tol", [("bilinear", 1e-12), ("nearest", 0.0)])
def test_oracle_yaw_and_half_turns_are_rolls_and_flips(mode, tol):
    H, W = 32, 64
    img = np.random.default_rng(0).random((3, H, W))
    cases = [("identity", np.eye(3), img),
             ("180 about y", FLIP_Y, np.roll(img, W // 2, axis=-1)),
             ("180 about z", FLIP_Z, img[:, ::-1, ::-1]),
             ("180 about x", FLIP_X, np.roll(img[:, ::-1, ::-1], W // 2, axis=-1))]
    cases += [(f"Ry({k} 2 pi / W)", Ry(k * 2 * math.pi / W), np.roll(img, -k, axis=-1)) for k in (1, 3, -5, 17, 40)]
    for name, R, want in cases:
        err = float(np.abs(np_rotate_envmap(img, R, mode) - want).max())
        print(f"{mode} {name}: {err:.2e}")
        assert err <= tol, name


def test_oracle_turning_the_map_is_turning_the_latent():
    """G10's SO2 model at 32 x 64: f(Z R^T, D) against rotate(f(Z, D), R).  Ry(3 2 pi / 64) lands on pixel centres: the
    tolerance test_oracle_golden.py uses for this golden (5e-6, the fp32 oracle's own noise).  Ry(0.7) falls between pixels:
    what is left is bilinear's own error on that smooth map, a few 1e-6 (printed, held to the same 5e-6)."""
    from reni_amd.rotation import rotate_latent
    g = load_golden("g10_equivariance.npz")
    sd = sd_from(g, "sd_SO2.")
    spec = O.DecoderSpec(49, "SO2", 128, 5, 3, True, "tanh")
    Z = torch.from_numpy(g["Z_SO2"])
    D = O.get_directions(64)
    base = O.reni_forward(spec, sd, Z, D)[0].double().numpy().reshape(32, 64, 3).transpose(2, 0, 1)
    assert np.abs(g["Ry"] - Ry(0.7)).max() <= 1e-6
    for name, R in (("Ry(3 2 pi / 64)", Ry(3 * 2 * math.pi / 64)), ("Ry(0.7)", Ry(0.7))):
        Rt = torch.from_numpy(R).float()
        turned = O.reni_forward(spec, sd, rotate_latent(Z, Rt), D)[0].double().numpy().reshape(32, 64, 3).transpose(2, 0, 1)
        err = np.abs(np_rotate_envmap(base, R) - turned)
        print(f"{name}: max {err.max():.2e} rms {np.sqrt((err ** 2).mean()):.2e}")
        assert err.max() <= 5e-6
        # the other sign would be off by the map's own variation
        assert np.abs(np_rotate_envmap(base, R.T) - turned).max() > 1e-3


# ------------------------------------------------------------------------------------------ 2. rotation.py on CPU tensors
def test_random_rotations_are_rotations_and_reproducible():
    from reni_amd.rotation import random_rotations, rotation_y
    for group in ("SO2", "SO3"):
        R = random_rotations(64, group, torch.Generator().manual_seed(5))
        assert R.shape == (64, 3, 3) and R.dtype == torch.float32
        M = R.double()
        assert float((M @ M.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
        assert float((torch.linalg.det(M) - 1).abs().max()) <= 1e-6
        assert torch.equal(R, random_rotations(64, group, torch.Generator().manual_seed(5)))
        assert not torch.equal(R, random_rotations(64, group, torch.Generator().manual_seed(6)))
        assert not torch.equal(R[0], R[1])
        y = torch.tensor([0.0, 1.0, 0.0])
        if group == "SO2":
            assert torch.equal(R @ y, y.expand(64, 3)) and torch.equal(y @ R, y.expand(64, 3))
        else:
            assert float(((R @ y) - y).abs().max()) > 0.5
    assert np.abs(rotation_y(0.7).numpy() - Ry(0.7)).max() <= 1e-7
    assert rotation_y(torch.tensor([0.1, 0.2])).shape == (2, 3, 3)
    with pytest.raises(ValueError):
        random_rotations(4, "SO4")
    # SO3 is uniform: the mean of R over many draws vanishes (each entry has variance 1/3: 5 sigma of the mean of 4096)
    big = random_rotations(4096, "SO3", torch.Generator().manual_seed(0)).double().mean(0)
    assert float(big.abs().max()) <= 5 * math.sqrt(1 / 3 / 4096)


def test_rotate_latent_against_rotated_directions_on_the_golden_models():
    """f(Z R^T, D) = f(Z, D R): turning the latent by R is looking at the map from directions turned by R^T"""
    from reni_amd.rotation import rotate_latent
    g = load_golden("g10_equivariance.npz")
    D = O.get_directions(64)
    for eq, Rk in (("SO2", "Ry"), ("SO3", "R3")):
        sd = sd_from(g, f"sd_{eq}.")
        spec = O.DecoderSpec(49, eq, 128, 5, 3, True, "tanh")
        Z = torch.from_numpy(g[f"Z_{eq}"]); R = torch.from_numpy(g[Rk])
        a = O.reni_forward(spec, sd, rotate_latent(Z, R), D)
        b = O.reni_forward(spec, sd, Z, D @ R)
        assert float((a - b).abs().max()) < 5e-6
        assert torch.equal(rotate_latent(Z, R), Z @ R.T)
        per_row = rotate_latent(Z.repeat(2, 1, 1), torch.stack((R, torch.eye(3))))
        assert torch.equal(per_row[1], Z[0]) and torch.allclose(per_row[0], (Z @ R.T)[0], atol=1e-7)
    with pytest.raises(ValueError):
        rotate_latent(torch.zeros(2, 9, 3), torch.zeros(3, 3, 3))


def test_rotate_envmap_checks_the_matrix_before_it_needs_the_device():
    from reni_amd import _lib, rotation
    img = torch.ones(3, 8, 16)
    for bad in (torch.diag(torch.tensor([1.0, 1.0, -1.0])), torch.eye(3) * 1.01, torch.eye(3) + 1e-3 * torch.ones(3, 3),
                torch.eye(4), torch.full((3, 3), float("nan"))):
        with pytest.raises(ValueError):
            rotation.rotate_envmap(img, bad)
        with pytest.raises(ValueError):
            rotation.rotate_mask(torch.ones(1, 128, 3), bad)
    with pytest.raises(ValueError):
        rotation.rotate_mask(torch.ones(1, 100, 3), torch.eye(3))  # not H x 2H
    with pytest.raises(_lib.RENILibraryError):  # a good matrix gets as far as the op, which has no CPU fallback
        rotation.rotate_envmap(img, torch.from_numpy(Ry(0.3)).float())


# ------------------------------------------------------------------------------------------ the bound against an emulation
@pytest.mark.parametrize("size", [(16, 32), (64, 128)])
def test_bound_covers_an_fp32_emulation_of_the_chain(size):
    """not the device (its atan2f and sqrtf are other implementations), but every rounding the derivation counts is in it"""
    H, W = size
    x = sky_maps(2, H, W, H + W)
    worst = 0.0
    for name, R in rotation_list():
        R32 = R.astype(np.float32)
        for n in range(2):
            ref = np_rotate_envmap(x[n], R32)
            bound, keep = rotate_bound(x[n], R32)
            got = emulate_kernel_fp32(x[n], R32)
            ratio = float((np.abs(got - ref) / bound)[:, keep].max())
            left = int((~keep).sum())
            print(f"{H}x{W} {name} map {n}: largest err / bound {ratio:.3f}, left out {left} of {H * W}")
            assert ratio <= 1.0 and left <= 2 * W  # 2 / H of the map
            assert np.isfinite(got).all() and got.min() >= x[n].min() and got.max() <= x[n].max()
            worst = max(worst, ratio)
    print(f"{H}x{W}: worst {worst:.3f}")


# ------------------------------------------------------------------------------------------ 3. ISA audit
def test_rotate_translation_unit_isa_audit():
    """reni_tu_rotate.hip with build.sh's flags: both instances present, no hazard after its transcendentals, no scratch"""
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "rotate.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_rotate.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    assert len(set(re.findall(r"^(_Z\w*k_rotate_envmap\w*):", text, re.M))) == 2
    assert isa_audit.violations(text) == []
    assert isa_audit.valu_to_mfma(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) >= 2 and all(int(x) == 0 for x in sizes)
    assert "v_mul_f32" in text and "v_fma_f32" in text and "global_atomic" not in text


# ------------------------------------------------------------------------------------------ 4. C ABI, no CPU fallback, config
def test_c_abi_rejects_bad_arguments_before_any_device_work():
    from reni_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 255) & ~255
    st4 = (ctypes.c_int64 * 4)(96, 32, 8, 1)

    def rot(B=1, C=3, H=4, W=8, ptrs=(p,) * 5, strides=st4, index=None, n_src=1, rot_stride=9, mode=1):
        return lib.reni_rotate_envmap(B, C, H, W, ptrs[0], strides, index, n_src, ptrs[1], rot_stride, ptrs[2], ptrs[3], mode,
                                      ptrs[4], None)

    for kw in (dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(W=-2), dict(W=7), dict(B=1 << 16), dict(C=1 << 16),
               dict(H=1 << 15, W=1 << 15), dict(strides=None), dict(strides=(ctypes.c_int64 * 4)(96, 32, -8, 1)),
               dict(strides=(ctypes.c_int64 * 4)(96, 32, 1 << 31, 1)), dict(strides=(ctypes.c_int64 * 4)(96, 32, 8, 1 << 31)),
               dict(rot_stride=3), dict(rot_stride=-9), dict(rot_stride=12), dict(mode=2), dict(mode=-1),
               dict(index=p, n_src=0), dict(index=p, n_src=-3)):
        assert rot(**kw) == -1, kw
        assert lib.reni_last_error().startswith(b"rotate:")
    for k in range(5):
        ptrs = [p] * 5
        ptrs[k] = None
        assert rot(ptrs=ptrs) == -1 and b"NULL" in lib.reni_last_error()
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    defs = dict(re.findall(r"#define\s+(RENI_ROTATE_[A-Z]+)\s+(\d+)", header))
    assert {k: int(v) for k, v in defs.items()} == {"RENI_ROTATE_NEAREST": _lib.ROTATE_MODE["nearest"],
                                                    "RENI_ROTATE_BILINEAR": _lib.ROTATE_MODE["bilinear"]}


def _write_exr_pair(d):
    from reni_amd import exr
    d.mkdir(parents=True, exist_ok=True)
    exr.write_exr(str(d / "a.exr"), np.ones((8, 16, 3), np.float32) * 2, pixel_type="half", compression="zip")
    exr.write_exr(str(d / "b.exr"), np.ones((8, 16, 3), np.float32), pixel_type="half", compression="zip")


def test_rotation_has_no_cpu_fallback(tmp_path):
    from reni_amd import _lib, ops
    from reni_amd.custom_transforms import transform_builder
    from reni_amd.data import RENIDatasetHDR, ResidentDataset
    with pytest.raises(_lib.RENILibraryError):
        ops.rotate_envmap(torch.ones(3, 8, 16), torch.eye(3))
    with pytest.raises(_lib.RENILibraryError):
        ops.rotate_envmap(torch.ones(2, 3, 8, 16), torch.eye(3).expand(2, 3, 3), "nearest", index=torch.tensor([1, 0]))
    _write_exr_pair(tmp_path)
    ds = RENIDatasetHDR(str(tmp_path), transform_builder([["resize", [4, 8]], ["minmaxnormalise", []]]))
    with pytest.raises(_lib.RENILibraryError):
        ResidentDataset(ds, device="cpu", rotate="SO2")
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RENILibraryError):
            ResidentDataset(ds, rotate="SO3", rotate_seed=3)


def test_rotate_augment_needs_the_resident_dataset(tmp_path):
    from reni_amd.lightning_module import RENI
    from tests.test_gpu_workflows import _config
    _write_exr_pair(tmp_path / "Train")
    cfg = _config()
    cfg.DATASET = types.SimpleNamespace(NAME="RENI_HDR", ROTATE_AUGMENT="SO2", RENI_HDR=types.SimpleNamespace(
        PATH=str(tmp_path), TRANSFORMS=[["minmaxnormalise", [-1.0, 1.0]]], IS_HDR=True))
    with pytest.raises(ValueError, match="RESIDENT"):
        RENI(cfg, "FIT_DECODER").setup_dataset()
    cfg.DATASET.ROTATE_AUGMENT = None  # off: the plain host dataset, as before
    mod = RENI(cfg, "FIT_DECODER")
    mod.setup_dataset()
    assert len(mod.dataset) == 2 and not hasattr(mod.dataset, "batch")
    cfg.DATASET.ROTATE_AUGMENT = "SO3"  # only FIT_DECODER augments: the other tasks ignore the key
    mod = RENI(cfg, "FIT_LATENT")
    (tmp_path / "Test").mkdir()
    _write_exr_pair(tmp_path / "Test")
    mod.setup_dataset()
    assert len(mod.dataset) == 2
