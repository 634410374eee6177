"""CPU tests of diffuse irradiance (reni_amd.baselines' getDiffuseMap / shRender / shRenderL2 / windowing family,
reni_tu_diffuse.hip).

Holds the float64 numpy restatement of the reference's conventions (getDiffuseMap's grid, solid angles and clamped-cosine
sum; the Ramamoorthi-Hanrahan band factors and L2 closed form; the normal map; Sloan's windowing) that
tests/test_gpu_diffuse.py compares the HIP kernels against, and checks it against the golden made from the reference
(tests/golden/make_g24_diffuse.py)."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from reni_amd.baselines import diffuse_map_tables, reni_grid_weights
from tests import isa_audit
from tests.test_baselines_cpu import np_sh_basis, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G24 = os.path.join(ROOT, "tests", "golden", "g24_diffuse.npz")
DM_SHAPES = ((32, 16), (64, 32), (64, 16))
SR_LMAX = (0, 1, 2, 5)
SR_WIDTHS = (16, 32, 64)


# ------------------------------------------------------------------------------------------ numpy restatement
def np_dm_grid(W, wl):
    """getDiffuseMap's grid: (in_dirs [H W, 3], solid angle [H W], out_dirs [hl wl, 3]).  Directions at the pixel's
    top-left corner with v flipped: lat = pi (1 - y / H - 0.5), theta = 2 pi (1 - x / W), d = (cos lat sin theta, sin lat,
    cos lat cos theta); solid angle of the row centre; output pixel (x, y) looks along input (int(x / wl W), int(y / hl H))"""
    H, hl = W // 2, wl // 2
    lat = np.pi * ((1 - np.arange(H) / H) - 0.5)[:, None] * np.ones((1, W))
    th = 2 * np.pi * (1 - np.arange(W) / W)[None, :] * np.ones((H, 1))
    d = np.stack([np.cos(lat) * np.sin(th), np.sin(lat), np.cos(lat) * np.cos(th)], -1)
    sa = np.repeat(np_solid_angle_rows(W)[:, None], W, axis=1)
    xs = [int(x / wl * W) for x in range(wl)]
    ys = [int(y / hl * H) for y in range(hl)]
    return d.reshape(-1, 3), sa.reshape(-1), d[np.asarray(ys)[:, None], np.asarray(xs)[None, :]].reshape(-1, 3)


def np_solid_angle_rows(W):
    H = W // 2
    th = (1.0 - (np.arange(H) + 0.5) / H) * np.pi
    return 2 * np.pi / W * (np.cos(th - np.pi / H / 2) - np.cos(th + np.pi / H / 2))


def np_clamped_cosine(src, in_dirs, w, out_dirs):
    """E [N, P, 3] = sum_i max(0, out . in_i) w_i src[n, i, c] / pi, float64"""
    A = np.maximum(0.0, np.asarray(out_dirs, np.float64) @ np.asarray(in_dirs, np.float64).T) * np.asarray(w, np.float64)
    return np.einsum("pq,nqc->npc", A, np.asarray(src, np.float64)) / np.pi


def np_diffuse_map(img, W, wl):
    d, sa, od = np_dm_grid(W, wl)
    return np_clamped_cosine(img.reshape(1, -1, 3), d, sa, od)[0].reshape(wl // 2, wl, 3)


def np_diffuse_coeffs(lmax):
    """A_l / pi: 1, 2/3 (both even at lmax 0, as the reference), then for even l 2 (-1)^(l/2 - 1) / ((l + 2)(l - 1)) l! /
    (2^l ((l/2)!)^2), 0 for odd l"""
    out = [1.0, 2.0 / 3.0]
    for l in range(2, lmax + 1):
        out.append(0.0 if l % 2 else 2.0 * (-1) ** (l // 2 - 1) / ((l + 2) * (l - 1))
                   * math.factorial(l) / (2**l * math.factorial(l // 2) ** 2))
    return np.asarray(out)


def np_normal_map(W):
    """[H, W, 3]: (sin t cos(p + pi), sin t sin(p + pi), cos t), t = y pi / H, p = x 2 pi / W (the SH basis grid)"""
    H = W // 2
    t = (np.arange(H) * np.pi / H)[:, None] * np.ones((1, W))
    p = (np.arange(W) * 2 * np.pi / W)[None, :] * np.ones((H, 1)) + np.pi
    return np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], -1)


def np_sh_render_l2(L, n):
    """shRenderL2: C4 L0 + 2 C2 (L3 x + L1 y + L2 z) + C1 L8 (x^2 - y^2) + C3 L6 z^2 - C5 L6 + 2 C1 (L4 xy + L7 xz + L5 yz),
    / pi, with the reference's five-digit constants"""
    C1, C2, C3, C4, C5 = 0.429043, 0.511664, 0.743125, 0.886227, 0.247708
    x, y, z = (n[..., k:k + 1] for k in range(3))
    return (C4 * L[0] + 2 * C2 * (L[3] * x + L[1] * y + L[2] * z) + C1 * L[8] * (x * x - y * y) + C3 * L[6] * z * z
            - C5 * L[6] + 2 * C1 * (L[4] * x * y + L[7] * x * z + L[5] * y * z)) / np.pi


def np_sh_render(coeffs, W):
    lmax = int(round(math.sqrt(coeffs.shape[0]))) - 1
    band = np_diffuse_coeffs(lmax)[[int(math.sqrt(t)) for t in range(coeffs.shape[0])]]
    return np.einsum("yxt,tc->yxc", np_sh_basis(W, lmax), coeffs * band[:, None])


def np_window_factor(c, maxLaplacian=10.0):
    """Newton's method on target - sum_l L_l B_l / (1 + f L_l)^2, L_l = l^2 (l + 1)^2, B_l = sum_(m = -1..l) mean_c c[l, m]"""
    lmax = int(round(math.sqrt(c.shape[0]))) - 1
    Ls = np.asarray([float(l * l * (l + 1) * (l + 1)) for l in range(1, lmax + 1)])
    Bs = np.asarray([sum(c[l * l + l + m].mean() for m in range(-1, l + 1)) for l in range(1, lmax + 1)])
    if (Ls * Bs).sum() <= maxLaplacian**2:
        return 0.0
    f = 0.0
    for _ in range(10000):
        g = maxLaplacian**2 - (Ls * Bs / (1 + f * Ls) ** 2).sum()
        delta = -g / (2 * Ls * Ls * Bs / (1 + f * Ls) ** 3).sum()
        f += delta
        if abs(delta) < 1e-7:
            break
    return f


def np_apply_window(c, f):
    if f <= 0:
        return c.copy()
    ls = np.sqrt(np.arange(c.shape[0])).astype(int)
    return c / (1 + f * (ls * ls * (ls + 1.0) * (ls + 1.0)))[:, None]


# ------------------------------------------------------------------------------------------ restatement vs golden
@pytest.mark.parametrize("W,wl", DM_SHAPES)
def test_diffuse_map_restatement_reproduces_the_reference(W, wl):
    g = np.load(G24)
    for i, img in enumerate(g[f"dm_w{W}_imgs"]):
        ref = g[f"dm_w{W}_l{wl}"][i]
        r = np_diffuse_map(img, W, wl)
        assert rel(r, ref) < 2e-7, (W, wl, i)  # the reference's result is float32 of its float64 sum
    assert np.allclose(np_dm_grid(W, wl)[1].reshape(W // 2, W), g[f"sa_w{W}"], rtol=1e-14, atol=0)


def test_sh_irradiance_restatement_reproduces_the_reference():
    g = np.load(G24)
    for lmax in range(16):
        assert np.allclose(np_diffuse_coeffs(lmax), g[f"dc_l{lmax}"], rtol=1e-14, atol=1e-16), lmax
    for lmax in SR_LMAX:
        for W in SR_WIDTHS:
            assert rel(np_sh_render(g[f"sr_l{lmax}_coeffs"], W), g[f"sr_l{lmax}_w{W}"]) < 1e-12, (lmax, W)
    c9 = g["sr_l2_coeffs"]
    for W in SR_WIDTHS:
        assert np.abs(np_normal_map(W) - g[f"nm_w{W}"]).max() < 1e-14
        assert rel(np_sh_render_l2(c9, np_normal_map(W)), g[f"srd_w{W}"]) < 2e-7
    assert rel(np_sh_render_l2(c9, g["srn_normals"]), g["srn_out"]) < 2e-7


def test_windowing_restatement_reproduces_the_reference():
    g = np.load(G24)
    assert float(g["win0_factor"]) == 0.0
    assert float(g["win1_factor"]) > 0 and float(g["win2_factor"]) > 0
    for k in range(3):
        c = g[f"win{k}_coeffs"]
        f = np_window_factor(c)
        assert abs(f - float(g[f"win{k}_factor"])) <= 1e-6 * max(abs(f), 1e-3), k
        for key in ("applied", "applied_auto"):
            assert np.allclose(np_apply_window(c, float(g[f"win{k}_factor"])), g[f"win{k}_{key}"], rtol=1e-13, atol=0)


def test_reni_grid_constant_map_convention():
    """On RENI's own grid (pixel-centre directions, exact band solid angles) a constant map of 1 has irradiance 1 up to
    the grid's quadrature error: 1.78e-3 at W = 32, 4.7e-4 at W = 64 (float64)."""
    from reni_amd import baselines
    from reni_amd.utils import get_directions
    for W, dev in ((32, 1.78e-3), (64, 4.7e-4)):
        w = reni_grid_weights(W)
        assert abs(w.sum() - 4 * np.pi) < 1e-12
        d = get_directions(W)[0].double().numpy()
        E = np_clamped_cosine(np.ones((1, d.shape[0], 3)), d, w, d)
        assert abs(np.abs(E - 1).max() - dev) < 0.01 * dev, W


# ------------------------------------------------------------------------------------------ library host side
def test_library_host_tables_match_the_restatement():
    from reni_amd import baselines
    g = np.load(G24)
    for W, wl in DM_SHAPES + ((600, 32),):
        d, sa, od = diffuse_map_tables(W, wl)
        rd, rsa, rod = np_dm_grid(W, wl)
        assert np.abs(d - rd).max() < 1e-14 and np.abs(od - rod).max() < 1e-14, (W, wl)
        assert np.allclose(sa, rsa, rtol=1e-14, atol=0)
    for W in (32, 64):
        assert np.array_equal(baselines.getSolidAngleMap(W), g[f"sa_w{W}"])
    for lmax in range(16):
        assert np.array_equal(baselines.getDiffuseCoefficients(lmax), g[f"dc_l{lmax}"]), lmax
    for W in SR_WIDTHS:
        assert np.array_equal(baselines.getNormalMap(W), g[f"nm_w{W}"])
    for k in range(3):
        c = g[f"win{k}_coeffs"]
        f = baselines.findWindowingFactor(c.copy())
        assert f == float(g[f"win{k}_factor"]), k
        assert np.array_equal(baselines.applyWindowing(c.copy(), f), g[f"win{k}_applied"])
        assert np.array_equal(baselines.applyWindowing(c.copy()), g[f"win{k}_applied_auto"])
    assert [baselines.l_from_idx(i) for i in range(10)] == [0, 1, 1, 1, 2, 2, 2, 2, 2, 3]
    assert np.array_equal(baselines.getSolidAngle(np.arange(8), 16), np_solid_angle_rows(16))


def test_diffuse_wrappers_refuse_what_needs_cv2():
    from reni_amd import baselines
    img = np.ones((8, 16, 3), np.float32)
    with pytest.raises(NotImplementedError, match="cv2"):
        baselines.getDiffuseMap(img, width=32, widthLowRes=16, outputWidth=16)  # would resize the map
    with pytest.raises(NotImplementedError, match="cv2"):
        baselines.getDiffuseMap(img, width=16, widthLowRes=8)  # would upsample the result to outputWidth = 16
    with pytest.raises(NotImplementedError, match="cv2"):
        baselines.getDiffuseMap(img, width=16, widthLowRes=8, outputWidth=12)


def test_diffuse_ops_have_no_cpu_fallback():
    from reni_amd import _lib, baselines, ops
    src, d, w = torch.ones(2, 10, 3), torch.zeros(10, 3), torch.ones(10)
    with pytest.raises(_lib.RENILibraryError):
        ops.diffuse_convolve(src, d, w, d, 1.0)
    with pytest.raises(_lib.RENILibraryError):
        baselines.diffuse_convolve(src, d, w, d)
    with pytest.raises(_lib.RENILibraryError):
        ops.sh_irradiance_l2(torch.ones(2, 9, 3), torch.zeros(5, 3))
    with pytest.raises(_lib.RENILibraryError):
        baselines.irradiance_map(torch.ones(2, 8 * 16, 3))
    with pytest.raises(_lib.RENILibraryError):
        baselines.sh_irradiance(torch.ones(2, 9, 3), 16)


# ------------------------------------------------------------------------------------------ ISA audit, C ABI checks
def test_diffuse_translation_unit_isa_audit():
    """reni_tu_diffuse.hip with build.sh's flags: no MFMA / transcendental / SDWA hazard, no scratch, the MFMA in the
    convolution kernel."""
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "diffuse.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_diffuse.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    for k in ("k_diffuse_convolve", "k_diffuse_reduce", "k_sh_irradiance_l2"):
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.valu_to_mfma(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert sizes and all(int(x) == 0 for x in sizes)
    mf = isa_audit.mfma_functions(text)
    assert any("k_diffuse_convolve" in f for f in mf)


def test_c_abi_rejects_bad_shapes_and_null_pointers():
    """Argument checks run before any device work, so they hold without a GPU."""
    from reni_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def conv(N, P, Q, ptrs=(p,) * 5, strides=(30, 3, 1), ws=p, wsb=4096):
        return lib.reni_diffuse_convolve(N, P, Q, ptrs[0], ptrs[1], ptrs[2], ptrs[3], *strides, 1.0, ptrs[4], ws, wsb, None)

    for N, P, Q in ((0, 4, 10), (1, 0, 10), (1, 4, 0), (-1, 4, 10), (1, 1 << 29, 10), (1, 4, 1 << 29), (1 << 22, 1 << 8, 10)):
        assert conv(N, P, Q) == -1, (N, P, Q)
        assert lib.reni_diffuse_workspace_bytes(N, P, Q) == 0
    for k in range(5):
        ptrs = [p] * 5
        ptrs[k] = None
        assert conv(1, 4, 10, ptrs=ptrs) == -1 and b"NULL" in lib.reni_last_error()
    for st in ((-1, 3, 1), (30, -3, 1), (30, 3, -1)):
        assert conv(1, 4, 10, strides=st) == -1
    # a split i range needs the workspace: P = 512, Q = 180 000 (one 600-wide map to 32 x 16) splits
    need = lib.reni_diffuse_workspace_bytes(1, 512, 180000)
    assert need > 0 and lib.reni_diffuse_workspace_bytes(3, 512, 180000) > need
    assert conv(1, 512, 180000, ws=None, wsb=0) == -2
    assert conv(1, 512, 180000, ws=p + 4, wsb=need) == -2
    assert lib.reni_diffuse_workspace_bytes(64, 32768, 1000) == 0  # a short i range is never split
    sh = lib.reni_sh_irradiance_l2
    for N, P, st in ((0, 8, 0), (1, 0, 0), (2, 8, 3), (2, 8, 25), (1, 1 << 29, 0)):
        assert sh(N, P, p, p, st, p, None) == -1, (N, P, st)
    for k in range(3):
        ptrs = [p] * 3
        ptrs[k] = None
        assert sh(2, 8, ptrs[0], ptrs[1], 24, ptrs[2], None) == -1 and b"NULL" in lib.reni_last_error()
