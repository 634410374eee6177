"""CPU tests of glossy lighting (reni_amd.glossy, reni_tu_glossy.hip).

Holds the float64 numpy restatement of the lobe convolution and of the lookup, written from include/reni_hip.h's definitions,
that tests/test_gpu_glossy.py compares the HIP kernels against; the Funk-Hecke check of that restatement and of
``lobe_band_scale``; the tolerance rule; and what can be checked of the library without a GPU."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from reni_amd import _lib, glossy
from reni_amd.baselines import getDiffuseCoefficients, reni_grid_weights
from reni_amd.utils import get_directions
from tests import isa_audit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ numpy restatement
def np_lobe(lobe, t):
    """f(t), float64, from the header: tc = clamp(t, 0, 1), m = clamp((1 + t) / 2, 0, 1); PHONG tc^n, BLINN m^(s / 2),
    GGX tc a^2 / (m (a^2 - 1) + 1)^2"""
    kind, p = lobe
    t = np.asarray(t, np.float64)
    tc = np.minimum(np.maximum(t, 0.0), 1.0)
    m = np.minimum(np.maximum((1.0 + t) / 2.0, 0.0), 1.0)
    if kind == "phong":
        return np.power(tc, p)
    if kind == "blinn":
        return np.power(m, p / 2.0)
    assert kind == "ggx"
    return tc * (p * p) / np.square(m * (p * p - 1.0) + 1.0)


def np_lobe_convolve(src, in_dirs, w, out_dirs, lobes, normalise=True, scale=1.0):
    """[N, Lv, P, 3] float64: num = sum_i f_l(o . d_i) w_i src[n, i, c], den = sum_i f_l w_i; num / den where den > 0 (else
    0) when normalise, else scale num.  The inputs are taken as they are (fp32 values in float64)."""
    src, w = np.asarray(src, np.float64), np.asarray(w, np.float64)
    t = np.asarray(out_dirs, np.float64) @ np.asarray(in_dirs, np.float64).T
    out = []
    for lobe in lobes:
        A = np_lobe(lobe, t) * w
        num = np.einsum("pq,nqc->npc", A, src)
        if normalise:
            den = A.sum(1)[None, :, None]
            num = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
        else:
            num = num * scale
        out.append(num)
    return np.stack(out, 1)


def lobe_sensitivity(lobe):
    """S of the issue's table: |d ln f / dt| at the lobe's peak t = 1"""
    kind, p = lobe
    return {"phong": p, "blinn": p / 4.0, "ggx": 1.0 / (p * p)}[kind]


def lobe_tol(lobe):
    """fp32 kernel against the float64 sums of the same fp32 inputs, relative to max |reference| of the lobe's output:
    1e-5 (tests/test_gpu_diffuse.py's figure for this accumulation) + S 2^-22 (the lobe's log-sensitivity at its peak times
    the rounding of the three-term fp32 dot product)"""
    return 1e-5 + lobe_sensitivity(lobe) * 2.0 ** -22


# ------------------------------------------------------------------------------------------ lookup: oracle and bound
LERP_U = 4.0  # the level mix is one more lerp: gl = fl(1 - fl), gl v0, the fma with v1 -- three roundings, one for second order


def lookup_coordinates(H, W, dirs):
    """(row, col, sin phi_s) float64 [P] of directions [P, 3] (any length): the header's chain, phi = atan2(sqrt(x^2 + z^2), y),
    theta = atan2(x, -z), row = phi / pi H - 1/2, col = (theta / pi + 1) W / 2 - 1/2.  The zero vector has sin phi_s = 0."""
    s = np.asarray(dirs, np.float64)
    rho = np.sqrt(s[:, 0] ** 2 + s[:, 2] ** 2)
    phis = np.arctan2(rho, s[:, 1])
    thetas = np.arctan2(s[:, 0], -s[:, 2])
    nrm = np.sqrt(rho ** 2 + s[:, 1] ** 2)
    return phis / np.pi * H - 0.5, (thetas / np.pi + 1.0) * (W / 2) - 0.5, np.where(nrm > 0, rho / np.where(nrm > 0, nrm, 1.0), 0.0)


def np_lookup(img, dirs):
    """img [..., H, W] (float64 arithmetic) sampled bilinearly on the sphere at dirs [P, 3] -> (value [..., P], bound [..., P],
    keep [P]).  The bound is tests/test_rotate_cpu.py::rotate_bound for arbitrary directions: its coordinate error constants
    A_ROW, B_COL (they allow 8.2 u for the error of s, which a caller's direction does not have: kept), the largest
    row / column neighbour differences among the 4 x 4 taps around the cell, its K_SUM for the value and its CAP rule for
    keep (outside the polar caps, where col is ill-conditioned)."""
    from tests.test_rotate_cpu import A_ROW, B_COL, CAP, EPS32, K_SUM, fetch
    img = np.asarray(img, np.float64)
    H, W = img.shape[-2:]
    row, col, sin_s = lookup_coordinates(H, W, dirs)
    keep = sin_s >= CAP * math.sin(math.pi / (2 * H))
    i, j = np.floor(row).astype(np.int64), np.floor(col).astype(np.int64)
    taps = [[fetch(img, i + a, j + b) for b in range(-1, 3)] for a in range(-1, 3)]
    fr, fc = row - i, col - j
    val = ((1 - fr) * ((1 - fc) * taps[1][1] + fc * taps[1][2]) + fr * ((1 - fc) * taps[2][1] + fc * taps[2][2]))
    Sr = np.max([np.abs(taps[a + 1][b] - taps[a][b]) for a in range(3) for b in range(4)], axis=0)
    Sc = np.max([np.abs(taps[a][b + 1] - taps[a][b]) for a in range(4) for b in range(3)], axis=0)
    mag = ((1 - fr) * ((1 - fc) * np.abs(taps[1][1]) + fc * np.abs(taps[1][2]))
           + fr * ((1 - fc) * np.abs(taps[2][1]) + fc * np.abs(taps[2][2])))
    dr = A_ROW * H * EPS32
    dc = B_COL * W * EPS32 / np.maximum(sin_s, 1e-300)
    return val, dr * Sr + dc * Sc + K_SUM * EPS32 * mag, keep


def np_lookup_chain(chain, dirs, level):
    """chain [Lv, H, W, 3], dirs [P, 3], level [P] (fp32 values) -> (value [P, 3], bound [P, 3], keep [P]): the level clamped
    to [0, Lv - 1], floor(level) and the next level mixed linearly; the bound mixes the levels' bounds and adds the lerp's
    rounding LERP_U u (gl |v0| + fl |v1|)."""
    from tests.test_rotate_cpu import EPS32
    chain = np.asarray(chain, np.float64)
    Lv = chain.shape[0]
    val, bnd, keep = np_lookup(chain.transpose(0, 3, 1, 2), dirs)  # [Lv, 3, P]
    lv = np.clip(np.asarray(level, np.float64), 0.0, Lv - 1.0)
    l0 = np.floor(lv).astype(np.int64)
    l1 = np.minimum(l0 + 1, Lv - 1)
    fl = lv - l0
    p = np.arange(len(lv))
    v0, v1, b0, b1 = val[l0, :, p], val[l1, :, p], bnd[l0, :, p], bnd[l1, :, p]  # [P, 3]
    fl = fl[:, None]
    out = (1 - fl) * v0 + fl * v1
    bound = (1 - fl) * b0 + fl * b1 + np.where(fl > 0, LERP_U * EPS32 * ((1 - fl) * np.abs(v0) + fl * np.abs(v1)), 0.0)
    return out, bound, keep


def emulate_lookup_fp32(chain, dirs, level):
    """the kernel's chain with numpy's fp32 functions, each operation rounded once (as tests/test_rotate_cpu.py does for the
    rotation): what the bound is checked against without a GPU"""
    from tests.test_rotate_cpu import fetch
    f = np.float32
    chain = np.asarray(chain, f)
    Lv, H, W, _ = chain.shape
    s = np.asarray(dirs, f)

    def fma(a, b, c):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f)

    phi = np.arctan2(np.sqrt(fma(s[:, 2], s[:, 2], s[:, 0] * s[:, 0])), s[:, 1])
    theta = np.arctan2(s[:, 0], -s[:, 2])
    row = np.minimum(np.maximum(fma(phi, f(H / np.pi), f(-0.5)), f(-1)), f(H))
    col = np.minimum(np.maximum(fma(theta, f(W / (2 * np.pi)), f(W / 2 - 0.5)), f(-1)), f(W))
    fi, fj = np.floor(row), np.floor(col)
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    fr, fc = row - fi, col - fj
    gr, gc = f(1) - fr, f(1) - fc
    img = chain.transpose(0, 3, 1, 2)
    top = fma(fc, fetch(img, i, j + 1), gc * fetch(img, i, j))
    bot = fma(fc, fetch(img, i + 1, j + 1), gc * fetch(img, i + 1, j))
    v = fma(fr, bot, gr * top)  # [Lv, 3, P]
    lv = np.minimum(np.maximum(np.asarray(level, f), f(0)), f(Lv - 1))
    l0 = np.floor(lv).astype(np.int64)
    l1 = np.minimum(l0 + 1, Lv - 1)
    fl = (lv - np.floor(lv)).astype(f)
    p = np.arange(len(lv))
    v0, v1 = v[l0, :, p], v[l1, :, p]
    return np.where(fl[:, None] > 0, fma(fl[:, None], v1, (f(1) - fl)[:, None] * v0), v0)


def random_dirs(n, seed):
    """n uniform random directions scaled by random lengths in [0.1, 10), fp32"""
    g = np.random.default_rng(seed)
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * np.exp(g.uniform(np.log(0.1), np.log(10.0), (n, 1)))).astype(np.float32)


@pytest.mark.parametrize("H,W", [(8, 16), (16, 32)])
def test_lookup_bound_covers_an_fp32_emulation_of_the_chain(H, W):
    g = np.random.default_rng(H)
    chain = g.random((3, H, W, 3)).astype(np.float32)
    dirs = random_dirs(4096, 7 + H)
    level = g.uniform(-0.5, 2.5, 4096).astype(np.float32)
    val, bound, keep = np_lookup_chain(chain, dirs, level)
    assert (~keep).mean() <= 0.03
    err = np.abs(emulate_lookup_fp32(chain, dirs, level).astype(np.float64) - val)
    ratio = (err / bound)[keep].max()
    print(f"lookup emulation {H} x {W}: largest error / bound {ratio:.3f}")
    assert ratio <= 1.0
    # pixel centres reproduce the map
    cd = get_directions(W)[0].numpy()
    for l in range(3):
        v, b, k = np_lookup_chain(chain, cd, np.full(len(cd), float(l), np.float32))
        assert k.all() and (np.abs(v - chain[l].reshape(-1, 3)) <= b).all()


# ------------------------------------------------------------------------------------------ Funk-Hecke
FH_C = (1.0, 0.7, -0.5, 0.4)
FH_AXES = np.asarray([[0.0, 1.0, 0.0], [0.6, 0.0, 0.8], [-0.48, 0.64, 0.6], [2.0 / 7.0, -3.0 / 7.0, 6.0 / 7.0]])
FH_LOBES = (glossy.phong(1), glossy.phong(8), glossy.phong(64), glossy.ggx(0.5))  # ggx: alpha = 0.25


def _legendre(l, x):
    return np.polynomial.legendre.legval(x, [0.0] * l + [1.0])


def fh_field(dirs, band_scale=None):
    """L(d) = sum_(l <= 3) c_l Lambda_l P_l(d . a_l) (Lambda = 1: the field itself) as grey [P, 3]"""
    d = np.asarray(dirs, np.float64)
    v = sum(FH_C[l] * (1.0 if band_scale is None else band_scale[l]) * _legendre(l, d @ FH_AXES[l]) for l in range(4))
    return np.repeat(v[:, None], 3, 1)


def fh_case(W, Wo=16, lobes=FH_LOBES):
    """(restated prefilter [Lv, P, 3] of the field on RENI's W grid at the Wo x Wo / 2 grid, analytic [Lv, P, 3]), float64.
    The field is rounded to fp32 first, as the device sees it."""
    d = get_directions(W)[0].numpy()
    od = get_directions(Wo)[0].numpy()
    src = fh_field(d).astype(np.float32)[None]
    ref = np_lobe_convolve(src, d, reni_grid_weights(W).astype(np.float32), od, [tuple(l) for l in lobes])[0]
    ana = np.stack([fh_field(od, glossy.lobe_band_scale(l, 3)) for l in lobes])
    return ref, ana


def test_axes_are_unit():
    assert np.allclose(np.linalg.norm(FH_AXES, axis=1), 1.0, atol=1e-15)


def test_funk_hecke_restatement_converges_at_second_order():
    """The normalised prefilter of a band-limited field on RENI's grid approaches sum c_l Lambda_l P_l(o . a_l): every
    doubling of W cuts the largest error at least 3x (second order is 4x)."""
    err = {}
    for W in (32, 64, 128):
        ref, ana = fh_case(W)
        err[W] = np.abs(ref - ana).reshape(len(FH_LOBES), -1).max(1)
    for k, lobe in enumerate(FH_LOBES):
        assert err[32][k] >= 3 * err[64][k] and err[64][k] >= 3 * err[128][k], (lobe, err[32][k], err[64][k], err[128][k])


def test_band_scales():
    dc = getDiffuseCoefficients(9)
    assert np.abs(glossy.lobe_band_scale(glossy.phong(1), 9) - dc).max() < 1e-10
    assert np.abs(glossy.lobe_band_scale(glossy.ggx(1.0), 9) - dc).max() < 1e-10
    for lobe in (glossy.phong(8), glossy.phong(4096), glossy.blinn(20), glossy.blinn(500), glossy.ggx(0.5), glossy.ggx(0.1)):
        lam = glossy.lobe_band_scale(lobe, 6)
        assert abs(lam[0] - 1.0) < 1e-13, lobe
        assert np.all(np.abs(lam) <= 1.0 + 1e-13), lobe
    # phong(n), band 1 in closed form: int_0^1 t^(n + 1) / int_0^1 t^n = (n + 1) / (n + 2)
    for n in (1.0, 8.0, 64.0, 500.0):
        assert abs(glossy.lobe_band_scale(glossy.phong(n), 1)[1] - (n + 1) / (n + 2)) < 1e-12, n
    # a sharp lobe leaves the low bands alone
    assert np.all(glossy.lobe_band_scale(glossy.phong(4096), 3) > 0.998)


def test_lobe_constructors_and_definitions():
    assert glossy.ggx(0.5) == glossy.Lobe("ggx", 0.25)
    for bad in (lambda: glossy.phong(0), lambda: glossy.blinn(-1), lambda: glossy.ggx(0), lambda: glossy.ggx(1.5)):
        with pytest.raises(ValueError):
            bad()
    t = np.linspace(-1, 1, 201)
    for lobe in (glossy.phong(3), glossy.blinn(20), glossy.ggx(0.7)):
        assert np.abs(glossy.lobe_value(lobe, t) - np_lobe(tuple(lobe), t)).max() < 1e-15
    # PHONG(1) and GGX(1) are the clamped cosine; BLINN(s) is (n . h)^s of the shader with view = normal
    assert np.array_equal(np_lobe(("phong", 1.0), t), np.maximum(t, 0))
    assert np.abs(np_lobe(("ggx", 1.0), t) - np.maximum(t, 0)).max() == 0
    ang = np.arccos(t)
    n, l = np.asarray([0.0, 0.0, 1.0]), np.stack([np.sin(ang), 0 * ang, np.cos(ang)], -1)
    h = (n + l) / np.maximum(np.linalg.norm(n + l, axis=-1, keepdims=True), 1e-6)
    for s in (20.0, 500.0):
        assert np.abs(np.clip(h @ n, 0, 1) ** s - np_lobe(("blinn", s), t)).max() < 1e-12, s
    assert abs(glossy.blinn_phong_norm(500.0) - 502.0 / 8.0) < 1e-12


def test_tolerance_rule():
    assert lobe_tol(("phong", 1.0)) == 1e-5 + 2.0 ** -22
    assert lobe_tol(("blinn", 500.0)) == 1e-5 + 125 * 2.0 ** -22
    assert lobe_tol(("ggx", 0.0625)) == 1e-5 + 256 * 2.0 ** -22  # S = 1 / alpha^2


def test_glossy_ops_have_no_cpu_fallback():
    from reni_amd import ops
    from reni_amd.envmap_shader import EnvironmentMap
    src, d, w = torch.ones(2, 10, 3), torch.zeros(10, 3), torch.ones(10)
    L = [glossy.phong(2)]
    with pytest.raises(_lib.RENILibraryError):
        ops.lobe_convolve(src, d, w, d, ["phong"], [2.0])
    with pytest.raises(_lib.RENILibraryError):
        glossy.lobe_convolve(src, d, w, d, L)
    with pytest.raises(_lib.RENILibraryError):
        glossy.prefilter(torch.ones(2, 8 * 16, 3), L)
    with pytest.raises(_lib.RENILibraryError):
        ops.envmap_lookup(torch.ones(2, 8, 16, 3), d)
    with pytest.raises(_lib.RENILibraryError):
        glossy.lookup(torch.ones(2, 3, 8, 16, 3), d, 1.0)
    with pytest.raises(_lib.RENILibraryError):
        glossy.sh_glossy(torch.ones(2, 16, 3), glossy.phong(8), 16)
    env = EnvironmentMap(torch.ones(1, 8 * 16, 3), get_directions(16), torch.ones(1, 8 * 16, 3))
    with pytest.raises(_lib.RENILibraryError):
        glossy.shade_prefiltered(env, torch.ones(5, 3), torch.zeros(5, 3), (0.0, 0.0, 2.0), 20.0, 0.5, 0.5, 16)


# ------------------------------------------------------------------------------------------ ISA audit, C ABI checks
def test_glossy_translation_unit_isa_audit():
    """reni_tu_glossy.hip with build.sh's flags: no MFMA / transcendental / SDWA hazard (the lobes' v_log / v_exp / v_rcp sit
    directly in front of the multiply that feeds the MFMA), no scratch, every kernel present, the MFMA in the convolution."""
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "glossy.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_glossy.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    for k in ("k_lobe_convolve", "k_lobe_finish", "k_envmap_lookup"):
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.valu_to_mfma(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert sizes and all(int(x) == 0 for x in sizes)
    mf = isa_audit.mfma_functions(text)
    assert mf and all("k_lobe_convolve" in f for f in mf)
    assert len(mf) == 6  # three kinds x one or two column tiles
    # the generators are there: two transcendentals per A value for PHONG / BLINN, a reciprocal for GGX
    assert "v_log_f32" in text and "v_exp_f32" in text and "v_rcp_f32" in text


def test_header_build_and_binding_name_the_unit():
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    for name in ("reni_lobe_workspace_bytes", "reni_lobe_convolve", "reni_envmap_lookup"):
        assert re.search(r"^(int|size_t) " + name + r"\(", header, re.M) and name in _lib.EXPORTS
    build = open(os.path.join(ROOT, "reni_amd", "csrc", "build.sh")).read()
    assert re.search(r"for tu in [^;]*\bglossy\b", build) and "_build/glossy.o" in build
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(RENI_LOBE_[A-Z]+)\s+(\d+)\b", header)}
    assert {k[len("RENI_LOBE_"):].lower(): v for k, v in defs.items()} == _lib.LOBE_KIND


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    """Argument checks run before any device work, so they hold without a GPU."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    wsb = lib.reni_lobe_workspace_bytes

    def conv(N=1, P=4, Q=10, ptrs=(p,) * 5, strides=(30, 3, 1), kinds=(0,), params=(2.0,), n_lobes=None, ws=p, wsn=1 << 15,
             normalise=1):
        ck = (ctypes.c_int32 * max(len(kinds), 1))(*kinds) if kinds is not None else None
        cp = (ctypes.c_float * max(len(params), 1))(*params) if params is not None else None
        nl = len(kinds) if n_lobes is None else n_lobes
        return lib.reni_lobe_convolve(N, P, Q, ptrs[0], ptrs[1], ptrs[2], ptrs[3], *strides, nl, ck, cp, normalise, 1.0, ptrs[4],
                                      ws, wsn, None)

    for N, P, Q in ((0, 4, 10), (1, 0, 10), (1, 4, 0), (-1, 4, 10), (1, 1 << 29, 10), (1, 4, 1 << 29), (1 << 22, 1 << 8, 10)):
        assert conv(N, P, Q) == -1, (N, P, Q)
        assert wsb(N, P, Q, 1) == 0
    assert wsb(1 << 18, 1 << 8, 10, 1) > 0  # n_lobes (3 N + 1) P < 2^30 with one lobe, not with 16
    assert conv(1 << 18, 1 << 8, 10, kinds=(0,) * 16, params=(2.0,) * 16) == -1 and wsb(1 << 18, 1 << 8, 10, 16) == 0
    for nl in (0, 17, -1):
        assert conv(kinds=(0,) * 17, params=(2.0,) * 17, n_lobes=nl) == -1 and b"n_lobes" in lib.reni_last_error(), nl
        assert wsb(1, 4, 10, nl) == 0
    for kind in (3, -1, 100):
        assert conv(kinds=(0, kind), params=(2.0, 2.0)) == -1 and b"kind" in lib.reni_last_error(), kind
    for kind, par in ((0, 0.0), (0, -1.0), (0, float("nan")), (0, float("inf")), (1, 0.0), (1, -20.0), (2, 0.0), (2, -0.5),
                      (2, 1.0001), (2, 2.0), (2, float("nan"))):
        assert conv(kinds=(1, kind), params=(20.0, par)) == -1, (kind, par)
        assert b"parameter" in lib.reni_last_error() or b"alpha" in lib.reni_last_error()
    for k in range(5):
        ptrs = [p] * 5
        ptrs[k] = None
        assert conv(ptrs=ptrs) == -1 and b"NULL" in lib.reni_last_error(), k
    assert conv(kinds=None, n_lobes=1) == -1 and b"NULL" in lib.reni_last_error()
    assert conv(params=None, n_lobes=1) == -1 and b"NULL" in lib.reni_last_error()
    for st in ((-1, 3, 1), (30, -3, 1), (30, 3, -1)):
        assert conv(strides=st) == -1 and b"strides" in lib.reni_last_error()
    # the workspace is always needed (the partial sums and the division's operands); it grows with maps, lobes and the split
    need = wsb(1, 4, 10, 1)
    assert need >= 4 * 4 * 4 and wsb(2, 4, 10, 1) > need and wsb(1, 4, 10, 3) > need
    assert wsb(1, 512, 180000, 1) > 8 * wsb(1, 512, 1000, 1)  # P = 512, Q = 180 000 splits the i range
    for normalise in (0, 1):
        assert conv(ws=None, wsn=0, normalise=normalise) == -2
        assert conv(ws=p + 4, normalise=normalise) == -2
        assert conv(wsn=need - 257, normalise=normalise) == -2
    # lookup
    st5 = (ctypes.c_int64 * 5)(3 * 8 * 16 * 3, 8 * 16 * 3, 16 * 3, 3, 1)

    def look(N=2, Lv=3, H=8, W=16, P=5, src=p, st=st5, dirs=p, dn=0, level=None, ln=0, out=p):
        return lib.reni_envmap_lookup(N, Lv, H, W, P, src, st, dirs, dn, level, ln, 0.0, out, None)

    for kw in (dict(N=0), dict(Lv=0), dict(H=0), dict(W=0), dict(P=0), dict(W=15), dict(N=65536), dict(Lv=65536),
               dict(H=1 << 15, W=1 << 15), dict(P=1 << 29), dict(N=1 << 10, P=1 << 19)):
        assert look(**kw) == -1, kw
    for kw in (dict(src=None), dict(st=None), dict(dirs=None), dict(out=None)):
        assert look(**kw) == -1 and b"NULL" in lib.reni_last_error(), kw
    for k in range(5):
        neg = (ctypes.c_int64 * 5)(*st5)
        neg[k] = -1
        assert look(st=neg) == -1 and b"strides" in lib.reni_last_error(), k
    big = (ctypes.c_int64 * 5)(*st5)
    big[2] = 1 << 31
    assert look(st=big) == -1
    for dn in (1, 3, 16):
        assert look(dn=dn) == -1 and b"dirs_stride_n" in lib.reni_last_error()
    for ln in (1, 3, 15):
        assert look(level=p, ln=ln) == -1 and b"level_stride_n" in lib.reni_last_error()
