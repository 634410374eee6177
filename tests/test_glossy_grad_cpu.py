"""CPU tests of differentiable glossy lighting (reni_tu_glossy_bwd.hip, the autograd functions of reni_amd.glossy).

Holds the fp32 numpy restatement of the lookup's transpose -- the tap table of k_envmap_lookup_taps and the sequential
per-texel sum of k_envmap_lookup_bwd -- with the bound tests/test_gpu_glossy_grad.py holds the device to, and what can be
checked of the new entries without a GPU: the ISA audit of the unit, the header / build / binding, the argument checks."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from reni_amd import _lib, glossy
from reni_amd.utils import get_directions
from tests import isa_audit
from tests.test_glossy_cpu import emulate_lookup_fp32, random_dirs
from tests.test_rotate_cpu import EPS32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("reni_lobe_denominators_workspace_bytes", "reni_lobe_denominators", "reni_lobe_backward_workspace_bytes",
       "reni_lobe_convolve_backward", "reni_envmap_lookup_taps", "reni_envmap_lookup_backward")


# ------------------------------------------------------------------------------------------ lookup transpose: restatement
def emulate_lookup_taps_fp32(Lv, H, W, dirs, level):
    """(index [P, 8] int64, weight [P, 8] fp32): the tap table of the header -- emulate_lookup_fp32's coordinate chain, each
    operation rounded once; taps (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1) on floor(level), then on the next level; the
    weights {gr gc, gr fc, fr gc, fr fc} x {gl, fl}, the next level 0 unless fl > 0"""
    f = np.float32
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

    def tap(i, j):  # tests/test_rotate_cpu.py::fetch's address: a row beyond a pole is the same row seen from the other side
        lo, hi = i < 0, i >= H
        j = np.where(lo | hi, j + W // 2, j)
        i = np.where(lo, -1 - i, np.where(hi, 2 * H - 1 - i, i))
        return i * W + np.mod(j, W)

    e4 = [tap(i, j), tap(i, j + 1), tap(i + 1, j), tap(i + 1, j + 1)]
    w4 = [gr * gc, gr * fc, fr * gc, fr * fc]
    lv = np.minimum(np.maximum(np.asarray(level, f), f(0)), f(Lv - 1))
    l0 = np.floor(lv).astype(np.int64)
    l1 = np.minimum(l0 + 1, Lv - 1)
    fl = (lv - np.floor(lv)).astype(f)
    gl = f(1) - fl
    two = fl > 0
    idx = np.stack([l0 * H * W + e for e in e4] + [l1 * H * W + e for e in e4], 1)
    wgt = np.stack([np.where(two, w * gl, w) for w in w4] + [np.where(two, w * fl, f(0)) for w in w4], 1).astype(f)
    return idx, wgt


def emulate_lookup_backward_fp32(g, idx, wgt, E):
    """[E, 3] fp32: every element's sum of weight x upstream over its taps, in the order a stable sort of the indices leaves
    them, one fp32 product and one fp32 addition a tap (taps of weight 0 are passed over)"""
    f = np.float32
    g = np.asarray(g, f)
    flat, w = idx.reshape(-1), wgt.reshape(-1)
    order = np.argsort(flat, kind="stable")
    keys = flat[order]
    offsets = np.searchsorted(keys, np.arange(E + 1))
    rank = np.arange(len(keys)) - offsets[keys]
    out = np.zeros((E, 3), f)
    for r in range(int(rank.max()) + 1):
        sel = order[rank == r]
        sel = sel[w[sel] != 0]
        out[flat[sel]] = out[flat[sel]] + (w[sel, None] * g[sel >> 3]).astype(f)
    return out


def lookup_transpose_case(H, W, seed=0):
    """(dirs [4096, 3], level [4096]) of the issue: random directions, every pixel centre, the six axes, the zero vector and
    (1e-8, 1, 0); levels in [-0.5, 2.5] with exact 1.0 and 2.0 among them"""
    g = np.random.default_rng(1000 + H + seed)
    special = np.asarray([[0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [1e-8, 1, 0]], np.float32)
    centres = get_directions(W)[0].numpy().astype(np.float32)
    dirs = np.concatenate([random_dirs(4096 - len(special) - len(centres), 11 + H + seed), centres, special])
    level = g.uniform(-0.5, 2.5, 4096).astype(np.float32)
    level[[0, 5, 4095]] = 1.0
    level[[1, 7, 4090]] = 2.0
    return dirs, level


def lookup_transpose_check(out, J, g, what):
    """out [E, 3] against J^T g in float64, J [P, E]: |out - J^T g| <= (8 + n_t) EPS32 (|J|^T |g|) per element, n_t the number of
    non-zero entries of the element's row of J^T; elements nobody sampled are exactly 0.  The 8: three roundings in each of
    the two weight products, the product with g, one spare; n_t: the fp32 sum, in any order."""
    J, g64, out = np.asarray(J, np.float64), np.asarray(g, np.float64), np.asarray(out, np.float64)
    ref, mag = J.T @ g64, np.abs(J).T @ np.abs(g64)
    nt = (J != 0).sum(0)
    bound = (8 + nt)[:, None] * EPS32 * mag
    err = np.abs(out - ref)
    ratio = float((err / np.where(bound > 0, bound, 1.0))[nt > 0].max())
    print(f"lookup transpose {what}: largest error / bound {ratio:.3f}, n_t up to {int(nt.max())}, {int((nt == 0).sum())} unsampled")
    assert (err <= bound).all(), (what, ratio)
    assert (out[nt == 0] == 0).all(), what
    return ratio


def host_J(Lv, H, W, dirs, level, chunk=128):
    """J [P, E] fp32 from emulate_lookup_fp32 on the one-hot chains, `chunk` of them a call (one a channel)"""
    E = Lv * H * W
    J = np.zeros((len(dirs), E), np.float32)
    for e0 in range(0, E, chunk):
        n = min(chunk, E - e0)
        chain = np.zeros((E, n), np.float32)
        chain[np.arange(e0, e0 + n), np.arange(n)] = 1.0
        J[:, e0:e0 + n] = emulate_lookup_fp32(chain.reshape(Lv, H, W, n), dirs, level)
    return J


@pytest.mark.parametrize("H,W", [(8, 16), (16, 32)])
def test_lookup_transpose_restatement_meets_the_bound(H, W):
    Lv = 3
    dirs, level = lookup_transpose_case(H, W)
    idx, wgt = emulate_lookup_taps_fp32(Lv, H, W, dirs, level)
    assert idx.min() >= 0 and idx.max() < Lv * H * W
    J = host_J(Lv, H, W, dirs, level)
    # the table IS the forward's matrix: scattering the weights reproduces J to the rounding of a duplicate tap's sum
    S = np.zeros_like(J, dtype=np.float64)
    np.add.at(S, (np.repeat(np.arange(len(dirs)), 8), idx.reshape(-1)), wgt.reshape(-1).astype(np.float64))
    assert np.abs(S - J).max() <= 2 * EPS32
    g = np.random.default_rng(H).standard_normal((len(dirs), 3)).astype(np.float32)
    out = emulate_lookup_backward_fp32(g, idx, wgt, Lv * H * W)
    lookup_transpose_check(out, J, g, f"{H} x {W} (host)")
    # exact levels read one level only
    assert (wgt[level == 1.0][:, 4:] == 0).all() and (wgt[level == 2.0][:, 4:] == 0).all()
    assert (idx[level == 1.0][:, :4] // (H * W) == 1).all() and (idx[level == 2.0][:, :4] // (H * W) == 2).all()


# ------------------------------------------------------------------------------------------ ISA audit, C ABI checks
def _assembly(unit):
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "unit.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, unit), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        return open(out).read()


def test_glossy_backward_translation_unit_isa_audit():
    """reni_tu_glossy_bwd.hip with build.sh's flags: no MFMA / transcendental / SDWA hazard, no scratch, every kernel present,
    the MFMAs in the six instances of the transposed convolution and nowhere else"""
    text = _assembly("reni_tu_glossy_bwd.hip")
    for k in ("k_lobe_recip", "k_lobe_convolve_t", "k_lobe_finish_t", "k_envmap_lookup_taps", "k_envmap_lookup_bwd"):
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.valu_to_mfma(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert sizes and all(int(x) == 0 for x in sizes)
    mf = isa_audit.mfma_functions(text)
    assert len(mf) == 6 and all("k_lobe_convolve_t" in f for f in mf)  # three kinds x one or two column tiles
    assert "v_mfma_f32_32x32x2_f32" in text and "atomic" not in text
    # the drain pad is in every instance, behind its last MFMA
    assert text.count("s_nop 15") == 6


def test_forward_unit_keeps_its_six_mfma_functions():
    """the denominators entry launches the forward's own instances: no seventh MFMA function in reni_tu_glossy.hip"""
    text = _assembly("reni_tu_glossy.hip")
    mf = isa_audit.mfma_functions(text)
    assert len(mf) == 6 and all("k_lobe_convolve" in f and "k_lobe_convolve_t" not in f for f in mf)
    assert "k_lobe_den_finish" in text


def test_header_build_and_binding_name_the_new_entries():
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    for name in NEW:
        assert re.search(r"^(int|size_t) " + name + r"\(", header, re.M) and name in _lib.EXPORTS, name
    assert "summed by ONE lane" in header  # the known limit of the gather is stated
    build = open(os.path.join(ROOT, "reni_amd", "csrc", "build.sh")).read()
    assert re.search(r"for tu in [^;]*\bglossy_bwd\b", build) and "_build/glossy_bwd.o" in build
    lib = _lib.load()
    for name in NEW:
        getattr(lib, name)


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    wsb = lib.reni_lobe_backward_workspace_bytes

    def conv(N=1, P=4, Q=10, ptrs=(p,) * 5, strides=(30, 3, 1), kinds=(0,), params=(2.0,), n_lobes=None, ws=p, wsn=1 << 15,
             normalise=1, den=p):
        ck = (ctypes.c_int32 * max(len(kinds), 1))(*kinds) if kinds is not None else None
        cp = (ctypes.c_float * max(len(params), 1))(*params) if params is not None else None
        nl = len(kinds) if n_lobes is None else n_lobes
        return lib.reni_lobe_convolve_backward(N, P, Q, ptrs[0], ptrs[1], ptrs[2], ptrs[3], nl, ck, cp, normalise, 1.0, den,
                                               ptrs[4], *strides, ws, wsn, None)

    for N, P, Q in ((0, 4, 10), (1, 0, 10), (1, 4, 0), (-1, 4, 10), (1, 1 << 29, 10), (1, 4, 1 << 29), (1 << 22, 1 << 8, 10)):
        assert conv(N, P, Q) == -1, (N, P, Q)
        assert wsb(N, P, Q, 1) == 0
    for nl in (0, 17, -1):
        assert conv(kinds=(0,) * 17, params=(2.0,) * 17, n_lobes=nl) == -1 and b"n_lobes" in lib.reni_last_error(), nl
        assert wsb(1, 4, 10, nl) == 0
    for kind in (3, -1, 100):
        assert conv(kinds=(0, kind), params=(2.0, 2.0)) == -1 and b"kind" in lib.reni_last_error(), kind
    for kind, par in ((0, 0.0), (0, -1.0), (0, float("nan")), (0, float("inf")), (1, 0.0), (2, 0.0), (2, 1.0001), (2, float("nan"))):
        assert conv(kinds=(1, kind), params=(20.0, par)) == -1, (kind, par)
        assert b"parameter" in lib.reni_last_error() or b"alpha" in lib.reni_last_error()
    for k in range(5):
        ptrs = [p] * 5
        ptrs[k] = None
        assert conv(ptrs=ptrs) == -1 and b"NULL" in lib.reni_last_error(), k
    assert conv(kinds=None, n_lobes=1) == -1 and b"NULL" in lib.reni_last_error()
    assert conv(params=None, n_lobes=1) == -1 and b"NULL" in lib.reni_last_error()
    assert conv(den=None) == -1 and b"den" in lib.reni_last_error()  # required iff normalise:
    assert conv(den=None, normalise=0, ws=None, wsn=0) == -2         # ... without it the next check is reached
    for st in ((-1, 3, 1), (30, -3, 1), (30, 3, -1)):
        assert conv(strides=st) == -1 and b"strides" in lib.reni_last_error()
    need = wsb(1, 4, 10, 1)
    assert need >= 3 * 3 * 10 * 4 and wsb(2, 4, 10, 1) > need  # three kinds' slabs of [3 N][Q] partial sums ...
    assert wsb(1, 1000, 10, 3) > wsb(1, 1000, 10, 1)  # ... and r [n_lobes][P]
    assert wsb(1, 180000, 512, 1) > 8 * wsb(1, 1000, 512, 1)  # Q = 512, P = 180 000 splits the o range
    for normalise in (0, 1):
        assert conv(ws=None, wsn=0, normalise=normalise) == -2
        assert conv(ws=p + 4, normalise=normalise) == -2
        assert conv(wsn=need - 257, normalise=normalise) == -2

    # the denominators
    dwb = lib.reni_lobe_denominators_workspace_bytes

    def den(P=4, Q=10, ptrs=(p,) * 4, kinds=(0,), params=(2.0,), n_lobes=None, ws=p, wsn=1 << 15):
        ck = (ctypes.c_int32 * max(len(kinds), 1))(*kinds) if kinds is not None else None
        cp = (ctypes.c_float * max(len(params), 1))(*params) if params is not None else None
        nl = len(kinds) if n_lobes is None else n_lobes
        return lib.reni_lobe_denominators(P, Q, ptrs[0], ptrs[1], ptrs[2], nl, ck, cp, ptrs[3], ws, wsn, None)

    for P, Q in ((0, 10), (4, 0), (-1, 10), (1 << 29, 10), (4, 1 << 29)):
        assert den(P, Q) == -1 and dwb(P, Q, 1) == 0, (P, Q)
    for nl in (0, 17):
        assert den(kinds=(0,) * 17, params=(2.0,) * 17, n_lobes=nl) == -1 and dwb(4, 10, nl) == 0
    assert den(kinds=(5,)) == -1 and b"kind" in lib.reni_last_error()
    assert den(kinds=(2,), params=(1.5,)) == -1 and b"alpha" in lib.reni_last_error()
    for k in range(4):
        ptrs = [p] * 4
        ptrs[k] = None
        assert den(ptrs=ptrs) == -1 and b"NULL" in lib.reni_last_error(), k
    assert den(kinds=None, n_lobes=1) == -1 and den(params=None, n_lobes=1) == -1
    dneed = dwb(4, 10, 1)
    assert dneed >= 4 * 4 and dwb(4, 10, 3) > dneed and dwb(512, 180000, 1) > 8 * dwb(512, 1000, 1)
    assert den(ws=None, wsn=0) == -2 and den(ws=p + 4) == -2 and den(wsn=dneed - 257) == -2

    # the lookup's taps and transpose
    def taps(T=2, Lv=3, H=8, W=16, P=5, dirs=p, dn=0, level=None, ln=0, idx=p, wgt=p):
        return lib.reni_envmap_lookup_taps(T, Lv, H, W, P, dirs, dn, level, ln, 0.0, idx, wgt, None)

    def back(N=2, Lv=3, H=8, W=16, P=5, g=p, T=1, wgt=p, order=p, offsets=p, out=p):
        return lib.reni_envmap_lookup_backward(N, Lv, H, W, P, g, T, wgt, order, offsets, out, None)

    for kw in (dict(Lv=0), dict(H=0), dict(W=0), dict(P=0), dict(W=15), dict(Lv=65536), dict(H=1 << 15, W=1 << 15),
               dict(Lv=4, H=1 << 14, W=1 << 15), dict(P=1 << 29)):
        assert taps(**kw) == -1 and back(**kw) == -1, kw
    assert taps(T=0) == -1 and taps(T=65536) == -1 and taps(T=1 << 10, P=1 << 19) == -1
    assert back(N=0) == -1 and back(N=65536) == -1 and back(N=1 << 10, P=1 << 19) == -1
    for kw in (dict(dirs=None), dict(idx=None), dict(wgt=None)):
        assert taps(**kw) == -1 and b"NULL" in lib.reni_last_error(), kw
    for dn in (1, 3, 16):
        assert taps(dn=dn) == -1 and b"dirs_stride_n" in lib.reni_last_error()
    for ln in (1, 3, 15):
        assert taps(level=p, ln=ln) == -1 and b"level_stride_n" in lib.reni_last_error()
    for kw in (dict(g=None), dict(out=None)):
        assert back(**kw) == -1 and b"NULL" in lib.reni_last_error(), kw
    for kw in (dict(wgt=None), dict(order=None), dict(offsets=None)):  # a bad tap table or CSR pointer
        assert back(**kw) == -1 and b"tap table" in lib.reni_last_error(), kw
    for T in (0, 3, -1):  # one table for all maps, or one a map
        assert back(T=T) == -1 and b"n_tables" in lib.reni_last_error(), T


def test_new_ops_and_the_renderer_have_no_cpu_fallback():
    from reni_amd import ops
    from reni_amd.envmap_shader import EnvironmentMap, GBuffer
    d, w = torch.zeros(10, 3), torch.ones(10)
    with pytest.raises(_lib.RENILibraryError):
        ops.lobe_denominators(d, w, d, ["phong"], [2.0])
    with pytest.raises(_lib.RENILibraryError):
        ops.lobe_convolve_backward(torch.ones(2, 1, 10, 3), d, w, d, ["phong"], [2.0])
    with pytest.raises(_lib.RENILibraryError):
        ops.lobe_convolve_backward(torch.ones(2, 1, 10, 3), d, w, d, ["phong"], [2.0], normalise=False)
    with pytest.raises(_lib.RENILibraryError):
        ops.envmap_lookup_table(2, 3, 8, 16, d, 1.0)
    with pytest.raises(_lib.RENILibraryError):
        ops.envmap_lookup_backward(torch.ones(2, 10, 3), 3, 8, 16, d, 1.0)
    # a map that requires grad on the CPU still has no fallback
    with pytest.raises(_lib.RENILibraryError):
        glossy.lobe_convolve(torch.ones(2, 10, 3, requires_grad=True), d, w, d, [glossy.phong(2)])
    with pytest.raises(_lib.RENILibraryError):
        glossy.lookup(torch.ones(2, 3, 8, 16, 3, requires_grad=True), d, 1.0)
    env = EnvironmentMap(torch.ones(1, 8 * 16, 3), get_directions(16), torch.ones(1, 8 * 16, 3))
    r = glossy.PrefilteredRenderer(GBuffer(torch.ones(16, 3), torch.zeros(16, 3), (0.0, 0.0, 2.0), 4), kd=0.6, out_width=8)
    assert r.ks == pytest.approx(0.4) and r.shininess == 500.0 and torch.equal(r.camera_center, torch.tensor([0.0, 0.0, 2.0]))
    with pytest.raises(_lib.RENILibraryError):
        r(envmap=env)
    with pytest.raises(ValueError):
        glossy.PrefilteredRenderer(object(), kd=0.5)
    with pytest.raises(ValueError):
        glossy.PrefilteredRenderer(GBuffer(torch.ones(16, 3), torch.zeros(16, 3), (0.0, 0.0, 2.0), 4), kd=0.5, out_width=7)


def test_constants_that_require_grad_raise():
    """directions, weights and levels are constants: asking for their gradient is an error, not silence"""
    src, d, w = torch.ones(2, 10, 3), torch.zeros(10, 3), torch.ones(10)
    L = [glossy.phong(2)]
    for kw in (dict(in_dirs=d.clone().requires_grad_()), dict(out_dirs=d.clone().requires_grad_()),
               dict(in_weight=w.clone().requires_grad_())):
        a = dict(in_dirs=d, in_weight=w, out_dirs=d)
        a.update(kw)
        with pytest.raises(ValueError, match="requires grad"):
            glossy.lobe_convolve(src, a["in_dirs"], a["in_weight"], a["out_dirs"], L)
    with pytest.raises(ValueError, match="dirs requires grad"):
        glossy.lookup(torch.ones(2, 8, 16, 3), d.clone().requires_grad_())
    with pytest.raises(ValueError, match="level requires grad"):
        glossy.lookup(torch.ones(2, 3, 8, 16, 3), d, torch.ones(10, requires_grad=True))
