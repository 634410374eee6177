"""GPU tests of the glossy lighting kernels (reni_tu_glossy.hip, reni_tu_glossy_bwd.hip) at the shapes where their tails,
guards, splits and tile edges act: the cases of tests/glossy_edge_cases.py against float64, per map and per lobe, within
tests/test_glossy_cpu.py::lobe_tol (twice it for the normalised transpose, as tests/test_gpu_glossy_grad.py has it);
indicator maps that show a texel visited twice or never as a factor of 2 or as 0; sixteen lobes a launch; determinism and
batch independence across a three-way split; pinned values at t = 1, 0, -1; guard bands around every output; poisoned
workspaces; and the lookup, its tap table and its transpose at H = 1, 2, W = 2, one level and P around a 256-lane block.
tests/test_glossy_edges_cpu.py shows that plain fp32 arithmetic stays within 0.75 of each budget at every case.

Each parity test prints its worst error / budget before it asserts (pytest -s or -rA shows them)."""
import ctypes

import numpy as np
import pytest
import torch

from reni_amd import glossy, ops
from tests import glossy_edge_cases as E
from tests.test_glossy_cpu import lobe_tol, np_lobe_convolve, np_lookup_chain
from tests.test_glossy_grad_cpu import lookup_transpose_check
from tests.test_gpu_baseline_edges import Carved, _workspace
from tests.test_gpu_glossy_grad import _device_J
from tests.test_rotate_cpu import EPS32

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
NINE = E.LOBE_SETS["nine"]
ONE_KIND = (glossy.phong(8), glossy.phong(64))
FWD_IDS = [f"{P}x{Q}" for P, Q in E.FWD_SHAPES]
BWD_IDS = [f"{P}x{Q}" for P, Q in E.BWD_SHAPES]
LOOKUP_IDS = ["x".join(str(v) for v in c) for c in E.LOOKUP_CASES]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from reni_amd import _lib
    return _lib.load()


def _kp(lobes):
    return [l.kind for l in lobes], [l.param for l in lobes]


def _ckp(lobes):
    from reni_amd import _lib
    return (len(lobes), (ctypes.c_int32 * len(lobes))(*[_lib.LOBE_KIND[l.kind] for l in lobes]),
            (ctypes.c_float * len(lobes))(*[l.param for l in lobes]))


def _np(x):
    return x.double().cpu().numpy()


_OPERANDS = {}


def _fwd(P, Q, name="nine"):
    """the forward case with its tensors on the device (moved once)"""
    key = ("f", P, Q, name)
    if key not in _OPERANDS:
        c = E.fwd_case(P, Q, name)
        _OPERANDS[key] = (c, c.src.to(DEV), c.in_dirs.to(DEV), c.w.to(DEV), c.out_dirs.to(DEV))
    return _OPERANDS[key]


def _bwd(P, Q, name="nine"):
    key = ("b", P, Q, name)
    if key not in _OPERANDS:
        c = E.bwd_case(P, Q, name)
        _OPERANDS[key] = (c, c.g.to(DEV), c.in_dirs.to(DEV), c.w.to(DEV), c.out_dirs.to(DEV))
    return _OPERANDS[key]


def _ratios(out, ref, lobes, factor=1.0):
    """[N, Lv]: error / budget of every map and lobe; out, ref [N, Lv, ...]"""
    out = _np(out) if isinstance(out, torch.Tensor) else np.asarray(out, np.float64)
    assert out.shape == ref.shape and np.isfinite(out).all()
    return np.stack([E.per_map_rel(out[:, k], ref[:, k]) / (factor * lobe_tol(tuple(l))) for k, l in enumerate(lobes)], 1)


# ---------------------------------------------------------------------------------------------- C entry points
def c_lobe_convolve(src, in_dirs, w, out_dirs, lobes, normalise, scale, out_ptr, ws_fill=0, planar=False):
    """reni_lobe_convolve through the C entry point: src [N, Q, 3], or [N, 3, Q] when planar; the output wherever out_ptr says"""
    N, Q, P = src.shape[0], in_dirs.shape[0], out_dirs.shape[0]
    assert tuple(src.shape) == ((N, 3, Q) if planar else (N, Q, 3))
    lib = _lib()
    Lv, ck, cp = _ckp(lobes)
    need = int(lib.reni_lobe_workspace_bytes(N, P, Q, Lv))
    ws, wp, wn = _workspace(need, ws_fill)
    sn, si, sc = (int(s) for s in src.stride())
    if planar:
        si, sc = sc, si
    rc = lib.reni_lobe_convolve(N, P, Q, out_dirs.data_ptr(), in_dirs.data_ptr(), w.data_ptr(), src.data_ptr(), sn, si, sc, Lv, ck, cp,
                                1 if normalise else 0, float(scale), out_ptr, wp, wn, _stream())
    assert rc == 0, lib.reni_last_error()
    torch.cuda.synchronize()
    return need


def c_lobe_denominators(in_dirs, w, out_dirs, lobes, den_ptr, ws_fill=0):
    Q, P = in_dirs.shape[0], out_dirs.shape[0]
    lib = _lib()
    Lv, ck, cp = _ckp(lobes)
    need = int(lib.reni_lobe_denominators_workspace_bytes(P, Q, Lv))
    ws, wp, wn = _workspace(need, ws_fill)
    rc = lib.reni_lobe_denominators(P, Q, out_dirs.data_ptr(), in_dirs.data_ptr(), w.data_ptr(), Lv, ck, cp, den_ptr, wp, wn, _stream())
    assert rc == 0, lib.reni_last_error()
    torch.cuda.synchronize()
    return need


def c_lobe_backward(g, in_dirs, w, out_dirs, lobes, normalise, scale, den, out_ptr, planar=False, ws_fill=0):
    """reni_lobe_convolve_backward through the C entry point: grad_src [N, Q, 3], or [N, 3, Q] when planar, at out_ptr"""
    N, Q, P = g.shape[0], in_dirs.shape[0], out_dirs.shape[0]
    assert g.is_contiguous() and tuple(g.shape) == (N, len(lobes), P, 3)
    lib = _lib()
    Lv, ck, cp = _ckp(lobes)
    need = int(lib.reni_lobe_backward_workspace_bytes(N, P, Q, Lv))
    ws, wp, wn = _workspace(need, ws_fill)
    sn, si, sc = (3 * Q, 1, Q) if planar else (3 * Q, 3, 1)
    rc = lib.reni_lobe_convolve_backward(N, P, Q, out_dirs.data_ptr(), in_dirs.data_ptr(), w.data_ptr(), g.data_ptr(), Lv, ck, cp,
                                         1 if normalise else 0, float(scale), den.data_ptr() if normalise else None, out_ptr,
                                         sn, si, sc, wp, wn, _stream())
    assert rc == 0, lib.reni_last_error()
    torch.cuda.synchronize()
    return need


# ---------------------------------------------------------------------------------------------- forward parity
@pytest.mark.parametrize("P,Q", E.FWD_SHAPES, ids=FWD_IDS)
def test_forward_edge_shapes_match_float64(P, Q):
    """Q = 1, 2, 3 (the odd tail with and without a main loop), P < 32 and P = 33, 257 (idle waves, masked rows, a second
    workgroup), the split boundary 4095 | 4096 | 4097 and three chunks at 6145, ncol = 4, 31, 34, 64, 67; the interleaved
    and the planar layout give the same bits; an indicator map's result is one product."""
    c, src, in_dirs, w, out_dirs = _fwd(P, Q)
    worst = [0.0, 0.0, 0.0]
    for N in E.LB_N:
        s = src[:N]
        out = glossy.lobe_convolve(s, in_dirs, w, out_dirs, NINE)
        raw = glossy.lobe_convolve(s, in_dirs, w, out_dirs, NINE, normalise=False, scale=E.SCALE)
        assert out.shape == raw.shape == (N, 9, P, 3)
        rn = _ratios(out, c.num[:N] / c.den[None, :, :, None], NINE)
        ru = _ratios(raw, E.SCALE * c.num[:N], NINE)
        worst[0], worst[1] = max(worst[0], rn.max()), max(worst[1], ru.max())
        print(f"forward ({P}, {Q}) N={N}: error / budget normalised {rn.max():.3f}, unnormalised {ru.max():.3f}")
        assert rn.max() <= 1.0 and ru.max() <= 1.0, (P, Q, N, rn.max(), ru.max())
        planar = s.permute(0, 2, 1).contiguous()  # [N, 3, Q]
        for normalise, want in ((True, out), (False, raw)):
            got = Carved(N, 9, P, 3)
            c_lobe_convolve(planar, in_dirs, w, out_dirs, NINE, normalise, E.SCALE, got.ptr, planar=True)
            got.check(want, f"planar {(P, Q, N, normalise)}")
        if Q != 3:  # the wrapper tells the layouts apart by shape: it reads [N, 3, 3] as [N, Q, 3]
            assert torch.equal(glossy.lobe_convolve(planar, in_dirs, w, out_dirs, NINE), out), (P, Q, N)
            assert torch.equal(glossy.lobe_convolve(planar.permute(0, 2, 1), in_dirs, w, out_dirs, NINE, normalise=False, scale=E.SCALE), raw)
    ind = glossy.lobe_convolve(c.ind_src.to(DEV), in_dirs, w, out_dirs, NINE, normalise=False, scale=E.SCALE)
    ri = _ratios(ind, c.ind_ref, NINE)
    worst[2] = ri.max()
    print(f"forward ({P}, {Q}) indicator maps at texels {c.ind_texel}: error / budget {ri.max():.3f}")
    assert ri.max() <= 1.0, (P, Q, ri.max())
    for k in range(len(c.ind_texel)):  # nothing of a map reaches a channel it does not have
        others = [ch for ch in range(3) if ch != k % 3]
        assert float(ind[k][:, :, others].abs().max()) == 0.0, (P, Q, k)
    print(f"forward ({P}, {Q}): worst error / budget normalised {worst[0]:.3f}, unnormalised {worst[1]:.3f}, indicator {worst[2]:.3f}")


@pytest.mark.parametrize("P,Q", E.FWD_SHAPES, ids=FWD_IDS)
def test_denominators_are_the_forwards_at_the_edge_shapes(P, Q):
    c, _, in_dirs, w, out_dirs = _fwd(P, Q)
    den = ops.lobe_denominators(in_dirs, w, out_dirs, *_kp(NINE))
    assert den.shape == (9, P)
    raw = glossy.lobe_convolve(torch.ones(1, Q, 3, device=DEV), in_dirs, w, out_dirs, NINE, normalise=False, scale=1.0)
    for ch in range(3):
        assert torch.equal(raw[0, :, :, ch], den), (P, Q, ch)
    r = _ratios(den[None], c.den[None], NINE)
    print(f"denominators ({P}, {Q}): error / budget {r.max():.3f}")
    assert r.max() <= 1.0
    for k in (0, 4, 8):  # a lobe's denominators do not depend on the lobes around it
        assert torch.equal(ops.lobe_denominators(in_dirs, w, out_dirs, *_kp(NINE[k:k + 1]))[0], den[k]), (P, Q, k)


# ---------------------------------------------------------------------------------------------- transpose parity
@pytest.mark.parametrize("P,Q", E.BWD_SHAPES, ids=BWD_IDS)
def test_transpose_edge_shapes_match_float64(P, Q):
    """The forward's shapes with P and Q exchanged: the reduction over the rows has 1, 2, 3 steps, an odd tail, two and three
    chunks; every lobe alone, the nine together (the do-while over the lobes of a kind), the indicator gradients, planar."""
    c, g, in_dirs, w, out_dirs = _bwd(P, Q)
    kinds, params = _kp(NINE)
    den = ops.lobe_denominators(in_dirs, w, out_dirs, kinds, params)
    worst = {True: 0.0, False: 0.0}
    for N in E.LB_N:
        for normalise, ref, factor in ((True, c.refN[:, :N], 2.0), (False, c.refU[:, :N], 1.0)):
            outs = [ops.lobe_convolve_backward(g[:N, k:k + 1].contiguous(), in_dirs, w, out_dirs, [l.kind], [l.param], normalise,
                                               E.SCALE, den=den[k:k + 1] if normalise else None) for k, l in enumerate(NINE)]
            assert all(o.shape == (N, Q, 3) for o in outs)
            r = _ratios(torch.stack(outs, 1), np.swapaxes(ref, 0, 1), NINE, factor)
            worst[normalise] = max(worst[normalise], r.max())
            assert r.max() <= 1.0, (P, Q, N, normalise, r.max())
            # the nine together: within the sum of the lobes' budgets, map by map
            bound = sum(factor * lobe_tol(tuple(l)) * np.abs(ref[k]).reshape(N, -1).max(axis=1) for k, l in enumerate(NINE))
            gN = g[:N].contiguous()
            out = ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, kinds, params, normalise, E.SCALE, den=den if normalise else None)
            err = np.abs(_np(out) - ref.sum(0)).reshape(N, -1).max(axis=1)
            print(f"transpose ({P}, {Q}) N={N} {'normalised' if normalise else 'unnormalised'}: error / budget a lobe alone "
                  f"{r.max():.3f}, the nine together {(err / bound).max():.3f}")
            assert bool(torch.isfinite(out).all()) and (err <= bound).all(), (P, Q, N, normalise, (err / bound).max())
            planar = ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, kinds, params, normalise, E.SCALE,
                                                den=den if normalise else None, planar=True)
            assert planar.shape == (N, 3, Q) and torch.equal(planar.permute(0, 2, 1), out)
        # the denominators are computed inside when they are not handed in: the same bits
        assert torch.equal(ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, kinds, params, True),
                           ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, kinds, params, True, den=den))
    # indicator gradients at the first and last row and either side of the chunk boundaries: one product a texel
    ig = c.ind_g.to(DEV)
    K = len(c.ind_row)
    for normalise, ref, factor in ((True, c.indN, 2.0), (False, c.indU, 1.0)):
        outs = [ops.lobe_convolve_backward(ig[:, k:k + 1].contiguous(), in_dirs, w, out_dirs, [l.kind], [l.param], normalise, E.SCALE,
                                           den=den[k:k + 1] if normalise else None) for k, l in enumerate(NINE)]
        stack = torch.stack(outs, 1)
        r = _ratios(stack, np.swapaxes(ref, 0, 1), NINE, factor)
        print(f"transpose ({P}, {Q}) indicator gradients at rows {c.ind_row}, {'normalised' if normalise else 'unnormalised'}: "
              f"error / budget {r.max():.3f}")
        assert r.max() <= 1.0, (P, Q, normalise, r.max())
        for k in range(K):
            others = [ch for ch in range(3) if ch != k % 3]
            assert float(stack[k][:, :, others].abs().max()) == 0.0, (P, Q, k)
        bound = sum(factor * lobe_tol(tuple(l)) * np.abs(ref[k]).reshape(K, -1).max(axis=1) for k, l in enumerate(NINE))
        out = ops.lobe_convolve_backward(ig, in_dirs, w, out_dirs, kinds, params, normalise, E.SCALE, den=den if normalise else None)
        assert (np.abs(_np(out) - ref.sum(0)).reshape(K, -1).max(axis=1) <= bound).all(), (P, Q, normalise)
    print(f"transpose ({P}, {Q}): worst error / budget normalised {worst[True]:.3f}, unnormalised {worst[False]:.3f}")


@pytest.mark.parametrize("P,Q,which", [(33, 4097, "f"), (4097, 33, "b")], ids=["33x4097", "4097x33"])
def test_adjoint_identity_across_the_split(P, Q, which):
    """<A x, y> = <x, A^T y> in float64 from the device's outputs, unnormalised, lobe by lobe, within the sum of the two
    budgets: lobe_tol max |A x| sum |y| + lobe_tol max |A^T y| sum |x|, map by map"""
    N = 11
    if which == "f":
        c, x, in_dirs, w, out_dirs = _fwd(P, Q)
        y = torch.randn(N, 9, P, 3, generator=torch.Generator().manual_seed(P)).to(DEV)
    else:
        c, y, in_dirs, w, out_dirs = _bwd(P, Q)
        x = (torch.rand(N, Q, 3, generator=torch.Generator().manual_seed(P)) * 3).to(DEV)
    x, y = x[:N], y[:N].contiguous()
    Ax = _np(glossy.lobe_convolve(x, in_dirs, w, out_dirs, NINE, normalise=False, scale=E.SCALE))  # [N, 9, P, 3]
    x64, y64 = _np(x), _np(y)
    worst = 0.0
    for k, l in enumerate(NINE):
        ATy = _np(ops.lobe_convolve_backward(y[:, k:k + 1].contiguous(), in_dirs, w, out_dirs, [l.kind], [l.param], False, E.SCALE))
        lhs, rhs = (Ax[:, k] * y64[:, k]).sum(), (x64 * ATy).sum()
        bound = lobe_tol(tuple(l)) * ((np.abs(Ax[:, k]).reshape(N, -1).max(1) * np.abs(y64[:, k]).reshape(N, -1).sum(1)).sum()
                                      + (np.abs(ATy).reshape(N, -1).max(1) * np.abs(x64).reshape(N, -1).sum(1)).sum())
        worst = max(worst, abs(lhs - rhs) / bound)
        assert abs(lhs - rhs) <= bound, (l, lhs, rhs, bound)
    print(f"adjoint ({P}, {Q}): largest |<Ax, y> - <x, A^T y>| / bound {worst:.4f}")


# ---------------------------------------------------------------------------------------------- sixteen lobes
@pytest.mark.parametrize("name", ["phong16", "mix16"])
def test_sixteen_lobes_a_launch(name):
    """LB_MAX_LOBES lobes: sixteen of one kind along z (forward) and inside one workgroup's loop (transpose), and 6 + 5 + 5"""
    L = E.LOBE_SETS[name]
    kinds, params = _kp(L)
    c, src, in_dirs, w, out_dirs = _fwd(*E.SIXTEEN_FWD, name)
    s = src[:11]
    for normalise, ref in ((True, c.num[:11] / c.den[None, :, :, None]), (False, E.SCALE * c.num[:11])):
        kw = dict(normalise=normalise, scale=E.SCALE)
        out = glossy.lobe_convolve(s, in_dirs, w, out_dirs, L, **kw)
        r = _ratios(out, ref, L)
        print(f"{name} forward {'normalised' if normalise else 'unnormalised'}: error / budget {r.max():.3f}")
        assert r.max() <= 1.0
        for k, l in enumerate(L):
            assert torch.equal(glossy.lobe_convolve(s, in_dirs, w, out_dirs, [l], **kw)[:, 0], out[:, k]), l
        assert torch.equal(glossy.lobe_convolve(s, in_dirs, w, out_dirs, L[::-1], **kw), out.flip(1))
    c, g, in_dirs, w, out_dirs = _bwd(*E.SIXTEEN_BWD, name)
    g = g[:11].contiguous()
    den = ops.lobe_denominators(in_dirs, w, out_dirs, kinds, params)
    dref = _ratios(den[None], c.den[None], L)
    assert dref.max() <= 1.0
    for normalise, ref, factor in ((True, c.refN[:, :11], 2.0), (False, c.refU[:, :11], 1.0)):
        outs = [ops.lobe_convolve_backward(g[:, k:k + 1].contiguous(), in_dirs, w, out_dirs, [l.kind], [l.param], normalise, E.SCALE,
                                           den=den[k:k + 1] if normalise else None) for k, l in enumerate(L)]
        r = _ratios(torch.stack(outs, 1), np.swapaxes(ref, 0, 1), L, factor)
        bound = sum(factor * lobe_tol(tuple(l)) * np.abs(ref[k]).reshape(11, -1).max(axis=1) for k, l in enumerate(L))
        out = ops.lobe_convolve_backward(g, in_dirs, w, out_dirs, kinds, params, normalise, E.SCALE, den=den if normalise else None)
        err = np.abs(_np(out) - ref.sum(0)).reshape(11, -1).max(axis=1)
        # the reversed list with the gradients flipped is the same sum, its lobes added in the other order
        rk, rp = _kp(L[::-1])
        rev = ops.lobe_convolve_backward(g.flip(1).contiguous(), in_dirs, w, out_dirs, rk, rp, normalise, E.SCALE,
                                         den=den.flip(0).contiguous() if normalise else None)
        err_rev = np.abs(_np(rev) - ref.sum(0)).reshape(11, -1).max(axis=1)
        print(f"{name} transpose {'normalised' if normalise else 'unnormalised'}: error / budget a lobe alone {r.max():.3f}, the "
              f"sixteen together {(err / bound).max():.3f}, reversed {(err_rev / bound).max():.3f}")
        assert r.max() <= 1.0 and (err <= bound).all() and (err_rev <= bound).all()


# ---------------------------------------------------------------------------------------------- determinism, batch independence
@pytest.mark.parametrize("normalise", [True, False])
def test_three_way_split_is_deterministic_and_batch_independent(normalise):
    """(1, 6145) forward and (6145, 1) transposed: the finish loops run twice.  Two calls give the same bits; maps 0, 10 and
    N - 1 alone give the bits they have in a batch of 11 and of 22; a map that holds an Inf and a NaN leaves every other map's
    bits, those of its own 32-column tile among them, as they were."""
    c, src, in_dirs, w, out_dirs = _fwd(1, 6145)
    assert c.S == 3
    kw = dict(normalise=normalise, scale=E.SCALE)
    for N in (11, 22):
        full = glossy.lobe_convolve(src[:N], in_dirs, w, out_dirs, NINE, **kw)
        assert torch.equal(glossy.lobe_convolve(src[:N], in_dirs, w, out_dirs, NINE, **kw), full)
        for n in (0, 10, N - 1):
            assert torch.equal(glossy.lobe_convolve(src[n:n + 1], in_dirs, w, out_dirs, NINE, **kw)[0], full[n]), (N, n)
        bad = src[:N].clone()
        bad[5, 6144, 0], bad[5, 2049, 1], bad[5, 7, 2] = float("inf"), float("nan"), float("-inf")
        other = [n for n in range(N) if n != 5]
        got = glossy.lobe_convolve(bad, in_dirs, w, out_dirs, NINE, **kw)
        assert torch.equal(got[other], full[other]) and not bool(torch.isfinite(got[5]).all()), N
    c, g, in_dirs, w, out_dirs = _bwd(6145, 1)
    assert c.S == 3
    kinds, params = _kp(NINE)
    den = ops.lobe_denominators(in_dirs, w, out_dirs, kinds, params)
    bk = dict(normalise=normalise, scale=E.SCALE, den=den if normalise else None)
    for N in (11, 22):
        gN = g[:N].contiguous()
        full = ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, kinds, params, **bk)
        assert torch.equal(ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, kinds, params, **bk), full)
        for n in (0, 10, N - 1):
            assert torch.equal(ops.lobe_convolve_backward(g[n:n + 1].contiguous(), in_dirs, w, out_dirs, kinds, params, **bk)[0], full[n])
        bad = gN.clone()
        bad[5, 0, 6144, 0], bad[5, 4, 2049, 1], bad[5, 8, 0, 2] = float("inf"), float("nan"), float("-inf")
        other = [n for n in range(N) if n != 5]
        got = ops.lobe_convolve_backward(bad, in_dirs, w, out_dirs, kinds, params, **bk)
        assert torch.equal(got[other], full[other]) and not bool(torch.isfinite(got[5]).all()), N


# ---------------------------------------------------------------------------------------------- pinned values
def _pinned(in_dirs, w, out_dirs, src, what, lobes=NINE):
    """both results of a small case against float64 of the same fp32 inputs, per map and lobe; returns them"""
    i, ww, o, s = (torch.as_tensor(np.asarray(x, np.float32)).to(DEV) for x in (in_dirs, w, out_dirs, src))
    norm = glossy.lobe_convolve(s, i, ww, o, lobes)
    raw = glossy.lobe_convolve(s, i, ww, o, lobes, normalise=False, scale=E.SCALE)
    ops64 = (_np(s), _np(i), _np(ww), _np(o), [tuple(l) for l in lobes])
    refn, refu = np_lobe_convolve(*ops64), np_lobe_convolve(*ops64, normalise=False, scale=E.SCALE)
    assert bool(torch.isfinite(norm).all()) and bool(torch.isfinite(raw).all()), what
    for got, ref, name in ((norm, refn, "normalised"), (raw, refu, "unnormalised")):
        err = np.abs(_np(got) - ref)
        for k, l in enumerate(lobes):
            scale = np.abs(ref[:, k]).reshape(len(ref), -1).max(axis=1)
            e = err[:, k].reshape(len(ref), -1).max(axis=1)
            assert (e <= lobe_tol(tuple(l)) * scale).all(), (what, name, l, e, scale)  # (a map that is 0 in float64 is 0 here)
    return norm, raw


def test_pinned_directions():
    """t = 1 (an output direction that IS a texel's: the fp32 dot rounds to 1 or just above it), t = -1, t = 0 exactly, and
    directions of length 2 (t = 4, -4: the clamps act) -- against float64 of the same inputs, and where the value is known
    exactly, against that"""
    gen = torch.Generator().manual_seed(77)
    u = E._unit(gen, 40).float().numpy()  # 40 texels, each its own output direction: every row has t = 1 with one of them
    w = (0.5 + 0.5 * torch.rand(40, generator=gen)).numpy() * (4 * np.pi / 40)
    src = (torch.rand(3, 40, 3, generator=gen) * 3).numpy()
    t = E.t_fp32(u, u).diagonal()
    assert (t >= 1 - 2.0 ** -22).all() and (t > 1).any() and (t <= 1).any()  # both sides of 1 occur
    _pinned(u, w, u, src, "t = 1")
    # the six axes at length 2: t = 0, +-2, +-4, all exact, so only the clamps act
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    _pinned(axes, w[:6], 2 * axes, src[:, :6], "length 2, t = +-2")
    _pinned(2 * axes, w[:6], 2 * axes, src[:, :6], "length 2 both, t = +-4")
    # one texel, seen head-on, from behind and edge-on.  (Without blinn(500): (1/2)^250 is 0 in fp32 and not in float64, the
    # underflow that tests/glossy_edge_cases.py keeps out of every comparison)
    lobes = [l for l in NINE if not (l.kind == "blinn" and l.param > 100)]
    one, w1, s1 = np.asarray([[0.0, 0.0, 1.0]], np.float32), np.asarray([1.5], np.float32), np.asarray([[[1.0, 2.0, 0.5]]], np.float32)
    rows = np.asarray([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [0, 0, 2], [0, 0, -2]], np.float32)
    norm, raw = _pinned(one, w1, rows, s1, "axes", lobes)
    norm, raw = norm.cpu().numpy(), raw.cpu().numpy()
    for k, l in enumerate(lobes):
        peak = 1.0 / l.param ** 2 if l.kind == "ggx" else 1.0  # f(1)
        for row in (0, 4):  # t = 1 and t = 2: f(1) w scale src, and the map itself when normalised
            assert np.abs(raw[0, k, row] - peak * 1.5 * E.SCALE * s1[0, 0]).max() <= 16 * EPS32 * peak * 1.5 * 2, (l, row)
            assert np.abs(norm[0, k, row] - s1[0, 0]).max() <= 8 * EPS32 * 2, (l, row)
        for row in (1, 5):  # t = -1, -2: every lobe is exactly 0, and the normalised result follows "0 where the sum is not positive"
            assert (raw[0, k, row] == 0).all() and (norm[0, k, row] == 0).all(), (l, row)
        for row in (2, 3):  # t = 0: phong and ggx are exactly 0; blinn is (1/2)^(s/2)
            if l.kind == "blinn":
                assert np.abs(norm[0, k, row] - s1[0, 0]).max() <= 8 * EPS32 * 2 and (raw[0, k, row] > 0).all(), (l, row)
            else:
                assert (raw[0, k, row] == 0).all() and (norm[0, k, row] == 0).all(), (l, row)


def test_zero_and_negative_weights():
    """All-zero weights give 0 and no NaN, normalised or not, in both directions; a row whose weights sum to a negative
    denominator follows "0 where the sum is not positive" while the row beside it stays what float64 says"""
    gen = torch.Generator().manual_seed(78)
    d, o = E._unit(gen, 37).float().to(DEV), E._unit(gen, 35).float().to(DEV)
    src = (torch.rand(3, 37, 3, generator=gen) * 3).to(DEV)
    g = torch.randn(3, 9, 35, 3, generator=gen).to(DEV)
    zero = torch.zeros(37, device=DEV)
    kinds, params = _kp(NINE)
    for normalise in (True, False):
        out = glossy.lobe_convolve(src, d, zero, o, NINE, normalise=normalise, scale=E.SCALE)
        assert torch.equal(out, torch.zeros_like(out)), normalise
        back = ops.lobe_convolve_backward(g, d, zero, o, kinds, params, normalise, E.SCALE)
        assert torch.equal(back, torch.zeros_like(back)), normalise
    assert torch.equal(ops.lobe_denominators(d, zero, o, kinds, params), torch.zeros(9, 35, device=DEV))
    # two opposite texels of weight +1 and -1: the row at the second one has den = -f(1) + f(-1) < 0
    in_dirs = np.asarray([[1, 0, 0], [-1, 0, 0]], np.float32)
    w = np.asarray([1.0, -1.0], np.float32)
    s2 = np.asarray([[[1.0, 2.0, 3.0], [0.5, 0.25, 4.0]]], np.float32)
    norm, raw = _pinned(in_dirs, w, in_dirs, s2, "negative weight")
    assert float(norm[0, :, 1].abs().max()) == 0.0 and float(norm[0, :, 0].min()) > 0
    assert float(raw[0, :, 1].max()) < 0  # the unnormalised sum is what it is
    i, ww = torch.from_numpy(in_dirs).to(DEV), torch.from_numpy(w).to(DEV)
    den = ops.lobe_denominators(i, ww, i, kinds, params)
    assert bool((den[:, 0] > 0).all()) and bool((den[:, 1] < 0).all())
    g2 = torch.randn(2, 9, 2, 3, generator=gen).to(DEV)
    back = _np(ops.lobe_convolve_backward(g2, i, ww, i, kinds, params, True))
    # float64: r = 1 / den where den > 0, else 0 -- row 1 contributes nothing
    for k, l in enumerate(NINE):
        one = _np(ops.lobe_convolve_backward(g2[:, k:k + 1].contiguous(), i, ww, i, [l.kind], [l.param], True))
        f = E.np_lobe(tuple(l), np.asarray([[1.0, -1.0]]))[0]  # row 0 against the two texels
        ref = (w.astype(np.float64) * f)[None, :, None] * _np(g2)[:, k, 0][:, None, :] / (f * w).sum()
        assert np.abs(one - ref).max() <= 2 * lobe_tol(tuple(l)) * np.abs(ref).max(), l
    assert np.isfinite(back).all()


# ---------------------------------------------------------------------------------------------- guard bands
def test_convolution_outputs_stay_inside_their_buffers():
    """forward (33, 3), N = 11: the second output tile holds one live row, the odd tail is the second of two steps, ncol = 34
    leaves two live columns in the second tile; the denominators; the transpose (3, 33) in both stride orders"""
    N = 11
    c, src, in_dirs, w, out_dirs = _fwd(33, 3)
    for normalise in (True, False):
        out = Carved(N, 9, 33, 3)
        c_lobe_convolve(src[:N].contiguous(), in_dirs, w, out_dirs, NINE, normalise, E.SCALE, out.ptr)
        out.check(glossy.lobe_convolve(src[:N], in_dirs, w, out_dirs, NINE, normalise=normalise, scale=E.SCALE), f"forward {normalise}")
    den = Carved(9, 33)
    c_lobe_denominators(in_dirs, w, out_dirs, NINE, den.ptr)
    den.check(ops.lobe_denominators(in_dirs, w, out_dirs, *_kp(NINE)), "denominators")
    c, g, in_dirs, w, out_dirs = _bwd(3, 33)
    gN = g[:N].contiguous()
    d = ops.lobe_denominators(in_dirs, w, out_dirs, *_kp(NINE))
    for normalise in (True, False):
        for planar in (False, True):
            out = Carved(*((N, 3, 33) if planar else (N, 33, 3)))
            c_lobe_backward(gN, in_dirs, w, out_dirs, NINE, normalise, E.SCALE, d, out.ptr, planar=planar)
            out.check(ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, *_kp(NINE), normalise, E.SCALE, den=d, planar=planar),
                      f"transpose {normalise} planar {planar}")


def test_lookup_outputs_stay_inside_their_buffers():
    """(H, W, Lv, P) = (2, 4, 2, 257): one lane in the second block; the lookup, the taps' two tables, the lookup's transpose"""
    H, W, Lv, P = 2, 4, 2, 257
    c = E.lookup_case(H, W, Lv, P)
    lib = _lib()
    chain = torch.from_numpy(c.chain).to(DEV)
    dirs, level = torch.from_numpy(c.dirs).to(DEV), torch.from_numpy(c.level).to(DEV)
    out = Carved(3, P, 3)
    st = (ctypes.c_int64 * 5)(*chain.stride())
    rc = lib.reni_envmap_lookup(3, Lv, H, W, P, chain.data_ptr(), st, dirs.data_ptr(), 0, level.data_ptr(), 0, 0.0, out.ptr, _stream())
    assert rc == 0, lib.reni_last_error()
    out.check(glossy.lookup(chain, dirs, level), "lookup")
    per, lnp = torch.from_numpy(c.per_map).to(DEV), torch.from_numpy(c.level_np).to(DEV)
    for T, d, dn, lv, ln in ((1, dirs, 0, level, 0), (3, per, 3 * P, lnp, P)):
        idx, wgt = Carved(T, 8 * P), Carved(T, P, 8)
        rc = lib.reni_envmap_lookup_taps(T, Lv, H, W, P, d.data_ptr(), dn, lv.data_ptr(), ln, 0.0, idx.ptr, wgt.ptr, _stream())
        assert rc == 0, lib.reni_last_error()
        torch.cuda.synchronize()
        table = ops.envmap_lookup_table(3, Lv, H, W, d, lv)
        wgt.check(table[0], f"tap weights T={T}")
        index = idx.values().view(torch.int32)
        assert bool((idx.buf[:4096] == 0x5A17C0DE).all()) and bool((idx.buf[4096 + idx.n:] == 0x5A17C0DE).all()), "tap indices: a stray store"
        assert int(index.min()) >= 0 and int(index.max()) < Lv * H * W
        keys, order = torch.sort(index, dim=1, stable=True)
        assert torch.equal(order, table[1])
        g = torch.randn(3, P, 3, generator=torch.Generator().manual_seed(T)).to(DEV)
        back = Carved(3, Lv, H, W, 3)
        rc = lib.reni_envmap_lookup_backward(3, Lv, H, W, P, g.data_ptr(), T, table[0].data_ptr(), table[1].data_ptr(),
                                             table[2].data_ptr(), back.ptr, _stream())
        assert rc == 0, lib.reni_last_error()
        back.check(ops.envmap_lookup_backward(g, Lv, H, W, d, lv), f"lookup backward T={T}")


# ---------------------------------------------------------------------------------------------- poisoned workspaces
@pytest.mark.parametrize("lobes", [ONE_KIND, NINE], ids=["one-kind", "three-kinds"])
@pytest.mark.parametrize("P,Q", [(33, 4097), (1, 6145)], ids=["33x4097", "1x6145"])
def test_split_paths_with_a_poisoned_workspace(P, Q, lobes):
    """Every byte of the workspace 0xFF (NaN floats), then 0x00, before the call: the partial sums of two and three chunks, the
    transpose's r and its (kind, split) slabs -- with one kind present only the first S of the 3 S slabs exist -- must all be
    written before they are read.  Finite, and the same bits under both fills."""
    N = 11
    c, src, in_dirs, w, out_dirs = _fwd(P, Q)
    s = src[:N].contiguous()
    for normalise in (True, False):
        runs = []
        for fill in (0xFF, 0x00):
            out = Carved(N, len(lobes), P, 3)
            assert c_lobe_convolve(s, in_dirs, w, out_dirs, lobes, normalise, E.SCALE, out.ptr, ws_fill=fill) > 256
            runs.append(out)
        assert bool(torch.isfinite(runs[0].values()).all()), (P, Q, normalise)
        runs[0].check(runs[1].values(), f"forward {(P, Q, normalise)}")
    runs = []
    for fill in (0xFF, 0x00):
        den = Carved(len(lobes), P)
        c_lobe_denominators(in_dirs, w, out_dirs, lobes, den.ptr, ws_fill=fill)
        runs.append(den)
    assert bool(torch.isfinite(runs[0].values()).all()) and bool((runs[0].values() > 0).all())
    runs[0].check(runs[1].values(), f"denominators {(P, Q)}")
    # the transpose at the exchanged shape
    c, g, in_dirs, w, out_dirs = _bwd(Q, P)
    idx = [NINE.index(l) for l in lobes] if lobes is NINE else [1, 2]  # phong(8), phong(64) of the nine
    gl = g[:N, idx].contiguous()
    den = ops.lobe_denominators(in_dirs, w, out_dirs, *_kp(lobes))
    for normalise in (True, False):
        runs = []
        for fill in (0xFF, 0x00):
            out = Carved(N, P, 3)  # (the transpose's Q is this shape's P)
            c_lobe_backward(gl, in_dirs, w, out_dirs, lobes, normalise, E.SCALE, den, out.ptr, ws_fill=fill)
            runs.append(out)
        assert bool(torch.isfinite(runs[0].values()).all()), (Q, P, normalise)
        runs[0].check(runs[1].values(), f"transpose {(Q, P, normalise)}")


# ---------------------------------------------------------------------------------------------- lookup
def _range_check(out, chain, level_clean, what):
    """out [P, 3] of one map is a mix of the texels of the levels it reads (up to the lerps' rounding), wherever it looks"""
    Lv = chain.shape[0]
    lv = np.clip(level_clean, 0, Lv - 1)
    l0 = np.floor(lv).astype(int)
    l1 = np.minimum(l0 + 1, Lv - 1)
    flat = chain.reshape(Lv, -1)
    lo, hi = np.minimum(flat.min(1)[l0], flat.min(1)[l1]), np.maximum(flat.max(1)[l0], flat.max(1)[l1])
    slack = 8 * 2.0 ** -24 * np.abs(chain).max()
    assert np.isfinite(out).all(), what
    assert (out >= lo[:, None] - slack).all() and (out <= hi[:, None] + slack).all(), what


@pytest.mark.parametrize("H,W,Lv,P", E.LOOKUP_CASES, ids=LOOKUP_IDS)
def test_lookup_edge_cases_match_the_oracle(H, W, Lv, P):
    """H = 1 (both rows of every cell are row 0, one of them seen from the far side), H = 2, W = 2 (half = 1: the far side is
    the other column), Lv = 1 (the level never mixes), P = 1, 255, 256, 257, 513; a NaN level reads level 0.  The random
    directions against np_lookup_chain within its bound, the oracle leaving out at most 0.03 of them; every direction, the
    poles and the zero vector among them, finite and inside the range of the levels it reads."""
    c = E.lookup_case(H, W, Lv, P)
    chain = torch.from_numpy(c.chain).to(DEV)
    shared, per = torch.from_numpy(c.dirs).to(DEV), torch.from_numpy(c.per_map).to(DEV)
    lv_p, lv_np = torch.from_numpy(c.level).to(DEV), torch.from_numpy(c.level_np).to(DEV)
    const = 0.5 * (Lv - 1) + 0.125
    worst = 0.0
    for dirs, dt in ((c.dirs, shared), (c.per_map, per)):
        for level, lt in ((np.zeros(P, np.float32), None), (np.full(P, const, np.float32), const), (c.level_clean, lv_p),
                          (c.level_np_clean, lv_np)):
            out = glossy.lookup(chain, dt, lt)
            assert out.shape == (3, P, 3)
            assert torch.equal(glossy.lookup(chain, dt, lt), out)
            o = _np(out)
            for n in range(3):
                d = dirs if dirs.ndim == 2 else dirs[n]
                lv = level if level.ndim == 1 else level[n]
                val, bound, keep = np_lookup_chain(c.chain[n], d, lv)
                keep = keep[:c.R]
                assert (~keep).mean() <= E.LEFT_OUT, (n, (~keep).mean())
                ratio = (np.abs(o[n] - val) / bound)[:c.R][keep]
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1.0).all(), (dirs.ndim, n, float(ratio.max()))
                _range_check(o[n], c.chain[n], lv, (H, W, Lv, P, n))
    print(f"lookup {H} x {W}, Lv {Lv}, P {P}: largest error / bound {worst:.3f}")
    # a strided view over planar memory is read in place; a map does not depend on the batch
    planar = chain.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)
    assert torch.equal(glossy.lookup(planar, shared, lv_p), glossy.lookup(chain, shared, lv_p))
    assert torch.equal(glossy.lookup(chain[1:2], per[1:2], lv_np[1:2])[0], glossy.lookup(chain, per, lv_np)[1])
    if Lv == 1:  # plain maps are a chain of one level, whatever the level says
        assert torch.equal(glossy.lookup(chain[:, 0], shared), glossy.lookup(chain, shared, lv_p))


@pytest.mark.parametrize("H,W,Lv,P", E.LOOKUP_CASES, ids=LOOKUP_IDS)
def test_lookup_taps_and_transpose_at_the_edge_cases(H, W, Lv, P):
    """The tap table IS the forward's matrix (the device's own, from one-hot chains; E <= 54), and the transpose gathers
    through it: with one table for the maps and with one a map."""
    c = E.lookup_case(H, W, Lv, P)
    Ee = Lv * H * W
    shared, per = torch.from_numpy(c.dirs).to(DEV), torch.from_numpy(c.per_map).to(DEV)
    lv_p, lv_np = torch.from_numpy(c.level).to(DEV), torch.from_numpy(c.level_np).to(DEV)
    g = torch.randn(3, P, 3, generator=torch.Generator().manual_seed(H + P)).to(DEV)
    g64 = _np(g)
    J = _device_J(Lv, H, W, shared, lv_p)  # [P, E]
    wgt, order, offsets = ops.envmap_lookup_table(3, Lv, H, W, shared, lv_p)
    assert wgt.shape == (1, P, 8) and order.shape == (1, 8 * P) and offsets.shape == (1, Ee + 1)
    wf, od, of = wgt.reshape(-1).double().cpu().numpy(), order[0].cpu().numpy(), offsets[0].cpu().numpy()
    assert of[0] == 0 and of[-1] == 8 * P and sorted(od.tolist()) == list(range(8 * P))
    S = np.zeros((P, Ee))
    for e in range(Ee):
        taps = od[of[e]:of[e + 1]]
        np.add.at(S[:, e], taps >> 3, wf[taps])
    assert np.abs(S - J).max() <= 2 * EPS32, np.abs(S - J).max()
    assert np.abs(S.sum(1) - 1).max() <= 8 * EPS32  # a direction's weights sum to 1
    out = ops.envmap_lookup_backward(g, Lv, H, W, shared, lv_p)  # T = 1
    assert out.shape == (3, Lv, H, W, 3)
    for n in range(3):
        lookup_transpose_check(out[n].reshape(Ee, 3).cpu().numpy(), J, g64[n], f"{H} x {W}, Lv {Lv}, P {P} shared, map {n}")
    assert torch.equal(ops.envmap_lookup_backward(g, Lv, H, W, shared, lv_p), out)
    assert torch.equal(ops.envmap_lookup_backward(g, Lv, H, W, table=(wgt, order, offsets)), out)
    assert torch.equal(ops.envmap_lookup_backward(g[2:3], Lv, H, W, shared, lv_p)[0], out[2])
    pm = ops.envmap_lookup_backward(g, Lv, H, W, per, lv_np)  # T = N
    assert ops.envmap_lookup_table(3, Lv, H, W, per, lv_np)[0].shape == (3, P, 8)
    for n in range(3):
        Jn = _device_J(Lv, H, W, per[n], lv_np[n])
        lookup_transpose_check(pm[n].reshape(Ee, 3).cpu().numpy(), Jn, g64[n], f"{H} x {W}, Lv {Lv}, P {P} per map, map {n}")
    assert torch.equal(ops.envmap_lookup_backward(g, Lv, H, W, per, lv_np), pm)
    # through autograd
    maps = torch.from_numpy(c.chain).to(DEV).requires_grad_()
    glossy.lookup(maps, shared, lv_p).backward(g)
    assert torch.equal(maps.grad, out)


def test_every_direction_on_one_texel_and_a_map_nobody_samples():
    """513 equal directions at a pixel centre of the 3 x 6 maps: one lane of the transpose sums all 513 taps.  Two calls give
    the same bits, the total meets lookup_transpose_check's rule ((8 + n_t) EPS32 (|J|^T |g|)), every texel and level nobody
    sampled is exactly 0, and so is the whole gradient of a map whose upstream is 0."""
    from reni_amd.utils import get_directions
    H, W, Lv, P = 3, 6, 3, 513
    Ee = Lv * H * W
    centre = get_directions(W)[0][7]  # row 1, column 1
    dirs = centre[None].repeat(P, 1).to(DEV)
    g = torch.randn(3, P, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    g[1] = 0.0
    for level in (1.0, 1.5):
        J = _device_J(Lv, H, W, dirs, level)
        nt = (J != 0).sum(0)
        assert nt.max() == P and (J[0] == J).all()
        out = ops.envmap_lookup_backward(g, Lv, H, W, dirs, level)
        assert torch.equal(ops.envmap_lookup_backward(g, Lv, H, W, dirs, level), out)
        for n in range(3):
            lookup_transpose_check(out[n].reshape(Ee, 3).cpu().numpy(), J, _np(g[n]), f"one texel, level {level}, map {n}")
        assert float(out[1].abs().max()) == 0.0  # nobody's gradient reaches this map
        assert float(out[:, 0].abs().max()) == 0.0  # nobody reads level 0
        if level == 1.0:
            assert float(out[:, 2].abs().max()) == 0.0 and int((out[0, 1] != 0).any(-1).sum()) <= 4
        # the forward at these directions is the same value P times
        chain = torch.rand(3, Lv, H, W, 3, generator=torch.Generator().manual_seed(6)).to(DEV)
        val = glossy.lookup(chain, dirs, level)
        assert torch.equal(val, val[:, :1].expand(-1, P, -1))
