"""CPU check of the glossy edge-shape case lists (tests/glossy_edge_cases.py): the lists hold the shapes they name, the library
splits them as the names say, every output row lies next to its texel, every float64 denominator is well away from zero,
and an fp32 restatement of each kernel -- the kernel's dot order, the lobes of reni_sphere.inc, every operation rounded once,
ONE sequential chain over the reduction -- stays within 0.75 of the budget tests/test_gpu_glossy_edges.py applies against
float64 (tests/test_glossy_cpu.py::lobe_tol; twice it for the normalised transpose).  A case that plain fp32 arithmetic
already pushed to its bound would make the GPU comparison say nothing about the kernel; it fails here first.

The lookup cases keep the bound of np_lookup_chain: the fp32 restatements of the lookup and of its transpose are checked
against it at the new sizes, and the oracle alone against its cap on the share of directions it leaves out."""
import numpy as np
import pytest

from reni_amd import _lib
from tests import glossy_edge_cases as E
from tests.test_glossy_cpu import emulate_lookup_fp32, lobe_tol, np_lookup_chain
from tests.test_glossy_grad_cpu import (emulate_lookup_backward_fp32, emulate_lookup_taps_fp32, host_J, lookup_transpose_check)
from tests.test_rotate_cpu import EPS32

SIXTEEN = ("phong16", "mix16")


def _fwd_splits(P, Q):
    """S of the forward at (P, Q), from the two workspace-size entry points"""
    lib = _lib.load()
    S = (int(lib.reni_lobe_workspace_bytes(1, P, Q, 1)) - 256) // (4 * 4 * P)
    assert int(lib.reni_lobe_workspace_bytes(1, P, Q, 1)) - 256 == S * 4 * P * 4
    assert int(lib.reni_lobe_denominators_workspace_bytes(P, Q, 1)) - 256 == S * P * 4
    return S


def _bwd_splits(P, Q):
    """S of the transpose at (P, Q): its workspace is r [P] rounded up to 256 bytes and 3 S slabs [3][Q]"""
    slabs = int(_lib.load().reni_lobe_backward_workspace_bytes(1, P, Q, 1)) - 256 - ((4 * P + 255) & ~255)
    assert slabs % (3 * 3 * Q * 4) == 0
    return slabs // (3 * 3 * Q * 4)


def test_case_lists_hold_the_shapes_they_name():
    assert len(E.FWD_SHAPES) == 16 and len(set(E.FWD_SHAPES)) == 16 and E.FWD_SHAPES[-1] == (1, 6145)
    for P in (1, 31, 33, 257):
        for Q in (1, 2, 3):
            assert (P, Q) in E.FWD_SHAPES and (Q, P) in E.BWD_SHAPES
    for shape in ((1, 4095), (1, 4096), (33, 4097)):
        assert shape in E.FWD_SHAPES and shape[::-1] in E.BWD_SHAPES
    assert E.BWD_SHAPES == tuple((Q, P) for P, Q in E.FWD_SHAPES)
    assert E.LB_N == (1, 10, 11, 21, 22) and E.NMAX == 22
    # with the column of ones: N = 10 is the last shape of CT = 1, N = 21 a column pair that is exactly full
    assert [3 * N + 1 for N in E.LB_N] == [4, 31, 34, 64, 67]
    assert [(3 * N + 1 <= 32, (3 * N + 1 + 63) // 64) for N in E.LB_N] == [(True, 1), (True, 1), (False, 1), (False, 1), (False, 2)]
    assert len(E.LOBE_SETS["nine"]) == 9 and len(E.PHONG16) == len(E.MIX16) == 16
    assert [l.param for l in E.PHONG16] == list(range(1, 17)) and {l.kind for l in E.PHONG16} == {"phong"}
    assert [l.kind for l in E.MIX16[:6]] == ["phong", "blinn", "ggx"] * 2
    assert E.SIXTEEN_FWD == (1, 4097) and E.SIXTEEN_BWD == (4097, 1)
    assert E.LOOKUP_CASES == ((1, 2, 1, 1), (1, 2, 3, 255), (2, 2, 1, 256), (2, 4, 2, 257), (3, 6, 3, 513))


def test_the_library_splits_the_shapes_as_named():
    """The restated split rule is the library's wherever the entry points show it, and gives the named chunks: none at 4095,
    two of 2048 at 4096, 2050 + 2047 at 4097, 2050 + 2050 + 2045 at 6145 -- for the transpose with the sizes exchanged."""
    for rows in (1, 3, 33, 257, 777, 2000):
        for red in (1, 2, 3, 2047, 4095, 4096, 4097, 5003, 6143, 6144, 6145, 8191, 8192, 180000):
            assert _fwd_splits(rows, red) == E.lb_split(rows, red)[0], (rows, red)
            assert _bwd_splits(red, rows) == E.lb_split(rows, red)[0], (rows, red)
    assert E.lb_split(1, 4095) == (1, 4096) and E.lb_split(1, 4096) == (2, 2048)
    assert E.lb_split(33, 4097) == (2, 2050) and 4097 - 2050 == 2047
    S, chunk = E.lb_split(1, 6145)
    assert (S, chunk, 6145 - (S - 1) * chunk) == (3, 2050, 2045) and _fwd_splits(1, 6145) == 3 and _bwd_splits(6145, 1) == 3
    assert E.lb_split(1, 4097) == (2, 2050)  # the sixteen-lobe shapes split too
    for P, Q in E.FWD_SHAPES:
        assert (_fwd_splits(P, Q) > 1) == (Q >= 4096) and (_bwd_splits(Q, P) > 1) == (Q >= 4096)
    assert E.edge_indices(6145, 3, 2050) == [6144, 0, 2049, 2050, 4099, 4100]
    assert E.edge_indices(3, 1, 4) == [2, 0] and E.edge_indices(1, 1, 2) == [0]


def _check_directions(c, reduction_edges_seen_by):
    d, o = c.in_dirs.double().numpy(), c.out_dirs.double().numpy()
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6 and np.abs(np.linalg.norm(o, axis=1) - 1).max() < 1e-6
    cos = (o * d[c.texel]).sum(1)
    assert cos.min() >= 0.999, (c.P, c.Q, cos.min())
    assert (c.den > 0).all() and (c.den >= 0.1 * c.den.max(axis=1, keepdims=True)).all(), (c.P, c.Q)
    w = c.w.double().numpy()
    assert w.min() >= 0.5 * 4 * np.pi / c.Q * (1 - 1e-6) and w.max() <= 4 * np.pi / c.Q * (1 + 1e-6)
    return cos


@pytest.mark.parametrize("P,Q", E.FWD_SHAPES)
def test_forward_cases_leave_room_for_the_kernel(P, Q):
    c = E.fwd_case(P, Q)
    assert (c.S, c.chunk) == E.lb_split(P, Q)
    _check_directions(c, "rows")
    edges = E.edge_indices(Q, c.S, c.chunk)
    assert c.texel[0] == Q - 1 and list(c.texel[:min(P, len(edges))]) == edges[:min(P, len(edges))]
    assert c.ind_texel == edges[:min(P, len(edges))] and len(c.ind_src) == len(c.ind_texel)
    if P >= Q:  # every texel is looked at when there are rows enough
        assert set(c.texel.tolist()) == set(range(Q))
    # an indicator map's result is one product in one channel: exactly zero in the others, and not negligible in its own
    for k, i in enumerate(c.ind_texel):
        assert (c.ind_ref[k][:, :, [ch for ch in range(3) if ch != k % 3]] == 0).all()
        assert (c.ind_ref[k, :, :, k % 3].max(axis=1) > 0.3 * E.SCALE * float(c.w[i])).all()
    print(f"forward ({P}, {Q}): fp32 restatement / budget: normalised {c.room[0]:.3f}, unnormalised {c.room[1]:.3f}, "
          f"indicator {c.room[2]:.3f} (draw {c.attempt})")
    assert max(c.room) <= E.ROOM


@pytest.mark.parametrize("P,Q", E.BWD_SHAPES)
def test_transposed_cases_leave_room_for_the_kernel(P, Q):
    c = E.bwd_case(P, Q)
    assert (c.S, c.chunk) == E.lb_split(Q, P)
    _check_directions(c, "texels")
    assert c.ind_row == E.edge_indices(P, c.S, c.chunk) and c.ind_row[0] == P - 1
    assert tuple(c.refN.shape) == (9, E.NMAX, Q, 3) and np.abs(c.refN).reshape(9 * E.NMAX, -1).max(axis=1).min() > 0
    print(f"transpose ({P}, {Q}): fp32 restatement / budget: normalised {c.room[0]:.3f}, unnormalised {c.room[1]:.3f}, "
          f"indicator {c.room[2]:.3f} / {c.room[3]:.3f} (draw {c.attempt})")
    assert max(c.room) <= E.ROOM


@pytest.mark.parametrize("name", SIXTEEN)
def test_sixteen_lobe_cases_leave_room_for_the_kernel(name):
    f, b = E.fwd_case(*E.SIXTEEN_FWD, name), E.bwd_case(*E.SIXTEEN_BWD, name)
    assert len(f.lobes) == len(b.lobes) == 16 and f.S == b.S == 2
    _check_directions(f, "rows")
    _check_directions(b, "texels")
    print(f"{name}: forward {max(f.room):.3f}, transpose {max(b.room):.3f} of the budgets")
    assert max(f.room) <= E.ROOM and max(b.room) <= E.ROOM


def test_restatement_notices_a_dropped_tail_and_a_short_finish():
    """The margins mean something: without its last texel, or without its last chunk, the float64 result of a case is off by
    many budgets (so a kernel that dropped either cannot hide inside one)."""
    for P, Q in ((1, 3), (33, 4097), (1, 6145)):
        c = E.fwd_case(P, Q)
        src, d, w, o = (x.numpy() for x in (c.src, c.in_dirs, c.w, c.out_dirs))
        for cut in (Q - 1, (c.S - 1) * c.chunk):
            num, _ = E.forward_ref(src[:, :cut], d[:cut], w[:cut], o, c.lobes)
            assert E.worst_ratio(E.SCALE * num, E.SCALE * c.num, c.lobes) > 10, (P, Q, cut)


# ---------------------------------------------------------------------------------------------- lookup
@pytest.mark.parametrize("H,W,Lv,P", E.LOOKUP_CASES)
def test_lookup_cases_keep_the_bound_and_the_cap(H, W, Lv, P):
    c = E.lookup_case(H, W, Lv, P)
    assert c.dirs.shape == (P, 3) and c.per_map.shape == (3, P, 3) and c.level.shape == (P,) and c.level_np.shape == (3, P)
    assert c.R == (P if P == 1 else P - len(E.LOOKUP_SPECIAL))
    if P > 1:
        assert np.isnan(c.level).sum() == 2 and np.isnan(c.level_np).sum() == 1 and (c.level == Lv - 1.0).sum() >= 2
        assert (c.dirs[c.R:] == E.LOOKUP_SPECIAL).all()
    lv = c.level[~np.isnan(c.level)]
    assert lv.min() >= -0.5 and lv.max() <= Lv - 0.5 and (lv == np.floor(lv)).any()
    worst = 0.0
    for n, (dirs, level) in enumerate([(c.dirs, c.level_clean)] + [(c.per_map[m], c.level_np_clean[m]) for m in range(3)]):
        val, bound, keep = np_lookup_chain(c.chain[n % 3], dirs, level)
        assert (~keep[:c.R]).mean() <= E.LEFT_OUT, (n, (~keep[:c.R]).mean())  # the oracle alone, at these sizes
        got = emulate_lookup_fp32(c.chain[n % 3], dirs, level).astype(np.float64)
        assert np.isfinite(got).all()
        ratio = (np.abs(got - val) / bound)[:c.R][keep[:c.R]].max()
        worst = max(worst, float(ratio))
        assert ratio <= 1.0, (n, ratio)
    print(f"lookup emulation {H} x {W}, Lv {Lv}, P {P}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("H,W,Lv,P", E.LOOKUP_CASES)
def test_lookup_transpose_restatement_meets_the_bound_at_the_edge_sizes(H, W, Lv, P):
    c = E.lookup_case(H, W, Lv, P)
    idx, wgt = emulate_lookup_taps_fp32(Lv, H, W, c.dirs, c.level_clean)
    assert idx.min() >= 0 and idx.max() < Lv * H * W
    J = host_J(Lv, H, W, c.dirs, c.level_clean)
    S = np.zeros_like(J, dtype=np.float64)
    np.add.at(S, (np.repeat(np.arange(P), 8), idx.reshape(-1)), wgt.reshape(-1).astype(np.float64))
    assert np.abs(S - J).max() <= 2 * EPS32
    g = np.random.default_rng(H + P).standard_normal((P, 3)).astype(np.float32)
    lookup_transpose_check(emulate_lookup_backward_fp32(g, idx, wgt, Lv * H * W), J, g, f"{H} x {W}, Lv {Lv}, P {P} (host)")


def test_tolerances_are_those_of_the_existing_tests():
    assert lobe_tol(("phong", 500.0)) == 1e-5 + 500 * 2.0 ** -22 and E.SCALE == 0.75 and E.ROOM == 0.75 and E.LEFT_OUT == 0.03
