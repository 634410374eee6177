"""Split-sum shading from a prefiltered chain, without a GPU: the float64 reference against itself (tests/split_sum_ref.py), the
approximation's quality against the exact float64 shader (tests/microfacet_ref.py), and the argument checks of the two entry
points (every check comes before any HIP call).

Recorded figures (float64, this file prints them):
  * DFG: the 128 x 128 midpoint rule against direct quadrature of DESIGN 4.4m's k and k f, relative to the direct A0, over the
    table's corners and the rows r in {0.1, 0.25, 1}: 3.62e-2 in the grazing column x = 0 (its worst: r = 0.1), 2.03e-2
    elsewhere (r = 0.25, next to the grazing column); the anchor A0(1, 1) = pi (1 - ln 2) to 2.49e-5.
  * a constant 32 x 64 map, 8 x 8 sphere: split-sum S0 / S1 against the exact sums, relative to the largest exact value:
    2.33e-3 / 7.01e-3 at roughness 0.7, 3.76e-4 / 1.69e-3 at roughness 1 (what is left is the exact shader's own texel sum).
  * a smooth 32 x 64 map, roughness 0.7: S0 0.300, S1 0.224, composed colours 8.58e-2 -- the n = v = r approximation itself.
"""
import ctypes
import math

import pytest
import torch

from reni_amd import _lib, glossy
from tests import microfacet_ref as GR
from tests import split_sum_ref as SR

F64 = torch.float64
# what float64 shows (see the docstring); the gates are 2 x (the rule's gap) and 1.5 x (the approximation's quality)
DFG_GAP_GRAZING, DFG_GAP_REST, ANCHOR_GAP = 3.625e-2, 2.028e-2, 2.49e-5
CONST_GAP = {0.7: (2.33e-3, 7.01e-3), 1.0: (3.76e-4, 1.69e-3)}
SMOOTH_GAP = (0.300, 0.224, 8.59e-2)


def test_entry_points_are_declared_exported_built_and_documented():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "reni_hip.h")).read()
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    lib = _lib.load()
    for n in ("reni_envmap_lookup_dquery", "reni_ggx_dfg"):
        assert re.search(r"^int " + n + r"\(", header, re.M) and n in _lib.EXPORTS and n in integration, n
        assert getattr(lib, n) is not None
    build = open(os.path.join(root, "reni_amd", "csrc", "build.sh")).read()
    assert " splitsum;" in build and "_build/splitsum.o" in build
    for name in ("sample", "ggx_dfg", "dfg_lookup", "shade_split_sum", "roughness_level", "PrefilteredRenderer"):
        assert callable(getattr(glossy, name)), name


def test_restated_lookup_matches_a_central_difference():
    """d out / d dirs and d out / d level of ``lookup_ref`` by autograd against a hand-written central difference, away from
    cell edges (the queries' fractional parts lie in [0.15, 0.85]; the step is 1e-6 of the direction's length)."""
    H, W, Lv, N, P = 8, 16, 3, 2, 300
    g = torch.Generator().manual_seed(3)
    maps = torch.randn(N, Lv, H, W, 3, generator=g, dtype=F64)
    d, lv = SR.make_queries(H, W, Lv, P, seed=11, N=N)
    up = torch.randn(N, P, 3, generator=g, dtype=F64)
    ad, al = SR.dquery_autograd(maps, d, lv, up)
    f = lambda dd, ll: (SR.lookup_ref(maps, dd, ll) * up).sum(-1)
    d64, l64 = d.double(), lv.double()
    h = 1e-6
    for k in range(3):
        e = torch.zeros(3, dtype=F64)
        e[k] = h
        cd = (f(d64 + e, l64) - f(d64 - e, l64)) / (2 * h)
        assert float((cd - ad[..., k]).abs().max()) <= 1e-6 * float(ad.abs().max())
    cl = (f(d64, l64 + h) - f(d64, l64 - h)) / (2 * h)
    assert float((cl - al).abs().max()) <= 1e-6 * float(al.abs().max())
    # the closed form the kernel evaluates is that derivative
    cd, cl = SR.dquery_closed(maps, d, lv, up, dtype=F64)
    assert float((cd - ad).abs().max()) <= 1e-12 * float(ad.abs().max()) and float((cl - al).abs().max()) <= 1e-12 * float(al.abs().max())


def test_reference_derivative_conventions():
    """zeros at a pole direction, for the zero vector, outside the level's closed range, for a NaN level and for Lv = 1; the right
    slope at an interior knot and the left slope at the top one"""
    g = torch.Generator().manual_seed(4)
    maps = torch.randn(1, 3, 4, 8, 3, generator=g, dtype=F64)
    d = torch.tensor([[0.0, 1.0, 0.0], [0.0, -2.0, 0.0], [0.0, 0.0, 0.0], [0.3, 0.2, -0.5]], dtype=F64)
    lv = torch.tensor([0.5, 1.0, 2.0, float("nan")], dtype=F64)
    up = torch.ones(1, 4, 3, dtype=F64)
    ad, al = SR.dquery_autograd(maps, d, lv, up)
    assert bool((ad[:3] == 0).all()) and bool((ad[3] != 0).any()) and bool(torch.isfinite(ad).all())
    v = lambda l: SR.lookup_ref(maps, d, float(l))[0].sum(-1)
    assert torch.allclose(al[1], (v(2) - v(1))[1], rtol=1e-12) and torch.allclose(al[2], (v(2) - v(1))[2], rtol=1e-12)
    assert float(al[3]) == 0.0
    _, out = SR.dquery_autograd(maps, d, torch.tensor([-0.5, 2.5, 0.5, 1.5], dtype=F64), up)
    assert float(out[0]) == 0.0 and float(out[1]) == 0.0 and float(out[2]) != 0.0
    _, one = SR.dquery_autograd(maps[:, :1], d, torch.tensor([0.0, 0.0, 0.0, 0.0], dtype=F64), up)
    assert bool((one == 0).all())


def test_dfg_rule_against_direct_quadrature_and_the_anchor():
    xi = [i / 31 for i in range(32)]
    graz = rest = 0.0
    for r in (0.1, 0.25, 1.0):   # r = 0.1 and r = 1 hold the table's four corners
        a0, a1 = SR.dfg_rule_at(xi, [r] * 32)
        for i, x in enumerate(xi):
            d0, d1 = SR.dfg_direct(x, r)
            gap = max(abs(float(a0[i]) - d0), abs(float(a1[i]) - d1)) / d0
            graz, rest = (max(graz, gap), rest) if i == 0 else (graz, max(rest, gap))
    anchor = math.pi * (1.0 - math.log(2.0))
    agap = abs(float(SR.dfg_rule_at([1.0], [1.0])[0]) - anchor) / anchor
    print(f"DFG rule against direct quadrature: grazing column {graz:.3e}, elsewhere {rest:.3e}; anchor {agap:.3e}")
    assert graz <= 2 * DFG_GAP_GRAZING and rest <= 2 * DFG_GAP_REST and agap <= 2 * ANCHOR_GAP
    assert abs(SR.dfg_direct(1.0, 1.0)[0] - anchor) <= 1e-9


def _quality(rough, const):
    W, Wo = 64, 32
    nrm, pos, cam = SR.sphere_gbuffer(8)
    dirs, sinw = SR.grid_dirs(W)
    L = torch.full((1, W * W // 2, 3), 0.7, dtype=F64) if const else SR.smooth_map(W)
    C = L * sinw[None, :, None]
    terms = SR.shade_split_sum_ref(C, W, nrm, pos, cam, 0.8, rough, 0.0, glossy.CHAIN_ROUGHNESS, Wo, terms=True)
    exact = GR.shade_terms_ggx_ref(nrm, pos, cam, dirs[None], C, torch.tensor(rough, dtype=F64) ** 2)
    q = lambda a, b: float((a - b).abs().max() / b.abs().max())
    bc = torch.tensor([0.8, 0.5, 0.3], dtype=F64)
    col, ecol = GR.compose_microfacet_ref(*terms, bc, 0.5), GR.compose_microfacet_ref(*exact, bc, 0.5)
    bg = (nrm == 0).all(-1)
    assert bool(bg.any()) and float(col[:, bg].abs().max()) == 0.0
    return q(terms[1], exact[1]), q(terms[2], exact[2]), q(col, ecol)


@pytest.mark.parametrize("rough", [0.7, 1.0])
def test_split_sum_is_the_exact_shader_on_a_constant_map_up_to_quadrature(rough):
    """The texel measure Q / (2 pi^2) and the normalised chain put A_m in the shader's units: S_m = L A_m Q / (2 pi^2)."""
    s0, s1, _ = _quality(rough, True)
    print(f"constant map, roughness {rough}: S0 {s0:.3e}, S1 {s1:.3e} of the largest exact value")
    assert s0 <= 1.5 * CONST_GAP[rough][0] and s1 <= 1.5 * CONST_GAP[rough][1]


def test_split_sum_quality_on_a_smooth_map():
    s0, s1, col = _quality(0.7, False)
    print(f"smooth map, roughness 0.7: S0 {s0:.3e}, S1 {s1:.3e}, colours {col:.3e} of the largest exact value")
    assert s0 <= 1.5 * SMOOTH_GAP[0] and s1 <= 1.5 * SMOOTH_GAP[1] and col <= 1.5 * SMOOTH_GAP[2]


def test_queries_land_in_one_cell_in_float32_and_float64():
    for (H, W) in ((4, 8), (8, 16)):
        for Lv in (1, 2, 3):
            for N in (None, 3):
                d, lv = SR.make_queries(H, W, Lv, 300, seed=H * 100 + Lv * 10 + (N or 1), N=N)
                assert SR.same_cells(d, lv, H, W, Lv)
                n = d.norm(dim=-1)
                assert float(n.min()) >= 0.29 and float(n.max()) <= 3.01


def test_dquery_argument_errors():
    lib = _lib.load()
    st = (ctypes.c_int64 * 5)(0, 0, 8, 1, 1)
    fn = lib.reni_envmap_lookup_dquery
    p = 256  # (a non-NULL pointer: no check dereferences it)

    def err(*a):
        rc = fn(*a, None)
        return rc, lib.reni_last_error().decode()

    ok = dict(N=1, Lv=2, H=4, W=8, P=5)
    base = lambda **k: [dict(ok, **k)[n] for n in ("N", "Lv", "H", "W", "P")]
    assert err(*base(P=0), p, st, p, 0, None, 0, 0.0, p, p, None) == (-1, "lookup: sizes must be >= 1")
    rc, msg = err(*base(W=7), p, st, p, 0, None, 0, 0.0, p, p, None)
    assert rc == -1 and msg.startswith("lookup: W must be even")
    rc, msg = err(*base(N=70000), p, st, p, 0, None, 0, 0.0, p, p, None)
    assert rc == -1 and msg.startswith("lookup: need N, Lv <= 65535")
    for args in ((None, st, p, 0, None, 0, 0.0, p, p, None), (p, None, p, 0, None, 0, 0.0, p, p, None),
                 (p, st, None, 0, None, 0, 0.0, p, p, None), (p, st, p, 0, None, 0, 0.0, None, p, None)):
        assert err(*base(), *args) == (-1, "lookup: NULL argument")
    neg = (ctypes.c_int64 * 5)(0, 0, -8, 1, 1)
    assert err(*base(), p, neg, p, 0, None, 0, 0.0, p, p, None) == (-1, "lookup: src strides must be >= 0")
    big = (ctypes.c_int64 * 5)(0, 0, 2 ** 31, 1, 1)
    rc, msg = err(*base(), p, big, p, 0, None, 0, 0.0, p, p, None)
    assert rc == -1 and "< 2^31" in msg
    rc, msg = err(*base(), p, st, p, 7, None, 0, 0.0, p, p, None)
    assert rc == -1 and msg.startswith("lookup: dirs_stride_n must be 0")
    rc, msg = err(*base(), p, st, p, 0, p, 3, 0.0, p, p, p)
    assert rc == -1 and msg.startswith("lookup: level_stride_n must be 0")
    assert err(*base(), p, st, p, 0, p, 0, 0.0, p, None, None) == (-1, "lookup dquery: d_dirs and d_level are both NULL")
    assert err(*base(), p, st, p, 0, None, 0, 0.0, p, None, p) == (-1, "lookup dquery: d_level needs a level array")


def test_ggx_dfg_argument_errors():
    lib = _lib.load()
    fn = lib.reni_ggx_dfg
    msg = lambda: lib.reni_last_error().decode()
    assert fn(1, 32, 0.1, 128, 128, 256, None) == -1 and "R_v, R_r" in msg()
    assert fn(32, 1025, 0.1, 128, 128, 256, None) == -1 and "R_v, R_r" in msg()
    assert fn(32, 32, 0.1, 0, 128, 256, None) == -1 and "M_u, M_phi" in msg()
    assert fn(32, 32, 0.1, 128, 1025, 256, None) == -1 and "M_u, M_phi" in msg()
    assert fn(1024, 1024, 0.1, 1024, 1024, 256, None) == -1 and "2^28" in msg()
    for bad in (0.0, 1.0, float("nan"), -0.5):
        assert fn(32, 32, bad, 128, 128, 256, None) == -1 and "r_min" in msg()
    assert fn(32, 32, 0.1, 128, 128, None, None) == -1 and msg() == "ggx dfg: NULL argument"


def test_cpu_tensors_fail_loudly():
    from reni_amd.envmap_shader import EnvironmentMap
    from reni_amd.utils import get_directions, get_sineweight
    maps = torch.rand(1, 2, 4, 8, 3, requires_grad=True)
    d = torch.randn(5, 3, requires_grad=True)
    with pytest.raises(_lib.RENILibraryError, match="no CPU fallback"):
        glossy.sample(maps, d, torch.rand(5))
    with pytest.raises(_lib.RENILibraryError, match="no CPU fallback"):
        glossy.sample(maps.detach(), d.detach(), 0.5)
    with pytest.raises(_lib.RENILibraryError, match="no CPU fallback"):
        glossy.ggx_dfg(device="cpu")
    env = EnvironmentMap(torch.rand(1, 128, 3), get_directions(16), get_sineweight(16))
    nrm, pos, cam = SR.sphere_gbuffer(4)
    with pytest.raises(_lib.RENILibraryError, match="no CPU fallback"):
        glossy.shade_split_sum(env, nrm, pos, cam, 0.8, 0.5, 0.0, out_width=8)
    with pytest.raises(ValueError, match="cannot require grad"):
        glossy.shade_split_sum(env, nrm, pos.clone().requires_grad_(True), cam, 0.8, 0.5, 0.0, out_width=8)
    with pytest.raises(ValueError, match="cannot require grad"):
        glossy.shade_split_sum(env, nrm, pos, cam.clone().requires_grad_(True), 0.8, 0.5, 0.0, out_width=8)
    with pytest.raises(ValueError, match="chain_roughness"):
        glossy.shade_split_sum(env, nrm, pos, cam, 0.8, 0.5, 0.0, chain_roughness=(0.5, 0.3), out_width=8)


def test_lookup_still_refuses_a_query_that_requires_grad():
    maps = torch.rand(1, 2, 4, 8, 3)
    with pytest.raises(ValueError, match="dirs requires grad"):
        glossy.lookup(maps, torch.randn(5, 3, requires_grad=True), 0.5)
    with pytest.raises(ValueError, match="level requires grad"):
        glossy.lookup(maps, torch.randn(5, 3), torch.rand(5, requires_grad=True))


def test_dfg_lookup_and_level_map_are_plain_torch():
    """bilinear read at the table's nodes and between them; d nv and d roughness by autograd; the level map's knots and sides"""
    t = torch.arange(2 * 3 * 4, dtype=F64).reshape(2, 3, 4)
    nv = torch.tensor([0.0, 1.0, 0.5, 1.0 / 3.0], dtype=F64, requires_grad=True)
    r = torch.tensor([0.1, 1.0, 0.55, 0.1], dtype=F64, requires_grad=True)
    A0, A1 = glossy.dfg_lookup(t, nv, r, 0.1)
    assert torch.allclose(A0.detach(), torch.tensor([0.0, 11.0, 5.5, 1.0], dtype=F64)) and torch.allclose(A1 - A0, torch.full((4,), 12.0, dtype=F64))
    gnv, gr = torch.autograd.grad(A0.sum(), (nv, r))
    assert torch.allclose(gnv, torch.full((4,), 3.0, dtype=F64)) and torch.allclose(gr, torch.full((4,), 4.0 * 2 / 0.9, dtype=F64))
    w0, w1 = SR.dfg_lookup_ref(t, nv, r, 0.1)
    assert torch.allclose(w0, A0) and torch.allclose(w1, A1)
    rho = (0.2, 0.4, 0.8, 1.0)
    x = torch.tensor([0.2, 0.3, 0.4, 0.8, 1.0], dtype=F64, requires_grad=True)
    lv = glossy.roughness_level(x, rho)
    assert torch.allclose(lv.detach(), torch.tensor([1.0, 1.5, 2.0, 3.0, 4.0], dtype=F64))
    (gx,) = torch.autograd.grad(lv.sum(), x)
    assert torch.allclose(gx, torch.tensor([5.0, 5.0, 2.5, 5.0, 5.0], dtype=F64))   # right of an interior knot, left of the last
    assert torch.allclose(SR.roughness_level_ref(x, rho), lv)
