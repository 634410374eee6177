"""GPU tests of split-sum shading from a prefiltered chain (reni_envmap_lookup_dquery, reni_ggx_dfg; glossy.sample / ggx_dfg /
shade_split_sum / PrefilteredRenderer(materials=)) against the float64 reference tests/split_sum_ref.py, whose autograd is the
reference for every gradient.

Tolerances.  The query's derivative is held, element by element, to max(K EPS32 sum |terms|, 2e-5 largest reference value) with
EPS32 = 2^-23 and K four times the worst ratio of the closed form evaluated in float32 torch on the CPU over the same cases
(``split_sum_ref.dquery_closed``) -- never the device's output.  The DFG table is held the same way against the float64 rule
(its terms are positive: the sum of their absolute values is the value).  The composed paths (shade_split_sum, the renderer) are
held, quantity by quantity, to max(4 x the error of the reference itself evaluated in float32 on the CPU, 2e-5 x the largest
reference value).  Measured ratios: DESIGN 4.4n.
"""
import functools
import types

import pytest
import torch

from tests import split_sum_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
SIZES = [(4, 8), (8, 16)]
P = 300  # crosses a 256-lane block
SHAPES = [(H, W, Lv) for (H, W) in SIZES for Lv in (1, 2, 3)]
VARIANTS = [(N, per_d, per_l) for N in (1, 3) for per_d in (False, True) for per_l in (False, True)]


@functools.lru_cache(maxsize=None)
def _case(H, W, Lv, N, per_d, per_l):
    g = torch.Generator().manual_seed(1000 * H + 100 * Lv + 10 * N + 2 * per_d + per_l)
    maps = torch.randn(N, Lv, H, W, 3, generator=g)
    d, lv = SR.make_queries(H, W, Lv, P, seed=7 * H + Lv + N, N=N)
    d = d if per_d else d[0]
    lv = lv if per_l else lv[0]
    up = torch.randn(N, P, 3, generator=g)
    ref = SR.dquery_autograd(maps, d, lv, up)
    scale = SR.dquery_scales(maps, d, lv, up)
    return types.SimpleNamespace(maps=maps, d=d, lv=lv, up=up, ref=ref, scale=scale)


@functools.lru_cache(maxsize=None)
def _K():
    """(K of d_dirs, K of d_level): 4 x the float32 CPU emulation's worst ratio over every case, at least 4"""
    kd = kl = 1.0
    for (H, W, Lv) in SHAPES:
        for v in VARIANTS:
            c = _case(H, W, Lv, *v)
            ed, el = SR.dquery_closed(c.maps, c.d, c.lv, c.up, dtype=torch.float32)
            kd = max(kd, SR.error_ratio(ed, c.ref[0], c.scale[0]))
            kl = max(kl, SR.error_ratio(el, c.ref[1], c.scale[1]))
    return 4.0 * kd, 4.0 * kl


def _sample_grads(c, need_d=True, need_l=True, maps=None):
    from reni_amd import glossy
    maps = c.maps.to(DEV) if maps is None else maps
    d = c.d.to(DEV).requires_grad_(need_d)
    lv = c.lv.to(DEV).requires_grad_(need_l)
    out = glossy.sample(maps, d, lv)
    (out * c.up.to(DEV)[: out.shape[0]]).sum().backward()
    return out.detach(), d.grad, lv.grad


@pytest.mark.parametrize("H,W,Lv", SHAPES)
def test_sample_forward_is_lookup_and_query_gradients_match_float64(H, W, Lv):
    from reni_amd import glossy
    Kd, Kl = _K()
    worst_d = worst_l = 0.0
    for v in VARIANTS:
        c = _case(H, W, Lv, *v)
        assert SR.same_cells(c.d, c.lv, H, W, Lv)
        out, gd, gl = _sample_grads(c)
        assert torch.equal(out, glossy.lookup(c.maps.to(DEV), c.d.to(DEV), c.lv.to(DEV)))
        assert gd.shape == c.d.shape and gl.shape == c.lv.shape
        for got, ref, scale, K in ((gd, c.ref[0], c.scale[0], Kd), (gl, c.ref[1], c.scale[1], Kl)):
            err = (got.double().cpu() - ref).abs()
            assert bool(torch.isfinite(got).all()) and bool((err <= SR.bound(ref, scale, K)).all()), (v, float(err.max()))
        worst_d = max(worst_d, SR.error_ratio(gd, c.ref[0], c.scale[0]))
        worst_l = max(worst_l, SR.error_ratio(gl, c.ref[1], c.scale[1]))
        assert float(c.ref[0].abs().max()) > 0 and (Lv == 1 or float(c.ref[1].abs().max()) > 0)
        if Lv == 1:
            assert bool((gl == 0).all())
    print(f"dquery {H}x{W} Lv {Lv}: device ratio d_dirs {worst_d:.2f} (K {Kd:.1f}), d_level {worst_l:.2f} (K {Kl:.1f})")


def test_exact_zeros_and_the_knot_rule():
    from reni_amd import glossy, ops
    g = torch.Generator().manual_seed(5)
    maps = torch.randn(2, 3, 4, 8, 3, generator=g).to(DEV)
    d = torch.tensor([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 0.0], [0.3, 0.2, -0.5], [0.3, 0.2, -0.5], [0.3, 0.2, -0.5],
                      [0.3, 0.2, -0.5], [-0.4, 0.1, 0.2]], device=DEV)
    lv = torch.tensor([0.5, 0.5, 0.5, float("nan"), -0.5, 2.5, 1.0, 2.0], device=DEV)
    up = torch.randn(2, 8, 3, generator=g).to(DEV)
    gd, gl = ops.envmap_lookup_dquery(maps, d, lv, up, need_dirs=True, need_level=True)
    assert bool(torch.isfinite(gd).all()) and bool(torch.isfinite(gl).all())
    assert bool((gd[:3] == 0).all()) and bool((gd[3:] != 0).any(-1).all())
    assert bool((gl[3:6] == 0).all()) and bool((gl[[0, 1, 2, 6, 7]] != 0).all())
    # the knot rule: the slope to the right of level 1, to the left of level Lv - 1 = 2 -- in both cases v(2) - v(1)
    v1, v2 = glossy.lookup(maps, d, 1.0).double(), glossy.lookup(maps, d, 2.0).double()
    want = ((v2 - v1) * up.double()).sum(-1).sum(0)
    a1, a2 = glossy.lookup(maps.abs(), d, 1.0).double(), glossy.lookup(maps.abs(), d, 2.0).double()   # the sums of |terms|
    tol = 16 * SR.EPS32 * ((a2 + a1) * up.double().abs()).sum(-1).sum(0)
    assert bool(((gl.double() - want).abs() <= tol)[6:].all())
    # Lv = 1: no slope at all
    _, g1 = ops.envmap_lookup_dquery(maps[:, :1], d, torch.zeros(8, device=DEV), up, need_dirs=False, need_level=True)
    assert bool((g1 == 0).all())
    # per-map operands take the same zeros
    gdn, gln = ops.envmap_lookup_dquery(maps, d.expand(2, -1, -1).contiguous(), lv.expand(2, -1).contiguous(), up, True, True)
    assert bool((gdn[:, :3] == 0).all()) and bool((gln[:, 3:6] == 0).all()) and bool(torch.isfinite(gdn).all())


@pytest.mark.parametrize("per_d,per_l", [(False, False), (True, False), (False, True), (True, True)])
def test_bit_properties(per_d, per_l):
    """asking for d_dirs does not move d_level's bits (and the other way round); two calls give equal bits; with per-map operands
    map n's rows are the same alone and in the batch"""
    from reni_amd import ops
    c = _case(8, 16, 3, 3, per_d, per_l)
    maps, d, lv, up = c.maps.to(DEV), c.d.to(DEV), c.lv.to(DEV), c.up.to(DEV)
    gd, gl = ops.envmap_lookup_dquery(maps, d, lv, up, True, True)
    gd2, gl2 = ops.envmap_lookup_dquery(maps, d, lv, up, True, True)
    assert torch.equal(gd, gd2) and torch.equal(gl, gl2)
    only_d, none_l = ops.envmap_lookup_dquery(maps, d, lv, up, True, False)
    none_d, only_l = ops.envmap_lookup_dquery(maps, d, lv, up, False, True)
    assert none_l is None and none_d is None and torch.equal(only_d, gd) and torch.equal(only_l, gl)
    for n in range(3):
        dn, ln = (d[n] if per_d else d), (lv[n] if per_l else lv)
        a, b = ops.envmap_lookup_dquery(maps[n:n + 1], dn, ln, up[n:n + 1], True, True)
        if per_d:
            assert torch.equal(a, gd[n])
        if per_l:
            assert torch.equal(b, gl[n])


def test_dquery_runs_only_when_asked_for(monkeypatch):
    from reni_amd import glossy, ops
    c = _case(4, 8, 2, 3, False, False)
    calls, real = [], ops.envmap_lookup_dquery
    monkeypatch.setattr(ops, "envmap_lookup_dquery",
                        lambda *a, **k: calls.append((k.get("need_dirs"), k.get("need_level"))) or real(*a, **k))
    maps = c.maps.to(DEV).requires_grad_(True)
    glossy.sample(maps, c.d.to(DEV), c.lv.to(DEV)).sum().backward()   # the maps alone: the existing gather, no dquery call
    assert calls == [] and float(maps.grad.abs().max()) > 0
    assert torch.equal(glossy.sample(c.maps.to(DEV), c.d.to(DEV), c.lv.to(DEV)), glossy.lookup(c.maps.to(DEV), c.d.to(DEV), c.lv.to(DEV)))
    assert calls == []
    _sample_grads(c, need_d=True, need_l=False)
    assert calls == [(True, False)]
    _sample_grads(c, need_d=False, need_l=True)
    assert calls == [(True, False), (False, True)]
    _, gd, gl = _sample_grads(c, maps=maps)
    assert calls[-1] == (True, True) and len(calls) == 3
    want_d, want_l = real(c.maps.to(DEV), c.d.to(DEV), c.lv.to(DEV), c.up.to(DEV), True, True)
    assert torch.equal(gd, want_d) and torch.equal(gl, want_l)


# ------------------------------------------------------------------------------------------------- the DFG table
@functools.lru_cache(maxsize=None)
def _dfg_refs(Rv, Rr, M):
    """(the float64 table, its float32 evaluation on the CPU, the scales of its entries)"""
    return (SR.dfg_table_ref(Rv, Rr, 0.1, M, M, F64), SR.dfg_table_ref(Rv, Rr, 0.1, M, M, torch.float32),
            SR.dfg_table_ref(Rv, Rr, 0.1, M, M, F64, scale=True))


@pytest.mark.parametrize("Rv,Rr,M", [(32, 32, 128), (2, 2, 128), (5, 3, 8)])
def test_ggx_dfg_matches_the_float64_rule(Rv, Rr, M):
    from reni_amd import ops
    K = 4.0
    for shape in ((32, 32, 128), (2, 2, 128), (5, 3, 8)):
        r64, r32, sc = _dfg_refs(*shape)
        K = max(K, 4.0 * SR.error_ratio(r32, r64, sc))
    ref, _, scale = _dfg_refs(Rv, Rr, M)
    got = ops.ggx_dfg(Rv, Rr, 0.1, M, M, DEV)
    assert got.shape == (2, Rr, Rv) and torch.equal(got, ops.ggx_dfg(Rv, Rr, 0.1, M, M, DEV))
    err = (got.double().cpu() - ref).abs()
    print(f"ggx_dfg {Rv}x{Rr} M {M}: device ratio {SR.error_ratio(got, ref, scale):.2f} (K {K:.1f})")
    assert bool((err <= SR.bound(ref, scale, K)).all())


def test_ggx_dfg_is_cached_and_anchored():
    import math
    from reni_amd import glossy
    t = glossy.ggx_dfg(32, 0.1, DEV)
    assert t is glossy.ggx_dfg(32, 0.1, DEV) and t.shape == (2, 32, 32)
    assert abs(float(t[0, 31, 31]) - math.pi * (1 - math.log(2))) <= 2 * 2.49e-5 * 0.964 + 1e-5


# ------------------------------------------------------------------------------------------------- shade_split_sum
RHO = (0.2, 0.45, 1.0)
QUANT = ("colours", "dC", "dn", "d_roughness", "d_base_color", "d_metallic")


def _envmap(C):
    """an EnvironmentMap whose (premultiplied) map IS the leaf C [B, Q, 3] on the device"""
    from reni_amd.envmap_shader import EnvironmentMap
    from reni_amd.utils import get_directions
    W = int(round((2 * C.shape[1]) ** 0.5))
    D = get_directions(W).to(DEV)
    env = EnvironmentMap(environment_map=C, directions=D.expand(C.shape[0], -1, -1), sineweight=torch.ones(1, 1, 1, device=DEV))
    env.environment_map = C
    return env


def _ref_eval(p, dtype):
    C = p.C.to(dtype).clone().requires_grad_(True)
    n = p.nrm.to(dtype).clone().requires_grad_(True)
    r = p.rough.to(dtype).clone().requires_grad_(True)
    bc = p.base_color.to(dtype).clone().requires_grad_(True)
    me = p.metallic.to(dtype).clone().requires_grad_(True)
    col = SR.shade_split_sum_ref(C, p.W, n, p.pos, p.cam, bc, r, me, p.rho, p.Wo, table=SR.dfg_table(p.dfg_size, 0.1), dtype=dtype)
    grads = torch.autograd.grad((col * p.w.to(dtype)).sum(), (C, n, r, bc, me))
    return dict(zip(QUANT, [col.detach()] + [x.detach() for x in grads]))


def _held(p, got):
    """every quantity within max(4 x the float32 reference's error, 2e-5 x the largest float64 value)"""
    r64, r32 = _ref_eval(p, F64), _ref_eval(p, torch.float32)
    for k in QUANT:
        ref = r64[k]
        tol = max(4.0 * float((r32[k].double() - ref).abs().max()), SR.FLOOR * float(ref.abs().max()))
        err = float((got[k].double().cpu() - ref).abs().max())
        print(f"{p.name} {k}: error {err:.3e}, bound {tol:.3e}, largest {float(ref.abs().max()):.3e}")
        assert float(ref.abs().max()) > 0 and bool(torch.isfinite(got[k]).all()) and err <= tol, k
    return r64


@functools.lru_cache(maxsize=None)
def _sphere_problem():
    nrm, pos, cam = SR.sphere_gbuffer(8)
    NP = nrm.shape[0]
    g = torch.Generator().manual_seed(31)
    W, B = 32, 2
    _, sinw = SR.grid_dirs(W, torch.float32)
    C = torch.rand(B, W * W // 2, 3, generator=g) * 4.0 * sinw[None, :, None]
    return types.SimpleNamespace(name="sphere 8x8", W=W, Wo=16, rho=RHO, dfg_size=8, nrm=nrm, pos=pos, cam=cam, C=C,
                                 rough=0.15 + 0.85 * torch.rand(NP, generator=g), base_color=torch.rand(NP, 3, generator=g),
                                 metallic=torch.rand(NP, generator=g), w=torch.randn(B, NP, 3, generator=g), bg=(nrm == 0).all(-1))


def test_shade_split_sum_matches_float64_on_a_sphere_with_background():
    from reni_amd import glossy
    p = _sphere_problem()
    C = p.C.to(DEV).requires_grad_(True)
    n = p.nrm.to(DEV).requires_grad_(True)
    r, bc, me = (x.to(DEV).requires_grad_(True) for x in (p.rough, p.base_color, p.metallic))
    col = glossy.shade_split_sum(_envmap(C), n, p.pos.to(DEV), p.cam, bc, r, me, chain_roughness=p.rho, out_width=p.Wo,
                                 dfg_size=p.dfg_size)
    (col * p.w.to(DEV)).sum().backward()
    got = dict(zip(QUANT, (col.detach(), C.grad, n.grad, r.grad, bc.grad, me.grad)))
    _held(p, got)
    bg = p.bg.to(DEV)
    assert bool(bg.any()) and bool((~bg).any())
    assert float(col.detach()[:, bg].abs().max()) == 0.0
    for k in ("dn", "d_roughness", "d_base_color", "d_metallic"):
        assert float(got[k][bg].abs().max()) == 0.0, k
    col2 = glossy.shade_split_sum(_envmap(C.detach()), p.nrm.to(DEV), p.pos.to(DEV), p.cam, bc.detach(), r.detach(), me.detach(),
                                  chain_roughness=p.rho, out_width=p.Wo, dfg_size=p.dfg_size)
    assert torch.equal(col2, col.detach())


@pytest.mark.parametrize("rough", [0.7, 1.0])
def test_constant_map_gives_the_exact_shaders_specular_sums(rough):
    """base colour 1 / 0 with metallic 1 make the colours S0 / S1; the exact sums are shade_terms_ggx's.  Within 1.5 x the gap
    float64 shows (tests/test_split_sum_cpu.py: the exact shader's own texel sum)."""
    from reni_amd import glossy
    from reni_amd.envmap_shader import shade_terms_ggx
    from tests.test_split_sum_cpu import CONST_GAP
    W = 64
    nrm, pos, cam = SR.sphere_gbuffer(8)
    _, sinw = SR.grid_dirs(W, torch.float32)
    C = (0.7 * sinw[None, :, None].expand(1, -1, 3)).contiguous().to(DEV)
    env = _envmap(C)
    _, e0, e1 = shade_terms_ggx(nrm.to(DEV), pos.to(DEV), cam, env, rough * rough)
    s = [glossy.shade_split_sum(env, nrm.to(DEV), pos.to(DEV), cam, bc, rough, 1.0, out_width=32) for bc in (1.0, 0.0)]
    for m, (got, ex) in enumerate(zip(s, (e0, e1))):
        gap = float((got - ex).abs().max() / ex.abs().max())
        print(f"constant map, roughness {rough}: S{m} {gap:.3e} of the largest exact value")
        assert gap <= 1.5 * CONST_GAP[rough][m]


# ------------------------------------------------------------------------------------------------- the renderer
def test_renderer_with_spatial_microfacet_materials_matches_float64():
    from reni_amd.envmap_shader import GBuffer, MicrofacetMaterials
    from reni_amd.glossy import PrefilteredRenderer
    p = _sphere_problem()
    mat = MicrofacetMaterials(p.base_color, p.rough, p.metallic, learn=("base_color", "roughness", "metallic")).to(DEV)
    n = p.nrm.to(DEV).requires_grad_(True)
    r = PrefilteredRenderer(GBuffer(n, p.pos.to(DEV), p.cam, 8), materials=mat, chain_roughness=p.rho, out_width=p.Wo, dfg_size=p.dfg_size)
    C = p.C.to(DEV).requires_grad_(True)
    col, normals = r(envmap=_envmap(C))
    assert col.shape == (2, 8, 8, 3) and normals.shape == (2, 8, 8, 3)
    assert torch.equal(normals[0].reshape(-1, 3), torch.nn.functional.normalize(n.detach(), p=2, dim=-1, eps=1e-6))
    (col.reshape(2, -1, 3) * p.w.to(DEV)).sum().backward()
    _held(p, dict(zip(QUANT, (col.detach().reshape(2, -1, 3), C.grad, n.grad, mat.roughness.grad, mat.base_color.grad, mat.metallic.grad))))


def test_renderer_with_textured_microfacet_materials_matches_float64():
    """The UV sphere at 16 x 16 with base colour, roughness, metallic and normal textures: from the device's own per-pixel values
    and bent normals (the fetch has its own tests) the colours are the float64 split-sum's and the gradients of the base
    colour, roughness and metallic textures are the float64 per-pixel gradients gathered through the device's taps; the
    returned normals stay the geometry's and every texture, the normal texture included, gets a finite, non-zero gradient."""
    from reni_amd.glossy import PrefilteredRenderer
    from reni_amd.mesh import FoVPerspectiveCameras, MeshRasterizer, RasterizationSettings, look_at_view_transform
    from reni_amd.textures import TexturedMicrofacetMaterials
    from tests.test_gpu_microfacet import _bumps, _sphere_mesh
    mesh = _sphere_mesh()
    S, B, W = 16, 2, 32
    g = torch.Generator().manual_seed(41)
    tex = {"base_color": 0.2 + 0.6 * torch.rand(16, 32, 3, generator=g), "roughness": 0.2 + 0.7 * torch.rand(8, 16, generator=g),
           "metallic": torch.rand(4, 8, generator=g), "normal": _bumps(8, 16, 0.4, 42)}
    mat = TexturedMicrofacetMaterials(tex["base_color"], tex["roughness"], tex["metallic"], normal=tex["normal"], learn=tuple(tex)).to(DEV)
    R, T = look_at_view_transform(2.7, 10.0, 25.0, device=DEV)
    ras = MeshRasterizer(cameras=FoVPerspectiveCameras(device=DEV), raster_settings=RasterizationSettings(image_size=S))
    r = PrefilteredRenderer(ras, materials=mat, shader_cameras=FoVPerspectiveCameras(R=R, T=T, device=DEV), chain_roughness=RHO,
                            out_width=16, dfg_size=8)
    _, sinw = SR.grid_dirs(W, torch.float32)
    C = (torch.rand(B, W * W // 2, 3, generator=g) * 4.0 * sinw[None, :, None]).to(DEV)
    col, normals = r(meshes_world=mesh, R=R, T=T, envmap=_envmap(C))
    wcol = torch.randn(B, S, S, 3, generator=g)
    (col * wcol.to(DEV)).sum().backward()
    _, nrm, pos = ras.gbuffer(mesh, R, T)
    assert torch.equal(normals[0].reshape(-1, 3), torch.nn.functional.normalize(nrm, p=2, dim=-1, eps=1e-6))
    with torch.no_grad():
        bc, ro, me = (v.cpu() for v in mat.values(ras, mesh, R, T))
        bent = mat.shading_normals(ras, mesh, R, T, nrm).cpu()
    assert not torch.equal(bent, nrm.cpu())
    table = SR.dfg_table(8, 0.1)
    args = (32, bent, pos.cpu(), r.camera_center, bc, ro, me, RHO, 16)
    ref = SR.shade_split_sum_ref(C.cpu(), *args, table=table)
    r32 = SR.shade_split_sum_ref(C.cpu(), *args, table=table, dtype=torch.float32)
    tol = max(4.0 * float((r32.double() - ref).abs().max()), SR.FLOOR * float(ref.abs().max()))
    err = float((col.detach().reshape(B, -1, 3).double().cpu() - ref).abs().max())
    print(f"textured renderer colours: error {err:.3e}, bound {tol:.3e}, largest {float(ref.abs().max()):.3e}")
    assert err <= tol and float(ref.abs().max()) > 0
    for k in tex:
        gk = getattr(mat, k).grad
        assert gk is not None and bool(torch.isfinite(gk).all()) and float(gk.abs().max()) > 0, k
    # the value textures' gradients: the float64 per-pixel gradient pushed through the device's taps in float64; a texel is
    # held to the per-pixel bound (4 x the float32 reference's error, floored) times its coverage plus the gather's rounding
    # (64 2^-23 of the sum of the absolute values of its terms)
    from tests.test_gpu_microfacet import _transpose_lookup
    per_pixel = {}
    for dt in (F64, torch.float32):
        leaves = [x.to(dt).clone().requires_grad_(True) for x in (bc, ro, me)]
        out = SR.shade_split_sum_ref(C.cpu(), 32, bent, pos.cpu(), r.camera_center, *leaves, RHO, 16, table=table, dtype=dt)
        per_pixel[dt] = torch.autograd.grad((out * wcol.reshape(B, -1, 3).to(dt)).sum(), leaves)
    for i, k in enumerate(mat.NAMES):
        g64, g32 = per_pixel[F64][i], per_pixel[torch.float32][i].double()
        g64, g32 = (g64, g32) if g64.dim() == 2 else (g64[:, None], g32[:, None])
        tol_p = max(4.0 * float((g32 - g64).abs().max()), SR.FLOOR * float(g64.abs().max()))
        taps = ras.texture_taps(mesh, R, T, size=tuple(tex[k].shape[:2]))
        want = _transpose_lookup(tex[k], taps, g64)
        cover = _transpose_lookup(tex[k], taps, torch.full_like(g64, tol_p)) + 64 * SR.EPS32 * _transpose_lookup(tex[k], taps, g64.abs())
        got = getattr(mat, k).grad.cpu().double()
        over = float(((got - want).abs() - cover).max())
        print(f"textured renderer d {k}: worst error {float((got - want).abs().max()):.3e}, largest {float(want.abs().max()):.3e}")
        assert float(want.abs().max()) > 0 and over <= 0.0, k


def test_renderer_without_materials_keeps_its_bits():
    from reni_amd.envmap_shader import GBuffer
    from reni_amd.glossy import PrefilteredRenderer, shade_prefiltered
    p = _sphere_problem()
    env = _envmap(p.C.to(DEV))
    gb = GBuffer(p.nrm.to(DEV), p.pos.to(DEV), p.cam, 8)
    col, _ = PrefilteredRenderer(gb, 0.6, shininess=40.0, out_width=16)(envmap=env)
    want = shade_prefiltered(env, p.nrm.to(DEV), p.pos.to(DEV), p.cam, 40.0, 0.6, 0.4, 16)
    assert torch.equal(col.reshape(2, -1, 3), want) and float(want.abs().max()) > 0
    with pytest.raises(ValueError, match="kd is required"):
        PrefilteredRenderer(gb)
    with pytest.raises(ValueError, match="materials must be"):
        PrefilteredRenderer(gb, materials=object())


def test_roughness_fit_through_the_prefiltered_renderer():
    """15 Adam steps on a per-pixel roughness (0.7 towards a target rendered at 0.3) on a 16 x 16 sphere with bent normals under a
    16 x 32 map: the loss falls below half its start.  The learning rate is the one at which the float64 reference alone
    (``split_sum_ref.fit_reference``) ends at 0.24 of its start (DESIGN 4.4n has both curves)."""
    from reni_amd.envmap_shader import GBuffer, MicrofacetMaterials
    from reni_amd.glossy import PrefilteredRenderer
    f = SR.FIT
    nrm, pos, cam, C = SR.fit_problem()
    NP = nrm.shape[0]
    env = _envmap(C.to(DEV))
    gb = GBuffer(nrm.to(DEV), pos.to(DEV), cam, f["S"])
    kw = dict(chain_roughness=f["rho"], out_width=f["Wo"], dfg_size=f["dfg_size"])
    bc = torch.tensor(f["base_color"])
    with torch.no_grad():
        target = PrefilteredRenderer(gb, materials=MicrofacetMaterials(bc, torch.full((NP,), f["target"]), f["metallic"]).to(DEV), **kw)(envmap=env)[0]
    mat = MicrofacetMaterials(bc, torch.full((NP,), f["start"]), f["metallic"], learn=("roughness",)).to(DEV)
    r = PrefilteredRenderer(gb, materials=mat, **kw)
    opt = torch.optim.Adam([mat.roughness], lr=f["lr"])
    losses = []
    for _ in range(f["steps"]):
        opt.zero_grad()
        loss = ((r(envmap=env)[0] - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("roughness fit through PrefilteredRenderer: loss", " ".join(f"{x:.4e}" for x in losses))
    assert bool(torch.isfinite(mat.roughness).all()) and losses[-1] < 0.5 * losses[0]
