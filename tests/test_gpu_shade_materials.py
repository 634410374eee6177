"""GPU tests of the shader's per-pixel materials (reni_envmap_shade_terms[_backward], envmap_shader.shade_terms /
compose_materials / SpatialMaterials, HipMeshRenderer(materials=), lighting.shade_sampled(materials=)) against the float64
reference tests/shade_materials_ref.py, whose autograd is the reference for every gradient.

Tolerances are the scalar shader's (test_gpu_shader.py): the maximum error over the maximum reference magnitude is at most
2e-4 when any shininess of the case exceeds 100 (the fp32 noise floor of x ** 500) and 2e-5 otherwise -- for D, S, T, dC,
d albedo and d ks.  The composed shininess gradient ds_p = sum_{b,c} g ks (norm'(s_p) S + norm(s_p) T) cancels by
construction (the two parts have opposite signs and nearly equal size under smooth lighting), so its error is held against
the size of its parts, rtol * max_p sum_{b,c} |g| ks (|norm'(s_p)| |S| + norm(s_p) |T|) from the float64 reference (the same
scale when one shininess is shared by all pixels and the gradient is the sum over them).
"""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import shade_materials_ref as MR
from tests import visibility_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")

# (B, NP, J, per-image directions): test_gpu_shader.py's small shapes and the mask-word cases
SHAPES = [(1, 300, 200, False),     # one workgroup, one split
          (3, 1000, 515, False),    # splits > 1, JW = 17
          (5, 257, 1030, False),    # B > BC, one pixel past a workgroup, JW = 33
          (9, 64, 129, False),      # one texel past an LDS stage
          (2, 130, 512, False),     # JW = 16: the 16-byte mask loads
          (2, 500, 300, True),      # per-image directions: the BC = 1 instances
          (3, 1, 1, False)]
SHININESS = ["s500", "s20", "per_pixel"]
CASES = [s + (k,) for s in SHAPES for k in SHININESS]


def _problem(B, NP, J, seed, frac_bg=0.2, per_image_dirs=False):  # test_gpu_shader.py's
    g = torch.Generator().manual_seed(seed)
    nrm = torch.randn(NP, 3, generator=g) * 0.7
    pos = torch.randn(NP, 3, generator=g) * 0.4
    bg = torch.rand(NP, generator=g) < frac_bg
    nrm[bg] = 0.0
    pos[bg] = 0.0
    cam = torch.tensor([0.0, 0.0, 2.0])
    shape = (B, J, 3) if per_image_dirs else (1, J, 3)
    L = torch.nn.functional.normalize(torch.randn(shape, generator=g), dim=-1)
    C = torch.exp(torch.randn(B, J, 3, generator=g)) * torch.rand(1, J, 1, generator=g)
    return nrm, pos, cam, L, C


def _pack(vis_bool):
    return torch.from_numpy(VR.pack_bits(vis_bool.numpy())).to(DEV)


def _reference(c, vis):
    """float64 terms and every gradient of one case under one mask (None or booleans), computed once."""
    f64 = torch.float64
    C = c.C.to(f64).requires_grad_(True)
    s = c.shin.to(f64).requires_grad_(True)
    a = c.albedo.to(f64).requires_grad_(True)
    k = c.ks.to(f64).requires_grad_(True)
    D, S, T = MR.shade_terms_ref(c.nrm, c.pos, c.cam, c.L, C, s, vis=vis)
    (dC,) = torch.autograd.grad((D * c.gD.to(f64)).sum() + (S * c.gS.to(f64)).sum(), C, retain_graph=True)
    col = MR.compose_ref(D, S, a, k, s)
    dC_col, da, dk, ds = torch.autograd.grad((col * c.w.to(f64)).sum(), (C, a, k, s))
    bound = MR.shininess_grad_bound(c.w, k.detach(), s.detach(), S.detach(), T.detach())
    return types.SimpleNamespace(D=D.detach(), S=S.detach(), T=T.detach(), dC=dC, col=col.detach(), dC_col=dC_col, da=da, dk=dk,
                                 ds=ds, ds_scale=float(bound.max()))


@functools.lru_cache(maxsize=None)
def _case(B, NP, J, per_image, kind):
    nrm, pos, cam, L, C = _problem(B, NP, J, seed=100 + B + NP, per_image_dirs=per_image)
    g = torch.Generator().manual_seed(7 * NP + J)
    shin = {"s500": torch.tensor(500.0), "s20": torch.tensor(20.0)}.get(kind)
    if shin is None:
        shin = torch.rand(NP, generator=g) * 495.0 + 5.0
    c = types.SimpleNamespace(B=B, NP=NP, J=J, nrm=nrm, pos=pos, cam=cam, L=L, C=C, shin=shin, per_image=per_image,
                              rtol=2e-4 if float(shin.max()) > 100 else 2e-5, bg=(nrm == 0).all(-1))
    c.albedo = torch.rand(NP, 3, generator=g)
    c.ks = torch.rand(NP, generator=g) * 0.8 + 0.1
    c.gD, c.gS, c.w = (torch.randn(B, NP, 3, generator=g) for _ in range(3))
    c.vis = torch.rand(L.shape[0], NP, J, generator=g) < 0.6
    c.ref = {"none": _reference(c, None), "random": _reference(c, c.vis)}
    c.dev = types.SimpleNamespace(nrm=nrm.to(DEV), pos=pos.to(DEV), L=(L if per_image else L[0]).to(DEV), C=C.to(DEV),
                                  shin=shin.to(DEV), gD=c.gD.to(DEV), gS=c.gS.to(DEV), w=c.w.to(DEV), vis=_pack(c.vis))
    return c


def _fwd(c, vis=None, need_ds=True, shin=None):
    from reni_amd import ops
    d = c.dev
    return ops.envmap_shade_terms(d.nrm, d.pos, c.cam, d.L, d.C, d.shin if shin is None else shin, vis=vis, need_ds=need_ds)


def _bwd(c, vis=None):
    from reni_amd import ops
    d = c.dev
    return ops.envmap_shade_terms_backward(d.nrm, d.pos, c.cam, d.L, d.gD, d.gS, d.shin, vis=vis)


def _close(name, got, ref, rtol, scale=None):
    got, ref = got.detach().double().cpu(), ref.double()
    scale = float(ref.abs().max()) if scale is None else scale
    err = float((got - ref).abs().max())
    print(f"{name}: max error {err:.3e}, scale {scale:.3e}, ratio {err / scale if scale > 0 else 0.0:.3e} (bound {rtol:g})")
    assert torch.isfinite(got).all(), name
    assert err <= rtol * scale, (name, err / scale if scale > 0 else err)


@pytest.mark.parametrize("B,NP,J,per_image,kind", CASES)
@pytest.mark.parametrize("mask", ["none", "random"])
def test_terms_and_every_gradient_match_float64(B, NP, J, per_image, kind, mask):
    from reni_amd.envmap_shader import EnvironmentMap, SpatialMaterials, blinn_phong_shading_materials
    c = _case(B, NP, J, per_image, kind)
    r, d = c.ref[mask], c.dev
    vis = None if mask == "none" else d.vis
    D, S, T = _fwd(c, vis)
    for name, got, ref in (("D", D, r.D), ("S", S, r.S), ("T", T, r.T)):
        _close(name, got, ref, c.rtol)
    _close("dC", _bwd(c, vis), r.dC, c.rtol)
    # without dS/ds the other two terms keep their bits
    D2, S2, none = _fwd(c, vis, need_ds=False)
    assert none is None and torch.equal(D2, D) and torch.equal(S2, S)
    # the autograd path: map, albedo, ks and shininess through shade_terms + compose_materials
    Cg = d.C.clone().requires_grad_(True)
    env = EnvironmentMap(environment_map=Cg, directions=d.L if per_image else d.L.expand(B, -1, -1),
                         sineweight=torch.ones(1, J, 1, device=DEV))
    m = SpatialMaterials(c.albedo, c.ks, c.shin, learn=("albedo", "ks", "shininess")).to(DEV)
    col = blinn_phong_shading_materials(d.nrm, d.pos, c.cam, env, *m.values(), vis=vis)
    _close("colours", col, r.col, c.rtol)
    (col * d.w).sum().backward()
    _close("dC through compose", Cg.grad, r.dC_col, c.rtol)
    _close("d albedo", m.albedo.grad, r.da, c.rtol)
    _close("d ks", m.ks.grad, r.dk, c.rtol)
    _close("d shininess", m.shininess.grad, r.ds, c.rtol, scale=r.ds_scale)
    # background pixels: exact zeros in every term and in their shininess gradient; everything finite
    if c.bg.any():
        bgd = c.bg.to(DEV)
        for t in (D, S, T, col):
            assert float(t[:, bgd].abs().max()) == 0.0
        if kind == "per_pixel":
            assert float(m.shininess.grad[bgd].abs().max()) == 0.0


@pytest.mark.parametrize("B,NP,J,per_image,kind", CASES)
def test_all_ones_mask_gives_the_unmasked_bits_and_all_zeros_gives_zeros(B, NP, J, per_image, kind):
    c = _case(B, NP, J, per_image, kind)
    plain, dC = _fwd(c), _bwd(c)
    ones = _pack(torch.ones_like(c.vis))
    for got, want in zip(_fwd(c, ones), plain):
        assert torch.equal(got, want)
    assert torch.equal(_bwd(c, ones), dC)
    if c.L.shape[0] > 1:  # per-image directions also take one mask for all images
        for got, want in zip(_fwd(c, ones[:1]), plain):
            assert torch.equal(got, want)
    full = torch.full_like(ones, -1)  # the bits past J set as well: they are never read
    for got, want in zip(_fwd(c, full), plain):
        assert torch.equal(got, want)
    zeros = torch.zeros_like(ones)
    for got in _fwd(c, zeros) + (_bwd(c, zeros),):
        assert float(got.abs().max()) == 0.0


@pytest.mark.parametrize("B,NP,J,per_image,kind", CASES)
def test_repeatable_adjoint_and_within_tolerance_of_the_scalar_shader(B, NP, J, per_image, kind):
    from reni_amd import ops
    from reni_amd.envmap_shader import compose_materials
    c = _case(B, NP, J, per_image, kind)
    d = c.dev
    for vis in (None, d.vis):
        D, S, T = _fwd(c, vis)
        dC = _bwd(c, vis)
        for got, want in zip(_fwd(c, vis), (D, S, T)):   # fixed-order partial sums: two calls give the same bits
            assert torch.equal(got, want)
        assert torch.equal(_bwd(c, vis), dC)
        # D and S are linear in C and dC is their adjoint: <gD, D(C)> + <gS, S(C)> = <dC(gD, gS), C>
        lhs = (D.double() * d.gD.double()).sum() + (S.double() * d.gS.double()).sum()
        rhs = (dC.double() * d.C.double()).sum()
        size = (D.double().abs() * d.gD.double().abs()).sum() + (S.double().abs() * d.gS.double().abs()).sum()
        assert abs(float(lhs - rhs)) <= 1e-5 * float(size)
        if kind != "per_pixel":  # scalar materials: both paths lie within rtol of float64, so within 2 rtol of each other
            s = float(c.shin)
            old = ops.envmap_shade(d.nrm, d.pos, c.cam, d.L, d.C, s, 0.4, 0.6, vis=vis)
            new = compose_materials(D, S, 0.4, 0.6, s)
            ref = MR.compose_ref(c.ref["none" if vis is None else "random"].D, c.ref["none" if vis is None else "random"].S, 0.4, 0.6, s)
            assert float((new - old).abs().max()) <= 2 * c.rtol * float(ref.abs().max())
            # one value handed over as a per-pixel array takes the stride-1 path and gives the same bits
            for got, want in zip(_fwd(c, vis, shin=torch.full((NP,), s, device=DEV)), (D, S, T)):
                assert torch.equal(got, want)


def test_need_ds_follows_the_shininess_requiring_grad():
    """T is computed only when the shininess requires grad and grad is enabled: the forward then takes the third term's
    workspace and kernel instance; the results of D and S do not depend on it."""
    from reni_amd.envmap_shader import EnvironmentMap, _ShadeTermsFn, shade_terms
    c = _case(3, 1000, 515, False, "per_pixel")
    d = c.dev
    env = EnvironmentMap(environment_map=d.C.clone().requires_grad_(True), directions=d.L.expand(3, -1, -1),
                         sineweight=torch.ones(1, 515, 1, device=DEV))
    seen = []
    import reni_amd.ops as ops
    orig = ops.envmap_shade_terms

    def spy(*a, **k):
        seen.append(k.get("need_ds"))
        return orig(*a, **k)

    ops.envmap_shade_terms = spy
    try:
        s = d.shin.clone().requires_grad_(True)
        D, S = shade_terms(d.nrm, d.pos, c.cam, env, s)
        D0, S0 = shade_terms(d.nrm, d.pos, c.cam, env, d.shin)
        with torch.no_grad():
            shade_terms(d.nrm, d.pos, c.cam, env, s)
    finally:
        ops.envmap_shade_terms = orig
    assert seen == [True, False, False]
    assert torch.equal(D, D0) and torch.equal(S, S0)
    (gs,) = torch.autograd.grad((S * d.gS).sum(), s)
    _close("ds = sum gS T", gs, (c.ref["none"].T * c.gS.double()).sum(dim=(0, 2)), c.rtol,
           scale=float((c.ref["none"].T.abs() * c.gS.double().abs()).sum(dim=(0, 2)).max()))


# ------------------------------------------------------------------------------------------------- renderer and workflow
@functools.lru_cache(maxsize=None)
def _teapot(shadows):
    from reni_amd.mesh import build_hip_renderer
    return build_hip_renderer(TEAPOT, 0, 32, 0.5, "cuda", shadows=shadows)


@functools.lru_cache(maxsize=None)
def _grid(W=32):
    from reni_amd.utils import get_directions, get_sineweight
    return get_directions(W).to(DEV), get_sineweight(W).to(DEV)


def _envmap(C, W=32):
    """-> (EnvironmentMap of C [B, J, 3] on the W/2 x W grid, the grid's directions [J, 3], its sine weights [1, J, 1])."""
    from reni_amd.envmap_shader import EnvironmentMap
    D, Sw = _grid(W)   # one tensor for every call: the renderer's visibility mask is cached by the directions' memory
    return EnvironmentMap(environment_map=C, directions=D.expand(C.shape[0], -1, -1), sineweight=Sw), D[0], Sw


@pytest.mark.parametrize("shadows", [False, True])
def test_a_float_kd_renderer_takes_todays_call_and_gives_todays_bits(shadows):
    from reni_amd import ops
    r, R, T, mesh = _teapot(shadows)
    assert not r.spatial
    C = (torch.rand(2, 512, 3, generator=torch.Generator().manual_seed(3)) * 4.0).to(DEV)
    env, D, _ = _envmap(C)
    col, _ = r(meshes_world=mesh, R=R, T=T, envmap=env)
    _, nrm, pos = r.rasterizer.gbuffer(mesh, R, T)
    vis = r.rasterizer.visibility(mesh, R, T, D) if shadows else None
    assert torch.equal(col.reshape(2, -1, 3), ops.envmap_shade(nrm, pos, r.camera_center, D, env.environment_map, 500.0, 0.5, 0.5, vis=vis))


def test_fit_albedo_ks_shininess_and_map_through_the_mesh_renderer():
    """tests/golden/teapot.obj at 32 x 32 under a 16 x 32 map, B = 2, shadows on.  The target has an albedo pattern, ks 0.3,
    s 40; the fit starts from albedo 0.5, ks 0.5, s 20 and a perturbed map and learns all four with Adam for 20 steps.  At
    step 0 every .grad matches the float64 reference within the bounds of the module docstring (s <= 100: 2e-5); every
    parameter stays finite; the final loss is below the initial one."""
    from reni_amd.envmap_shader import SpatialMaterials
    from reni_amd.mesh import build_hip_renderer, unpack_visibility
    S_, B = 32, 2
    NP, J = S_ * S_, 16 * 32
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(S_), torch.arange(S_), indexing="ij")
    checker = (((yy // 4) + (xx // 4)) % 2).float().reshape(NP, 1)
    albedo_gt = 0.25 + 0.5 * checker * torch.tensor([1.0, 0.6, 0.3]) + 0.1 * torch.rand(NP, 3, generator=g)
    C_gt = torch.rand(B, J, 3, generator=g) * 4.0
    target_r, R, T, mesh = build_hip_renderer(TEAPOT, 0, S_, None, "cuda", shadows=True,
                                              materials=SpatialMaterials(albedo_gt, 0.3, 40.0))
    with torch.no_grad():
        target = target_r(meshes_world=mesh, R=R, T=T, envmap=_envmap(C_gt.to(DEV))[0])[0]
    assert target.shape == (B, S_, S_, 3) and float(target.max()) > 0

    mats = SpatialMaterials(torch.full((NP, 3), 0.5), 0.5, 20.0, learn=("albedo", "ks", "shininess"))
    r, R, T, mesh = build_hip_renderer(TEAPOT, 0, S_, None, "cuda", shadows=True, materials=mats)
    assert r.spatial and {n for n, _ in r.named_parameters()} == {"materials.albedo", "materials.ks", "materials.shininess"}
    C0 = C_gt * (0.7 + 0.6 * torch.rand(B, J, 3, generator=g))
    Cp = C0.clone().to(DEV).requires_grad_(True)
    opt = torch.optim.Adam([{"params": [Cp, mats.albedo, mats.ks], "lr": 0.02}, {"params": [mats.shininess], "lr": 0.5}])
    losses = []
    for step in range(20):
        opt.zero_grad()
        env, D, Sw = _envmap(Cp)
        col, _ = r(meshes_world=mesh, R=R, T=T, envmap=env)
        loss = ((col - target) ** 2).mean()
        loss.backward()
        losses.append(float(loss))
        if step == 0:
            _, nrm, pos = r.rasterizer.gbuffer(mesh, R, T)
            vis = unpack_visibility(r.rasterizer.visibility(mesh, R, T, D), J).cpu()
            f64 = torch.float64
            C64 = C0.to(f64).requires_grad_(True)
            a64 = torch.full((NP, 3), 0.5, dtype=f64, requires_grad=True)
            k64, s64 = torch.tensor(0.5, dtype=f64, requires_grad=True), torch.tensor(20.0, dtype=f64, requires_grad=True)
            Dr, Sr, Tr = MR.shade_terms_ref(nrm.cpu(), pos.cpu(), r.camera_center, D.cpu()[None], C64 * Sw.cpu().to(f64), s64, vis=vis)
            col_ref = MR.compose_ref(Dr, Sr, a64, k64, s64)
            diff = col_ref - target.reshape(B, NP, 3).cpu().to(f64)
            loss_ref = (diff ** 2).mean()
            gC, ga, gk, gs = torch.autograd.grad(loss_ref, (C64, a64, k64, s64))
            assert abs(losses[0] - float(loss_ref)) <= 1e-4 * float(loss_ref)
            rtol = 2e-5
            _close("d map", Cp.grad, gC, rtol)
            _close("d albedo", mats.albedo.grad, ga, rtol)
            _close("d ks", mats.ks.grad, gk, rtol)
            gup = (2.0 * diff / diff.numel()).detach()  # the upstream gradient of the colours
            _close("d shininess", mats.shininess.grad, gs, rtol,
                   scale=float(MR.shininess_grad_bound(gup, k64.detach(), s64.detach(), Sr.detach(), Tr.detach()).max()))
        opt.step()
    for p in (Cp, mats.albedo, mats.ks, mats.shininess):
        assert torch.isfinite(p).all()
    print("loss", losses[0], "->", losses[-1])
    assert losses[-1] < losses[0]


def test_shade_sampled_with_materials_is_the_terms_path_on_per_image_lists():
    from reni_amd import lighting
    from reni_amd.envmap_shader import SpatialMaterials, compose_materials
    c = _case(2, 500, 300, True, "per_pixel")
    d = c.dev
    samples = lighting.LightSamples(index=torch.zeros(2, 300, dtype=torch.int32, device=DEV), dirs=d.L,
                                    pdf=torch.ones(2, 300, device=DEV), radiance=d.C, colors=d.C)
    m = SpatialMaterials(c.albedo, c.ks, c.shin).to(DEV)
    for vis in (None, d.vis):
        got = lighting.shade_sampled(samples, d.nrm, d.pos, c.cam, visibility=vis, materials=m)
        D, S, _ = _fwd(c, vis, need_ds=False)
        assert torch.equal(got, compose_materials(D, S, *m.values()))
        _close("sampled colours", got, c.ref["none" if vis is None else "random"].col, c.rtol)
