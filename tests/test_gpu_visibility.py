"""GPU tests of cast shadows: the ray caster (reni_tu_visibility.hip) against the float64 restatement of
tests/visibility_ref.py on every ray the restatement decides, the masked shader instances against float64 arithmetic with the
GPU's own mask, and the Python layers above them (MeshRasterizer.visibility, HipMeshRenderer(shadows=True), sampled lights,
ambient occlusion, FIT_INVERSE from a config)."""
import functools

import numpy as np
import pytest
import torch

from tests import visibility_ref as VR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TEAPOT = VR.TEAPOT


# ------------------------------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _accel(kind, key):
    from reni_amd import ops
    sc = VR.teapot_scene() if kind == "teapot" else VR.soup_scene(*key)
    return ops.mesh_visibility_prepare(torch.from_numpy(sc["verts"]).to(DEV), torch.from_numpy(sc["faces"]).to(DEV))


def _mask(kind, key, no_cull=False, dirs=None):
    """int32 words [NB, NP, JW] (on the host) of a shared scene from the library."""
    from reni_amd import ops
    sc = VR.teapot_scene() if kind == "teapot" else VR.soup_scene(*key)
    d = torch.from_numpy(sc["dirs"] if dirs is None else dirs).to(DEV)
    vis = ops.mesh_visibility(torch.from_numpy(sc["origins"]).to(DEV), torch.from_numpy(sc["own"]).to(DEV), d, _accel(kind, key),
                              sc["t_min"], no_cull=no_cull)
    return vis.cpu()


def _check_against_float64(vis, sc, occ, dec):
    from reni_amd.mesh import unpack_visibility
    NP, J = sc["origins"].shape[0], sc["dirs"].shape[0]
    assert vis.dtype == torch.int32 and tuple(vis.shape) == (1, NP, (J + 31) // 32)
    assert 1.0 - dec.mean() <= VR.UNDECIDED_MAX
    visible = unpack_visibility(vis, J)[0].numpy()
    bad = (visible != ~occ) & dec
    assert not bad.any(), f"{int(bad.sum())} decided rays differ, first (pixel, direction) {np.argwhere(bad)[:4].tolist()}"
    words = vis[0].numpy().view(np.uint32)
    if J % 32:
        assert not (words[:, -1] >> np.uint32(J % 32)).any(), "padding bits at j >= J must be 0"
    bg = sc["own"] < 0
    assert not words[bg].any(), "background rows must be 0"
    print(f"rays {NP * J}, undecided {int((~dec).sum())}, occluded {occ[~bg].mean() if (~bg).any() else 0:.3f}, "
          f"GPU vs float64 on undecided rays: {int(((visible != ~occ) & ~dec).sum())} differ")


def _masked_ref(nrm, pos, cam, L, C, s, kd, ks, mask):
    """oracle.reni_oracle.blinn_phong_gbuffer's arithmetic with the coefficient of (p, j) multiplied by mask [B or 1, NP, J]; float64."""
    dt = torch.float64
    N = torch.nn.functional.normalize(nrm.to(dt), p=2, dim=-1, eps=1e-6)
    V = torch.nn.functional.normalize(cam.to(dt)[None] - pos.to(dt), p=2, dim=-1, eps=1e-6)
    L = L.to(dt)
    sv = torch.as_tensor(s, dtype=dt)
    diffuse = torch.einsum("pk,bjk->bpj", N, L).clamp(0.0, 1.0)
    Hv = torch.nn.functional.normalize(V[None, :, None, :] + L[:, None, :, :], p=2, dim=-1, eps=1e-6)
    spec = torch.einsum("pk,bpjk->bpj", N, Hv).clamp(0.0, 1.0) ** sv
    norm = (sv + 2) / (4 * (2 - torch.exp(-sv / 2)))
    M = (kd * diffuse + norm * ks * spec) * mask.to(dt)
    return torch.einsum("bjk,bpj->bpk", C, M)


def _unit_dirs(g, *shape):
    return torch.nn.functional.normalize(torch.randn(*shape, 3, generator=g), dim=-1)


# ------------------------------------------------------------------------------------------------- 1. mask vs float64
@pytest.mark.parametrize("F,NP,J", VR.SOUP_CASES)
def test_soup_mask_matches_float64_on_decided_rays(F, NP, J):
    sc, occ, dec = VR.soup_case(F, NP, J)
    _check_against_float64(_mask("soup", (F, NP, J)), sc, occ, dec)


def test_teapot_mask_matches_float64_on_decided_rays():
    sc, occ, dec = VR.teapot_case()
    vis = _mask("teapot", None)
    _check_against_float64(vis, sc, occ, dec)
    from reni_amd.mesh import unpack_visibility
    fg = sc["own"] >= 0
    share = unpack_visibility(vis, 128)[0].numpy()[fg].mean()
    assert 0.2 < share < 0.7  # the teapot does shadow itself (float64: 0.47 of the foreground rays are visible)


# --------------------------------------------------------------------------------------------- 2. per-image directions
def test_per_image_directions_equal_shared_calls():
    key = (130, 257, 33)
    g = torch.Generator().manual_seed(5)
    dirs = _unit_dirs(g, 3, 33).numpy()
    vis = _mask("soup", key, dirs=dirs)
    assert tuple(vis.shape) == (3, 257, 2)
    for b in range(3):
        one = _mask("soup", key, dirs=dirs[b])
        assert tuple(one.shape) == (1, 257, 2) and torch.equal(vis[b], one[0])
    assert not torch.equal(vis[0], vis[1])


# ------------------------------------------------------------------------------------------ 3. determinism and culling
@pytest.mark.parametrize("F,NP,J", VR.SOUP_CASES)
def test_soup_mask_is_deterministic_and_culling_changes_no_bit(F, NP, J):
    a = _mask("soup", (F, NP, J))
    assert torch.equal(a, _mask("soup", (F, NP, J)))
    assert torch.equal(a, _mask("soup", (F, NP, J), no_cull=True))


def test_teapot_mask_is_deterministic_and_culling_changes_no_bit():
    a = _mask("teapot", None)
    assert torch.equal(a, _mask("teapot", None))
    assert torch.equal(a, _mask("teapot", None, no_cull=True))
    # the order of the faces inside the record is free: the given order (no Morton sort) gives the same bits as well
    from reni_amd import ops
    sc = VR.teapot_scene()
    v, f = torch.from_numpy(sc["verts"]).to(DEV), torch.from_numpy(sc["faces"]).to(DEV)
    plain = ops.mesh_visibility_prepare(v, f, order=torch.arange(f.shape[0], device=DEV))
    b = ops.mesh_visibility(torch.from_numpy(sc["origins"]).to(DEV), torch.from_numpy(sc["own"]).to(DEV),
                            torch.from_numpy(sc["dirs"]).to(DEV), plain, sc["t_min"])
    assert torch.equal(a, b.cpu())


# ------------------------------------------------------------------------------------------ 4. masked shader vs float64
SHADER_NP = 257


@functools.lru_cache(maxsize=None)
def _shader_case(B, J, per_image):
    """Inputs and the float64 reference (forward, and backward by autograd) of one masked-shader case, computed once."""
    g = torch.Generator().manual_seed(1000 * B + J + (7 if per_image else 0))
    NP = SHADER_NP
    nrm, pos, cam = torch.randn(NP, 3, generator=g), torch.randn(NP, 3, generator=g) * 0.4, torch.tensor([0.0, 0.0, 2.0])
    dirs = _unit_dirs(g, B, J) if per_image else _unit_dirs(g, J)
    C = torch.rand(B, J, 3, generator=g)
    w = torch.randn(B, NP, 3, generator=g)
    rng = np.random.default_rng([B, J, int(per_image)])
    mask = rng.random((B if per_image else 1, NP, J)) < 0.5
    words = torch.from_numpy(VR.pack_bits(mask))
    Cd = C.double().requires_grad_(True)
    L = dirs if per_image else dirs.expand(B, J, 3)
    ref = _masked_ref(nrm, pos, cam, L, Cd, 500.0, 0.5, 0.5, torch.from_numpy(mask))
    (ref_g,) = torch.autograd.grad((ref * w.double()).sum(), Cd)
    return dict(nrm=nrm, pos=pos, cam=cam, dirs=dirs, C=C, w=w, mask=mask, words=words, ref=ref.detach(), ref_g=ref_g)


# (J = 256 beside the three odd sizes: 8 words per pixel, the forward instance's 16-byte row loads; the others take the guarded loads)
SHADER_CASES = [(B, J, False) for B in (1, 5) for J in (33, 129, 300, 256)] + [(3, J, True) for J in (33, 129, 300, 256)]


@pytest.mark.parametrize("B,J,per_image", SHADER_CASES)
def test_masked_shader_against_float64(B, J, per_image):
    from reni_amd import ops
    from reni_amd.mesh import unpack_visibility
    c = _shader_case(B, J, per_image)
    nrm, pos, dirs, vis = c["nrm"].to(DEV), c["pos"].to(DEV), c["dirs"].to(DEV), c["words"].to(DEV)
    assert (unpack_visibility(c["words"], J).numpy() == c["mask"]).all()
    col = ops.envmap_shade(nrm, pos, c["cam"], dirs, c["C"].to(DEV), 500.0, 0.5, 0.5, vis=vis)
    gC = ops.envmap_shade_backward(nrm, pos, c["cam"], dirs, c["w"].to(DEV), 500.0, 0.5, 0.5, vis=vis)
    ef = float((col.cpu().double() - c["ref"]).abs().max()) / float(c["ref"].abs().max())
    eb = float((gC.cpu().double() - c["ref_g"]).abs().max()) / float(c["ref_g"].abs().max())
    print(f"B {B} J {J} per_image {per_image}: forward {ef:.3g}, backward {eb:.3g} of the reference's max (bound 2e-4)")
    assert ef <= 2e-4 and eb <= 2e-4
    # the mask did something: the unmasked result is far from the masked reference
    plain = ops.envmap_shade(nrm, pos, c["cam"], dirs, c["C"].to(DEV), 500.0, 0.5, 0.5)
    assert float((plain.cpu().double() - c["ref"]).abs().max()) > 1e-2 * float(c["ref"].abs().max())
    # deterministic
    assert torch.equal(col, ops.envmap_shade(nrm, pos, c["cam"], dirs, c["C"].to(DEV), 500.0, 0.5, 0.5, vis=vis))
    assert torch.equal(gC, ops.envmap_shade_backward(nrm, pos, c["cam"], dirs, c["w"].to(DEV), 500.0, 0.5, 0.5, vis=vis))


@pytest.mark.parametrize("B,J,per_image", SHADER_CASES)
def test_all_ones_mask_is_the_unmasked_shader_bit_for_bit_and_all_zero_is_zero(B, J, per_image):
    from reni_amd import ops
    c = _shader_case(B, J, per_image)
    nrm, pos, dirs = c["nrm"].to(DEV), c["pos"].to(DEV), c["dirs"].to(DEV)
    C, w = c["C"].to(DEV), c["w"].to(DEV)
    NB = B if per_image else 1
    ones = torch.from_numpy(VR.pack_bits(np.ones((NB, SHADER_NP, J), bool))).to(DEV)
    zeros = torch.zeros_like(ones)
    col = ops.envmap_shade(nrm, pos, c["cam"], dirs, C, 500.0, 0.5, 0.5)
    gC = ops.envmap_shade_backward(nrm, pos, c["cam"], dirs, w, 500.0, 0.5, 0.5)
    assert torch.equal(ops.envmap_shade(nrm, pos, c["cam"], dirs, C, 500.0, 0.5, 0.5, vis=ones), col)
    assert torch.equal(ops.envmap_shade_backward(nrm, pos, c["cam"], dirs, w, 500.0, 0.5, 0.5, vis=ones), gC)
    z = ops.envmap_shade(nrm, pos, c["cam"], dirs, C, 500.0, 0.5, 0.5, vis=zeros)
    zg = ops.envmap_shade_backward(nrm, pos, c["cam"], dirs, w, 500.0, 0.5, 0.5, vis=zeros)
    assert float(z.abs().max()) == 0.0 and float(zg.abs().max()) == 0.0
    if per_image:  # one mask for all images of per-image lists is accepted too
        one = ones[:1].contiguous()
        assert torch.equal(ops.envmap_shade(nrm, pos, c["cam"], dirs, C, 500.0, 0.5, 0.5, vis=one), col)


# ---------------------------------------------------------------------------------------- 5, 6. the renderer: autograd, physics
@functools.lru_cache(maxsize=None)
def _teapot_renderers(kd):
    from reni_amd.mesh import build_hip_renderer
    return build_hip_renderer(TEAPOT, 0, 32, kd, "cuda", shadows=True), build_hip_renderer(TEAPOT, 0, 32, kd, "cuda")


def _envmap(B, seed, W=16):
    from reni_amd.envmap_shader import EnvironmentMap
    from reni_amd.utils import get_directions, get_sineweight
    g = torch.Generator().manual_seed(seed)
    D, Sw = get_directions(W), get_sineweight(W)
    C = (torch.rand(B, D.shape[1], 3, generator=g) * 4.0).to(DEV).requires_grad_(True)
    env = EnvironmentMap(environment_map=C, directions=D.expand(B, -1, -1).to(DEV), sineweight=Sw.to(DEV))
    return env, C, D[0].to(DEV)


def test_renderer_autograd_is_the_masked_backward_and_shadows_off_is_todays_renderer():
    from reni_amd import ops
    (rs, R, T, mesh), (r0, R0, T0, mesh0) = _teapot_renderers(0.5)
    assert rs.shadows and not r0.shadows
    env, C, D = _envmap(2, 11)
    col, normals = rs(meshes_world=mesh, R=R, T=T, envmap=env)
    assert col.shape == (2, 32, 32, 3) and normals.shape == (2, 32, 32, 3)
    w = torch.randn(2, 32, 32, 3, generator=torch.Generator().manual_seed(12)).to(DEV)
    (g,) = torch.autograd.grad((col * w).sum(), env.environment_map)
    _, nrm, pos = rs.rasterizer.gbuffer(mesh, R, T)
    mask = rs.rasterizer.visibility(mesh, R, T, D)
    assert tuple(mask.shape) == (1, 1024, 4)
    want = ops.envmap_shade_backward(nrm, pos, rs.camera_center, D, w.reshape(2, -1, 3), 500.0, 0.5, 0.5, vis=mask)
    assert torch.equal(g, want)
    assert torch.equal(col.reshape(2, -1, 3), ops.envmap_shade(nrm, pos, rs.camera_center, D, env.environment_map.detach(),
                                                               500.0, 0.5, 0.5, vis=mask))
    # shadows=False: what the renderer gave before it knew about shadows -- the unmasked entry point on the same G-buffer
    col0, normals0 = r0(meshes_world=mesh0, R=R0, T=T0, envmap=env)
    _, nrm0, pos0 = r0.rasterizer.gbuffer(mesh0, R0, T0)
    assert torch.equal(nrm0, nrm) and torch.equal(pos0, pos)
    assert torch.equal(col0.reshape(2, -1, 3), ops.envmap_shade(nrm0, pos0, r0.camera_center, D, env.environment_map.detach(),
                                                                500.0, 0.5, 0.5))
    (g0,) = torch.autograd.grad((col0 * w).sum(), env.environment_map)
    assert torch.equal(g0, ops.envmap_shade_backward(nrm0, pos0, r0.camera_center, D, w.reshape(2, -1, 3), 500.0, 0.5, 0.5))
    assert torch.equal(normals0, normals) and not torch.equal(col0, col)
    # the mask is cached: the same grid (a fresh view of the same memory) casts no rays again, another grid does
    n0 = ops.launch_count()
    assert rs.rasterizer.visibility(mesh, R, T, env.directions[0]) is rs.rasterizer.visibility(mesh, R, T, env.directions[0])
    rs(meshes_world=mesh, R=R, T=T, envmap=env)
    n1 = ops.launch_count()
    rs.rasterizer.visibility(mesh, R, T, D.clone())
    assert ops.launch_count() == n1 + 1 and rs.rasterizer.visibility(mesh, R, T, D) is not mask
    assert torch.equal(rs.rasterizer.visibility(mesh, R, T, D), mask)
    assert n1 - n0 <= 1  # (at most the one pass for env.directions' own memory; none for the render after it)


def test_shadows_only_ever_darken_a_non_negative_map():
    from reni_amd.mesh import unpack_visibility
    (rs, R, T, mesh), (r0, R0, T0, mesh0) = _teapot_renderers(1.0)
    env, C, D = _envmap(3, 21)
    with torch.no_grad():
        dark = rs(meshes_world=mesh, R=R, T=T, envmap=env)[0].reshape(3, -1, 3)
        lit = r0(meshes_world=mesh0, R=R0, T=T0, envmap=env)[0].reshape(3, -1, 3)
    assert bool((dark <= lit).all()) and bool((dark >= 0).all())
    frag, nrm, pos = rs.rasterizer.gbuffer(mesh, R, T)
    fg = (frag.pix_to_face.reshape(-1) >= 0).cpu()
    assert bool((dark[:, fg] < lit[:, fg]).any()), "the teapot casts no shadow on itself"
    assert float(dark[:, ~fg].abs().max()) == 0.0 and float(lit[:, ~fg].abs().max()) == 0.0
    # where a pixel sees every direction that can light it (kd = 1: those with n . l > 0; the margin keeps fp32's view of
    # the horizon inside the set), the shadowed render is the unshadowed one, bit for bit
    visible = unpack_visibility(rs.rasterizer.visibility(mesh, R, T, D), D.shape[0])[0].cpu()
    n = torch.nn.functional.normalize(nrm.double().cpu(), dim=-1, eps=1e-6)
    can_light = (n @ D.double().cpu().t()) > -1e-3
    free = fg & ~((~visible) & can_light).any(dim=1)
    shadowed = fg & ((~visible) & ((n @ D.double().cpu().t()) > 0.05)).any(dim=1)
    print(f"foreground {int(fg.sum())}, fully lit {int(free.sum())}, shadowed {int(shadowed.sum())}")
    assert int(free.sum()) >= 10 and int(shadowed.sum()) >= 50  # (float64 on the restated G-buffer: 46 and most of the rest)
    assert torch.equal(dark[:, free], lit[:, free])
    # a pixel that loses a direction with a clear cosine under a map that is positive everywhere gets darker
    assert bool((dark[:, shadowed].sum(-1) < lit[:, shadowed].sum(-1)).all())


# --------------------------------------------------------------------------------------------------- 7. sampled lights
def test_sampled_lights_cast_shadows():
    from reni_amd import lighting
    from reni_amd.mesh import unpack_visibility
    (rs, R, T, mesh), _ = _teapot_renderers(0.5)
    B, S = 2, 48
    g = torch.Generator().manual_seed(31)
    dirs = _unit_dirs(g, B, S).to(DEV)
    colors = torch.rand(B, S, 3, generator=g).to(DEV)
    samples = lighting.LightSamples(index=torch.zeros(B, S, dtype=torch.int32, device=DEV), dirs=dirs,
                                    pdf=torch.ones(B, S, device=DEV), radiance=colors, colors=colors)
    _, nrm, pos = rs.rasterizer.gbuffer(mesh, R, T)
    vis = lighting.light_visibility(rs.rasterizer, mesh, R, T, samples)
    assert tuple(vis.shape) == (B, 1024, 2) and vis.dtype == torch.int32
    for b in range(B):  # each image's list is a shared-direction pass of its own
        assert torch.equal(vis[b], rs.rasterizer.visibility(mesh, R, T, dirs[b].contiguous())[0])
    cam = torch.tensor([0.0, 0.0, 2.0])
    out = lighting.shade_sampled(samples, nrm, pos, cam, 500.0, 0.5, 0.5, visibility=vis)
    mask = unpack_visibility(vis, S).cpu()
    ref = _masked_ref(nrm.cpu(), pos.cpu(), cam, dirs.cpu(), colors.cpu().double(), 500.0, 0.5, 0.5, mask)
    err = float((out.cpu().double() - ref).abs().max()) / float(ref.abs().max())
    print(f"sampled lights: {err:.3g} of the reference's max (bound 2e-4); visible share {float(mask.double().mean()):.3f}")
    assert err <= 2e-4
    plain = lighting.shade_sampled(samples, nrm, pos, cam, 500.0, 0.5, 0.5)
    assert bool((out <= plain).all()) and bool((out < plain).any())


# ------------------------------------------------------------------------------------------------- 8. ambient occlusion
def _ao_scene(verts, faces, origin, own, W=16):
    from reni_amd import lighting, ops
    from reni_amd.utils import get_directions, get_sineweight
    D = get_directions(W)[0].to(DEV)
    wts = get_sineweight(W)[0, :, 0].to(DEV)
    v = torch.tensor(verts, dtype=torch.float32, device=DEV)
    f = torch.tensor(faces, dtype=torch.int64, device=DEV)
    pos = torch.tensor([origin], dtype=torch.float32, device=DEV)
    vis = ops.mesh_visibility(pos, torch.tensor([own], device=DEV), D, ops.mesh_visibility_prepare(v, f), 1e-4)
    nrm = torch.tensor([[0.0, 0.0, 3.0]], device=DEV)  # (not normalised: the shader does that)
    return float(lighting.ambient_occlusion(vis, nrm, D, wts)[0])


def test_ambient_occlusion_of_an_open_and_of_a_covered_point():
    floor = [[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]]
    below = [[-1.0, -1.0, -5.0], [1.0, -1.0, -5.0], [0.0, 1.0, -5.0]]       # under the horizon of the point's normal
    lid = [[-40.0, -30.0, 0.01], [40.0, -30.0, 0.01], [0.0, 50.0, 0.01]]    # covers every grid direction above the horizon
    assert _ao_scene(floor + below, [[0, 1, 2], [3, 4, 5]], [0.0, -0.2, 0.0], 0) == 1.0
    assert _ao_scene(floor + lid, [[0, 1, 2], [3, 4, 5]], [0.0, -0.2, 0.0], 0) == 0.0
    assert _ao_scene(floor + lid, [[0, 1, 2], [3, 4, 5]], [0.0, -0.2, 0.0], -1) == 0.0   # a background pixel sees nothing
    half = [[0.0, -50.0, 0.01], [0.0, 50.0, 0.01], [60.0, 0.0, 0.01]]       # covers the directions with x > 0 only
    assert 0.3 < _ao_scene(floor + half, [[0, 1, 2], [3, 4, 5]], [0.0, -0.2, 0.0], 0) < 0.7


def test_ambient_occlusion_on_the_teapot_against_float64():
    from reni_amd import lighting
    from reni_amd.mesh import unpack_visibility
    from reni_amd.utils import get_directions, get_sineweight
    (rs, R, T, mesh), _ = _teapot_renderers(0.5)
    D = get_directions(16)[0].to(DEV)
    wts = get_sineweight(16)[0, :, 0].to(DEV)
    frag, nrm, pos = rs.rasterizer.gbuffer(mesh, R, T)
    vis = rs.rasterizer.visibility(mesh, R, T, D)
    ao = lighting.ambient_occlusion(vis, nrm, D, wts).cpu().double()
    assert tuple(ao.shape) == (1024,)
    n = torch.nn.functional.normalize(nrm.cpu().double(), dim=-1, eps=1e-6)
    cosw = (n @ D.cpu().double().t()).clamp(0.0, 1.0) * wts.cpu().double()[None]
    num, den = (cosw * unpack_visibility(vis, 128)[0].cpu().double()).sum(1), cosw.sum(1)
    ref = torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(den))
    fg = (frag.pix_to_face.reshape(-1) >= 0).cpu()
    assert float(ao[~fg].abs().max()) == 0.0 and bool((den[~fg] == 0).all())
    # each of the two shader calls is held to 2e-4 of its reference's max (smoke()'s bar), the denominator's max being the
    # larger one: |ao - ref| <= (|d num| + ref |d den|) / den <= 2 * 2e-4 * max(den) / den
    bound = 4e-4 * float(den.max()) / den[fg]
    err = (ao[fg] - ref[fg]).abs()
    print(f"ambient occlusion: worst error {float(err.max()):.3g}, worst error / bound {float((err / bound).max()):.3g}; "
          f"mean {float(ref[fg].mean()):.3f}")
    assert bool((err <= bound).all())
    assert bool((ao >= 0).all()) and bool((ao <= 1).all())
    assert bool((ref[fg] < 0.9).any()) and bool((ref[fg] == 1.0).any())  # some pixels sit in shadow, some see their whole hemisphere


# ---------------------------------------------------------------------------------------------- 9. FIT_INVERSE, SHADOWS
def _inverse_cfg(shadows):
    from tests.test_gpu_workflows import _config, _task
    cfg = _config("VariationalAutoDecoder")
    extra = {} if shadows is None else {"SHADOWS": shadows}
    cfg.RENI.FIT_INVERSE = _task(BATCH_SIZE=2, LR_START=1e-2, LR_END=1e-2, COSINE_SIMILARITY_WEIGHT=1e-4, OBJECT_PATH=TEAPOT,
                                 RENDER_RESOLUTION=32, KD_VALUE=1.0, **extra)
    return cfg


def test_fit_inverse_with_shadows_from_the_config():
    from reni_amd import ops, trainer
    from reni_amd.data import SyntheticEnvMapDataset
    from reni_amd.lightning_module import RENI
    from reni_amd.mesh import HipMeshRenderer
    ds = SyntheticEnvMapDataset(4, 16, 32)
    torch.manual_seed(0)
    m = RENI(_inverse_cfg(True), "FIT_INVERSE", dataset=ds)
    hist = trainer.fit(m, max_epochs=5, device=DEV)  # 4 images in batches of 2: 10 steps
    assert isinstance(m.renderer, HipMeshRenderer) and m.renderer.shadows
    assert hist[-1]["loss"] < hist[0]["loss"]
    # the config without the key, or with False, builds today's renderer; its ground-truth renders are the brighter ones
    for flag in (None, False):
        torch.manual_seed(0)
        plain = RENI(_inverse_cfg(flag), "FIT_INVERSE", dataset=ds)
        plain.setup()
        plain.on_fit_start()
        assert isinstance(plain.renderer, HipMeshRenderer) and not plain.renderer.shadows
        assert bool((m.gt_renders <= plain.gt_renders).all()) and bool((m.gt_renders < plain.gt_renders).any())
    # further renders through the module reuse the cached mask: no visibility pass is launched
    imgs = torch.stack([ds[i][0] for i in (0, 1)]).to(DEV).permute(0, 2, 3, 1).reshape(2, -1, 3)
    directions, sineweight = m._grids(imgs)
    with torch.no_grad():
        a = m.get_render(imgs, directions, sineweight)
        n0 = ops.launch_count()
        b = m.get_render(imgs, directions, sineweight)
    assert ops.launch_count() == n0 and torch.equal(a, b)
    # ... and so does a second renderer on the same rasteriser
    again = HipMeshRenderer(m.renderer.rasterizer, kd=1.0, shadows=True)
    kw = m.render_kwargs
    from reni_amd.envmap_shader import EnvironmentMap
    env = EnvironmentMap(environment_map=torch.rand(2, directions.shape[-2], 3, device=DEV),
                         directions=directions.expand(2, -1, -1), sineweight=sineweight)
    n0 = ops.launch_count()
    with torch.no_grad():
        c = again(envmap=env, **kw)[0]
        d = m.renderer(envmap=env, **kw)[0]
    assert ops.launch_count() == n0 and torch.equal(c, d)
