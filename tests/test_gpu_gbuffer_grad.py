"""GPU tests of the G-buffer's gradient with respect to the vertices (reni_tu_raster_bwd.hip, ops.gbuffer_backward,
ops.vertex_normals_backward, the autograd nodes of reni_amd.mesh) against the float64 reference of
tests/gbuffer_grad_ref.py evaluated with the device's own pix_to_face.

Bounds: max(K 2^-23 sum |terms|, 2e-5 max |ref|) per element, sum |terms| accumulated by the reference, K = 4 x the worst
ratio of the float32 CPU evaluation over the same cases (K_GVERTS, K_VNORMALS, K_E2E of the case file; DESIGN 4.4p has the
measured figures, the device's among them).  Every test prints its figure before it asserts."""
import pytest
import torch

from tests import gbuffer_grad_ref as G
from tests import raster_edge_cases as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(key):
    v, f, R, T, S = G.case(*key)
    return torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), R, T, S


def _raster(key):
    from reni_amd import ops
    v, f, R, T, S = _dev(key)
    vn = ops.vertex_normals(v, f)
    p2f = ops.rasterize_mesh(v, f, vn, R, T, S, E.TANF)[0]
    return v, f, vn, R, T, S, p2f


def _to_dev(g):
    return None if g is None else g.float().to(DEV)


@pytest.mark.parametrize("variant", G.VARIANTS)
@pytest.mark.parametrize("key", G.CASES, ids=G.case_id)
def test_gbuffer_backward_matches_the_float64_reference(key, variant):
    from reni_amd import ops
    v, f, vn, R, T, S, p2f = _raster(key)
    gN, gX = G.upstream(key, variant)
    got = ops.gbuffer_backward(v, f, vn, R, T, S, p2f, _to_dev(gN), _to_dev(gX), tan_half_fov=E.TANF)
    p2f_cpu = p2f.reshape(-1).cpu()
    ref = G.reference(key, p2f_cpu, gN, gX)
    _, terms = G.closed_form(*G._inputs(key, G.F64)[:4], S, E.TANF, p2f_cpu, gN, gX)
    print(f"g_verts {G.case_id(key)} {variant}: error / (2^-23 sum |terms|) = {G.error_ratio(got, ref, terms):.4g}, "
          f"error / bound = {G.over_bound(got, ref, terms, G.K_GVERTS):.4g}, covered {int((p2f_cpu >= 0).sum())}")
    assert got.shape == ref.shape and torch.isfinite(got).all()
    assert G.over_bound(got, ref, terms, G.K_GVERTS) <= 1.0  # no case and no vertex left out


@pytest.mark.parametrize("key", G.CASES, ids=G.case_id)
def test_vertex_normals_backward_matches_the_float64_reference(key):
    from reni_amd import ops
    v, f, *_ = _dev(key)
    gn = G.normals_upstream(key)
    got = ops.vertex_normals_backward(v, f, gn.float().to(DEV))
    vc, fc = G.case(*key)[:2]
    ref = G.vertex_normals_reference(vc, fc, gn)
    _, terms = G.vn_closed_form(torch.from_numpy(vc).double(), torch.from_numpy(fc), gn)
    print(f"vertex-normal backward {G.case_id(key)}: error / (2^-23 sum |terms|) = {G.error_ratio(got, ref, terms):.4g}")
    assert G.over_bound(got, ref, terms, G.K_VNORMALS) <= 1.0
    # lists kept by the caller give the same bits
    assert torch.equal(got, ops.vertex_normals_backward(v, f, gn.float().to(DEV), vf=ops.vertex_face_lists(f, v.shape[0])))


def test_exact_zeros():
    from reni_amd import ops
    key = ("unreferenced", 16)
    v, f, vn, R, T, S, p2f = _raster(key)
    gN, gX = (_to_dev(g) for g in G.upstream(key, "both"))
    g = ops.gbuffer_backward(v, f, vn, R, T, S, p2f, gN, gX, tan_half_fov=E.TANF)
    assert (g[G.UNREFERENCED] == 0).all() and (g != 0).any()
    assert (ops.vertex_normals_backward(v, f, torch.randn_like(v))[G.UNREFERENCED] == 0).all()
    for a, b in ((torch.zeros_like(gN), torch.zeros_like(gX)), (torch.zeros_like(gN), None), (None, torch.zeros_like(gX))):
        assert (ops.gbuffer_backward(v, f, vn, R, T, S, p2f, a, b, tan_half_fov=E.TANF) == 0).all()  # a zero upstream
    assert (ops.vertex_normals_backward(v, f, torch.zeros_like(v)) == 0).all()
    key = ("behind", 16)  # all background: nothing through the pixel paths, so nothing at all
    v, f, vn, R, T, S, p2f = _raster(key)
    assert (p2f < 0).all()
    for variant in G.VARIANTS:
        gN, gX = (_to_dev(g) for g in G.upstream(key, variant))
        assert (ops.gbuffer_backward(v, f, vn, R, T, S, p2f, gN, gX, tan_half_fov=E.TANF) == 0).all()


def test_malformed_tables_add_nothing():
    """entries that do not fit -- list entries outside [0, S*S), offsets outside the list, a pixel whose pix_to_face is not the
    face or lies outside [-1, F) -- are skipped: the gradient is that of the well-formed entries alone"""
    from reni_amd import ops
    key = ("ico", 17)
    v, f, vn, R, T, S, p2f = _raster(key)
    gN, gX = (_to_dev(g) for g in G.upstream(key, "both"))
    F = f.shape[0]
    off, lst = ops.face_pixel_table(p2f, F)

    def run(p, table):
        return ops.gbuffer_backward(v, f, vn, R, T, S, p, gN, gX, tan_half_fov=E.TANF, table=table)

    good = run(p2f, None)
    assert torch.equal(good, run(p2f, (off, lst)))
    dropped = lst[int(off[0])::3]  # every third covered pixel
    p2f_kept = p2f.reshape(-1).clone()
    p2f_kept[dropped] = -1
    kept = run(p2f_kept, (off, lst))  # (the same table: the same lanes take the same pixels)
    assert (kept != good).any()
    junk = torch.tensor([-1, S * S, 2 ** 40], device=DEV).repeat(dropped.numel() // 3 + 1)[:dropped.numel()]
    bad_list = lst.clone()
    bad_list[int(off[0])::3] = junk
    assert torch.equal(kept, run(p2f, (off, bad_list)))
    p2f_bad = p2f.reshape(-1).clone()
    p2f_bad[dropped] = torch.tensor([F, F + 3, -7], device=DEV).repeat(dropped.numel() // 3 + 1)[:dropped.numel()]
    assert torch.equal(kept, run(p2f_bad, (off, lst)))
    off_wide = off.clone()
    off_wide[0], off_wide[F] = -5, S * S + 7  # face 0 is offered the background as well: none of it is its own
    wide = run(p2f, (off_wide, lst))
    assert float((wide - good).abs().max()) <= 1e-5 * float(good.abs().max())  # (face 0's lanes take other pixels: rounding)


def _mesh_and_rasterizer(key, requires_grad, S=None):
    from reni_amd.mesh import FoVPerspectiveCameras, MeshRasterizer, Meshes, RasterizationSettings
    v, f, R, T, S0 = _dev(key)
    v = v.clone().requires_grad_(requires_grad)
    mesh = Meshes(verts=[v], faces=[f])
    rast = MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=S or S0))
    return v, f, R.to(DEV), T.to(DEV), mesh, rast


def test_two_runs_are_bit_equal_and_two_rasterisers_accumulate():
    from reni_amd import ops
    from reni_amd.mesh import FoVPerspectiveCameras, MeshRasterizer, RasterizationSettings, look_at_view_transform
    for key in (("cover", 33), ("fan", 16), ("soup", 17)):
        v, f, vn, R, T, S, p2f = _raster(key)
        gN, gX = (_to_dev(g) for g in G.upstream(key, "both"))
        a = ops.gbuffer_backward(v, f, vn, R, T, S, p2f, gN, gX, tan_half_fov=E.TANF)
        b = ops.gbuffer_backward(v, f, vn, R, T, S, p2f, gN, gX, tan_half_fov=E.TANF)
        assert torch.equal(a, b)
        gn = torch.randn_like(v)
        assert torch.equal(ops.vertex_normals_backward(v, f, gn), ops.vertex_normals_backward(v, f, gn))
    # two rasterisers (two cameras) on one Meshes: verts.grad is the sum of the two separate gradients
    key = ("ico", 16)
    v, f, R, T, mesh, rast = _mesh_and_rasterizer(key, True)
    R2, T2 = look_at_view_transform(2.0, 20.0, 40.0, device=DEV)
    rast2 = MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=17))
    w = [torch.randn(n, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(3)) for n in (256, 256, 289, 289)]

    def loss1():
        _, n, x = rast.gbuffer(mesh, R, T)
        return (n * w[0]).sum() + (x * w[1]).sum()

    def loss2():
        _, n, x = rast2.gbuffer(mesh, R2, T2)
        return (n * w[2]).sum() + (x * w[3]).sum()

    (g1,) = torch.autograd.grad(loss1(), v)
    (g2,) = torch.autograd.grad(loss2(), v)
    (loss1() + loss2()).backward()
    assert (g1 != 0).any() and (g2 != 0).any()
    assert torch.equal(v.grad, g1 + g2)
    # two renders of one cached G-buffer are back-propagated separately
    l1, l2 = loss1(), loss1()
    (h1,) = torch.autograd.grad(l1, v)
    (h2,) = torch.autograd.grad(l2, v)
    assert torch.equal(h1, g1) and torch.equal(h2, g1)
    # the normals alone: Meshes.verts_normals_packed() carries the vertex-normal backward
    wn = torch.randn_like(v)
    (gn,) = torch.autograd.grad((mesh.verts_normals_packed() * wn).sum(), v)
    assert torch.equal(gn, ops.vertex_normals_backward(v.detach(), f, wn))


def _env(B=1, smooth=False):
    from reni_amd.envmap_shader import EnvironmentMap
    D, C = G.envmap_8x16(smooth=smooth, B=B)
    return EnvironmentMap(environment_map=C.float().to(DEV), directions=D.float().expand(B, -1, -1).to(DEV),
                          sineweight=torch.ones(1, device=DEV))


def test_without_requires_grad_nothing_changes():
    """gbuffer and a HipMeshRenderer render return the bits of ops.rasterize_mesh and of the scalar shader called directly"""
    from reni_amd import ops
    from reni_amd.envmap_shader import blinn_phong_shading_gbuffer
    from reni_amd.mesh import HipMeshRenderer
    key = ("ico", 16)
    v, f, R, T, mesh, rast = _mesh_and_rasterizer(key, False)
    frags, nrm, pos = rast.gbuffer(mesh, R, T)
    direct = ops.rasterize_mesh(v, f, ops.vertex_normals(v, f), R, T, 16, rast.cameras.tan_half_fov())
    for a, b in zip((frags.pix_to_face, frags.zbuf, frags.bary_coords, frags.dists, nrm, pos), direct):
        assert torch.equal(a, b)
    assert not nrm.requires_grad and not pos.requires_grad and rast.gbuffer(mesh, R, T)[1] is nrm
    env = _env(2)
    for kd, shadows in ((1.0, False), (0.6, False), (0.6, True)):
        renderer = HipMeshRenderer(rast, kd=kd, shadows=shadows)
        col, normals = renderer(meshes_world=mesh, R=R, T=T, envmap=env)
        vis = rast.visibility(mesh, R, T, env.directions[0]) if shadows else None
        want = blinn_phong_shading_gbuffer(direct[4], direct[5], renderer.camera_center, env, 500.0, kd, 1.0 - kd, vis=vis)
        assert torch.equal(col, want.reshape(2, 16, 16, 3))
        assert torch.equal(normals[0], torch.nn.functional.normalize(direct[4], dim=-1, eps=1e-6).reshape(16, 16, 3))
    # with requires_grad the forward is the same kernel: same bits in the G-buffer, the render equal to rounding
    v2, _, _, _, mesh2, rast2 = _mesh_and_rasterizer(key, True)
    _, n2, x2 = rast2.gbuffer(mesh2, R, T)
    assert n2.requires_grad and x2.requires_grad and torch.equal(n2, nrm) and torch.equal(x2, pos)
    with torch.no_grad():
        assert not rast2.gbuffer(mesh2, R, T)[1].requires_grad
    col2, _ = HipMeshRenderer(rast2, kd=0.6)(meshes_world=mesh2, R=R, T=T, envmap=env)
    col, _ = HipMeshRenderer(rast, kd=0.6)(meshes_world=mesh, R=R, T=T, envmap=env)
    assert float((col2.detach() - col).abs().max()) <= 2e-5 * float(col.abs().max())


def test_normals_follow_an_in_place_vertex_edit():
    from reni_amd import ops
    key = ("ico", 16)
    v, f, R, T, mesh, rast = _mesh_and_rasterizer(key, False)
    n0 = mesh.verts_normals_packed()
    assert mesh.verts_normals_packed() is n0  # kept while nothing changes
    _, nrm0, _ = rast.gbuffer(mesh, R, T)
    v.mul_(torch.tensor([1.0, 0.7, 1.2], device=DEV))
    n1 = mesh.verts_normals_packed()
    assert torch.equal(n1, ops.vertex_normals(v, f)) and not torch.equal(n1, n0)
    _, nrm1, _ = rast.gbuffer(mesh, R, T)
    assert torch.equal(nrm1, ops.rasterize_mesh(v, f, n1, R, T, 16, rast.cameras.tan_half_fov())[4])


def _renderer(kind, shadows, rast, R, T, NP):
    from reni_amd.envmap_shader import MicrofacetMaterials, SpatialMaterials
    from reni_amd.mesh import FoVPerspectiveCameras, HipMeshRenderer
    mat = G.e2e_materials(kind, NP)
    cams = FoVPerspectiveCameras(R=R.cpu(), T=T.cpu())  # the rendering camera's centre, (0, 0, 2)
    if kind == "scalar":
        return HipMeshRenderer(rast, kd=mat["kd"], shadows=shadows, shader_cameras=cams)
    cls = SpatialMaterials if kind == "spatial" else MicrofacetMaterials
    return HipMeshRenderer(rast, materials=cls(**mat).to(DEV), shadows=shadows, shader_cameras=cams)


@pytest.mark.parametrize("kind,shadows", G.E2E_CONFIGS, ids=lambda x: str(x))
def test_end_to_end_gradient_through_the_renderer(kind, shadows):
    """d loss / d verts through HipMeshRenderer against the float64 chain: the geometry reference, then the shaders'
    restatements with the positions detached and the device's own face assignment and visibility mask"""
    from reni_amd.mesh import unpack_visibility
    S = G.E2E_S
    v, f, R, T, mesh, rast = _mesh_and_rasterizer(("ico", S), True)
    renderer = _renderer(kind, shadows, rast, R, T, S * S)
    assert torch.allclose(renderer.camera_center, torch.tensor(G.CAMERA_CENTER), atol=1e-6)
    env = _env(1)
    col, normals = renderer(meshes_world=mesh, R=R, T=T, envmap=env)
    w = G.e2e_weights(1, S * S)
    (col.reshape(1, S * S, 3) * w.float().to(DEV)).sum().backward()
    p2f = rast.gbuffer(mesh, R, T, differentiable=False)[0].pix_to_face.reshape(-1).cpu()
    vis = None
    if shadows:
        vis = unpack_visibility(rast.visibility(mesh, R, T, env.directions[0]), env.directions.shape[1]).cpu()
    ref, terms = G.e2e_chain(kind, p2f, vis)
    print(f"end to end {kind} shadows={shadows}: error / (2^-23 sum |terms|) = {G.error_ratio(v.grad, ref, terms):.4g}, "
          f"error / bound = {G.over_bound(v.grad, ref, terms, G.K_E2E):.4g}, max |ref| = {float(ref.abs().max()):.4g}")
    assert (ref != 0).any() and normals.requires_grad
    assert G.over_bound(v.grad, ref, terms, G.K_E2E) <= 1.0


def test_returned_normals_carry_the_gradient():
    """a normal-target loss on the renderer's second output reaches the vertices"""
    from reni_amd.mesh import HipMeshRenderer
    S = 16
    v, f, R, T, mesh, rast = _mesh_and_rasterizer(("ico", S), True)
    _, normals = HipMeshRenderer(rast, kd=1.0)(meshes_world=mesh, R=R, T=T, envmap=_env(1))
    w = torch.randn(1, S, S, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    (normals * w).sum().backward()
    p2f = rast.gbuffer(mesh, R, T, differentiable=False)[0].pix_to_face.reshape(-1).cpu()
    vc, fc = G.case("ico", S)[:2]
    verts = torch.from_numpy(vc).double().requires_grad_(True)
    N, _ = G.gbuffer(verts, torch.from_numpy(fc), R[0].cpu().double(), T[0].cpu().double(), S, E.TANF, p2f)
    (ref,) = torch.autograd.grad((torch.nn.functional.normalize(N, dim=-1, eps=1e-6) * w.reshape(-1, 3).cpu().double()).sum(), verts)
    assert float((v.grad.cpu().double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())


def test_out_of_scope_renderers_raise():
    from reni_amd.glossy import PrefilteredRenderer
    from reni_amd.mesh import FoVPerspectiveCameras, HipMeshRenderer, MeshRasterizer, Meshes, RasterizationSettings
    from reni_amd.textures import TexturedMaterials, TexturedMicrofacetMaterials
    v, f, R, T, _ = _dev(("ico", 16))
    vt = torch.rand(v.shape[0], 2, device=DEV)
    v = v.clone().requires_grad_(True)
    mesh = Meshes(verts=[v], faces=[f], verts_uvs=[vt], faces_uvs=[f])
    rast = MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=16))
    env = _env(1)
    tex = torch.full((8, 8, 3), 0.5)
    for renderer in (HipMeshRenderer(rast, materials=TexturedMaterials(albedo=tex).to(DEV)),
                     HipMeshRenderer(rast, materials=TexturedMicrofacetMaterials(base_color=tex).to(DEV)),
                     PrefilteredRenderer(rast, kd=1.0, out_width=16)):
        with pytest.raises(ValueError, match="vertices require grad"):
            renderer(meshes_world=mesh, R=R.to(DEV), T=T.to(DEV), envmap=env)
    with torch.no_grad():  # nothing is asked of the geometry: the same renderers render
        HipMeshRenderer(rast, materials=TexturedMaterials(albedo=tex).to(DEV))(meshes_world=mesh, R=R.to(DEV), T=T.to(DEV), envmap=env)


def test_a_vertex_fit_recovers_the_sphere():
    """40 Adam steps on the displaced icosphere at S = 32, kd = 1, under a smooth map: the loss (MSE on the pixels covered in
    both the start and the target renders) falls to at most sqrt(rho_ref) of its start, rho_ref the float64 CPU loop's ratio"""
    from reni_amd.mesh import FoVPerspectiveCameras, HipMeshRenderer, MeshRasterizer, Meshes, RasterizationSettings
    rho_ref, _ = G.fit_reference()
    assert rho_ref <= 0.25
    target_v, start_v, f, R, T = G.fit_meshes()
    S = G.FIT_S
    env = _env(1, smooth=True)
    faces = torch.from_numpy(f).to(DEV)
    R, T = R.to(DEV), T.to(DEV)

    def renderer_of(verts):
        mesh = Meshes(verts=[verts], faces=[faces])
        rast = MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=S))
        return mesh, rast, HipMeshRenderer(rast, kd=1.0)

    with torch.no_grad():
        mesh_t, rast_t, rend_t = renderer_of(torch.from_numpy(target_v).to(DEV))
        target, _ = rend_t(meshes_world=mesh_t, R=R, T=T, envmap=env)
        cov_t = rast_t(mesh_t, R=R, T=T).pix_to_face.reshape(-1) >= 0
    verts = torch.from_numpy(start_v).to(DEV).requires_grad_(True)
    mesh, rast, rend = renderer_of(verts)
    mask = (cov_t & (rast(mesh, R=R, T=T).pix_to_face.reshape(-1) >= 0)).reshape(S, S)
    opt = torch.optim.Adam([verts], lr=G.FIT_LR)
    losses = []
    for _ in range(G.FIT_STEPS + 1):
        col, _ = rend(meshes_world=mesh, R=R, T=T, envmap=env)
        loss = ((col - target)[:, mask] ** 2).mean()
        losses.append(float(loss.detach()))
        if len(losses) > G.FIT_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    rho = losses[-1] / losses[0]
    print(f"vertex fit: rho_ref = {rho_ref:.4g}, device ratio = {rho:.4g} (bound sqrt(rho_ref) = {rho_ref ** 0.5:.4g})")
    assert rho <= rho_ref ** 0.5
