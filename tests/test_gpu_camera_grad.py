"""GPU tests of the camera gradients (reni_tu_camera.hip, k_gb_face<true>, k_sil_face<true>; ops.gbuffer_backward_camera,
ops.soft_silhouette_backward_camera; the autograd nodes and the camera parameterisations of reni_amd.mesh) against the float64
references of tests/camera_grad_ref.py, evaluated with the device's own pix_to_face, vertex normals and trans.

Bounds: max(K 2^-23 sum |terms|, 2e-5 max |ref|) per element, max |ref| over gR, gT and g_tan separately, sum |terms| accumulated
by the reference, K = 4 x the worst ratio of the float32 CPU evaluation over the same cases (K_SIL, K_GBUF, K_E2E of the
reference file; DESIGN 4.4s has the measured figures, the device's among them).  The silhouette's gradient must lie within the
bound of reference_lo widened per element by |reference_hi - reference_lo| (the undecided pairs taken either way), as in
tests/test_gpu_silhouette.py.  Where it does not -- on the device ico-33 sharp alone, 5 undecided pairs of 2129, gR[1][0] =
6.84559 against lo 6.85048 and hi 6.85518, 4.3 2^-23 sum |terms| beyond that widening against K = 3.81 -- it must lie within the
unwidened bound of one of the 2^n mixtures of the undecided pairs' choices (``camera_grad_ref.sil_check``, which says why).
Every test prints its figure, and which of the two assertions it passed, before it asserts."""
import math

import pytest
import torch

from tests import camera_grad_ref as C
from tests import gbuffer_grad_ref as G
from tests import raster_edge_cases as E
from tests import silhouette_ref as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIL_COMBOS = tuple((key, name) for key in S.CASES for name in S.SETTINGS)
DTAN_DFOV = (math.pi / 360.0) / math.cos(math.radians(30.0)) ** 2  # d tan(fov / 2) / d fov at 60 degrees, fov in degrees


def _combo_id(c):
    return S.case_id(c[0]) + "-" + c[1]


def _to_dev(g):
    return None if g is None else g.float().to(DEV)


def _pack(out):
    return C.pack(*(t.detach().double().cpu() for t in out[1:]))


# -------------------------------------------------------------------------------------------------------- the silhouette
def _sil_check(tag, v, f, Rm, T, Simg, name, gA):
    """the camera call on a mesh (numpy) against the references; the equal-bits properties; -> (device tensors, outputs)"""
    from reni_amd import ops
    vd, fd = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    sigma, r = S.setting(name, Simg)
    alpha, trans = ops.soft_silhouette(vd, fd, Rm, T, Simg, E.TANF, sigma, r)
    args = (vd, fd, Rm, T, Simg, E.TANF, sigma, r, trans, gA.float().to(DEV))
    out = ops.soft_silhouette_backward_camera(*args)
    got = _pack(out)
    lo, hi, terms, deltas = C.sil_bounds_of(v, f, Rm, T, Simg, name, gA, trans.double().cpu())
    over, how = C.sil_check(got, lo, hi, terms, deltas)
    print(f"silhouette camera {tag}: error / (2^-23 sum |terms|) = {C.sil_error_ratio(got, lo, hi, terms):.4g}, error / bound = "
          f"{C.sil_over_bound(got, lo, hi, terms):.4g} widened by |hi - lo|; asserted: {over:.4g} by {how} ({deltas.shape[1]} undecided pairs), "
          f"max |ref| = {float(lo.abs().max()):.4g}, max |hi - lo| = {float((hi - lo).abs().max()):.4g}")
    assert out[1].shape == (3, 3) and out[2].shape == (3,) and out[3].shape == () and torch.isfinite(got).all()
    assert over <= 1.0  # no case and no component left out
    # two calls agree; g_verts is the existing entry point's; camera-only mode gives the combined call's bits
    again = ops.soft_silhouette_backward_camera(*args)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    assert torch.equal(out[0], ops.soft_silhouette_backward(*args))
    only = ops.soft_silhouette_backward_camera(*args, need_verts=False)
    assert only[0] is None and all(torch.equal(a, b) for a, b in zip(out[1:], only[1:]))
    return args, alpha, trans, out


@pytest.mark.parametrize("combo", SIL_COMBOS, ids=_combo_id)
def test_silhouette_camera_gradient_matches_the_float64_reference(combo):
    from reni_amd import ops
    key, name = combo
    v, f, Rm, T, Simg = S.case(*key)
    args, alpha, trans, out = _sil_check(_combo_id(combo), v, f, Rm, T, Simg, name, S.upstream(key, name))
    # exact zeros: a zero upstream; nothing in front of the camera; a cover whose trans is 0 everywhere
    zero = ops.soft_silhouette_backward_camera(*args[:-1], torch.zeros_like(args[-1]), need_verts=False)
    assert all((t == 0).all() for t in zero[1:])
    if key[0] == "behind" or (key[0] == "cover" and name != "wide"):
        assert all((t == 0).all() for t in out[1:])
    if key[0] == "cover" and name != "wide":
        assert (trans == 0).all()


def test_silhouette_camera_gradient_is_exactly_zero_where_trans_is_zero():
    """cover-33, wide: an upstream that lives only on the pixels whose trans is 0 gives exactly 0"""
    from reni_amd import ops
    key, name = ("cover", 33), "wide"
    v, f, Rm, T, Simg = S.case(*key)
    vd, fd = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    sigma, r = S.setting(name, Simg)
    _, trans = ops.soft_silhouette(vd, fd, Rm, T, Simg, E.TANF, sigma, r)
    gA = S.upstream(key, name).float().to(DEV)
    gA = torch.where(trans == 0, gA, torch.zeros_like(gA))
    out = ops.soft_silhouette_backward_camera(vd, fd, Rm, T, Simg, E.TANF, sigma, r, trans, gA)
    print(f"cover-33 wide: {int((trans == 0).sum())} of {Simg * Simg} pixels with trans = 0")
    assert (trans == 0).any() and (gA != 0).any() and all((t == 0).all() for t in out)


# -------------------------------------------------------------------------------------------------------- the G-buffer
def _gbuf_check(tag, v, f, Rm, T, Simg, gN, gX):
    from reni_amd import ops
    vd, fd = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    vn = ops.vertex_normals(vd, fd)
    p2f = ops.rasterize_mesh(vd, fd, vn, Rm, T, Simg, E.TANF)[0]
    args = (vd, fd, vn, Rm, T, Simg, p2f, _to_dev(gN), _to_dev(gX))
    out = ops.gbuffer_backward_camera(*args, tan_half_fov=E.TANF)
    got = _pack(out)
    ref, terms = C.gbuf_closed_form(torch.from_numpy(v).double(), torch.from_numpy(f), Rm[0].double(), T[0].double(), Simg, E.TANF,
                                    p2f.reshape(-1).cpu(), gN, gX, vn.double().cpu())
    over = C.over_bound(got, ref, terms, C.K_GBUF)
    print(f"G-buffer camera {tag}: error / (2^-23 sum |terms|) = {C.error_ratio(got, ref, terms):.4g}, error / bound = {over:.4g}, "
          f"max |ref| = {float(ref.abs().max()):.4g}, covered {int((p2f >= 0).sum())}")
    assert out[1].shape == (3, 3) and out[2].shape == (3,) and out[3].shape == () and torch.isfinite(got).all()
    assert over <= 1.0  # no case and no component left out
    again = ops.gbuffer_backward_camera(*args, tan_half_fov=E.TANF)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    assert torch.equal(out[0], ops.gbuffer_backward(*args, tan_half_fov=E.TANF))
    only = ops.gbuffer_backward_camera(*args, tan_half_fov=E.TANF, need_verts=False)
    assert only[0] is None and all(torch.equal(a, b) for a, b in zip(out[1:], only[1:]))
    return args, p2f, out


@pytest.mark.parametrize("variant", G.VARIANTS)
@pytest.mark.parametrize("key", G.CASES, ids=G.case_id)
def test_gbuffer_camera_gradient_matches_the_float64_reference(key, variant):
    from reni_amd import ops
    v, f, Rm, T, Simg = G.case(*key)
    gN, gX = G.upstream(key, variant)
    args, p2f, out = _gbuf_check(f"{G.case_id(key)} {variant}", v, f, Rm, T, Simg, gN, gX)
    # exact zeros: a zero upstream; an all-background scene
    zeros = tuple(None if g is None else torch.zeros_like(g) for g in args[7:])
    zero = ops.gbuffer_backward_camera(*args[:7], *zeros, tan_half_fov=E.TANF, need_verts=False)
    assert all((t == 0).all() for t in zero[1:])
    if key[0] == "behind":
        assert (p2f < 0).all() and all((t == 0).all() for t in out[1:])
    elif key[0] != "cover" or variant != "gN_only":  # (one face, one normal: N_p does not depend on the weights)
        assert any((t != 0).any() for t in out[1:])


# -------------------------------------------------------------------------------------------------------- reducer edges
@pytest.mark.parametrize("F", C.STRIP_F)
def test_reducer_chunk_edges(F):
    """strips of C - 1, C, C + 1 and 2 C + 1 faces at S = 16 (C the reducer's chunk): one launch with a part-filled and a full
    chunk, two launches with a second chunk of one face, and three chunks"""
    v, f, Rm, T, Simg = C.strip_case(F)
    gen = torch.Generator().manual_seed(4000 + F)
    gA = torch.randn(Simg * Simg, generator=gen).double()
    gN, gX = torch.randn(Simg * Simg, 3, generator=gen).double(), torch.randn(Simg * Simg, 3, generator=gen).double()
    # the wide setting: every face has some hundred pixels within its blur radius and next to no pair is undecided
    *_, out = _sil_check(f"strip F={F} wide", v, f, Rm, T, Simg, "wide", gA)
    *_, short = _sil_check(f"strip F={F} wide, without the last face", v, f[:F - 1], Rm, T, Simg, "wide", gA)
    assert not torch.equal(out[1], short[1])  # the last face of the last chunk is in the sum
    _gbuf_check(f"strip F={F} both", v, f, Rm, T, Simg, gN, gX)


# -------------------------------------------------------------------------------------------------------- the errors
def test_c_abi_errors():
    from tests.test_camera_grad_cpu import check_c_abi_errors
    check_c_abi_errors()


# -------------------------------------------------------------------------------------------------------- autograd
def _scene(key, size=None, verts_grad=False, fov=None):
    """(verts, mesh, rasteriser, R [1,3,3], T [1,3] on the host) of a case on the device"""
    from reni_amd.mesh import FoVPerspectiveCameras, MeshRasterizer, Meshes, RasterizationSettings
    v, f, Rm, T, S0 = G.case(*key)
    vd = torch.from_numpy(v).to(DEV).requires_grad_(verts_grad)
    mesh = Meshes(verts=[vd], faces=[torch.from_numpy(f).to(DEV)])
    cams = FoVPerspectiveCameras(device=DEV) if fov is None else FoVPerspectiveCameras(fov=fov, device=DEV)
    return vd, mesh, MeshRasterizer(cams, RasterizationSettings(image_size=size or S0)), Rm, T


def test_autograd_of_leaf_cameras_through_the_silhouette():
    from reni_amd import ops
    key, Simg = ("ico", 16), 16
    sigma, r = S.setting("sharp", Simg)
    w = torch.randn(Simg, Simg, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    v, mesh, rast, R0, T0 = _scene(key)
    f = mesh.faces_packed()
    alpha0, trans = ops.soft_silhouette(v, f, R0, T0, Simg, E.TANF, sigma, r)
    _, gR, gT, g_tan = ops.soft_silhouette_backward_camera(v, f, R0, T0, Simg, E.TANF, sigma, r, trans, w.reshape(-1), need_verts=False)
    assert (gR != 0).any() and (gT != 0).any() and g_tan != 0
    # [1,3,3] / [1,3] on the device and [3,3] / [3] on the host: the gradients come back in those shapes, on those devices
    for R, T in ((R0.to(DEV).clone(), T0.to(DEV).clone()), (R0[0].clone(), T0[0].clone())):
        R.requires_grad_(True), T.requires_grad_(True)
        alpha = rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r)
        assert alpha.requires_grad and not v.requires_grad
        (alpha * w).sum().backward()
        assert R.grad.shape == R.shape and T.grad.shape == T.shape and R.grad.device == R.device
        assert torch.equal(R.grad.reshape(3, 3).to(DEV), gR) and torch.equal(T.grad.reshape(3).to(DEV), gT)
    # T alone: R gets none
    R, T = R0.to(DEV).clone(), T0.to(DEV).clone().requires_grad_(True)
    (rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r) * w).sum().backward()
    assert R.grad is None and torch.equal(T.grad.reshape(3), gT)
    # two views accumulate on one leaf pair; a second rasteriser of another size
    R, T = R0.to(DEV).clone().requires_grad_(True), T0.to(DEV).clone().requires_grad_(True)
    _, _, rast2, _, _ = _scene(key, size=17)
    sigma2, r2 = S.setting("sharp", 17)
    w2 = torch.randn(17, 17, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    _, trans2 = ops.soft_silhouette(v, f, R0, T0, 17, E.TANF, sigma2, r2)
    _, gR2, gT2, _ = ops.soft_silhouette_backward_camera(v, f, R0, T0, 17, E.TANF, sigma2, r2, trans2, w2.reshape(-1), need_verts=False)
    ((rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r) * w).sum()
     + (rast2.silhouette(mesh, R, T, sigma=sigma2, blur_radius=r2) * w2).sum()).backward()
    assert torch.equal(R.grad[0], gR + gR2) and torch.equal(T.grad[0], gT + gT2)
    (rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r) * w).sum().backward()  # ... and over calls
    assert torch.equal(R.grad[0], (gR + gR2) + gR)
    # an in-place edit of R re-rasterises, and so does a new tensor
    before = rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r).detach().clone()
    with torch.no_grad():
        T[0, 2] += 0.3
    after = rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r)
    assert not torch.equal(before, after.detach())
    assert torch.equal(after.detach().reshape(-1), ops.soft_silhouette(v, f, R.detach(), T.detach(), Simg, E.TANF, sigma, r)[0])
    assert torch.equal(rast.silhouette(mesh, R0.to(DEV), T0.to(DEV), sigma=sigma, blur_radius=r).reshape(-1), alpha0)


def test_autograd_of_vertices_camera_and_fov_together():
    from reni_amd import ops
    key, Simg = ("ico", 16), 16
    sigma, r = S.setting("sharp", Simg)
    w = torch.randn(Simg, Simg, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    wN = torch.randn(Simg * Simg, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    wX = torch.randn(Simg * Simg, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(7))
    fov = torch.tensor(60.0, device=DEV, requires_grad=True)
    v, mesh, rast, R0, T0 = _scene(key, verts_grad=True, fov=fov)
    f = mesh.faces_packed()
    R, T = R0.to(DEV).clone().requires_grad_(True), T0.to(DEV).clone().requires_grad_(True)
    tanf = rast.cameras.tan_half_fov()
    assert tanf == E.TANF or abs(tanf - E.TANF) < 1e-7
    # the silhouette
    (rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r) * w).sum().backward()
    _, trans = ops.soft_silhouette(v.detach(), f, R0, T0, Simg, tanf, sigma, r)
    gv, gR, gT, g_tan = ops.soft_silhouette_backward_camera(v.detach(), f, R0, T0, Simg, tanf, sigma, r, trans, w.reshape(-1))
    assert torch.equal(v.grad, gv) and torch.equal(R.grad[0], gR) and torch.equal(T.grad[0], gT)
    assert fov.grad.shape == () and abs(float(fov.grad) - float(g_tan) * DTAN_DFOV) <= 1e-5 * abs(float(g_tan) * DTAN_DFOV)
    # the G-buffer, on the same leaves: everything accumulates
    _, nrm, pos = rast.gbuffer(mesh, R, T)
    assert nrm.requires_grad and pos.requires_grad
    ((nrm * wN).sum() + (pos * wX).sum()).backward()
    vn = mesh._normals_value()
    p2f = rast.gbuffer(mesh, R, T, differentiable=False)[0].pix_to_face
    hv, hR, hT, h_tan = ops.gbuffer_backward_camera(v.detach(), f, vn, R0, T0, Simg, p2f, wN, wX, tan_half_fov=tanf)
    assert torch.equal(v.grad, gv + hv) and torch.equal(R.grad[0], gR + hR) and torch.equal(T.grad[0], gT + hT)
    want = (float(g_tan) + float(h_tan)) * DTAN_DFOV
    assert abs(float(fov.grad) - want) <= 1e-5 * (abs(float(g_tan)) + abs(float(h_tan))) * DTAN_DFOV
    # only the normals' upstream: gX is None inside the node
    R2 = R0.to(DEV).clone().requires_grad_(True)
    (rast.gbuffer(mesh, R2, T.detach())[1] * wN).sum().backward()
    assert torch.equal(R2.grad[0], ops.gbuffer_backward_camera(v.detach(), f, vn, R0, T0, Simg, p2f, wN, None, tan_half_fov=tanf)[1])
    # an optimiser's in-place step on the fov re-rasterises
    a0 = rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r).detach().clone()
    with torch.no_grad():
        fov.sub_(10.0)
    a1 = rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r).detach()
    assert not torch.equal(a0, a1)
    assert torch.equal(a1.reshape(-1), ops.soft_silhouette(v.detach(), f, R0, T0, Simg, rast.cameras.tan_half_fov(), sigma, r)[0])
    assert abs(rast.cameras.tan_half_fov() - math.tan(math.radians(25.0))) < 1e-7


def test_nothing_of_the_camera_requires_grad_nothing_changes():
    """vertices alone: the existing entry points' bits; nothing at all: the cached tensors themselves"""
    from reni_amd import ops
    key, Simg = ("ico", 16), 16
    sigma, r = S.setting("sharp", Simg)
    w = torch.randn(Simg, Simg, device=DEV, generator=torch.Generator(DEV).manual_seed(8))
    wN = torch.randn(Simg * Simg, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
    v, mesh, rast, R0, T0 = _scene(key, verts_grad=True)
    f = mesh.faces_packed()
    R, T = R0.to(DEV), T0.to(DEV)
    (rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r) * w).sum().backward()
    _, trans = ops.soft_silhouette(v.detach(), f, R, T, Simg, E.TANF, sigma, r)
    gs = ops.soft_silhouette_backward(v.detach(), f, R, T, Simg, E.TANF, sigma, r, trans, w.reshape(-1))
    assert torch.equal(v.grad, gs) and R.grad is None
    (rast.gbuffer(mesh, R, T)[1] * wN).sum().backward()
    p2f = rast.gbuffer(mesh, R, T, differentiable=False)[0].pix_to_face
    gg = ops.gbuffer_backward(v.detach(), f, mesh._normals_value(), R, T, Simg, p2f, wN, None, tan_half_fov=E.TANF)
    assert torch.equal(v.grad, gs + gg)
    v0, mesh0, rast0, _, _ = _scene(key)
    a = rast0.silhouette(mesh0, R, T, sigma=sigma, blur_radius=r)
    assert not a.requires_grad and a.grad_fn is None and rast0.silhouette(mesh0, R, T, sigma=sigma, blur_radius=r) is a
    out = rast0.gbuffer(mesh0, R, T)
    assert not out[1].requires_grad and rast0.gbuffer(mesh0, R, T)[1] is out[1]
    Rg = R.clone().requires_grad_(True)
    with torch.no_grad():  # grad disabled: no node either
        assert not rast0.silhouette(mesh0, Rg, T, sigma=sigma, blur_radius=r).requires_grad


def test_a_parameter_behind_look_at_rotation():
    """the camera position as the leaf: R and T come from camera_from_position, the gradient reaches the position and agrees
    with float64 autograd through the restatement"""
    from reni_amd.mesh import camera_from_position
    key, Simg = ("ico", 16), 16
    sigma, r = S.setting("sharp", Simg)
    w = torch.randn(Simg, Simg, generator=torch.Generator().manual_seed(10))
    v, mesh, rast, _, _ = _scene(key)
    pos = C.camera_position(2.2, 15.0, 25.0)
    P = pos.float().to(DEV).requires_grad_(True)
    R, T = camera_from_position(P)
    assert R.device == P.device and R.requires_grad
    (rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r) * w.to(DEV)).sum().backward()
    P64 = pos.clone().requires_grad_(True)
    R64, T64 = camera_from_position(P64)
    vc, fc = G.case(*key)[:2]
    alpha, _ = S.soft_alpha(torch.from_numpy(vc).double(), torch.from_numpy(fc), R64[0], T64[0], Simg, E.TANF, sigma, r)
    (ref,) = torch.autograd.grad((alpha * w.double().reshape(-1)).sum(), P64)
    err = float((P.grad.double().cpu() - ref).abs().max()) / float(ref.abs().max())
    print(f"d loss / d camera position: {P.grad.tolist()} against {ref.tolist()}, relative error {err:.3g}")
    assert (ref != 0).all() and err <= 1e-3  # (float32 R and T: the pose itself is rounded)


def test_out_of_scope_renderers_name_the_camera():
    from tests.test_gpu_gbuffer_grad import _env
    from reni_amd.glossy import PrefilteredRenderer
    from reni_amd.mesh import FoVPerspectiveCameras, HipMeshRenderer, MeshRasterizer, Meshes, RasterizationSettings
    from reni_amd.textures import TexturedMaterials, TexturedMicrofacetMaterials
    v, f, R, T, _ = G.case("ico", 16)
    v, f = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    mesh = Meshes(verts=[v], faces=[f], verts_uvs=[torch.rand(v.shape[0], 2, device=DEV)], faces_uvs=[f])
    rast = MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=16))
    env = _env(1)
    tex = torch.full((8, 8, 3), 0.5)
    Rg = R.to(DEV).clone().requires_grad_(True)
    for renderer in (HipMeshRenderer(rast, materials=TexturedMaterials(albedo=tex).to(DEV)),
                     HipMeshRenderer(rast, materials=TexturedMicrofacetMaterials(base_color=tex).to(DEV)),
                     PrefilteredRenderer(rast, kd=1.0, out_width=16)):
        with pytest.raises(ValueError, match="camera"):
            renderer(meshes_world=mesh, R=Rg, T=T.to(DEV), envmap=env)
        with torch.no_grad():  # nothing is asked of the camera: the same renderers render
            renderer(meshes_world=mesh, R=Rg, T=T.to(DEV), envmap=env)


# ------------------------------------------------------------------------------------------- end to end: the renderer
@pytest.mark.parametrize("kind,shadows", C.E2E_CONFIGS, ids=lambda x: str(x))
def test_end_to_end_camera_gradient_through_the_renderer(kind, shadows):
    """d loss / d (R, T, fov) through HipMeshRenderer against the float64 chain: the shaders' restatements with the positions
    detached and the device's own face assignment, vertex normals and visibility mask, then the camera reference"""
    from tests.test_gpu_gbuffer_grad import _env, _renderer
    from reni_amd.mesh import unpack_visibility
    Simg = G.E2E_S
    fov = torch.tensor(60.0, device=DEV, requires_grad=True)
    v, mesh, rast, R0, T0 = _scene(("ico", Simg), fov=fov)
    R, T = R0.to(DEV).clone().requires_grad_(True), T0.to(DEV).clone().requires_grad_(True)
    renderer = _renderer(kind, shadows, rast, R0.to(DEV), T0.to(DEV), Simg * Simg)
    env = _env(1)
    col, normals = renderer(meshes_world=mesh, R=R, T=T, envmap=env)
    w = G.e2e_weights(1, Simg * Simg)
    (col.reshape(1, Simg * Simg, 3) * w.float().to(DEV)).sum().backward()
    p2f = rast.gbuffer(mesh, R, T, differentiable=False)[0].pix_to_face.reshape(-1).cpu()
    vis = None
    if shadows:
        vis = unpack_visibility(rast.visibility(mesh, R, T, env.directions[0]), env.directions.shape[1]).cpu()
    ref, terms = C.e2e_chain(kind, p2f, vis, normals=mesh._normals_value())
    got = C.pack(R.grad.double().cpu(), T.grad.double().cpu(), fov.grad.double().cpu() / DTAN_DFOV)
    over = C.over_bound(got, ref, terms, C.K_E2E)
    print(f"end to end camera {kind} shadows={shadows}: error / (2^-23 sum |terms|) = {C.error_ratio(got, ref, terms):.4g}, "
          f"error / bound = {over:.4g}, max |ref| = {float(ref.abs().max()):.4g}")
    assert (ref != 0).all() and normals.requires_grad and not v.requires_grad
    assert over <= 1.0


# --------------------------------------------------------------------------------------------------------------- a fit
def test_a_pose_fit_finds_the_camera():
    """60 Adam steps on the camera position (through look_at_rotation) of the squashed icosphere at S = 32, the sharp setting
    and the soft IoU alone, from (3.3, 30, 50) towards (2.7, 10, 20): the device closes at least half the distance the
    float64 CPU loop closes (its start and end are recorded in the reference file)."""
    from reni_amd.mesh import FoVPerspectiveCameras, MeshRasterizer, Meshes, RasterizationSettings, camera_from_position, silhouette_iou
    v, f = C.fit_mesh()
    Simg = C.FIT_S
    sigma, r = S.setting(C.FIT_SETTING, Simg)
    mesh = Meshes(verts=[torch.from_numpy(v).to(DEV)], faces=[torch.from_numpy(f).to(DEV)])
    rast = MeshRasterizer(FoVPerspectiveCameras(device=DEV), RasterizationSettings(image_size=Simg))
    mask = C.fit_mask().to(DEV).reshape(Simg, Simg)
    target = C.camera_position(*C.FIT_TARGET)
    P = C.camera_position(*C.FIT_START).float().to(DEV).requires_grad_(True)
    opt = torch.optim.Adam([P], lr=C.FIT_LR)
    d0 = float((P.detach().double().cpu() - target).norm())
    losses = []
    for _ in range(C.FIT_STEPS + 1):
        R, T = camera_from_position(P)
        loss = silhouette_iou(rast.silhouette(mesh, R, T, sigma=sigma, blur_radius=r), mask)
        losses.append(float(loss.detach()))
        if len(losses) > C.FIT_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    d1 = float((P.detach().double().cpu() - target).norm())
    gain = C.FIT_DIST_START - C.FIT_DIST_END
    print(f"pose fit: |C - C*| {d0:.4f} -> {d1:.4f} (float64 reference {C.FIT_DIST_START:.4f} -> {C.FIT_DIST_END:.4f}), "
          f"loss {losses[0]:.4f} -> {losses[-1]:.4f} (reference {C.FIT_LOSS_START:.4f} -> {C.FIT_LOSS_END:.4f})")
    assert gain > 1.0
    assert d0 - d1 >= 0.5 * gain and losses[-1] < losses[0]
