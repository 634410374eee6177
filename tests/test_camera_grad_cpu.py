"""CPU tests of the camera gradients (reni_tu_camera.hip, ops.gbuffer_backward_camera, ops.soft_silhouette_backward_camera, the
camera parameterisations of reni_amd.mesh): the float64 references of tests/camera_grad_ref.py against central differences and
against their own autograd, the error-budget constants and the pinned fit, the parameterisations, and everything of the new
entry points that holds without a GPU (declarations, argument checks, the ISA of the new kernels)."""
import ctypes
import math
import os

import pytest
import torch

from tests import camera_grad_ref as C
from tests import gbuffer_grad_ref as G
from tests import raster_edge_cases as E
from tests import silhouette_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reni_gbuffer_backward_camera_workspace_bytes", "reni_gbuffer_backward_camera",
         "reni_soft_silhouette_backward_camera_workspace_bytes", "reni_soft_silhouette_backward_camera")
CD_CASES = (("ico", 16), ("tetra", 8), ("soup", 17))


# ------------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("key", CD_CASES, ids=S.case_id)
def test_silhouette_autograd_matches_central_differences(key):
    """1e-9 relative on ico-16 sharp, as measured when the feature was specified; the other cases a little looser"""
    name = "sharp"
    v, f, R, T, Simg, tanh = S.inputs(key)
    sigma, r = S.setting(name, Simg)
    gA = S.upstream(key, name)
    with torch.no_grad():
        cd = C.central_differences(lambda R_, T_, t_: C.sil_objective(v, f, R_, T_, Simg, t_, sigma, r, gA), R, T, tanh)
    ref = C.sil_autograd(key, name, gA)
    rel = float((cd - ref).abs().max() / ref.abs().max())
    print(f"silhouette {S.case_id(key)}: central differences vs autograd, relative {rel:.3g}")
    assert (ref != 0).all() and rel <= (1e-9 if key == ("ico", 16) else 1e-7)


@pytest.mark.parametrize("key", CD_CASES, ids=G.case_id)
def test_gbuffer_autograd_matches_central_differences(key):
    v, f, R, T, Simg = G._inputs(key, C.F64)
    gN, gX = G.upstream(key, "both")
    p2f = G.cpu_pix_to_face(key)
    with torch.no_grad():
        cd = C.central_differences(lambda R_, T_, t_: C.gbuf_objective(v, f, R_, T_, Simg, t_, p2f, gN, gX), R, T, E.TANF)
    ref = C.gbuf_autograd(key, p2f, gN, gX)
    rel = float((cd - ref).abs().max() / ref.abs().max())
    print(f"G-buffer {G.case_id(key)}: central differences vs autograd, relative {rel:.3g}")
    assert (ref != 0).all() and rel <= 1e-7


@pytest.mark.parametrize("key", S.CASES, ids=S.case_id)
def test_silhouette_closed_form_matches_autograd_in_float64(key):
    """per element within 1e-12 of sum |terms| (the sums cancel: the result is no scale), both ways for the undecided pairs"""
    for name in S.SETTINGS:
        gA = S.upstream(key, name)
        refs = C.sil_references(key, name, gA)
        for choice, (g, terms) in zip(("lo", "hi"), refs):
            auto = C.sil_autograd(key, name, gA, choice)
            assert ((auto - g).abs() <= 1e-12 * terms).all(), (name, choice)
            assert (terms >= g.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("key", G.CASES, ids=G.case_id)
def test_gbuffer_closed_form_matches_autograd_in_float64(key):
    p2f = G.cpu_pix_to_face(key)
    for variant in G.VARIANTS:
        gN, gX = G.upstream(key, variant)
        g, terms = C.gbuf_reference(key, p2f, gN, gX)
        auto = C.gbuf_autograd(key, p2f, gN, gX)
        assert ((auto - g).abs() <= 1e-12 * terms).all(), variant
        assert (terms >= g.abs() * (1 - 1e-12)).all()


def test_the_gbuffer_camera_gradient_is_the_barycentric_path_alone():
    """given vertex normals enter as constants: the reference with the normals handed in equals the default, and a vertex
    normal scaled by 2 scales a gN-only gradient by 2"""
    key = ("ico", 16)
    v, f, *_ = G._inputs(key, C.F64)
    p2f = G.cpu_pix_to_face(key)
    gN, _ = G.upstream(key, "gN_only")
    n = G.vertex_normals(v, f)
    a, _ = C.gbuf_reference(key, p2f, gN, None)
    b, _ = C.gbuf_reference(key, p2f, gN, None, n)
    c, _ = C.gbuf_reference(key, p2f, gN, None, 2.0 * n)
    assert torch.equal(a, b) and torch.allclose(c, 2.0 * a, rtol=1e-12, atol=0)
    assert ((C.gbuf_autograd(key, p2f, gN, None, 2.0 * n) - c).abs() <= 1e-12 * c.abs().max()).all()


def test_exact_zeros_of_the_references():
    key = ("behind", 16)
    for name in S.SETTINGS:
        (lo, tl), (hi, th) = C.sil_references(key, name, S.upstream(key, name))
        assert (lo == 0).all() and (hi == 0).all() and (tl == 0).all()
    g, terms = C.gbuf_reference(key, G.cpu_pix_to_face(key), *G.upstream(key, "both"))
    assert (g == 0).all() and (terms == 0).all()


def test_error_budget_constants_are_the_measured_ones():
    """K = 4 x the worst ratio of the float32 CPU evaluation, hard-coded in the reference file: still what is measured."""
    rs, rg = C.float32_ratios()
    re2e = C.e2e_float32_ratio()
    print(f"float32 closed forms, worst error / (2^-23 sum |terms|): silhouette {rs:.4g}, G-buffer {rg:.4g}, end to end {re2e:.4g}")
    assert C.K_SIL / 2 <= 4 * rs <= C.K_SIL * 1.001
    assert C.K_GBUF / 2 <= 4 * rg <= C.K_GBUF * 1.001
    assert C.K_E2E / 2 <= 4 * re2e <= C.K_E2E * 1.001


def test_fit_reference_is_the_recorded_one():
    d0, d1, losses = C.fit_reference()
    print(f"float64 pose fit: |C - C*| {d0:.4f} -> {d1:.4f}, loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert abs(d0 - C.FIT_DIST_START) < 1e-6 and abs(d1 - C.FIT_DIST_END) < 1e-6
    assert abs(losses[0] - C.FIT_LOSS_START) < 1e-6 and abs(losses[-1] - C.FIT_LOSS_END) < 1e-6
    assert C.FIT_DIST_END < 0.1 * C.FIT_DIST_START and int(C.fit_mask().sum()) > 50


def test_strip_cases_sit_on_the_reducers_chunk_edges():
    """C is the reducer's chunk, and every face of a strip has pixels within the blur radius: no chunk sums zeros alone"""
    import re
    src = open(os.path.join(ROOT, "reni_amd", "csrc", "reni_internal.h")).read()
    assert int(re.search(r"constexpr int CAM_CHUNK = (\d+);", src).group(1)) == C.CHUNK
    assert C.STRIP_F == (C.CHUNK - 1, C.CHUNK, C.CHUNK + 1, 2 * C.CHUNK + 1)
    F = C.STRIP_F[-1]
    v, f, R, T, Simg = C.strip_case(F)
    assert f.shape == (F, 3) and v.shape == (F + 2, 3)
    sigma, r = S.setting("sharp", Simg)
    with torch.no_grad():
        idx, x, y, _ = S.taking_part(torch.from_numpy(v).double(), torch.from_numpy(f), R[0].double(), T[0].double(), E.TANF)
        near = S.pairs(x, y, Simg, r)["member"].any(dim=0)
    assert idx.numel() == F and bool(near.all())


# --------------------------------------------------------------------------------------------------- the parameterisations
# look_at_view_transform(dist, elev, azim, degrees) of the parent commit: R (9) and T (3) as float32 bit patterns
PARENT_LOOK_AT = {
    (2.0, 0.0, 0.0, True): (0xbf800000, 0x0, 0x80000000, 0x0, 0x3f800000, 0x80000000, 0x0, 0x80000000, 0xbf800000, 0x80000000,
                            0x80000000, 0x40000000),
    (2.7, 10.0, 20.0, True): (0xbf708fb3, 0xbd73442b, 0xbeac7435, 0x0, 0x3f7c1c5d, 0xbe31d0d5, 0x3eaf1d44, 0xbe271798, 0xbf6ce81a,
                              0x80000000, 0x33000000, 0x402ccccc),
    (3.3, 30.0, 50.0, True): (0xbf248dbb, 0xbec41b7d, 0xbf29d57f, 0x0, 0x3f5db3d8, 0xbf000000, 0x3f441b7d, 0xbea48dbb, 0xbf0e81f4,
                              0x34000000, 0xb3800000, 0x40533333),
    (1.0, 90.0, 0.0, True): (0x3f800000, 0x0, 0x0, 0x0, 0x333bbd2e, 0xbf800000, 0x80000000, 0x3f800000, 0x333bbd2e, 0x80000000,
                             0x80000000, 0x3f800000),
    (2.0, -35.0, 200.0, True): (0x3f708fb2, 0xbe48e206, 0x3e8f71fc, 0x0, 0x3f51b3f3, 0x3f12d5e8, 0xbeaf1d44, 0xbf09faf5, 0x3f450e69,
                                0x80000000, 0x80000000, 0x40000000),
    (0.5, 0.0, 180.0, True): (0x3f800000, 0x0, 0x33bbbd2e, 0x0, 0x3f800000, 0x80000000, 0xb3bbbd2e, 0x0, 0x3f800000, 0x80000000,
                              0x80000000, 0x3f000000),
    (1.5, 0.3, -1.2, False): (0xbeb986f2, 0x3e8d0601, 0x3f63f1f9, 0x0, 0x3f7490ef, 0xbe974e6d, 0xbf6e9a1d, 0xbddb4edf, 0xbeb13da8,
                              0x80000000, 0x32e00000, 0x3fbfffff),
}


def test_look_at_view_transform_keeps_the_parents_bits_for_floats():
    from reni_amd.mesh import look_at_view_transform
    for (dist, elev, azim, degrees), bits in PARENT_LOOK_AT.items():
        R, T = look_at_view_transform(dist, elev, azim, degrees=degrees)
        assert R.shape == (1, 3, 3) and T.shape == (1, 3) and R.dtype == torch.float32 and R.device.type == "cpu"
        got = tuple(x & 0xffffffff for x in torch.cat([R.reshape(-1), T.reshape(-1)]).view(torch.int32).tolist())
        assert got == bits, (dist, elev, azim)


def test_look_at_view_transform_keeps_the_graph_of_tensors():
    from reni_amd.mesh import look_at_view_transform
    d = torch.tensor(2.7, requires_grad=True)
    e = torch.tensor(10.0, requires_grad=True)
    a = torch.tensor(20.0, requires_grad=True)
    R, T = look_at_view_transform(d, e, a)
    R0, T0 = look_at_view_transform(2.7, 10.0, 20.0)
    assert torch.equal(R.detach(), R0) and torch.equal(T.detach(), T0) and R.requires_grad and T.requires_grad
    gd, ge, ga = torch.autograd.grad(T[0, 2] + R[0, 0, 2], (d, e, a))
    assert abs(float(gd) - 1.0) < 1e-5 and float(ga) != 0.0  # T = (0, 0, dist); R's last column follows the azimuth
    R1, _ = look_at_view_transform(2.7, e, 20.0)  # one tensor among numbers
    assert R1.requires_grad and torch.equal(R1.detach(), R0)


@pytest.mark.parametrize("pose", [k[:3] for k in PARENT_LOOK_AT if k[3] and k[1] != 90.0])
def test_position_helpers_reproduce_look_at_view_transform(pose):
    from reni_amd.mesh import camera_from_position, look_at_rotation, look_at_view_transform
    R0, T0 = look_at_view_transform(*pose)
    Cw = C.camera_position(*pose)
    R, T = camera_from_position(Cw)
    assert R.dtype == torch.float64 and R.shape == (1, 3, 3) and T.shape == (1, 3)
    assert float((R - R0).abs().max()) <= 2e-7 and float((T - T0).abs().max()) <= 1e-6
    assert torch.equal(look_at_rotation(Cw), R) and torch.equal(look_at_rotation(Cw.reshape(1, 3)), R)
    assert float((Cw @ R[0] + T[0]).abs().max()) <= 1e-15  # the camera's centre is the view-space origin
    # float32 in, float32 out; a position that requires grad gives an R and a T that do
    p = Cw.float().requires_grad_(True)
    R32, T32 = camera_from_position(p)
    assert R32.dtype == torch.float32 and R32.requires_grad and T32.requires_grad
    (g,) = torch.autograd.grad(T32[0, 2], p)
    assert float((g - p.detach() / p.detach().norm()).abs().max()) <= 1e-5  # T_z = |C| when looking at the origin
    # another target and another up vector
    R2 = look_at_rotation(Cw, at=(0.1, -0.2, 0.3), up=(0.0, 0.0, 1.0))
    assert float((R2[0].T @ R2[0] - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-14
    z = (torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64) - Cw)
    assert float((R2[0][:, 2] - z / z.norm()).abs().max()) <= 1e-14


def test_so3_exp_map_is_a_rotation_and_differentiable():
    from reni_amd.mesh import so3_exp_map
    w = torch.tensor([[0.3, -1.2, 0.7], [0.0, 0.0, 0.0], [1e-3, -2e-3, 5e-4], [0.0, math.pi / 2, 0.0], [3.0, 0.5, -0.2]], dtype=torch.float64)
    R = so3_exp_map(w)
    eye = torch.eye(3, dtype=torch.float64)
    assert R.shape == (5, 3, 3) and so3_exp_map(w[0]).shape == (1, 3, 3)
    assert float((R @ R.transpose(1, 2) - eye).abs().max()) <= 1e-14 and float((torch.linalg.det(R) - 1.0).abs().max()) <= 1e-14
    assert torch.equal(R[1], eye)
    assert float((R[3] - torch.tensor([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]], dtype=torch.float64)).abs().max()) <= 1e-15
    assert float((R[0] - torch.linalg.matrix_exp(torch.tensor([[0, -0.7, -1.2], [0.7, 0, -0.3], [1.2, 0.3, 0]], dtype=torch.float64))).abs().max()) <= 1e-14
    for row in w:
        assert torch.autograd.gradcheck(so3_exp_map, (row.clone().requires_grad_(True),))
    # finite at 0, where the derivative is the generator: d R / d w_x = hat(e_x)
    w0 = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(so3_exp_map(w0)[0, 2, 1], w0)
    assert torch.equal(g, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64))
    assert so3_exp_map(torch.zeros(3)).dtype == torch.float32


def test_fov_tensor_is_kept_and_read_at_its_current_value():
    from reni_amd.mesh import FoVPerspectiveCameras
    plain = FoVPerspectiveCameras()
    assert plain.tan_half_fov() == math.tan(math.radians(60.0) / 2.0) and plain.tan_half_fov_tensor() is None
    fov = torch.tensor(60.0, requires_grad=True)
    cams = FoVPerspectiveCameras(fov=fov)
    assert cams.fov is fov and isinstance(cams.tan_half_fov(), float)
    assert abs(cams.tan_half_fov() - plain.tan_half_fov()) < 1e-7
    t = cams.tan_half_fov_tensor()
    (g,) = torch.autograd.grad(t, fov)
    assert abs(float(g) - (math.pi / 360.0) / math.cos(math.radians(30.0)) ** 2) < 1e-7
    with torch.no_grad():
        fov.sub_(10.0)  # an optimiser's step
    assert abs(cams.tan_half_fov() - math.tan(math.radians(25.0))) < 1e-7
    assert FoVPerspectiveCameras(fov=torch.tensor(1.0), degrees=False).tan_half_fov_tensor() is None  # needs no gradient
    assert abs(FoVPerspectiveCameras(fov=torch.tensor(1.0), degrees=False).tan_half_fov() - math.tan(0.5)) < 1e-7
    with pytest.raises(ValueError):
        FoVPerspectiveCameras(fov=torch.tensor([60.0]))


# ------------------------------------------------------------------------------- what holds of the entry points without a GPU
def test_header_and_integration_name_the_entry_points():
    from reni_amd import _lib
    h = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name + "(" in h and name in _lib.EXPORTS and name in doc
    for script in ("build.sh", "isa_core.sh"):
        text = open(os.path.join(ROOT, "reni_amd", "csrc", script)).read()
        assert " camera " in text
    assert "_build/camera.o" in open(os.path.join(ROOT, "reni_amd", "csrc", "build.sh")).read()
    for word in ("gR[i][j]", "g_tan", "grad_camera [13]", "nine free numbers"):
        assert word in h


def test_cpu_tensors_and_bad_shapes_raise():
    from reni_amd import _lib, ops
    v, f = torch.rand(3, 3), torch.tensor([[0, 1, 2]])
    I, Z = torch.eye(3), torch.zeros(3)
    p2f, g = torch.zeros(16, dtype=torch.int64), torch.rand(16, 3)
    for need in (True, False):
        with pytest.raises(_lib.RENILibraryError):
            ops.gbuffer_backward_camera(v, f, v, I, Z, 4, p2f, g, None, need_verts=need)
        with pytest.raises(_lib.RENILibraryError):
            ops.soft_silhouette_backward_camera(v, f, I, Z, 4, 0.5, 1e-3, 1e-2, torch.rand(16), torch.rand(16), need_verts=need)
        with pytest.raises(ValueError):
            ops.gbuffer_backward_camera(v, f, v, I, Z, 4, p2f, None, None, need_verts=need)
        with pytest.raises(ValueError):
            ops.gbuffer_backward_camera(v, f, v, torch.eye(2), Z, 4, p2f, g, None, need_verts=need)
        with pytest.raises(ValueError):
            ops.soft_silhouette_backward_camera(v, f, I, Z, 4, 0.5, 0.0, 1e-2, torch.rand(16), torch.rand(16), need_verts=need)
        with pytest.raises(ValueError):
            ops.soft_silhouette_backward_camera(v, f, I, Z, 4, 0.5, 1e-3, 1e-2, torch.rand(15), torch.rand(16), need_verts=need)


def check_c_abi_errors():
    """Argument checks run before any device work, so they hold with and without a GPU (tests/test_gpu_camera_grad.py runs
    them again beside the device)."""
    from reni_amd import _lib
    lib = _lib.load()
    R, T = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (ctypes.c_float * 3)()
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 255) & ~255
    gb_need = lib.reni_gbuffer_backward_camera_workspace_bytes(3, 1, 8, 8)
    sil_need = lib.reni_soft_silhouette_backward_camera_workspace_bytes(3, 1, 8, 8)
    assert lib.reni_gbuffer_backward_workspace_bytes(3, 1, 8, 8) + 13 * 4 <= gb_need <= 4096
    assert lib.reni_soft_silhouette_backward_workspace_bytes(3, 1, 8, 8) + 13 * 4 <= sil_need <= 4096
    # the chunk sums of the reducer: none up to a chunk of 512 faces, one record per chunk beyond it
    grow = [lib.reni_soft_silhouette_backward_camera_workspace_bytes(3, F, 8, 8) - lib.reni_soft_silhouette_backward_workspace_bytes(3, F, 8, 8)
            for F in (512, 513, 1025)]
    assert grow[0] == 512 * 13 * 4 and grow[1] == ((513 * 13 * 4 + 255) & ~255) + 256 and grow[2] == ((1025 * 13 * 4 + 255) & ~255) + 256
    for fn in (lib.reni_gbuffer_backward_camera_workspace_bytes, lib.reni_soft_silhouette_backward_camera_workspace_bytes):
        assert fn(0, 1, 8, 8) == 0 and fn(3, 0, 8, 8) == 0 and fn(3, 1, 0, 8) == 0

    def gb(V=3, F=1, tanh=0.5, H=8, W=8, ptrs=None, lists=(p, p), gN=p, gX=p, gv=p, gc=p, ws=p, wsn=4096, Rp=R, Tp=T):
        ptrs = [p] * 6 if ptrs is None else ptrs
        return lib.reni_gbuffer_backward_camera(V, F, ptrs[0], ptrs[1], ptrs[2], Rp, Tp, tanh, H, W, ptrs[3], ptrs[4], ptrs[5],
                                                lists[0], lists[1], gN, gX, gv, gc, ws, wsn, None)

    def sil(V=3, F=1, tanh=0.5, H=8, W=8, sigma=1e-3, r=1e-2, ptrs=None, lists=(p, p), gv=p, gc=p, ws=p, wsn=4096, Rp=R, Tp=T):
        ptrs = [p] * 4 if ptrs is None else ptrs
        return lib.reni_soft_silhouette_backward_camera(V, F, ptrs[0], ptrs[1], Rp, Tp, tanh, H, W, sigma, r, ptrs[2], ptrs[3],
                                                        lists[0], lists[1], gv, gc, ws, wsn, None)

    for call, who, n in ((gb, b"gbuffer backward camera:", 6), (sil, b"soft silhouette backward camera:", 4)):
        for kw in (dict(V=0), dict(F=0), dict(H=8, W=9), dict(H=0, W=0), dict(tanh=0.0), dict(tanh=float("nan"))):
            assert call(**kw) == -1 and lib.reni_last_error().startswith(who), kw
        for i in range(n):
            ptrs = [p] * n
            ptrs[i] = None
            assert call(ptrs=ptrs) == -1 and b"NULL" in lib.reni_last_error()
        assert call(Rp=None) == -1 and b"NULL" in lib.reni_last_error()
        assert call(Tp=None) == -1 and b"NULL" in lib.reni_last_error()
        assert call(gc=None) == -1 and lib.reni_last_error().startswith(who) and b"NULL grad_camera" in lib.reni_last_error()
        assert call(gv=None, gc=None) == -1 and b"both NULL" in lib.reni_last_error()
        # grad_verts wants its lists; without it they are not looked at
        assert call(lists=(None, p)) == -1 and b"NULL" in lib.reni_last_error()
        assert call(lists=(p, None)) == -1 and b"NULL" in lib.reni_last_error()
        assert call(ws=None, wsn=0) == -2 and call(wsn=32) == -2 and call(ws=p + 8) == -2  # RENI_EWORKSPACE
        assert call(gv=None, lists=(None, None), wsn=32) == -2  # camera-only: past every argument check
        assert lib.reni_last_error().startswith(who) and b"workspace" in lib.reni_last_error()
    assert gb(gN=None, gX=None) == -1 and b"both upstream" in lib.reni_last_error()
    for kw in (dict(sigma=0.0), dict(sigma=float("nan")), dict(r=-1e-9), dict(r=float("inf"))):
        assert sil(**kw) == -1
    # a workspace that holds the existing entry point's needs but not the camera records
    assert gb(wsn=gb_need - 256 - 64) == -2 and sil(wsn=sil_need - 256 - 64) == -2


def test_c_abi_rejects_bad_sizes_null_pointers_and_short_workspaces():
    check_c_abi_errors()


def _unit_isa(unit):
    import subprocess
    import tempfile
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, unit + ".s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, f"reni_tu_{unit}.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        return open(out).read()


@pytest.mark.parametrize("unit,kernels", [("camera", ("k_cam_reduce",)), ("raster_bwd", ("k_gb_faceILb0E", "k_gb_faceILb1E")),
                                          ("silhouette", ("k_sil_faceILb0E", "k_sil_faceILb1E"))])
def test_new_kernels_isa_audit(unit, kernels):
    """the camera instances of the two face kernels and the reducer with build.sh's flags, through the existing audit
    functions: no MFMA / transcendental -> VALU / SDWA hazard, no scratch"""
    import re
    from tests import isa_audit
    text = _unit_isa(unit)
    for k in kernels:
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text and "atomic" not in text
    sizes = [int(m.group(1)) for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", text)]
    assert sizes and all(s == 0 for s in sizes)
