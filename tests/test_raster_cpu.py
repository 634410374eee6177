"""CPU tests of the mesh pipeline in front of the environment-map shader (reni_amd.mesh, reni_tu_raster.hip).

Holds the float64 numpy restatement of pytorch3d's conventions as the reference uses them (Meshes.verts_normals_packed,
FoVPerspectiveCameras defaults, MeshRasterizer with blur_radius 0, one face per pixel, perspective_correct False, and the
shader's interpolate_face_attributes) that tests/test_gpu_raster.py compares the HIP kernels against, and checks it on
hand-worked cases here."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import isa_audit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")
TAN30 = math.tan(math.pi / 6)
EPS = 1e-8            # pytorch3d kEpsilon
BORDER_WIN = 1e-5     # winner's smallest barycentric below this: the pixel is on an edge, fp32 may pick the neighbour
BORDER_OTHER = 1e-4   # another face's |smallest barycentric| below this: it may or may not cover the pixel in fp32
ZREL = 1e-6           # two candidate depths this close (relative): the fp32 order may differ
# fp32 barycentrics of a face carry an error of up to ~10 u L D / |A| (calibrated on the random soups of test_gpu_raster.py):
# u = 2^-24, L = max(1, largest |NDC coordinate|), D = longest edge, A = NDC area.  A sliver or a face reaching behind the
# camera is ill-conditioned; its tolerances and border bands widen by FP32_K times that bound.
FP32_K = 64.0


# ---------------------------------------------------------------------------------------------------- numpy restatement
def np_vertex_normals(verts, faces):
    """sum over the faces of each vertex of cross(v1 - v0, v2 - v0), then v / max(|v|, 1e-6); faces with an index outside
    [0, V) add nothing."""
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    V = len(verts)
    n = np.zeros((V, 3))
    f = faces[np.all((faces >= 0) & (faces < V), axis=1)]
    fn = np.cross(verts[f[:, 1]] - verts[f[:, 0]], verts[f[:, 2]] - verts[f[:, 0]])
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-6)


def np_project(points, R, T, tan_half=TAN30):
    """world [N,3] -> (NDC x, NDC y, view z): p_view = p R + T; x / (z tan(fov/2)); the z kept is view z; no epsilon."""
    v = np.asarray(points, np.float64) @ np.asarray(R, np.float64).reshape(3, 3) + np.asarray(T, np.float64).reshape(3)
    w = v[:, 2] * tan_half
    with np.errstate(divide="ignore", invalid="ignore"):
        return v[:, 0] / w, v[:, 1] / w, v[:, 2]


def pixel_ndc(S):
    """NDC x of each column and NDC y of each row: +X left, +Y up."""
    i = np.arange(S)
    centre = -1.0 + (2.0 * (S - 1 - i) + 1.0) / S
    return centre, centre  # (x of column c, y of row r)


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _line_d2(px, py, ax, ay, bx, by):
    bax, bay = bx - ax, by - ay
    l2 = bax * bax + bay * bay
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.clip((bax * (px - ax) + bay * (py - ay)) / l2, 0.0, 1.0)
    dx, dy = ax + t * bax - px, ay + t * bay - py
    return np.where(l2 <= EPS, (px - bx) ** 2 + (py - by) ** 2, dx * dx + dy * dy)


def np_rasterize(verts, faces, vnormals, R, T, S, tan_half=TAN30, chunk=128):
    """-> dict of pix_to_face [S,S] (-1 background), zbuf, bary [S,S,3], dists, normals / positions [S*S,3] (the winner's
    interpolation, not normalised; background -1 / 0 as the kernel writes), amb [S,S]: pixels whose winner fp32
    arithmetic may legitimately change (an edge, a near depth tie, a depth near 0), and wtol [S,S]: the winner's fp32
    barycentric error band (FP32_K u L D / |A|; 0 on the background)."""
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    V, F = len(verts), len(faces)
    ok = np.all((faces >= 0) & (faces < V), axis=1)
    fs = np.where(ok[:, None], faces, 0)
    x, y, z = np_project(verts, R, T, tan_half)
    X, Y, Z = x[fs], y[fs], z[fs]  # [F,3]
    area = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    with np.errstate(invalid="ignore"):
        valid = ok & ~(Z.max(axis=1) < 0) & ~(np.abs(area) <= EPS)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        L = np.maximum(1.0, np.maximum(np.abs(X).max(axis=1), np.abs(Y).max(axis=1)))
        D = np.sqrt(np.max([(X[:, i] - X[:, j]) ** 2 + (Y[:, i] - Y[:, j]) ** 2 for i, j in ((0, 1), (1, 2), (0, 2))], axis=0))
        werr = np.where(valid, FP32_K * 2.0 ** -24 * L * D / np.abs(area), 0.0)  # [F]: fp32 error band of a barycentric
    xs, ys = pixel_ndc(S)
    PX = np.broadcast_to(xs[None, :], (S, S)).reshape(-1)
    PY = np.broadcast_to(ys[:, None], (S, S)).reshape(-1)

    def cand(f0, f1):
        sl = slice(f0, f1)
        x0, y0, x1, y1, x2, y2 = (a[sl, None] for a in (X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2]))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            A = _edge(x2, y2, x0, y0, x1, y1) + EPS
            w0 = _edge(PX, PY, x1, y1, x2, y2) / A
            w1 = _edge(PX, PY, x2, y2, x0, y0) / A
            w2 = _edge(PX, PY, x0, y0, x1, y1) / A
            pz = w0 * Z[sl, 0, None] + w1 * Z[sl, 1, None] + w2 * Z[sl, 2, None]
            wmin = np.minimum(w0, np.minimum(w1, w2))
            v = valid[sl, None]
            inside = v & (wmin > 0) & (pz >= 0)
            border = v & (np.abs(wmin) < np.maximum(BORDER_OTHER, werr[sl, None])) & (pz >= -1e-6)
        return w0, w1, w2, pz, wmin, inside, border

    NP = S * S
    best_z = np.full(NP, np.inf)
    best_f = np.full(NP, -1, np.int64)
    best_w = np.full((NP, 3), -1.0)
    for f0 in range(0, F, chunk):
        f1 = min(F, f0 + chunk)
        w0, w1, w2, pz, wmin, inside, _ = cand(f0, f1)
        zc = np.where(inside, pz, np.inf)
        k = np.argmin(zc, axis=0)  # first minimum: the lowest index wins a tie
        zk = zc[k, np.arange(NP)]
        upd = zk < best_z  # strict: an earlier chunk keeps a tie
        best_z[upd] = zk[upd]
        best_f[upd] = f0 + k[upd]
        best_w[upd] = np.stack([w0[k, np.arange(NP)], w1[k, np.arange(NP)], w2[k, np.arange(NP)]], 1)[upd]
    hit = best_f >= 0
    wtol = np.where(hit, werr[np.maximum(best_f, 0)], 0.0)
    amb = hit & (best_w.min(axis=1) < np.maximum(BORDER_WIN, wtol))
    for f0 in range(0, F, chunk):
        f1 = min(F, f0 + chunk)
        _, _, _, pz, _, inside, border = cand(f0, f1)
        me = (np.arange(f0, f1)[:, None] == best_f[None, :])
        zref = np.where(hit, best_z, np.inf)[None, :]
        with np.errstate(invalid="ignore"):
            near = np.abs(pz - zref) <= ZREL * np.abs(zref) + 1e-12
            amb |= np.any(~me & inside & near, axis=0)
            amb |= np.any(~me & border & ((pz <= zref * (1 + ZREL) + 1e-12) | ~hit[None, :]), axis=0)
            amb |= np.any((inside | border) & (np.abs(pz) < 1e-6), axis=0)
    out_n = np.zeros((NP, 3))
    out_p = np.zeros((NP, 3))
    dists = np.full(NP, -1.0)
    vn = np.asarray(vnormals, np.float64)
    if hit.any():
        fi = faces[best_f[hit]]
        w = best_w[hit]
        out_n[hit] = np.einsum("pk,pkd->pd", w, vn[fi])
        out_p[hit] = np.einsum("pk,pkd->pd", w, verts[fi])
        f = best_f[hit]
        px, py = PX[hit], PY[hit]
        d = np.minimum(_line_d2(px, py, X[f, 0], Y[f, 0], X[f, 1], Y[f, 1]),
                       np.minimum(_line_d2(px, py, X[f, 0], Y[f, 0], X[f, 2], Y[f, 2]),
                                  _line_d2(px, py, X[f, 1], Y[f, 1], X[f, 2], Y[f, 2])))
        dists[hit] = -d
    zbuf = np.where(hit, best_z, -1.0)
    return {"pix_to_face": best_f.reshape(S, S), "zbuf": zbuf.reshape(S, S), "bary": best_w.reshape(S, S, 3),
            "dists": dists.reshape(S, S), "normals": out_n, "positions": out_p, "amb": amb.reshape(S, S),
            "wtol": wtol.reshape(S, S)}


def ndc_to_world(ndc_xy, zview, tan_half=TAN30):
    """Inverse of np_project for the identity camera (R = I, T = 0): world points at view depth zview."""
    ndc_xy = np.asarray(ndc_xy, np.float64)
    return np.concatenate([ndc_xy * zview * tan_half, np.full((len(ndc_xy), 1), zview)], axis=1)


I3, Z3 = np.eye(3), np.zeros(3)


# ---------------------------------------------------------------------------------------------------- OBJ loading
def test_obj_parsing_face_syntaxes_polygons_negative_indices(tmp_path):
    from reni_amd.mesh import load_obj
    p = tmp_path / "m.obj"
    p.write_text("""# comment line
o thing
v 0 0 0
v 1 0 0   # trailing comment
v 1 1 0
v 0 1 0
vn 0 0 1
vt 0.5 0.5
f 1 2 3
f 1/1 3/1 4/1
f 1//1 2//1 4//1
f 1/1/1 2/1/1 3/1/1 4/1/1
v 2 0 0
v 2 1 0
f -1 -2 -4 -5 -6
f 2 5 6
""")
    v, f = load_obj(str(p))
    assert v.dtype == torch.float32 and f.dtype == torch.int64
    np.testing.assert_array_equal(v.numpy(), [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0], [2, 1, 0]])
    want = [[0, 1, 2], [0, 2, 3], [0, 1, 3],
            [0, 1, 2], [0, 2, 3],                        # quad: fan (0, 1, 2), (0, 2, 3)
            [5, 4, 2], [5, 2, 1], [5, 1, 0],             # pentagon of negative indices (relative to the 6 vertices read)
            [1, 4, 5]]
    np.testing.assert_array_equal(f.numpy(), want)


def test_obj_errors(tmp_path):
    from reni_amd.mesh import load_obj
    with pytest.raises(FileNotFoundError):
        load_obj(str(tmp_path / "missing.obj"))
    p = tmp_path / "bad.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nf 1 2\n")
    with pytest.raises(ValueError):
        load_obj(str(p))


def test_teapot_fixture():
    from reni_amd.mesh import load_obj
    v, f = load_obj(TEAPOT)
    assert f.shape == (2464, 3) and v.shape[1] == 3
    assert int(f.min()) == 0 and int(f.max()) == v.shape[0] - 1
    vals = np.array([[float(t) for t in ln.split()[1:4]] for ln in open(TEAPOT) if ln.startswith("v ")])
    np.testing.assert_array_equal(v.numpy(), vals.astype(np.float32))
    lo, hi = vals.min(0), vals.max(0)
    np.testing.assert_allclose(np.maximum(-lo, hi), [1.03, 0.5, 0.66], atol=0.03)


# ---------------------------------------------------------------------------------------------------- camera
def test_look_at_and_camera_centres():
    from reni_amd.mesh import FoVPerspectiveCameras, look_at_view_transform
    R, T = look_at_view_transform(2.0, 0.0, 0.0)
    assert R.shape == (1, 3, 3) and T.shape == (1, 3)
    np.testing.assert_allclose(R[0].numpy(), np.diag([-1.0, 1.0, -1.0]), atol=1e-7)
    np.testing.assert_allclose(T[0].numpy(), [0.0, 0.0, 2.0], atol=1e-7)
    cam = FoVPerspectiveCameras()
    np.testing.assert_array_equal(cam.get_camera_center().numpy(), [[0.0, 0.0, 0.0]])  # the shader's (quirk)
    np.testing.assert_allclose(cam.get_camera_center(R, T).numpy(), [[0.0, 0.0, 2.0]], atol=1e-7)
    assert abs(cam.tan_half_fov() - TAN30) < 1e-15
    # elevated / rotated camera: the centre is at distance 2 in the asked direction, looking at the origin
    R2, T2 = look_at_view_transform(2.0, 30.0, 45.0)
    c = cam.get_camera_center(R2, T2)[0].double().numpy()
    e, a = math.radians(30), math.radians(45)
    np.testing.assert_allclose(c, [2 * math.cos(e) * math.sin(a), 2 * math.sin(e), 2 * math.cos(e) * math.cos(a)], atol=1e-6)
    o_view = np.zeros(3) @ R2[0].double().numpy() + T2[0].double().numpy()
    np.testing.assert_allclose(o_view, [0, 0, 2], atol=1e-6)  # the origin lies on the optical axis


def test_rotate_axis_angle_y():
    from reni_amd.mesh import rotate_axis_angle_y
    p = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    np.testing.assert_allclose(rotate_axis_angle_y(p, 90.0).numpy(), [[0, 0, -1], [1, 0, 0], [0, 1, 0]], atol=1e-6)
    assert torch.equal(rotate_axis_angle_y(p, 0.0), p)


def test_projection_of_a_known_point():
    x, y, z = np_project([[0.5, 0.25, 2.0]], I3, Z3)
    np.testing.assert_allclose([x[0], y[0], z[0]], [0.5 / (2 * TAN30), 0.25 / (2 * TAN30), 2.0], rtol=1e-15)
    R = np.diag([-1.0, 1.0, -1.0])
    x, y, z = np_project([[0.5, 0.25, 0.0]], R, [0, 0, 2])  # look_at (2, 0, 0): world +x lands at NDC -x (the right side)
    np.testing.assert_allclose([x[0], y[0], z[0]], [-0.5 / (2 * TAN30), 0.25 / (2 * TAN30), 2.0], rtol=1e-15)


# ---------------------------------------------------------------------------------------------------- rasteriser restatement
def _tri_at(cx, cy, r, z, reverse=False):
    ndc = [[cx - r, cy - r], [cx + r, cy - r], [cx, cy + r]]
    if reverse:
        ndc = ndc[::-1]
    return ndc_to_world(ndc, z)


def test_pixel_centres_and_the_left_right_flip():
    """S = 4: pixel (row 0, col 0) sits at NDC (+0.75, +0.75) -- the top LEFT pixel is at +x."""
    xs, ys = pixel_ndc(4)
    np.testing.assert_allclose(xs, [0.75, 0.25, -0.25, -0.75])
    np.testing.assert_allclose(ys, [0.75, 0.25, -0.25, -0.75])
    v = _tri_at(0.75, 0.75, 0.2, 2.0)
    vn = np_vertex_normals(v, [[0, 1, 2]])
    out = np_rasterize(v, [[0, 1, 2]], vn, I3, Z3, 4)
    want = np.full((4, 4), -1)
    want[0, 0] = 0
    np.testing.assert_array_equal(out["pix_to_face"], want)
    np.testing.assert_allclose(out["bary"][0, 0], [0.25, 0.25, 0.5], atol=1e-6)  # y half way from the base to the apex
    np.testing.assert_allclose(out["zbuf"][0, 0], 2.0, rtol=1e-7)
    np.testing.assert_allclose(out["dists"][0, 0], -(0.04 / math.sqrt(0.2)) ** 2, rtol=1e-6)  # nearest: the slanted edges
    np.testing.assert_allclose(out["positions"][0], [0.75 * 2 * TAN30, 0.75 * 2 * TAN30, 2.0], rtol=1e-6)
    bg = out["pix_to_face"].reshape(-1) < 0
    assert np.all(out["zbuf"].reshape(-1)[bg] == -1) and np.all(out["bary"].reshape(-1, 3)[bg] == -1)
    assert np.all(out["dists"].reshape(-1)[bg] == -1) and np.all(out["normals"][bg] == 0) and np.all(out["positions"][bg] == 0)
    # the mirror image in x lands in the top RIGHT pixel
    out = np_rasterize(_tri_at(-0.75, 0.75, 0.2, 2.0), [[0, 1, 2]], vn, I3, Z3, 4)
    assert out["pix_to_face"][0, 3] == 0 and (out["pix_to_face"] >= 0).sum() == 1


def test_back_facing_triangles_are_kept():
    a = np_rasterize(_tri_at(0.25, -0.25, 0.4, 3.0), [[0, 1, 2]], np.zeros((3, 3)), I3, Z3, 8)
    b = np_rasterize(_tri_at(0.25, -0.25, 0.4, 3.0, reverse=True), [[0, 1, 2]], np.zeros((3, 3)), I3, Z3, 8)
    assert (a["pix_to_face"] == 0).sum() > 4
    np.testing.assert_array_equal(a["pix_to_face"], b["pix_to_face"])
    np.testing.assert_allclose(a["bary"][a["pix_to_face"] == 0], b["bary"][b["pix_to_face"] == 0][:, ::-1], atol=1e-12)


def test_degenerate_and_bad_index_faces_are_skipped():
    v = np.concatenate([_tri_at(0.0, 0.0, 0.5, 2.0), ndc_to_world([[-0.5, -0.5], [0.0, 0.0], [0.5, 0.5]], 2.0)])
    faces = [[3, 4, 5],   # collinear: zero area
             [0, 1, 6],   # index out of range
             [0, -1, 2]]  # negative index
    out = np_rasterize(v, faces, np.zeros((6, 3)), I3, Z3, 16)
    assert np.all(out["pix_to_face"] == -1)
    faces.append([0, 1, 2])
    out = np_rasterize(v, faces, np.zeros((6, 3)), I3, Z3, 16)
    assert set(np.unique(out["pix_to_face"])) == {-1, 3}
    # a face entirely behind the camera is skipped; pixels whose depth is negative are rejected
    out = np_rasterize(_tri_at(0.0, 0.0, 0.5, -2.0), [[0, 1, 2]], np.zeros((3, 3)), I3, Z3, 16)
    assert np.all(out["pix_to_face"] == -1)


def test_nearest_face_wins_and_a_depth_tie_goes_to_the_lower_index():
    near, far = _tri_at(0.0, 0.0, 0.6, 2.0), _tri_at(0.0, 0.0, 0.6, 3.0)
    v = np.concatenate([far, near, near])
    out = np_rasterize(v, [[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.zeros((9, 3)), I3, Z3, 16)
    cov = out["pix_to_face"] >= 0
    assert cov.sum() > 20 and np.all(out["pix_to_face"][cov] == 1)  # nearer than face 0; tied with face 2: the lower
    np.testing.assert_allclose(out["zbuf"][cov], 2.0, rtol=1e-7)  # (A carries + 1e-8)
    out = np_rasterize(v, [[6, 7, 8], [3, 4, 5], [0, 1, 2]], np.zeros((9, 3)), I3, Z3, 16)
    assert np.all(out["pix_to_face"][cov] == 0)


def test_vertex_normals_restatement():
    # a unit square split in two (area-weighted: both halves equal) and a vertex shared with a perpendicular face
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    n = np_vertex_normals(v, [[0, 1, 2], [0, 2, 3], [0, 4, 3]])
    np.testing.assert_allclose(n[1], [0, 0, 1])
    np.testing.assert_allclose(n[2], [0, 0, 1])
    np.testing.assert_allclose(n[4], [-1, 0, 0])
    # vertex 0: (0,0,1) + (0,0,1) from the square halves (each |cross| = 1) + (-1,0,0) from the third -> normalised
    np.testing.assert_allclose(n[0], np.array([-1, 0, 2]) / math.sqrt(5))
    assert np.all(np_vertex_normals(v, [[0, 1, 9]]) == 0)  # an out-of-range face adds nothing


# ---------------------------------------------------------------------------------------------------- no CPU path
def test_cpu_tensors_raise():
    from reni_amd import _lib, ops
    from reni_amd.mesh import build_hip_renderer
    v = torch.rand(3, 3)
    f = torch.tensor([[0, 1, 2]])
    with pytest.raises(_lib.RENILibraryError):
        ops.vertex_normals(v, f)
    with pytest.raises(_lib.RENILibraryError):
        ops.rasterize_mesh(v, f, v, torch.eye(3), torch.zeros(3), 8)
    with pytest.raises(_lib.RENILibraryError):
        build_hip_renderer(TEAPOT, 0, 16, 1.0, "cpu")
    with pytest.raises(FileNotFoundError):
        build_hip_renderer(TEAPOT + ".missing", 0, 16, 1.0, "cuda")


def test_header_declares_the_raster_entry_points():
    from reni_amd import _lib
    h = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    for name in ("reni_raster_workspace_bytes", "reni_mesh_vertex_normals", "reni_rasterize_mesh"):
        assert name + "(" in h and name in _lib.EXPORTS


# ---------------------------------------------------------------------------------------------------- ISA audit
def test_raster_translation_unit_isa_audit():
    """reni_tu_raster.hip with build.sh's flags: no MFMA / transcendental / SDWA hazard, no scratch."""
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "raster.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_raster.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    for k in ("k_vertex_normals", "k_face_setup", "k_raster_tile"):
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text
    for m in __import__("re").finditer(r"\.private_segment_fixed_size:\s*(\d+)", text):
        assert int(m.group(1)) == 0


def test_c_abi_rejects_bad_sizes_and_null_pointers():
    """Argument checks run before any device work, so they hold without a GPU."""
    import ctypes
    from reni_amd import _lib
    lib = _lib.load()
    R, T = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (ctypes.c_float * 3)()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    outs = [p] * 6
    for V, F, H, W, tanh in ((3, 1, 8, 9, 0.5), (0, 1, 8, 8, 0.5), (3, 0, 8, 8, 0.5), (3, 1, 0, 0, 0.5), (3, 1, 8, 8, 0.0)):
        assert lib.reni_rasterize_mesh(V, F, p, p, p, R, T, tanh, H, W, *outs, p, 4096, None) == -1
        assert lib.reni_last_error()
    assert lib.reni_rasterize_mesh(3, 1, p, None, p, R, T, 0.5, 8, 8, *outs, p, 4096, None) == -1
    assert b"NULL" in lib.reni_last_error()
    assert lib.reni_rasterize_mesh(3, 1, p, p, p, R, T, 0.5, 8, 8, *outs, None, 0, None) == -2  # RENI_EWORKSPACE
    assert lib.reni_mesh_vertex_normals(0, 1, p, p, p, p, p, None) == -1
    assert lib.reni_mesh_vertex_normals(3, 1, p, p, None, p, p, None) == -1
    assert lib.reni_raster_workspace_bytes(3, 10, 8, 8) >= 10 * 64 and lib.reni_raster_workspace_bytes(0, 10, 8, 8) == 0
