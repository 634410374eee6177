"""float64 reference of the G-buffer's gradient with respect to the vertex positions (reni_tu_raster_bwd.hip), and the cases.

A torch restatement of reni_tu_raster.hip's projection, barycentric weights, interpolation and vertex normals for a GIVEN
pix_to_face (the face assignment is held fixed); the gradient of sum_p (gN_p . N_p + gX_p . X_p) comes from autograd
(``reference``).  ``closed_form`` is the same gradient written out by hand in the kernels' structure -- per-face sums in NDC,
per-vertex gather, vertex-normal chain -- in any dtype: in float64 it is checked against autograd and accumulates
sum |terms| (the scale of the error bound), in float32 it gives the error-budget constant K.  The face assignment of the CPU
tests is ``np_rasterize``'s (tests/test_raster_cpu.py); the GPU tests pass the device's own.

Plain data and torch on the CPU; nothing here touches a device."""
import functools

import numpy as np
import torch

from tests import raster_edge_cases as E
from tests.test_raster_cpu import np_rasterize, np_vertex_normals

F64 = torch.float64
U = 2.0 ** -23
FLOOR = 2e-5  # of the largest reference value: the project's usual floor
# The error-budget constants: 4 x the worst ratio |float32 closed form - float64| / (2^-23 sum |terms|) that
# ``float32_ratios()`` reaches on the CPU over every case and upstream variant (tests/test_gbuffer_grad_cpu.py checks that
# they still are; DESIGN 4.4p records the measurement and the device's own worst ratios).
K_GVERTS = 1150.0   # 4 x 286.5 (the "bad_faces" case with an upstream for the normals)
K_VNORMALS = 7.5   # 4 x 1.865
VARIANTS = ("both", "gN_only", "gX_only")


# ------------------------------------------------------------------------------------------------------------ the cases
def _icosphere(levels=1):
    from tests.test_gpu_raster import _icosphere as ico
    return ico(levels)


def _tilt(verts, deg=(17.0, 31.0)):
    """a fixed rotation about x then y, so that no edge of a regular solid lines up with the pixel grid"""
    a, b = np.deg2rad(deg[0]), np.deg2rad(deg[1])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    return (np.asarray(verts, np.float64) @ Rx.T @ Ry.T).astype(np.float32)


CASES = (("tetra", 8), ("ico", 15), ("ico", 16), ("ico", 17), ("ico", 33), ("cover", 33), ("fan", 16), ("strip", 255), ("strip", 256),
         ("strip", 257), ("soup", 17), ("unreferenced", 16), ("bad_faces", 16), ("behind", 16), ("tiny_normal", 16))
UNREFERENCED = 5  # the vertex of ("unreferenced", S) that no face names


def case_id(key):
    return "-".join(str(k) for k in key)


@functools.lru_cache(maxsize=None)
def case(kind, arg):
    """-> (verts float32 [V, 3], faces int64 [F, 3], R [1, 3, 3], T [1, 3], S)"""
    R, T = E.camera()
    if kind == "tetra":
        v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * (0.5 / np.sqrt(3))
        return _tilt(v), np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64), R, T, arg
    if kind == "ico":
        v, f = _icosphere(1)
        return _tilt(v), f, R, T, arg
    if kind == "cover":  # one face under all S * S pixels
        v, f, R, T, S, _ = E.scene("cover", arg)
        return v, f, R, T, S
    if kind == "fan":  # 300 faces round vertex 0
        v, f, _, _ = E.normals_mesh("fan")
        return (v * np.float32(0.9)).astype(np.float32), f, R, T, arg
    if kind == "strip":  # V around a block of the per-vertex kernels; the strip starts at the left edge of the view
        v, f = E.strip_mesh(arg)
        v = v.copy()
        v[:, 0] -= np.float32(1.0)
        return v, f, R, T, 33
    if kind == "soup":  # overlapping faces, faces that win no pixel, faces reaching behind the camera, bad indices
        v, f, R, T, S, _ = E.scene("soup", arg)
        return v, f, R, T, S
    if kind == "unreferenced":
        v, f = _icosphere(1)
        v = np.insert(_tilt(v), UNREFERENCED, [[0.1, 0.2, 0.9]], axis=0).astype(np.float32)
        return v, np.where(f >= UNREFERENCED, f + 1, f), R, T, arg
    if kind == "bad_faces":  # bad-index faces, a repeated corner and three corners on a line beside the sphere's good faces
        v, f = _icosphere(1)
        v = np.concatenate([_tilt(v), [[0.0, 0.0, 0.8]], [[0.1, 0.1, 0.8]], [[0.2, 0.2, 0.8]]]).astype(np.float32)
        f = np.concatenate([f[:40], [[0, 1, 45], [-1, 5, 6], [7, 2 ** 40, 8], [3, 3, 9], [42, 43, 44]], f[40:]])
        return v, f.astype(np.int64), R, T, arg
    if kind == "behind":  # everything behind the camera: no pixel is covered
        v, f, R, T, S, _ = E.scene("empty", "behind")
        return v, f, R, T, arg
    if kind == "tiny_normal":  # face 1 is face 0 reversed on copies of its vertices 2 and 1: u_0 = 0 exactly, the max branch
        v = np.array([[0.0, 0.45, 0.1], [-0.4, -0.3, 0.0], [0.45, -0.25, 0.05], [0.45, -0.25, 0.05], [-0.4, -0.3, 0.0],
                      [0.1, -0.6, -0.2]], np.float32)
        return v, np.array([[0, 1, 2], [0, 3, 4], [1, 5, 2]], np.int64), R, T, arg
    raise ValueError(kind)


def upstream(key, variant):
    """(gN, gX), float32-representable float64 tensors [S*S, 3] or None"""
    S = case(*key)[4]
    g = torch.Generator().manual_seed(1000 + CASES.index(key))
    gN = torch.randn(S * S, 3, generator=g).double()
    gX = torch.randn(S * S, 3, generator=g).double()
    return (None if variant == "gX_only" else gN), (None if variant == "gN_only" else gX)


@functools.lru_cache(maxsize=None)
def cpu_pix_to_face(key):
    """np_rasterize's face assignment of a case [S*S] (the CPU tests' stand-in for the device's)"""
    v, f, R, T, S = case(*key)
    out = np_rasterize(v, f, np_vertex_normals(v, f), R[0].double().numpy(), T[0].double().numpy(), S, tan_half=E.TANF)
    return torch.from_numpy(out["pix_to_face"].reshape(-1).copy())


# ------------------------------------------------------------------------------------------- restatement of the forward
def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def vertex_normals(verts, faces):
    """n_v = u_v / max(|u_v|, 1e-6), u_v summed per corner over the faces whose indices are in range (torch, differentiable)"""
    V = verts.shape[0]
    f = faces[((faces >= 0) & (faces < V)).all(dim=1)]
    fn = torch.cross(verts[f[:, 1]] - verts[f[:, 0]], verts[f[:, 2]] - verts[f[:, 0]], dim=1)
    u = torch.zeros_like(verts)
    for k in range(3):
        u = u.index_add(0, f[:, k], fn)
    return u / u.norm(dim=1, keepdim=True).clamp_min(1e-6)


def _valid_faces(verts, faces, R, T, tan_half):
    V = verts.shape[0]
    ok = ((faces >= 0) & (faces < V)).all(dim=1)
    fs = torch.where(ok[:, None], faces, torch.zeros_like(faces))
    q = verts.detach()[fs] @ R + T
    x, y = q[..., 0] / (q[..., 2] * tan_half), q[..., 1] / (q[..., 2] * tan_half)
    area = _edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
    return ok & ~(q[..., 2].max(dim=1).values < 0) & ~(area.abs() <= 1e-8)


def _pixels(S, dtype):
    i = torch.arange(S, dtype=dtype)
    c = -1.0 + (2.0 * (S - 1 - i) + 1.0) / S
    return c[None, :].expand(S, S).reshape(-1), c[:, None].expand(S, S).reshape(-1)  # NDC x of the column, y of the row


def gbuffer(verts, faces, R, T, S, tan_half, pix_to_face, normals=None):
    """(N [S*S, 3], X [S*S, 3]) for the given face assignment (torch, differentiable in verts); normals: the vertex normals
    to interpolate, default ``vertex_normals(verts, faces)``"""
    dtype = verts.dtype
    R, T = R.reshape(3, 3).to(dtype), T.reshape(3).to(dtype)
    F = faces.shape[0]
    n = vertex_normals(verts, faces) if normals is None else normals
    valid = _valid_faces(verts, faces, R, T, tan_half)
    p2f = pix_to_face.reshape(-1)
    hit = (p2f >= 0) & (p2f < F)
    hit = hit & valid[p2f.clamp(0, F - 1)]
    idx = faces[p2f[hit]]  # [Np, 3]
    p = verts[idx]
    q = p @ R + T
    x, y = q[..., 0] / (q[..., 2] * tan_half), q[..., 1] / (q[..., 2] * tan_half)
    PX, PY = _pixels(S, dtype)
    px, py = PX[hit], PY[hit]
    A = _edge(x[:, 2], y[:, 2], x[:, 0], y[:, 0], x[:, 1], y[:, 1]) + 1e-8
    w = torch.stack([_edge(px, py, x[:, 1], y[:, 1], x[:, 2], y[:, 2]), _edge(px, py, x[:, 2], y[:, 2], x[:, 0], y[:, 0]),
                     _edge(px, py, x[:, 0], y[:, 0], x[:, 1], y[:, 1])], 1) / A[:, None]
    N = torch.zeros(S * S, 3, dtype=dtype).index_put((hit.nonzero()[:, 0],), (w[..., None] * n[idx]).sum(1))
    X = torch.zeros(S * S, 3, dtype=dtype).index_put((hit.nonzero()[:, 0],), (w[..., None] * p).sum(1))
    return N, X


def objective(verts, faces, R, T, S, tan_half, pix_to_face, gN, gX):
    N, X = gbuffer(verts, faces, R, T, S, tan_half, pix_to_face)
    out = verts.sum() * 0.0
    if gN is not None:
        out = out + (gN.to(verts.dtype) * N).sum()
    if gX is not None:
        out = out + (gX.to(verts.dtype) * X).sum()
    return out


def reference(key, pix_to_face, gN, gX):
    """g_verts [V, 3] float64 by autograd through the restatement"""
    v, f, R, T, S = case(*key)
    verts = torch.from_numpy(v).double().requires_grad_(True)
    obj = objective(verts, torch.from_numpy(f), R[0].double(), T[0].double(), S, E.TANF, pix_to_face.cpu(), gN, gX)
    (g,) = torch.autograd.grad(obj, verts)
    return g


def vertex_normals_reference(verts, faces, g):
    """d/d verts of sum_v g_v . n_v, float64 autograd"""
    v = torch.as_tensor(verts).double().requires_grad_(True)
    (out,) = torch.autograd.grad((vertex_normals(v, torch.as_tensor(faces)) * g.double()).sum(), v)
    return out


def normals_upstream(key):
    V = case(*key)[0].shape[0]
    return torch.randn(V, 3, generator=torch.Generator().manual_seed(2000 + CASES.index(key))).double()


# -------------------------------------------------------------------------------- the gradient written out by hand
def _cross(a, b):
    return torch.cross(a, b, dim=1)


def _abs_cross(a, b):
    """sum |terms| of cross(a, b) for magnitudes a, b >= 0"""
    return torch.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2],
                        a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)


def vn_closed_form(verts, faces, gn, gn_mag=None):
    """(d/d verts of sum_v gn_v . n_v, sum |terms|) in verts' dtype, in the kernels' structure: g u_v from g n_v, then per
    face G_f = sum of its corners' g u and the cross products to its three corners.  gn_mag: sum |terms| gn itself carries."""
    V = verts.shape[0]
    f = faces[((faces >= 0) & (faces < V)).all(dim=1)]
    p0, p1, p2 = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    a, b = p1 - p0, p2 - p0
    fn = _cross(a, b)
    u = torch.zeros_like(verts)
    for k in range(3):
        u = u.index_add(0, f[:, k], fn)
    ln = u.norm(dim=1, keepdim=True)
    big = ln > 1e-6
    inv = 1.0 / ln.clamp_min(1e-6)
    n = u * inv
    gm = gn.abs() if gn_mag is None else gn_mag
    gu = torch.where(big, (gn - n * (n * gn).sum(1, keepdim=True)) * inv, gn * 1e6)
    gu_m = torch.where(big, (gm + n.abs() * (n.abs() * gm).sum(1, keepdim=True)) * inv, gm * 1e6)
    G = gu[f[:, 0]] + gu[f[:, 1]] + gu[f[:, 2]]
    Gm = gu_m[f[:, 0]] + gu_m[f[:, 1]] + gu_m[f[:, 2]]
    da, db = _cross(b, G), _cross(G, a)
    dam, dbm = _abs_cross(b.abs(), Gm), _abs_cross(Gm, a.abs())
    out = torch.zeros_like(verts).index_add(0, f[:, 1], da).index_add(0, f[:, 2], db).index_add(0, f[:, 0], -(da + db))
    mag = torch.zeros_like(verts).index_add(0, f[:, 1], dam).index_add(0, f[:, 2], dbm).index_add(0, f[:, 0], dam + dbm)
    return out, mag


def closed_form(verts, faces, R, T, S, tan_half, pix_to_face, gN, gX):
    """(g_verts, sum |terms|) [V, 3] each, in verts' dtype: per pixel the contribution to its face's 25 sums, per face the
    fold of dA and (x, y) -> q -> p, per vertex the gather, then the vertex-normal chain.  sum |terms| follows the same chain
    with every addend and every coefficient replaced by its magnitude."""
    dtype = verts.dtype
    R, T = R.reshape(3, 3).to(dtype), T.reshape(3).to(dtype)
    V, F = verts.shape[0], faces.shape[0]
    n = vertex_normals(verts, faces)
    valid = _valid_faces(verts, faces, R, T, tan_half)
    p2f = pix_to_face.reshape(-1)
    hit = (p2f >= 0) & (p2f < F)
    hit = hit & valid[p2f.clamp(0, F - 1)]
    fidx = p2f[hit]
    Np = int(fidx.numel())
    zeros = torch.zeros(S * S, 3, dtype=dtype)
    gn = (zeros if gN is None else gN.to(dtype))[hit]
    gp = (zeros if gX is None else gX.to(dtype))[hit]
    # per face
    safe = torch.where(valid[:, None], faces, torch.zeros_like(faces))
    pf = verts[safe]  # [F, 3, 3]
    qf = pf @ R + T
    xf, yf, zf = qf[..., 0] / (qf[..., 2] * tan_half), qf[..., 1] / (qf[..., 2] * tan_half), qf[..., 2]
    Af = _edge(xf[:, 2], yf[:, 2], xf[:, 0], yf[:, 0], xf[:, 1], yf[:, 1]) + 1e-8
    x, y, A = xf[fidx], yf[fidx], Af[fidx]
    PX, PY = _pixels(S, dtype)
    px, py = PX[hit], PY[hit]
    w = torch.stack([_edge(px, py, x[:, 1], y[:, 1], x[:, 2], y[:, 2]), _edge(px, py, x[:, 2], y[:, 2], x[:, 0], y[:, 0]),
                     _edge(px, py, x[:, 0], y[:, 0], x[:, 1], y[:, 1])], 1) / A[:, None]
    nk, pk = n[safe][fidx], pf[fidx]  # [Np, 3, 3]
    ck = (gn[:, None, :] * nk).sum(2) + (gp[:, None, :] * pk).sum(2)  # [Np, 3]
    ckm = (gn.abs()[:, None, :] * nk.abs()).sum(2) + (gp.abs()[:, None, :] * pk.abs()).sum(2)
    d, dm = ck / A[:, None], ckm / A.abs()[:, None]
    sA = -(ck * w).sum(1) / A
    sAm = (ckm * w.abs()).sum(1) / A.abs()
    gx, gy = torch.zeros(Np, 3, dtype=dtype), torch.zeros(Np, 3, dtype=dtype)
    gxm, gym = torch.zeros(Np, 3, dtype=dtype), torch.zeros(Np, 3, dtype=dtype)
    for k in range(3):
        ia, ib = (k + 1) % 3, (k + 2) % 3
        for (acc, accm, i, coef) in ((gx, gxm, ia, py - y[:, ib]), (gy, gym, ia, x[:, ib] - px), (gx, gxm, ib, y[:, ia] - py),
                                    (gy, gym, ib, px - x[:, ia])):
            acc[:, i] += d[:, k] * coef
            accm[:, i] += dm[:, k] * coef.abs()

    def per_face(t):
        return torch.zeros((F,) + tuple(t.shape[1:]), dtype=dtype).index_add(0, fidx, t)

    GX, GY, SA, GXm, GYm, SAm = (per_face(t) for t in (gx, gy, sA, gxm, gym, sAm))
    WN, WX = per_face(w[:, :, None] * gn[:, None, :]), per_face(w[:, :, None] * gp[:, None, :])  # [F, 3, 3]
    WNm, WXm = per_face(w.abs()[:, :, None] * gn.abs()[:, None, :]), per_face(w.abs()[:, :, None] * gp.abs()[:, None, :])
    direct, directm = torch.zeros(F, 3, 3, dtype=dtype), torch.zeros(F, 3, 3, dtype=dtype)
    for k in range(3):
        i1, i2 = (k + 1) % 3, (k + 2) % 3
        tx = GX[:, k] + SA * (yf[:, i2] - yf[:, i1])
        ty = GY[:, k] + SA * (xf[:, i1] - xf[:, i2])
        txm = GXm[:, k] + SAm * (yf[:, i2] - yf[:, i1]).abs()
        tym = GYm[:, k] + SAm * (xf[:, i1] - xf[:, i2]).abs()
        wz = zf[:, k] * tan_half
        gq = torch.stack([tx / wz, ty / wz, -(tx * xf[:, k] + ty * yf[:, k]) / zf[:, k]], 1)  # [F, 3]
        gqm = torch.stack([txm / wz.abs(), tym / wz.abs(), (txm * xf[:, k].abs() + tym * yf[:, k].abs()) / zf[:, k].abs()], 1)
        direct[:, k] = WX[:, k] + gq @ R.t()
        directm[:, k] = WXm[:, k] + gqm @ R.t().abs()
    direct = torch.where(valid[:, None, None], direct, torch.zeros_like(direct))
    directm = torch.where(valid[:, None, None], directm, torch.zeros_like(directm))
    g, gm = torch.zeros(V, 3, dtype=dtype), torch.zeros(V, 3, dtype=dtype)
    gnv, gnvm = torch.zeros(V, 3, dtype=dtype), torch.zeros(V, 3, dtype=dtype)
    vf = valid.nonzero()[:, 0]
    for k in range(3):
        i = faces[vf, k]
        g, gm = g.index_add(0, i, direct[vf, k]), gm.index_add(0, i, directm[vf, k])
        gnv, gnvm = gnv.index_add(0, i, WN[vf, k]), gnvm.index_add(0, i, WNm[vf, k])
    if gN is not None:
        a, am = vn_closed_form(verts, faces, gnv, gnvm)
        g, gm = g + a, gm + am
    return g, gm


# ------------------------------------------------------------------------------------------------------------ the bound
def bound(ref, terms, K):
    """max(K 2^-23 sum |terms|, 2e-5 max |ref|), elementwise"""
    return (K * U * terms).clamp_min(FLOOR * float(ref.abs().max()) if ref.numel() else 0.0)


def error_ratio(got, ref, terms):
    """worst |got - ref| / (2^-23 sum |terms|); where sum |terms| is 0 the value must be exact (else inf)"""
    err = (torch.as_tensor(got).detach().double().cpu() - ref).abs()
    scale = U * terms.double()
    ratio = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(ratio.max())


def over_bound(got, ref, terms, K):
    """worst |got - ref| / bound; <= 1 passes"""
    err = (torch.as_tensor(got).detach().double().cpu() - ref).abs()
    b = bound(ref, terms.double(), K)
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(ratio.max())


def _inputs(key, dtype):
    v, f, R, T, S = case(*key)
    return torch.from_numpy(v).to(dtype), torch.from_numpy(f), R[0].to(dtype), T[0].to(dtype), S


@functools.lru_cache(maxsize=None)
def scales(key, variant):
    """(float64 closed form, sum |terms|) of a case with the CPU face assignment"""
    gN, gX = upstream(key, variant)
    return closed_form(*_inputs(key, F64), E.TANF, cpu_pix_to_face(key), gN, gX)


@functools.lru_cache(maxsize=None)
def float32_ratios():
    """(worst ratio of g_verts, worst ratio of the vertex-normal backward) of the closed forms evaluated in float32 torch on
    the CPU against float64, over every case and upstream variant, with the CPU face assignment"""
    worst_g = worst_n = 0.0
    for key in CASES:
        v32, f, R32, T32, S = _inputs(key, torch.float32)
        for variant in VARIANTS:
            gN, gX = upstream(key, variant)
            ref, terms = scales(key, variant)
            got, _ = closed_form(v32, f, R32, T32, S, float(np.float32(E.TANF)), cpu_pix_to_face(key), gN, gX)
            worst_g = max(worst_g, error_ratio(got, ref, terms))
        gn = normals_upstream(key)
        ref, terms = vn_closed_form(_inputs(key, F64)[0], f, gn)
        got, _ = vn_closed_form(v32, f, gn.float())
        worst_n = max(worst_n, error_ratio(got, ref, terms))
    return worst_g, worst_n


# ------------------------------------------------------------------------------- end to end: the geometry behind a shader
E2E_S = 16
E2E_CONFIGS = tuple((m, sh) for m in ("scalar", "spatial", "microfacet") for sh in (False, True))
CAMERA_CENTER = (0.0, 0.0, 2.0)  # of E.camera(): the renderers of the end-to-end tests are given it (shader_cameras)
# 4 x the worst ratio of the float32 CPU evaluation of the whole chain (``e2e_float32_ratio``), as K_GVERTS
K_E2E = 1220.0  # 4 x 303.9


def e2e_mesh():
    v, f, R, T, _ = case("ico", E2E_S)
    return v, f, R, T


def envmap_8x16(smooth=False, B=1):
    """(directions [1, 128, 3], colours times sine weight [B, 128, 3]) of an 8 x 16 map, float32-representable float64"""
    from reni_amd.utils import get_directions, get_sineweight
    D, Sw = get_directions(16), get_sineweight(16)
    if smooth:
        d = D[0]
        C = torch.stack([1.0 + 0.8 * d[:, 0], 1.0 + 0.8 * d[:, 1], 1.0 - 0.5 * d[:, 0] + 0.4 * d[:, 2]], 1)[None].expand(B, -1, -1)
    else:
        C = torch.rand(B, D.shape[1], 3, generator=torch.Generator().manual_seed(5)) * 2.0
    return D.float().double(), (C.float() * Sw.float()).float().double()


def e2e_materials(kind, NP):
    """the material inputs of a configuration, float32-representable"""
    g = torch.Generator().manual_seed(11)
    if kind == "scalar":
        return {"kd": 1.0}
    if kind == "spatial":
        return {"albedo": (0.3 + 0.6 * torch.rand(NP, 3, generator=g)).float(), "ks": (0.1 + 0.3 * torch.rand(NP, generator=g)).float(),
                "shininess": (10.0 + 40.0 * torch.rand(NP, generator=g)).float()}
    return {"base_color": (0.3 + 0.6 * torch.rand(NP, 3, generator=g)).float(), "roughness": (0.3 + 0.5 * torch.rand(NP, generator=g)).float(),
            "metallic": (0.8 * torch.rand(NP, generator=g)).float()}


def e2e_weights(B, NP):
    return torch.randn(B, NP, 3, generator=torch.Generator().manual_seed(13)).float().double()


def shade(kind, mat, N, X, D, C, vis, dtype):
    """colours [B, NP, 3] of a configuration from the G-buffer (N, X) by the shaders' float64 restatements, X detached"""
    from tests import microfacet_ref as M
    from tests import shade_materials_ref as SM
    cam = torch.tensor(CAMERA_CENTER, dtype=dtype)
    X = X.detach()
    if kind == "scalar":
        Dd, Sd, _ = SM.shade_terms_ref(N, X, cam, D, C, 500.0, vis=vis, dtype=dtype)
        return SM.compose_ref(Dd, Sd, mat["kd"], 1.0 - mat["kd"], 500.0)
    if kind == "spatial":
        Dd, Sd, _ = SM.shade_terms_ref(N, X, cam, D, C, mat["shininess"].to(dtype), vis=vis, dtype=dtype)
        return SM.compose_ref(Dd, Sd, mat["albedo"].to(dtype), mat["ks"].to(dtype), mat["shininess"].to(dtype))
    r = mat["roughness"].to(dtype).clamp(0.1, 1.0)
    Dd, S0, S1 = M.shade_terms_ggx_ref(N, X, cam, D, C, r * r, vis=vis, dtype=dtype)
    return M.compose_microfacet_ref(Dd, S0, S1, mat["base_color"].to(dtype), mat["metallic"].to(dtype))


def e2e_chain(kind, pix_to_face, vis, dtype=F64):
    """(d loss / d verts, sum |terms|) [V, 3] of loss = sum w . colours through the float restatements in ``dtype``: the
    shader's gradient with respect to the pixel normals by autograd, then ``closed_form`` with it as gN (gX = None: the
    positions are detached).  sum |terms| is the geometry chain's, for that gN."""
    v, f, R, T = e2e_mesh()
    S = E2E_S
    verts, faces = torch.from_numpy(v).to(dtype), torch.from_numpy(f)
    tanh = E.TANF if dtype == F64 else float(np.float32(E.TANF))
    N, X = gbuffer(verts, faces, R[0].to(dtype), T[0].to(dtype), S, tanh, pix_to_face)
    N = N.detach().requires_grad_(True)
    D, C = envmap_8x16()
    col = shade(kind, e2e_materials(kind, S * S), N, X, D.to(dtype), C.to(dtype), vis, dtype)
    (gN,) = torch.autograd.grad((col * e2e_weights(C.shape[0], S * S).to(dtype)).sum(), N)
    return closed_form(verts, faces, R[0].to(dtype), T[0].to(dtype), S, tanh, pix_to_face, gN, None)


@functools.lru_cache(maxsize=None)
def e2e_float32_ratio():
    """worst ratio of the float32 CPU evaluation of the whole chain over the three materials (no mask: the mask is the
    device's), with the CPU face assignment"""
    p2f = cpu_pix_to_face(("ico", E2E_S))
    worst = 0.0
    for kind in ("scalar", "spatial", "microfacet"):
        ref, terms = e2e_chain(kind, p2f, None, F64)
        got, _ = e2e_chain(kind, p2f, None, torch.float32)
        worst = max(worst, error_ratio(got, ref, terms))
    return worst


# ---------------------------------------------------------------------------------------------------------------- a fit
FIT_S, FIT_STEPS, FIT_LR, FIT_AMPLITUDE = 32, 40, 2e-3, 0.04


def fit_meshes():
    """(target verts, start verts, faces, R, T): the icosphere and the same sphere displaced radially by a smooth function of
    FIT_AMPLITUDE of the radius"""
    v, f, R, T, _ = case("ico", FIT_S)
    d = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    bump = np.sin(3.0 * d[:, 0] + 1.0) * np.cos(2.0 * d[:, 1]) + 0.5 * d[:, 2]
    return v, (v.astype(np.float64) * (1.0 + FIT_AMPLITUDE * bump[:, None])).astype(np.float32), f, R, T


def _fit_render(verts, f, R, T, D, C):
    p2f = np_rasterize(verts.detach().numpy(), f, np_vertex_normals(verts.detach().numpy(), f), R[0].double().numpy(),
                       T[0].double().numpy(), FIT_S, tan_half=E.TANF)["pix_to_face"].reshape(-1)
    p2f = torch.from_numpy(p2f.copy())
    N, X = gbuffer(verts, torch.from_numpy(f), R[0].double(), T[0].double(), FIT_S, E.TANF, p2f)
    return shade("scalar", {"kd": 1.0}, N, X, D, C, None, F64), p2f >= 0


@functools.lru_cache(maxsize=None)
def fit_reference():
    """rho_ref: final / initial loss of FIT_STEPS Adam steps in float64 on the CPU (re-rasterised every step, the loss the MSE
    on the pixels covered in both the start and the target renders)"""
    target_v, start_v, f, R, T = fit_meshes()
    D, C = envmap_8x16(smooth=True)
    with torch.no_grad():
        target, cov_t = _fit_render(torch.from_numpy(target_v).double(), f, R, T, D, C)
        _, cov_s = _fit_render(torch.from_numpy(start_v).double(), f, R, T, D, C)
    mask = cov_t & cov_s
    verts = torch.from_numpy(start_v).double().requires_grad_(True)
    opt = torch.optim.Adam([verts], lr=FIT_LR)
    losses = []
    for _ in range(FIT_STEPS + 1):
        col, _ = _fit_render(verts, f, R, T, D, C)
        loss = ((col - target)[:, mask] ** 2).mean()
        losses.append(float(loss.detach()))
        if len(losses) > FIT_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    return losses[-1] / losses[0], losses
