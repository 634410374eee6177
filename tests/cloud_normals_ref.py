"""float64 reference of the cloud-neighbourhood unit (reni_tu_knn.hip; ops.knn_points, ops.cloud_normals; the normals of
reni_amd/mesh_losses.py), and the cases.

Everything restates include/reni_hip.h's definitions ("cloud neighbourhoods") in float64 ON THE FLOAT32-ROUNDED INPUTS: ``knn``
(the K + 1 smallest pairs (d, j) of every query by a blockwise stable sort, never more than a block of the N x M matrix),
``normals`` (covariance of the listed neighbours and ``numpy.linalg.eigh``), ``normal_term`` (the chamfer normal term, both
normal gradients and sum |terms|), ``face_normals`` (unit face normals of sampled faces, their vertex gradient and
sum |terms|).  ``normals32`` is the device's written order (list-order mean, fmaf-free moments, 6 cyclic Jacobi sweeps) in
float32 numpy, and ``normal_term`` / ``face_normals`` take a dtype: evaluated in float32 on the CPU they give the error-budget
constants K.  Plain data, numpy and torch on the CPU; nothing here touches a device."""
import functools

import numpy as np
import torch

from tests import mesh_reg_ref as M
from tests import points_ref as P

F64 = torch.float64
U = M.U
DIST_K, MARGIN_K = P.DIST_K, P.MARGIN_K   # the same expression as reni_nearest_points: the same constants
UNDECIDED_CAP = 0.01
GAP_FLOOR = 1e-3          # a point with (l1 - l0) / l2 below this may be left out of the normals' parity (capped at 1 %)
F32_MAX = 3.4028234663852886e38
SWEEPS = 6
# Error-budget constants: 4 x the worst ratio of the float32 CPU evaluation against float64 (``float32_ratios()``;
# tests/test_cloud_normals_cpu.py checks that they still are).  K_E: eigenvalues over 2^-23 l2; K_N: the angle to the reference
# normal over 2^-23 l2 / (l1 - l0); K_FN, K_FNG: sampled face normals and their vertex gradient over 2^-23 sum |terms|;
# K_NT, K_NTG: the chamfer normal term and its normal gradients over 2^-23 sum |terms|.
# Measured worst ratios: eigenvalues 2.4285, angle 1.6230; face normals 0.6793, their gradient 1.2945; term 0.4898, its gradients 2.8977
K_E, K_N = 9.72, 6.50
K_FN, K_FNG = 2.72, 5.18
K_NT, K_NTG = 1.96, 11.6


def case_id(key):
    return "-".join(str(k) for k in key)


# ------------------------------------------------------------------------------------------------------------------ k-NN
# (kind, N, M, K, scale): points_ref's clouds -- one point, M < K, one tile +- 1, one workgroup of queries +- 1 (256 and 512),
# a K that is no bucket, sizes that are sliced, every bucket
KNN_CASES = (tuple(("cube", n, m, k, 1.0) for n, m, k in (
    (1, 1, 1), (5, 3, 8), (257, 255, 8), (300, 1023, 16), (300, 1024, 16), (300, 1025, 16), (511, 700, 4), (512, 700, 4),
    (513, 700, 4), (513, 4097, 5), (1000, 4097, 32), (64, 20000, 32)))
    + (("spheres", 257, 1023, 16, 1e-3), ("spheres", 257, 1023, 16, 1e3)))


def knn_clouds(key):
    kind, n, m, _, scale = key
    return P.nn_clouds((kind, n, m, scale))


def knn(x, y, K, block=128):
    """-> dict: d [N, K + 1] float64 and idx [N, K + 1] int64, the K + 1 smallest pairs (d, j) in ascending lexicographic order
    (a stable sort by d keeps ascending j among equals); a j whose d is NaN or does not fit float32 is not listed, unfilled
    slots hold +inf and -1; und [N]: two consecutive distances among the K + 1 lie within MARGIN_K 2^-23 of each other"""
    x, y = x.to(F64), y.to(F64)
    N, M_ = x.shape[0], y.shape[0]
    W = K + 1
    d = torch.full((N, W), float("inf"), dtype=F64)
    idx = torch.full((N, W), -1, dtype=torch.int64)
    for b in range(0, N, block):
        D = P.dist_matrix(x[b:b + block], y)
        D = torch.where(torch.isfinite(D) & (D <= F32_MAX), D, torch.full_like(D, float("inf")))
        ds, js = torch.sort(D, dim=1, stable=True)
        w = min(W, M_)
        d[b:b + block, :w] = ds[:, :w]
        idx[b:b + block, :w] = js[:, :w]
    idx[~torch.isfinite(d)] = -1
    hi, lo = d[:, 1:], d[:, :-1]
    und = (torch.isfinite(hi) & ((hi - lo) <= MARGIN_K * U * hi)).any(1)
    return {"d": d, "idx": idx, "und": und}


@functools.lru_cache(maxsize=None)
def knn_of(key):
    return knn(*knn_clouds(key), key[3])


def knn_independent(x, y, K):
    """the same lists by a plain loop over the queries and Python's sort of (d, j) tuples: an independent route"""
    x, y = x.to(F64), y.to(F64)
    rows_d, rows_j = [], []
    for i in range(x.shape[0]):
        e = y - x[i]
        dd = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]).tolist()
        pairs = sorted((v, j) for j, v in enumerate(dd) if v == v and v <= F32_MAX)[:K]
        pairs += [(float("inf"), -1)] * (K - len(pairs))
        rows_d.append([p[0] for p in pairs])
        rows_j.append([p[1] for p in pairs])
    return torch.tensor(rows_d, dtype=F64), torch.tensor(rows_j, dtype=torch.int64)


def lattice():
    """x = y = the 9^3 integer lattice: every distance is an exact integer, ties go by the lowest index"""
    r = torch.arange(9, dtype=torch.float32)
    x = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    return x, x.clone()


# ---------------------------------------------------------------------------------------------------------------- normals
NORMAL_CLOUDS = (("sphere", 1500), ("cubesurf", 2000), ("ellipsoid", 1800), ("plane", 1000))
NORMAL_KS = (8, 16, 32)
NORMAL_CASES = tuple((kind, n, k) for kind, n in NORMAL_CLOUDS for k in NORMAL_KS)


@functools.lru_cache(maxsize=None)
def normal_cloud(kind, n):
    """float32 [n, 3]: the unit sphere, the surface of [-1, 1]^3, the ellipsoid (1, 0.7, 0.4), the plane z = 0 with 1 % noise"""
    g = np.random.default_rng(31 + n)
    if kind in ("sphere", "ellipsoid"):
        p = g.normal(size=(n, 3))
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        if kind == "ellipsoid":
            p *= np.array([1.0, 0.7, 0.4])
    elif kind == "cubesurf":
        p = g.uniform(-1.0, 1.0, size=(n, 3))
        axis, side = g.integers(0, 3, size=n), g.integers(0, 2, size=n) * 2.0 - 1.0
        p[np.arange(n), axis] = side
    elif kind == "plane":
        p = g.uniform(-1.0, 1.0, size=(n, 3))
        p[:, 2] = 0.01 * g.normal(size=n)
    else:
        raise KeyError(kind)
    return torch.from_numpy(p.astype(np.float32))


def normals(y, idx):
    """-> dict of float64: eig [N, 3] ascending (clamped at 0), normal [N, 3] (the unit eigenvector of the smallest, sign free),
    count [N]; from the neighbours idx [N, K] lists (a slot of -1 is skipped); fewer than 3: zeros"""
    Y = y.to(F64).numpy()
    J = idx.numpy()
    ok = (J >= 0) & (J < Y.shape[0])
    cnt = ok.sum(1)
    pts = Y[np.clip(J, 0, Y.shape[0] - 1)] * ok[:, :, None]
    mean = pts.sum(1) / np.maximum(cnt, 1)[:, None]
    e = (pts - mean[:, None, :]) * ok[:, :, None]
    C = np.einsum("nka,nkb->nab", e, e) / np.maximum(cnt, 1)[:, None, None]
    w, v = np.linalg.eigh(C)
    few = cnt < 3
    w = np.maximum(w, 0.0)
    nrm = v[:, :, 0].copy()
    w[few] = 0.0
    nrm[few] = 0.0
    return {"eig": torch.from_numpy(w), "normal": torch.from_numpy(nrm), "count": torch.from_numpy(cnt)}


def normals32(y, idx):
    """(normal [N, 3], eig [N, 3]) float32 in the device's written order: mean and moments in list order, ``SWEEPS`` cyclic
    Jacobi sweeps, ascending compare-exchanges, the column of the smallest over its length (an fmaf is a rounded product and a
    rounded sum here); sign free"""
    f = np.float32
    Y = y.numpy().astype(f)
    J = idx.numpy()
    N, K = J.shape
    ok = (J >= 0) & (J < Y.shape[0])
    Jc = np.clip(J, 0, Y.shape[0] - 1)
    s = np.zeros((N, 3), f)
    for k in range(K):
        s = s + Y[Jc[:, k]] * ok[:, k:k + 1].astype(f)
    cnt = ok.sum(1)
    fc = np.maximum(cnt, 1).astype(f)
    m = s / fc[:, None]
    C = np.zeros((N, 3, 3), f)
    for k in range(K):
        e = (Y[Jc[:, k]] - m) * ok[:, k:k + 1].astype(f)
        C = C + e[:, :, None] * e[:, None, :]
    A = C / fc[:, None, None]
    V = np.tile(np.eye(3, dtype=f), (N, 1, 1))
    one = f(1)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                apq = A[:, p, q].copy()
                nz = apq != 0
                theta = (A[:, q, q] - A[:, p, p]) / (f(2) * apq)
                t = np.copysign(one, theta) / (np.abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                sn = t * c
                t, c, sn = np.where(nz, t, f(0)), np.where(nz, c, one), np.where(nz, sn, f(0))
                A[:, p, p] = A[:, p, p] - t * apq
                A[:, q, q] = A[:, q, q] + t * apq
                A[:, p, q] = A[:, q, p] = 0
                arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                A[:, r, p] = A[:, p, r] = c * arp - sn * arq
                A[:, r, q] = A[:, q, r] = sn * arp + c * arq
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = c[:, None] * vp - sn[:, None] * vq
                V[:, :, q] = sn[:, None] * vp + c[:, None] * vq
    w = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1)
    for p, q in ((0, 1), (1, 2), (0, 1)):
        sw = w[:, q] < w[:, p]
        w[sw, p], w[sw, q] = w[sw, q].copy(), w[sw, p].copy()
        V[sw, :, p], V[sw, :, q] = V[sw, :, q].copy(), V[sw, :, p].copy()
    w = np.maximum(w, f(0))
    v = V[:, :, 0]
    nrm = v / np.sqrt(v[:, 2] * v[:, 2] + (v[:, 1] * v[:, 1] + v[:, 0] * v[:, 0]))[:, None]
    few = cnt < 3
    nrm[few] = 0
    w[few] = 0
    return torch.from_numpy(nrm), torch.from_numpy(w)


def angle(a, b):
    """the angle between the lines of a and b [N, 3] (sign free), float64 [N]: asin |a x b| / (|a| |b|)"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    s = torch.cross(a, b, dim=1).norm(dim=1) / (a.norm(dim=1) * b.norm(dim=1)).clamp_min(1e-300)
    return torch.asin(s.clamp(max=1.0))


def normal_ratios(got_n, got_e, ref):
    """(worst eigenvalue error / (2^-23 l2), worst angle / (2^-23 l2 / (l1 - l0)), the share of points left out for a gap ratio
    below GAP_FLOOR, the smallest gap ratio) of a device or float32 evaluation against ``normals``' dict"""
    e = ref["eig"]
    l0, l1, l2 = e[:, 0], e[:, 1], e[:, 2]
    live = ref["count"] >= 3
    re = ((torch.as_tensor(got_e).double() - e).abs().max(1).values / (U * l2).clamp_min(1e-300))[live]
    gap = ((l1 - l0) / l2.clamp_min(1e-300))
    keep = live & (gap >= GAP_FLOOR)
    ra = (angle(got_n, ref["normal"]) / (U * l2 / (l1 - l0).clamp_min(1e-300)))[keep]
    return (float(re.max()) if re.numel() else 0.0, float(ra.max()) if ra.numel() else 0.0,
            float((live & ~keep).float().mean()), float(gap[live].min()) if live.any() else float("inf"))


@functools.lru_cache(maxsize=None)
def normal_case(key):
    """(cloud, the reference's own neighbour lists idx [N, K], ``normals`` of them)"""
    kind, n, k = key
    y = normal_cloud(kind, n)
    idx = knn(y, y, k)["idx"][:, :k].contiguous()
    return y, idx, normals(y, idx)


# --------------------------------------------------------------------------------------------------- the chamfer normal term
NT_CASES = ("cube", "spheres", "star", "r128", "r129", "coincident")
NT_WEIGHTS = ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (0.3, 1.7))
EPS_COS = 1e-6


@functools.lru_cache(maxsize=None)
def nt_normals(name):
    """unit float32 normals for points_ref's chamfer case: random directions (seeded by the sizes)"""
    x, y = P.ch_clouds(name)
    out = []
    for t, seed in ((x, 41), (y, 43)):
        v = np.random.default_rng(seed + t.shape[0]).normal(size=(t.shape[0], 3))
        out.append(torch.from_numpy((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)))
    return tuple(out)


def _cos_parts(a, b, abs_cosine):
    """t = 1 - c(a, b) per row (c the cosine similarity with both norms clamped at EPS_COS, absolute on request), d t / d a,
    d t / d b, and sum |terms| of each"""
    na, nb = a.norm(dim=1).clamp_min(EPS_COS), b.norm(dim=1).clamp_min(EPS_COS)
    dot, adot = (a * b).sum(1), (a.abs() * b.abs()).sum(1)
    c = dot / (na * nb)
    sg = -torch.sign(c) if abs_cosine else -torch.ones_like(c)
    big_a, big_b = (a.norm(dim=1) > EPS_COS).to(a.dtype), (b.norm(dim=1) > EPS_COS).to(a.dtype)
    ga = sg[:, None] * (b / (na * nb)[:, None] - (big_a * dot / (na ** 3 * nb))[:, None] * a)
    gb = sg[:, None] * (a / (na * nb)[:, None] - (big_b * dot / (nb ** 3 * na))[:, None] * b)
    ta = b.abs() / (na * nb)[:, None] + (big_a * adot / (na ** 3 * nb))[:, None] * a.abs()
    tb = a.abs() / (na * nb)[:, None] + (big_b * adot / (nb ** 3 * na))[:, None] * b.abs()
    return 1.0 - (c.abs() if abs_cosine else c), 1.0 + adot / (na * nb), ga, gb, ta, tb


def normal_term(nx, ny, idx_xy, idx_yx, weights=(1.0, 1.0), abs_cosine=True, dtype=F64):
    """value, d / d nx, d / d ny of w_x mean_i (1 - c(nx_i, ny_idx_xy[i])) + w_y mean_j (1 - c(ny_j, nx_idx_yx[j])) with the
    matches held constant, in ``dtype``, each with its sum |terms|"""
    wx, wy = weights
    X, Y = nx.to(dtype), ny.to(dtype)
    N, M_ = X.shape[0], Y.shape[0]
    t1, v1, ga1, gb1, ta1, tb1 = _cos_parts(X, Y[idx_xy], abs_cosine)
    t2, v2, ga2, gb2, ta2, tb2 = _cos_parts(Y, X[idx_yx], abs_cosine)
    cx, cy = torch.tensor(wx / N, dtype=dtype), torch.tensor(wy / M_, dtype=dtype)
    value = torch.tensor(wx, dtype=dtype) * t1.mean() + torch.tensor(wy, dtype=dtype) * t2.mean()
    terms = cx * v1.sum() + cy * v2.sum()
    gx = cx * ga1 + cy * P._seq_rows(idx_yx, gb2, N)
    gy = cy * ga2 + cx * P._seq_rows(idx_xy, gb1, M_)
    gx_terms = cx * ta1 + cy * P._seq_rows(idx_yx, tb2, N)
    gy_terms = cy * ta2 + cx * P._seq_rows(idx_xy, tb1, M_)
    return {"value": value, "value_terms": terms, "gx": gx, "gy": gy, "gx_terms": gx_terms, "gy_terms": gy_terms}


def normal_term_autograd(nx, ny, idx_xy, idx_yx, weights, abs_cosine):
    """the same objective through torch.nn.functional.cosine_similarity and autograd in float64"""
    X, Y = nx.to(F64).requires_grad_(True), ny.to(F64).requires_grad_(True)
    cs = torch.nn.functional.cosine_similarity
    c1, c2 = cs(X, Y[idx_xy], dim=1, eps=EPS_COS), cs(Y, X[idx_yx], dim=1, eps=EPS_COS)
    if abs_cosine:
        c1, c2 = c1.abs(), c2.abs()
    L = weights[0] * (1 - c1).mean() + weights[1] * (1 - c2).mean()
    gx, gy = torch.autograd.grad(L, (X, Y), allow_unused=True)
    z = lambda g, t: torch.zeros_like(t) if g is None else g  # noqa: E731
    return L.detach(), z(gx, X), z(gy, Y)


@functools.lru_cache(maxsize=None)
def nt_of(name, weights=(1.0, 1.0), abs_cosine=True):
    ref = P.chamfer_of(name, (1.0, 1.0))
    nx, ny = nt_normals(name)
    ix, iy = ref["matches"][0]["idx"], ref["matches"][1]["idx"]
    return normal_term(nx, ny, ix, iy, weights, abs_cosine)


# ------------------------------------------------------------------------------------------------------- sampled face normals
FN_MESHES = (("tetra", 8), ("ico", 16), ("bad_faces", 16), ("soup", 17))
EPS_NORM = 2.220446049250313e-16  # sys.float_info.epsilon: pytorch3d's clamp of the normal's length


def face_normals(v, f, face, upstream, dtype=F64):
    """unit normals n [S, 3] of the faces ``face`` [S] (cross(v1 - v0, v2 - v0) over its clamped length), the vertex gradient gv
    [V, 3] of sum(n * upstream), and sum |terms| of both, in ``dtype``"""
    X = v.to(dtype)
    G_ = upstream.to(dtype)
    tri = X[f[face]]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cr = lambda a, b: torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],  # noqa: E731
                                   a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    acr = lambda a, b: torch.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2],  # noqa: E731
                                    a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)
    c = cr(e1, e2)
    c_terms = acr(e1.abs(), e2.abs())
    ln = (c * c).sum(1).sqrt()
    big = (ln > EPS_NORM).to(dtype)[:, None]
    L = ln.clamp_min(EPS_NORM)[:, None]
    n = c / L
    n_terms = c_terms / L + big * n.abs() * (n.abs() * c_terms).sum(1, keepdim=True) / L
    gc = (G_ - big * n * (n * G_).sum(1, keepdim=True)) / L
    gc_terms = (G_.abs() + big * n.abs() * (n.abs() * G_.abs()).sum(1, keepdim=True)) / L
    g1, g2 = cr(e2, gc), cr(gc, e1)
    t1, t2 = acr(e2.abs(), gc_terms), acr(gc_terms, e1.abs())
    index = f[face].t().reshape(-1)  # first corners, second, third
    rows = torch.cat([-(g1 + g2), g1, g2])
    rows_t = torch.cat([t1 + t2, t1, t2])
    V = v.shape[0]
    return {"n": n, "n_terms": n_terms, "gv": P._seq_rows(index, rows, V), "gv_terms": P._seq_rows(index, rows_t, V)}


def face_normals_autograd(v, f, face, upstream):
    X = v.to(F64).requires_grad_(True)
    tri = X[f[face]]
    c = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
    n = c / c.norm(dim=1, keepdim=True).clamp_min(EPS_NORM)
    (g,) = torch.autograd.grad((n * upstream.to(F64)).sum(), X)
    return n.detach(), g


@functools.lru_cache(maxsize=None)
def fn_case(key):
    """(verts, faces, u, upstream, the float64 sampler's dict, ``face_normals`` of its faces)"""
    v, f = P.sample_mesh(key)
    u, up = P.sample_u(), P.sample_upstream(P.sample_u().shape[0], seed=13)
    s = P.sample(v, f, u, up)  # (its own vertex gradient is not used: "und_rows" is)
    return v, f, u, up, s, face_normals(v, f, s["face"], up)


def max_dihedral_cos(v, f):
    """the cosine of the largest angle between the unit normals of two faces that share an edge (a closed 2-manifold)"""
    tri = v.to(F64)[f]
    n = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
    n = n / n.norm(dim=1, keepdim=True)
    owner = {}
    worst = 1.0
    for fi, face in enumerate(f.tolist()):
        for a, b in ((face[0], face[1]), (face[1], face[2]), (face[2], face[0])):
            key = (min(a, b), max(a, b))
            if key in owner:
                worst = min(worst, float((n[fi] * n[owner[key]]).sum()))
            else:
                owner[key] = fi
    return worst


def cube_mesh(h=0.6):
    """the cube [-h, h]^3: 8 vertices, 12 outward-wound triangles (h = 0.6 cuts the unit sphere, h = 1.2 encloses it)"""
    v = torch.tensor([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], dtype=torch.float32)
    f = torch.tensor([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                      [1, 5, 7], [1, 7, 3]], dtype=torch.int64)
    return v, f


def consistency(vp, fp, vt, ft, u):
    """normal consistency between SAMPLES (``geometry_scores(surface=False, normals=True)``) in float64 with the same u for both
    meshes: (pred, true) values, and for each the bound that sums, over the samples, K_FN 2^-23 of both normals' sum |terms|
    and 1 for every sample whose own face, match or matched sample's face is undecided"""
    sp, st = P.sample(vp, fp, u), P.sample(vt, ft, u)
    up0 = torch.zeros(u.shape[0], 3)
    np_, nt = face_normals(vp, fp, sp["face"], up0), face_normals(vt, ft, st["face"], up0)
    out = []
    for a, sa, b, sb in ((np_, sp, nt, st), (nt, st, np_, sp)):
        m = P.nearest(sa["points"].float(), sb["points"].float())  # (the device searches the float32 samples)
        j = m["idx"]
        c = (a["n"] * b["n"][j]).sum(1).abs()
        und = sa["und"] | m["und"] | sb["und"][j]
        rounding = K_FN * U * ((a["n_terms"] * b["n"][j].abs()).sum(1) + (a["n"].abs() * b["n_terms"][j]).sum(1))
        out.append((float(c.mean()), float((torch.where(und, torch.ones_like(c), rounding)).mean())))
    return out


def consistency_surface(vp, fp, vt, ft, u):
    """normal consistency between a sample and the nearest TRIANGLE of the other mesh (``geometry_scores(surface=True,
    normals=True)``) in float64 with the same u for both meshes: (pred, true) values and their bounds.  The match is the
    lowest face among the smallest distances of pointmesh_ref's pair function.  A face whose distance lies within both pairs'
    distance bounds (K_D 2^-23 (s + s_best)) of the smallest is one the device may name instead: the row's bound is the
    largest difference of |cos| over those faces, plus K_FN 2^-23 of both normals' sum |terms|; a sample whose own face is
    undecided counts 1."""
    from tests import pointmesh_ref as PM
    sp, st = P.sample(vp, fp, u), P.sample(vt, ft, u)
    zero = torch.zeros(u.shape[0], 3)
    out = []
    for (sa, va, fa), (vb, fb) in (((sp, vp, fp), (vt, ft)), ((st, vt, ft), (vp, fp))):
        a = face_normals(va, fa, sa["face"], zero)
        b = face_normals(vb, fb, torch.arange(fb.shape[0]), torch.zeros(fb.shape[0], 3))
        A, B, Cc = PM.corners(vb, fb)
        R = PM.pair(sa["points"].float()[:, None, :], A[None], B[None], Cc[None])
        D, S = R["d"].double(), R["s"].double()
        D[:, ~PM.take_part(fb, vb.shape[0])] = float("inf")
        db = D.min(dim=1).values
        first = (D == db[:, None]).to(torch.int64).argmax(dim=1)
        sb = S.gather(1, first[:, None])
        tied = (D - db[:, None]) <= PM.K_D * U * (S + sb)
        c_all = (a["n"][:, None, :] * b["n"][None, :, :]).sum(-1).abs()          # [n, F]
        c = c_all.gather(1, first[:, None])[:, 0]
        spread = torch.where(tied, (c_all - c[:, None]).abs(), torch.zeros_like(c_all)).max(dim=1).values
        rounding = K_FN * U * ((a["n_terms"] * b["n"][first].abs()).sum(1) + (a["n"].abs() * b["n_terms"][first]).sum(1))
        row = torch.where(sa["und"], torch.ones_like(c), spread + rounding)
        out.append((float(c.mean()), float(row.mean()), float((tied.sum(1) > 1).float().mean())))
    return out


# ---------------------------------------------------------------------------------------------------------- the constants
def float32_ratios():
    """(eigenvalues, angle, face normals, their vertex gradient, normal term, its gradients): the worst ratios of the float32
    CPU evaluations against float64, in the units the K_* constants are stated in"""
    we = wa = 0.0
    for key in NORMAL_CASES:
        y, idx, ref = normal_case(key)
        n32, e32 = normals32(y, idx)
        re, ra, _, _ = normal_ratios(n32, e32, ref)
        we, wa = max(we, re), max(wa, ra)
    wn = wg = 0.0
    for key in FN_MESHES:
        v, f, u, up, s, ref = fn_case(key)
        got = face_normals(v, f, s["face"], up, torch.float32)
        wn = max(wn, M.error_ratio(got["n"], ref["n"], ref["n_terms"]))
        wg = max(wg, M.error_ratio(got["gv"], ref["gv"], ref["gv_terms"]))
    wv = wt = 0.0
    for name in NT_CASES:
        nx, ny = nt_normals(name)
        ch = P.chamfer_of(name, (1.0, 1.0))
        ix, iy = ch["matches"][0]["idx"], ch["matches"][1]["idx"]
        for weights in NT_WEIGHTS:
            for ac in (True, False):
                ref = nt_of(name, weights, ac)
                got = normal_term(nx, ny, ix, iy, weights, ac, torch.float32)
                wv = max(wv, M.error_ratio(got["value"].reshape(1), ref["value"].reshape(1), ref["value_terms"].reshape(1)))
                wt = max(wt, M.error_ratio(got["gx"], ref["gx"], ref["gx_terms"]), M.error_ratio(got["gy"], ref["gy"], ref["gy_terms"]))
    return we, wa, wn, wg, wv, wt
