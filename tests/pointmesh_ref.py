"""Reference of the point-against-mesh unit (reni_tu_pointmesh.hip; ops.nearest_faces, ops.faces_nearest_points;
mesh_losses.nearest_surface, point_mesh_distance, geometry_scores(surface=True)): a float64 restatement of the pair function of
include/reni_hip.h ("points against a mesh") on the float32-rounded inputs, the searches block by block (never more than a block
of the N x F matrix), the closed form of point_mesh_distance's value and gradients with the matches held constant, the same
written order in float32 on the CPU (what the error-budget constants come from), and the cases.  Read-only once computed."""
import functools
import os

import numpy as np
import torch

from tests import mesh_reg_ref as M

F64, F32 = torch.float64, torch.float32
U = M.U
TILE = 256        # PM_TILE: targets staged in LDS at a time
QUERIES = 512     # PM_QUERIES: queries per workgroup
SHORT = 128       # the longest range one lane of the gathers sums alone (CH_SHORT, TX_SHORT)
REGIONS = ("a", "b", "ab", "c", "ac", "bc", "interior")  # in the order they are tested
# Error-budget constants: 4 x the worst ratio of the float32 CPU evaluation (``float32_ratios()``; tests/test_pointmesh_cpu.py
# checks that they still are) over the bounded cases below.
#   dist2:    |d - d_ref| <= K_D 2^-23 s,  s = |p - a|^2 + |ab|^2 + |ac|^2 of the named face     measured worst ratio 8.005
#             (the "small" soups: q = a + v ab + w ac is rounded at the size of the coordinates, about 1, while s is the square
#             of a distance of 0.05 or so; random triangles of the cube reach 0.68, the icosphere 1.30, points on or within 1e-2
#             of their triangle 0.03)
#   weights:  |w - w_ref| <= K_W 2^-23 s^2 / |ab x ac|^2                                          measured worst ratio 0.2189
#   point_mesh_distance: value, points.grad, verts.grad against 2^-23 sum |terms|                 measured 0.4796, 1.3229, 1.4360
K_D, K_W = 32.1, 0.88
K_VALUE, K_GP, K_GV = 1.92, 5.30, 5.75
WEIGHTS = ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0), (0.3, 1.7))
G_UP = 2.5  # the upstream factor of the gradient tests


def case_id(key):
    return "-".join(f"{k:g}" if isinstance(k, float) else str(k) for k in key)


# ------------------------------------------------------------------------------------------------------- the pair function
def _fma(a, b, c):
    """fmaf in float32 (the product of two float32 is exact in double; the sum is rounded to double, then to float: the device's
    bits except where those two roundings disagree with one), a * b + c in float64"""
    if a.dtype == F32:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


def _dot(u, v):
    return _fma(u[..., 2], v[..., 2], _fma(u[..., 1], v[..., 1], u[..., 0] * v[..., 0]))


def pair(p, a, b, c, dtype=F64):
    """The header's pair function, broadcast over the leading dimensions of p, a, b, c [..., 3] (float32 values): a dict of
    v, w, u (the weights of b, c, a), region (an index into REGIONS), q (the closest point), d, and the scales s, cross2."""
    p, a, b, c = (t.to(dtype) for t in (p, a, b, c))
    ab, ac = b - a, c - a
    ap = p - a
    bp, cp = ap - ab, ap - ac
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = _fma(d1, d4, -(d3 * d2)), _fma(d5, d2, -(d1 * d6)), _fma(d3, d6, -(d5 * d4))
    e43, e56 = d4 - d3, d5 - d6
    zero, one = torch.zeros_like(d1), torch.ones_like(d1)
    nv, nw, den = vb, vc, (va + vb) + vc
    region = torch.full(d1.shape, 6, dtype=torch.int64)
    for code, cond, cv, cw, cd in ((5, (va <= 0) & (e43 >= 0) & (e56 >= 0), e56, e43, e43 + e56),
                                   (4, (vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),
                                   (3, (d6 >= 0) & (d5 <= d6), zero, one, one),
                                   (2, (vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),
                                   (1, (d3 >= 0) & (d4 <= d3), one, zero, one),
                                   (0, (d1 <= 0) & (d2 <= 0), zero, zero, one)):  # the last written is the first tested
        nv, nw, den = torch.where(cond, cv, nv), torch.where(cond, cw, nw), torch.where(cond, cd, den)
        region = torch.where(cond, torch.full_like(region, code), region)
    r = one / den
    v = torch.fmin(torch.fmax(nv * r, zero), one)  # (fmaxf: a NaN becomes 0)
    w = torch.fmin(torch.fmax(nw * r, zero), one - v)
    u = (one - v) - w
    q = torch.stack([_fma(w, ac[..., k], _fma(v, ab[..., k], a[..., k] + zero)) for k in range(3)], dim=-1)
    rr = p - q
    d = _fma(rr[..., 2], rr[..., 2], _fma(rr[..., 1], rr[..., 1], rr[..., 0] * rr[..., 0]))
    s = ((ap * ap).sum(-1) + (ab * ab).sum(-1) + (ac * ac).sum(-1)).double()
    cross2 = (torch.linalg.cross(ab.double().expand(*d.shape, 3), ac.double().expand(*d.shape, 3)) ** 2).sum(-1)
    return {"v": v, "w": w, "u": u, "region": region, "q": q, "r": rr, "d": d, "s": s, "cross2": cross2}


def take_part(faces, V):
    """[F] bool: the regularisers' rule -- indices in [0, V), pairwise different"""
    f = torch.as_tensor(faces)
    return (((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2]))


def corners(verts, faces):
    """(a, b, c) [F, 3] float32; a face with an index out of range reads vertex 0 (it takes no part: never used)"""
    f = torch.as_tensor(faces)
    f = torch.where((f >= 0) & (f < verts.shape[0]), f, torch.zeros_like(f))
    return verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]


def pair_rows(points, verts, faces, pi, fi, dtype=F64):
    """``pair`` of the listed (point, face) pairs, one per row"""
    a, b, c = corners(verts, faces)
    return pair(points[pi], a[fi], b[fi], c[fi], dtype)


def _search(points, verts, faces, by_face, dtype):
    """The best target of every query: d (float64, +inf: none), idx (the lowest of the smallest, -1: none).  ``by_face``: the
    queries are the faces and the targets the points."""
    N, F = points.shape[0], faces.shape[0]
    a, b, c = corners(verts, faces)
    part = take_part(faces, verts.shape[0])
    Q, T = (F, N) if by_face else (N, F)
    d = torch.full((Q,), float("inf"), dtype=F64)
    idx = torch.full((Q,), -1, dtype=torch.int64)
    block = max(1, (1 << 19) // T)
    for s in range(0, Q, block):
        e = min(Q, s + block)
        if by_face:
            D = pair(points[None, :, :], a[s:e, None, :], b[s:e, None, :], c[s:e, None, :], dtype)["d"].double()
            D[~part[s:e], :] = float("inf")
        else:
            D = pair(points[s:e, None, :], a[None], b[None], c[None], dtype)["d"].double()
            D[:, ~part] = float("inf")
        D[torch.isnan(D)] = float("inf")  # a NaN wins no comparison
        db = D.min(dim=1).values
        first = (D == db[:, None]).to(torch.int64).argmax(dim=1)  # the lowest index among equal minima
        d[s:e] = db
        idx[s:e] = torch.where(torch.isfinite(db), first, torch.full_like(first, -1))
    return d, idx


def nearest_faces(points, verts, faces, dtype=F64):
    """-> dict: d [N] float64 (+inf: no face), idx [N] (the lowest face among the smallest d; -1), and ``pair_rows`` of the match
    (v, w, u, region, q, s, cross2; rows without a match hold face 0's)"""
    d, idx = _search(points, verts, faces, False, dtype)
    out = pair_rows(points, verts, faces, torch.arange(points.shape[0]), idx.clamp_min(0), dtype)
    out.update({"d": d, "idx": idx})
    return out


def faces_nearest_points(points, verts, faces, dtype=F64):
    """-> the same per FACE: idx [F] is the lowest point among the smallest d(p_i, f)"""
    d, idx = _search(points, verts, faces, True, dtype)
    out = pair_rows(points, verts, faces, idx.clamp_min(0), torch.arange(faces.shape[0]), dtype)
    out.update({"d": d, "idx": idx})
    return out


def dist_bound(row, k=None):
    """K_D 2^-23 s of ``pair`` rows"""
    return (K_D if k is None else k) * U * row["s"]


def weight_bound(row, k=None):
    """K_W 2^-23 s^2 / |ab x ac|^2 of ``pair`` rows (an error of a few 2^-24 s^2 in va, vb, vc over their sum, 4 area^2; an edge's
    quotient has the smaller s / |edge|^2)"""
    return (K_W if k is None else k) * U * row["s"] ** 2 / row["cross2"].clamp_min(1e-300)


# --------------------------------------------------------------------------------------------- point_mesh_distance, closed form
def value_and_grads(points, verts, faces, weights=(1.0, 1.0), matches=None, bary=None, dtype=F64):
    """L = w0 mean_i d(p_i, f_i) + w1 mean_f d(p_{i_f}, f) over the queries with a match, and its gradients with the matches
    (face_of_point [N], point_of_face [F]; -1: none; None: the reference's own) and the barycentrics ((u, v, w) of every point
    [N, 3] and of every face [F, 3]; None: the reference's own for those matches) held constant:
    d L / d p = c 2 r, d L / d (a, b, c) = -c 2 r (u, v, w), r = p - (u a + v b + w c).  -> value, gp [N, 3], gv [V, 3] and the
    sums of the absolute values of the terms of each (value_terms: c (s + sum |r| (|p| + u |a| + v |b| + w |c|)): the scale the
    distances are bounded by, and the products of r r written out).  The weights
    of a thin triangle are ill-conditioned (``weight_bound``), the closed form behind them is not: a comparison passes the
    evaluated side's own weights in, and the weights are bounded where the searches are."""
    w0, w1 = (float(w) for w in weights)
    N, V = points.shape[0], verts.shape[0]
    if matches is None:
        matches = (nearest_faces(points, verts, faces)["idx"], faces_nearest_points(points, verts, faces)["idx"])
    f = torch.as_tensor(faces)
    P, X = points.to(dtype), verts.to(dtype)
    out = {"value": torch.zeros((), dtype=dtype), "value_terms": torch.zeros((), dtype=dtype)}
    for k in ("gp", "gp_terms"):
        out[k] = torch.zeros(N, 3, dtype=dtype)
    for k in ("gv", "gv_terms"):
        out[k] = torch.zeros(V, 3, dtype=dtype)
    for k, (wt, pi, fi) in enumerate(((w0, torch.arange(N), matches[0]), (w1, matches[1], torch.arange(f.shape[0])))):
        keep = (pi >= 0) & (fi >= 0)
        pi, fi = pi[keep], fi[keep]
        if wt == 0.0 or pi.numel() == 0:
            continue
        row = pair_rows(points, verts, faces, pi, fi, dtype)
        if bary is not None:
            given = bary[k][keep].to(dtype)
            row["u"], row["v"], row["w"] = given[:, 0], given[:, 1], given[:, 2]
        c = torch.tensor(wt, dtype=dtype) / pi.numel()
        p = P[pi]
        tri = X[f[fi]]  # [n, 3 corners, 3]
        wgt = torch.stack([row["u"], row["v"], row["w"]], dim=1)  # [n, 3 corners]
        q = (wgt[:, :, None] * tri).sum(1)
        q_terms = (wgt[:, :, None] * tri.abs()).sum(1)
        r, r_terms = p - q, p.abs() + q_terms
        # the value: in float32 the pair function's own d, as the device sums it (q = a + v ab + w ac with its own weights)
        d = row["d"] if dtype == F32 else (r * r).sum(1)
        out["value"] = out["value"] + c * d.sum()
        out["value_terms"] = out["value_terms"] + c * (row["s"].to(dtype) + (r.abs() * r_terms).sum(1)).sum()
        out["gp"].index_add_(0, pi, 2 * c * r)
        out["gp_terms"].index_add_(0, pi, 2 * c * r_terms)
        for k in range(3):
            out["gv"].index_add_(0, f[fi, k], -2 * c * wgt[:, k, None] * r)
            out["gv_terms"].index_add_(0, f[fi, k], 2 * c * wgt[:, k, None] * r_terms)
    out["matches"] = matches
    return out


def own_bary(points, verts, faces, matches, dtype=F64):
    """the (u, v, w) of ``pair`` for the matches, as ``value_and_grads`` takes them: ([N, 3], [F, 3]); rows without a match hold 0"""
    res = []
    for pi, fi in ((torch.arange(points.shape[0]), matches[0]), (matches[1], torch.arange(faces.shape[0]))):
        row = pair_rows(points, verts, faces, pi.clamp_min(0), fi.clamp_min(0), dtype)
        w = torch.stack([row["u"], row["v"], row["w"]], dim=1)
        res.append(torch.where(((pi >= 0) & (fi >= 0))[:, None], w, torch.zeros_like(w)))
    return tuple(res)


# ---------------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def cloud(n, seed, scale=1.0):
    """float32 [n, 3] uniform in [-1, 1]^3, times scale"""
    g = np.random.default_rng(seed)
    return torch.from_numpy((g.uniform(-1.0, 1.0, size=(n, 3)) * scale).astype(np.float32))


@functools.lru_cache(maxsize=None)
def soup(kind, F, seed, scale=1.0):
    """(verts float32 [3 F, 3], faces int64 [F, 3]) of F separate triangles: "big" -- the corners uniform in [-1, 1]^3; "small"
    -- a centre uniform in the cube and corners within 0.02 of it"""
    g = np.random.default_rng(seed)
    if kind == "big":
        v = g.uniform(-1.0, 1.0, size=(F, 3, 3))
    else:
        v = g.uniform(-1.0, 1.0, size=(F, 1, 3)) + 0.02 * g.uniform(-1.0, 1.0, size=(F, 3, 3))
    return torch.from_numpy((v.reshape(3 * F, 3) * scale).astype(np.float32)), torch.arange(3 * F, dtype=torch.int64).reshape(F, 3)


def ico(level):
    from reni_amd.mesh import ico_sphere
    m = ico_sphere(level)
    return m.verts_packed().clone(), m.faces_packed().clone()


# (queries, targets): one of each, one query against several tiles and many workgroups against one target, a tile +- 1, a
# workgroup of queries +- 1, and a size the library slices
SEARCH_SHAPES = ((1, 1), (1, TILE * 4 + 1), (QUERIES * 8 + 1, 1), (300, TILE - 1), (300, TILE), (300, TILE + 1),
                 (QUERIES - 1, 700), (QUERIES, 700), (QUERIES + 1, 700), (64, 20000))
ICO_F = 320  # ico_sphere(2)
# (kind, direction, queries, targets, scale); direction "pf": points are the queries (nearest_faces), "fp": faces are
SEARCH_CASES = (tuple(("big", d, q, t, 1.0) for d in ("pf", "fp") for q, t in SEARCH_SHAPES)
                + tuple((k, d, q, t, 1.0) for k in ("small", "near") for d in ("pf", "fp") for q, t in ((300, TILE + 1), (QUERIES + 1, 700)))
                + tuple(("ico", "pf", q, ICO_F, 1.0) for q in sorted({q for q, _ in SEARCH_SHAPES}))
                + tuple(("ico", "fp", ICO_F, t, 1.0) for t in sorted({t for _, t in SEARCH_SHAPES}))
                + tuple((k, d, *((300, ICO_F) if (k, d) == ("ico", "pf") else (ICO_F, 300) if k == "ico" else (300, TILE + 1)), s)
                        for k in ("big", "ico") for d in ("pf", "fp") for s in (1e-3, 1e3)))


@functools.lru_cache(maxsize=None)
def search_inputs(key):
    """-> (points [N, 3], verts [V, 3], faces [F, 3])"""
    kind, direction, queries, targets, scale = key
    N, F = (queries, targets) if direction == "pf" else (targets, queries)
    if kind == "ico":
        v, f = ico(2)
        assert F == f.shape[0]
        return cloud(N, 11 + N, 1.5 * scale), v * np.float32(scale), f
    v, f = soup("small" if kind == "small" else "big", F, 23 + F, scale)
    if kind != "near":
        return cloud(N, 11 + N, scale), v, f
    # "near": points on a triangle (a third of them, up to the rounding of the combination) or within 1e-2 of it
    g = np.random.default_rng(37 + N)
    tri = v.double().numpy()[f.numpy()[g.integers(0, F, size=N)]]
    w = g.dirichlet(np.ones(3), size=N)
    off = g.normal(size=(N, 3)) * 1e-2 * g.uniform(size=(N, 1)) * (g.uniform(size=(N, 1)) > 1 / 3)
    return torch.from_numpy(((w[:, :, None] * tri).sum(1) + off * scale).astype(np.float32)), v, f


@functools.lru_cache(maxsize=None)
def search_of(key):
    """the float64 reference of a search case, computed once"""
    p, v, f = search_inputs(key)
    return (faces_nearest_points if key[1] == "fp" else nearest_faces)(p, v, f)


def degenerate_mesh():
    """Needles (the third corner within 1e-6 of the opposite edge), exact zero-area faces and coincident corners among a few
    ordinary triangles: checked for valid weights and a finite distance only"""
    g = np.random.default_rng(5)
    tri = g.uniform(-1.0, 1.0, size=(24, 3, 3))
    t = g.uniform(0.1, 0.9, size=(24, 1))
    tri[:8, 2] = tri[:8, 0] + t[:8] * (tri[:8, 1] - tri[:8, 0]) + 1e-6 * g.normal(size=(8, 3))  # needles
    tri[8:12] = np.round(tri[8:12] * 4) / 4
    tri[8:12, 2] = 0.5 * (tri[8:12, 0] + tri[8:12, 1])  # exactly on the edge: no area
    tri[12:16, 1] = tri[12:16, 0]                        # a == b
    tri[16:18, 2] = tri[16:18, 0]                        # a == c
    tri[18:20, 1] = tri[18:20, 2] = tri[18:20, 0]        # a point
    v = torch.from_numpy(tri.reshape(72, 3).astype(np.float32))
    return v, torch.arange(72, dtype=torch.int64).reshape(24, 3)


def region_case():
    """One triangle and a grid of points on both sides of its plane that lands in all seven regions"""
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    x = torch.linspace(-1.0, 2.0, 13)
    p = torch.stack(torch.meshgrid(x, x, torch.tensor([-0.5, 0.5]), indexing="ij"), dim=-1).reshape(-1, 3)
    return p.to(F32), v, torch.tensor([[0, 1, 2]])


SQUARE = torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 2.0, 0.0], [0.0, 2.0, 0.0]])


def tie_points():
    """(1, 1, z), (0, 0, z), (3, 3, z) for z = +-1, +-0.5: on the diagonal's line, so both faces of the split square are at the
    same exactly representable distance"""
    return torch.tensor([[x, x, z] for x in (1.0, 0.0, 3.0) for z in (1.0, -1.0, 0.5, -0.5)])


def tie_faces(swapped=False, repeat=1):
    f = torch.tensor([[0, 2, 3], [0, 1, 2]] if swapped else [[0, 1, 2], [0, 2, 3]])
    return f.repeat(repeat, 1)


@functools.lru_cache(maxsize=None)
def teapot():
    from reni_amd.mesh import load_obj
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "teapot.obj")
    return load_obj(path)


PMD_CASES = ("ico1", "teapot", "bad_faces", "soup", "star80", "star320", "on_vertices")


@functools.lru_cache(maxsize=None)
def pmd_inputs(name):
    """-> (points, verts, faces) of a point_mesh_distance case"""
    if name == "ico1":
        return (cloud(300, 3, 1.5),) + ico(1)
    if name == "teapot":
        v, f = teapot()
        lo, hi = v.min(0).values, v.max(0).values
        return (cloud(1000, 4) * (hi - lo) * 0.6 + (hi + lo) * 0.5).to(F32), v, f
    if name in ("bad_faces", "soup"):
        v, f = M.mesh((name, 16 if name == "bad_faces" else 17))
        v, f = torch.from_numpy(v).clone(), torch.from_numpy(f).clone()
        v[~torch.isfinite(v)] = 0.0
        lo, hi = v.min(0).values, v.max(0).values
        return (cloud(300, 5) * (hi - lo) * 0.6 + (hi + lo) * 0.5).to(F32), v, f
    if name.startswith("star"):  # every face is nearest to point 0, at the centre: its range is F long (80: one lane, 320: the wave)
        v, f = ico(1 if name == "star80" else 2)
        far = cloud(299, 6)
        far = far / far.norm(dim=1, keepdim=True) * 10.0
        return torch.cat([torch.zeros(1, 3), far]).to(F32), v, f
    v, f = ico(1)  # "on_vertices": the points are the vertices
    return v.clone(), v, f


@functools.lru_cache(maxsize=None)
def pmd_of(name, weights=(1.0, 1.0)):
    p, v, f = pmd_inputs(name)
    return value_and_grads(p, v, f, weights)


# ------------------------------------------------------------------------------------------------- the float32 CPU evaluation
def bounded_cases():
    """the search cases the bounds hold on (all of them: the needles are not among them)"""
    return SEARCH_CASES


@functools.lru_cache(maxsize=None)
def float32_ratios():
    """(distance, weights, value, points.grad, verts.grad): the worst ratios of the written order evaluated in float32 on the CPU
    against float64 -- the pair function at the reference's matches of every search case, and the closed form of every
    point_mesh_distance case with every weight pair"""
    rd = rw = 0.0
    for key in bounded_cases():
        p, v, f = search_inputs(key)
        ref = search_of(key)
        keep = ref["idx"] >= 0
        qi = torch.arange(ref["idx"].numel())[keep]
        pi, fi = (ref["idx"][keep], qi) if key[1] == "fp" else (qi, ref["idx"][keep])
        lo, hi = pair_rows(p, v, f, pi, fi, F32), pair_rows(p, v, f, pi, fi, F64)
        rd = max(rd, float(((lo["d"].double() - hi["d"]).abs() / (U * hi["s"])).max()))
        for k in ("v", "w", "u"):
            rw = max(rw, float(((lo[k].double() - hi[k]).abs() / weight_bound(hi, 1.0)).max()))
    rv = rp = rg = 0.0
    for name in PMD_CASES:
        p, v, f = pmd_inputs(name)
        for weights in WEIGHTS:
            matches = pmd_of(name)["matches"]
            bary = own_bary(p, v, f, matches, F32)  # the evaluated side's own weights, held constant on both sides
            hi = value_and_grads(p, v, f, weights, matches, bary)
            lo = value_and_grads(p, v, f, weights, matches, bary, F32)
            rv = max(rv, M.error_ratio(lo["value"].reshape(1), hi["value"].reshape(1), hi["value_terms"].reshape(1)))
            rp = max(rp, M.error_ratio(lo["gp"], hi["gp"], hi["gp_terms"]))
            rg = max(rg, M.error_ratio(lo["gv"], hi["gv"], hi["gv_terms"]))
    return rd, rw, rv, rp, rg


# ------------------------------------------------------------------------------------------------------------------ the fit
FIT_STEPS, FIT_LR, FIT_POINTS = 60, 0.02, 3000
ELLIPSOID = (1.5, 1.0, 0.7)  # DESIGN 4.4u's target: the unit icosphere (level 3) scaled by these
