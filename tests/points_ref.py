"""float64 reference of the point-cloud unit (reni_tu_points.hip; ops.nearest_points, chamfer_grad, mesh_sample_table,
mesh_sample_points; reni_amd/mesh_losses.py), and the cases.

Everything is a restatement of include/reni_hip.h's definitions ("point clouds") in float64 ON THE FLOAT32-ROUNDED INPUTS:
``nearest`` (best and second-best distance of every query, blockwise, never more than a block of the N x M matrix at a time),
``chamfer`` (value, both gradients and sum |terms| per element with the matches held constant), ``sample`` (areas, CDF, faces,
barycentrics, points and sum |terms|).  ``chamfer(..., dtype=float32)`` is the same written order in float32 on the CPU: it
gives the error-budget constants K.  Plain data and torch on the CPU; nothing here touches a device."""
import functools

import numpy as np
import torch

from tests import mesh_reg_ref as M

F64 = torch.float64
U, FLOOR = M.U, M.FLOOR
TILE = 1024       # NP_TILE: targets staged in LDS at a time
QUERIES = 512     # NP_QUERIES: queries per workgroup
SHORT = 128       # CH_SHORT: the longest range one lane sums alone
UNDECIDED_CAP = 0.01
DIST_K = 4.0      # dist2 within 4 * 2^-23 d_ref: five roundings of relative 2^-24 on a sum of non-negative terms
MARGIN_K = 8.0    # a query is undecided where best and second best differ by <= 8 * 2^-23 d_second
# Error-budget constants of the chamfer value and gradients, and of the sampled points and their vertex gradient: 4 x the worst
# ratio |float32 CPU evaluation - float64| / (2^-23 sum |terms|) of ``float32_ratios()`` over the cases below
# (tests/test_points_cpu.py checks that they still are).  Measured worst ratios: value 1.1008, gradients 1.5007; points 1.2235, vertex gradient 1.1106
K_VALUE, K_GRAD = 4.41, 6.01
K_POINTS, K_VGRAD = 4.90, 4.45
# the CDF budget of the sampler: u0 within this of a CDF step may fall on either side.  An area is a cross product, a sum of
# squares and a root in fp32 (relative error a few 2^-24 on a triangle that is not a needle), the prefix sums are in double and
# the quotient is rounded once (2^-24): 16 * 2^-23 covers them with room for the needle-free cases used here.
CDF_BUDGET = 16.0 * U
WEIGHT_BOUND = 4.0 * U   # r = sqrtf(u1), 1 - r, r (1 - u2), r u2: at most four roundings of values <= 1


def case_id(key):
    return "-".join(str(k) for k in key)


# -------------------------------------------------------------------------------------------------------------- the clouds
@functools.lru_cache(maxsize=None)
def cloud(kind, n, seed, scale=1.0):
    """float32 [n, 3]: "cube" uniform in [-1, 1]^3, "sphere" on the unit sphere, "shell" on the sphere of radius 1.25; times scale"""
    g = np.random.default_rng(seed)
    if kind == "cube":
        p = g.uniform(-1.0, 1.0, size=(n, 3))
    else:
        p = g.normal(size=(n, 3))
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        if kind == "shell":
            p *= 1.25
    return torch.from_numpy((p * scale).astype(np.float32))


# (name, N, M): random cube clouds; the shapes the kernel takes other paths at -- one point, one tile +- 1, one workgroup of
# queries +- 1, a size that must be sliced, more than one workgroup and tile
NN_SHAPES = ((1, 1), (1, 4097), (4097, 1), (255, 257), (257, 255), (300, TILE - 1), (300, TILE), (300, TILE + 1),
             (QUERIES - 1, 700), (QUERIES, 700), (QUERIES + 1, 700), (64, 20000), (1000, 4097))
NN_CASES = (tuple(("cube", n, m, 1.0) for n, m in NN_SHAPES)
            + (("cube", 4097, 1000, 1.0), ("spheres", 4097, 1000, 1.0), ("spheres", 1000, 4097, 1.0), ("spheres", 257, 1023, 1.0), ("cube", 257, 1023, 1e-3), ("cube", 257, 1023, 1e3),
               ("spheres", 257, 1023, 1e-3), ("spheres", 257, 1023, 1e3)))


def nn_clouds(key):
    kind, n, m, scale = key
    if kind == "cube":
        return cloud("cube", n, 11 + n, scale), cloud("cube", m, 23 + m, scale)
    return cloud("sphere", n, 11 + n, scale), cloud("shell", m, 23 + m, scale)


def dist_matrix(x, y):
    d = x[:, None, :] - y[None, :, :]
    return (d * d).sum(-1)


@functools.lru_cache(maxsize=None)
def _nearest_cached(key):
    return nearest(*nn_clouds(key))


def nearest(x, y, block=256):
    """-> dict of float64 / int64 [N]: d (the smallest distance), idx (its lowest index), d2 (the smallest distance over the OTHER
    indices, +inf for M = 1), und (best and second best within MARGIN_K 2^-23 d2: the device may name either)"""
    x, y = x.to(F64), y.to(F64)
    N, M_ = x.shape[0], y.shape[0]
    d = torch.empty(N, dtype=F64)
    idx = torch.empty(N, dtype=torch.int64)
    d2 = torch.full((N,), float("inf"), dtype=F64)
    for b in range(0, N, block):
        D = dist_matrix(x[b:b + block], y)
        db, ib = D.min(dim=1)  # (torch returns the first of equal minima on the CPU; made sure of below)
        first = (D == db[:, None]).to(torch.int64).argmax(dim=1)
        d[b:b + block], idx[b:b + block] = db, first
        if M_ > 1:
            D.scatter_(1, first[:, None], float("inf"))
            d2[b:b + block] = D.min(dim=1).values
    und = torch.isfinite(d2) & ((d2 - d) <= MARGIN_K * U * d2)  # (one target: nothing to confuse it with)
    return {"d": d, "idx": idx, "d2": d2, "und": und}


def nearest_of(key):
    return _nearest_cached(key)


def lattice():
    """x: the 9^3 integer lattice; y: the same lattice shifted by half a step -- every interior query has eight nearest targets at
    exactly 0.75 in fp32, so the lowest index must win"""
    r = torch.arange(9, dtype=torch.float32)
    x = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    return x, x + 0.5


# --------------------------------------------------------------------------------------------------------------- chamfer
def _ranged(n_near, N=40, M_extra=60, seed=5):
    """x_0 at the origin with n_near targets in a small ball round it; the other x on a sphere of radius 10, each with a few
    targets of its own: the longest range of the gather is n_near"""
    g = np.random.default_rng(seed + n_near)
    x = g.normal(size=(N, 3))
    x = 10.0 * x / np.linalg.norm(x, axis=1, keepdims=True)
    x[0] = 0.0
    near = g.normal(size=(n_near, 3)) * 0.1
    owner = 1 + g.integers(0, N - 1, size=M_extra)
    far = x[owner] + g.normal(size=(M_extra, 3)) * 0.1
    y = np.concatenate([near, far])[g.permutation(n_near + M_extra)]
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.float32))


CH_CASES = ("cube", "uneven", "spheres", "star", "r100", "r128", "r129", "coincident")
WEIGHTS = ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0), (0.3, 1.7))
G_UP = 2.5  # the upstream factor of the g != 1 tests


@functools.lru_cache(maxsize=None)
def ch_clouds(name):
    if name == "cube":
        return cloud("cube", 300, 1), cloud("cube", 700, 2)
    if name == "uneven":
        return cloud("cube", 1000, 3), cloud("cube", 257, 4)
    if name == "spheres":
        return cloud("sphere", 600, 5), cloud("shell", 513, 6)
    if name == "star":  # N = 300, M = 5000, every y nearest to x_0: a range far past 128
        return _ranged(5000, N=300, M_extra=0)
    if name[0] == "r":  # the longest range: 100 (in 65 .. 128), exactly 128, 129
        return _ranged(int(name[1:]))
    if name == "coincident":
        x = cloud("cube", 500, 7)
        return x, x.clone()
    raise KeyError(name)


def longest_range(name):
    x, y = ch_clouds(name)
    return int(torch.bincount(nearest(y, x)["idx"], minlength=x.shape[0]).max())


def _seq_rows(index, rows, n):
    """sum of rows by index, left to right (index_add on the CPU)"""
    return torch.zeros(n, rows.shape[1], dtype=rows.dtype).index_add(0, index, rows)


def chamfer(x, y, weights=(1.0, 1.0), dtype=F64, matches=None):
    """value, grad_x, grad_y of L = (w_x / N) sum_i d_x[i] + (w_y / M) sum_j d_y[j] with the matches of the float64 search held
    constant, in ``dtype``; with sum |terms| of each, and the rows that touch an undecided match"""
    wx, wy = weights
    if matches is None:
        matches = (nearest(x, y), nearest(y, x))
    nx, ny = matches
    X, Y = x.to(dtype), y.to(dtype)
    N, M_ = X.shape[0], Y.shape[0]
    ex = X - Y[nx["idx"]]        # x_i - y_idx_xy[i]
    ey = X[ny["idx"]] - Y        # x_idx_yx[j] - y_j
    dx, dy = (ex * ex).sum(1), (ey * ey).sum(1)
    cx, cy = torch.tensor(2.0 * wx / N, dtype=dtype), torch.tensor(2.0 * wy / M_, dtype=dtype)
    value = torch.tensor(wx, dtype=dtype) * (dx.sum() / N) + torch.tensor(wy, dtype=dtype) * (dy.sum() / M_)
    gx = cx * ex + cy * _seq_rows(ny["idx"], ey, N)
    gy = -(cy * ey) - cx * _seq_rows(nx["idx"], ex, M_)
    gx_terms = cx * ex.abs() + cy * _seq_rows(ny["idx"], ey.abs(), N)
    gy_terms = cy * ey.abs() + cx * _seq_rows(nx["idx"], ex.abs(), M_)
    # a row of grad_x touches an undecided match if its own match is one (and weighs), or an undecided y_j is matched to it
    und_x = (nx["und"] & (wx > 0)) | (torch.zeros(N).index_add(0, ny["idx"], (ny["und"] & (wy > 0)).float()) > 0)
    und_y = (ny["und"] & (wy > 0)) | (torch.zeros(M_).index_add(0, nx["idx"], (nx["und"] & (wx > 0)).float()) > 0)
    return {"value": value, "value_terms": value.abs(), "gx": gx, "gy": gy, "gx_terms": gx_terms, "gy_terms": gy_terms,
            "und_x": und_x, "und_y": und_y, "matches": matches}


@functools.lru_cache(maxsize=None)
def chamfer_of(name, weights=(1.0, 1.0)):
    x, y = ch_clouds(name)
    return chamfer(x, y, weights)


def chamfer_autograd(x, y, weights=(1.0, 1.0)):
    """the same objective through torch's min and autograd in float64 (an independent route to the gradients)"""
    X, Y = x.to(F64).requires_grad_(True), y.to(F64).requires_grad_(True)
    D = dist_matrix(X, Y)
    L = weights[0] * D.min(dim=1).values.mean() + weights[1] * D.min(dim=0).values.mean()
    gx, gy = torch.autograd.grad(L, (X, Y), allow_unused=True)
    z = lambda g, t: torch.zeros_like(t) if g is None else g  # noqa: E731
    return L.detach(), z(gx, X), z(gy, Y)


# -------------------------------------------------------------------------------------------------------------- sampling
SAMPLE_MESHES = (("tetra", 8), ("ico", 16), ("bad_faces", 16), ("soup", 17), ("two", 0))


@functools.lru_cache(maxsize=None)
def sample_mesh(key):
    """-> (verts float32 [V, 3], faces int64 [F, 3]) as tensors; ("two", 0): two triangles with areas 1 : 3"""
    if key[0] == "two":
        v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 2, 0], [3, 0, 1], [5, 0, 1], [3, 3, 1]], dtype=torch.float32)
        return v, torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int64)
    v, f = M.mesh(key)
    return torch.from_numpy(v).clone(), torch.from_numpy(f).clone()


@functools.lru_cache(maxsize=None)
def sample_u(n=2000, seed=3):
    """float32 [n, 3] in [0, 1): random rows, then the edges -- u0 = 0, values next to 1, u1 = 0, u2 = 0"""
    g = np.random.default_rng(seed)
    u = g.uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)
    u = np.minimum(u, np.float32(1.0) - np.float32(2.0 ** -24))
    top = np.float32(1.0) - np.float32(2.0 ** -24)
    u[0] = (0.0, 0.0, 0.0)
    u[1] = (top, top, top)
    u[2] = (0.0, top, 0.5)
    u[3] = (top, 0.0, 0.5)
    u[4] = (0.5, 0.0, 0.0)
    u[5] = (0.25, 0.5, top)
    u[6] = (0.75, 0.5, 0.0)
    return torch.from_numpy(u)


def areas(v, f):
    """float64 [F]: the area of a face that takes part (indices in [0, V), pairwise different), else 0"""
    V = v.shape[0]
    part = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])
    tri = v.to(F64)[f.clamp(0, V - 1)]
    a = 0.5 * torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1).norm(dim=1)
    a = torch.where(part & torch.isfinite(a), a, torch.zeros_like(a))
    return a, part


def sample(v, f, u, upstream=None):
    """the float64 sampler: faces, weights [S, 3], points [S, 3] and their sum |terms|, the samples whose u0 lies within
    CDF_BUDGET of a CDF step (either neighbouring face may be named), and with ``upstream`` [S, 3] the vertex gradient of
    sum(points * upstream), its sum |terms| and the vertex rows an undecided sample touches"""
    a, part = areas(v, f)
    total = a.sum()
    F_, V = f.shape[0], v.shape[0]
    U64 = u.to(F64)
    out = {"area": a, "part": part, "total": total}
    if not (total > 0):
        out.update(face=torch.zeros(u.shape[0], dtype=torch.int64), w=torch.zeros(u.shape[0], 3, dtype=F64),
                   points=torch.zeros(u.shape[0], 3, dtype=F64), und=torch.zeros(u.shape[0], dtype=torch.bool))
        return out
    cdf = torch.cumsum(a, 0) / total
    last = int((a > 0).nonzero().max())
    cdf[last:] = 1.0
    face = torch.searchsorted(cdf, U64[:, 0].contiguous(), right=True).clamp_max(F_ - 1)
    steps = cdf[:last][a[:last] > 0]  # (the last step is exactly 1 on the device too, and u0 < 1: decided by construction)
    und = ((U64[:, 0:1] - steps[None, :]).abs() <= CDF_BUDGET).any(1)
    r = U64[:, 1].sqrt()
    w = torch.stack([1.0 - r, r * (1.0 - U64[:, 2]), r * U64[:, 2]], 1)
    corners = v.to(F64)[f[face]]                       # [S, 3, 3]
    points = (w[:, :, None] * corners).sum(1)
    terms = (w[:, :, None] * corners.abs()).sum(1)
    out.update(cdf=cdf, face=face, w=w, points=points, points_terms=terms, und=und)
    if upstream is not None:
        G_ = upstream.to(F64)
        rows = (w[:, :, None] * G_[:, None, :]).reshape(-1, 3)
        index = f[face].reshape(-1)
        out["gv"] = _seq_rows(index, rows, V)
        out["gv_terms"] = _seq_rows(index, rows.abs(), V)
        touched = torch.zeros(V).index_add(0, f[face[und]].reshape(-1), torch.ones(int(und.sum()) * 3))
        if int(und.sum()):  # the face the device may have named instead: the neighbours in the CDF, faces without area skipped
            mass = (a > 0).nonzero()[:, 0]
            pos = torch.searchsorted(mass, face[und])
            for d in (-1, 1):
                other = mass[(pos + d).clamp(0, mass.numel() - 1)]
                touched.index_add_(0, f[other].reshape(-1), torch.ones(other.numel() * 3))
        out["und_rows"] = touched > 0
    return out


def sample_upstream(n, seed=9):
    return torch.from_numpy(np.random.default_rng(seed).normal(size=(n, 3)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------- the constants
def float32_ratios():
    """(value, gradient, points, vertex gradient): the worst |float32 CPU evaluation - float64| / (2^-23 sum |terms|) over the
    chamfer cases and weights and over the sampling meshes, undecided rows left out"""
    wv = wg = 0.0
    for name in CH_CASES:
        x, y = ch_clouds(name)
        for weights in WEIGHTS:
            ref = chamfer_of(name, weights)
            got = chamfer(x, y, weights, torch.float32, ref["matches"])
            wv = max(wv, M.error_ratio(got["value"].reshape(1), ref["value"].reshape(1), ref["value_terms"].reshape(1)))
            wg = max(wg, M.error_ratio(got["gx"], ref["gx"], ref["gx_terms"], ~ref["und_x"]))
            wg = max(wg, M.error_ratio(got["gy"], ref["gy"], ref["gy_terms"], ~ref["und_y"]))
    wp = wq = 0.0
    u = sample_u()
    up = sample_upstream(u.shape[0])
    for key in SAMPLE_MESHES:
        v, f = sample_mesh(key)
        ref = sample(v, f, u, up)
        w32 = ref["w"].float()
        corners = v[f[ref["face"]]]
        pts = torch.zeros(u.shape[0], 3)
        for k in range(3):  # the fetch's chain: fmaf(w_k, v_k, acc) from 0 (here a rounded product and a rounded sum)
            pts = pts + w32[:, k:k + 1] * corners[:, k]
        wp = max(wp, M.error_ratio(pts, ref["points"], ref["points_terms"]))
        rows = (w32[:, :, None] * up[:, None, :]).reshape(-1, 3)
        gv = _seq_rows(f[ref["face"]].reshape(-1), rows, v.shape[0])
        wq = max(wq, M.error_ratio(gv, ref["gv"], ref["gv_terms"]))
    return wv, wg, wp, wq
