"""float64 reference of the mesh regularisers (reni_tu_meshreg.hip, ops.mesh_regularizers), and the cases.

``topology`` restates the lists' definition with plain Python loops (nothing of ops.mesh_edge_lists); ``losses`` is a torch
restatement of include/reni_hip.h's definitions, differentiable by autograd; ``closed_form`` is the same values and gradients
written out by hand in the kernels' structure (per edge, per pair, per vertex, gather), in any dtype, and accumulates
sum |terms| per element with the conditioning carried along: the terms of r over |r|, of the normals over |n|, of Heron's
factors over the factors.  In float64 it is checked against autograd and against central differences; evaluated in float32 on
the CPU it gives the error-budget constants K.  Its sums run left to right (``_seq_sum``, index_add): the plain float32
evaluation in the written order.

Plain data and torch on the CPU; nothing here touches a device."""
import functools

import numpy as np
import torch

from tests import gbuffer_grad_ref as G
from tests.silhouette_ref import UNDECIDED_CAP  # 0.02

F64 = torch.float64
U, FLOOR = G.U, G.FLOOR
UNDECIDED_REL = 2.0 ** -16
AREA_FLOOR, NRM_FLOOR = 1e-12, 1e-8
LOSSES = ("edge", "uniform", "cot", "normal")
TARGET = {"edge": 0.05}  # target_length of the edge-loss parity tests (0 is the default of the API; 0.05 exercises the difference)
FUSED = (0.7, 1.3, 0.4)  # the weights (edge, laplacian, normal) of the fused parity tests
# V, E = 2V - 3 and P = V - 3 of a strip on both sides of 256 (the kernels' block), of 512 and, E, of 4096 (the reducer's chunk:
# V = 2050 is the first two-level reduction)
STRIPS = (129, 130, 255, 256, 257, 258, 259, 260, 512, 513, 515, 516, 2049, 2050)
CASES = ((("tetra", 8), ("ico", 16), ("fan", 16), ("cover", 33), ("soup", 17), ("unreferenced", 16), ("bad_faces", 16),
          ("tiny_normal", 16)) + tuple(("strip", V) for V in STRIPS)
         + (("book", 0), ("double", 0), ("hinge", 90), ("hinge", 0), ("bad_faces_cot", 16)))
# Error-budget constants: 4 x the worst ratio |float32 closed form - float64| / (2^-23 sum |terms|) of ``float32_ratios()`` on the
# CPU over the parity cases of each quantity (tests/test_mesh_reg_cpu.py checks that they still are; DESIGN 4.4t has the table)
# loss -> (K value, K grad_verts); measured worst ratios: edge 0.663, 2.239; uniform 0.312, 0.420; cot 0.0497, 0.167;
# normal 0.0916, 0.259
K = {"edge": (2.66, 8.96), "uniform": (1.25, 1.69), "cot": (0.199, 0.669), "normal": (0.367, 1.04)}


def case_id(key):
    return "-".join(str(k) for k in key)


@functools.lru_cache(maxsize=None)
def mesh(key):
    """-> (verts float32 [V, 3], faces int64 [F, 3])"""
    kind, arg = key
    if kind == "book":  # three faces on one edge: multiplicity 3, three pairs
        v = np.array([[0.1, -0.2, 0.0], [0.0, 0.3, 0.9], [0.8, 0.1, 0.4], [-0.5, 0.6, 0.3], [-0.2, -0.7, 0.5]], np.float32)
        return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)
    if kind == "double":  # one face listed twice: every edge has multiplicity 2 and cos = -1
        v = np.array([[0.1, -0.2, 0.0], [0.0, 0.3, 0.9], [0.8, 0.1, 0.4]], np.float32)
        return v, np.array([[0, 1, 2], [0, 1, 2]], np.int64)
    if kind == "hinge":  # two faces folded by arg degrees about their shared edge (0: flat, cos = 1; 90: cos = 0)
        t = np.deg2rad(float(arg))
        v = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.15, 0.5, 0.0], [0.3, -0.5 * np.cos(t), 0.5 * np.sin(t)]], np.float32)
        return v, np.array([[0, 1, 2], [1, 0, 3]], np.int64)
    if kind == "bad_faces_cot":  # "bad_faces" with vertex 43 off the line of 42 and 44: its face has an area (the cot parity case)
        v, f = mesh(("bad_faces", arg))
        v = v.copy()
        v[43] += (np.random.default_rng(43).normal(size=3) * 0.05).astype(np.float32)
        return v, f
    v, f = G.case(kind, arg)[:2]
    return v, f


class Topology:
    pass


@functools.lru_cache(maxsize=None)
def topology(key):
    """``build_topology`` of a case: computed once, read-only"""
    v, faces = mesh(key)
    return build_topology(v.shape[0], faces)


def build_topology(V, faces):
    """the lists by their definition: edges [E, 2]; the half edges (edge, face, corner k, opposite vertex) in ascending
    (edge, face); the pairs (edge, c, d) in ascending (edge, face, face); the directed neighbour entries (v, j, edge) in
    ascending (v, edge); the faces taking part"""
    half = []
    part = []
    for f, tri in enumerate(faces.tolist()):
        if not all(0 <= i < V for i in tri) or len(set(tri)) != 3:
            continue
        part.append(f)
        for k in range(3):
            p, q = tri[(k + 1) % 3], tri[(k + 2) % 3]
            half.append((min(p, q), max(p, q), f, k, tri[k]))
    half.sort()
    edges = sorted({(a, b) for a, b, _, _, _ in half})
    eid = {e: i for i, e in enumerate(edges)}
    by_edge = [[] for _ in edges]
    for a, b, f, k, o in half:
        by_edge[eid[(a, b)]].append((f, k, o))
    pairs = [(e, ents[i][2], ents[j][2]) for e, ents in enumerate(by_edge) for i in range(len(ents)) for j in range(i + 1, len(ents))]
    nb = sorted([(a, e, b) for e, (a, b) in enumerate(edges)] + [(b, e, a) for e, (a, b) in enumerate(edges)])
    T = Topology()
    lt = lambda rows, n: torch.tensor(rows, dtype=torch.int64).reshape(-1, n)  # noqa: E731
    T.V, T.F = V, faces.shape[0]
    T.edges = lt(edges, 2)
    T.half = lt([(eid[(a, b)], f, k, o) for a, b, f, k, o in half], 4)
    T.pairs = lt(pairs, 3)
    T.nb = lt([(vv, j, e) for vv, e, j in nb], 3)
    T.part = torch.tensor(part, dtype=torch.int64)
    T.faces = torch.from_numpy(faces)
    T.E, T.P, T.H = len(edges), len(pairs), len(half)
    T.mult = [len(x) for x in by_edge]
    return T


def verts(key, dtype=F64):
    return torch.from_numpy(mesh(key)[0]).to(dtype)


# ------------------------------------------------------------------------------------------ restatement of the definitions
def _cot_weights(x, T):
    """(w_e [E], cot [Fp, 3]) as constants"""
    with torch.no_grad():
        tri = T.faces[T.part]
        x0, x1, x2 = x[tri[:, 0]], x[tri[:, 1]], x[tri[:, 2]]
        A, B, C = (x1 - x2).norm(dim=1), (x0 - x2).norm(dim=1), (x0 - x1).norm(dim=1)
        s = 0.5 * (A + B + C)
        area = (s * (s - A) * (s - B) * (s - C)).clamp_min(0.0).sqrt().clamp_min(AREA_FLOOR)
        cot = torch.stack([B * B + C * C - A * A, A * A + C * C - B * B, A * A + B * B - C * C], 1) / (4.0 * area)[:, None]
        local = torch.full((T.F,), -1, dtype=torch.int64)
        local[T.part] = torch.arange(T.part.numel())
        w = torch.zeros(T.E, dtype=x.dtype).index_add(0, T.half[:, 0], cot[local[T.half[:, 1]], T.half[:, 2]])
    return w, cot


def losses(x, T, target=0.0, method="uniform"):
    """(L_e, L_l, L_n) of the definitions, torch, differentiable in x"""
    zero = x.sum() * 0.0
    Le = Ll = Ln = zero
    if T.E:
        ln = (x[T.edges[:, 0]] - x[T.edges[:, 1]]).norm(dim=1)
        Le = ((ln - target) ** 2).sum() / T.E
        v, j, e = T.nb[:, 0], T.nb[:, 1], T.nb[:, 2]
        w = torch.ones(T.E, dtype=x.dtype) if method == "uniform" else _cot_weights(x, T)[0]
        s = torch.zeros(T.V, dtype=x.dtype).index_add(0, v, w[e])
        deg = torch.zeros(T.V, dtype=x.dtype).index_add(0, v, torch.ones_like(w[e]))
        n = torch.where(s > 0, 1.0 / s.clamp_min(1e-300), s)
        S = torch.zeros_like(x).index_add(0, v, w[e][:, None] * x[j])
        r = torch.where((deg > 0)[:, None], S * n[:, None] - x, torch.zeros_like(x))
        Ll = r.norm(dim=1).sum() / T.V
    if T.P:
        xa, xb = x[T.edges[T.pairs[:, 0], 0]], x[T.edges[T.pairs[:, 0], 1]]
        e, p, q = xb - xa, x[T.pairs[:, 1]] - xa, x[T.pairs[:, 2]] - xa
        n0, n1 = torch.cross(e, p, dim=1), -torch.cross(e, q, dim=1)
        cs = (n0 * n1).sum(1) / (n0.norm(dim=1).clamp_min(NRM_FLOOR) * n1.norm(dim=1).clamp_min(NRM_FLOOR))
        Ln = (1.0 - cs).sum() / T.P
    return Le, Ll, Ln


def reference(key, loss, target=0.0):
    """(value, grad_verts [V, 3]) float64 by autograd through the restatement; loss: one of LOSSES"""
    x = verts(key).requires_grad_(True)
    Le, Ll, Ln = losses(x, topology(key), target, "cot" if loss == "cot" else "uniform")
    val = {"edge": Le, "uniform": Ll, "cot": Ll, "normal": Ln}[loss]
    (g,) = torch.autograd.grad(val, x, allow_unused=True)
    return float(val.detach()), (torch.zeros_like(x) if g is None else g)


# -------------------------------------------------------------------------------- values and gradients written out by hand
def _seq_sum(t):
    return torch.cumsum(t, 0)[-1] if t.numel() else torch.zeros((), dtype=t.dtype)


def _norm(t):
    return (t * t).sum(1).sqrt()


def closed_form(x, T, loss, target=0.0):
    """dict(value, value_terms, g [V, 3], g_terms [V, 3], und_rows [V] bool, und_value bool) of one loss in x's dtype.
    und_*: the elements an undecided branch reaches (UNDECIDED_REL of the accumulated terms moves it across)."""
    dt = x.dtype
    V = T.V
    z3 = torch.zeros(V, 3, dtype=dt)
    out = {"value": torch.zeros((), dtype=dt), "value_terms": torch.zeros((), dtype=dt), "g": z3.clone(), "g_terms": z3.clone(),
           "und_rows": torch.zeros(V, dtype=torch.bool), "und_value": False}
    if not T.E:
        return out
    a, b = T.edges[:, 0], T.edges[:, 1]
    if loss == "edge":
        d = x[a] - x[b]
        ln = _norm(d)
        diff = ln - target
        out["value"], out["value_terms"] = _seq_sum(diff * diff) / T.E, _seq_sum((ln + target) ** 2) / T.E
        pos = ln > 0
        k = torch.where(pos, 2.0 * diff / ln.clamp_min(1e-300), torch.zeros_like(ln))
        km = torch.where(pos, 2.0 * (ln + target) / ln.clamp_min(1e-300), torch.zeros_like(ln))
        g, gm = k[:, None] * d, km[:, None] * d.abs()
        out["g"] = z3.index_add(0, a, g).index_add(0, b, -g) / T.E
        out["g_terms"] = z3.index_add(0, a, gm).index_add(0, b, gm) / T.E
        und = pos & (ln < UNDECIDED_REL * _norm(x[a].abs() + x[b].abs()))
        out["und_rows"][a[und]] = True
        out["und_rows"][b[und]] = True
        out["und_value"] = bool(und.any())
        return out
    if loss in ("uniform", "cot"):
        v, j, e = T.nb[:, 0], T.nb[:, 1], T.nb[:, 2]
        und_v = torch.zeros(V, dtype=torch.bool)
        if loss == "uniform":
            w, wt = torch.ones(T.E, dtype=dt), torch.zeros(T.E, dtype=dt)
        else:
            tri = T.faces[T.part]
            x0, x1, x2 = x[tri[:, 0]], x[tri[:, 1]], x[tri[:, 2]]
            A2, B2, C2 = ((x1 - x2) ** 2).sum(1), ((x0 - x2) ** 2).sum(1), ((x0 - x1) ** 2).sum(1)
            A, B, C = A2.sqrt(), B2.sqrt(), C2.sqrt()
            s = 0.5 * ((A + B) + C)
            root = (s * (s - A) * (s - B) * (s - C)).clamp_min(0.0).sqrt()
            area = root.clamp_min(AREA_FLOOR)
            # relative error scale of the area: half the sum of its factors' (s + X) / |s - X|
            rel = 0.5 * (1.0 + sum((s + X) / (s - X).abs().clamp_min(1e-300) for X in (A, B, C)))
            und_f = (rel * UNDECIDED_REL >= 1.0) | ((root - AREA_FLOOR).abs() <= UNDECIDED_REL * rel * root)
            rel = torch.where(root > AREA_FLOOR, rel, torch.zeros_like(rel))
            cot = torch.stack([(B2 + C2) - A2, (A2 + C2) - B2, (A2 + B2) - C2], 1) / (4.0 * area)[:, None]
            cott = ((A2 + B2 + C2) / (4.0 * area))[:, None] + cot.abs() * rel[:, None]
            local = torch.full((T.F,), -1, dtype=torch.int64)
            local[T.part] = torch.arange(T.part.numel())
            hf, hk = local[T.half[:, 1]], T.half[:, 2]
            w = torch.zeros(T.E, dtype=dt).index_add(0, T.half[:, 0], cot[hf, hk])
            wt = torch.zeros(T.E, dtype=dt).index_add(0, T.half[:, 0], cott[hf, hk])
            und_v[tri[und_f].reshape(-1)] = True
        we, wte = w[e], wt[e]
        s_v = torch.zeros(V, dtype=dt).index_add(0, v, we)
        st = torch.zeros(V, dtype=dt).index_add(0, v, wte + we.abs())
        deg = torch.zeros(V, dtype=dt).index_add(0, v, torch.ones_like(we))
        has = deg > 0
        if loss == "uniform":
            n = torch.where(has, 1.0 / deg.clamp_min(1.0), torch.zeros_like(deg))
            nt = n.clone()
        else:
            pos = s_v > 0
            n = torch.where(pos, 1.0 / s_v.clamp_min(1e-300), s_v)
            nt = torch.where(pos, st / (s_v * s_v).clamp_min(1e-300), st)
            und_v |= has & (s_v.abs() <= UNDECIDED_REL * st)
        S = z3.index_add(0, v, we[:, None] * x[j])
        St = z3.index_add(0, v, (we.abs() + wte)[:, None] * x[j].abs())
        r = torch.where(has[:, None], S * n[:, None] - x, z3)
        Tr = torch.where(has[:, None], St * n.abs()[:, None] + S.abs() * nt[:, None] + x.abs(), z3)
        ln = _norm(r)
        pos = ln > 0
        lns = ln.clamp_min(1e-300)
        lnt = torch.where(pos, (r.abs() * Tr).sum(1) / lns, _norm(Tr))
        out["value"], out["value_terms"] = _seq_sum(ln) / V, _seq_sum(torch.maximum(lnt, ln)) / V
        u = torch.where(pos[:, None], r / lns[:, None], z3)
        ut = torch.where(pos[:, None], Tr / lns[:, None] + u.abs() * (lnt / lns)[:, None], z3)
        q, qt = n[:, None] * u, n.abs()[:, None] * ut + nt[:, None] * u.abs()
        out["g"] = (z3.index_add(0, v, we[:, None] * q[j]) - u) / V
        out["g_terms"] = (z3.index_add(0, v, we.abs()[:, None] * qt[j] + wte[:, None] * q[j].abs()) + ut) / V
        und_v |= pos & (ln < UNDECIDED_REL * _norm(Tr))
        rows = und_v.clone()
        rows[v[und_v[j]]] = True  # the neighbours of an undecided vertex
        # (the weights are constants of the gradient: an undecided vertex reaches no further than its neighbours)
        out["und_rows"], out["und_value"] = rows, bool(und_v.any())
        return out
    if loss != "normal":
        raise ValueError(loss)
    if not T.P:
        return out
    ia, ib, ic, id_ = T.edges[T.pairs[:, 0], 0], T.edges[T.pairs[:, 0], 1], T.pairs[:, 1], T.pairs[:, 2]
    xa = x[ia]
    e, p, q = x[ib] - xa, x[ic] - xa, x[id_] - xa
    cross, ac = G._cross, G._abs_cross
    n0, n1 = cross(e, p), cross(q, e)
    T0, T1 = ac(e.abs(), p.abs()), ac(q.abs(), e.abs())
    len0, len1 = _norm(n0), _norm(n1)
    big0, big1 = len0 > NRM_FLOOR, len1 > NRM_FLOOR
    l0, l1 = len0.clamp_min(NRM_FLOOR), len1.clamp_min(NRM_FLOOR)
    zero = torch.zeros_like(l0)
    l0t = torch.where(big0, (n0.abs() * T0).sum(1) / l0, zero)
    l1t = torch.where(big1, (n1.abs() * T1).sum(1) / l1, zero)
    dot, dott = (n0 * n1).sum(1), (T0 * n1.abs() + n0.abs() * T1).sum(1)
    cs = dot / (l0 * l1)
    cst = dott / (l0 * l1) + cs.abs() * (l0t / l0 + l1t / l1)
    val, valt = 1.0 - cs, 1.0 + cst
    out["value"], out["value_terms"] = _seq_sum(val) / T.P, _seq_sum(valt) / T.P

    def side(na, nb_, Ta, Tb, la, lb, lat, lbt, big):
        k = torch.where(big, cs / la, zero)
        Gv = -(nb_ / lb[:, None] - k[:, None] * na) / la[:, None]
        inner = (Tb / lb[:, None] + nb_.abs() * (lbt / (lb * lb))[:, None]
                 + torch.where(big, cst / la + cs.abs() * lat / (la * la), zero)[:, None] * na.abs() + k.abs()[:, None] * Ta)
        return Gv, inner / la[:, None] + Gv.abs() * (lat / la)[:, None]

    G0, G0t = side(n0, n1, T0, T1, l0, l1, l0t, l1t, big0)
    G1, G1t = side(n1, n0, T1, T0, l1, l0, l1t, l0t, big1)
    gb, gc, gd = cross(p, G0) + cross(G1, q), cross(G0, e), cross(e, G1)
    gbt, gct, gdt = ac(p.abs(), G0t) + ac(G1t, q.abs()), ac(G0t, e.abs()), ac(e.abs(), G1t)
    ga, gat = -((gb + gc) + gd), gbt + gct + gdt
    out["g"] = z3.index_add(0, ia, ga).index_add(0, ib, gb).index_add(0, ic, gc).index_add(0, id_, gd) / T.P
    out["g_terms"] = z3.index_add(0, ia, gat).index_add(0, ib, gbt).index_add(0, ic, gct).index_add(0, id_, gdt) / T.P
    und = ((len0 - NRM_FLOOR).abs() <= UNDECIDED_REL * (n0.abs() * T0).sum(1) / len0.clamp_min(1e-300)) | \
          ((len1 - NRM_FLOOR).abs() <= UNDECIDED_REL * (n1.abs() * T1).sum(1) / len1.clamp_min(1e-300))
    for idx in (ia, ib, ic, id_):
        out["und_rows"][idx[und]] = True
    out["und_value"] = bool(und.any())
    return out


def target_of(loss):
    return TARGET.get(loss, 0.0)


@functools.lru_cache(maxsize=None)
def scales(key, loss):
    """the float64 closed form of a case (values, gradients, sum |terms|, the undecided elements): computed once, read-only"""
    return closed_form(verts(key), topology(key), loss, target_of(loss))


def parity_cases(loss):
    """the cases whose parity is bounded: for "cot", "bad_faces" (its collinear face is undecided by construction and reaches
    more than UNDECIDED_CAP of the elements) gives way to "bad_faces_cot"; the other losses do not need the replacement"""
    if loss == "cot":
        return tuple(k for k in CASES if k[0] != "bad_faces")
    return tuple(k for k in CASES if k[0] != "bad_faces_cot")


def undecided_share(key, loss):
    """(undecided elements, elements): the rows of grad_verts times 3, and the value"""
    s = scales(key, loss)
    return 3 * int(s["und_rows"].sum()) + int(s["und_value"]), 3 * topology(key).V + 1


# ------------------------------------------------------------------------------------------------------------ the bound
def bound(ref, terms, k):
    return G.bound(ref, terms, k)


def error_ratio(got, ref, terms, keep=None):
    """worst |got - ref| / (2^-23 sum |terms|) over the kept rows; where sum |terms| is 0 the value must be exact (else inf)"""
    got, ref, terms = (torch.as_tensor(t).detach().double().cpu() for t in (got, ref, terms))
    if keep is not None:
        got, ref, terms = got[keep], ref[keep], terms[keep]
    return G.error_ratio(got, ref, terms) if ref.numel() else 0.0


def over_bound(got, ref, terms, k, keep=None):
    """worst |got - ref| / max(k 2^-23 sum |terms|, 2e-5 max |ref|) over the kept rows; <= 1 passes.  The floor is of the
    whole reference, undecided rows included only in so far as they are finite."""
    got, ref, terms = (torch.as_tensor(t).detach().double().cpu() for t in (got, ref, terms))
    if keep is not None:
        got, ref, terms = got[keep], ref[keep], terms[keep]
    return G.over_bound(got, ref, terms, k) if ref.numel() else 0.0


@functools.lru_cache(maxsize=None)
def float32_ratios():
    """loss -> (worst ratio of the value, worst ratio of grad_verts) of the closed form evaluated in float32 torch on the CPU
    against float64, over the loss's parity cases, undecided elements left out"""
    res = {}
    for loss in LOSSES:
        wv = wg = 0.0
        for key in parity_cases(loss):
            ref = scales(key, loss)
            got = closed_form(verts(key, torch.float32), topology(key), loss, float(np.float32(target_of(loss))))
            if not ref["und_value"]:
                wv = max(wv, error_ratio(got["value"].reshape(1), ref["value"].reshape(1), ref["value_terms"].reshape(1)))
            wg = max(wg, error_ratio(got["g"], ref["g"], ref["g_terms"], ~ref["und_rows"]))
        res[loss] = (wv, wg)
    return res


# ---------------------------------------------------------------------------------------------------------------- a fit
FIT_STEPS, FIT_LR, FIT_NOISE = 40, 5e-3, 0.08
FIT_WEIGHTS = {"laplacian": 1.0, "normal": 0.1, "edge": 0.1}
# the float64 reference's loss before and after FIT_STEPS Adam steps (tests/test_mesh_reg_cpu.py pins them)
FIT_START, FIT_END = 0.09343297292089842, 0.057341008401933735


def fit_mesh():
    """(clean verts, start verts, faces, target_length): the level-1 icosphere, the same sphere with fixed-seed radial noise of
    FIT_NOISE of the radius, and the mean edge length of the clean sphere"""
    v, f = mesh(("ico", 16))
    rng = np.random.default_rng(7)
    start = (v.astype(np.float64) * (1.0 + FIT_NOISE * rng.standard_normal(v.shape[0]))[:, None]).astype(np.float32)
    T = topology(("ico", 16))
    x = torch.from_numpy(v).double()
    target = float((x[T.edges[:, 0]] - x[T.edges[:, 1]]).norm(dim=1).mean())
    return v, start, f, float(np.float32(target))


@functools.lru_cache(maxsize=None)
def fit_reference():
    """the losses of FIT_STEPS Adam steps on the restatement in float64 on the CPU, FIT_STEPS + 1 values"""
    _, start, _, target = fit_mesh()
    T = topology(("ico", 16))
    x = torch.from_numpy(start).double().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=FIT_LR)
    out = []
    for step in range(FIT_STEPS + 1):
        Le, Ll, Ln = losses(x, T, target, "uniform")
        loss = FIT_WEIGHTS["edge"] * Le + FIT_WEIGHTS["laplacian"] * Ll + FIT_WEIGHTS["normal"] * Ln
        out.append(float(loss.detach()))
        if step == FIT_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    return out
