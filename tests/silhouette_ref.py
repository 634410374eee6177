"""float64 reference of the soft silhouette and of its gradient with respect to the vertex positions
(reni_tu_silhouette.hip), the cases, the settings and the classification of (pixel, face) pairs.

``soft_alpha`` is a torch restatement of the definition in include/reni_hip.h, differentiable in the vertices: autograd gives
the gradient of sum_p gA_p alpha_p with membership, inside / outside and the winning edge held fixed (they are comparisons)
and a clamped t constant (clamp's gradient) -- ``reference``.  ``closed_form`` is the same forward and the same gradient written
out by hand in the kernels' structure -- per pair the coefficient -gA trans prob / sigma and the two corners of the winning
edge, per face the six NDC sums and (x, y) -> q -> p, per vertex the gather -- in any dtype: in float64 it is checked against
autograd and accumulates sum |terms| (the scale of the error bound), in float32 it gives the error-budget constants K.

A pair is UNDECIDED when a relative change of 2^-16 in a distance flips its membership (outside and |d - r| <= 2^-16 r) or the
winning edge between two candidates whose nearest points differ.  ``reference_lo`` / ``reference_hi`` take every undecided
choice one way / the other (lo: not a member, the first winner; hi: a member, the runner-up); a result is compared with both.

Plain data and torch on the CPU; nothing here touches a device."""
import functools
import math

import numpy as np
import torch

from tests import gbuffer_grad_ref as G
from tests import raster_edge_cases as E

F64 = torch.float64
U = 2.0 ** -23
FLOOR = 2e-5  # of the largest reference value: the project's usual floor
UNDECIDED_REL = 2.0 ** -16
UNDECIDED_CAP = 0.02  # of the participating pairs, in every case and setting
SAME_POINT = 1e-24  # squared NDC distance below which two nearest points are one (a shared corner)
# The error-budget constants: 4 x the worst ratio error / (2^-23 sum |terms|) that ``float32_ratios()`` reaches on the CPU over
# every case and setting (tests/test_silhouette_cpu.py checks that they still are; DESIGN 4.4r has the measurement and the
# device's own worst ratios).
K_ALPHA = 35.5  # 4 x 8.797 (ico-33, sharp)
K_GVERTS = 122.0  # 4 x 30.32 (strip-257, inside_only)

CASES = tuple(k for k in G.CASES if k[0] != "tiny_normal")
UNREFERENCED = G.UNREFERENCED
SETTINGS = ("sharp", "wide", "inside_only", "short_cut")
DEFAULT_R = math.log(1.0 / 1e-4 - 1.0)  # blur_radius / sigma of pytorch3d's convention
EDGES = ((0, 1), (0, 2), (1, 2))

case_id = G.case_id
COVER_TILT = 7.0  # degrees about the view axis: the cover triangle's axis of symmetry leaves the odd image's middle column


@functools.lru_cache(maxsize=None)
def case(kind, arg):
    """``gbuffer_grad_ref.case``; the cover triangle turned in its plane, so that the pixels of the middle column are no longer
    at one distance from its two slanted edges (25 ties of 1089 pairs otherwise: more than UNDECIDED_CAP).  It still holds the
    whole view, every edge more than 0.8 NDC units away from it."""
    v, f, R, T, S = G.case(kind, arg)
    if kind == "cover":
        a = np.deg2rad(COVER_TILT)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        v = (v.astype(np.float64) @ Rz.T).astype(np.float32)
    return v, f, R, T, S


def setting(name, S):
    """(sigma, blur_radius) of a setting at image size S, both float32-representable: sigma = k (2 / S)^2"""
    k = 32.0 if name == "wide" else 0.25
    sigma = float(np.float32(k * (2.0 / S) ** 2))
    r = {"sharp": DEFAULT_R * sigma, "wide": DEFAULT_R * sigma, "inside_only": 0.0, "short_cut": sigma}[name]
    return sigma, float(np.float32(r))


def upstream(key, name):
    """gA [S*S], a float32-representable float64 tensor"""
    S = case(*key)[4]
    g = torch.Generator().manual_seed(3000 + 10 * CASES.index(key) + SETTINGS.index(name))
    return torch.randn(S * S, generator=g).double()


def inputs(key, dtype=F64):
    v, f, R, T, S = case(*key)
    tanh = E.TANF if dtype == F64 else float(np.float32(E.TANF))
    return torch.from_numpy(v).to(dtype), torch.from_numpy(f), R[0].to(dtype), T[0].to(dtype), S, tanh


# ------------------------------------------------------------------------------------------- restatement of the forward
def taking_part(verts, faces, R, T, tan_half):
    """(indices of the faces that take part [Fp], their NDC x, y and view z [Fp, 3] each), differentiable in verts"""
    V = verts.shape[0]
    ok = ((faces >= 0) & (faces < V)).all(dim=1)
    idx = ok.nonzero()[:, 0]
    q = verts[faces[idx]] @ R + T
    with torch.no_grad():
        z = q[..., 2]
        x, y = q[..., 0] / (z * tan_half), q[..., 1] / (z * tan_half)
        area = G._edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
        part = ~(area.abs() <= 1e-8) & (z > 0).all(dim=1) & torch.isfinite(x).all(dim=1) & torch.isfinite(y).all(dim=1)
    idx, q = idx[part], q[part]
    z = q[..., 2]
    return idx, q[..., 0] / (z * tan_half), q[..., 1] / (z * tan_half), z


def pairs(x, y, S, r, choice="lo", rel=UNDECIDED_REL):
    """Every pixel against every taking-part face, [P, Fp] each: the winning edge, its t, c - p, d, inside, membership, and
    the two kinds of undecided pairs.  ``choice``: which way the undecided pairs go."""
    dtype = x.dtype
    PX, PY = G._pixels(S, dtype)
    PX, PY = PX[:, None], PY[:, None]
    ts, tms, cxs, cys, ds = [], [], [], [], []
    for a, b in EDGES:
        ax, ay, bx, by = x[None, :, a], y[None, :, a], x[None, :, b], y[None, :, b]
        bax, bay = bx - ax, by - ay
        l2 = bax * bax + bay * bay
        deg = (l2 <= 1e-8).expand(PX.shape[0], -1)
        safe = torch.where(l2 <= 1e-8, torch.ones_like(l2), l2)
        raw = (bax * (PX - ax) + bay * (PY - ay)) / safe
        t = torch.where(deg, torch.ones_like(raw), raw.clamp(0.0, 1.0))
        free = ~deg & (raw.detach() > 0) & (raw.detach() < 1)  # t is computed, not a constant 0 or 1: sum |terms| of its dot product
        tms.append(torch.where(free, ((bax * (PX - ax)).abs() + (bay * (PY - ay)).abs()) / safe, t).detach())
        cx = torch.where(deg, bx.expand_as(t), ax + t * bax)
        cy = torch.where(deg, by.expand_as(t), ay + t * bay)
        ts.append(t); cxs.append(cx); cys.append(cy); ds.append((cx - PX) ** 2 + (cy - PY) ** 2)
    t, tm, cx, cy, d3 = torch.stack(ts), torch.stack(tms), torch.stack(cxs), torch.stack(cys), torch.stack(ds)
    with torch.no_grad():
        dd = d3.detach()
        win = torch.zeros(dd.shape[1:], dtype=torch.int64)
        best = dd[0].clone()
        for e in (1, 2):  # the first edge with the strictly smallest distance
            m = dd[e] < best
            win, best = torch.where(m, torch.full_like(win, e), win), torch.where(m, dd[e], best)
        # the runner-up: the first smallest of the other two
        masked = dd.clone().scatter_(0, win[None], float("inf"))
        second = torch.zeros_like(win)
        sbest = masked[0].clone()
        for e in (1, 2):
            m = masked[e] < sbest
            second, sbest = torch.where(m, torch.full_like(second, e), second), torch.where(m, masked[e], sbest)
        cw = (cx.detach().gather(0, win[None])[0], cy.detach().gather(0, win[None])[0])
        cs = (cx.detach().gather(0, second[None])[0], cy.detach().gather(0, second[None])[0])
        apart = (cw[0] - cs[0]) ** 2 + (cw[1] - cs[1]) ** 2 > SAME_POINT
        und_edge = (sbest - best <= rel * best) & apart
        edge = torch.where(und_edge, second, win) if choice == "hi" else win
    pick = edge[None]
    t, cx, cy, d = t.gather(0, pick)[0], cx.gather(0, pick)[0], cy.gather(0, pick)[0], d3.gather(0, pick)[0]
    tm = tm.gather(0, pick)[0]
    with torch.no_grad():
        x0, y0, x1, y1, x2, y2 = (c[None, :] for c in (x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2]))
        A = G._edge(x2, y2, x0, y0, x1, y1) + 1e-8
        w = torch.stack([G._edge(PX, PY, x1, y1, x2, y2) / A, G._edge(PX, PY, x2, y2, x0, y0) / A, G._edge(PX, PY, x0, y0, x1, y1) / A])
        inside = (w > 0).all(dim=0)
        dv = d.detach()
        # a pixel centre on an edge's line: inside alone decides membership where d >= r (the central differences avoid these)
        on_edge = (w.abs().min(dim=0).values <= 1e-6) & (w > -1e-6).all(dim=0) & (dv >= r)
        und_member = ~inside & ((dv - r).abs() <= rel * r) & (r > 0)
        member = inside | (dv < r)
        either = member | und_member
        member = either if choice == "hi" else member & ~und_member
    return {"edge": edge, "t": t, "tm": tm, "dxm": (cx.abs() + PX.abs()).detach(), "dym": (cy.abs() + PY.abs()).detach(), "dx": cx - PX, "dy": cy - PY, "d": d, "inside": inside, "member": member, "either": either, "on_edge": on_edge,
            "undecided": (und_member | und_edge) & either}


def soft_alpha(verts, faces, R, T, S, tan_half, sigma, r, choice="lo"):
    """(alpha [S*S], trans [S*S]) by the definition, torch, differentiable in verts"""
    _, x, y, _ = taking_part(verts, faces, R, T, tan_half)
    p = pairs(x, y, S, r, choice)
    sd = torch.where(p["inside"], -p["d"], p["d"])
    prob = torch.sigmoid(-sd / sigma)  # 1 / (1 + exp(sd / sigma)), with a gradient that stays finite where exp overflows
    trans = torch.where(p["member"], 1.0 - prob, torch.ones_like(prob)).prod(dim=1)
    return 1.0 - trans, trans


def reference(key, name, gA, choice="lo"):
    """g_verts [V, 3] float64 by autograd through the restatement"""
    v, f, R, T, S, tanh = inputs(key)
    sigma, r = setting(name, S)
    verts = v.clone().requires_grad_(True)
    alpha, _ = soft_alpha(verts, f, R, T, S, tanh, sigma, r, choice)
    (g,) = torch.autograd.grad((alpha * gA).sum() + verts.sum() * 0.0, verts)
    return g


def count_pairs(key, name, rel=UNDECIDED_REL):
    """(participating pairs, undecided pairs) of a case and setting, from the float64 reference alone"""
    v, f, R, T, S, tanh = inputs(key)
    sigma, r = setting(name, S)
    with torch.no_grad():
        _, x, y, _ = taking_part(v, f, R, T, tanh)
        p = pairs(x, y, S, r, rel=rel)
    return int(p["either"].sum()), int(p["undecided"].sum())


# -------------------------------------------------------------------------------- the gradient written out by hand
@torch.no_grad()
def closed_form(verts, faces, R, T, S, tan_half, sigma, r, gA=None, choice="lo", trans=None):
    """-> dict(alpha, trans, terms_alpha [S*S]; g, terms_g [V, 3] when gA is given) in verts' dtype, in the kernels'
    structure.  ``trans``: the transmittance the gradient is evaluated with (default: this evaluation's own).  sum |terms|
    follows the same chain with every addend and every coefficient replaced by its magnitude (the weights 1 - t and t of a
    computed t by 1 + sum |terms of t| and sum |terms of t|, c - p by |c| + |p|: near an end of the edge 1 - t cancels, under
    or beside an axis-parallel edge c - p does); alpha's is 1 plus the sum
    of the probabilities that enter its product."""
    dtype = verts.dtype
    R, T = R.reshape(3, 3).to(dtype), T.reshape(3).to(dtype)
    V = verts.shape[0]
    idx, x, y, z = taking_part(verts, faces, R, T, tan_half)
    p = pairs(x, y, S, r, choice)
    member, inside = p["member"], p["inside"]
    prob = 1.0 / (1.0 + torch.exp(torch.where(inside, -p["d"], p["d"]) / sigma))
    own = torch.where(member, 1.0 - prob, torch.ones_like(prob)).prod(dim=1)
    out = {"alpha": 1.0 - own, "trans": own, "terms_alpha": 1.0 + torch.where(member, prob, torch.zeros_like(prob)).sum(dim=1)}
    if gA is None:
        return out
    tr = own if trans is None else trans.reshape(-1).to(dtype)
    g = gA.to(dtype)[:, None] * (-(tr[:, None] * prob) / sigma) * torch.where(inside, -2.0, 2.0).to(dtype)
    g = torch.where(member, g, torch.zeros_like(g))
    wa, wb, e = g * (1.0 - p["t"]), g * p["t"], p["edge"]
    zero = torch.zeros_like(g)
    k = (torch.where(e == 2, zero, wa), torch.where(e == 0, wb, torch.where(e == 2, wa, zero)), torch.where(e == 0, zero, wb))
    wam, wbm = g.abs() * torch.where(p["tm"] == p["t"], 1.0 - p["t"], 1.0 + p["tm"]), g.abs() * p["tm"]
    km = (torch.where(e == 2, zero, wam), torch.where(e == 0, wbm, torch.where(e == 2, wam, zero)), torch.where(e == 0, zero, wbm))
    Fp = idx.numel()
    direct, directm = torch.zeros(Fp, 3, 3, dtype=dtype), torch.zeros(Fp, 3, 3, dtype=dtype)
    for c in range(3):
        tx, ty = (k[c] * p["dx"]).sum(0), (k[c] * p["dy"]).sum(0)
        txm, tym = (km[c] * p["dxm"]).sum(0), (km[c] * p["dym"]).sum(0)
        wz = z[:, c] * tan_half
        gq = torch.stack([tx / wz, ty / wz, -(tx * x[:, c] + ty * y[:, c]) / z[:, c]], 1)
        gqm = torch.stack([txm / wz.abs(), tym / wz.abs(), (txm * x[:, c].abs() + tym * y[:, c].abs()) / z[:, c].abs()], 1)
        direct[:, c] = gq @ R.t()
        directm[:, c] = gqm @ R.t().abs()
    gv, gm = torch.zeros(V, 3, dtype=dtype), torch.zeros(V, 3, dtype=dtype)
    for c in range(3):
        i = faces[idx, c]
        gv, gm = gv.index_add(0, i, direct[:, c]), gm.index_add(0, i, directm[:, c])
    out["g"], out["terms_g"] = gv, gm
    return out


def _evaluate(key, name, gA, trans, choice, dtype=F64):
    v, f, R, T, S, tanh = inputs(key, dtype)
    sigma, r = setting(name, S)
    return closed_form(v, f, R, T, S, tanh, sigma, r, gA, choice, trans)


def reference_lo(key, name, gA=None, trans=None):
    """the float64 closed form with every undecided pair left out and the first winner kept"""
    return _evaluate(key, name, gA, trans, "lo")


def reference_hi(key, name, gA=None, trans=None):
    """... with every undecided pair taken in and the runner-up edge winning"""
    return _evaluate(key, name, gA, trans, "hi")


# ------------------------------------------------------------------------------------------------------------ the bound
def _excess(got, lo, hi, widen):
    """how far got lies from the references, per element: alpha (widen False) from the interval [min, max] of the two;
    the gradient (widen True) from reference_lo, less |reference_hi - reference_lo|"""
    got = torch.as_tensor(got).detach().double().cpu().reshape(lo.shape)
    if widen:
        return ((got - lo).abs() - (hi - lo).abs()).clamp_min(0.0)
    return (torch.minimum(lo, hi) - got).clamp_min(0.0) + (got - torch.maximum(lo, hi)).clamp_min(0.0)


def error_ratio(got, lo, hi, terms, widen):
    """worst excess / (2^-23 sum |terms|); where sum |terms| is 0 the value must be exact (else inf)"""
    err = _excess(got, lo.double(), hi.double(), widen)
    scale = U * terms.double()
    ratio = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(ratio.max()) if ratio.numel() else 0.0


def over_bound(got, lo, hi, terms, K, widen):
    """worst excess / max(K 2^-23 sum |terms|, 2e-5 max |ref|); <= 1 passes"""
    err = _excess(got, lo.double(), hi.double(), widen)
    b = G.bound(lo.double(), terms.double(), K)
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(ratio.max()) if ratio.numel() else 0.0


@functools.lru_cache(maxsize=None)
def float32_ratios():
    """(worst ratio of alpha, worst ratio of g_verts) of the closed form evaluated in float32 torch on the CPU against float64,
    over every case and setting; the float64 gradient is evaluated with the float32 transmittance, as the device tests
    evaluate it with the device's"""
    worst_a = worst_g = 0.0
    for key in CASES:
        for name in SETTINGS:
            gA = upstream(key, name)
            got = _evaluate(key, name, gA, None, "lo", torch.float32)
            lo, hi = reference_lo(key, name, gA, got["trans"].double()), reference_hi(key, name, gA, got["trans"].double())
            worst_a = max(worst_a, error_ratio(got["alpha"], lo["alpha"], hi["alpha"], lo["terms_alpha"], False))
            worst_g = max(worst_g, error_ratio(got["g"], lo["g"], hi["g"], torch.maximum(lo["terms_g"], hi["terms_g"]), True))
    return worst_a, worst_g


# ---------------------------------------------------------------------------------------------------------------- a fit
FIT_S, FIT_STEPS, FIT_LR, FIT_SCALE, FIT_SETTING = 32, 40, 4e-3, 0.8, "sharp"
# hard IoU of the float64 CPU loop (``fit_reference``) before the first and after the last step
FIT_IOU_START, FIT_IOU_END = 0.6013513513513513, 0.8040540540540541  # 89 / 148 -> 119 / 148 pixels


def fit_meshes():
    """(target verts, start verts, faces, R, T): the tilted icosphere and the same sphere scaled by FIT_SCALE about its centre"""
    v, f, R, T, _ = case("ico", FIT_S)
    c = v.astype(np.float64).mean(axis=0)
    return v, (c + FIT_SCALE * (v.astype(np.float64) - c)).astype(np.float32), f, R, T


def hard_coverage(verts, f, R, T):
    """the hard coverage [S*S] bool of np_rasterize (the CPU stand-in for the device's rasteriser)"""
    from tests.test_raster_cpu import np_rasterize, np_vertex_normals
    v = np.asarray(verts, np.float32)
    out = np_rasterize(v, f, np_vertex_normals(v, f), R[0].double().numpy(), T[0].double().numpy(), FIT_S, tan_half=E.TANF)
    return torch.from_numpy(out["pix_to_face"].reshape(-1) >= 0)


def hard_iou(a, b):
    return float((a & b).sum()) / max(float((a | b).sum()), 1.0)


def soft_iou_loss(alpha, mask):
    """mesh.silhouette_iou, restated: 1 - sum(a m) / sum(a + m - a m)"""
    m = mask.to(alpha.dtype)
    return 1.0 - (alpha * m).sum() / (alpha + m - alpha * m).sum()


@functools.lru_cache(maxsize=None)
def fit_reference():
    """(hard IoU at the start, at the end, the losses) of FIT_STEPS Adam steps in float64 on the CPU with the soft IoU alone"""
    target_v, start_v, f, R, T = fit_meshes()
    mask = hard_coverage(target_v, f, R, T)
    sigma, r = setting(FIT_SETTING, FIT_S)
    faces = torch.from_numpy(f)
    verts = torch.from_numpy(start_v).double().requires_grad_(True)
    opt = torch.optim.Adam([verts], lr=FIT_LR)
    iou0 = hard_iou(hard_coverage(start_v, f, R, T), mask)
    losses = []
    for _ in range(FIT_STEPS + 1):
        alpha, _ = soft_alpha(verts, faces, R[0].double(), T[0].double(), FIT_S, E.TANF, sigma, r)
        loss = soft_iou_loss(alpha, mask)
        losses.append(float(loss.detach()))
        if len(losses) > FIT_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    return iou0, hard_iou(hard_coverage(verts.detach().float().numpy(), f, R, T), mask), losses
