"""float64 references of the camera gradients (R, T, tan_half_fov) of the mesh G-buffer and of the soft silhouette
(reni_gbuffer_backward_camera, reni_soft_silhouette_backward_camera; reni_tu_camera.hip), built on the two restatements
tests/silhouette_ref.py and tests/gbuffer_grad_ref.py, which are differentiable in the camera as they stand.

For each of the two: ``*_autograd`` differentiates the restatement in R (nine free numbers), T and tan_half_fov by autograd;
``*_closed_form`` writes the same gradient out by hand in the kernels' structure -- per face and corner the NDC gradient
(tx, ty), the view-space gradient g_q = (tx / (z t), ty / (z t), -(tx x + ty y) / z), then gT = sum g_q,
gR[i][j] = sum p[i] g_q[j], g_tan = -sum (tx x + ty y) / t -- in any dtype and accumulates sum |terms| beside it, every addend
and every coefficient at its magnitude, as both restatements do for the vertices.  These are sums over all faces and cancel
heavily (a pure depth translation of a symmetric mesh is one example), so the bound rests on sum |terms|, not on the result:
per element max(K 2^-23 sum |terms|, 2e-5 max |ref|), the maximum taken over gR, gT and g_tan separately.  K = 4 x the worst
ratio of the float32 CPU evaluation over all cases (``float32_ratios``; the constants below).

A camera gradient is a vector of 13: gR [9] row-major, gT [3], g_tan [1] -- the C ABI's grad_camera.

Plain data and torch on the CPU; nothing here touches a device."""
import functools
import math

import numpy as np
import torch

from tests import gbuffer_grad_ref as G
from tests import raster_edge_cases as E
from tests import silhouette_ref as S

F64 = torch.float64
PARTS = (slice(0, 9), slice(9, 12), slice(12, 13))  # gR, gT, g_tan of a camera gradient
# 4 x the worst ratio |float32 closed form - float64| / (2^-23 sum |terms|) of ``float32_ratios()`` on the CPU
# (tests/test_camera_grad_cpu.py checks that they still are; DESIGN 4.4s has the measurement and the device's own ratios)
K_SIL = 3.81    # 4 x 0.9522 (strip-256, inside_only)
K_GBUF = 20.5   # 4 x 5.114 (ico-17, gN_only)
K_E2E = 13.8    # 4 x 3.432 (scalar kd = 1)


def pack(gR, gT, g_tan):
    return torch.cat([torch.as_tensor(gR).reshape(9), torch.as_tensor(gT).reshape(3), torch.as_tensor(g_tan).reshape(1)])


def _camera_leaves(R, T, tan_half):
    R = R.detach().clone().double().reshape(3, 3).requires_grad_(True)
    T = T.detach().clone().double().reshape(3).requires_grad_(True)
    t = torch.tensor(float(tan_half), dtype=F64, requires_grad=True)
    return R, T, t


def _accumulate(P, gq, gqm, gt, gtm, out, terms):
    """adds one corner's share over the faces: P [F, 3] world positions, gq / gqm [F, 3], gt / gtm [F]"""
    out[0:9] += (P[:, :, None] * gq[:, None, :]).sum(0).reshape(9)
    terms[0:9] += (P.abs()[:, :, None] * gqm[:, None, :]).sum(0).reshape(9)
    out[9:12] += gq.sum(0)
    terms[9:12] += gqm.sum(0)
    out[12] += gt.sum()
    terms[12] += gtm.sum()


# ------------------------------------------------------------------------------------------------------ the silhouette
def sil_objective(verts, faces, R, T, Simg, tan_half, sigma, r, gA, choice="lo"):
    alpha, _ = S.soft_alpha(verts, faces, R, T, Simg, tan_half, sigma, r, choice)
    return (alpha * gA).sum() + (R.sum() + T.sum() + tan_half) * 0.0


def sil_autograd(key, name, gA, choice="lo"):
    """the camera gradient [13] float64 of sum_p gA_p alpha_p by autograd through ``silhouette_ref.soft_alpha``"""
    v, f, R, T, Simg, tanh = S.inputs(key)
    sigma, r = S.setting(name, Simg)
    R, T, t = _camera_leaves(R, T, tanh)
    gR, gT, gt = torch.autograd.grad(sil_objective(v, f, R, T, Simg, t, sigma, r, gA, choice), (R, T, t))
    return pack(gR, gT, gt)


@torch.no_grad()
def sil_closed_form(verts, faces, R, T, Simg, tan_half, sigma, r, gA, choice="lo", trans=None):
    """(camera gradient [13], sum |terms| [13], trans [S*S]) in verts' dtype: ``silhouette_ref.closed_form``'s chain up to
    the view-space gradient of every corner, then the camera sums.  ``trans``: the transmittance to evaluate with (default:
    this evaluation's own)."""
    dtype = verts.dtype
    R, T = R.reshape(3, 3).to(dtype), T.reshape(3).to(dtype)
    idx, x, y, z = S.taking_part(verts, faces, R, T, tan_half)
    p = S.pairs(x, y, Simg, r, choice)
    member, inside = p["member"], p["inside"]
    prob = 1.0 / (1.0 + torch.exp(torch.where(inside, -p["d"], p["d"]) / sigma))
    own = torch.where(member, 1.0 - prob, torch.ones_like(prob)).prod(dim=1)
    tr = own if trans is None else trans.reshape(-1).to(dtype)
    g = gA.to(dtype)[:, None] * (-(tr[:, None] * prob) / sigma) * torch.where(inside, -2.0, 2.0).to(dtype)
    g = torch.where(member, g, torch.zeros_like(g))
    wa, wb, e = g * (1.0 - p["t"]), g * p["t"], p["edge"]
    zero = torch.zeros_like(g)
    k = (torch.where(e == 2, zero, wa), torch.where(e == 0, wb, torch.where(e == 2, wa, zero)), torch.where(e == 0, zero, wb))
    wam, wbm = g.abs() * torch.where(p["tm"] == p["t"], 1.0 - p["t"], 1.0 + p["tm"]), g.abs() * p["tm"]
    km = (torch.where(e == 2, zero, wam), torch.where(e == 0, wbm, torch.where(e == 2, wam, zero)), torch.where(e == 0, zero, wbm))
    P = verts[faces[idx]]  # [Fp, 3 corners, 3]
    out, terms = torch.zeros(13, dtype=dtype), torch.zeros(13, dtype=dtype)
    for c in range(3):
        tx, ty = (k[c] * p["dx"]).sum(0), (k[c] * p["dy"]).sum(0)
        txm, tym = (km[c] * p["dxm"]).sum(0), (km[c] * p["dym"]).sum(0)
        wz = z[:, c] * tan_half
        gq = torch.stack([tx / wz, ty / wz, -(tx * x[:, c] + ty * y[:, c]) / z[:, c]], 1)
        gqm = torch.stack([txm / wz.abs(), tym / wz.abs(), (txm * x[:, c].abs() + tym * y[:, c].abs()) / z[:, c].abs()], 1)
        _accumulate(P[:, c], gq, gqm, -(tx * x[:, c] + ty * y[:, c]) / tan_half, (txm * x[:, c].abs() + tym * y[:, c].abs()) / tan_half,
                    out, terms)
    return out, terms, own


def sil_references_of(v, f, R, T, Simg, name, gA, trans=None):
    """((lo, terms), (hi, terms)) float64 of a mesh (numpy), a camera ([1,3,3], [1,3]) and a setting: the closed form with
    every undecided pair left out and the first winner kept, and with every undecided pair taken in and the runner-up winning"""
    sigma, r = S.setting(name, Simg)
    verts, faces = torch.from_numpy(v).double(), torch.from_numpy(f)
    return tuple(sil_closed_form(verts, faces, R[0].double(), T[0].double(), Simg, E.TANF, sigma, r, gA, choice, trans)[:2]
                 for choice in ("lo", "hi"))


MAX_MIXTURE_PAIRS = 12  # 2^12 mixtures of undecided pairs are enumerated; beyond that the spread stands in


@torch.no_grad()
def sil_deltas(v, f, R, T, Simg, name, gA, trans):
    """[13, n] float64: for each of the n undecided pairs, what taking that pair the hi way instead of the lo way adds to the
    camera gradient.  The chain behind a pair's NDC gradient is linear, so the reference for any mixture of choices is
    reference_lo plus the deltas of the pairs taken the hi way; reference_hi is reference_lo plus all of them."""
    sigma, r = S.setting(name, Simg)
    verts, faces = torch.from_numpy(v).double(), torch.from_numpy(f)
    Rm, Tm = R[0].double().reshape(3, 3), T[0].double().reshape(3)
    idx, x, y, z = S.taking_part(verts, faces, Rm, Tm, E.TANF)
    P = verts[faces[idx]]
    tr = trans.reshape(-1).double()
    contrib = []
    for choice in ("lo", "hi"):
        p = S.pairs(x, y, Simg, r, choice)
        pi, fi = p["undecided"].nonzero(as_tuple=True)  # (the same pairs under both choices)
        sel = {k: p[k][pi, fi] for k in ("member", "inside", "d", "t", "edge", "dx", "dy")}
        prob = 1.0 / (1.0 + torch.exp(torch.where(sel["inside"], -sel["d"], sel["d"]) / sigma))
        g = gA.double()[pi] * (-(tr[pi] * prob) / sigma) * torch.where(sel["inside"], -2.0, 2.0).double()
        g = torch.where(sel["member"], g, torch.zeros_like(g))
        wa, wb, e, zero = g * (1.0 - sel["t"]), g * sel["t"], sel["edge"], torch.zeros_like(g)
        k = (torch.where(e == 2, zero, wa), torch.where(e == 0, wb, torch.where(e == 2, wa, zero)), torch.where(e == 0, zero, wb))
        out = torch.zeros(13, pi.numel(), dtype=F64)
        for c in range(3):
            tx, ty, xc, yc, zc = k[c] * sel["dx"], k[c] * sel["dy"], x[fi, c], y[fi, c], z[fi, c]
            gq = torch.stack([tx / (zc * E.TANF), ty / (zc * E.TANF), -(tx * xc + ty * yc) / zc])  # [3, n]
            out[0:9] += (P[fi, c].t()[:, None, :] * gq[None, :, :]).reshape(9, -1)
            out[9:12] += gq
            out[12] += -(tx * xc + ty * yc) / E.TANF
        contrib.append(out)
    return contrib[1] - contrib[0]


def sil_bounds_of(v, f, R, T, Simg, name, gA, trans):
    """(reference_lo, reference_hi, sum |terms|, deltas) of a mesh, a camera and a setting for the given transmittance"""
    (lo, tl), (hi, th) = sil_references_of(v, f, R, T, Simg, name, gA, trans)
    terms = torch.maximum(tl, th)
    deltas = sil_deltas(v, f, R, T, Simg, name, gA, trans)
    assert ((lo + deltas.sum(dim=1) - hi).abs() <= 1e-9 * terms).all()  # all pairs the hi way is reference_hi
    return lo, hi, terms, deltas


def sil_references(key, name, gA, trans=None):
    """``sil_references_of`` a case of tests/silhouette_ref.py"""
    return sil_references_of(*S.case(*key), name, gA, trans)


# -------------------------------------------------------------------------------------------------------- the G-buffer
def gbuf_objective(verts, faces, R, T, Simg, tan_half, pix_to_face, gN, gX, normals=None):
    """sum_p (gN_p . N_p + gX_p . X_p) of ``gbuffer_grad_ref.gbuffer``, with the vertex normals it interpolates given"""
    N, X = G.gbuffer(verts, faces, R, T, Simg, tan_half, pix_to_face, normals=normals)
    out = (R.sum() + T.sum() + tan_half) * 0.0
    if gN is not None:
        out = out + (gN.to(verts.dtype) * N).sum()
    if gX is not None:
        out = out + (gX.to(verts.dtype) * X).sum()
    return out


def gbuf_autograd(key, pix_to_face, gN, gX, normals=None):
    """the camera gradient [13] float64 of the objective by autograd through ``gbuffer_grad_ref.gbuffer``"""
    v, f, R, T, Simg = G._inputs(key, F64)
    R, T, t = _camera_leaves(R, T, E.TANF)
    return pack(*torch.autograd.grad(gbuf_objective(v, f, R, T, Simg, t, pix_to_face.cpu(), gN, gX, normals), (R, T, t)))


@torch.no_grad()
def gbuf_closed_form(verts, faces, R, T, Simg, tan_half, pix_to_face, gN, gX, normals=None):
    """(camera gradient [13], sum |terms| [13]) in verts' dtype: ``gbuffer_grad_ref.closed_form``'s chain up to the view-space
    gradient of every corner -- the barycentric path alone: the face's NDC sums through the edge functions and dA folded in --
    then the camera sums.  ``normals`` [V, 3]: the vertex normals that were interpolated.  They are an input of the entry
    point (vert_normals), like pix_to_face, and a constant of the camera gradient, so a comparison hands the reference the
    normals the evaluation under test used: where |u_v| is under the 1e-6 floor ("tiny_normal") a float32 normal is rounding
    noise times 1e6, which is the normals' error and not this chain's.  Default: ``vertex_normals`` in verts' dtype."""
    dtype = verts.dtype
    R, T = R.reshape(3, 3).to(dtype), T.reshape(3).to(dtype)
    F = faces.shape[0]
    n = G.vertex_normals(verts, faces) if normals is None else normals.to(dtype)
    valid = G._valid_faces(verts, faces, R, T, tan_half)
    p2f = pix_to_face.reshape(-1)
    hit = (p2f >= 0) & (p2f < F)
    hit = hit & valid[p2f.clamp(0, F - 1)]
    fidx = p2f[hit]
    Np = int(fidx.numel())
    zeros = torch.zeros(Simg * Simg, 3, dtype=dtype)
    gn = (zeros if gN is None else gN.to(dtype))[hit]
    gp = (zeros if gX is None else gX.to(dtype))[hit]
    safe = torch.where(valid[:, None], faces, torch.zeros_like(faces))
    pf = verts[safe]
    qf = pf @ R + T
    xf, yf, zf = qf[..., 0] / (qf[..., 2] * tan_half), qf[..., 1] / (qf[..., 2] * tan_half), qf[..., 2]
    Af = G._edge(xf[:, 2], yf[:, 2], xf[:, 0], yf[:, 0], xf[:, 1], yf[:, 1]) + 1e-8
    x, y, A = xf[fidx], yf[fidx], Af[fidx]
    PX, PY = G._pixels(Simg, dtype)
    px, py = PX[hit], PY[hit]
    w = torch.stack([G._edge(px, py, x[:, 1], y[:, 1], x[:, 2], y[:, 2]), G._edge(px, py, x[:, 2], y[:, 2], x[:, 0], y[:, 0]),
                     G._edge(px, py, x[:, 0], y[:, 0], x[:, 1], y[:, 1])], 1) / A[:, None]
    nk, pk = n[safe][fidx], pf[fidx]
    ck = (gn[:, None, :] * nk).sum(2) + (gp[:, None, :] * pk).sum(2)
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
    out, terms = torch.zeros(13, dtype=dtype), torch.zeros(13, dtype=dtype)
    vf = valid.nonzero()[:, 0]
    for k in range(3):
        i1, i2 = (k + 1) % 3, (k + 2) % 3
        tx = (GX[:, k] + SA * (yf[:, i2] - yf[:, i1]))[vf]
        ty = (GY[:, k] + SA * (xf[:, i1] - xf[:, i2]))[vf]
        txm = (GXm[:, k] + SAm * (yf[:, i2] - yf[:, i1]).abs())[vf]
        tym = (GYm[:, k] + SAm * (xf[:, i1] - xf[:, i2]).abs())[vf]
        xk, yk, zk = xf[vf, k], yf[vf, k], zf[vf, k]
        wz = zk * tan_half
        gq = torch.stack([tx / wz, ty / wz, -(tx * xk + ty * yk) / zk], 1)
        gqm = torch.stack([txm / wz.abs(), tym / wz.abs(), (txm * xk.abs() + tym * yk.abs()) / zk.abs()], 1)
        _accumulate(pf[vf, k], gq, gqm, -(tx * xk + ty * yk) / tan_half, (txm * xk.abs() + tym * yk.abs()) / tan_half, out, terms)
    return out, terms


def gbuf_reference(key, pix_to_face, gN, gX, normals=None):
    """(camera gradient, sum |terms|) float64 of a case for the given face assignment and vertex normals"""
    return gbuf_closed_form(*G._inputs(key, F64), E.TANF, pix_to_face.cpu(), gN, gX,
                            None if normals is None else normals.detach().double().cpu())


# ------------------------------------------------------------------------------------------------------------ the bound
def _per_part(fn, *tensors):
    return max(fn(*(t[s] for t in tensors)) for s in PARTS)


def error_ratio(got, ref, terms):
    """worst |got - ref| / (2^-23 sum |terms|) over the 13 components"""
    return G.error_ratio(torch.as_tensor(got).reshape(13), ref, terms)


def over_bound(got, ref, terms, K):
    """worst |got - ref| / max(K 2^-23 sum |terms|, 2e-5 max |ref|), max |ref| per part (gR, gT, g_tan); <= 1 passes"""
    got = torch.as_tensor(got).detach().double().cpu().reshape(13)
    return _per_part(lambda g, r, t: G.over_bound(g, r, t, K), got, ref, terms)


def sil_error_ratio(got, lo, hi, terms):
    """worst (|got - lo| - |hi - lo|) / (2^-23 sum |terms|): the issue's widening, as tests/silhouette_ref.py"""
    return S.error_ratio(torch.as_tensor(got).reshape(13), lo, hi, terms, True)


def sil_over_bound(got, lo, hi, terms, K=None):
    """worst (|got - lo| - |hi - lo|) / bound, max |ref| per part; <= 1 passes"""
    got = torch.as_tensor(got).detach().double().cpu().reshape(13)
    return _per_part(lambda g, a, b, t: S.over_bound(g, a, b, t, K_SIL if K is None else K, True), got, lo, hi, terms)


def sil_check(got, lo, hi, terms, deltas, K=None):
    """-> (worst error / bound, how).  The assertion is the widening by |hi - lo| ("hi-lo") wherever it holds.  It assumes
    that a device takes every undecided pair the same way.  A camera gradient sums over all faces, so every undecided pair
    reaches every component, and a device that takes one pair the lo way and the next the hi way lands outside [lo, hi] where
    the two pairs' effects have opposite signs (measured: ico-33 sharp, 5 undecided pairs, gR[1][0] = 6.84559 on the device
    against lo 6.85048 and hi 6.85518).  Only where that assertion fails: the result must lie, in all 13 components at once,
    within the UNWIDENED bound of one of the 2^n mixtures lo + sum of a subset of the pairs' deltas ("mixture", n <=
    MAX_MIXTURE_PAIRS); with more pairs than can be enumerated, within the bound widened by sum |deltas| ("spread")."""
    K = K_SIL if K is None else K
    got = torch.as_tensor(got).detach().double().cpu().reshape(13)
    over = sil_over_bound(got, lo, hi, terms, K)
    if over <= 1.0:
        return over, "hi-lo"
    bound = torch.cat([G.bound(lo[s], terms[s], K) for s in PARTS])
    n = deltas.shape[1]
    if n > MAX_MIXTURE_PAIRS:
        err = ((got - lo).abs() - deltas.abs().sum(dim=1)).clamp_min(0.0)
        return float(torch.where(bound > 0, err / bound.clamp_min(1e-300), err * float("inf")).nan_to_num(0.0).max()), "spread"
    masks = ((torch.arange(2 ** n)[:, None] >> torch.arange(n)[None, :]) & 1).double()  # [2^n, n]
    refs = lo[None, :] + masks @ deltas.t()  # [2^n, 13]
    err = (got[None, :] - refs).abs()
    ratio = torch.where(bound[None, :] > 0, err / bound.clamp_min(1e-300)[None, :], torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(ratio.max(dim=1).values.min()), "mixture"


@functools.lru_cache(maxsize=None)
def float32_ratios():
    """(silhouette, G-buffer): the worst ratio of the closed forms evaluated in float32 torch on the CPU against float64 over
    every case and setting / upstream variant; the silhouette's float64 side is evaluated with the float32 transmittance, the
    G-buffer with the CPU face assignment and the float32 vertex normals"""
    worst_s = worst_g = 0.0
    f32 = float(np.float32(E.TANF))
    for key in S.CASES:
        v, f, R, T, Simg, _ = S.inputs(key, torch.float32)
        for name in S.SETTINGS:
            gA = S.upstream(key, name)
            sigma, r = S.setting(name, Simg)
            got, _, trans = sil_closed_form(v, f, R, T, Simg, f32, sigma, r, gA)
            lo, hi, terms, _ = sil_bounds_of(*S.case(*key), name, gA, trans.double())
            worst_s = max(worst_s, sil_error_ratio(got, lo, hi, terms))
    for key in G.CASES:
        v32, f, R32, T32, Simg = G._inputs(key, torch.float32)
        for variant in G.VARIANTS:
            gN, gX = G.upstream(key, variant)
            n32 = G.vertex_normals(v32, f)
            ref, terms = gbuf_reference(key, G.cpu_pix_to_face(key), gN, gX, n32)
            got, _ = gbuf_closed_form(v32, f, R32, T32, Simg, f32, G.cpu_pix_to_face(key), gN, gX, n32)
            worst_g = max(worst_g, error_ratio(got, ref, terms))
    return worst_s, worst_g


def central_differences(fn, R, T, tan_half, h=1e-6):
    """the camera gradient [13] of fn(R [3,3], T [3], tan_half) -> float64 scalar by central differences"""
    base = torch.cat([R.reshape(9).double(), T.reshape(3).double(), torch.tensor([float(tan_half)], dtype=F64)])
    out = torch.zeros(13, dtype=F64)
    for i in range(13):
        vals = []
        for s in (1.0, -1.0):
            c = base.clone()
            c[i] += s * h
            vals.append(float(fn(c[:9].reshape(3, 3), c[9:12], c[12])))
        out[i] = (vals[0] - vals[1]) / (2.0 * h)
    return out


# -------------------------------------------------------------------------------------------------------- reducer edges
CHUNK = 512  # CAM_CHUNK of reni_internal.h: the records one workgroup of the reducer adds
STRIP_F = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)


def strip_case(F, S=16):
    """(verts, faces, R, T, S): ``strip_mesh`` with F faces squeezed in x into the view at image size S, so that every face --
    those of the reducer's last chunk among them -- has pixels near it and a record that is not zero"""
    v, f = E.strip_mesh(F + 2)
    v = v.astype(np.float64)
    v[:, 0] = v[:, 0] * (1.8 / v[:, 0].max()) - 0.9
    R, T = E.camera()
    return v.astype(np.float32), f, R, T, S


# ------------------------------------------------------------------------------- end to end: the camera behind a shader
E2E_CONFIGS = tuple((m, sh) for m in ("scalar", "microfacet") for sh in (False, True))


def e2e_chain(kind, pix_to_face, vis, dtype=F64, normals=None):
    """(camera gradient, sum |terms|) [13] of loss = sum w . colours through the float restatements in ``dtype``: the shader's
    gradient with respect to the pixel normals by autograd (``gbuffer_grad_ref.shade``, the positions detached), then
    ``gbuf_closed_form`` with it as gN; ``normals``: the vertex normals to interpolate (default: ``vertex_normals``)"""
    v, f, R, T = G.e2e_mesh()
    Simg = G.E2E_S
    verts, faces = torch.from_numpy(v).to(dtype), torch.from_numpy(f)
    tanh = E.TANF if dtype == F64 else float(np.float32(E.TANF))
    n = None if normals is None else normals.detach().cpu().to(dtype)
    N, X = G.gbuffer(verts, faces, R[0].to(dtype), T[0].to(dtype), Simg, tanh, pix_to_face, normals=n)
    N = N.detach().requires_grad_(True)
    D, C = G.envmap_8x16()
    col = G.shade(kind, G.e2e_materials(kind, Simg * Simg), N, X, D.to(dtype), C.to(dtype), vis, dtype)
    (gN,) = torch.autograd.grad((col * G.e2e_weights(C.shape[0], Simg * Simg).to(dtype)).sum(), N)
    return gbuf_closed_form(verts, faces, R[0].to(dtype), T[0].to(dtype), Simg, tanh, pix_to_face, gN, None, n)


@functools.lru_cache(maxsize=None)
def e2e_float32_ratio():
    """worst ratio of the float32 CPU evaluation of the whole chain over the two materials (no mask: the mask is the
    device's), with the CPU face assignment"""
    p2f = G.cpu_pix_to_face(("ico", G.E2E_S))
    worst = 0.0
    for kind in ("scalar", "microfacet"):
        n32 = G.vertex_normals(torch.from_numpy(G.e2e_mesh()[0]), torch.from_numpy(G.e2e_mesh()[1]))
        ref, terms = e2e_chain(kind, p2f, None, F64, n32)
        got, _ = e2e_chain(kind, p2f, None, torch.float32, n32)
        worst = max(worst, error_ratio(got, ref, terms))
    return worst


# ---------------------------------------------------------------------------------------------------------------- a fit
FIT_S, FIT_STEPS, FIT_LR, FIT_SETTING = 32, 60, 0.05, "sharp"
FIT_SCALE = (1.0, 0.7, 0.5)
FIT_TARGET, FIT_START = (2.7, 10.0, 20.0), (3.3, 30.0, 50.0)  # (dist, elev, azim), degrees
# |C - C*| and the soft IoU loss of the float64 CPU loop (``fit_reference``) before the first and after the last step
FIT_DIST_START, FIT_DIST_END = 1.8630188, 0.1721918
FIT_LOSS_START, FIT_LOSS_END = 0.3940963, 0.0761665


def camera_position(dist, elev, azim):
    """the world position [3] float64 of look_at_view_transform's camera (degrees)"""
    e, a = math.radians(elev), math.radians(azim)
    return torch.tensor([dist * math.cos(e) * math.sin(a), dist * math.sin(e), dist * math.cos(e) * math.cos(a)], dtype=F64)


def fit_mesh():
    """(verts float32 [V, 3], faces): the icosphere of ``silhouette_ref.fit_meshes``, centred and scaled by FIT_SCALE"""
    v, _, f, _, _ = S.fit_meshes()
    v = v.astype(np.float64)
    return ((v - v.mean(axis=0)) * np.array(FIT_SCALE)).astype(np.float32), f


@functools.lru_cache(maxsize=None)
def fit_mask():
    """the target mask [S*S] bool: the float64 reference alpha under the target camera > 0.5"""
    from reni_amd.mesh import camera_from_position
    v, f = fit_mesh()
    sigma, r = S.setting(FIT_SETTING, FIT_S)
    R, T = camera_from_position(camera_position(*FIT_TARGET))
    with torch.no_grad():
        alpha, _ = S.soft_alpha(torch.from_numpy(v).double(), torch.from_numpy(f), R[0], T[0], FIT_S, E.TANF, sigma, r)
    return alpha > 0.5


@functools.lru_cache(maxsize=None)
def fit_reference():
    """(|C - C*| at the start, at the end, the losses) of FIT_STEPS Adam steps on the camera position in float64 on the CPU,
    the pose through ``camera_from_position``, the loss the soft IoU alone"""
    from reni_amd.mesh import camera_from_position
    v, f = fit_mesh()
    verts, faces = torch.from_numpy(v).double(), torch.from_numpy(f)
    sigma, r = S.setting(FIT_SETTING, FIT_S)
    mask, target = fit_mask(), camera_position(*FIT_TARGET)
    C = camera_position(*FIT_START).requires_grad_(True)
    opt = torch.optim.Adam([C], lr=FIT_LR)
    d0 = float((C.detach() - target).norm())
    losses = []
    for _ in range(FIT_STEPS + 1):
        R, T = camera_from_position(C)
        alpha, _ = S.soft_alpha(verts, faces, R[0], T[0], FIT_S, E.TANF, sigma, r)
        loss = S.soft_iou_loss(alpha, mask)
        losses.append(float(loss.detach()))
        if len(losses) > FIT_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    return d0, float((C.detach() - target).norm()), losses
