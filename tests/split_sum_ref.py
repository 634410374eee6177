"""float64 reference of split-sum shading from a prefiltered chain (reni_tu_splitsum.hip, glossy.sample / ggx_dfg /
shade_split_sum), in plain torch: the lookup in the forward's own conventions, the DFG rule, and shade_split_sum.  Its autograd
is the reference for every gradient of the feature.  Besides the definitions: the closed form of the query's derivative evaluated
in a chosen dtype (``dquery_closed``: in float32 it is the emulation the GPU test takes its factor K from), the sums of the
absolute values of its terms (``dquery_scales``), a direct quadrature of DESIGN 4.4m's k and k f (``dfg_direct``), and the GPU
test's queries.

The lookup (k_envmap_lookup): phi = atan2(sqrt(x^2 + z^2), y), theta = atan2(x, -z), row = phi H / pi - 1/2,
col = theta W / (2 pi) + W / 2 - 1/2; the four taps around (row, col), a row beyond a pole folded back to the far side
(W / 2 columns away), a column wrapped across the seam; the level clamped to [0, Lv - 1], l0 = min(floor(level), Lv - 2) and
the next level mixed linearly (at the top knot that is the pair (Lv - 2, Lv - 1) with fraction 1: the same value as the
forward's, and the left-sided slope).  The derivative with respect to a direction is defined as 0 at a pole direction and for
the zero vector; with respect to the level it is 0 outside the closed range and for a NaN.
"""
import functools
import math

import torch

F64 = torch.float64
EPS32 = 2.0 ** -23
FLOOR = 2e-5  # of the largest reference value, as in tests/microfacet_ref.py


# ------------------------------------------------------------------------------------------------ the lookup
def coords(dirs, H, W):
    """(row, col, ok) of directions [..., 3] in their own dtype; ok: where the derivative is not defined as 0.  The gradient
    flows through the ok entries only (the others keep the forward's value: atan2(0, -0) = pi and so on)."""
    x, y, z = dirs.unbind(-1)
    rho2, q2 = x * x + z * z, x * x + y * y + z * z
    ok = (rho2 > 0) & (q2 > 0)
    phi_v = torch.atan2(torch.sqrt(rho2.detach()), y.detach())
    theta_v = torch.atan2(x.detach(), -z.detach())
    safe = torch.where(ok[..., None], dirs, torch.tensor([1.0, 0.0, 0.0], dtype=dirs.dtype).expand_as(dirs))
    xs, ys, zs = safe.unbind(-1)
    phi_s = torch.atan2(torch.sqrt(xs * xs + zs * zs), ys)
    theta_s = torch.atan2(xs, -zs)
    okf = ok.to(dirs.dtype)
    phi = phi_v + (phi_s - phi_s.detach()) * okf
    theta = theta_v + (theta_s - theta_s.detach()) * okf
    row = phi * (H / math.pi) - 0.5
    col = theta * (W / (2.0 * math.pi)) + (0.5 * W - 0.5)
    return row, col, ok


def taps(row, col, H, W):
    """the forward's folded taps: (fr, fc, rows (i0, i1), columns (j00, j01, j10, j11)); integer tensors"""
    fi, fj = torch.floor(row.detach()), torch.floor(col.detach())
    fr, fc = row - fi, col - fj
    i, j = fi.long(), fj.long()
    half = W // 2
    i0, i1 = i, i + 1
    x0, x1 = (i0 < 0) | (i0 >= H), i1 >= H
    i0 = torch.where(i0 < 0, -1 - i0, i0)
    i0 = torch.where(i0 >= H, 2 * H - 1 - i0, i0).clamp(0, H - 1)
    i1 = torch.where(i1 >= H, 2 * H - 1 - i1, i1).clamp(0, H - 1)
    j0, j1 = j % W, (j + 1) % W
    j0f, j1f = (j0 + half) % W, (j1 + half) % W
    return fr, fc, (i0, i1), (torch.where(x0, j0f, j0), torch.where(x0, j1f, j1), torch.where(x1, j0f, j0), torch.where(x1, j1f, j1))


def level_pair(level, Lv):
    """(la, lb, fl): the pair of levels and the fraction, differentiable in level (0 outside the closed range, NaN -> level 0)"""
    nan = torch.isnan(level)
    lv = torch.where(nan, torch.zeros_like(level), level).clamp(0.0, float(Lv - 1))
    la = torch.floor(lv.detach()).long().clamp(max=Lv - 2).clamp(min=0)
    lb = (la + 1).clamp(max=Lv - 1)
    fl = (lv - la) if Lv > 1 else torch.zeros_like(lv)
    return la, lb, fl


def _bilinear(m, n_idx, l, fr, fc, ii, jj):
    """m [N, Lv, H, W, 3]; n_idx, l and the taps broadcast to [N, P] -> [N, P, 3]"""
    i0, i1 = ii
    j00, j01, j10, j11 = jj
    b00, b01, b10, b11 = m[n_idx, l, i0, j00], m[n_idx, l, i0, j01], m[n_idx, l, i1, j10], m[n_idx, l, i1, j11]
    fr, fc = fr[..., None], fc[..., None]
    return (1 - fr) * ((1 - fc) * b00 + fc * b01) + fr * ((1 - fc) * b10 + fc * b11)


def lookup_ref(maps, dirs, level=None, dtype=F64):
    """out [N, P, 3] of maps [N, H, W, 3] / [N, Lv, H, W, 3] at dirs [P, 3] / [N, P, 3] and level (None, a number, [P] or
    [N, P]); differentiable in all three."""
    m = maps.to(dtype)
    if m.dim() == 4:
        m = m.unsqueeze(1)
    N, Lv, H, W, _ = m.shape
    d = dirs.to(dtype)
    d = d.unsqueeze(0).expand(N, -1, -1) if d.dim() == 2 else d
    P = d.shape[1]
    row, col, _ = coords(d, H, W)
    fr, fc, ii, jj = taps(row, col, H, W)
    lv = torch.as_tensor(0.0 if level is None else level, dtype=dtype)
    lv = lv.expand(N, P) if lv.dim() < 2 else lv
    la, lb, fl = level_pair(lv, Lv)
    n_idx = torch.arange(N)[:, None].expand(N, P)
    va = _bilinear(m, n_idx, la, fr, fc, ii, jj)
    vb = _bilinear(m, n_idx, lb, fr, fc, ii, jj)
    return (1 - fl)[..., None] * va + fl[..., None] * vb


def dquery_closed(maps, dirs, level, grad_out, dtype=torch.float32, absolute=False):
    """The closed form reni_envmap_lookup_dquery evaluates, in ``dtype`` (float32: the emulation of the kernel, in its order up
    to the fused multiply-adds): (d_dirs shaped like dirs, d_level shaped like level or None).  absolute: every term at its
    absolute value -- the sums the rounding of the closed form is measured against (``dquery_scales``)."""
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    sub = (lambda a, b: a.abs() + b.abs()) if absolute else (lambda a, b: a - b)
    m = maps.to(dtype)
    if m.dim() == 4:
        m = m.unsqueeze(1)
    N, Lv, H, W, _ = m.shape
    d0 = dirs.detach().to(dtype)
    shared_d = d0.dim() == 2
    d = d0.unsqueeze(0).expand(N, -1, -1) if shared_d else d0
    P = d.shape[1]
    g = grad_out.to(dtype)
    x, y, z = d.unbind(-1)
    rho2 = x * x + z * z
    q2 = rho2 + y * y
    row_scale = torch.tensor(H / math.pi, dtype=dtype)
    col_scale = torch.tensor(W / (2.0 * math.pi), dtype=dtype)
    row = torch.atan2(torch.sqrt(rho2), y) * row_scale - 0.5
    col = torch.atan2(x, -z) * col_scale + torch.tensor(0.5 * W - 0.5, dtype=dtype)
    fr, fc, (i0, i1), (j00, j01, j10, j11) = taps(row, col, H, W)
    gr, gc = 1 - fr, 1 - fc
    tensor_level = isinstance(level, torch.Tensor) and level.dim() > 0
    lv0 = torch.as_tensor(0.0 if level is None else level).detach().to(dtype)
    shared_l = lv0.dim() < 2
    lv = lv0.expand(N, P) if shared_l else lv0
    lvc = torch.where(torch.isnan(lv), torch.zeros_like(lv), lv).clamp(0.0, float(Lv - 1))
    l0 = torch.floor(lvc).long()
    fl = lvc - l0
    la = l0.clamp(max=Lv - 2).clamp(min=0)
    lb = (la + 1).clamp(max=Lv - 1)
    top = l0 != la
    wa = torch.where(top, torch.zeros_like(fl), 1 - fl)
    wb = torch.where(top, torch.ones_like(fl), fl)
    n_idx = torch.arange(N)[:, None].expand(N, P)

    def four(l):
        return m[n_idx, l, i0, j00], m[n_idx, l, i0, j01], m[n_idx, l, i1, j10], m[n_idx, l, i1, j11]

    a00, a01, a10, a11 = four(la)
    b00, b01, b10, b11 = four(lb)
    e = lambda t: t[..., None]
    dra = e(gc) * sub(a10, a00) + e(fc) * sub(a11, a01)
    drb = e(gc) * sub(b10, b00) + e(fc) * sub(b11, b01)
    dca = e(gr) * sub(a01, a00) + e(fr) * sub(a11, a10)
    dcb = e(gr) * sub(b01, b00) + e(fr) * sub(b11, b10)
    Gr = (ab(g) * (e(wa) * dra + e(wb) * drb)).sum(-1)
    Gc = (ab(g) * (e(wa) * dca + e(wb) * dcb)).sum(-1)
    if absolute:
        va = e(gr) * (e(gc) * a00.abs() + e(fc) * a01.abs()) + e(fr) * (e(gc) * a10.abs() + e(fc) * a11.abs())
        vb = e(gr) * (e(gc) * b00.abs() + e(fc) * b01.abs()) + e(fr) * (e(gc) * b10.abs() + e(fc) * b11.abs())
    else:
        va = e(gr) * (e(gc) * a00 + e(fc) * a01) + e(fr) * (e(gc) * a10 + e(fc) * a11)
        vb = e(gr) * (e(gc) * b00 + e(fc) * b01) + e(fr) * (e(gc) * b10 + e(fc) * b11)
    Gl = (ab(g) * sub(vb, va)).sum(-1)
    if shared_d:
        Gr, Gc = Gr.sum(0, keepdim=True), Gc.sum(0, keepdim=True)
        x, y, z, rho2, q2, row = x[:1], y[:1], z[:1], rho2[:1], q2[:1], row[:1]
    ok = (rho2 > 0) & (q2 > 0) & torch.isfinite(q2) & (row > -1) & (row < H)
    one = torch.ones_like(rho2)
    rho2s, q2s = torch.where(ok, rho2, one), torch.where(ok, q2, one)
    rho = torch.sqrt(rho2s)
    tr, tc = row_scale * Gr, col_scale * Gc
    px, py, pz = (y / q2s) * (x / rho), -(rho / q2s), (y / q2s) * (z / rho)
    tx, tz = -z / rho2s, x / rho2s
    if absolute:
        dd = torch.stack((tr * px.abs() + tc * tx.abs(), tr * py.abs(), tr * pz.abs() + tc * tz.abs()), -1)
    else:
        dd = torch.stack((tr * px + tc * tx, tr * py, tr * pz + tc * tz), -1)
    dd = torch.where(ok[..., None], dd, torch.zeros_like(dd))
    dd = dd[0] if shared_d else dd
    dl = None
    if tensor_level:
        inr = (lv >= 0) & (lv <= Lv - 1) & (Lv > 1)
        if shared_l:
            dl = torch.where(inr[0], Gl.sum(0), torch.zeros_like(Gl[0])).reshape(lv0.shape)
        else:
            dl = torch.where(inr, Gl, torch.zeros_like(Gl))
    return dd, dl


def dquery_scales(maps, dirs, level, grad_out):
    """float64 sums of the absolute values of the terms of (d_dirs, d_level)"""
    return dquery_closed(maps, dirs, level, grad_out, dtype=F64, absolute=True)


def dquery_autograd(maps, dirs, level, grad_out):
    """(d_dirs, d_level) by float64 autograd of ``lookup_ref``"""
    d = dirs.detach().to(F64).clone().requires_grad_(True)
    tensor_level = isinstance(level, torch.Tensor) and level.dim() > 0
    lv = level.detach().to(F64).clone().requires_grad_(True) if tensor_level else level
    out = lookup_ref(maps, d, lv)
    grads = torch.autograd.grad((out * grad_out.to(F64)).sum(), (d, lv) if tensor_level else (d,), allow_unused=True)
    dl = grads[1] if tensor_level else None
    if dl is None and tensor_level:
        dl = torch.zeros_like(lv)
    return grads[0], dl


def bound(ref, scale, factor):
    """max(factor EPS32 scale, FLOOR largest |ref|), elementwise in the reference's shape"""
    floor = FLOOR * float(ref.abs().max()) if ref.numel() else 0.0
    return (factor * EPS32 * scale).clamp_min(floor)


def error_ratio(got, ref, scale):
    """worst |got - ref| / (EPS32 scale) over the elements whose scale is positive; where it is 0 the value must be exact"""
    err = (torch.as_tensor(got).detach().double().cpu() - ref).abs()
    exact = scale <= 0
    if bool((err[exact] > 0).any()):
        return float("inf")
    r = err[~exact] / (EPS32 * scale[~exact])
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ the GPU test's queries
def make_queries(H, W, Lv, P, seed, N=None):
    """Queries from target (row, col, level) whose fractional parts lie in [0.15, 0.85]: the interior, rows in (-0.5, 0) and
    (H - 1, H - 0.5) beyond each pole, columns across the seam on both sides, lengths from 0.3 to 3.  -> (dirs, level), float32,
    [P, 3] / [P] or with N [N, P, 3] / [N, P]."""
    g = torch.Generator().manual_seed(seed)
    shape = (P,) if N is None else (N, P)
    frac = lambda: 0.15 + 0.7 * torch.rand(shape, generator=g, dtype=F64)
    row = torch.randint(0, max(H - 1, 1), shape, generator=g).double() + frac()
    col = torch.randint(0, W - 1, shape, generator=g).double() + frac()
    kind = torch.randint(0, 8, shape, generator=g)
    row = torch.where(kind == 0, -0.45 + 0.3 * torch.rand(shape, generator=g, dtype=F64), row)          # beyond the first pole
    row = torch.where(kind == 1, (H - 1) + 0.15 + 0.3 * torch.rand(shape, generator=g, dtype=F64), row)  # beyond the last
    col = torch.where(kind == 2, -0.45 + 0.3 * torch.rand(shape, generator=g, dtype=F64), col)          # the seam, low side
    col = torch.where(kind == 3, (W - 1) + 0.15 + 0.3 * torch.rand(shape, generator=g, dtype=F64), col)  # the seam, high side
    phi = (row + 0.5) * (math.pi / H)
    theta = (col - 0.5 * W + 0.5) * (2.0 * math.pi / W)
    length = 0.3 + 2.7 * torch.rand(shape, generator=g, dtype=F64)
    d = torch.stack((torch.sin(phi) * torch.sin(theta), torch.cos(phi), -torch.sin(phi) * torch.cos(theta)), -1) * length[..., None]
    level = (torch.randint(0, max(Lv - 1, 1), shape, generator=g).double() + frac()) if Lv > 1 else frac()
    return d.float(), level.float()


def same_cells(dirs, level, H, W, Lv):
    """do the float32 and the float64 evaluation of the coordinates land in the same cell, for every query?"""
    out = []
    for dt in (torch.float32, F64):
        d = dirs.to(dt)
        x, y, z = d.unbind(-1)
        row = torch.atan2(torch.sqrt(x * x + z * z), y) * torch.tensor(H / math.pi, dtype=dt) - 0.5
        col = torch.atan2(x, -z) * torch.tensor(W / (2.0 * math.pi), dtype=dt) + (0.5 * W - 0.5)
        out.append((torch.floor(row).long(), torch.floor(col).long(), torch.floor(level.to(dt).clamp(0, Lv - 1)).long()))
    return all(bool((a == b).all()) for a, b in zip(*out))


# ------------------------------------------------------------------------------------------------ the DFG table
def _lam(t, al2):
    return torch.sqrt(al2 + (1.0 - al2) * t * t)


def dfg_rule_at(x, r, M_u=128, M_phi=128, dtype=F64, scale=False):
    """(A0, A1) at N.V = x and roughness = r (tensors of one shape) by the rule reni_ggx_dfg is defined as.  scale: A1's terms
    with f replaced by f + 5 (1 - V.H)^4 V.H -- what one rounding of V.H moves f = (1 - V.H)^5 by, in units of that rounding:
    the scale an fp32 evaluation of A1 is held against (A0's terms are positive: its scale is its value)."""
    x, r = torch.as_tensor(x, dtype=dtype).reshape(-1, 1, 1), torch.as_tensor(r, dtype=dtype).reshape(-1, 1, 1)
    al = r * r
    al2 = al * al
    u = ((torch.arange(M_u, dtype=dtype) + 0.5) / M_u).reshape(1, -1, 1)
    phi = (2.0 * math.pi * ((torch.arange(M_phi, dtype=dtype) + 0.5) / M_phi)).reshape(1, 1, -1)
    c2 = (1.0 - u) / (al2 * u + (1.0 - u))  # 1 + (alpha^2 - 1) u, in the form that does not cancel towards u = 1
    nh, sh = torch.sqrt(c2), torch.sqrt((1.0 - c2).clamp_min(0.0))
    Vx, Vz = torch.sqrt((1.0 - x * x).clamp_min(0.0)), x
    vh = Vz * nh + Vx * (sh * torch.cos(phi))
    nl = 2.0 * vh * nh - Vz
    open_ = (nl > 0) & (vh > 0)
    nls = torch.where(open_, nl, torch.zeros_like(nl))
    den = (nh * (nls + _lam(nls, al2))) * (Vz + _lam(Vz, al2))
    val = torch.where(open_, (2.0 * nls) * vh / den, torch.zeros_like(nls))
    vc = vh.clamp(max=1.0)
    f = (1.0 - vc) ** 5
    if scale:
        f = f + 5.0 * (1.0 - vc) ** 4 * vc.abs()
    wq = 2.0 * math.pi / (M_u * M_phi)
    return val.sum(dim=(1, 2)) * wq, (val * f).sum(dim=(1, 2)) * wq


def dfg_table_ref(R_v, R_r, r_min, M_u=128, M_phi=128, dtype=F64, scale=False):
    """the table [2, R_r, R_v] of reni_ggx_dfg by ``dfg_rule_at`` (scale: the scales of its entries); the grid values are formed
    in ``dtype`` as the kernel forms them in float32"""
    xi = torch.arange(R_v, dtype=dtype) / (R_v - 1)
    rj = torch.arange(R_r, dtype=dtype) * torch.tensor((1.0 - r_min) / (R_r - 1), dtype=dtype) + torch.tensor(r_min, dtype=dtype)
    rows = [torch.stack(dfg_rule_at(xi, rj[j].expand(R_v), M_u, M_phi, dtype, scale)) for j in range(R_r)]
    return torch.stack(rows, 1)  # [2, R_r, R_v]


_GL = None


def dfg_direct(x, r, n_gl=24, n_chi=1024):
    """(A0, A1) at one (x, r), float64, by DIRECT quadrature of DESIGN 4.4m's k and k f over the light direction L: polar
    coordinates (psi, chi) about the mirror direction R = 2 (N.V) N - V, where the lobe peaks; psi in Gauss-Legendre panels
    whose edges halve towards 0 (pi 2^-k), chi by the midpoint rule.  No change of variables to the half vector."""
    global _GL
    import numpy as np
    if _GL is None or _GL[0] != n_gl:
        _GL = (n_gl,) + tuple(torch.as_tensor(t) for t in np.polynomial.legendre.leggauss(n_gl))
    gx, gw = _GL[1], _GL[2]
    edges = [0.0] + [math.pi * 2.0 ** -k for k in range(20, -1, -1)]
    psi = torch.cat([0.5 * (b - a) * gx + 0.5 * (b + a) for a, b in zip(edges[:-1], edges[1:])])
    wpsi = torch.cat([0.5 * (b - a) * gw for a, b in zip(edges[:-1], edges[1:])])
    chi = 2.0 * math.pi * (torch.arange(n_chi, dtype=F64) + 0.5) / n_chi
    x = float(x)
    sx = math.sqrt(max(1.0 - x * x, 0.0))
    V = torch.tensor([sx, 0.0, x], dtype=F64)
    N = torch.tensor([0.0, 0.0, 1.0], dtype=F64)
    R = torch.tensor([-sx, 0.0, x], dtype=F64)
    e1 = torch.tensor([0.0, 1.0, 0.0], dtype=F64)
    e2 = torch.linalg.cross(R, e1)
    sp, cp = torch.sin(psi)[:, None, None], torch.cos(psi)[:, None, None]
    L = cp * R + sp * (torch.cos(chi)[None, :, None] * e1 + torch.sin(chi)[None, :, None] * e2)  # [psi, chi, 3]
    Hn = torch.nn.functional.normalize(V + L, dim=-1, eps=1e-6)
    a = float(r) ** 2
    a2 = a * a
    pos = lambda t: torch.where(t > 0, t, torch.zeros_like(t)).clamp(max=1.0)
    x_l, x_h = L @ N, Hn @ N
    nl, nh, nv = pos(x_l), pos(x_h), max(min(x, 1.0), 0.0)
    uu = (Hn @ V).clamp(0.0, 1.0)
    f = (1.0 - uu) ** 5
    s2 = (torch.linalg.cross(N.expand_as(Hn), Hn, dim=-1) ** 2).sum(-1)
    d = a2 * nh * nh + s2
    lam_l = torch.sqrt(a2 + (1.0 - a2) * nl * nl)
    lam_v = math.sqrt(a2 + (1.0 - a2) * nv * nv)
    k = torch.where(x_h > 0, a2 * nl / (torch.where(d > 0, d, torch.ones_like(d)) ** 2 * (nl + lam_l) * (nv + lam_v)), torch.zeros_like(nl))
    w = (wpsi * torch.sin(psi))[:, None] * (2.0 * math.pi / n_chi)
    return float((k * w).sum()), float((k * f * w).sum())


def dfg_lookup_ref(table, nv, roughness, roughness_min):
    """bilinear read of a table [2, R_r, R_v] (float64), differentiable in nv and roughness"""
    Rr, Rv = table.shape[1], table.shape[2]
    xx = nv.clamp(0.0, 1.0) * (Rv - 1)
    yy = (roughness.clamp(roughness_min, 1.0) - roughness_min) * ((Rr - 1) / (1.0 - roughness_min))
    i0 = torch.floor(xx.detach()).long().clamp(0, Rv - 2)
    j0 = torch.floor(yy.detach()).long().clamp(0, Rr - 2)
    fx, fy = xx - i0, yy - j0
    t = table
    A = (1 - fy) * ((1 - fx) * t[:, j0, i0] + fx * t[:, j0, i0 + 1]) + fy * ((1 - fx) * t[:, j0 + 1, i0] + fx * t[:, j0 + 1, i0 + 1])
    return A[0], A[1]


# ------------------------------------------------------------------------------------------------ shade_split_sum
def grid_dirs(W, dtype=F64):
    """RENI's own grid [W / 2 * W, 3] and its sine weight [W / 2 * W]: the float32 values the device holds
    (utils.get_directions / get_sineweight), in ``dtype``"""
    from reni_amd.utils import get_directions, get_sineweight
    return get_directions(W)[0].to(dtype), get_sineweight(W)[0, :, 0].to(dtype)


def lobe_ggx(t, alpha):
    tc, m = t.clamp(0.0, 1.0), ((1.0 + t) / 2.0).clamp(0.0, 1.0)
    a2 = alpha * alpha
    return tc * a2 / (m * (a2 - 1.0) + 1.0) ** 2


def roughness_level_ref(r, rho):
    K = len(rho)
    if K == 1:
        return torch.ones_like(r)
    knots = torch.tensor(rho, dtype=r.dtype)
    k = torch.bucketize(r.detach(), knots[1:-1].contiguous(), right=True)
    return (1.0 + k.to(r.dtype)) + (r - knots[k]) / (knots[k + 1] - knots[k])


def split_sum_chain_ref(C, W, Wo, rho):
    """[B, 1 + K, Wo / 2, Wo, 3] in C's dtype: level 0 the clamped-cosine sum of the premultiplied map C [B, Q, 3], the others
    the lobe-weighted mean radiance"""
    dirs, sinw = grid_dirs(W, C.dtype)
    odirs, _ = grid_dirs(Wo, C.dtype)
    t = odirs @ dirs.T  # [Po, Q]
    levels = [torch.einsum("oq,bqc->boc", t.clamp(0.0, 1.0), C)]
    for x in rho:
        f = lobe_ggx(t, x * x)
        den = f @ sinw
        levels.append(torch.einsum("oq,bqc->boc", f, C) / den[None, :, None])
    return torch.stack(levels, 1).view(C.shape[0], 1 + len(rho), Wo // 2, Wo, 3)


def shade_split_sum_ref(C, W, nrm, pos, cam, base_color, roughness, metallic, rho, Wo, roughness_min=0.1, f0=0.04, table=None,
                        dfg_size=32, terms=False, dtype=F64):
    """colours [B, NP, 3] in ``dtype`` (terms: (D, S0, S1) instead); C [B, Q, 3] the premultiplied map on the W grid; C, nrm,
    base_color, roughness and metallic may require grad.  table: the float64 DFG table (``dfg_table(dfg_size, roughness_min)``
    when None)."""
    C = C.to(dtype)
    chain = split_sum_chain_ref(C, W, Wo, rho)
    nd = nrm.to(dtype)
    n = torch.nn.functional.normalize(nd, p=2, dim=-1, eps=1e-6)
    v = torch.nn.functional.normalize(cam.to(dtype)[None] - pos.to(dtype), p=2, dim=-1, eps=1e-6)
    r = 2.0 * (n * v).sum(-1, keepdim=True) * n - v
    mask = (nrm != 0).any(-1, keepdim=True).to(dtype)
    nv = (n * v).sum(-1).clamp(0.0, 1.0)
    NP = n.shape[0]
    rc = torch.as_tensor(roughness).to(dtype).reshape(-1).expand(NP).clamp(max(roughness_min, rho[0]), rho[-1])
    D = lookup_ref(chain, n, 0.0, dtype)
    Pm = lookup_ref(chain, r, roughness_level_ref(rc, rho), dtype)
    if table is None:
        table = dfg_table(dfg_size, roughness_min)
    A0, A1 = dfg_lookup_ref(table.to(dtype), nv, rc, roughness_min)
    measure = C.shape[1] / (2.0 * math.pi ** 2)
    S0, S1 = Pm * (A0 * measure)[None, :, None], Pm * (A1 * measure)[None, :, None]
    if terms:
        return D * mask, S0 * mask, S1 * mask
    bc = torch.as_tensor(base_color).to(dtype)
    me = torch.as_tensor(metallic).to(dtype)
    me = me.reshape(-1, 1) if me.numel() > 1 else me.reshape(1, 1)
    F0 = f0 * (1 - me) + bc * me
    return ((1 - me) * bc * D + F0 * S0 + (1 - F0) * S1) * mask


@functools.lru_cache(maxsize=None)
def dfg_table(size, r_min, M=128, dtype=F64):
    return dfg_table_ref(size, size, r_min, M, M, dtype)


def sphere_gbuffer(S=8, radius=0.8, cam=(0.0, 0.0, 2.0)):
    """An S x S orthographic G-buffer of a sphere about the origin with background pixels (zero normal, zero position):
    (normals [S S, 3] un-normalised, positions [S S, 3], camera [3]), float32."""
    c = (torch.arange(S, dtype=torch.float32) + 0.5) / S * 2.0 - 1.0
    yy, xx = torch.meshgrid(-c, c, indexing="ij")
    r2 = xx * xx + yy * yy
    hit = r2 < radius * radius
    zz = torch.sqrt((radius * radius - r2).clamp_min(0.0))
    pos = torch.stack((xx, yy, zz), -1) * hit[..., None]
    nrm = pos * 1.7  # (not unit length: the shader normalises)
    return nrm.reshape(-1, 3), pos.reshape(-1, 3), torch.tensor(cam)


FIT = dict(S=16, W=32, Wo=32, rho=(0.2, 0.3, 0.45, 0.6, 0.8, 1.0), start=0.7, target=0.3, steps=15, lr=0.02, dfg_size=16,
           base_color=(0.8, 0.6, 0.4), metallic=0.6)


def fit_problem():
    """The roughness fit's scene: a 16 x 16 sphere G-buffer whose normals are bent by a fixed bump pattern (a tangent-space
    normal texture applied on the host), under a 16 x 32 map with a few lights on a dim ground.  -> (normals, positions, camera,
    C [1, Q, 3] premultiplied), float32"""
    p = FIT
    nrm, pos, cam = sphere_gbuffer(p["S"])
    g = torch.Generator().manual_seed(5)
    bump = (torch.rand(nrm.shape[0], 3, generator=g) * 2 - 1) * 0.25
    hit = (nrm != 0).any(-1, keepdim=True)
    nrm = (torch.nn.functional.normalize(nrm, dim=-1, eps=1e-6) + bump) * hit
    dirs, sinw = grid_dirs(p["W"], torch.float32)
    Q = dirs.shape[0]
    L = 0.2 + 0.3 * torch.rand(1, Q, 3, generator=g)
    for k in range(6):
        c = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0)
        L = L + (8.0 * torch.rand(3, generator=g))[None, None] * torch.exp(-(1 - dirs @ c) / 0.02)[None, :, None]
    return nrm, pos, cam, L * sinw[None, :, None]


def fit_reference(lr=None, steps=None):
    """the loss curve of the fit in the float64 reference"""
    p = FIT
    nrm, pos, cam, C = fit_problem()
    bc = torch.tensor(p["base_color"], dtype=F64)
    table = dfg_table(p["dfg_size"], 0.1)
    render = lambda r: shade_split_sum_ref(C, p["W"], nrm, pos, cam, bc, r, p["metallic"], p["rho"], p["Wo"], table=table)
    NP = nrm.shape[0]
    with torch.no_grad():
        target = render(torch.full((NP,), p["target"], dtype=F64))
    r = torch.full((NP,), p["start"], dtype=F64, requires_grad=True)
    opt = torch.optim.Adam([r], lr=p["lr"] if lr is None else lr)
    losses = []
    for _ in range(p["steps"] if steps is None else steps):
        opt.zero_grad()
        loss = ((render(r) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def smooth_map(W, B=1, seed=0):
    """A smooth positive radiance [B, Q, 3] on the W grid (low-order polynomials of the direction), float64, NOT premultiplied"""
    dirs, _ = grid_dirs(W)
    g = torch.Generator().manual_seed(seed)
    c1 = torch.randn(B, 3, 3, generator=g, dtype=F64) * 0.3
    c2 = torch.randn(B, 3, 3, generator=g, dtype=F64) * 0.2
    lin = torch.einsum("qk,bkc->bqc", dirs, c1)
    quad = torch.einsum("qk,bkc->bqc", dirs * dirs.roll(1, -1), c2)
    return (1.0 + lin + quad).clamp_min(0.05)
