"""Float64 torch restatement of the UV-texture definitions of include/reni_hip.h ("UV-space textures"): pixel
UV, footprint Jacobian, level of detail, the 8 taps, the box pyramid and the fetch.  It takes nothing from the library; its
autograd is the reference of every gradient.  Also here, because the CPU and the GPU tests share them: the fp32 numpy
emulation of the coordinate and lambda chain, the lookup cases of the GPU test, and the constants K, K' of the tolerance
(four times the worst ratio the emulation reaches over those cases)."""
import functools
import math

import numpy as np
import torch

F64 = torch.float64
EPS24 = 2.0 ** -24


# ---- geometry ---------------------------------------------------------------------------------------------------------
def pixel_uv_ref(verts, faces, verts_uvs, faces_uvs, R, T, tan_half_fov, S, pix_to_face, bary):
    """-> (uv [P,2], jac [P,4], valid [P] bool) in float64 from the (fp32) inputs."""
    P = S * S
    verts, vt, bary = verts.to(F64), verts_uvs.to(F64), bary.reshape(P, 3).to(F64)
    R, T = torch.as_tensor(R).reshape(3, 3).to(F64), torch.as_tensor(T).reshape(3).to(F64)
    f = pix_to_face.reshape(P).long()
    Fn, V, Tn = faces.shape[0], verts.shape[0], vt.shape[0]
    valid = (f >= 0) & (f < Fn)
    fs = f.clamp(0, Fn - 1)
    vi, ti = faces[fs].long(), faces_uvs[fs].long()
    valid &= ((vi >= 0) & (vi < V)).all(1) & ((ti >= 0) & (ti < Tn)).all(1)
    vi, ti = vi.clamp(0, V - 1), ti.clamp(0, Tn - 1)
    view = verts[vi] @ R + T                                       # [P,3,3]
    w = view[..., 2] * float(tan_half_fov)
    x, y = view[..., 0] / w, view[..., 1] / w                      # NDC
    t = vt[ti]                                                     # [P,3,2]
    uv = (bary[:, :, None] * t).sum(1)
    A = (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0]) - (y[:, 2] - y[:, 0]) * (x[:, 1] - x[:, 0]) + 1e-8
    dwdx = torch.stack([y[:, 2] - y[:, 1], y[:, 0] - y[:, 2], y[:, 1] - y[:, 0]], 1) / A[:, None]
    dwdy = torch.stack([x[:, 1] - x[:, 2], x[:, 2] - x[:, 0], x[:, 0] - x[:, 1]], 1) / A[:, None]
    step = -2.0 / S
    jac = torch.stack([(dwdx * t[..., 0]).sum(1), (dwdx * t[..., 1]).sum(1), (dwdy * t[..., 0]).sum(1), (dwdy * t[..., 1]).sum(1)], 1) * step
    valid &= torch.isfinite(uv).all(1)
    uv = torch.where(valid[:, None], uv, torch.zeros_like(uv))
    jac = torch.where(valid[:, None], jac, torch.zeros_like(jac))
    return uv, jac, valid


def jac_bound(verts, faces, verts_uvs, faces_uvs, R, T, tan_half_fov, S, pix_to_face):
    """[P] float64: a bound on the fp32 error of every component of jac, from the chain's roundings.  An NDC coordinate (a
    3-term dot, +T, x tan, /) carries at most 6 roundings: d = 6 eps max(|x|, |y|, 1).  An edge difference then errs by
    <= 3 d; a numerator N = sum_k e_k t_k by <= 3 d sum|t| + 3 eps sum|e_k t_k|; the area A (two products of differences)
    by <= 12 d e_max + 2 eps |A|; jac = N step / A by step / |A| (err N + |N| err A / |A|) + 3 eps |jac|.  Twice that is
    allowed (the order of the products inside the compiler's FMA contraction is not fixed by the source)."""
    eps = EPS24
    P = S * S
    vq, vt = verts.to(F64), verts_uvs.to(F64)
    R, T = torch.as_tensor(R).reshape(3, 3).to(F64), torch.as_tensor(T).reshape(3).to(F64)
    f = pix_to_face.reshape(P).long().clamp(0, faces.shape[0] - 1)
    vi = faces[f].long().clamp(0, vq.shape[0] - 1)
    ti = faces_uvs[f].long().clamp(0, vt.shape[0] - 1)
    view = vq[vi] @ R + T
    w = view[..., 2] * float(tan_half_fov)
    x, y = view[..., 0] / w, view[..., 1] / w
    t = vt[ti].abs()
    d = 6 * eps * torch.maximum(torch.maximum(x.abs().max(1).values, y.abs().max(1).values), torch.ones(P, dtype=F64))
    ex = torch.stack([y[:, 2] - y[:, 1], y[:, 0] - y[:, 2], y[:, 1] - y[:, 0]], 1).abs()
    ey = torch.stack([x[:, 1] - x[:, 2], x[:, 2] - x[:, 0], x[:, 0] - x[:, 1]], 1).abs()
    emax = torch.maximum(ex.max(1).values, ey.max(1).values)
    A = ((x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0]) - (y[:, 2] - y[:, 0]) * (x[:, 1] - x[:, 0]) + 1e-8).abs()
    errA = 12 * d * emax + 2 * eps * A
    step = 2.0 / S
    out = torch.zeros(P, dtype=F64)
    for e in (ex, ey):
        for c in (0, 1):
            N = (e * t[..., c]).sum(1)                      # >= |N|
            errN = 3 * d * t[..., c].sum(1) + 3 * eps * N
            out = torch.maximum(out, step / A * (errN + N * errA / A) + 3 * eps * N * step / A)
    return 2 * out


# ---- pyramid ----------------------------------------------------------------------------------------------------------
def level_sizes(H0, W0, L):
    return [(max(1, H0 >> l), max(1, W0 >> l)) for l in range(L)]


def full_levels(H0, W0):
    pow2 = H0 & (H0 - 1) == 0 and W0 & (W0 - 1) == 0
    return max(H0, W0).bit_length() if pow2 else 1


def level_offsets(H0, W0, L):
    off = [0]
    for h, w in level_sizes(H0, W0, L):
        off.append(off[-1] + h * w)
    return off


def pyramid_ref(tex, L):
    """tex [H0,W0,C] -> [E,C]: the levels back to back, box rule, summed ((a00 + a01) + (a10 + a11)) / 4."""
    H, W, C = tex.shape
    levels, cur = [tex.reshape(-1, C)], tex
    for _ in range(L - 1):
        h, w = cur.shape[:2]
        if h > 1 and w > 1:
            cur = ((cur[0::2, 0::2] + cur[0::2, 1::2]) + (cur[1::2, 0::2] + cur[1::2, 1::2])) * 0.25
        elif w > 1:
            cur = (cur[:, 0::2] + cur[:, 1::2]) * 0.5
        else:
            cur = (cur[0::2] + cur[1::2]) * 0.5
        levels.append(cur.reshape(-1, C))
    return torch.cat(levels, 0)


# ---- level of detail and taps -----------------------------------------------------------------------------------------
def lod_ref(jac, P, H0, W0, L, lod_bias):
    """lambda [P] float64; jac None: clamp(lod_bias, 0, L - 1) everywhere."""
    if jac is None:
        return torch.full((P,), min(max(float(lod_bias), 0.0), L - 1.0), dtype=F64)
    j = jac.to(F64)
    rho = torch.maximum(torch.hypot(j[:, 0] * W0, j[:, 1] * H0), torch.hypot(j[:, 2] * W0, j[:, 3] * H0))
    ok = torch.isfinite(j).all(1) & torch.isfinite(rho) & (rho > 0)
    lam = torch.log2(torch.where(ok, rho, torch.ones_like(rho))) + float(lod_bias)
    return torch.where(ok, lam.clamp(0.0, L - 1.0), torch.zeros_like(lam))


def _axis(t, n, n0, wrap, align, flip):
    if align:
        c = t.clamp(0.0, 1.0)
        x = ((1.0 - c) if flip else c) * (n0 - 1)
    elif wrap == "repeat":
        r = t - torch.floor(t)
        x = ((1.0 - r) if flip else r) * n - 0.5
    else:
        x = (((1.0 - t) if flip else t) * n - 0.5).clamp(0.0, n - 1.0)
    x0 = torch.floor(x)
    fr = x - x0
    k = x0.long()
    if wrap == "repeat" and not align:
        return k % n, (k + 1) % n, fr
    k = k.clamp(0, n - 1)
    return k, (k + 1).clamp(max=n - 1), fr


def taps_ref(uv, H0, W0, L, jac=None, valid=None, wrap="clamp", align_corners=False, lod_bias=0.0):
    """-> (index int64 [P,8], weight float64 [P,8]) by the header's definition."""
    uv = uv.to(F64)
    P = uv.shape[0]
    ok = torch.isfinite(uv).all(1)
    if valid is not None:
        ok &= valid.bool() if valid.dtype == torch.bool else valid >= 0
    u = torch.where(ok, uv[:, 0], torch.zeros(P, dtype=F64))
    v = torch.where(ok, uv[:, 1], torch.zeros(P, dtype=F64))
    lam = lod_ref(jac, P, H0, W0, L, lod_bias)
    l0 = torch.floor(lam).long().clamp(0, L - 1)
    fl = lam - l0
    fl = torch.where(l0 >= L - 1, torch.zeros_like(fl), fl)
    l1 = torch.where(fl > 0, l0 + 1, l0)
    off = torch.tensor(level_offsets(H0, W0, L))
    idx = torch.zeros(P, 8, dtype=torch.int64)
    wgt = torch.zeros(P, 8, dtype=F64)
    for s, (lv, lw) in enumerate(((l0, 1.0 - fl), (l1, fl))):
        for l in range(L):
            m = lv == l
            if not bool(m.any()):
                continue
            Hl, Wl = max(1, H0 >> l), max(1, W0 >> l)
            x0, x1, fx = _axis(u[m], Wl, W0, wrap, align_corners, False)
            y0, y1, fy = _axis(v[m], Hl, H0, wrap, align_corners, True)
            gx, gy = 1.0 - fx, 1.0 - fy
            base = int(off[l])
            idx[m, 4 * s:4 * s + 4] = torch.stack([base + y0 * Wl + x0, base + y0 * Wl + x1, base + y1 * Wl + x0, base + y1 * Wl + x1], 1)
            wgt[m, 4 * s:4 * s + 4] = torch.stack([gy * gx, gy * fx, fy * gx, fy * fx], 1) * lw[m][:, None]
    idx[~ok] = 0
    wgt[~ok] = 0.0
    return idx, wgt


def fetch_ref(pyr, idx, wgt):
    """out [P,C] = sum_k wgt[p,k] pyr[idx[p,k]]; a tap of weight 0 reads nothing (a NaN texel stays out)."""
    vals = pyr[idx]                                                # [P,8,C]
    vals = torch.where((wgt == 0)[:, :, None], torch.zeros_like(vals), vals)
    return (wgt[:, :, None] * vals).sum(1)


def sample_ref(tex, uv, L, **kw):
    """tex [H,W,C] (float64, may require grad) looked up at uv -> [P,C]."""
    H0, W0 = tex.shape[:2]
    idx, wgt = taps_ref(uv, H0, W0, L, **kw)
    return fetch_ref(pyramid_ref(tex, L), idx, wgt)


# ---- fp32 emulation of the coordinate and lambda chain (numpy, every operation rounded to fp32) -------------------------
def taps_emulated(uv, H0, W0, L, jac=None, valid=None, wrap="clamp", align_corners=False, lod_bias=0.0):
    """The same taps with every step in numpy float32 (products and sums rounded one by one: no FMA, numpy's log2)."""
    f = np.float32
    uv = np.asarray(uv, dtype=f)
    P = uv.shape[0]
    ok = np.isfinite(uv).all(1)
    if valid is not None:
        va = np.asarray(valid)
        ok &= va.astype(bool) if va.dtype == bool else va >= 0
    u, v = np.where(ok, uv[:, 0], f(0)), np.where(ok, uv[:, 1], f(0))
    if jac is None:
        lam = np.full(P, min(max(f(lod_bias), f(0)), f(L - 1)), dtype=f)
    else:
        j = np.asarray(jac, dtype=f)
        a0, a1, a2, a3 = j[:, 0] * f(W0), j[:, 1] * f(H0), j[:, 2] * f(W0), j[:, 3] * f(H0)
        with np.errstate(all="ignore"):
            rho = np.fmax(np.hypot(a0, a1), np.hypot(a2, a3)).astype(f)
            good = np.isfinite(j).all(1) & np.isfinite(a0) & np.isfinite(a1) & np.isfinite(a2) & np.isfinite(a3) & np.isfinite(rho) & (rho > 0)
            lam = np.log2(np.where(good, rho, f(1))).astype(f) + f(lod_bias)
        lam = np.where(good, np.clip(lam, f(0), f(L - 1)), f(0)).astype(f)
    l0 = np.clip(np.floor(lam).astype(np.int64), 0, L - 1)
    fl = (lam - l0.astype(f)).astype(f)
    fl = np.where(l0 >= L - 1, f(0), fl)
    l1 = np.where(fl > 0, l0 + 1, l0)
    off = level_offsets(H0, W0, L)

    def axis(t, n, n0, flip):
        if align_corners:
            c = np.clip(t, f(0), f(1))
            x = ((f(1) - c) if flip else c) * f(n0 - 1)
        elif wrap == "repeat":
            r = (t - np.floor(t)).astype(f)
            x = (((f(1) - r) if flip else r) * f(n)).astype(f) - f(0.5)
        else:
            x = np.clip((((f(1) - t) if flip else t) * f(n)).astype(f) - f(0.5), f(0), f(n - 1))
        x = x.astype(f)
        x0 = np.floor(x)
        fr = (x - x0).astype(f)
        k = x0.astype(np.int64)
        if wrap == "repeat" and not align_corners:
            return k % n, (k + 1) % n, fr
        k = np.clip(k, 0, n - 1)
        return k, np.minimum(k + 1, n - 1), fr

    idx = np.zeros((P, 8), dtype=np.int64)
    wgt = np.zeros((P, 8), dtype=f)
    for s, (lv, lw) in enumerate(((l0, (f(1) - fl).astype(f)), (l1, fl))):
        for l in range(L):
            m = lv == l
            if not m.any():
                continue
            Hl, Wl = max(1, H0 >> l), max(1, W0 >> l)
            x0, x1, fx = axis(u[m], Wl, W0, False)
            y0, y1, fy = axis(v[m], Hl, H0, True)
            gx, gy = (f(1) - fx).astype(f), (f(1) - fy).astype(f)
            idx[m, 4 * s:4 * s + 4] = np.stack([off[l] + y0 * Wl + x0, off[l] + y0 * Wl + x1, off[l] + y1 * Wl + x0, off[l] + y1 * Wl + x1], 1)
            w4 = np.stack([(gy * gx).astype(f), (gy * fx).astype(f), (fy * gx).astype(f), (fy * fx).astype(f)], 1)
            wgt[m, 4 * s:4 * s + 4] = (w4 * lw[m][:, None]).astype(f)
    idx[~ok] = 0
    wgt[~ok] = 0
    return idx, wgt


def pyramid_emulated(tex, L):
    """numpy float32, the kernel's summation order."""
    cur = np.asarray(tex, dtype=np.float32)
    C = cur.shape[2]
    out = [cur.reshape(-1, C)]
    for _ in range(L - 1):
        h, w = cur.shape[:2]
        if h > 1 and w > 1:
            cur = ((cur[0::2, 0::2] + cur[0::2, 1::2]) + (cur[1::2, 0::2] + cur[1::2, 1::2])) * np.float32(0.25)
        elif w > 1:
            cur = (cur[:, 0::2] + cur[:, 1::2]) * np.float32(0.5)
        else:
            cur = (cur[0::2] + cur[1::2]) * np.float32(0.5)
        out.append(cur.reshape(-1, C))
    return np.concatenate(out, 0)


def fetch_emulated(pyr, idx, wgt):
    acc = np.zeros((idx.shape[0], pyr.shape[1]), dtype=np.float32)
    for k in range(8):
        t = np.where((wgt[:, k] == 0)[:, None], np.float32(0), pyr[idx[:, k]])
        acc = (acc + (wgt[:, k][:, None] * t).astype(np.float32)).astype(np.float32)
    return acc


def fetch_backward_emulated(g, idx, wgt, E):
    """fp32 scatter in tap-table order (ascending position per texel), one rounding per product and per sum."""
    out = np.zeros((E, g.shape[1]), dtype=np.float32)
    flat, w = idx.reshape(-1), wgt.reshape(-1)
    order = np.argsort(flat, kind="stable")
    order = order[w[order] != 0]
    prod = (w[order][:, None] * g[order >> 3]).astype(np.float32)
    np.add.at(out, flat[order], prod)   # unbuffered: one fp32 addition per entry, in this order
    return out


# ---- the tolerance ----------------------------------------------------------------------------------------------------
def scale_factor(H0, W0, uv):
    """1 + max(H0, W0) max(1, |uv|max) over the finite uv: texels per unit of uv times the size of uv."""
    a = uv[torch.isfinite(uv)].abs()
    return 1.0 + max(H0, W0) * max(1.0, float(a.max()) if a.numel() else 1.0)


def fetch_bound(K, H0, W0, uv, tex):
    fin = tex[torch.isfinite(tex)]
    return K * EPS24 * scale_factor(H0, W0, uv) * float(fin.max() - fin.min())


def grad_bound(Kp, H0, W0, L, uv, idx_ref, g, wgt_ref=None):
    """[E] per texel: K' 2^-24 scale x the sum of |g| (max over channels) over the float64 reference's taps of that texel.
    The taps are the reference's eight per pixel (an unused one, of weight 0, is a tap too); an invalid pixel -- every
    reference weight 0 -- has none.  A texel that no reference tap names has bound 0: its gradient must be exactly 0."""
    E = level_offsets(H0, W0, L)[-1]
    gm = g.abs().to(F64).max(1).values
    gm = torch.where(torch.isfinite(gm), gm, torch.zeros_like(gm))
    if wgt_ref is not None:
        gm = torch.where((wgt_ref != 0).any(1), gm, torch.zeros_like(gm))
    S = torch.zeros(E, dtype=F64).index_add_(0, idx_ref.reshape(-1), gm.repeat_interleave(8))
    return Kp * EPS24 * scale_factor(H0, W0, uv) * S


# ---- the GPU test's lookup cases (shared with the CPU test, which derives K and K' from them) ---------------------------
SIZES = [  # (H0, W0, levels)
    (1, 1, 1), (1, 8, 1), (1, 8, 4), (8, 1, 1), (8, 1, 4), (2, 2, 1), (2, 2, 2), (3, 5, 1), (16, 4, 1), (16, 4, 3), (16, 4, 5),
    (64, 64, 7),
]
PIXELS = [1, 63, 64, 65, 257, 4097]
CHANNELS = [1, 3, 5, 8]


def make_case(H0, W0, L, P, C, wrap, align, seed, lod_bias=0.0, with_jac=True, far=False, special=True):
    """One lookup: fp32 tensors uv [P,2], jac [P,4] or None, valid [P] int64, tex [H0,W0,C], g [P,C]."""
    g = torch.Generator().manual_seed(seed)
    uv = torch.rand(P, 2, generator=g) * 1.6 - 0.3
    if far:
        uv = (torch.rand(P, 2, generator=g) * 2 - 1) * 1e3
    valid = torch.arange(P, dtype=torch.int64)
    if special and P >= 63:
        uv[0] = torch.tensor([0.0, 0.0]); uv[1] = torch.tensor([1.0, 1.0]); uv[2] = torch.tensor([0.0, 1.0]); uv[3] = torch.tensor([1.0, 0.0])
        uv[7, 0] = float("nan"); uv[9, 1] = float("inf"); uv[11] = torch.tensor([float("-inf"), float("nan")])
        valid[13] = -1; valid[14] = -1; valid[P - 1] = -1   # background / missing-UV pixels
    jac = None
    if with_jac:
        # footprints from 1/4 texel to 8 texels per pixel, random orientation; a few zero and non-finite ones
        k = torch.rand(P, generator=g) * 5 - 2
        th = torch.rand(P, generator=g) * 2 * math.pi
        r = torch.exp2(k)
        an = 0.3 + 0.7 * torch.rand(P, generator=g)
        jac = torch.stack([r * torch.cos(th) / W0, r * torch.sin(th) / H0, -an * r * torch.sin(th) / W0, an * r * torch.cos(th) / H0], 1)
        if special and P >= 63:
            jac[5] = 0.0
            jac[6, 2] = float("nan")
            jac[8, 0] = float("inf")
    tex = torch.rand(H0, W0, C, generator=g) * 2 - 0.5
    gout = torch.randn(P, C, generator=g)
    return {"H0": H0, "W0": W0, "L": L, "P": P, "C": C, "wrap": wrap, "align": align, "lod_bias": float(lod_bias),
            "uv": uv.float(), "jac": None if jac is None else jac.float(), "valid": valid, "tex": tex.float(), "g": gout.float()}


def lookup_cases():
    """The GPU test's list: every size with a sweep of P, C, wrap, alignment and lod_bias over it (not the full product)."""
    cases, seed = [], 100
    for si, (H0, W0, L) in enumerate(SIZES):
        for pi, P in enumerate(PIXELS):
            C = CHANNELS[(si + pi) % 4]
            wrap = "repeat" if (si + pi) % 2 else "clamp"
            seed += 1
            cases.append(make_case(H0, W0, L, P, C, wrap, False, seed, far=(wrap == "repeat" and pi % 3 == 1)))
        if L == 1:  # align_corners: one level, clamp
            for P in (65, 257):
                seed += 1
                cases.append(make_case(H0, W0, 1, P, CHANNELS[si % 4], "clamp", True, seed))
        else:  # lod_bias: lambda to exactly 0, exactly L - 1, an integer between (no footprint: the bias alone), and a fraction
            for bias, jacs in ((-100.0, True), (100.0, True), (float((L - 1) // 2), False), (0.5 * (L - 1), False), (-0.75, True)):
                seed += 1
                cases.append(make_case(H0, W0, L, 257, 3, "clamp" if seed % 2 else "repeat", False, seed, lod_bias=bias, with_jac=jacs))
    return cases


def case_reference(c):
    """float64: (out [P,C], gtex [H0,W0,C], idx, wgt) of a case."""
    tex = c["tex"].to(F64).requires_grad_(True)
    idx, wgt = taps_ref(c["uv"], c["H0"], c["W0"], c["L"], jac=c["jac"], valid=c["valid"], wrap=c["wrap"],
                        align_corners=c["align"], lod_bias=c["lod_bias"])
    pyr = pyramid_ref(tex, c["L"])
    out = fetch_ref(pyr, idx, wgt)
    (gt,) = torch.autograd.grad((out * c["g"].to(F64)).sum(), tex)
    return out.detach(), gt, idx, wgt


def level0_grad_bound(Kp, c, idx_ref, wgt_ref=None):
    """The per-texel bound carried to level 0 through the (exact in fp32 up to one rounding per level) box transpose: the
    bound of a level-0 texel is the sum over the levels of r^l times its ancestor's bound -- the transpose of the bounds."""
    H0, W0, L = c["H0"], c["W0"], c["L"]
    b = grad_bound(Kp, H0, W0, L, c["uv"], idx_ref, c["g"], wgt_ref)
    off, sizes = level_offsets(H0, W0, L), level_sizes(H0, W0, L)
    acc = b[off[L - 1]:off[L]].reshape(sizes[L - 1])
    for l in range(L - 2, -1, -1):
        h, w = sizes[l]
        r = 0.25 if h > 1 and w > 1 else 0.5
        up = acc
        if h > 1:
            up = up.repeat_interleave(2, 0)
        if w > 1:
            up = up.repeat_interleave(2, 1)
        acc = b[off[l]:off[l + 1]].reshape(h, w) + r * up
    return acc


@functools.lru_cache(maxsize=None)
def emulation_constants():
    """(K, K', worst fetch ratio, worst gradient ratio): the fp32 emulation against the float64 restatement over
    lookup_cases(), in units of the bounds with K = K' = 1; K and K' are four times the worst ratios (the margin is for FMA
    contraction and the device's log2)."""
    worst_f, worst_g = 0.0, 0.0
    for c in lookup_cases():
        out, gt, idx, rw = case_reference(c)
        ei, ew = taps_emulated(c["uv"].numpy(), c["H0"], c["W0"], c["L"], jac=None if c["jac"] is None else c["jac"].numpy(),
                               valid=c["valid"].numpy(), wrap=c["wrap"], align_corners=c["align"], lod_bias=c["lod_bias"])
        pyr = pyramid_emulated(c["tex"].numpy(), c["L"])
        eo = fetch_emulated(pyr, ei, ew)
        unit = fetch_bound(1.0, c["H0"], c["W0"], c["uv"], c["tex"])
        if unit > 0:
            worst_f = max(worst_f, float(np.abs(eo.astype(np.float64) - out.numpy()).max()) / unit)
        E = level_offsets(c["H0"], c["W0"], c["L"])[-1]
        eg = torch.from_numpy(fetch_backward_emulated(c["g"].numpy(), ei, ew, E))
        # the emulated level gradients folded as the device folds them: fp32, g_l += r g_{l+1} from the coarsest level down
        off, sizes = level_offsets(c["H0"], c["W0"], c["L"]), level_sizes(c["H0"], c["W0"], c["L"])
        acc = eg[off[-2]:off[-1]].reshape(*sizes[-1], -1)
        for l in range(c["L"] - 2, -1, -1):
            h, w = sizes[l]
            r = 0.25 if h > 1 and w > 1 else 0.5
            up = acc
            if h > 1:
                up = up.repeat_interleave(2, 0)
            if w > 1:
                up = up.repeat_interleave(2, 1)
            acc = eg[off[l]:off[l + 1]].reshape(h, w, -1) + r * up
        assert acc.dtype == torch.float32
        acc = acc.to(F64)
        unit_g = level0_grad_bound(1.0, c, idx, rw)
        err = (acc - gt).abs().max(2).values
        m = unit_g > 0
        assert bool((err[~m] == 0).all()), "a texel outside every footprint received a gradient in the emulation"
        if bool(m.any()):
            worst_g = max(worst_g, float((err[m] / unit_g[m]).max()))
    return 4.0 * worst_f, 4.0 * worst_g, worst_f, worst_g
