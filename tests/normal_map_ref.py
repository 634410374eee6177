"""References of the normal-mapped materials (reni_envmap_shade_terms_dnormals, textures.tangent_frames / perturb_normals).

1. ``dnormals_ref``: the definition in float64, written out (no autograd), with the strict gates:

       a(b,p,j)  = sum_c gD[b,p,c] C[b,j,c]            b'(b,p,j) = sum_c gS[b,p,c] C[b,j,c]
       gN[p]     = sum_b sum_j v ( [x_l > 0] a L + [x_h > 0] s_p nh^(s_p - 1) b' H )
       d_normals = (gN - N (N.gN)) / |n_p|  for |n_p| >= 1e-6,  gN / 1e-6 below it

   x_l = N.L and x_h = N.H are taken before their clamps, the clamp at 1 is ignored.  A zero normal has x_l = x_h = 0 and
   gets exactly 0 (torch autograd gives L a / 1e-6 there: clamp's backward passes the boundary).
2. ``dnormals_bound``: the per-pixel scale an fp32 evaluation is held against (see its docstring).
3. ``dnormals_emulated``: the kernel's chain in numpy fp32, in the kernel's order.
4. ``tangent_frames_ref`` / ``perturb_normals_ref``: the tangent frames and the perturbation in float64.
"""
import functools

import numpy as np
import torch

F64 = torch.float64
EPS24 = 2.0 ** -24
SH_TILE, SHADE_BC = 128, 4

# (B, NP, J, per-image directions): the terms path's seven shapes (tests/test_gpu_shade_materials.py)
SHAPES = [(1, 300, 200, False), (3, 1000, 515, False), (5, 257, 1030, False), (9, 64, 129, False), (2, 130, 512, False),
          (2, 500, 300, True), (3, 1, 1, False)]
SHININESS = ["s500", "s20", "per_pixel", "s1"]
MASKS = ["none", "random"]


def problem(B, NP, J, seed, frac_bg=0.2, per_image_dirs=False):
    """tests/test_gpu_shade_materials.py's generator."""
    g = torch.Generator().manual_seed(seed)
    nrm = torch.randn(NP, 3, generator=g) * 0.7
    pos = torch.randn(NP, 3, generator=g) * 0.4
    bg = torch.rand(NP, generator=g) < frac_bg
    nrm[bg] = 0.0
    pos[bg] = 0.0
    cam = torch.tensor([0.0, 0.0, 2.0])
    shape = (B, J, 3) if per_image_dirs else (1, J, 3)
    L = torch.nn.functional.normalize(torch.randn(shape, generator=g), dim=-1)
    C = torch.exp(torch.randn(B, J, 3, generator=g)) * torch.rand(1, J, 1, generator=g)
    return nrm, pos, cam, L, C


@functools.lru_cache(maxsize=None)
def case(B, NP, J, per_image, kind):
    """One test case (CPU tensors): the generator's problem, a shininess of ``kind``, upstream gradients and a 60 % mask."""
    nrm, pos, cam, L, C = problem(B, NP, J, seed=100 + B + NP, per_image_dirs=per_image)
    if NP == 1 and J == 1:
        # the stock seed gives this lone pixel a gradient of 0 (it faces away): turn its normal towards its texel
        nrm[0] = 0.7 * torch.nn.functional.normalize(L[0, 0] + torch.tensor([0.3, -0.2, 0.1]), dim=0)
        pos[0] = torch.tensor([0.1, -0.2, 0.05])
    g = torch.Generator().manual_seed(7 * NP + J)
    shin = {"s500": torch.tensor(500.0), "s20": torch.tensor(20.0), "s1": torch.tensor(1.0)}.get(kind)
    if shin is None:
        shin = torch.rand(NP, generator=g) * 495.0 + 5.0
    gD, gS = (torch.randn(B, NP, 3, generator=g) for _ in range(2))
    vis = torch.rand(L.shape[0], NP, J, generator=g) < 0.6
    if NP == 1 and J == 1:
        vis[:] = True  # (its one bit unset would leave nothing to check again)
    return dict(B=B, NP=NP, J=J, per_image=per_image, kind=kind, nrm=nrm, pos=pos, cam=cam, L=L, C=C, shin=shin, gD=gD, gS=gS,
                vis=vis, bg=(nrm == 0).all(-1))


def all_cases():
    return [s + (k,) for s in SHAPES for k in SHININESS]


# ------------------------------------------------------------------------------------------------ float64 definition
def _pairs(nrm, pos, cam, L):
    """N [NP,3], |n| [NP], x_l, x_h [NB,NP,J] (before the clamps), H [NB,NP,J,3] in float64."""
    n = nrm.to(F64)
    ln = n.norm(dim=-1)
    N = n / ln.clamp_min(1e-6)[:, None]
    v = cam.to(F64)[None] - pos.to(F64)
    V = v / v.norm(dim=-1).clamp_min(1e-6)[:, None]
    Ld = L.to(F64)
    h = V[None, :, None, :] + Ld[:, None, :, :]
    H = h / h.norm(dim=-1, keepdim=True).clamp_min(1e-6)
    x_l = torch.einsum("pk,bjk->bpj", N, Ld)
    x_h = torch.einsum("pk,bpjk->bpj", N, H)
    return N, ln, x_l, x_h, H


def _weights(nrm, pos, cam, L, C, gD, gS, shin, vis):
    N, ln, x_l, x_h, H = _pairs(nrm, pos, cam, L)
    B = C.shape[0]
    a = torch.einsum("bpc,bjc->bpj", gD.to(F64), C.to(F64))
    bp = torch.einsum("bpc,bjc->bpj", gS.to(F64), C.to(F64))
    s = torch.as_tensor(shin, dtype=F64)
    s = s.reshape(1, -1, 1) if s.numel() > 1 else s.reshape(1, 1, 1)
    gate_l, gate_h = (x_l > 0).expand(B, -1, -1), (x_h > 0).expand(B, -1, -1)
    nh = x_h.clamp(0.0, 1.0)
    dpow = torch.where(x_h > 0, s * nh.clamp_min(1e-300) ** (s - 1.0), torch.zeros_like(nh)).expand(B, -1, -1)
    v = torch.ones_like(a) if vis is None else vis.to(F64).expand(B, -1, -1)
    return N, ln, x_l, x_h, H, a, bp, s, v, gate_l, gate_h, dpow


def dnormals_ref(nrm, pos, cam, L, C, gD, gS, shin, vis=None):
    """d_normals [NP,3] in float64.  L [1 | B, J, 3], C [B,J,3], gD, gS [B,NP,3], shin a float, a 0-d tensor or [NP], vis
    None or booleans [1 | B, NP, J]."""
    N, ln, x_l, x_h, H, a, bp, s, v, gate_l, gate_h, dpow = _weights(nrm, pos, cam, L, C, gD, gS, shin, vis)
    B = C.shape[0]
    wl = v * gate_l.to(F64) * a
    wh = v * dpow * bp
    gN = torch.einsum("bpj,bjk->pk", wl, L.to(F64).expand(B, -1, -1)) + torch.einsum("bpj,bpjk->pk", wh, H.expand(B, -1, -1, -1))
    proj = (gN - N * (N * gN).sum(-1, keepdim=True)) / ln.clamp_min(1e-6)[:, None]
    return torch.where((ln >= 1e-6)[:, None], proj, gN / 1e-6)


def dnormals_bound(nrm, pos, cam, L, C, gD, gS, shin, vis=None):
    """(unit [NP], jump [NP]): an fp32 evaluation's error per pixel is held against K unit + jump, with

        unit = 2^-24 ( sum_{b,j} v [x_l > 0] |a|  +  sum_{b,j} v (1 + s_p) s_p nh^(s_p - 1) |b'| ) / max(|n_p|, 1e-6)

    (every pair's term at its own size, the specular ones with the factor 1 + s_p by which pow amplifies the rounding of
    nh), and jump, for shininess 1 only, = the size of the steps a gate that flips under fp32 rounding can add: |b'| of
    every pair with |x_h| < 1e-6 (s = 1 is the only shininess at which s nh^(s-1) does not vanish at nh = 0) and |a| of every
    pair with |x_l| < 1e-6; both over max(|n_p|, 1e-6).  (The diffuse gate is a step at every shininess; no allowance is made
    for it elsewhere, and none of the GPU test's cases needs one.)"""
    N, ln, x_l, x_h, H, a, bp, s, v, gate_l, gate_h, dpow = _weights(nrm, pos, cam, L, C, gD, gS, shin, vis)
    B = C.shape[0]
    den = ln.clamp_min(1e-6)
    unit = EPS24 * ((v * gate_l.to(F64) * a.abs()).sum(dim=(0, 2)) + (v * (1.0 + s) * dpow * bp.abs()).sum(dim=(0, 2))) / den
    near_l = ((x_l.abs() < 1e-6) & (s == 1.0)).expand(B, -1, -1).to(F64)
    near_h = ((x_h.abs() < 1e-6) & (s == 1.0)).expand(B, -1, -1).to(F64)
    # (a zero normal has x = 0 exactly on both sides: its gates cannot flip, and its gradient must be exactly 0)
    live = (ln > 0).to(F64)
    jump = live * ((v * near_l * a.abs()).sum(dim=(0, 2)) + (v * near_h * bp.abs()).sum(dim=(0, 2))) / den
    return unit, jump


# ------------------------------------------------------------------------------------------------ fp32 emulation
def n_splits(n_own, n_oth):
    wg_x = (n_own + 255) // 256
    s = (2048 + wg_x - 1) // wg_x
    s = min(s, (n_oth + SH_TILE - 1) // SH_TILE, 64)
    return max(s, 1)


def _fma(a, b, c):
    """fmaf: one rounding (the product of two floats is exact in float64; the sum is rounded there and again to float32,
    which differs from a single rounding only on a near-tie)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _normalize3(v):
    f = np.float32
    n = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(f)).astype(f)
    inv = (f(1.0) / np.maximum(n, f(1e-6))).astype(f)
    return (v * inv[:, None]).astype(f)


def dnormals_emulated(nrm, pos, cam, L, C, gD, gS, shin, vis=None):
    """The kernel's chain in numpy float32, in its order: a thread per pixel; per pair shade_pair's fmaf chains, a and b' as
    fmaf chains over the chunk's images and channels, the two accumulator fmafs per component; texels ascending within a
    split, one partial sum per (chunk, split); the reduce adds splits ascending into a chunk sum, the chunk sums ascending,
    and projects last.  rsq, log2 and exp2 are numpy's, correctly rounded to float32 (the device's are approximations)."""
    f = np.float32
    nrm, pos, cam, L, C, gD, gS = (np.ascontiguousarray(t.numpy(), dtype=f) for t in (nrm, pos, cam, L, C, gD, gS))
    B, J = C.shape[0], C.shape[1]
    NP = nrm.shape[0]
    s = np.broadcast_to(np.asarray(torch.as_tensor(shin).numpy(), dtype=f).reshape(-1), (NP,))
    sm1 = (s - f(1.0)).astype(f)
    N = _normalize3(nrm)
    V = _normalize3((cam[None, :] - pos).astype(f))
    per_image = L.shape[0] > 1
    step = 1 if per_image else SHADE_BC
    S = n_splits(NP, J)
    per_split = ((((J + SH_TILE - 1) // SH_TILE) + S - 1) // S) * SH_TILE
    total = np.zeros((NP, 3), f)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b0 in range(0, B, step):
            nb = min(step, B - b0)
            Lc = L[b0 if per_image else 0]                                   # [J, 3]
            vc = None if vis is None else vis[b0 if per_image else 0].numpy()  # [NP, J]
            # everything of a pair but the accumulation is independent of the walk: whole [NP, J] arrays
            nl = np.clip(_fma(N[:, None, 2], Lc[None, :, 2], _fma(N[:, None, 1], Lc[None, :, 1], (N[:, None, 0] * Lc[None, :, 0]).astype(f))), f(0), f(1))
            h = (V[:, None, :] + Lc[None, :, :]).astype(f)
            q = np.maximum(_fma(h[..., 2], h[..., 2], _fma(h[..., 1], h[..., 1], (h[..., 0] * h[..., 0]).astype(f))), f(1e-12))
            inv = (1.0 / np.sqrt(q.astype(np.float64))).astype(f)
            H = (h * inv[..., None]).astype(f)
            nh = np.clip(_fma(N[:, None, 2], H[..., 2], _fma(N[:, None, 1], H[..., 1], (N[:, None, 0] * H[..., 0]).astype(f))), f(0), f(1))
            lg = np.log2(nh.astype(np.float64)).astype(f)
            w = (s[:, None] * np.exp2((sm1[:, None] * lg).astype(f).astype(np.float64)).astype(f)).astype(f)
            ad = np.zeros((NP, J), f)
            as_ = np.zeros((NP, J), f)
            for b in range(nb):
                for c in range(3):
                    ad = _fma(gD[b0 + b, :, None, c], C[b0 + b, None, :, c], ad)
                    as_ = _fma(gS[b0 + b, :, None, c], C[b0 + b, None, :, c], as_)
            cl = np.where(nl > 0, ad, f(0)).astype(f)
            ch = np.where(nh > 0, (w * as_).astype(f), f(0)).astype(f)
            if vc is not None:
                cl, ch = np.where(vc, cl, f(0)).astype(f), np.where(vc, ch, f(0)).astype(f)
            chunk = np.zeros((NP, 3), f)
            for q0 in range(S):
                acc = np.zeros((NP, 3), f)
                for j in range(q0 * per_split, min(J, (q0 + 1) * per_split)):
                    acc = _fma(ch[:, j, None], H[:, j, :], _fma(cl[:, j, None], Lc[None, j, :], acc))
                chunk = (chunk + acc).astype(f)
            total = (total + chunk).astype(f)
        ln = np.sqrt(_fma(nrm[:, 2], nrm[:, 2], _fma(nrm[:, 1], nrm[:, 1], (nrm[:, 0] * nrm[:, 0]).astype(f)))).astype(f)
        inv = (f(1.0) / np.maximum(ln, f(1e-6))).astype(f)
        Nn = (nrm * inv[:, None]).astype(f)
        d = _fma(Nn[:, 2], total[:, 2], _fma(Nn[:, 1], total[:, 1], (Nn[:, 0] * total[:, 0]).astype(f)))
        proj = (_fma(-Nn, d[:, None], total) * inv[:, None]).astype(f)
        out = np.where((ln >= f(1e-6))[:, None], proj, (total * inv[:, None]).astype(f))
    return out.astype(f)


def error_ratio(got, c, mask):
    """(worst ratio of |got - reference| - jump to the bound's unit over the pixels of one case, float64 reference).  A pixel
    whose unit is 0 (background, or nothing lit) must be exactly 0 and counts as ratio 0 when it is, inf when it is not."""
    ref = reference(c["B"], c["NP"], c["J"], c["per_image"], c["kind"], mask)
    err = (torch.as_tensor(got).double() - ref["d"]).abs().max(dim=1).values
    over = (err - ref["jump"]).clamp_min(0.0)
    ratio = torch.where(ref["unit"] > 0, over / ref["unit"].clamp_min(1e-300), torch.where(over > 0, torch.full_like(over, float("inf")), over))
    return float(ratio.max()), ref


@functools.lru_cache(maxsize=None)
def reference(B, NP, J, per_image, kind, mask):
    c = case(B, NP, J, per_image, kind)
    vis = c["vis"] if mask == "random" else None
    args = (c["nrm"], c["pos"], c["cam"], c["L"], c["C"], c["gD"], c["gS"], c["shin"])
    unit, jump = dnormals_bound(*args, vis=vis)
    return dict(d=dnormals_ref(*args, vis=vis), unit=unit, jump=jump)


@functools.lru_cache(maxsize=None)
def emulation_constant():
    """(K, worst ratio): the fp32 emulation against the float64 definition over every case of the GPU test, in units of
    ``dnormals_bound`` with K = 1; K is four times the worst ratio (the margin is for the device's rsq, log and exp2 and for
    the products of normalize3, which the compiler is free to fuse)."""
    worst = 0.0
    for (B, NP, J, per_image, kind) in all_cases():
        c = case(B, NP, J, per_image, kind)
        for mask in MASKS:
            vis = c["vis"] if mask == "random" else None
            emu = dnormals_emulated(c["nrm"], c["pos"], c["cam"], c["L"], c["C"], c["gD"], c["gS"], c["shin"], vis=vis)
            r, _ = error_ratio(torch.from_numpy(emu), c, mask)
            worst = max(worst, r)
    return 4.0 * worst, worst


# ------------------------------------------------------------------------------------------------ tangent frames
def tangent_frames_ref(verts, faces, verts_uvs, faces_uvs, pix_valid, pixel_normals):
    """(tangent, bitangent [P,3] float64, valid [P] bool), pixel by pixel as the issue states it."""
    P = pix_valid.shape[0]
    t_out, b_out = torch.zeros(P, 3, dtype=F64), torch.zeros(P, 3, dtype=F64)
    ok = torch.zeros(P, dtype=torch.bool)
    v, vt, n = verts.to(F64), verts_uvs.to(F64), pixel_normals.to(F64)
    for p in range(P):
        fidx = int(pix_valid[p])
        if fidx < 0:
            continue
        p0, p1, p2 = (v[int(faces[fidx, k])] for k in range(3))
        (u0, v0), (u1, v1), (u2, v2) = (vt[int(faces_uvs[fidx, k])] for k in range(3))
        e1, e2 = p1 - p0, p2 - p0
        du1, dv1, du2, dv2 = u1 - u0, v1 - v0, u2 - u0, v2 - v0
        det = du1 * dv2 - du2 * dv1
        if not bool(torch.isfinite(det)) or float(det) == 0.0:
            continue
        Tf, Bf = (e1 * dv2 - e2 * dv1) / det, (e2 * du1 - e1 * du2) / det
        N = n[p] / n[p].norm().clamp_min(1e-6)
        tp = Tf - N * (N @ Tf)
        if float(tp.norm()) < 1e-12:
            continue
        t = tp / tp.norm()
        c = torch.linalg.cross(N, t)
        h = float(torch.sign(c @ Bf))
        if h == 0.0:
            continue
        t_out[p], b_out[p], ok[p] = t, h * c, True
    return t_out, b_out, ok


def perturb_normals_ref(pixel_normals, tangent, bitangent, valid, m, strength=1.0):
    """The direction strength m_x t + strength m_y b + m_z N at the length of the pixel's own normal (float64, autograd
    through m); invalid pixels keep their normal."""
    n = pixel_normals.to(F64)
    ln = n.norm(dim=-1, keepdim=True).clamp_min(1e-6)
    N = n / ln
    bent = ln * (strength * m[:, 0:1] * tangent.to(F64) + strength * m[:, 1:2] * bitangent.to(F64) + m[:, 2:3] * N)
    return torch.where(valid[:, None], bent, n)
