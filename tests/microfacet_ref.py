"""float64 reference of the microfacet (GGX) materials (reni_envmap_shade_ggx[_backward|_dpixel], envmap_shader.shade_terms_ggx /
compose_microfacet), in plain torch.  Its autograd is the reference for every gradient of the feature.

For pixel p with given normal n_p: N = n_p / max(|n_p|, 1e-6), V = normalize(cam - pos_p), a = alpha_p > 0; for texel j with
direction L, colour C[b,j,:] and visibility bit v(p,j):

    H   = (V + L) / max(|V + L|, 1e-6)
    x_l = N.L,  x_h = N.H,  x_v = N.V            nl, nh, nv = clamp(x, 0, 1)
    u   = clamp(V.H, 0, 1)                        f = (1 - u)^5
    s2  = |N x H|^2
    d   = a^2 nh^2 + s2
    lam(x) = sqrt(a^2 + (1 - a^2) x^2)
    k   = [x_h > 0] a^2 nl / ( d^2 (nl + lam(nl)) (nv + lam(nv)) )

    D [b,p,c] = sum_j v nl C[b,j,c]        S0[b,p,c] = sum_j v k C[b,j,c]        S1[b,p,c] = sum_j v k f C[b,j,c]
    colours   = (1 - metallic) base_color D + F0 S0 + (1 - F0) S1,   F0 = f0_dielectric (1 - metallic) + base_color metallic

The gates are strict, in the values and in autograd: a clamp is written where(x > 0, x, 0) (the derivative at x = 0 is 0, where
torch.clamp's backward passes the boundary) and the clamp at 1 is min(x, 1); the denominator of a closed gate is replaced by 1
before the division, so no 0 * inf reaches a gradient.  A zero normal then has exact zeros in every sum and every gradient.

Besides the definition: ``grad_scales`` (the per-pixel sums of the absolute values of the parts of d alpha and d normals, the
scale an fp32 evaluation of those cancelling sums is held against) and ``gate_allowance`` (what the pairs within 1e-6 of a gate
can add when fp32 rounding opens or closes it).
"""
import functools
import types

import torch

F64 = torch.float64
GATE_EPS = 1e-6

# (B, NP, J, per-image directions): the terms path's seven shapes (tests/test_gpu_shade_materials.py)
SHAPES = [(1, 300, 200, False), (3, 1000, 515, False), (5, 257, 1030, False), (9, 64, 129, False), (2, 130, 512, False),
          (2, 500, 300, True), (3, 1, 1, False)]
ROUGHNESS = ["r02", "r07", "per_pixel"]
MASKS = ["none", "random"]
QUANTITIES = ("D", "S0", "S1", "dC", "dalpha", "dn", "colours", "dC_col", "d_base_color", "d_roughness", "d_metallic")
FLOOR = 2e-5  # of the largest reference value: the scalar shader's tolerance


def _pos(x):
    """clamp(x, 0, 1) with strict gates (see the module docstring)."""
    return torch.where(x > 0, x, torch.zeros_like(x)).clamp(max=1.0)


def pairs(nrm, pos, cam, L, alpha, dtype=F64):
    """Everything of the (p, j) pairs, [NB, NP, J] each (NB = 1: a shared grid), differentiable in nrm and alpha.  L [NB,J,3],
    alpha a 0-d tensor or [NP]."""
    n = nrm.to(dtype)
    N = torch.nn.functional.normalize(n, p=2, dim=-1, eps=1e-6)
    V = torch.nn.functional.normalize(cam.to(dtype)[None] - pos.to(dtype), p=2, dim=-1, eps=1e-6)
    Ld = L.to(dtype)
    H = torch.nn.functional.normalize(V[None, :, None, :] + Ld[:, None, :, :], p=2, dim=-1, eps=1e-6)
    a = torch.as_tensor(alpha, dtype=dtype)
    a = a.reshape(1, -1, 1) if a.numel() > 1 else a.reshape(1, 1, 1)
    x_l = torch.einsum("pk,bjk->bpj", N, Ld)
    x_h = torch.einsum("pk,bpjk->bpj", N, H)
    x_v = (N * V).sum(-1)[None, :, None]
    nl, nh, nv = _pos(x_l), _pos(x_h), _pos(x_v)
    u = torch.einsum("pk,bpjk->bpj", V, H).clamp(0.0, 1.0)
    f = (1.0 - u) ** 5
    s2 = (torch.linalg.cross(N[None, :, None, :].expand_as(H), H, dim=-1) ** 2).sum(-1)
    a2 = a * a
    d = a2 * nh * nh + s2
    lam_l = torch.sqrt(a2 + (1.0 - a2) * nl * nl)
    lam_v = torch.sqrt(a2 + (1.0 - a2) * nv * nv)
    gate = x_h > 0
    # k / nl with the gate open (d of a zero normal is 0: replaced by 1, the value is then unused or an allowance's)
    kk_open = a2 / (torch.where(d > 0, d, torch.ones_like(d)) ** 2 * (nl + lam_l) * (nv + lam_v))
    k = torch.where(gate, kk_open * nl, torch.zeros_like(kk_open))
    return types.SimpleNamespace(N=N, V=V, H=H, len=n.norm(dim=-1), a=a, x_l=x_l, x_h=x_h, x_v=x_v, nl=nl, nh=nh, nv=nv, f=f,
                                 d=d, lam_l=lam_l, lam_v=lam_v, gate=gate, kk_open=kk_open, k=k)


def shade_terms_ggx_ref(nrm, pos, cam, L, C, alpha, vis=None, dtype=F64):
    """-> (D, S0, S1), each [B, NP, 3].  L [1 | B, J, 3], C [B, J, 3], alpha a float, a 0-d tensor or [NP], nrm [NP, 3] (nrm and
    alpha may require grad), vis None or booleans [1 | B, NP, J]."""
    q = pairs(nrm, pos, cam, L, alpha, dtype)
    m = [q.nl, q.k, q.k * q.f]
    if vis is not None:
        m = [x * vis.to(dtype) for x in m]
    Cd = C.to(dtype)
    B = Cd.shape[0]
    return tuple(torch.einsum("bjk,bpj->bpk", Cd, x.expand(B, -1, -1)) for x in m)


def compose_microfacet_ref(D, S0, S1, base_color, metallic, f0_dielectric=0.04):
    dt = D.dtype
    c = torch.as_tensor(base_color, dtype=dt)
    m = torch.as_tensor(metallic, dtype=dt)
    m = m.reshape(-1, 1) if m.numel() > 1 else m.reshape(1, 1)
    F0 = f0_dielectric * (1 - m) + c * m
    return (1 - m) * c * D + F0 * S0 + (1 - F0) * S1


def _abs_weights(q, C, gD, gS0, gS1, dtype):
    """A0 = sum_c |gD| C and A = sum_c (|gS0| + f |gS1|) C, [B, NP, J]: the upstream weights with every part at its own size."""
    Cd = C.to(dtype).abs()
    A0 = torch.einsum("bpc,bjc->bpj", gD.to(dtype).abs(), Cd)
    A = torch.einsum("bpc,bjc->bpj", gS0.to(dtype).abs(), Cd) + q.f * torch.einsum("bpc,bjc->bpj", gS1.to(dtype).abs(), Cd)
    return A0, A


def _parts(q, A0, A, v, open_gates):
    """(sum over b, j of the absolute values of the parts of d alpha [NP], of d normals [NP]) over the pairs weighted by v.
    d ln k / d alpha has four parts, 2 / a and three negative ones; d k / d N has the diffuse part, the two nl parts, the H part
    and the V part.  open_gates: as if every gate were open (for the allowance of pairs near a gate)."""
    a, a2 = q.a, q.a * q.a
    B = A.shape[0]
    kk = q.kk_open if open_gates else torch.where(q.gate, q.kk_open, torch.zeros_like(q.kk_open))
    nl = q.x_l.abs().clamp(max=1.0) if open_gates else q.nl
    k = kk * nl
    safe_d = torch.where(q.d > 0, q.d, torch.ones_like(q.d))
    dlna = 2.0 / a + 4.0 * a * q.nh ** 2 / safe_d + a * (1 - q.nl ** 2) / (q.lam_l * (q.nl + q.lam_l)) \
        + a * (1 - q.nv ** 2) / (q.lam_v * (q.nv + q.lam_v))
    pa = (v * k * A * dlna).expand(B, -1, -1).sum(dim=(0, 2))
    gl = torch.ones_like(q.x_l) if open_gates else (q.x_l > 0).to(A.dtype)
    gvv = torch.ones_like(q.x_v) if open_gates else (q.x_v > 0).to(A.dtype)
    dl = (1 + (1 - a2) * q.nl / q.lam_l) / (q.nl + q.lam_l)
    dv = (1 + (1 - a2) * q.nv / q.lam_v) / (q.nv + q.lam_v)
    pn = v * (gl * (A0 + kk * A + k * A * dl) + k * A * 4 * (1 - a2).abs() * q.nh / safe_d + gvv * k * A * dv)
    pn = pn.expand(B, -1, -1).sum(dim=(0, 2)) / q.len.clamp_min(1e-6)
    return pa, pn


def _near(q):
    """pairs within GATE_EPS of a gate (x_l, x_h, or the pixel's x_v), of pixels with a normal (a zero normal sits exactly on
    every gate on both sides: its gates cannot flip, and its results must be exactly 0)."""
    near = (q.x_l.abs() < GATE_EPS) | (q.x_h.abs() < GATE_EPS) | (q.x_v.abs() < GATE_EPS)
    return near & (q.len > 0)[None, :, None]


def grad_scales(nrm, pos, cam, L, C, alpha, gD, gS0, gS1, vis=None, dtype=F64):
    """-> (scale of d alpha [NP], scale of d normals [NP], allowance of d alpha [NP], allowance of d normals [NP])."""
    q = pairs(nrm, pos, cam, L, alpha, dtype)
    A0, A = _abs_weights(q, C, gD, gS0, gS1, dtype)
    v = torch.ones_like(q.x_l) if vis is None else vis.to(dtype)
    pa, pn = _parts(q, A0, A, v, False)
    ja, jn = _parts(q, A0, A, v * _near(q).to(dtype), True)
    return pa, pn, ja, jn


def gate_allowance(nrm, pos, cam, L, C, alpha, gD, gS0, gS1, vis=None, dtype=F64):
    """-> (J_D, J_S0, J_S1 [B,NP,3], J_dC [B,J,3]): the sums over the pairs within GATE_EPS of a gate alone, gates open, every
    part at its absolute value."""
    q = pairs(nrm, pos, cam, L, alpha, dtype)
    v = _near(q).to(dtype) * (1.0 if vis is None else vis.to(dtype))
    nl = q.x_l.abs().clamp(max=1.0)
    k = q.kk_open * nl
    Cd = C.to(dtype).abs()
    B = Cd.shape[0]
    m = [(v * x).expand(B, -1, -1) for x in (nl, k, k * q.f)]
    JD, JS0, JS1 = (torch.einsum("bjk,bpj->bpk", Cd, x) for x in m)
    JdC = sum(torch.einsum("bpk,bpj->bjk", g.to(dtype).abs(), x) for g, x in zip((gD, gS0, gS1), m))
    return JD, JS0, JS1, JdC


# ------------------------------------------------------------------------------------------------ the GPU test's cases
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
    """One case (CPU float32 tensors): the generator's problem, a roughness of ``kind``, materials, upstream gradients, a 60 %
    mask."""
    nrm, pos, cam, L, C = problem(B, NP, J, seed=100 + B + NP, per_image_dirs=per_image)
    if NP == 1 and J == 1:
        # the stock seed's lone pixel faces away from its texel: turn its normal towards it
        nrm[0] = 0.7 * torch.nn.functional.normalize(L[0, 0] + torch.tensor([0.3, -0.2, 0.1]), dim=0)
        pos[0] = torch.tensor([0.1, -0.2, 0.05])
    g = torch.Generator().manual_seed(7 * NP + J)
    rough = {"r02": torch.tensor(0.2), "r07": torch.tensor(0.7)}.get(kind)
    if rough is None:
        rough = torch.rand(NP, generator=g) * 0.9 + 0.1
    c = types.SimpleNamespace(B=B, NP=NP, J=J, per_image=per_image, kind=kind, nrm=nrm, pos=pos, cam=cam, L=L, C=C, rough=rough,
                              alpha=rough * rough, bg=(nrm == 0).all(-1))
    c.base_color = torch.rand(NP, 3, generator=g)
    c.metallic = torch.rand(NP, generator=g)
    c.gD, c.gS0, c.gS1, c.w = (torch.randn(B, NP, 3, generator=g) for _ in range(4))
    c.vis = torch.rand(L.shape[0], NP, J, generator=g) < 0.6
    if NP == 1 and J == 1:
        c.vis[:] = True  # (its one bit unset would leave nothing to check again)
    return c


def all_cases():
    return [s + (k,) for s in SHAPES for k in ROUGHNESS]


def evaluate(c, vis, dtype=F64):
    """Every compared quantity of one case under one mask (None or booleans), by the definition and its autograd in ``dtype``."""
    nrm = c.nrm.to(dtype).clone().requires_grad_(True)  # (clones: .to() of the same dtype is the case's own tensor)
    C = c.C.to(dtype).clone().requires_grad_(True)
    al = c.alpha.to(dtype).expand(c.NP).clone().requires_grad_(True)  # d alpha per pixel, as the dpixel call returns it
    D, S0, S1 = shade_terms_ggx_ref(nrm, c.pos, c.cam, c.L, C, al, vis=vis, dtype=dtype)
    loss = (D * c.gD.to(dtype)).sum() + (S0 * c.gS0.to(dtype)).sum() + (S1 * c.gS1.to(dtype)).sum()
    dC, dal, dn = torch.autograd.grad(loss, (C, al, nrm))
    # the composed path: roughness -> alpha = r^2 in the graph, base colour and metallic per pixel
    r = c.rough.to(dtype).clone().requires_grad_(True)
    bc = c.base_color.to(dtype).clone().requires_grad_(True)
    me = c.metallic.to(dtype).clone().requires_grad_(True)
    C2 = c.C.to(dtype).clone().requires_grad_(True)
    T = shade_terms_ggx_ref(c.nrm.to(dtype), c.pos, c.cam, c.L, C2, r * r, vis=vis, dtype=dtype)
    col = compose_microfacet_ref(*T, bc, me)
    dC_col, dbc, dr, dme = torch.autograd.grad((col * c.w.to(dtype)).sum(), (C2, bc, r, me))
    out = dict(D=D, S0=S0, S1=S1, dC=dC, dalpha=dal, dn=dn, colours=col, dC_col=dC_col, d_base_color=dbc, d_roughness=dr,
               d_metallic=dme)
    return {k: v.detach() for k, v in out.items()}


def composed_upstreams(c, dtype=F64):
    """(gD, gS0, gS1) that compose_microfacet's backward hands the terms for the upstream colour gradient c.w."""
    w, bc, m = c.w.to(dtype), c.base_color.to(dtype), c.metallic.to(dtype).reshape(-1, 1)
    F0 = 0.04 * (1 - m) + bc * m
    return w * (1 - m) * bc, w * F0, w * (1 - F0)


@functools.lru_cache(maxsize=None)
def reference(B, NP, J, per_image, kind, mask):
    """``entries`` of one of the GPU test's cases."""
    c = case(B, NP, J, per_image, kind)
    return entries(c, c.vis if mask == "random" else None)


def entries(c, vis):
    """float64 values, scales and allowances of one problem (a namespace with ``case``'s fields): {quantity: (reference, scale,
    allowance)} -- an evaluation is held to |got - reference| <= bound(scale) + allowance elementwise (``over_bound``; scale,
    allowance: floats or tensors that broadcast)."""
    ref = evaluate(c, vis)
    geo = (c.nrm, c.pos, c.cam, c.L, c.C, c.alpha)
    pa, pn, ja, jn = grad_scales(*geo, c.gD, c.gS0, c.gS1, vis=vis)
    JD, JS0, JS1, JdC = gate_allowance(*geo, c.gD, c.gS0, c.gS1, vis=vis)
    # the composed path: compose_microfacet is linear in the terms, so its allowances are the terms' under its own upstreams
    ups = composed_upstreams(c)
    pa2, _, ja2, _ = grad_scales(*geo, *ups, vis=vis)
    _, _, _, JdC2 = gate_allowance(*geo, *ups, vis=vis)
    bc, m = c.base_color.double(), c.metallic.double().reshape(-1, 1)
    F0 = 0.04 * (1 - m) + bc * m
    Jcol = (1 - m) * bc * JD + F0 * JS0 + (1 - F0) * JS1
    wa = c.w.double().abs()
    r2 = 2.0 * c.rough.double()
    sum_all = c.rough.numel() == 1  # one roughness for all pixels: its gradient is the sum over them
    out = {}
    mx = lambda t: float(t.abs().max())
    out["D"], out["S0"], out["S1"] = (ref["D"], mx(ref["D"]), JD), (ref["S0"], mx(ref["S0"]), JS0), (ref["S1"], mx(ref["S1"]), JS1)
    out["dC"] = (ref["dC"], mx(ref["dC"]), JdC)
    out["dalpha"] = (ref["dalpha"], pa, ja)
    out["dn"] = (ref["dn"], pn[:, None], jn[:, None])
    out["colours"] = (ref["colours"], mx(ref["colours"]), Jcol)
    out["dC_col"] = (ref["dC_col"], mx(ref["dC_col"]), JdC2)
    out["d_base_color"] = (ref["d_base_color"], mx(ref["d_base_color"]),
                           (wa * ((1 - m) * JD + m * (JS0 + JS1))).sum(0))
    out["d_metallic"] = (ref["d_metallic"], mx(ref["d_metallic"]), (wa * (bc * JD + (bc + 0.04) * (JS0 + JS1))).sum(dim=(0, 2)))
    out["d_roughness"] = (ref["d_roughness"], (r2 * pa2).sum() if sum_all else r2 * pa2, (r2 * ja2).sum() if sum_all else r2 * ja2)
    return out


def _over_and_scale(got, entry):
    ref, scale, allow = entry
    over = ((torch.as_tensor(got).detach().double().cpu() - ref).abs() - allow).clamp_min(0.0)
    scale = torch.as_tensor(scale, dtype=F64)
    scale = scale.expand_as(over) if scale.dim() else scale.reshape([1] * over.dim()).expand_as(over)
    return over, scale


def _worst(over, bound):
    """worst over / bound; where the bound is 0 the value must be exact: 0 when it is, inf when it is not."""
    ratio = torch.where(bound > 0, over / bound.clamp_min(1e-300), torch.where(over > 0, torch.full_like(over, float("inf")), over))
    return float(ratio.max()) if ratio.numel() else 0.0


def error_ratio(got, entry):
    """worst (|got - reference| - allowance) / scale over the elements."""
    return _worst(*_over_and_scale(got, entry))


def bound(entry, factor):
    """max(factor * scale, FLOOR * largest |reference|) + allowance, in the reference's shape: the quantity's factor on its own
    scale (elementwise for d alpha, d normals, d roughness), with the scalar shader's tolerance of the largest reference value
    as the floor."""
    ref, scale, allow = entry
    scale = torch.as_tensor(scale, dtype=F64)
    scale = scale.expand_as(ref) if scale.dim() else scale.reshape([1] * ref.dim()).expand_as(ref)
    floor = FLOOR * float(ref.abs().max()) if ref.numel() else 0.0
    return (factor * scale).clamp_min(floor) + allow


def over_bound(got, entry, factor):
    """worst (|got - reference| - allowance) / max(factor * scale, floor) over the elements (see ``bound``)."""
    over, _ = _over_and_scale(got, entry)
    return _worst(over, bound(entry, factor) - entry[2])


@functools.lru_cache(maxsize=None)
def float32_ratios():
    """{quantity: worst error ratio of the definition evaluated in float32 torch (CPU) against float64} over the 42 cases."""
    worst = {k: 0.0 for k in QUANTITIES}
    for (B, NP, J, per_image, kind) in all_cases():
        c = case(B, NP, J, per_image, kind)
        for mask in MASKS:
            got = evaluate(c, c.vis if mask == "random" else None, dtype=torch.float32)
            ref = reference(B, NP, J, per_image, kind, mask)
            for k in QUANTITIES:
                worst[k] = max(worst[k], error_ratio(got[k], ref[k]))
    return worst


@functools.lru_cache(maxsize=None)
def factors():
    """{quantity: factor}: four times the float32 evaluation's worst ratio (``over_bound`` applies the floor)."""
    return {k: 4.0 * r for k, r in float32_ratios().items()}
