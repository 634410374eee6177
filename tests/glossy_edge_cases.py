"""Edge shapes of the glossy lighting kernels (reni_tu_glossy.hip, reni_tu_glossy_bwd.hip): the case lists, the input
builders, the float64 references and the fp32 restatements that tests/test_glossy_edges_cpu.py and
tests/test_gpu_glossy_edges.py share.

Plain data on the CPU; nothing here touches a device.  Every builder is cached and deterministic: treat what it returns
as read-only.  A batch case of N maps is the first N maps of the builder's 22-map batch, so one float64 reference per
shape serves every N.  Every error is measured relative to max |reference| of ONE map (and one lobe), never of the batch.

Directions.  Uniform random directions do not work at these shapes: with Q = 3 and phong(500) an output row sees nothing,
the fp32 denominator underflows and the kernel's "0 where the sum is not positive" disagrees with float64 for a reason that
has nothing to do with the kernel; and a lone off-peak texel has |d ln f / dt| = p / t, above the peak sensitivity lobe_tol
budgets for.  So in_dirs are random unit vectors and every out_dirs[o] is a named texel's direction plus a perturbation of
length PERTURB, renormalised (cosine >= 0.999): row 0 looks at texel Q - 1 (the odd tail's), the next rows at texel 0 and at
the texels either side of each chunk boundary, the others walk the texels cyclically.  The transpose reduces over the rows:
there every row, the last one, the first one and those at the chunk boundaries among them, lies next to a texel, and the
indicator gradients sit at those rows.

A builder restates its case in fp32 (each operation rounded once, the kernel's dot order, the lobes of reni_sphere.inc, ONE
sequential chain over the reduction: a harsher order than the kernel's pairs and splits) and moves to its next seed until
that restatement stays within ROOM = 0.75 of every budget and every float64 denominator is above 0.1 of its lobe's
largest; the budgets themselves (tests/test_glossy_cpu.py::lobe_tol) are never widened."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from reni_amd import glossy
from tests.baseline_edge_cases import DF_N, DF_SHAPES
from tests.test_glossy_cpu import lobe_tol, np_lobe, random_dirs
from tests.test_gpu_glossy import LOBES

f32 = np.float32
ROOM = 0.75      # the share of a budget plain fp32 arithmetic may use up
PERTURB = 0.02   # length of the offset between an output row and its texel
SCALE = 0.75     # the unnormalised calls' scale (tests/test_gpu_glossy_grad.py's)
NMAX = 22
LB_N = DF_N      # 3 N + 1 = 4, 31 (the last CT = 1 shape), 34, 64 (a column pair exactly full), 67
assert LB_N == (1, 10, 11, 21, 22)

FWD_SHAPES = DF_SHAPES + ((1, 6145),)            # (P, Q); (1, 6145): three chunks, 2050 + 2050 + 2045
BWD_SHAPES = tuple((Q, P) for P, Q in FWD_SHAPES)  # (P, Q) of the transpose: its reduction runs over P
SIXTEEN_FWD, SIXTEEN_BWD = (1, 4097), (4097, 1)
PHONG16 = tuple(glossy.phong(n) for n in range(1, 17))
_MIX = ([glossy.phong(n) for n in (2, 8, 32, 64, 200, 500)], [glossy.blinn(s) for s in (10, 20, 50, 200, 500)],
        [glossy.ggx(r) for r in (1.0, 0.8, 0.5, 0.35, 0.25)])
MIX16 = tuple(_MIX[k % 3][k // 3] for k in range(18) if k // 3 < len(_MIX[k % 3]))  # phong, blinn, ggx, phong, ...
assert len(MIX16) == 16 and [sum(l.kind == k for l in MIX16) for k in ("phong", "blinn", "ggx")] == [6, 5, 5]
LOBE_SETS = {"nine": tuple(LOBES), "phong16": PHONG16, "mix16": MIX16}


# ---------------------------------------------------------------------------------------------- the split rule
def lb_split(rows, red):
    """(S, chunk) of reni_sphere.inc's dg_split: the forwards call it with (P, Q), the transpose with (Q, P)"""
    wgs = (rows + 255) // 256
    s = min((256 + wgs - 1) // wgs, max(red // 2048, 1))
    chunk = (red + s - 1) // s
    chunk += chunk & 1
    return (red + chunk - 1) // chunk, chunk


def edge_indices(n, S, chunk):
    """the reduction indices where the kernels' loops begin and end: the last (the odd tail's), the first, and the two either
    side of every chunk boundary"""
    out = [n - 1, 0]
    for s in range(1, S):
        out += [s * chunk - 1, s * chunk]
    seen = []
    for i in out:
        if 0 <= i < n and i not in seen:
            seen.append(i)
    return seen


# ---------------------------------------------------------------------------------------------- per-map error measure
def per_map_rel(a, b):
    """[N]: max |a - b| / max |b| of each map"""
    a = np.asarray(a, np.float64).reshape(len(b), -1)
    b = np.asarray(b, np.float64).reshape(len(b), -1)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-300)


def worst_ratio(out, ref, lobes, factor=1.0):
    """out, ref [N, Lv, ...]: the largest per-map, per-lobe error / (factor lobe_tol)"""
    return max(per_map_rel(np.asarray(out)[:, k], np.asarray(ref)[:, k]).max() / (factor * lobe_tol(tuple(l)))
               for k, l in enumerate(lobes))


# ---------------------------------------------------------------------------------------------- fp32 restatement
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def t_fp32(out_dirs, in_dirs):
    """[P, Q] fp32: t = fma(oz, dz, fma(oy, dy, ox dx)), the order of both kernels"""
    o, d = np.asarray(out_dirs, f32), np.asarray(in_dirs, f32)
    t = o[:, None, 0] * d[None, :, 0]
    t = _fma(o[:, None, 1], d[None, :, 1], t)
    return _fma(o[:, None, 2], d[None, :, 2], t)


def lobe_fp32(lobe, t):
    """reni_sphere.inc's generators in numpy fp32, every operation rounded once (log2 / exp2 / the reciprocal correctly rounded
    where the hardware's are within 1 ulp)"""
    kind, p = lobe
    t = np.asarray(t, f32)
    tc = np.minimum(np.maximum(t, f32(0)), f32(1))
    m = np.minimum(np.maximum(_fma(t, f32(0.5), f32(0.5)), f32(0)), f32(1))
    with np.errstate(divide="ignore"):
        if kind == "phong":
            return np.exp2(f32(p) * np.log2(tc))
        if kind == "blinn":
            return np.exp2((f32(0.5) * f32(p)) * np.log2(m))
    a2 = f32(p) * f32(p)
    r = f32(1) / _fma(m, a2, f32(1) - m)
    return ((a2 * r) * r) * tc


def _chain(av, b):
    """[Lv, C, R] fp32: sum_k av[l, r, k] b[(l,) c, k], one fp32 product and one fp32 addition a step, k in order"""
    b = np.broadcast_to(b, (av.shape[0],) + b.shape[-2:])
    acc = np.zeros((av.shape[0], b.shape[1], av.shape[1]), f32)
    for k in range(av.shape[2]):
        acc = acc + av[:, None, :, k] * b[:, :, k, None]
    assert acc.dtype == f32
    return acc


def forward_fp32(src, in_dirs, w, out_dirs, lobes):
    """(normalised [N, Lv, P, 3], unnormalised with SCALE [N, Lv, P, 3], den [Lv, P]) fp32: k_lobe_convolve + k_lobe_finish"""
    src, w = np.asarray(src, f32), np.asarray(w, f32)
    N, Q = src.shape[:2]
    f = np.stack([lobe_fp32(tuple(l), t_fp32(out_dirs, in_dirs)) for l in lobes])  # [Lv, P, Q]
    b = np.concatenate([src.transpose(0, 2, 1).reshape(3 * N, Q), np.ones((1, Q), f32)])
    acc = _chain(f * w, b)  # the scale of a normalised call is 1
    num, den = acc[:, :-1], acc[:, -1]
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = np.where(den[:, None] > 0, num / den[:, None], f32(0))
    raw = _chain(f * (w * f32(SCALE)), b[:-1])
    shape = lambda x: x.reshape(len(lobes), N, 3, -1).transpose(1, 0, 3, 2)
    return shape(norm), shape(raw), den


def backward_fp32(g, in_dirs, w, out_dirs, lobes, den):
    """(normalised, unnormalised with SCALE) [Lv, N, Q, 3] fp32, every lobe ALONE: k_lobe_recip, k_lobe_convolve_t,
    k_lobe_finish_t.  g [N, Lv, P, 3]; den [Lv, P] fp32, the forward's"""
    g, w = np.asarray(g, f32), np.asarray(w, f32)
    N, Lv, P = g.shape[:3]
    f = np.stack([lobe_fp32(tuple(l), t_fp32(out_dirs, in_dirs)) for l in lobes])  # [Lv, P, Q]
    with np.errstate(divide="ignore"):
        rN = np.where(den > 0, np.minimum(f32(1) / den, f32(3.4028234664e38)), f32(0)).astype(f32)
    out = []
    for r in (rN, np.full_like(rN, f32(SCALE))):
        av = (f * r[:, :, None]).transpose(0, 2, 1)  # [Lv, Q, P]
        res = _chain(av, g.transpose(1, 0, 3, 2).reshape(Lv, 3 * N, P))  # [Lv, 3 N, Q]
        out.append((res * w).reshape(Lv, N, 3, -1).transpose(0, 1, 3, 2))
    return out


# ---------------------------------------------------------------------------------------------- float64 references
def _A64(in_dirs, w, out_dirs, lobes):
    """(f [Lv, P, Q], A = f w) float64 of the fp32 inputs"""
    t = np.asarray(out_dirs, np.float64) @ np.asarray(in_dirs, np.float64).T
    f = np.stack([np_lobe(tuple(l), t) for l in lobes])
    return f, f * np.asarray(w, np.float64)


def forward_ref(src, in_dirs, w, out_dirs, lobes):
    """(num [N, Lv, P, 3], den [Lv, P]) float64: the normalised result is num / den, the unnormalised SCALE num"""
    _, A = _A64(in_dirs, w, out_dirs, lobes)
    return np.einsum("lpq,nqc->nlpc", A, np.asarray(src, np.float64)), A.sum(2)


def backward_ref(g, in_dirs, w, out_dirs, lobes):
    """(normalised, unnormalised with SCALE) [Lv, N, Q, 3] float64, lobe by lobe (their sum over the lobes is the call's)"""
    _, A = _A64(in_dirs, w, out_dirs, lobes)
    g = np.asarray(g, np.float64)
    den = A.sum(2)
    return np.einsum("lpq,nlpc->lnqc", A, g / den[None, :, :, None]), SCALE * np.einsum("lpq,nlpc->lnqc", A, g)


# ---------------------------------------------------------------------------------------------- directions
def _unit(gen, n):
    d = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    return d / d.norm(dim=1, keepdim=True)


def row_texels(P, Q, named):
    """[P]: the texel every output row looks at: row 0 the last texel, the next rows the rest of `named` as P allows, the
    others walk the texels cyclically"""
    tex = np.arange(P) % Q
    head = ([Q - 1] + [i for i in named if i != Q - 1])[:P]
    tex[:len(head)] = head
    return tex


def _directions(gen, P, Q, named):
    in_dirs = _unit(gen, Q)
    tex = row_texels(P, Q, named)
    o = in_dirs[torch.from_numpy(tex)] + PERTURB * _unit(gen, P)
    return in_dirs.float(), (o / o.norm(dim=1, keepdim=True)).float(), tex


def _weights(gen, Q):
    return ((0.5 + 0.5 * torch.rand(Q, generator=gen, dtype=torch.float64)) * (4 * math.pi / Q)).float()


def _dens_ok(den):
    return bool((den > 0).all() and (den >= 0.1 * den.max(axis=1, keepdims=True)).all())


# ---------------------------------------------------------------------------------------------- forward cases
@functools.lru_cache(maxsize=None)
def fwd_case(P, Q, lobes="nine"):
    """The forward case of a shape: src [NMAX, Q, 3], in_dirs, w, out_dirs (float32 tensors), texel [P], num / den (float64),
    the indicator batch ind_src [K, Q, 3] at the texels ind_texel with its unnormalised float64 result ind_ref [K, Lv, P, 3],
    and room: the largest share of a budget the fp32 restatement uses (normalised, unnormalised, indicator)."""
    L = LOBE_SETS[lobes]
    S, chunk = lb_split(P, Q)
    named = edge_indices(Q, S, chunk)
    for attempt in range(64):
        gen = torch.Generator().manual_seed(7000 + 131 * P + Q + 7919 * attempt)
        in_dirs, out_dirs, tex = _directions(gen, P, Q, named)
        w = _weights(gen, Q)
        src = torch.rand(NMAX, Q, 3, generator=gen) * 3
        num, den = forward_ref(src.numpy(), in_dirs.numpy(), w.numpy(), out_dirs.numpy(), L)
        if not _dens_ok(den):
            continue
        # the indicator maps: one a named texel that a row looks at
        ind_texel = [int(i) for i in dict.fromkeys(tex[:1 + len(named)].tolist()) if i in named]
        ind_src = torch.zeros(len(ind_texel), Q, 3)
        for k, i in enumerate(ind_texel):
            ind_src[k, i, k % 3] = 1.0
        f64, A = _A64(in_dirs.numpy(), w.numpy(), out_dirs.numpy(), L)
        ind_ref = np.zeros((len(ind_texel), len(L), P, 3))
        for k, i in enumerate(ind_texel):
            ind_ref[k, :, :, k % 3] = SCALE * A[:, :, i]
        norm32, raw32, den32 = forward_fp32(src.numpy(), in_dirs.numpy(), w.numpy(), out_dirs.numpy(), L)
        t32 = t_fp32(out_dirs.numpy(), in_dirs.numpy())
        ind32 = np.zeros_like(ind_ref, dtype=f32)
        for k, i in enumerate(ind_texel):
            for l, lobe in enumerate(L):
                ind32[k, l, :, k % 3] = lobe_fp32(tuple(lobe), t32[:, i]) * (w.numpy()[i] * f32(SCALE))
        room = (worst_ratio(norm32, num / den[None, :, :, None], L), worst_ratio(raw32, SCALE * num, L),
                worst_ratio(ind32, ind_ref, L))
        if max(room) <= ROOM:
            return SimpleNamespace(P=P, Q=Q, lobes=L, S=S, chunk=chunk, src=src, in_dirs=in_dirs, w=w, out_dirs=out_dirs,
                                   texel=tex, num=num, den=den, den32=den32, ind_texel=ind_texel, ind_src=ind_src,
                                   ind_ref=ind_ref, room=room, attempt=attempt)
    raise AssertionError(f"no draw of the forward case (P, Q) = ({P}, {Q}), {lobes}, keeps the fp32 restatement within ROOM of its budgets")


# ---------------------------------------------------------------------------------------------- transposed cases
@functools.lru_cache(maxsize=None)
def bwd_case(P, Q, lobes="nine"):
    """The transposed case of a shape (the reduction runs over the P rows, split by lb_split(Q, P)): g [NMAX, Lv, P, 3],
    in_dirs, w, out_dirs, the float64 results refN / refU [Lv, NMAX, Q, 3] lobe by lobe, den (float64), the indicator gradients
    ind_g [K, Lv, P, 3] at the rows ind_row with indN / indU [Lv, K, Q, 3], and room (normalised, unnormalised, the two
    indicator results)."""
    L = LOBE_SETS[lobes]
    S, chunk = lb_split(Q, P)
    for attempt in range(64):
        gen = torch.Generator().manual_seed(9000 + 131 * P + Q + 7919 * attempt)
        in_dirs, out_dirs, tex = _directions(gen, P, Q, [0])  # every row next to a texel; the last row next to texel Q - 1
        w = _weights(gen, Q)
        g = torch.randn(NMAX, len(L), P, 3, generator=gen)
        ops = (in_dirs.numpy(), w.numpy(), out_dirs.numpy(), L)
        _, A = _A64(*ops)
        den = A.sum(2)
        if not _dens_ok(den):
            continue
        refN, refU = backward_ref(g.numpy(), *ops)
        ind_row = edge_indices(P, S, chunk)
        ind_g = torch.zeros(len(ind_row), len(L), P, 3)
        for k, o in enumerate(ind_row):
            ind_g[k, :, o, k % 3] = 1.0
        indN, indU = backward_ref(ind_g.numpy(), *ops)
        den32 = _chain(np.stack([lobe_fp32(tuple(l), t_fp32(out_dirs.numpy(), in_dirs.numpy())) for l in L]) * w.numpy(),
                       np.ones((1, Q), f32))[:, 0]
        gotN, gotU = backward_fp32(g.numpy(), in_dirs.numpy(), w.numpy(), out_dirs.numpy(), L, den32)
        iN, iU = backward_fp32(ind_g.numpy(), in_dirs.numpy(), w.numpy(), out_dirs.numpy(), L, den32)
        sw = lambda x: np.swapaxes(x, 0, 1)  # [N, Lv, ...] for worst_ratio
        room = (worst_ratio(sw(gotN), sw(refN), L, 2.0), worst_ratio(sw(gotU), sw(refU), L),
                worst_ratio(sw(iN), sw(indN), L, 2.0), worst_ratio(sw(iU), sw(indU), L))
        if max(room) <= ROOM:
            return SimpleNamespace(P=P, Q=Q, lobes=L, S=S, chunk=chunk, g=g, in_dirs=in_dirs, w=w, out_dirs=out_dirs, texel=tex,
                                   refN=refN, refU=refU, den=den, ind_row=ind_row, ind_g=ind_g, indN=indN, indU=indU,
                                   room=room, attempt=attempt)
    raise AssertionError(f"no draw of the transposed case (P, Q) = ({P}, {Q}), {lobes}, keeps the fp32 restatement within ROOM of its budgets")


# ---------------------------------------------------------------------------------------------- lookup
# (H, W, Lv, P): H = 1 and 2 (both rows of a cell are the same row, or each other's far side), W = 2 (half = 1), one level,
# P on either side of a 256-lane block
LOOKUP_CASES = ((1, 2, 1, 1), (1, 2, 3, 255), (2, 2, 1, 256), (2, 4, 2, 257), (3, 6, 3, 513))
LOOKUP_MAPS = 3
LEFT_OUT = 0.03  # the share of directions the oracle may leave out (tests/test_gpu_glossy.py's cap)
_EPS = 1e-4
# the special directions of tests/test_gpu_glossy.py::test_lookup_special_directions_and_pixel_centres
LOOKUP_SPECIAL = np.asarray(
    [[0, 1, 0], [0, -1, 0], [0, 5, 0], [0, -0.01, 0], [0, 0, 0], [-0.0, 0.0, -0.0],  # poles, zero
     [0, 0, 1], [0, 0.5, 1], [1e-7, 0, 1], [-1e-7, 0, 1], [0, -0.5, 3], [-0.0, 0.2, 1],  # the +-pi seam
     [_EPS, 1, 0], [-_EPS, 1, _EPS], [0, -1, _EPS], [_EPS, -1, -_EPS], [1e-3, 1, 1e-3], [3e-2, -1, 1e-2],  # caps
     [0, 0, -1], [1, 0, 0], [-1, 0, 0]], np.float32)


def _lookup_dirs(H, n, seed):
    """n directions of random_dirs(., seed), in its order.  The oracle compares outside the polar caps only
    (tests/test_rotate_cpu.py's CAP rule), and at H = 1, 2, 3 the caps hold 96 %, 29 % and 13 % of the sphere: directions
    inside them are taken only while they stay within LEFT_OUT of the n, so that the oracle's own cap holds at these sizes."""
    from tests.test_glossy_cpu import lookup_coordinates
    from tests.test_rotate_cpu import CAP
    pool = random_dirs(8192 if H == 1 else 64 + 2 * n, seed)
    keep = lookup_coordinates(H, 2, pool)[2] >= CAP * math.sin(math.pi / (2 * H))
    allowed, out = int(LEFT_OUT * n), []
    for d, k in zip(pool, keep):
        if k or allowed > 0:
            out.append(d)
            allowed -= 0 if k else 1
        if len(out) == n:
            return np.stack(out)
    raise AssertionError(f"random_dirs(., {seed}) holds fewer than {n} directions for H = {H}")


@functools.lru_cache(maxsize=None)
def lookup_case(H, W, Lv, P):
    """chain [3, Lv, H, W, 3]; dirs [P, 3] and per_map [3, P, 3]: R random directions, then (where P allows) the special
    ones; level [P] and level_np [3, P] in [-0.5, Lv - 0.5] with exact integers and, where P allows, a NaN, which the kernels
    read as level 0: level_clean / level_np_clean hold 0 there, for the oracle.  The oracle's comparison and its cap cover
    the R random directions; the special ones (poles, the zero vector) are checked for finiteness and range, as
    tests/test_gpu_glossy.py checks them."""
    idx = LOOKUP_CASES.index((H, W, Lv, P))
    g = np.random.default_rng(600 + idx)
    chain = g.random((LOOKUP_MAPS, Lv, H, W, 3)).astype(f32)
    R = P - len(LOOKUP_SPECIAL) if P > len(LOOKUP_SPECIAL) else P
    tail = LOOKUP_SPECIAL[:P - R]
    dirs = np.concatenate([_lookup_dirs(H, R, 40 + idx), tail])
    per_map = np.stack([np.concatenate([_lookup_dirs(H, R, 400 + 10 * idx + n), tail]) for n in range(LOOKUP_MAPS)])
    level_np = g.uniform(-0.5, Lv - 0.5, (LOOKUP_MAPS, P)).astype(f32)
    level = g.uniform(-0.5, Lv - 0.5, P).astype(f32)
    level[0] = 0.0
    if P > 8:
        level[[1, 5]] = Lv - 1.0
        level[[2, P - 1]] = np.nan
        level[3] = min(1.0, Lv - 1.0)
        level_np[:, 0], level_np[:, 4], level_np[1, 7] = 0.0, Lv - 1.0, np.nan
    clean = lambda x: np.where(np.isnan(x), f32(0), x)
    return SimpleNamespace(H=H, W=W, Lv=Lv, P=P, R=R, chain=chain, dirs=dirs, per_map=per_map, level=level, level_np=level_np,
                           level_clean=clean(level), level_np_clean=clean(level_np))
