"""CPU tests of the map scores (reni_amd/metrics.py, reni_tu_metrics.hip: reni_pair_stats, reni_ssim).

Holds the float64 oracles tests/test_gpu_metrics.py compares the HIP kernels against (np_pair_stats, np_ssim_map / np_ssim,
written from the definitions in include/reni_hip.h, not from the kernels) and the error budget the comparison is held to
(stats_budget, ssim_budget).  Here: the oracles' own identities, the budget against a float32 restatement of the operation
chain, the host pieces of metrics.py, the unit's ISA audit and the C ABI's argument checks.

The error budget.  u = 2^-24 is fp32's unit roundoff.
  stored space   every term of a sum is formed from the given fp32 numbers with at most 4 roundings (difference, square or
                 product, the weight, the channel sum) and is non-negative; a summation tree over at most 2^24 terms is at most
                 24 levels deep, each level one rounding of a partial sum of non-negative terms: relative error at most
                 (4 + 24) u to first order, held to 64 u to cover the second-order terms and the double -> fp32 rounding of the
                 result.  Signed sums (entries 3 and 7) get the same 64 u on the sum of the terms' magnitudes.  Max and min
                 are exact.
  mapped spaces  exp and pow differ between libraries by a few ulp, the fp32 roundings of minmax shift every exponent by up to
                 u (|m0| + m1 - m0), and p - t cancels, so the bound is absolute: a mapped value carries a relative error k u, and
                     |d SSE| <= k u sum w sum_c |p - t| (|p| + |t|) + 64 u SSE
                     |d SAE| <= k u sum w sum_c (|p| + |t|)         + 64 u SAE
                     |d cos| <= 4 k u sum w                         + 64 u sum w       (a cosine moves by at most 2 (k u + k u))
                     |d max|, |d min| <= k u |max|, k u |min|
                     |d St2| <= 2 k u sum w sum_c t^2               + 64 u St2
                     |d St1| <= k u sum w sum_c |t|                 + 64 u sum w sum_c |t|
  SSIM           with A = 2 mu_p mu_t + C1, B = 2 cov + C2, C = mu_p^2 + mu_t^2 + C1, D = var_p + var_t + C2: |A| <= C and
                 |B| <= D, so the roundings of A and C move ssim = A B / (C D) by O(u); B and D are differences of moments of
                 size E[p^2] + E[t^2], so their roundings (and the inputs' relative errors) move it by
                 O(u) (E[p^2] + E[t^2]) / D.  Per pixel and channel
                     |d ssim| <= K u kappa,   kappa = 1 + 2 (E[p^2] + E[t^2]) / (var_p + var_t + C2)
                 (kappa from the float64 oracle), the map's bound is the channel mean, the image's the weighted mean + 64 u.
  the constants  K_MAP and K_SSIM per space are 4 x the largest ratio err / (u x shape term) that the float32 restatement below
                 (np32_pair_stats, np32_ssim: the same chain in numpy float32, summed once sequentially and once pairwise)
                 shows against the float64 oracle on the test inputs, rounded up: 4 because the device's expf, powf and the
                 contraction of a multiply-add are not numpy's and a few ulp of difference are expected.  The measured ratios
                 are printed by test_float32_restatement_stays_inside_the_budget, which asserts that the restatement stays
                 inside the budget and that the constants are indeed at least 4 x what it shows.  The 64 u is the bound of a
                 TREE, which the kernel is (8 terms per thread, a butterfly, then double); the sequential run's long sums
                 are outside that derivation -- their error grows with the number of terms -- and are asserted against the
                 bound derived for them (sequential_sum_u: n + 3 roundings, doubled for a quotient) instead; they do not
                 feed K_MAP, which models a mapped value's error.
"""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from oracle import reni_oracle as O
from reni_amd import metrics  # noqa: F401  (at import: without the module nothing in this file has a subject)
from tests import isa_audit
from tests.test_rotate_cpu import FLIP_X, FLIP_Y, FLIP_Z, sky_maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
SPACES = ("stored", "linear", "srgb")
SUM_U = 64.0  # the tree bound above, in units of u

# measured by test_float32_restatement_stays_inside_the_budget (largest ratio over 16 x 32 and 64 x 128, all weights, both
# summation orders), then x 4 and rounded up:            the restatement's largest ratio
K_MAP = {"stored": 0.0, "linear": 112.0, "srgb": 112.0}   # linear 27.3, srgb 27.4 (26 of them: the fp32 rounding of minmax)
K_SSIM = {"stored": 8.0, "linear": 13.0, "srgb": 10.0}     # stored 1.8, linear 3.2, srgb 2.4


# ------------------------------------------------------------------------------------------ inputs
def pair_maps(B, H, W, seed):
    """(pred, target) float32 [B, 3, H, W] in stored space: target = MinMaxNormalise(oracle.MINMAX) of sky_maps (five decades of
    range; map 1 has negatives, which the transform clips to the smallest positive value), pred = target plus a smooth
    ripple and noise of a few percent of the stored range"""
    from reni_amd.custom_transforms import MinMaxNormalise
    raw = torch.from_numpy(sky_maps(B, H, W, seed))
    t = torch.stack([MinMaxNormalise(O.MINMAX)(x) for x in raw]).numpy().astype(np.float32)
    g = np.random.default_rng(seed + 1000)
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    ripple = 0.03 * np.sin(2 * np.pi * (3 * xx + 2 * yy))[None, None]
    p = t + ripple + 0.02 * g.standard_normal(t.shape)
    return p.astype(np.float32), t


def sin_rows(H):
    return np.sin(np.pi * (np.arange(H) + 0.5) / H)


def np_exposure(target, minmax):
    """[B] float32: the nested 0.98-quantile of the linear target (float64, rounded once)"""
    lin = np_map(target, "linear", minmax, None)
    q = np.quantile(np.quantile(np.quantile(lin, 0.98, axis=1), 0.98, axis=1), 0.98, axis=1)
    return q.astype(np.float32)


# ------------------------------------------------------------------------------------------ float64 oracles
def np_map(x, space, minmax, expo):
    """x [B, 3, H, W] mapped into `space`, float64"""
    x = np.asarray(x, np.float64)
    if space == "stored":
        return x
    m0, m1 = float(minmax[0]), float(minmax[1])
    lin = np.exp(0.5 * (x + 1.0) * (m1 - m0) + m0)
    if space == "linear":
        return lin
    assert space == "srgb"
    y = np.clip(lin / np.asarray(expo, np.float64).reshape(-1, 1, 1, 1), 0.0, 1.0)
    return np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.abs(y) ** (1.0 / 2.4) - 0.055)


def _weight(weight, B, H, W):
    return np.ones((B, H, W)) if weight is None else np.broadcast_to(np.asarray(weight, np.float64), (B, H, W))


def np_pair_stats(pred, target, weight=None, space="stored", minmax=None, expo=None):
    """[B, 8] float64, the entries of reni_pair_stats from their definitions"""
    p, t = np_map(pred, space, minmax, expo), np_map(target, space, minmax, expo)
    B, _, H, W = p.shape
    w = _weight(weight, B, H, W)
    out = np.zeros((B, 8))
    out[:, 0] = w.sum((1, 2))
    out[:, 1] = (w * ((p - t) ** 2).sum(1)).sum((1, 2))
    out[:, 2] = (w * np.abs(p - t).sum(1)).sum((1, 2))
    cos = (p * t).sum(1) / (np.maximum(np.sqrt((p * p).sum(1)), 1e-20) * np.maximum(np.sqrt((t * t).sum(1)), 1e-20))
    out[:, 3] = (w * cos).sum((1, 2))
    live = np.broadcast_to((w > 0)[:, None], t.shape)
    out[:, 4] = np.where(live, t, -np.inf).max((1, 2, 3))
    out[:, 5] = np.where(live, t, np.inf).min((1, 2, 3))
    out[:, 6] = (w * (t * t).sum(1)).sum((1, 2))
    out[:, 7] = (w * t.sum(1)).sum((1, 2))
    return out


def gaussian11():
    x = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-x * x / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def sphere_pad(img, r=5):
    """img [..., H, W] -> [..., H + 2 r, W + 2 r]: tap (i, j) with i < 0 is row -1 - i at column j + W / 2, with i >= H row
    2 H - 1 - i at column j + W / 2; then the column modulo W"""
    H, W = img.shape[-2:]
    assert W % 2 == 0 and H >= r
    i = np.arange(-r, H + r)[:, None]
    j = np.arange(-r, W + r)[None, :]
    over = (i < 0) | (i >= H)
    ii = np.where(i < 0, -1 - i, np.where(i >= H, 2 * H - 1 - i, i))
    jj = np.mod(np.where(over, j + W // 2, j), W)
    return img[..., np.broadcast_to(ii, jj.shape), jj]


def _window_moments(x, y, g):
    """the five windowed moments of x, y [..., Hp, Wp] over every 11 x 11 window inside them: [5][..., Hp - 10, Wp - 10]"""
    def corr(a):
        n = a.shape[-1] - 10
        h = sum(g[k] * a[..., :, k:k + n] for k in range(11))
        m = a.shape[-2] - 10
        return sum(g[k] * h[..., k:k + m, :] for k in range(11))
    return corr(x), corr(y), corr(x * x), corr(y * y), corr(x * y)


def np_ssim_map(pred, target, space="stored", minmax=None, expo=None, L=1.0, sphere=True, with_kappa=False):
    """[B, H, W] float64: the channel-mean SSIM map (planar mode: zero on the border of 5); with_kappa: also the channel mean
    of kappa = 1 + 2 (E[p^2] + E[t^2]) / (var_p + var_t + C2), the condition number of ssim_budget"""
    p, t = np_map(pred, space, minmax, expo), np_map(target, space, minmax, expo)
    B, _, H, W = p.shape
    if sphere:
        p, t = sphere_pad(p), sphere_pad(t)
    mp, mt, epp, ett, ept = _window_moments(p, t, gaussian11())
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    vp, vt, cov = epp - mp * mp, ett - mt * mt, ept - mp * mt
    s = ((2 * mp * mt + C1) * (2 * cov + C2)) / ((mp * mp + mt * mt + C1) * (vp + vt + C2))
    kappa = 1.0 + 2.0 * (epp + ett) / (vp + vt + C2)
    s, kappa = s.mean(1), kappa.mean(1)
    if not sphere:
        full, fk = np.zeros((B, H, W)), np.zeros((B, H, W))
        full[:, 5:H - 5, 5:W - 5], fk[:, 5:H - 5, 5:W - 5] = s, kappa
        s, kappa = full, fk
    return (s, kappa) if with_kappa else s


def ssim_mean(smap, weight=None, sphere=True):
    """[B]: sum w ssim / sum w over all pixels (sphere), the plain mean over the (H - 10) x (W - 10) interior (planar)"""
    B, H, W = smap.shape
    if not sphere:
        assert weight is None
        return smap[:, 5:H - 5, 5:W - 5].mean((1, 2))
    w = _weight(weight, B, H, W)
    return (w * smap).sum((1, 2)) / w.sum((1, 2))


def np_ssim(pred, target, weight=None, space="stored", minmax=None, expo=None, L=1.0, sphere=True):
    return ssim_mean(np_ssim_map(pred, target, space, minmax, expo, L, sphere), weight, sphere)


# ------------------------------------------------------------------------------------------ the budget
def stats_budget(pred, target, weight=None, space="stored", minmax=None, expo=None, k=None, sum_u=None):
    """[B, 8]: bound on |fp32 kernel - float64 oracle| per entry of reni_pair_stats (the module docstring derives it)"""
    k = K_MAP[space] if k is None else k
    SUM = SUM_U if sum_u is None else sum_u  # (a tree; sequential_sum_u(n) for n terms added one after the other)
    p, t = np_map(pred, space, minmax, expo), np_map(target, space, minmax, expo)
    B, _, H, W = p.shape
    w = _weight(weight, B, H, W)
    ref = np_pair_stats(pred, target, weight, space, minmax, expo)

    def S(x):
        return (w * x.sum(1)).sum((1, 2))

    u = EPS32
    out = np.zeros((B, 8))
    out[:, 0] = SUM * u * ref[:, 0]
    out[:, 1] = k * u * S(np.abs(p - t) * (np.abs(p) + np.abs(t))) + SUM * u * ref[:, 1]
    out[:, 2] = k * u * S(np.abs(p) + np.abs(t)) + SUM * u * ref[:, 2]
    out[:, 3] = (4 * k + SUM) * u * ref[:, 0]
    out[:, 4] = k * u * np.abs(ref[:, 4])
    out[:, 5] = k * u * np.abs(ref[:, 5])
    out[:, 6] = (2 * k + SUM) * u * ref[:, 6]
    out[:, 7] = (k + SUM) * u * S(np.abs(t))
    return out


def ssim_budget(kappa, weight=None, space="stored", sphere=True, k=None, sum_u=None):
    """(per-pixel bound [B, H, W], per-image bound [B]) from the oracle's kappa map"""
    k = K_SSIM[space] if k is None else k
    pix = k * EPS32 * kappa
    return pix, ssim_mean(pix, weight, sphere) + (SUM_U if sum_u is None else sum_u) * EPS32


def sequential_sum_u(n):
    """the summation term, in units of u, for n terms added one after the other: n - 1 additions, each one rounding of a partial
    sum that is at most the sum of the magnitudes, plus the 4 roundings of a term; doubled for a quotient of two such sums"""
    return 2.0 * (n + 3)


# ------------------------------------------------------------------------------------------ float32 restatement
F = np.float32


def _sum32(x, axis_from, pairwise):
    """fp32 sum of x over its trailing axes from `axis_from`: numpy's pairwise reduction (of one contiguous row at a time: only
    then is it pairwise), or one term after the other"""
    x = np.ascontiguousarray(np.asarray(x, F))
    lead = x.shape[:axis_from]
    rows = x.reshape(int(np.prod(lead, dtype=np.int64)), -1)
    out = [r.sum(dtype=F) if pairwise else np.cumsum(r, dtype=F)[-1] for r in rows]
    return np.asarray(out, F).reshape(lead)


def np32_map(x, space, minmax, expo):
    x = np.asarray(x, F)
    if space == "stored":
        return x
    rng, m0 = F(float(minmax[1]) - float(minmax[0])), F(minmax[0])
    lin = np.exp((F(0.5) * (x + F(1))) * rng + m0)
    assert lin.dtype == F
    if space == "linear":
        return lin
    y = np.clip(lin / np.asarray(expo, F).reshape(-1, 1, 1, 1), F(0), F(1))
    return np.where(y <= F(0.0031308), F(12.92) * y, F(1.055) * np.power(np.abs(y), F(1.0 / 2.4)) - F(0.055)).astype(F)


def np32_pair_stats(pred, target, weight=None, space="stored", minmax=None, expo=None, pairwise=True):
    p, t = np32_map(pred, space, minmax, expo), np32_map(target, space, minmax, expo)
    B, _, H, W = p.shape
    w = _weight(weight, B, H, W).astype(F)
    d = p - t
    out = np.zeros((B, 8), F)
    out[:, 0] = _sum32(w, 1, pairwise)
    out[:, 1] = _sum32(w * (d * d).sum(1, dtype=F), 1, pairwise)
    out[:, 2] = _sum32(w * np.abs(d).sum(1, dtype=F), 1, pairwise)
    cos = (p * t).sum(1, dtype=F) / (np.maximum(np.sqrt((p * p).sum(1, dtype=F)), F(1e-20))
                                     * np.maximum(np.sqrt((t * t).sum(1, dtype=F)), F(1e-20)))
    out[:, 3] = _sum32(w * cos, 1, pairwise)
    live = np.broadcast_to((w > 0)[:, None], t.shape)
    out[:, 4] = np.where(live, t, -np.inf).max((1, 2, 3))
    out[:, 5] = np.where(live, t, np.inf).min((1, 2, 3))
    out[:, 6] = _sum32(w * (t * t).sum(1, dtype=F), 1, pairwise)
    out[:, 7] = _sum32(w * t.sum(1, dtype=F), 1, pairwise)
    assert cos.dtype == F
    return out.astype(np.float64)


def np32_ssim(pred, target, weight=None, space="stored", minmax=None, expo=None, L=1.0, sphere=True, pairwise=True):
    """(map [B, H, W], mean [B]) with every operation rounded to fp32, the taps of a window added in order or pairwise"""
    p, t = np32_map(pred, space, minmax, expo), np32_map(target, space, minmax, expo)
    B, _, H, W = p.shape
    if sphere:
        p, t = sphere_pad(p), sphere_pad(t)
    g = gaussian11().astype(F)

    def taps(terms):
        if pairwise:  # a balanced tree over the 11 taps
            while len(terms) > 1:
                terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
            return terms[0]
        acc = terms[0]
        for x in terms[1:]:
            acc = acc + x
        return acc

    def corr(a, b=None):
        n, m = a.shape[-1] - 10, a.shape[-2] - 10
        if b is None:
            h = taps([g[k] * a[..., :, k:k + n] for k in range(11)])
        else:
            h = taps([(g[k] * a[..., :, k:k + n]) * b[..., :, k:k + n] for k in range(11)])
        return taps([g[k] * h[..., k:k + m, :] for k in range(11)])

    mp, mt, epp, ett, ept = corr(p), corr(t), corr(p, p), corr(t, t), corr(p, t)
    C1, C2 = F((0.01 * L) ** 2), F((0.03 * L) ** 2)
    mp2, mt2, mpt = mp * mp, mt * mt, mp * mt
    vp, vt, cov = epp - mp2, ett - mt2, ept - mpt
    s = ((F(2) * mpt + C1) * (F(2) * cov + C2)) / (((mp2 + mt2) + C1) * ((vp + vt) + C2))
    s = (s[:, 0] + s[:, 1] + s[:, 2]) / F(3)
    assert s.dtype == F
    if sphere:
        w = _weight(weight, B, H, W).astype(F)
        mean = _sum32(w * s, 1, pairwise) / _sum32(w, 1, pairwise)
        return s.astype(np.float64), mean.astype(np.float64)
    full = np.zeros((B, H, W))
    full[:, 5:H - 5, 5:W - 5] = s
    return full, (_sum32(s, 1, pairwise) / F(s.shape[1] * s.shape[2])).astype(np.float64)


def weight_cases(H, W, golden):
    """[(name, float32 weight broadcastable to [B, H, W] or None)]: none, sin(phi) per row, every golden mask x sin(phi).
    The weights are fp32 numbers (the kernel's input): the oracle is handed the same numbers, widened."""
    from reni_amd.utils import mask_from_array
    out = [("none", None), ("sin", sin_rows(H)[:, None].astype(np.float32))]
    if W == 2 * H:
        for name, m in sorted(golden("masks.npz").items()):
            mask = mask_from_array(W, m)[0, :, 0].numpy().reshape(H, W).astype(np.float64)
            out.append((name, (mask * sin_rows(H)[:, None]).astype(np.float32)))
    return out


@pytest.mark.parametrize("size", [(16, 32), (64, 128)])
def test_float32_restatement_stays_inside_the_budget(size, golden):
    """not the device (its expf and powf are other implementations), but every rounding the derivation counts is in it.  The
    ratios printed here, x 4, are K_MAP and K_SSIM; the assertion holds the restatement to the budget."""
    H, W = size
    B = 3
    pred, target = pair_maps(B, H, W, H + W)
    expo = np_exposure(target, O.MINMAX)
    worst_map = {s: 0.0 for s in SPACES}
    worst_ssim = {s: 0.0 for s in SPACES}
    for space in SPACES:
        L = {"stored": 2.0, "linear": float(np_map(target, "linear", O.MINMAX, None).max()), "srgb": 1.0}[space]
        maps = {sph: np_ssim_map(pred, target, space, O.MINMAX, expo, L, sph, with_kappa=True) for sph in (True, False)}
        for wname, w in weight_cases(H, W, golden):
            ref = np_pair_stats(pred, target, w, space, O.MINMAX, expo)
            bud = stats_budget(pred, target, w, space, O.MINMAX, expo)
            unit = stats_budget(pred, target, w, space, O.MINMAX, expo, k=1.0) - stats_budget(pred, target, w, space, O.MINMAX, expo, k=0.0)
            for pairwise in (True, False):
                got = np32_pair_stats(pred, target, w, space, O.MINMAX, expo, pairwise)
                err = np.abs(got - ref)
                ratio = float((err / np.maximum(bud, 1e-300))[bud > 0].max())
                if space != "stored":
                    cols = slice(None) if pairwise else slice(4, 6)  # (sequential: the entries without a long sum, see below)
                    r = (err / np.maximum(unit, 1e-300))[:, cols][(unit > 0)[:, cols]]
                    worst_map[space] = max(worst_map[space], float(r.max()))
                else:
                    assert np.array_equal(got[:, 4:6], ref[:, 4:6])
                print(f"{H}x{W} {space} {wname} {'pairwise' if pairwise else 'sequential'}: stats err / budget {ratio:.3f}")
                # the 64 u of a sum is the bound of a summation TREE, which is what the kernel is.  n terms added one after the
                # other are held to the bound derived for that, sequential_sum_u(n); they do not feed K_MAP, which is about a
                # mapped value's error and not about the length of a sum
                if pairwise:
                    assert ratio <= 1.0, (space, wname, pairwise)
                else:
                    seq = stats_budget(pred, target, w, space, O.MINMAX, expo, sum_u=sequential_sum_u(H * W))
                    r_seq = float((err / np.maximum(seq, 1e-300))[seq > 0].max())
                    print(f"{H}x{W} {space} {wname} sequential: stats err / sequential budget {r_seq:.3f}")
                    assert r_seq <= 1.0, (space, wname)
                for sph in (True, False):
                    if not sph and w is not None:
                        continue
                    smap, kappa = maps[sph]
                    pix, img = ssim_budget(kappa, w, space, sph)
                    gmap, gmean = np32_ssim(pred, target, w, space, O.MINMAX, expo, L, sph, pairwise)
                    inner = (slice(None),) + ((slice(None), slice(None)) if sph else (slice(5, H - 5), slice(5, W - 5)))
                    r_pix = float((np.abs(gmap - smap)[inner] / pix[inner]).max())
                    r_img = float((np.abs(gmean - ssim_mean(smap, w, sph)) / img).max())
                    worst_ssim[space] = max(worst_ssim[space], r_pix * K_SSIM[space])
                    assert r_pix <= 1.0 and (r_img <= 1.0 or not pairwise), (space, wname, sph, pairwise, r_pix, r_img)
                    if not pairwise:
                        _, img_seq = ssim_budget(kappa, w, space, sph, sum_u=sequential_sum_u(H * W))
                        assert (np.abs(gmean - ssim_mean(smap, w, sph)) <= img_seq).all(), (space, wname, sph)
    for space in SPACES:
        print(f"{H}x{W} {space}: largest stats err / (u x shape term) {worst_map[space]:.1f} (K_MAP {K_MAP[space]:g}), "
              f"largest ssim err / (u kappa) {worst_ssim[space]:.1f} (K_SSIM {K_SSIM[space]:g})")
        if space != "stored":
            assert 4.0 * worst_map[space] <= K_MAP[space]
        assert 4.0 * worst_ssim[space] <= K_SSIM[space]


# ------------------------------------------------------------------------------------------ 1. the oracles' identities
def test_oracle_ssim_of_an_image_with_itself_is_one():
    pred, target = pair_maps(2, 16, 32, 3)
    for sphere in (True, False):
        assert np.abs(np_ssim_map(target, target, L=2.0, sphere=sphere)[:, 5:-5, 5:-5] - 1.0).max() <= 1e-12
        assert np.abs(np_ssim(target, target, None, L=2.0, sphere=sphere) - 1.0).max() <= 1e-12
    assert np_ssim(pred, target, None, L=2.0).max() < 0.999


@pytest.mark.parametrize("sphere", [True, False])
def test_oracle_ssim_of_constant_images(sphere):
    for a, b, L in ((0.3, 0.5, 1.0), (-0.2, 0.7, 2.0), (4.0, 4.0, 10.0)):
        x, y = np.full((1, 3, 12, 24), a), np.full((1, 3, 12, 24), b)
        C1 = (0.01 * L) ** 2
        want = (2 * a * b + C1) / (a * a + b * b + C1)
        assert abs(float(np_ssim(x, y, None, L=L, sphere=sphere)[0]) - want) <= 1e-12


def test_oracle_offset_gives_mse_and_psnr():
    from reni_amd import metrics
    _, t = pair_maps(2, 16, 32, 5)
    delta = 0.125
    w = sin_rows(16)[:, None]
    s = np_pair_stats(t.astype(np.float64) + delta, t, w)
    mse = s[:, 1] / (3 * s[:, 0])
    assert np.abs(mse - delta ** 2).max() <= 1e-12
    assert np.abs(s[:, 2] / (3 * s[:, 0]) - delta).max() <= 1e-12
    got = metrics.psnr_from_stats(torch.from_numpy(s), 2.0).numpy()
    assert np.abs(got - 10 * math.log10(4.0 / delta ** 2)).max() <= 1e-9
    rng = metrics.psnr_from_stats(torch.from_numpy(s), "target_range").numpy()
    assert np.abs(rng - 10 * np.log10((s[:, 4] - s[:, 5]) ** 2 / delta ** 2)).max() <= 1e-9


def test_oracle_weight_zero_removes_a_pixel_from_every_entry():
    p, t = pair_maps(2, 16, 32, 6)
    H, W = 16, 32
    w = np.broadcast_to(sin_rows(H)[:, None], (H, W)).copy()
    hot = np.unravel_index(np.argmax(t[0].max(0)), (H, W))  # the bright spot: map 0's maximum
    cold = np.unravel_index(np.argmin(t[0].min(0)), (H, W))  # and the pixel of its minimum
    w[hot] = 0.0
    w[cold] = 0.0
    p2, t2 = p.copy(), t.copy()
    for (r, c) in (hot, cold):  # whatever the pixels hold does not matter
        p2[:, :, r, c], t2[:, :, r, c] = 7.0, -9.0
    a, b = np_pair_stats(p, t, w), np_pair_stats(p2, t2, w)
    assert np.array_equal(a, b)
    full = np_pair_stats(p, t, np.broadcast_to(sin_rows(H)[:, None], (H, W)))
    assert a[0, 4] < full[0, 4] and a[0, 5] > full[0, 5] and (a[:, 0] < full[:, 0]).all()
    for space in ("linear", "srgb"):
        expo = np_exposure(t, O.MINMAX)
        assert np.array_equal(np_pair_stats(p, t, w, space, O.MINMAX, expo), np_pair_stats(p2, t2, w, space, O.MINMAX, expo))


def test_oracle_sphere_scores_do_not_change_under_rolls_and_half_turns():
    """the half turns as array operations (tests/test_rotate_cpu.py's nearest-mode test): FLIP_Y is a roll by W / 2, FLIP_Z the
    flip of both axes, FLIP_X both"""
    H, W = 16, 32
    p, t = pair_maps(2, H, W, 8)
    w = np.broadcast_to(sin_rows(H)[:, None], (H, W))
    turns = {"FLIP_Y": (FLIP_Y, lambda x: np.roll(x, W // 2, axis=-1)),
             "FLIP_Z": (FLIP_Z, lambda x: x[..., ::-1, ::-1]),
             "FLIP_X": (FLIP_X, lambda x: np.roll(x[..., ::-1, ::-1], W // 2, axis=-1))}
    for k in (1, 7, W // 2 + 3, W - 1):
        turns[f"roll {k}"] = (None, lambda x, k=k: np.roll(x, k, axis=-1))
    base_s = np_ssim(p, t, w, L=2.0)
    base_map = np_ssim_map(p, t, L=2.0)
    base_p = np_pair_stats(p, t, w)
    for name, (R, op) in turns.items():
        if R is not None:
            assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.allclose(R @ R.T, np.eye(3))
        assert np.abs(np_ssim(op(p), op(t), op(w), L=2.0) - base_s).max() <= 1e-12, name
        assert np.abs(np_ssim_map(op(p), op(t), L=2.0) - op(base_map)).max() <= 1e-12, name
        st = np_pair_stats(op(p), op(t), op(w))
        assert np.abs(st - base_p).max() <= 1e-12 * np.abs(base_p).max(), name
    assert np.abs(np_ssim(p, t, None, L=2.0, sphere=False) - np_ssim(np.roll(p, 3, -1), np.roll(t, 3, -1), None, L=2.0, sphere=False)).max() > 1e-6


def test_oracle_planar_mode_is_a_direct_valid_correlation():
    H, W = 14, 19
    g = np.random.default_rng(2)
    p, t = g.random((1, 3, H, W)), g.random((1, 3, H, W))
    k2 = np.outer(gaussian11(), gaussian11())
    want = np.zeros((H - 10, W - 10))
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    for c in range(3):
        for i in range(H - 10):
            for j in range(W - 10):
                a, b = p[0, c, i:i + 11, j:j + 11], t[0, c, i:i + 11, j:j + 11]
                ma, mb = (k2 * a).sum(), (k2 * b).sum()
                va, vb, cab = (k2 * a * a).sum() - ma * ma, (k2 * b * b).sum() - mb * mb, (k2 * a * b).sum() - ma * mb
                want[i, j] += ((2 * ma * mb + C1) * (2 * cab + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2)) / 3
    got = np_ssim_map(p, t, sphere=False)
    assert np.abs(got[0, 5:-5, 5:-5] - want).max() <= 1e-12
    assert not got[0, :5].any() and not got[0, :, :5].any() and not got[0, -5:].any() and not got[0, :, -5:].any()
    assert abs(float(np_ssim(p, t, None, sphere=False)[0]) - want.mean()) <= 1e-12


# ------------------------------------------------------------------------------------------ 2. host pieces of metrics.py
def test_gaussian_window():
    from reni_amd import metrics
    g = metrics.gaussian_window()
    assert g.shape == (11,) and g.dtype == np.float64 and abs(g.sum() - 1.0) <= 1e-15
    assert np.array_equal(g, g[::-1]) and np.array_equal(g, gaussian11())
    assert abs(g[5] / g[4] - math.exp(1.0 / 4.5)) <= 1e-12 and abs(g[5] / g[0] - math.exp(25.0 / 4.5)) <= 1e-9
    w = metrics.solid_angle_weight(16)
    assert w.shape == (16, 1) and w.dtype == torch.float32 and np.abs(w[:, 0].numpy() - sin_rows(16)).max() <= 2 ** -24


def test_exposure_is_the_nested_quantile_of_srgb():
    from reni_amd import metrics
    from reni_amd.custom_transforms import UnMinMaxNormlise
    _, t = pair_maps(3, 16, 32, 9)
    tt = torch.from_numpy(t)
    got = metrics.exposure(tt, O.MINMAX)
    lin = UnMinMaxNormlise(O.MINMAX)(tt)
    want = torch.quantile(torch.quantile(torch.quantile(lin, 0.98, dim=1), 0.98, dim=1), 0.98, dim=1)
    assert got.shape == (3,) and torch.equal(got, want)
    assert np.abs(got.numpy() - np_exposure(t, O.MINMAX)).max() <= 1e-5 * float(got.max())
    assert torch.equal(metrics.exposure(lin), want)
    out = tt.permute(0, 2, 3, 1).reshape(3, -1, 3)  # as a model output
    assert torch.equal(metrics.exposure(out, O.MINMAX), want)


def _raises_value_error(fn, *a, **k):
    with pytest.raises(ValueError):
        fn(*a, **k)


def test_bad_input_raises_value_error_before_the_library_is_touched(monkeypatch):
    from reni_amd import _lib, metrics, ops

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    p, t = (torch.from_numpy(x) for x in pair_maps(2, 16, 32, 1))
    mm = O.MINMAX
    for fn in (metrics.weighted_mse, metrics.mae, metrics.cosine, metrics.psnr, metrics.ssim, ops.pair_stats, ops.ssim,
               metrics.score_maps):
        _raises_value_error(fn, p, t[:1])                       # batch mismatch
        _raises_value_error(fn, p, t[:, :, :8])                 # size mismatch
        _raises_value_error(fn, p[:, :2], t[:, :2])             # not 3 channels
        _raises_value_error(fn, p.reshape(2, -1, 3)[:, :500], t.reshape(2, -1, 3)[:, :500])  # 500 pixels are not H x 2H
    for fn in (metrics.weighted_mse, metrics.mae, metrics.cosine, metrics.psnr, metrics.ssim, ops.pair_stats, ops.ssim):
        _raises_value_error(fn, p, t, space="linear")           # a mapped space without minmax
        _raises_value_error(fn, p, t, space="srgb")
        _raises_value_error(fn, p, t, space="log")
        _raises_value_error(fn, p, t, weight=-torch.ones(16, 1))            # negative weights
        _raises_value_error(fn, p, t, weight=torch.ones(3, 16, 32))         # does not broadcast
    _raises_value_error(ops.pair_stats, p, t, space="srgb", minmax=mm)                              # no exposure
    _raises_value_error(ops.pair_stats, p, t, space="srgb", minmax=mm, exposure=torch.ones(3))      # wrong length
    _raises_value_error(ops.pair_stats, p, t, space="linear", minmax=(1.0, 1.0))
    odd_p, odd_t = p[..., :31], t[..., :31]
    for space, kw in (("stored", {}), ("srgb", dict(minmax=mm))):
        _raises_value_error(metrics.ssim, odd_p, odd_t, space=space, **kw)                          # odd W on the sphere
        _raises_value_error(metrics.ssim, p, t, space=space, sphere=False, weight=torch.ones(16, 1), **kw)  # weight in planar mode
        _raises_value_error(metrics.ssim, p[:, :, :4], t[:, :, :4], space=space, **kw)              # H < 5 on the sphere
        _raises_value_error(metrics.ssim, p[:, :, :10], t[:, :, :10], space=space, sphere=False, **kw)  # no whole window
        _raises_value_error(metrics.ssim, p, t, space=space, L=0.0, **kw)
    _raises_value_error(metrics.ssim, p, t, space="linear", minmax=mm)                              # linear needs L
    _raises_value_error(metrics.psnr, p, t, space="stored", peak="max")
    _raises_value_error(metrics.psnr, p, t, space="stored", peak=-1.0)
    _raises_value_error(metrics.score_maps, odd_p, odd_t)
    _raises_value_error(metrics.score_maps, p, t, mask=torch.ones(1, 100, 3))
    _raises_value_error(metrics.score_maps, p, t, mask=2 * torch.ones(16, 32))
    _raises_value_error(metrics.score_maps, p, t, mask=torch.full((16, 32), float("nan")))   # a NaN is not in [0, 1]
    _raises_value_error(ops.pair_stats, p, t, weight=torch.full((16, 1), float("nan")))
    _raises_value_error(metrics.equivariance_error, torch.nn.Linear(1, 1), [0], torch.eye(3) * 1.1)


def test_weights_are_checked_on_every_call_unless_the_caller_vouches_for_them():
    """no memo: a negative weight raises whatever was checked before it, and check_weight=False does not look at the weight"""
    from reni_amd import _lib, ops
    p, t = (torch.from_numpy(x) for x in pair_maps(2, 16, 32, 1))
    for _ in range(3):  # a fresh tensor each time, freed and reallocated at will
        good = torch.ones(16, 32) * 0.5
        with pytest.raises(_lib.RENILibraryError):
            ops.pair_stats(p, t, good)
        del good
        bad = -torch.ones(16, 32) * 0.5
        for fn in (ops.pair_stats, ops.ssim):
            with pytest.raises(ValueError):
                fn(p, t, bad)
            with pytest.raises(_lib.RENILibraryError):  # not looked at: the call gets as far as the device check
                fn(p, t, bad, check_weight=False)
        del bad

    class Spy(torch.Tensor):
        looked = 0

        @classmethod
        def __torch_function__(cls, func, types, args=(), kwargs=None):
            if func in (torch.Tensor.__lt__, torch.Tensor.lt, torch.lt, torch.Tensor.__ge__, torch.Tensor.ge, torch.ge,
                        torch.Tensor.any, torch.Tensor.all, torch.Tensor.min):
                Spy.looked += 1
            return super().__torch_function__(func, types, args, kwargs or {})

    w = torch.ones(16, 32).as_subclass(Spy)
    for fn in (ops.pair_stats, ops.ssim):
        Spy.looked = 0
        with pytest.raises(_lib.RENILibraryError):
            fn(p, t, w, check_weight=False)
        assert Spy.looked == 0, fn.__name__
        with pytest.raises(_lib.RENILibraryError):
            fn(p, t, w)
        assert Spy.looked >= 1, fn.__name__


def test_metrics_have_no_cpu_fallback():
    from reni_amd import _lib, metrics, ops
    from reni_amd.data import SyntheticEnvMapDataset
    from reni_amd.models import RENIAutoDecoder
    p, t = (torch.from_numpy(x) for x in pair_maps(2, 16, 32, 1))
    w = metrics.solid_angle_weight(16)
    for call in (lambda: ops.pair_stats(p, t), lambda: ops.pair_stats(p, t, w, "linear", O.MINMAX),
                 lambda: ops.ssim(p, t, w, L=2.0), lambda: ops.ssim(p, t, None, L=2.0, sphere=False),
                 lambda: metrics.weighted_mse(p, t), lambda: metrics.mae(p, t, weight=w), lambda: metrics.cosine(p, t),
                 lambda: metrics.psnr(p, t, minmax=O.MINMAX), lambda: metrics.ssim(p, t, minmax=O.MINMAX, weight=w),
                 lambda: metrics.score_maps(p, t), lambda: metrics.score_maps(p, t, O.MINMAX, mask=torch.ones(16, 32)),
                 lambda: metrics.score_maps(p.permute(0, 2, 3, 1).reshape(2, -1, 3), t, O.MINMAX)):
        with pytest.raises(_lib.RENILibraryError):
            call()
    model = RENIAutoDecoder(2, 9, "SO2", 64, 3, 3, True, "tanh", 30, 30, False)
    with pytest.raises(_lib.RENILibraryError):
        metrics.evaluate(model, SyntheticEnvMapDataset(2, 16, 32))
    with pytest.raises(_lib.RENILibraryError):
        metrics.equivariance_error(model, [0, 1], torch.eye(3), width=32)


def test_lightning_module_has_evaluate():
    import inspect
    from reni_amd.lightning_module import RENI
    sig = inspect.signature(RENI.evaluate)
    assert list(sig.parameters) == ["self", "idx", "diffuse"] and sig.parameters["diffuse"].default is False


# ------------------------------------------------------------------------------------------ 3. build: ISA audit, header, C ABI
def test_metrics_translation_unit_isa_audit():
    """reni_tu_metrics.hip with build.sh's flags: three instances of each kernel, no hazard behind its exp / pow / rcp chains,
    no scratch, no float atomics, LDS small enough for two workgroups on a CU"""
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "metrics.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_metrics.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    assert len(set(re.findall(r"^(_Z\w*k_pair_stats\w*):", text, re.M))) == 3
    assert len(set(re.findall(r"^(_Z\w*k_ssim\w*):", text, re.M))) == 3
    assert len(set(re.findall(r"^(_Z\w*k_finish\w*):", text, re.M))) == 2
    assert isa_audit.violations(text) == []
    assert isa_audit.valu_to_mfma(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text and "global_atomic" not in text and "ds_add_f32" not in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 8 and all(int(x) == 0 for x in sizes)
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text)]
    assert len(lds) == 8 and max(lds) * 2 <= 160 * 1024
    assert "v_exp_f32" in text and "v_rcp_f32" in text and "v_sqrt_f32" in text


def test_header_declares_the_functions_and_the_bindings_constants():
    from reni_amd import _lib
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    for name in ("reni_pair_stats_workspace_bytes", "reni_pair_stats", "reni_ssim"):
        assert re.search(r"^(int|size_t) " + name + r"\(", header, re.M) and name in _lib.EXPORTS
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(RENI_(?:SPACE|SSIM)_[A-Z]+)\s+(\d+)", header)}
    assert defs == {"RENI_SPACE_STORED": _lib.SPACE["stored"], "RENI_SPACE_LINEAR": _lib.SPACE["linear"],
                    "RENI_SPACE_SRGB": _lib.SPACE["srgb"], "RENI_SSIM_SPHERE": _lib.SSIM_MODE["sphere"],
                    "RENI_SSIM_PLANAR": _lib.SSIM_MODE["planar"]}
    assert len(set(_lib.SPACE.values())) == 3 and len(set(_lib.SSIM_MODE.values())) == 2
    build = open(os.path.join(ROOT, "reni_amd", "csrc", "build.sh")).read()
    assert re.search(r"for tu in [^;]*\bmetrics\b", build) and "_build/metrics.o" in build


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    from reni_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 255) & ~255
    st4 = (ctypes.c_int64 * 4)(3 * 16 * 32, 16 * 32, 32, 1)
    st3 = (ctypes.c_int64 * 3)(0, 1, 0)
    need = lib.reni_pair_stats_workspace_bytes(1, 16, 32)
    assert need >= 8 * 4 and lib.reni_pair_stats_workspace_bytes(0, 16, 32) == 0 and lib.reni_pair_stats_workspace_bytes(1, 0, 32) == 0
    assert lib.reni_pair_stats_workspace_bytes(3, 512, 1024) >= 3 * (512 * 1024 // 2048) * 8 * 4

    def stats(B=1, H=16, W=32, pred=p, ps=st4, target=p, ts=st4, weight=None, wst=None, space=0, m0=-1.0, m1=1.0, expo=None,
              out=p, ws=p, nws=4096):
        return lib.reni_pair_stats(B, H, W, pred, ps, target, ts, weight, wst, space, m0, m1, expo, out, ws, nws, None)

    def ssim(B=1, H=16, W=32, pred=p, ps=st4, target=p, ts=st4, weight=None, wst=None, space=0, m0=-1.0, m1=1.0, expo=None,
             L=1.0, mode=0, out=p, smap=None, ws=p, nws=4096):
        return lib.reni_ssim(B, H, W, pred, ps, target, ts, weight, wst, space, m0, m1, expo, L, mode, out, smap, ws, nws, None)

    neg4 = (ctypes.c_int64 * 4)(3 * 16 * 32, 16 * 32, -32, 1)
    neg3 = (ctypes.c_int64 * 3)(0, -1, 0)
    common = (dict(B=0), dict(B=1 << 16), dict(H=0), dict(W=0), dict(H=1 << 15, W=1 << 15), dict(pred=None), dict(target=None),
              dict(ps=None), dict(ts=None), dict(out=None), dict(ps=neg4), dict(ts=neg4), dict(weight=p, wst=None),
              dict(weight=p, wst=neg3), dict(space=3), dict(space=-1), dict(space=1, m0=1.0, m1=1.0), dict(space=2),
              dict(space=2, m0=2.0, m1=1.0, expo=p))
    for fn, tag in ((stats, b"pair stats:"), (ssim, b"ssim:")):
        for kw in common:
            assert fn(**kw) == -1, (tag, kw)
            assert lib.reni_last_error().startswith(tag), (tag, kw, lib.reni_last_error())
        for kw in (dict(ws=None), dict(nws=4), dict(ws=p + 4)):
            assert fn(**kw) == -2, (tag, kw)
            assert b"workspace" in lib.reni_last_error()
    for kw in (dict(W=31), dict(H=4), dict(mode=2), dict(mode=-1), dict(L=0.0), dict(L=-1.0), dict(L=float("nan")),
               dict(mode=1, weight=p, wst=st3), dict(mode=1, H=10), dict(mode=1, W=10)):
        assert ssim(**kw) == -1, kw
        assert lib.reni_last_error().startswith(b"ssim:")
    assert b"even" in (ssim(W=31), lib.reni_last_error())[1]
    assert b"weight must be NULL" in (ssim(mode=1, weight=p, wst=st3), lib.reni_last_error())[1]
