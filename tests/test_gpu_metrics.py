"""GPU tests of the map scores (reni_tu_metrics.hip through ops.pair_stats / ops.ssim and reni_amd/metrics.py) against the
float64 oracles and the error budget of tests/test_metrics_cpu.py.

Every case prints its largest err / budget (the budget's constants are 4 x what a float32 restatement in numpy shows, so
about 0.25 is expected).  Measured on one MI355X, largest err / budget over every space, weight and mode of a size:

    size          pair_stats   ssim mean   ssim map (per pixel)
    16 x 32         0.159        0.027        0.250
    64 x 128        0.159        0.017        0.219
    128 x 256       0.179        0.010        0.245
    512 x 1024      0.160        0.007        0.276

Tie to reni_unnormalise_srgb: entry 6 0.004, entry 7 0.003 of the budget.  Rolled pairs: at most 0.006 of twice the budget.
evaluate against the oracle forward: at most 0.049 of budget + sensitivity (psnr_srgb_hidden); diffuse_psnr 0.004.
The run's output is kept as profiles/r07_gpu_metrics_tests.log.  profiles/tools/bench_metrics.py, same GPU: score_maps with a
mask and minmax takes 1.92 ms for 64 maps at 128 x 256 and 6.28 ms for 16 maps at 512 x 1024, the torch composition 3.57 ms and
14.60 ms (medians; DESIGN.md 4.6d, profiles/r07_metrics.md).
"""
import math

import numpy as np
import pytest
import torch

from oracle import reni_oracle as O
from reni_amd import metrics  # noqa: F401  (at import: without the module nothing in this file has a subject)
from tests.test_metrics_cpu import (EPS32, K_MAP, SUM_U, np_map, np_pair_stats, np_ssim_map, pair_maps, sin_rows, ssim_budget, ssim_mean,
                                    stats_budget, weight_cases)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SPACES = ("stored", "linear", "srgb")
MM = O.MINMAX


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _ssim_L(space, target):
    return {"stored": 2.0, "linear": float(np_map(target, "linear", MM, None).max()), "srgb": 1.0}[space]


# ------------------------------------------------------------------------------------------ 1. parity with the oracle
@pytest.mark.parametrize("size", [(16, 32), (64, 128), (128, 256), (512, 1024)])
def test_pair_stats_and_ssim_against_the_float64_oracle(size, golden):
    from reni_amd import metrics, ops
    H, W = size
    B = 3
    pred, target = pair_maps(B, H, W, H + W)
    p, t = _t(pred), _t(target)
    expo_t = metrics.exposure(t, MM)
    expo = expo_t.cpu().numpy()
    weights = weight_cases(H, W, golden)
    assert len(weights) >= 7
    worst = {"stats": 0.0, "ssim": 0.0, "map": 0.0}
    for space in SPACES:
        L = _ssim_L(space, target)
        for wname, w in weights:
            wt = _t(w)
            if wname == "sin":
                wt = wt.reshape(H, 1)  # sin(phi) per row, broadcast by the kernel through strides {0, 1, 0}
                assert torch.broadcast_to(wt, (B, H, W)).stride() == (0, 1, 0)
            got = ops.pair_stats(p, t, wt, space, MM, expo_t).cpu().numpy().astype(np.float64)
            ref = np_pair_stats(pred, target, w, space, MM, expo)
            bud = stats_budget(pred, target, w, space, MM, expo)
            err = np.abs(got - ref)
            exact = bud == 0
            assert (err[exact] == 0).all(), (space, wname)
            ratio = float((err[~exact] / bud[~exact]).max())
            print(f"{H}x{W} {space} {wname}: pair_stats largest err / budget {ratio:.3f}")
            worst["stats"] = max(worst["stats"], ratio)
            assert ratio <= 1.0, (space, wname, (err / np.maximum(bud, 1e-300)).max(0))
        for sphere in (True, False):
            smap, kappa = np_ssim_map(pred, target, space, MM, expo, L, sphere, with_kappa=True)
            checked_map = False
            for wname, w in weights if sphere else weights[:1]:
                wt = _t(w)
                pix, img = ssim_budget(kappa, w, space, sphere)
                if not checked_map:
                    mean, gmap = ops.ssim(p, t, wt, space, MM, expo_t, L, sphere, return_map=True)
                    gmap = gmap.cpu().numpy().astype(np.float64)
                    if sphere:
                        r_map = float((np.abs(gmap - smap) / pix).max())  # every pixel
                    else:
                        inner = (slice(None), slice(5, H - 5), slice(5, W - 5))
                        r_map = float((np.abs(gmap - smap)[inner] / pix[inner]).max())
                        border = np.ones((H, W), bool)
                        border[5:H - 5, 5:W - 5] = False
                        assert not gmap[:, border].any()  # the border of the planar map is zero
                    worst["map"] = max(worst["map"], r_map)
                    assert r_map <= 1.0, (space, sphere, r_map)
                    checked_map = True
                else:
                    mean = ops.ssim(p, t, wt, space, MM, expo_t, L, sphere)
                r_img = float((np.abs(mean.cpu().numpy().astype(np.float64) - ssim_mean(smap, w, sphere)) / img).max())
                print(f"{H}x{W} {space} {'sphere' if sphere else 'planar'} {wname}: ssim largest err / budget {r_img:.3f}"
                      f" (map {r_map:.3f})")
                worst["ssim"] = max(worst["ssim"], r_img)
                assert r_img <= 1.0, (space, sphere, wname)
    print(f"{H}x{W}: largest err / budget: pair_stats {worst['stats']:.3f}, ssim mean {worst['ssim']:.3f}, ssim map {worst['map']:.3f}")


# ------------------------------------------------------------------------------------------ 2. bit equality
def test_same_bits_across_calls_batches_and_layouts():
    from reni_amd import metrics, ops
    H, W, B = 64, 128, 4
    pred, target = pair_maps(B, H, W, 21)
    p, t = _t(pred), _t(target)
    expo = metrics.exposure(t, MM)
    w = metrics.solid_angle_weight(H, DEV)
    p_out = p.permute(0, 2, 3, 1).reshape(B, H * W, 3).contiguous()  # the model-output layout [B, P, 3], read in place
    t_out = t.permute(0, 2, 3, 1).reshape(B, H * W, 3).contiguous()
    for space in SPACES:
        full = ops.pair_stats(p, t, w, space, MM, expo)
        assert full.shape == (B, 8) and full.dtype == torch.float32
        assert torch.equal(full, ops.pair_stats(p, t, w, space, MM, expo))
        s_full, m_full = ops.ssim(p, t, w, space, MM, expo, 2.0, True, return_map=True)
        s2, m2 = ops.ssim(p, t, w, space, MM, expo, 2.0, True, return_map=True)
        assert torch.equal(s_full, s2) and torch.equal(m_full, m2)
        pl_full = ops.ssim(p, t, None, space, MM, expo, 2.0, False)
        for n in (0, 2, 3):
            e = expo[n:n + 1]
            assert torch.equal(ops.pair_stats(p[n:n + 1], t[n:n + 1], w, space, MM, e)[0], full[n])
            assert torch.equal(ops.ssim(p[n:n + 1], t[n:n + 1], w, space, MM, e, 2.0)[0], s_full[n])
            assert torch.equal(ops.ssim(p[n:n + 1], t[n:n + 1], None, space, MM, e, 2.0, False)[0], pl_full[n])
        assert torch.equal(ops.pair_stats(p_out, t_out, w, space, MM, expo, size=(H, W)), full)
        assert torch.equal(ops.pair_stats(p_out, t, w, space, MM, expo), full)  # mixed layouts, the size from the target
        s3, m3 = ops.ssim(p_out, t_out, w, space, MM, expo, 2.0, True, return_map=True, size=(H, W))
        assert torch.equal(s3, s_full) and torch.equal(m3, m_full)
        assert torch.equal(ops.ssim(p_out, t, None, space, MM, expo, 2.0, False), pl_full)


# ------------------------------------------------------------------------------------------ 3. tie to reni_unnormalise_srgb
def test_srgb_sums_are_those_of_unnormalise_srgb_and_a_map_scores_perfectly_against_itself():
    from reni_amd import metrics, ops
    H, W, B = 64, 128, 3
    pred, target = pair_maps(B, H, W, 33)
    p, t = _t(pred), _t(target)
    expo = metrics.exposure(t, MM)
    w = metrics.solid_angle_weight(H, DEV)
    srgb = ops.unnormalise_srgb(t, MM).double()  # the existing kernel: its own quantile, the same expressions
    wd = w.double().reshape(1, 1, H, 1)
    got = ops.pair_stats(p, t, w, "srgb", MM, expo).double().cpu().numpy()
    bud = stats_budget(pred, target, sin_rows(H)[:, None].astype(np.float32), "srgb", MM, expo.cpu().numpy())
    s6 = (wd * srgb * srgb).sum((1, 2, 3)).cpu().numpy()
    s7 = (wd * srgb).sum((1, 2, 3)).cpu().numpy()
    r6, r7 = np.abs(got[:, 6] - s6) / bud[:, 6], np.abs(got[:, 7] - s7) / bud[:, 7]
    print(f"entry 6 err / budget {r6.max():.3f}, entry 7 {r7.max():.3f}")
    assert r6.max() <= 1.0 and r7.max() <= 1.0
    for space in SPACES:
        same = ops.pair_stats(t, t, w, space, MM, expo)
        assert float(same[:, 1].abs().max()) == 0.0 and float(same[:, 2].abs().max()) == 0.0  # SSE = 0 exactly
        for sphere in (True, False):
            L = _ssim_L(space, target)
            _, kappa = np_ssim_map(target, target, space, MM, expo.cpu().numpy(), L, sphere, with_kappa=True)
            wn = sin_rows(H)[:, None].astype(np.float32) if sphere else None
            pix, img = ssim_budget(kappa, wn, space, sphere)
            mean, smap = ops.ssim(t, t, w if sphere else None, space, MM, expo, L, sphere, return_map=True)
            assert (np.abs(mean.cpu().numpy().astype(np.float64) - 1.0) <= img).all(), (space, sphere)
            inner = (slice(None),) + ((slice(None), slice(None)) if sphere else (slice(5, H - 5), slice(5, W - 5)))
            assert (np.abs(smap.cpu().numpy().astype(np.float64) - 1.0)[inner] <= pix[inner]).all(), (space, sphere)


# ------------------------------------------------------------------------------------------ 4. the seen / hidden split
def test_seen_plus_hidden_is_the_whole(golden):
    from reni_amd import metrics, ops
    from reni_amd.utils import mask_from_array
    H, W, B = 64, 128, 3
    pred, target = pair_maps(B, H, W, 44)
    p, t = _t(pred), _t(target)
    expo = metrics.exposure(t, MM)
    base = metrics.solid_angle_weight(H, DEV)
    for name, m in sorted(golden("masks.npz").items()):
        mask = mask_from_array(W, m).to(DEV)  # [1, P, 3]
        m2 = mask[0, :, 0].reshape(H, W)
        for space in SPACES:
            whole = ops.pair_stats(p, t, base, space, MM, expo).double()
            seen = ops.pair_stats(p, t, m2 * base, space, MM, expo).double()
            hidden = ops.pair_stats(p, t, (1 - m2) * base, space, MM, expo).double()
            for e in (0, 1, 2, 6):  # sums of non-negative terms: 64 u relative
                assert float(((seen[:, e] + hidden[:, e] - whole[:, e]).abs() / whole[:, e]).max()) <= 64 * EPS32, (name, space, e)
            mags = np_pair_stats(np.abs(pred), np.abs(target), sin_rows(H)[:, None], space, MM, expo.cpu().numpy())
            assert float(((seen[:, 3] + hidden[:, 3] - whole[:, 3]).abs() / whole[:, 0]).max()) <= 64 * EPS32  # |cos| <= 1
            if space == "stored":  # a signed sum: relative to the sum of the magnitudes
                scale = torch.from_numpy(mags[:, 7]).to(DEV)
            else:
                scale = whole[:, 7].abs()
            assert float(((seen[:, 7] + hidden[:, 7] - whole[:, 7]).abs() / scale).max()) <= 64 * EPS32
            assert torch.equal(torch.maximum(seen[:, 4], hidden[:, 4]), whole[:, 4])
            assert torch.equal(torch.minimum(seen[:, 5], hidden[:, 5]), whole[:, 5])
            assert bool((seen[:, 4] <= whole[:, 4]).all()) and bool((seen[:, 5] >= whole[:, 5]).all())
        scores = metrics.score_maps(p, t, MM, mask)
        assert set(scores) == {k + s for k in metrics.SCORES for s in ("", "_seen", "_hidden")}
        assert all(v.shape == (B,) and bool(torch.isfinite(v).all()) for v in scores.values())
        mse = {s: scores["wmse_stored" + s].double() for s in ("", "_seen", "_hidden")}
        ws = ops.pair_stats(p, t, m2 * base).double()[:, 0] / ops.pair_stats(p, t, base).double()[:, 0]
        assert float((ws * mse["_seen"] + (1 - ws) * mse["_hidden"] - mse[""]).abs().max()) <= 1e-5 * float(mse[""].max())
    plain = metrics.score_maps(p, t)
    assert set(plain) == {"wmse_stored", "cosine_stored"}


# ------------------------------------------------------------------------------------------ 5. invariance on the device
def test_sphere_ssim_does_not_change_when_both_maps_are_rolled():
    from reni_amd import metrics, ops
    H, W, B = 64, 128, 3
    pred, target = pair_maps(B, H, W, 55)
    p, t = _t(pred), _t(target)
    expo = metrics.exposure(t, MM)
    w = metrics.solid_angle_weight(H, DEV)
    wn = sin_rows(H)[:, None].astype(np.float32)
    for space in SPACES:
        L = _ssim_L(space, target)
        _, kappa = np_ssim_map(pred, target, space, MM, expo.cpu().numpy(), L, True, with_kappa=True)
        _, img = ssim_budget(kappa, wn, space, True)
        base = ops.ssim(p, t, w, space, MM, expo, L).double().cpu().numpy()
        for k in (1, 7, W // 2 + 3):
            rolled = ops.ssim(torch.roll(p, k, -1), torch.roll(t, k, -1), w, space, MM, expo, L).double().cpu().numpy()
            r = float((np.abs(rolled - base) / (2 * img)).max())
            print(f"{space} roll {k}: |ssim - ssim rolled| / (2 budget) {r:.3f}")
            assert r <= 1.0, (space, k)


# ------------------------------------------------------------------------------------------ 6. end to end
def _np_scores(out, target, minmax, weights):
    """score_maps from the numpy oracle: out, target [B, 3, H, W]; weights {suffix: [H, W] float32}.  Returns
    ({name: [B]}, {name: bound [B] on the fp32 kernels' error}) -- the bound is the budget propagated through the score"""
    B, _, H, W = out.shape
    expo = np.quantile(np.quantile(np.quantile(np_map(target, "linear", minmax, None), 0.98, axis=1), 0.98, axis=1), 0.98,
                       axis=1).astype(np.float32)
    scores, bounds = {}, {}
    smap, kappa = np_ssim_map(out, target, "srgb", minmax, expo, 1.0, True, with_kappa=True)
    peak = np_pair_stats(out, target, weights[""], "linear", minmax, expo)[:, 4]
    for suffix, w in weights.items():
        s = np_pair_stats(out, target, w, "stored")
        b = stats_budget(out, target, w, "stored")
        scores["wmse_stored" + suffix] = s[:, 1] / (3 * s[:, 0])
        bounds["wmse_stored" + suffix] = (b[:, 1] / s[:, 1] + b[:, 0] / s[:, 0] + 4 * EPS32) * scores["wmse_stored" + suffix]
        scores["cosine_stored" + suffix] = s[:, 3] / s[:, 0]
        bounds["cosine_stored" + suffix] = b[:, 3] / s[:, 0] + (b[:, 0] / s[:, 0] + 4 * EPS32)
        for space in ("linear", "srgb"):
            s = np_pair_stats(out, target, w, space, minmax, expo)
            b = stats_budget(out, target, w, space, minmax, expo)
            pk = peak if space == "linear" else np.ones(B)
            scores["psnr_" + space + suffix] = 10 * np.log10(pk * pk / (s[:, 1] / (3 * s[:, 0])))
            rel = b[:, 1] / s[:, 1] + b[:, 0] / s[:, 0] + (2 * 112 * EPS32 if space == "linear" else 0) + 16 * EPS32
            bounds["psnr_" + space + suffix] = 10 / math.log(10) * rel
        scores["ssim_srgb" + suffix] = ssim_mean(smap, w, True)
        bounds["ssim_srgb" + suffix] = ssim_budget(kappa, w, "srgb", True)[1]
    return scores, bounds, expo


def _sensitivity(out, target, minmax, weights, expo, delta):
    """{name: [B]}: the largest first-order change of every score when each output value moves by at most `delta`:
    delta x the l1 norm of the score's gradient, from a float64 torch restatement of the definitions."""
    import torch.nn.functional as Fn
    x = torch.from_numpy(np.asarray(out, np.float64)).requires_grad_(True)
    t = torch.from_numpy(np.asarray(target, np.float64))
    B, _, H, W = x.shape
    m0, m1 = minmax
    q = torch.from_numpy(np.asarray(expo, np.float64)).reshape(B, 1, 1, 1)

    def lin(v):
        return torch.exp(0.5 * (v + 1) * (m1 - m0) + m0)

    def srgb(v):
        y = torch.clamp(lin(v) / q, 0.0, 1.0)
        return torch.where(y <= 0.0031308, 12.92 * y, 1.055 * torch.clamp(y, min=1e-30) ** (1 / 2.4) - 0.055)

    def pad(v):
        i = np.arange(-5, H + 5)[:, None]
        j = np.arange(-5, W + 5)[None, :]
        over = (i < 0) | (i >= H)
        ii = np.where(i < 0, -1 - i, np.where(i >= H, 2 * H - 1 - i, i))
        jj = np.mod(np.where(over, j + W // 2, j), W)
        return v[..., torch.from_numpy(np.broadcast_to(ii, jj.shape).copy()), torch.from_numpy(jj)]

    g = torch.from_numpy(np.exp(-(np.arange(11) - 5.0) ** 2 / 4.5))
    g = g / g.sum()
    k2 = torch.outer(g, g).reshape(1, 1, 11, 11)

    def win(v):
        return Fn.conv2d(v.reshape(B * 3, 1, H + 10, W + 10), k2).reshape(B, 3, H, W)

    ps, ts = pad(srgb(x)), pad(srgb(t))
    mp, mt = win(ps), win(ts)
    vp, vt, cov = win(ps * ps) - mp * mp, win(ts * ts) - mt * mt, win(ps * ts) - mp * mt
    smap = (((2 * mp * mt + 1e-4) * (2 * cov + 9e-4)) / ((mp * mp + mt * mt + 1e-4) * (vp + vt + 9e-4))).mean(1)
    peak = lin(t).amax((1, 2, 3))
    scores = {}
    for suffix, w in weights.items():
        wt = torch.from_numpy(np.broadcast_to(np.asarray(w, np.float64), (H, W)).copy())
        sw = wt.sum()
        scores["wmse_stored" + suffix] = (wt * ((x - t) ** 2).sum(1)).sum((1, 2)) / (3 * sw)
        scores["cosine_stored" + suffix] = (wt * Fn.cosine_similarity(x, t, dim=1, eps=1e-20)).sum((1, 2)) / sw
        scores["psnr_linear" + suffix] = 10 * torch.log10(peak ** 2 / ((wt * ((lin(x) - lin(t)) ** 2).sum(1)).sum((1, 2)) / (3 * sw)))
        scores["psnr_srgb" + suffix] = 10 * torch.log10(1.0 / ((wt * ((srgb(x) - srgb(t)) ** 2).sum(1)).sum((1, 2)) / (3 * sw)))
        scores["ssim_srgb" + suffix] = (wt * smap).sum((1, 2)) / sw
    out_s = {}
    for name, v in scores.items():
        (gr,) = torch.autograd.grad(v.sum(), x, retain_graph=True)
        out_s[name] = delta * gr.abs().sum((1, 2, 3)).numpy()  # (image b's score depends on image b's output alone)
    return {k: v.detach().numpy() for k, v in scores.items()}, out_s


def _smoke_model():
    from reni_amd.models import RENIAutoDecoder
    torch.manual_seed(0)
    model = RENIAutoDecoder(2, 9, "SO2", 64, 3, 3, True, "tanh", 30, 30, False)
    spec = O.DecoderSpec(9, "SO2", 64, 3, 3, True, "tanh")
    params = {"net." + k: v.detach().clone() for k, v in model.net.state_dict().items()}
    Z = model.Z.detach().clone()
    model.set_compute_dtype("f32").to(DEV)
    return model, spec, params, Z


OUT_TOL = 1e-5  # smoke()'s tolerance on the fp32 forward against the oracle


def _check_table(table, ref, bounds, sens, what):
    assert set(table) >= set(ref), set(ref) - set(table)
    for name in sorted(ref):
        got = table[name].double().cpu().numpy()
        tol = bounds[name] + sens[name]
        err = np.abs(got - ref[name])
        print(f"{what} {name}: {got} oracle {ref[name]} err / tol {float((err / tol).max()):.3f} (budget share {float((bounds[name] / tol).min()):.2f})")
        assert (err <= tol).all(), (what, name, err, tol)


@pytest.mark.parametrize("masked", [False, True])
def test_evaluate_is_the_oracle_forward_scored_by_the_numpy_oracle(masked, golden):
    from reni_amd import metrics
    from reni_amd.data import SyntheticEnvMapDataset
    from reni_amd.utils import mask_from_array
    H, W = 16, 32
    model, spec, params, Z = _smoke_model()
    ds = SyntheticEnvMapDataset(2, H, W)
    D = O.get_directions(W)
    out = O.reni_forward(spec, params, Z, D.expand(2, -1, 3)).double().numpy().reshape(2, H, W, 3).transpose(0, 3, 1, 2)
    target = torch.stack([ds[i][0] for i in range(2)]).numpy()
    sin = sin_rows(H)[:, None].astype(np.float32)
    weights = {"": np.broadcast_to(sin, (H, W))}
    mask = None
    if masked:
        mask = mask_from_array(W, golden("masks.npz")["Mask-2.png"])
        m2 = mask[0, :, 0].reshape(H, W).numpy()
        weights["_seen"] = (m2 * sin).astype(np.float32)
        weights["_hidden"] = ((1 - m2) * sin).astype(np.float32)
    ref, bounds, expo = _np_scores(out, target, MM, weights)
    ref64, sens = _sensitivity(out, target, MM, weights, expo, OUT_TOL)
    for name in ref:  # the torch restatement the sensitivities come from is the same function
        assert np.abs(ref64[name] - ref[name]).max() <= 1e-9 * max(1.0, np.abs(ref[name]).max()), name
    table, means = metrics.evaluate(model, ds, mask=mask)
    assert all(v.shape == (2,) for v in table.values()) and set(means) == set(table)
    _check_table(table, ref, bounds, sens, "evaluate" + (" masked" if masked else ""))
    for k, v in means.items():
        assert abs(float(v) - float(table[k].mean())) <= 1e-6 * max(1.0, abs(float(v)))
    one, _ = metrics.evaluate(model, ds, idx=[1], batch_size=1, mask=mask)  # an image scores the same alone
    assert all(torch.equal(one[k][0], table[k][1]) for k in table)


def test_evaluate_diffuse_and_the_lightning_module(golden):
    import types
    from reni_amd import metrics
    from reni_amd.data import SyntheticEnvMapDataset
    from reni_amd.lightning_module import RENI
    from tests.test_diffuse_cpu import np_clamped_cosine
    from reni_amd.baselines import reni_grid_weights
    H, W = 16, 32
    model, spec, params, Z = _smoke_model()
    ds = SyntheticEnvMapDataset(2, H, W)
    D = O.get_directions(W)
    out = O.reni_forward(spec, params, Z, D.expand(2, -1, 3)).double().numpy().reshape(2, H * W, 3)
    target = torch.stack([ds[i][0] for i in range(2)]).numpy().transpose(0, 2, 3, 1).reshape(2, H * W, 3)
    m0, m1 = MM
    lin_o, lin_t = (np.exp(0.5 * (v.astype(np.float64) + 1) * (m1 - m0) + m0) for v in (out, target))
    dirs = D[0].double().numpy()
    sa = np.asarray(reni_grid_weights(W), np.float64).reshape(-1)
    irr_o = np_clamped_cosine(lin_o, dirs, sa, dirs)  # (np_diffuse_map is this function on the reference's grid; irradiance_map
    irr_t = np_clamped_cosine(lin_t, dirs, sa, dirs)  #  works on RENI's own, so the oracle is called with that grid)
    sin = np.broadcast_to(sin_rows(H)[:, None].astype(np.float32), (H, W))

    def as_img(v):
        return v.reshape(2, H, W, 3).transpose(0, 3, 1, 2)

    s = np_pair_stats(as_img(irr_o), as_img(irr_t), sin)
    want = 10 * np.log10(s[:, 4] ** 2 / (s[:, 1] / (3 * s[:, 0])))
    # budget: the two irradiance maps reach reni_pair_stats as fp32 numbers with a relative error of (K_MAP[linear] + SUM_U) u -- the
    # un-normalised radiance's k u, then a sum of non-negative terms -- which is stats_budget's "mapped value" with that k
    bud = stats_budget(as_img(irr_o), as_img(irr_t), sin, "stored", k=K_MAP["linear"] + SUM_U)
    budget = 10 / math.log(10) * (bud[:, 1] / s[:, 1] + bud[:, 0] / s[:, 0] + 2 * bud[:, 4] / s[:, 4] + 16 * EPS32)
    # sensitivity: |d score / d output|_1 x the output tolerance, through the float64 chain output -> radiance -> irradiance -> PSNR
    x = torch.from_numpy(out).requires_grad_(True)
    A = torch.from_numpy(np.maximum(0.0, dirs @ dirs.T) * sa / np.pi)
    io = torch.einsum("pq,nqc->npc", A, torch.exp(0.5 * (x + 1) * (m1 - m0) + m0))
    it = torch.from_numpy(irr_t)
    wt = torch.from_numpy(np.ascontiguousarray(sin, dtype=np.float64).reshape(-1))
    mse = (wt[None, :, None] * (io - it) ** 2).sum((1, 2)) / (3 * wt.sum())
    score = 10 * torch.log10(it.amax((1, 2)) ** 2 / mse)
    assert np.abs(score.detach().numpy() - want).max() <= 1e-9
    (gr,) = torch.autograd.grad(score.sum(), x)
    tol = budget + OUT_TOL * gr.abs().sum((1, 2)).numpy()
    table, _ = metrics.evaluate(model, ds, diffuse=True)
    got = table["diffuse_psnr"].double().cpu().numpy()
    print(f"diffuse_psnr {got} oracle {want} err / tol {np.abs(got - want) / tol}")
    assert (np.abs(got - want) <= tol).all()
    plain, _ = metrics.evaluate(model, ds)
    assert all(torch.equal(plain[k], table[k]) for k in plain)
    # RENI.evaluate: the module's model, dataset and mask
    mod = RENI.__new__(RENI)
    torch.nn.Module.__init__(mod)
    mod.model, mod.dataset, mod.mask = model, ds, None
    t2, m2 = mod.evaluate()
    assert all(torch.equal(t2[k], plain[k]) for k in plain)
    from reni_amd.utils import mask_from_array
    mod.mask = mask_from_array(W, golden("masks.npz")["Mask-2.png"])  # FIT_LATENT's inpainting mask [1, P, 3]
    t4, _ = mod.evaluate()
    masked, _ = metrics.evaluate(model, ds, mask=mod.mask)
    assert set(t4) == {k + sfx for k in metrics.SCORES for sfx in ("", "_seen", "_hidden")}
    assert all(torch.equal(t4[k], masked[k]) for k in masked) and all(torch.equal(t4[k], plain[k]) for k in plain)
    mod.mask = None
    t3, _ = mod.evaluate(idx=[1], diffuse=True)
    assert torch.equal(t3["diffuse_psnr"][0], table["diffuse_psnr"][1])


def test_equivariance_error_of_a_whole_pixel_yaw_is_a_roll():
    from reni_amd import metrics
    from reni_amd.rotation import rotate_latent, rotation_y
    from reni_amd.utils import get_directions
    W = 32
    H = W // 2
    model, _, _, _ = _smoke_model()
    k = 5
    R = rotation_y(k * 2 * math.pi / W)
    got = metrics.equivariance_error(model, [0, 1], R, mode="nearest", width=W, minmax=MM)
    with torch.no_grad():
        D = get_directions(W).to(DEV)
        Zs = model.Z[torch.tensor([0, 1], device=DEV)]
        base = model(Zs, D)
        turned = model(rotate_latent(Zs, R.to(DEV)), D)
        rolled = torch.roll(base.reshape(2, H, W, 3).permute(0, 3, 1, 2), -k, -1)  # rotation_y(k 2 pi / W) rolls by -k
    want = metrics.score_maps(turned, rolled, MM, size=(H, W))
    assert set(got) == set(want) == set(metrics.SCORES)
    for name in want:
        assert torch.equal(got[name], want[name]), name
    print({n: v.tolist() for n, v in got.items()})
    assert float(got["wmse_stored"].max()) <= 1e-8 and float(got["ssim_srgb"].min()) >= 0.999  # an SO2 model is yaw-equivariant
