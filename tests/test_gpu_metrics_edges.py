"""GPU tests of the map scores (reni_tu_metrics.hip through ops.pair_stats / ops.ssim / reni_amd.metrics) and of the light
tables (reni_tu_lights.hip) where their tiles, tails, wraps and carries act: the cases of tests/metrics_edge_cases.py against
the float64 oracles and the unchanged budgets of tests/test_metrics_cpu.py and tests/test_lighting_cpu.py.
tests/test_metrics_edges_cpu.py shows that plain fp32 arithmetic stays within half of the budget at every shape case.

    1. shapes        every tile, chunk and strand boundary of k_pair_stats, k_ssim and k_finish; W < 11; both poles in a window
    2. values        pred is target, constant and black images, pixels of weight 0 that hold a NaN or an infinity, no live
                     pixel, one live pixel, extreme exposures, PSNR of a map against itself, addressing
    3. stores        guard bands around out and map_out through the C entry points, poisoned workspaces
    4. light tables  rows of 4 and 16 tiles, marginals of 2 and 8: the carries of row_scan_d and row_cdf

Each parity test prints its largest err / budget before it asserts (pytest -s or -rA shows them); the run's output is kept as
profiles/gpu_metrics_edges_tests.log."""
import ctypes

import numpy as np
import pytest
import torch

from tests import metrics_edge_cases as E
from tests.test_gpu_baseline_edges import Carved, _workspace
from tests.test_gpu_lighting import _layouts, _np, _table_errors, _test_uniforms
from tests.test_lighting_cpu import np_select, sky_maps
from tests.test_metrics_cpu import EPS32, np_map, ssim_budget

pytestmark = pytest.mark.gpu
MM = E.MM


def _dev():
    return torch.device("cuda")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(_dev())


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _id(shape):
    return f"{shape[0]}x{shape[1]}"


def _mode(sphere):
    return "sphere" if sphere else "planar"


# ---------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("shape", E.PAIR_SHAPES, ids=_id)
def test_pair_stats_edge_shapes_match_float64(shape):
    """1 and 2 pixels, 21 pixels (one chunk, mostly the clamped tail), the chunk boundary 2047 | 2048 | 2049, and nblk = 7, 8, 9,
    17 partials per image through k_finish's eight strands; every entry of every image against the oracle"""
    from reni_amd import ops
    H, W = shape
    pred, target, expo = E.shape_inputs(H, W)
    p, t, q = _t(pred), _t(target), _t(expo)
    worst = 0.0
    for space in E.SPACES:
        for kind in E.WEIGHT_KINDS:
            w = E.weight(kind, H, W)
            got = ops.pair_stats(p, t, _t(w), space, MM, q)
            assert got.shape == (E.B, 8) and got.dtype == torch.float32
            ref, bud = E.stats_reference(pred, target, w, space, expo)
            r = E.stats_ratio(got.cpu().numpy(), ref, bud)
            print(f"{H}x{W} nblk={E.nblk(H, W)} {space} {kind}: pair_stats largest err / budget {r:.3f}")
            worst = max(worst, r)
            assert r <= 1.0, (space, kind, r)
    print(f"{H}x{W}: pair_stats largest err / budget {worst:.3f}")


@pytest.mark.parametrize("sphere,shape", [(True, s) for s in E.SPHERE_SHAPES] + [(False, s) for s in E.PLANAR_SHAPES],
                         ids=lambda v: _mode(v) if isinstance(v, bool) else _id(v))
def test_ssim_edge_shapes_match_float64(sphere, shape):
    """the map at every pixel and the mean of every image, under every weight: partial tiles (rlast / clast), W < 11 (a window
    wraps the row several times), both poles inside one window (H = 5), one-window and one-row planar interiors; the planar
    border is written as 0.  The same shapes run through pair_stats."""
    from reni_amd import ops
    H, W = shape
    pred, target, expo = E.shape_inputs(H, W)
    p, t, q = _t(pred), _t(target), _t(expo)
    worst = {"stats": 0.0, "map": 0.0, "mean": 0.0}
    for space in E.SPACES:
        L = E.ssim_L(space, target)
        smap, kappa = E.ssim_reference(pred, target, space, expo, L, sphere)
        for kind in E.WEIGHT_KINDS if sphere else E.WEIGHT_KINDS[:1]:
            w = E.weight(kind, H, W)
            pix, img = ssim_budget(kappa, w, space, sphere)
            mean, gmap = ops.ssim(p, t, _t(w), space, MM, q, L, sphere, return_map=True)
            assert mean.shape == (E.B,) and gmap.shape == (E.B, H, W)
            r_map = E.map_ratio(gmap.cpu().numpy(), smap, pix, sphere)  # every pixel with a window; the border exactly 0
            r_mean = E.mean_ratio(mean.cpu().numpy(), smap, w, img, sphere)
            assert _same_bits(ops.ssim(p, t, _t(w), space, MM, q, L, sphere), mean)  # with and without the map
            ref, bud = E.stats_reference(pred, target, w, space, expo)
            r_stats = E.stats_ratio(ops.pair_stats(p, t, _t(w), space, MM, q).cpu().numpy(), ref, bud)
            print(f"{_mode(sphere)} {H}x{W} {space} {kind}: largest err / budget: ssim map {r_map:.3f}, mean {r_mean:.3f}, "
                  f"pair_stats {r_stats:.3f}")
            for k, r in (("map", r_map), ("mean", r_mean), ("stats", r_stats)):
                worst[k] = max(worst[k], r)
            assert r_map <= 1.0 and r_mean <= 1.0 and r_stats <= 1.0, (space, kind, r_map, r_mean, r_stats)
    print(f"{_mode(sphere)} {H}x{W}: largest err / budget: ssim map {worst['map']:.3f}, mean {worst['mean']:.3f}, "
          f"pair_stats {worst['stats']:.3f}")


# ---------------------------------------------------------------------------------------------- 2. values
def _check_pair(name, pred, target, expo, space, sphere_modes=(True, False), kinds=("none", "sin", "random")):
    """pair_stats and ssim (map and mean) of one pair in one space against the oracle; returns the largest err / budget"""
    from reni_amd import ops
    H, W = pred.shape[-2:]
    p, t, q = _t(pred), _t(target), _t(expo)
    L = E.ssim_L(space, target)
    worst = 0.0
    for kind in kinds:
        w = E.weight(kind, H, W)
        got = ops.pair_stats(p, t, _t(w), space, MM, q).cpu().numpy()
        assert np.isfinite(got).all(), (name, space, kind, got)
        ref, bud = E.stats_reference(pred, target, w, space, expo)
        worst = max(worst, E.stats_ratio(got, ref, bud))
    for sphere in sphere_modes:
        smap, kappa = E.ssim_reference(pred, target, space, expo, L, sphere)
        for kind in kinds if sphere else ("none",):
            w = E.weight(kind, H, W)
            pix, img = ssim_budget(kappa, w, space, sphere)
            mean, gmap = ops.ssim(p, t, _t(w), space, MM, q, L, sphere, return_map=True)
            assert bool(torch.isfinite(gmap).all()) and bool(torch.isfinite(mean).all()), (name, space, sphere, kind)
            worst = max(worst, E.map_ratio(gmap.cpu().numpy(), smap, pix, sphere), E.mean_ratio(mean.cpu().numpy(), smap, w, img, sphere))
    print(f"{name} {H}x{W} {space}: largest err / budget {worst:.3f}")
    return worst


@pytest.mark.parametrize("shape", [(37, 50), (5, 2), (11, 11)], ids=_id)
def test_a_map_scores_perfectly_against_itself(shape):
    """pred IS target: SSE and SAE are exactly 0, the SSIM map and mean within budget of 1, metrics.psnr +inf and not NaN"""
    from reni_amd import metrics, ops
    H, W = shape
    _, target, expo = E.shape_inputs(H, W)
    t, q = _t(target), _t(expo)
    modes = [s for s in (True, False) if (W % 2 == 0 and H >= 5 if s else min(H, W) >= 11)]
    for space in E.SPACES:
        L = E.ssim_L(space, target)
        for kind in E.WEIGHT_KINDS:
            wt = _t(E.weight(kind, H, W))
            same = ops.pair_stats(t, t, wt, space, MM, q)
            assert bool((same[:, 1] == 0).all()) and bool((same[:, 2] == 0).all()), (space, kind)
            assert bool(torch.isfinite(same).all())
            psnr = metrics.psnr(t, t, space, MM, wt)
            assert bool((psnr == float("inf")).all()), (space, kind, psnr)
        for sphere in modes:
            _, kappa = E.ssim_reference(target, target, space, expo, L, sphere)
            for kind in E.WEIGHT_KINDS if sphere else E.WEIGHT_KINDS[:1]:
                w = E.weight(kind, H, W)
                pix, img = ssim_budget(kappa, w, space, sphere)
                mean, gmap = ops.ssim(t, t, _t(w), space, MM, q, L, sphere, return_map=True)
                r_map = E.map_ratio(gmap.cpu().numpy(), np.where(E.interior(H, W, sphere), 1.0, 0.0)[None], pix, sphere)
                r_mean = float((np.abs(mean.cpu().numpy().astype(np.float64) - 1.0) / img).max())
                print(f"self {_mode(sphere)} {H}x{W} {space} {kind}: |ssim - 1| / budget: map {r_map:.3f}, mean {r_mean:.3f}")
                assert r_map <= 1.0 and r_mean <= 1.0, (space, sphere, kind)


def test_constant_images_give_the_closed_form():
    """two different constants: every window has variance 0, ssim = (2 a b + C1) / (a^2 + b^2 + C1) of the mapped constants
    (tests/test_metrics_cpu.py::test_oracle_ssim_of_constant_images), kappa up to 2.8e3 -- within budget, as is pair_stats"""
    from reni_amd import ops
    H, W = E.VALUE_SHAPE
    for space in E.SPACES:
        pred, target, expo = E.constant_pair(space)
        L = E.ssim_L(space, target)
        want = E.constant_ssim(pred, target, space, expo, L)
        for sphere in (True, False):
            _, kappa = E.ssim_reference(pred, target, space, expo, L, sphere)
            pix, img = ssim_budget(kappa, None, space, sphere)
            mean, gmap = ops.ssim(_t(pred), _t(target), None, space, MM, _t(expo), L, sphere, return_map=True)
            inn = E.interior(H, W, sphere)
            r_map = float((np.abs(gmap.cpu().numpy().astype(np.float64) - want[:, None, None])[:, inn] / pix[:, inn]).max())
            r_mean = float((np.abs(mean.cpu().numpy().astype(np.float64) - want) / img).max())
            print(f"constant {_mode(sphere)} {space}: |ssim - closed form| / budget: map {r_map:.3f}, mean {r_mean:.3f} "
                  f"(kappa {kappa[:, inn].max():.0f})")
            assert r_map <= 1.0 and r_mean <= 1.0, (space, sphere)
        assert _check_pair("constant", pred, target, expo, space) <= 1.0


def test_black_images_and_black_pixels_stay_finite():
    """both images all zero: the cosine sum is 0 and every entry finite (in stored space all but sum w are exactly 0, and the SSIM
    exactly 1).  Single pixels with p = 0, t = 0 and both, inside an ordinary map: within budget of the oracle -- the product of
    the two 1e-20 floors of the cosine's norms is a float32 denormal, and 0 / denormal must come out 0"""
    from reni_amd import ops
    H, W = E.VALUE_SHAPE
    for space in E.SPACES:
        zp, zt, ze = E.value_pair("zero", space)
        assert _check_pair("zero", zp, zt, ze, space) <= 1.0
        bp, bt, be = E.value_pair("black pixels", space)
        assert _check_pair("black pixels", bp, bt, be, space) <= 1.0
    zero = _t(E.value_pair("zero", "stored")[0])
    for kind in E.WEIGHT_KINDS:
        got = ops.pair_stats(zero, zero, _t(E.weight(kind, H, W)))
        assert bool((got[:, 1:] == 0).all()) and bool((got[:, 0] > 0).all()), (kind, got)
    for sphere in (True, False):
        mean, gmap = ops.ssim(zero, zero, None, "stored", L=2.0, sphere=sphere, return_map=True)
        assert bool((mean == 1).all()) and bool((gmap[:, torch.from_numpy(E.interior(H, W, sphere)).to(_dev())] == 1).all())
    # the three black pixels alone, the rest of the image hidden: the cosine sum is exactly 0
    bp, bt, _ = E.value_pair("black pixels", "stored")
    w = np.zeros((H, W), np.float32)
    w[3, 4] = w[20, 33] = w[36, 49] = 1.0
    got = ops.pair_stats(_t(bp), _t(bt), _t(w))
    assert bool((got[:, 0] == 3).all()) and bool((got[:, 3] == 0).all()), got


def _hide(x, mask, value):
    y = x.clone()
    y[:, :, mask] = value
    return y


@pytest.mark.parametrize("shape", [(37, 50), (3, 5462)], ids=_id)
def test_weight_zero_hides_a_pixel_from_pair_stats(shape):
    """a NaN, +inf, -inf or a number whose radiance overflows, in pred, target or both, at pixels of weight 0 -- the first pixel,
    the last, two in the clamped tail's chunk (at 3 x 5462 the ninth chunk's only two), a whole 32 x 32 tile: all eight entries
    are the bits of the same call with ordinary numbers there"""
    from reni_amd import ops
    H, W = shape
    pred, target, expo = E.shape_inputs(H, W)
    p, t, q = _t(pred), _t(target), _t(expo)
    for mname, mask in E.hidden_masks(H, W).items():
        m = torch.from_numpy(mask).to(_dev())
        for kind in ("sin", "random"):
            w = np.broadcast_to(E.weight(kind, H, W), (E.B, H, W)).copy()
            w[:, mask] = 0.0
            wt = _t(w)
            for space in E.SPACES:
                clean = ops.pair_stats(p, t, wt, space, MM, q)
                assert bool(torch.isfinite(clean).all())
                ref, bud = E.stats_reference(pred, target, w, space, expo)
                assert E.stats_ratio(clean.cpu().numpy(), ref, bud) <= 1.0, (mname, kind, space)
                for vname, value in E.BAD_VALUES.items():
                    for which in ("pred", "target", "both"):
                        pb = _hide(p, m, value) if which != "target" else p
                        tb = _hide(t, m, value) if which != "pred" else t
                        got = ops.pair_stats(pb, tb, wt, space, MM, q)
                        assert _same_bits(got, clean), (mname, kind, space, vname, which, got, clean)


@pytest.mark.parametrize("sphere,shape,masks", [(True, (37, 50), ("first", "last", "tail", "tile")), (True, (7, 12), ("first",)),
                                                (False, (37, 50), ("first", "last", "tail", "tile"))],
                         ids=["sphere-37x50", "sphere-7x12", "planar-37x50"])
def test_a_hidden_pixel_still_feeds_the_windows_of_its_neighbours(sphere, shape, masks):
    """SSIM has no per-tap weight: a pixel of weight 0 is left out of the MEAN, but its value is a tap of every window that holds
    it (include/reni_hip.h).  With a value that is not finite once mapped, the map is NaN exactly on the pixels whose window
    holds it -- the set sphere_pad's tap rule gives -- and the bits of the clean run everywhere else; the mean is the clean run's,
    bit for bit, once every pixel of that set has weight 0.  A value the mapping makes finite (exp(-inf) = 0, the sRGB clamp of
    +inf = 1) leaves the map finite."""
    from reni_amd import ops
    H, W = shape
    pred, target, expo = E.shape_inputs(H, W)
    p, t, q = _t(pred), _t(target), _t(expo)
    for mname in masks:
        mask = E.hidden_masks(H, W)[mname]
        m = torch.from_numpy(mask).to(_dev())
        hits = E.window_hits(mask, sphere)
        assert hits.any() and not hits.all() and (not sphere or hits[mask].all())
        h = torch.from_numpy(hits).to(_dev())
        w = None
        if sphere:
            w = np.broadcast_to(E.weight("sin", H, W), (H, W)).copy()
            w[hits] = 0.0
        for space in E.SPACES:
            L = E.ssim_L(space, target)
            c_mean, c_map = ops.ssim(p, t, _t(w), space, MM, q, L, sphere, return_map=True)
            assert bool(torch.isfinite(c_map).all()) and bool(torch.isfinite(c_mean).all())
            for vname, value in E.BAD_VALUES.items():
                for which in ("pred", "target", "both"):
                    pb = _hide(p, m, value) if which != "target" else p
                    tb = _hide(t, m, value) if which != "pred" else t
                    mean, gmap = ops.ssim(pb, tb, _t(w), space, MM, q, L, sphere, return_map=True)
                    what = (mname, space, vname, which)
                    if E.mapped_is_finite(value, space):
                        assert bool(torch.isfinite(gmap).all()), what
                    else:
                        assert torch.equal(torch.isnan(gmap), h.expand(E.B, H, W)), what
                    assert _same_bits(gmap[:, ~h], c_map[:, ~h]), what
                    if sphere:
                        assert _same_bits(mean, c_mean), what
                    elif not E.mapped_is_finite(value, space):
                        assert bool(torch.isnan(mean).all()), what  # (the planar mean has no weight to hide the window with)


def test_no_live_pixel():
    """every weight 0: the sums are exactly 0, the maximum -inf, the minimum +inf, and the SSIM mean is NaN (0 / 0) -- whatever
    the images hold"""
    from reni_amd import ops
    H, W = E.VALUE_SHAPE
    pred, target, expo = E.shape_inputs(H, W)
    p, t, q = _t(pred), _t(target), _t(expo)
    want = torch.tensor([0, 0, 0, 0, float("-inf"), float("inf"), 0, 0], device=_dev()).expand(E.B, 8)
    for w in (torch.zeros(E.B, H, W), torch.zeros(H, 1)):
        wt = w.to(_dev())
        for space in E.SPACES:
            for pb in (p, _hide(p, torch.ones(H, W, dtype=torch.bool, device=_dev()), float("nan"))):
                got = ops.pair_stats(pb, t, wt, space, MM, q)
                assert torch.equal(got, want), (space, got)
            mean, gmap = ops.ssim(p, t, wt, space, MM, q, E.ssim_L(space, target), True, return_map=True)
            assert bool(torch.isnan(mean).all()) and bool(torch.isfinite(gmap).all()), (space, mean)


@pytest.mark.parametrize("where", ["first", "last"])
def test_exactly_one_live_pixel(where):
    """entries 4 and 5 are the largest and the smallest of the pixel's three channels (exact in stored space, equal only for a grey
    pixel), the sums are that pixel's terms within budget, the SSIM mean is the map's value there within 2 u"""
    from reni_amd import ops
    H, W = E.VALUE_SHAPE
    pred, target, expo = E.shape_inputs(H, W)
    r, c = (0, 0) if where == "first" else (H - 1, W - 1)
    grey = target.copy()
    grey[1, :, r, c] = grey[1, 0, r, c]  # image 1's live pixel is grey, image 0's is not
    w = np.zeros((E.B, H, W), np.float32)
    w[:, r, c] = 0.7
    p, t, q, wt = _t(pred), _t(grey), _t(expo), _t(w)
    for space in E.SPACES:
        got = ops.pair_stats(p, t, wt, space, MM, q).cpu().numpy()
        ref, bud = E.stats_reference(pred, grey, w, space, expo)
        ratio = E.stats_ratio(got, ref, bud)
        print(f"one live pixel ({where}) {space}: pair_stats largest err / budget {ratio:.3f}")
        assert ratio <= 1.0, (space, ratio)
        assert got[0, 4] > got[0, 5] and got[1, 4] == got[1, 5], (space, got[:, 4:6])
        if space == "stored":
            px = grey[:, :, r, c]
            assert np.array_equal(got[:, 4], px.max(1)) and np.array_equal(got[:, 5], px.min(1)) and np.array_equal(got[:, 0], w[:, r, c])
        mean, gmap = ops.ssim(p, t, wt, space, MM, q, E.ssim_L(space, grey), True, return_map=True)
        at = gmap[:, r, c].double()
        rel = float(((mean.double() - at).abs() / at.abs()).max())
        print(f"one live pixel ({where}) {space}: |ssim mean - map value| / (2 u |map value|) {rel / (2 * EPS32):.3f}")
        assert rel <= 2 * EPS32, (space, rel)


def test_extreme_exposures_in_srgb():
    """an exposure so large that every value lies on the sRGB curve's linear toe, one so small that every value clamps to 1 (two
    equal constant images: kappa = 1 + 4 / 9e-4, the largest budget of this file): both within budget"""
    pred, target, _ = E.shape_inputs(*E.VALUE_SHAPE)
    toe, clamp = E.extreme_exposures()
    for x in (pred, target):
        assert np_map(x, "srgb", MM, toe).max() <= 12.92 * 0.0031308 and np_map(x, "srgb", MM, toe).min() > 0
        assert (np_map(x, "srgb", MM, clamp) == np_map(x, "srgb", MM, clamp).flat[0]).all()
    assert _check_pair("toe", pred, target, toe, "srgb") <= 1.0
    assert _check_pair("clamp", pred, target, clamp, "srgb") <= 1.0


def _scores(p, t, w, space, q, L, size, sphere_ok, planar_ok):
    """every result of the two entry points for one pair: [pair_stats, sphere mean, sphere map, planar mean, planar map]"""
    from reni_amd import ops
    out = [ops.pair_stats(p, t, w, space, MM, q, size=size)]
    if sphere_ok:
        out += list(ops.ssim(p, t, w, space, MM, q, L, True, return_map=True, size=size))
    if planar_ok and w is None:
        out += list(ops.ssim(p, t, None, space, MM, q, L, False, return_map=True, size=size))
    return out


def _assert_same(a, b, what):
    assert len(a) == len(b) and len(a) >= 2
    for k, (x, y) in enumerate(zip(a, b)):
        assert _same_bits(x, y), (what, k)


@pytest.mark.parametrize("shape", [(37, 50), (5, 2)], ids=_id)
def test_results_do_not_depend_on_how_the_operands_are_addressed(shape):
    """planar contiguous, the model-output layout [B, P, 3] with size = (H, W), a non-contiguous slice of a larger tensor, a
    target expanded over the batch (stride 0), the same weights as [H, 1], [1, W], [B, 1, 1] and full [B, H, W]: identical bits;
    image b alone is image b of the batch"""
    H, W = shape
    pred, target, expo = E.shape_inputs(H, W)
    q = _t(expo)
    planar_ok = min(H, W) >= 11
    lp, lt = _layouts(pred.transpose(0, 2, 3, 1)), _layouts(target.transpose(0, 2, 3, 1))
    g = np.random.default_rng(5)
    weights = {"none": None, "rows": _t(g.random((H, 1))), "columns": _t(g.random((1, W))), "images": _t(g.random((E.B, 1, 1))),
               "full": _t(E.weight("random", H, W))}
    for space in E.SPACES:
        L = E.ssim_L(space, target)
        for wname, w in weights.items():
            p, t = lp["planar"], lt["planar"]
            base = _scores(p, t, w, space, q, L, None, True, planar_ok)
            assert all(bool(torch.isfinite(x).all()) for x in base)
            what = (space, wname)
            _assert_same(_scores(p, t, w, space, q, L, None, True, planar_ok), base, what + ("again",))
            _assert_same(_scores(lp["model"], lt["model"], w, space, q, L, (H, W), True, planar_ok), base, what + ("model",))
            _assert_same(_scores(lp["model"], t, w, space, q, L, None, True, planar_ok), base, what + ("mixed",))
            ps, ts = lp["slice"].permute(0, 3, 1, 2), lt["slice"].permute(0, 3, 1, 2)
            assert not ps.is_contiguous() and ps.stride() == (H * (W + 3) * 4, 1, (W + 3) * 4, 4)
            _assert_same(_scores(ps, ts, w, space, q, L, None, True, planar_ok), base, what + ("slice",))
            if w is not None:  # the same numbers, materialised
                full = torch.broadcast_to(w, (E.B, H, W)).contiguous()
                _assert_same(_scores(p, t, full, space, q, L, None, True, planar_ok), base, what + ("full weight",))
            for b in range(E.B):
                wb = w if w is None or w.shape[0] != E.B else w[b:b + 1]
                one = _scores(p[b:b + 1], t[b:b + 1], wb, space, q[b:b + 1], L, None, True, planar_ok)
                _assert_same(one, [x[b:b + 1] for x in base], what + ("alone", b))
            # one target for the whole batch, through a stride of 0
            shared = t[:1].expand(E.B, 3, H, W)
            assert shared.stride(0) == 0
            q0 = q[:1].expand(E.B).contiguous()
            _assert_same(_scores(p, shared, w, space, q0, L, None, True, planar_ok),
                         _scores(p, shared.contiguous(), w, space, q0, L, None, True, planar_ok), what + ("expanded",))


# ---------------------------------------------------------------------------------------------- 3. stray and missing stores
def _lib():
    from reni_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _c_head(p, t, w, space, q):
    from reni_amd import ops
    pv, tv, wv = ops._pair_args(p, t, w)
    m0, m1, qq = ops._space_args(space, MM, q, pv.shape[0], pv.device)
    return (pv, tv, wv, qq), ops._pair_call_head(pv, tv, wv, space, m0, m1, qq)


def c_pair_stats(p, t, w, space, q, out_ptr, ws_fill):
    """reni_pair_stats through the C entry point, the output wherever out_ptr says, every byte of the workspace `ws_fill`"""
    lib = _lib()
    keep, head = _c_head(p, t, w, space, q)
    B, _, H, W = keep[0].shape
    ws, wp, wn = _workspace(int(lib.reni_pair_stats_workspace_bytes(B, H, W)), ws_fill)
    rc = lib.reni_pair_stats(*head, out_ptr, wp, wn, _stream())
    assert rc == 0, lib.reni_last_error()
    torch.cuda.synchronize()


def c_ssim(p, t, w, space, q, L, sphere, out_ptr, map_ptr, ws_fill):
    from reni_amd import _lib as L_
    lib = _lib()
    keep, head = _c_head(p, t, w, space, q)
    B, _, H, W = keep[0].shape
    ws, wp, wn = _workspace(int(lib.reni_pair_stats_workspace_bytes(B, H, W)), ws_fill)
    rc = lib.reni_ssim(*head, float(L), L_.SSIM_MODE["sphere" if sphere else "planar"], out_ptr, map_ptr, wp, wn, _stream())
    assert rc == 0, lib.reni_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(3, 5462), (5, 2), (37, 50), (11, 11), (1, 2049), (7, 2048)], ids=_id)
def test_outputs_stay_inside_their_buffers_and_partials_are_written_before_they_are_read(shape):
    """out [B][8], out [B] and map_out [B][H][W] in the middle of sentinel-filled allocations: no store beside them, every word
    written (the planar border as 0, not left alone), the values those of the ops call -- once with the workspace all 0x00 and
    once all 0xFF (NaN partials): k_finish reads only the nblk = 1, 2, 7, 9 (pair_stats) and 1, 4 (ssim) partials that were
    written"""
    from reni_amd import ops
    H, W = shape
    pred, target, expo = E.shape_inputs(H, W)
    p, t, q = _t(pred), _t(target), _t(expo)
    assert E.nblk(H, W) in (1, 2, 7, 9)
    modes = [s for s in (True, False) if (W % 2 == 0 and H >= 5 if s else min(H, W) >= 11)]
    for space in E.SPACES:
        L = E.ssim_L(space, target)
        for kind in ("none", "random"):
            wt = _t(E.weight(kind, H, W))
            want = ops.pair_stats(p, t, wt, space, MM, q)
            for fill in (0x00, 0xFF):
                out = Carved(E.B, 8)
                c_pair_stats(p, t, wt, space, q, out.ptr, fill)
                out.check(want, f"pair_stats {space} {kind} ws={fill:#x}")
            for sphere in modes:
                if not sphere and wt is not None:
                    continue
                w_mean, w_map = ops.ssim(p, t, wt, space, MM, q, L, sphere, return_map=True)
                for fill in (0x00, 0xFF):
                    out, smap = Carved(E.B), Carved(E.B, H, W)
                    c_ssim(p, t, wt, space, q, L, sphere, out.ptr, smap.ptr, fill)
                    out.check(w_mean, f"ssim mean {_mode(sphere)} {space} {kind} ws={fill:#x}")
                    smap.check(w_map, f"ssim map {_mode(sphere)} {space} {kind} ws={fill:#x}")
                    alone = Carved(E.B)
                    c_ssim(p, t, wt, space, q, L, sphere, alone.ptr, None, fill)  # map_out NULL
                    alone.check(w_mean, f"ssim mean without a map {_mode(sphere)} {space} {kind} ws={fill:#x}")


# ---------------------------------------------------------------------------------------------- 4. light tables: wide rows
def _structure(pmf, cond, marg):
    """the promises of include/reni_hip.h on downloaded tables: ascending, exactly 0 in front of the first mass, exactly 1.0f from
    the last mass on, flat over every texel without mass; a row without mass is (j + 1) / W"""
    Bn, H, W = pmf.shape
    one = np.float32(1.0)
    assert np.all(cond[:, :, -1] == one) and np.all(marg[:, -1] == one)
    assert np.all(np.diff(cond, axis=2) >= 0) and np.all(np.diff(marg, axis=1) >= 0)
    for cdf, mass in ((cond, pmf > 0), (marg, (pmf > 0).any(2))):
        seen = np.cumsum(mass, -1)                                   # entries with mass up to and including this one
        left = seen[..., -1:] - seen                                 # ... and behind it
        some = seen[..., -1:] > 0
        assert np.all(cdf[(seen == 0) & some] == 0)
        assert np.all(cdf[(left == 0) & (seen > 0)] == one)
        assert np.all((np.diff(cdf, axis=-1) == 0)[~mass[..., 1:] & np.broadcast_to(some, mass.shape)[..., 1:]])
    dark = ~(pmf > 0).any(2)
    assert np.array_equal(cond[dark], np.broadcast_to(((np.arange(W) + 1.0) / W).astype(np.float32), (int(dark.sum()), W)))


@pytest.mark.parametrize("W,Bn", E.LIGHT_WIDTHS, ids=lambda v: str(v))
def test_wide_light_tables_match_float64(W, Bn):
    """W = 1024: four row tiles, two marginal tiles; W = 4096 (LT_MAX_W): sixteen and eight -- the multi-tile scan of k_lt_image
    and every carry of row_scan_d and row_cdf behind the second.  The budgets of test_tables_match_float64_in_stored_space,
    which come from a double-precision scan and do not depend on W."""
    from reni_amd import lighting
    m = E.light_maps(W, Bn)
    H = W // 2
    views = _layouts(m)
    for eps in E.LIGHT_MIXES:
        ref = E.light_reference(W, Bn, eps)
        tabs = {k: lighting.build_light_table(v, space="stored", uniform_mix=eps, size=(H, W)) for k, v in views.items()}
        got = _np(tabs["model"])
        errs = _table_errors(got, ref, E.LIGHT_PMF_REL, E.LIGHT_CDF_ABS)
        print(f"stored W={W} B={Bn} eps={eps}: err/budget pmf {errs[0]:.3f} cond {errs[1]:.3f} marg {errs[2]:.3f}")
        assert max(errs) <= 1.0, errs
        assert got[0].dtype == np.float32 and got[0].shape == (Bn, H, W) and got[2].shape == (Bn, H)
        _structure(*got)
        if eps == 0.0:  # the black row
            assert np.all(got[0][:, 1] == 0) and np.array_equal(got[2][:, 1], got[2][:, 0])
        else:
            assert np.all(got[0] > 0)
        for k in ("planar", "slice"):  # however the maps are addressed
            for a, b in zip((tabs[k].pmf, tabs[k].cond, tabs[k].marg), (tabs["model"].pmf, tabs["model"].cond, tabs["model"].marg)):
                assert torch.equal(a, b), k
        again = lighting.build_light_table(views["model"], space="stored", uniform_mix=eps, size=(H, W))
        assert torch.equal(again.pmf, tabs["model"].pmf) and torch.equal(again.cond, tabs["model"].cond) and torch.equal(again.marg, tabs["model"].marg)
        if W == 1024:
            for b in range(Bn):  # alone as inside the batch
                one = lighting.build_light_table(views["planar"][b:b + 1], space="stored", uniform_mix=eps)
                for a, g_ in zip(_np(one), got):
                    assert np.array_equal(a[0], g_[b]), b


@pytest.mark.parametrize("name", ["column 0", "column W-1", "third tile", "rows >= 256", "rows < 256"])
def test_each_carry_of_the_tiled_scans_alone_places_the_mass(name):
    """W = 1024, mass by mask in one place only: in column 0 (every later tile holds nothing but the carry), in column W - 1
    (three empty tiles in front), inside the third tile, in the marginal's second tile only and in its first only"""
    from reni_amd import lighting
    W, Bn = E.LIGHT_WIDTHS[0]
    H = W // 2
    mask = E.light_masks(W)[name]
    table = lighting.build_light_table(_t(E.light_maps(W, Bn)), space="stored", mask=_t(mask), uniform_mix=0.0)
    got = _np(table)
    ref = E.light_reference(W, Bn, 0.0, name)
    errs = _table_errors(got, ref, E.LIGHT_PMF_REL, E.LIGHT_CDF_ABS)
    print(f"mask '{name}' W={W}: err/budget pmf {errs[0]:.3f} cond {errs[1]:.3f} marg {errs[2]:.3f}")
    assert max(errs) <= 1.0, errs
    pmf, cond, marg = got
    assert np.all(pmf[:, mask == 0] == 0)
    _structure(pmf, cond, marg)
    lit = (pmf > 0).any(2)
    assert np.array_equal(lit, np.broadcast_to(mask.any(1) & (np.arange(H) != 1), (Bn, H)))  # (row 1 of the maps is black)
    one = np.float32(1.0)
    if name == "column 0":
        assert np.all(cond[lit] == one)
    elif name == "column W-1":
        assert np.all(cond[lit][:, :-1] == 0)
    elif name == "third tile":
        assert np.all(cond[lit][:, :2 * E.LT_TILE] == 0) and np.all(cond[lit][:, 3 * E.LT_TILE - 1:] == one)
    elif name == "rows >= 256":
        assert not lit[:, :E.LT_TILE].any() and np.all(marg[:, :E.LT_TILE] == 0) and np.all(marg[:, E.LT_TILE] > 0)
    else:
        assert not lit[:, E.LT_TILE:].any() and np.all(marg[:, E.LT_TILE - 1:] == one) and np.all(marg[:, E.LT_TILE - 2] < one)


def test_sampling_a_wide_table_is_the_searchsorted_rule():
    """W = 1024: random uniforms, the edge values and exact ties against np_select on the downloaded tables, bit for bit; no chosen
    texel has pmf 0"""
    from reni_amd import lighting
    W, Bn = E.LIGHT_WIDTHS[0]
    H = W // 2
    m = sky_maps(Bn, W, 200 + W, zero_row=True)
    mask = np.ones((H, W), np.float32)
    mask[:, W // 2:] = 0.0
    mask[:, 2::3] = 0.0
    maps = _t(m)
    table = lighting.build_light_table(maps, space="stored", mask=_t(mask))
    tabs = _np(table)
    _structure(*tabs)
    u = _test_uniforms(tabs, W)
    s = lighting.sample_lights(table, maps, u=_t(u))
    index = s.index.cpu().numpy()
    i, j = np_select(tabs[1], tabs[2], u)
    assert index.dtype == np.int32 and index.shape == (Bn, u.shape[0])
    assert np.array_equal(index, i * W + j)
    assert np.all(tabs[0].reshape(Bn, -1)[np.arange(Bn)[:, None], index] > 0) and np.all(index % W < W // 2) and np.all(index // W != 1)


def test_the_width_limit_is_4096():
    """H = 2048 with W = 4098 and W = 4094 raises (and the C entry point returns RENI_EINVAL before it touches a pointer);
    W = 4096 does not"""
    from reni_amd import lighting
    lib = _lib()
    st4, st3 = (ctypes.c_int64 * 4)(0, 0, 0, 0), (ctypes.c_int64 * 3)(0, 0, 0)
    for W in (4098, 4094):
        with pytest.raises(ValueError):
            lighting.build_light_table(torch.ones(1, 3, 2048, W, device=_dev()), space="stored")
        assert lib.reni_light_table_workspace_bytes(1, 2048, W) == 0
        assert lib.reni_light_table_build(1, 2048, W, None, st4, None, st3, 0, 0.0, 1.0, None, 0.0, None, None, None, None, 0, None) == -1
    table = lighting.build_light_table(torch.ones(1, 3, 2048, 4096, device=_dev()), space="stored")
    assert table.pmf.shape == (1, 2048, 4096) and bool((table.cond[:, :, -1] == 1).all()) and bool((table.marg[:, -1] == 1).all())
