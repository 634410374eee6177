"""CPU check of the case lists of tests/metrics_edge_cases.py: the lists hold the shapes they name, and at every shape case the
pairwise fp32 restatement of tests/test_metrics_cpu.py (np32_pair_stats, np32_ssim) stays within HALF of the budget that
tests/test_gpu_metrics_edges.py holds the HIP kernels to.  A case whose arithmetic alone uses up the bound would say nothing
about the kernel; it fails here first.  The largest per-pixel SSIM budget of any case, the constant images of the value cases
included, is capped at 5e-3 so that the bound cannot go slack (kappa of two constant images is 1 + 4 / 9e-4 at most here).

Each test prints its largest restatement / budget (pytest -s or -rA shows them)."""
import numpy as np
import pytest

from tests import metrics_edge_cases as E
from tests.test_metrics_cpu import np32_pair_stats, np32_ssim, ssim_budget

SSIM_PIXEL_BUDGET_CAP = 5e-3


def test_case_lists_hold_the_shapes_they_name():
    assert E.B == 2 and E.PS_CHUNK == 2048 and E.SS_T == 32
    assert [E.nblk(1, W) for W in (1, 2047, 2048, 2049)] == [1, 1, 1, 2]
    assert [E.nblk(H, W) for H, W in E.PAIR_SHAPES[-7:]] == [1, 1, 2, 7, 8, 9, 17]
    assert E.PAIR_SHAPES[:3] == ((1, 1), (1, 2), (3, 7))
    assert 3 * 5462 - 8 * E.PS_CHUNK == 2  # the ninth partial holds two pixels
    assert len(set(E.PAIR_SHAPES)) == 10 and len(set(E.SPHERE_SHAPES)) == 11 and len(set(E.PLANAR_SHAPES)) == 7
    assert all(W % 2 == 0 and H >= 5 for H, W in E.SPHERE_SHAPES) and all(min(s) >= 11 for s in E.PLANAR_SHAPES)
    assert [s for s in E.SPHERE_SHAPES if s[1] < 11] == [(5, 2), (6, 4), (5, 10)]
    assert {(31, 64), (32, 64), (33, 66)} <= set(E.SPHERE_SHAPES)           # the tile boundary in both axes
    assert (37, 50) in E.SPHERE_SHAPES and (50 // 2) % 2 == 1                  # partial tiles, W / 2 odd
    assert (65, 34) in E.SPHERE_SHAPES and -(-65 // E.SS_T) == 3 and 34 % E.SS_T == 2
    assert (43, 96) in E.SPHERE_SHAPES and 96 % E.SS_T == 0 and 43 % E.SS_T
    assert {(11, 11), (11, 12), (12, 11)} <= set(E.PLANAR_SHAPES)
    assert (42, 43) in E.PLANAR_SHAPES and (42 - 10, 43 - 10) == (32, 33)
    assert E.VALUE_SHAPE in E.SPHERE_SHAPES and E.VALUE_SHAPE in E.PLANAR_SHAPES and E.nblk(*E.VALUE_SHAPE) == 1
    for H, W in set(E.PAIR_SHAPES) | set(E.SPHERE_SHAPES):
        assert E.weight("none", H, W) is None and E.weight("sin", H, W).shape == (H, 1)
        w = E.weight("random", H, W)
        assert w.shape == (E.B, H, W) and w.dtype == np.float32 and w.min() >= 0.0 and w.max() <= 1.0
        assert (w > 0).reshape(E.B, -1).any(1).all()
        if H * W >= 1000:
            assert 0.2 <= (w == 0).mean() <= 0.3
    assert [(W, B) for W, B in E.LIGHT_WIDTHS] == [(1024, 2), (4096, 1)]
    m = E.light_masks(1024)
    assert len(m) == 5 and all(v.shape == (512, 1024) for v in m.values())
    assert m["column 0"].sum() == 512 and m["column W-1"][:, -1].all() and m["third tile"][:, 512:768].all()
    assert m["third tile"].sum() == 512 * 256 and not m["rows >= 256"][:256].any() and not m["rows < 256"][256:].any()


def test_window_hits_follow_the_sphere_rule():
    H, W = 7, 12
    bad = np.zeros((H, W), bool)
    bad[0, 0] = True
    hit = E.window_hits(bad, True)
    want = np.zeros((H, W), bool)
    for i in range(H):
        for j in range(W):
            for di in range(-5, 6):
                for dj in range(-5, 6):
                    r, c = i + di, j + dj
                    if r < 0:
                        r, c = -1 - r, c + W // 2
                    elif r >= H:
                        r, c = 2 * H - 1 - r, c + W // 2
                    want[i, j] |= bool(bad[r, c % W])
    assert np.array_equal(hit, want) and hit[0, 6] and not hit[6, 6]
    planar = np.zeros((13, 14), bool)
    planar[0, 0] = True
    hp = E.window_hits(planar, False)
    assert hp[5, 5] and hp.sum() == 1  # one window reaches the corner; the border has no window
    assert E.mapped_is_finite(float("inf"), "srgb") and not E.mapped_is_finite(float("inf"), "linear")
    assert E.mapped_is_finite(float("-inf"), "linear") and not E.mapped_is_finite(float("-inf"), "stored")
    assert not E.mapped_is_finite(100.0, "linear") and not any(E.mapped_is_finite(float("nan"), s) for s in E.SPACES)


@pytest.mark.parametrize("shape", E.PAIR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pair_stats_cases_leave_room_for_the_kernel(shape):
    H, W = shape
    pred, target, expo = E.shape_inputs(H, W)
    worst = 0.0
    for space in E.SPACES:
        for kind in E.WEIGHT_KINDS:
            w = E.weight(kind, H, W)
            ref, bud = E.stats_reference(pred, target, w, space, expo)
            r = E.stats_ratio(np32_pair_stats(pred, target, w, space, E.MM, expo), ref, bud)
            worst = max(worst, r)
            assert r <= 0.5, (space, kind, r)
    print(f"{H}x{W}: pair_stats restatement / budget {worst:.3f}")


@pytest.mark.parametrize("sphere,shape", [(True, s) for s in E.SPHERE_SHAPES] + [(False, s) for s in E.PLANAR_SHAPES],
                         ids=lambda v: ("sphere" if v else "planar") if isinstance(v, bool) else f"{v[0]}x{v[1]}")
def test_ssim_cases_leave_room_for_the_kernel(sphere, shape):
    H, W = shape
    pred, target, expo = E.shape_inputs(H, W)
    worst = {"stats": 0.0, "map": 0.0, "mean": 0.0, "pix": 0.0}
    for space in E.SPACES:
        L = E.ssim_L(space, target)
        smap, kappa = E.ssim_reference(pred, target, space, expo, L, sphere)
        for kind in E.WEIGHT_KINDS if sphere else E.WEIGHT_KINDS[:1]:
            w = E.weight(kind, H, W)
            pix, img = ssim_budget(kappa, w, space, sphere)
            gmap, gmean = np32_ssim(pred, target, w, space, E.MM, expo, L, sphere)
            r_map, r_mean = E.map_ratio(gmap, smap, pix, sphere), E.mean_ratio(gmean, smap, w, img, sphere)
            worst["map"], worst["mean"] = max(worst["map"], r_map), max(worst["mean"], r_mean)
            worst["pix"] = max(worst["pix"], float(pix[:, E.interior(H, W, sphere)].max()))
            assert r_map <= 0.5 and r_mean <= 0.5, (space, kind, r_map, r_mean)
            ref, bud = E.stats_reference(pred, target, w, space, expo)  # the SSIM shapes run through pair_stats as well
            r = E.stats_ratio(np32_pair_stats(pred, target, w, space, E.MM, expo), ref, bud)
            worst["stats"] = max(worst["stats"], r)
            assert r <= 0.5, (space, kind, r)
    print(f"{'sphere' if sphere else 'planar'} {H}x{W}: restatement / budget: ssim map {worst['map']:.3f}, mean {worst['mean']:.3f}, "
          f"pair_stats {worst['stats']:.3f}; largest per-pixel budget {worst['pix']:.2e}")
    assert worst["pix"] <= SSIM_PIXEL_BUDGET_CAP


@pytest.mark.parametrize("name", [n for n, *_ in E.value_pairs()])
def test_value_cases_keep_the_ssim_budget_tight(name):
    """the pairs of the value cases: the per-pixel budget stays under the cap (two constant images reach kappa = 4.4e3, the
    largest of the file), and the restatement stays inside the budget there too"""
    H, W = E.VALUE_SHAPE
    for space in E.SPACES:
        try:
            pred, target, expo = E.value_pair(name, space)
        except KeyError:
            continue  # (the exposure cases exist in sRGB space only)
        L = E.ssim_L(space, target)
        for sphere in (True, False):
            smap, kappa = E.ssim_reference(pred, target, space, expo, L, sphere)
            w = E.weight("sin", H, W) if sphere else None
            pix, img = ssim_budget(kappa, w, space, sphere)
            top = float(pix[:, E.interior(H, W, sphere)].max())
            gmap, gmean = np32_ssim(pred, target, w, space, E.MM, expo, L, sphere)
            r_map, r_mean = E.map_ratio(gmap, smap, pix, sphere), E.mean_ratio(gmean, smap, w, img, sphere)
            print(f"{name} {space} {'sphere' if sphere else 'planar'}: largest per-pixel budget {top:.2e}, restatement / budget "
                  f"map {r_map:.3f} mean {r_mean:.3f}")
            assert top <= SSIM_PIXEL_BUDGET_CAP, (space, sphere, top)
            assert r_map <= 1.0 and r_mean <= 1.0, (space, sphere, r_map, r_mean)
            if name == "constant":
                assert np.abs(smap[:, E.interior(H, W, sphere)] - E.constant_ssim(pred, target, space, expo, L)[:, None]).max() <= 1e-9
        ref, bud = E.stats_reference(pred, target, E.weight("random", H, W), space, expo)
        r = E.stats_ratio(np32_pair_stats(pred, target, E.weight("random", H, W), space, E.MM, expo), ref, bud)
        assert np.isfinite(ref).all() and r <= 1.0, (space, r)


def test_light_masks_leave_the_mass_where_they_say():
    """the oracle's tables under the five masks at W = 1024: nothing in front of the first mass, everything at the last"""
    W, Bn = E.LIGHT_WIDTHS[0]
    for name in E.light_masks(W):
        pmf, cond, marg = E.light_reference(W, Bn, 0.0, name)
        mask = E.light_masks(W)[name]
        assert (pmf[:, mask == 0] == 0).all() and abs(pmf.sum() - Bn) <= 1e-9
        assert np.abs(marg[:, -1] - 1.0).max() <= 1e-12
    assert (E.light_reference(W, Bn, 0.0, "rows >= 256")[2][:, :E.LT_TILE] == 0).all()
    assert np.abs(E.light_reference(W, Bn, 0.0, "rows < 256")[2][:, E.LT_TILE - 1:] - 1.0).max() <= 1e-12
    assert (E.light_reference(W, Bn, 0.0, "third tile")[1][:, 2:, :2 * E.LT_TILE] == 0).all()
