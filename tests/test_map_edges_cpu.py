"""CPU check of the resample, blur and rotation edge cases (tests/map_edge_cases.py): the lists hold the shapes they name,
and an fp32 restatement of each kernel -- every operation rounded once, in the kernel's written order -- stays within half of
the bound tests/test_gpu_map_edges.py applies against float64.  A case that plain fp32 arithmetic already pushed to its bound
would make the GPU comparison say nothing about the kernel; it fails here first.  For the rotation the oracle's own caps are
checked too: a yaw leaves out no pixel at any height, and no listed case has a pixel where a nearest tap may differ."""
import numpy as np
import pytest

from tests import map_edge_cases as E
from tests.test_resample_cpu import np_gaussian_blur, np_resample, resample_bound
from tests.test_rotate_cpu import emulate_coordinates_fp32, emulate_kernel_fp32, fetch, np_rotate_envmap, rotate_bound

IDS = [f"{N}x{C}-{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}" for N, C, p in E.RESAMPLE_CASES]


def test_case_lists_hold_the_shapes_they_name():
    assert len(E.RESAMPLE_PAIRS) == 12 and len(set(E.RESAMPLE_PAIRS)) == 12 and E.IDENTITY_PAIR in E.RESAMPLE_PAIRS
    px = [hd * wd for _, (hd, wd) in E.RESAMPLE_PAIRS]
    assert {1, 255, 256, 257} <= set(px) and max(max(s) for s, _ in E.RESAMPLE_PAIRS) == 1000
    assert {(N, C) for N, C, _ in E.RESAMPLE_CASES} == {(2, 3), (1, 1), (3, 5)}
    assert [h * w for h, w in E.CARVED_TARGETS] == [255, 256, 257]
    assert {tx for _, tx in E.GENERIC_TAPS} >= {3, 5, 6, 7} and all(ty != tx for ty, tx in E.GENERIC_TAPS[2:])
    assert [tx for _, tx in E.REGISTER_TAPS] == [1, 2, 4, 8] and all(ty != tx for ty, tx in E.REGISTER_TAPS)
    assert [E.blur_radius(s) for s in E.BLUR_SIGMAS] == [0, 2, 4, 12, 20, 49]
    assert sum(h * w % 256 == 0 for h, w in E.BLUR_SHAPES) == 1 and all(s in E.BLUR_SHAPES for s in E.BLUR_WORKSPACE_SHAPES)
    assert [s for s in E.ROTATE_SHAPES if s[0] * s[1] % 256 == 0] == [(16, 16), (8, 64)]
    assert all(w % 2 == 0 for _, w in E.ROTATE_SHAPES) and E.ROTATE_CARVED_SHAPE in E.ROTATE_SHAPES
    x = E.maps(2, 5, 9, 30, 1)
    assert x.shape == (2, 5, 9, 30) and x[0].min() > 0 and x[1].min() < 0 and (x.max(axis=(2, 3)) >= 1999).all()


# ------------------------------------------------------------------------------------------------ resampler
@pytest.mark.parametrize("case", E.RESAMPLE_CASES, ids=IDS)
def test_resample_cases_leave_room_for_the_kernel(case):
    N, C, pair = case
    x = E.resample_input(N, C, pair)
    worst = 0.0
    for mode in E.MODES:
        ri, rw, ci, cw = E.mode_tables(pair, mode)
        ref = np_resample(x, pair[1], mode)
        assert np.array_equal(ref, E.table_sum(x, ri, rw, ci, cw))  # the separated sum is np_resample's
        bound = resample_bound(x, pair[1], mode)
        assert np.array_equal(bound, E.table_bound(x, ri, rw, ci, cw)) and (bound > 0).all()
        got = E.table_sum_fp32(x, ri, rw.astype(np.float32), ci, cw.astype(np.float32))
        ratio = float((np.abs(got - ref) / bound).max())
        worst = max(worst, ratio)
        if pair == E.IDENTITY_PAIR:
            assert np.array_equal(got, x), mode
    print(f"resample {N}x{C} {pair[0]} -> {pair[1]}: fp32 restatement / bound {worst:.3f}")
    assert worst <= E.ROOM


@pytest.mark.parametrize("sizes", E.TABLE_SIZES)
def test_generic_tables_leave_room_and_notice_a_dropped_tap(sizes):
    (hs, ws), (hd, wd) = sizes
    x = E.resample_input(2, 3, sizes)
    for ty, tx in E.GENERIC_TAPS + E.REGISTER_TAPS:
        ri, rw = E.random_tables(hs, hd, ty, 100 + ty)
        ci, cw = E.random_tables(ws, wd, tx, 200 + tx)
        assert (rw != 0).all() and (cw != 0).all() and ri.min() >= 0 and ri.max() < hs and ci.min() >= 0 and ci.max() < ws
        ref, bound = E.table_sum(x, ri, rw, ci, cw), E.table_bound(x, ri, rw, ci, cw)
        ratio = float((np.abs(E.table_sum_fp32(x, ri, rw, ci, cw) - ref) / bound).max())
        assert ratio <= E.ROOM, (ty, tx, ratio)
        # without its last column tap, or its first row tap, the sum is off by many bounds at most pixels
        if tx > 1:
            off = np.abs(E.table_sum(x, ri, rw, ci[:, :-1], cw[:, :-1]) - ref) / bound
            assert np.median(off) > 100, (ty, tx)
        if ty > 1:
            off = np.abs(E.table_sum(x, ri[:, 1:], rw[:, 1:], ci, cw) - ref) / bound
            assert np.median(off) > 100, (ty, tx)
    wi, _ = E.random_tables(hs, hd, 3, 7, wild=True)
    assert wi.min() == -3 and wi.max() == hs + 4


# ------------------------------------------------------------------------------------------------ blur
@pytest.mark.parametrize("shape", E.BLUR_SHAPES)
def test_blur_cases_leave_room_for_the_kernel(shape):
    H, W = shape
    worst = 0.0
    for C in E.BLUR_CHANNELS:
        for n in range(2):
            img = E.blur_image(C, H, W, n)
            for sigma in E.BLUR_SIGMAS:
                ref = np_gaussian_blur(img, sigma, fp32_intermediate=False)
                bound = E.blur_bound(img, sigma)
                got = E.blur_fp32(img, sigma)
                assert ref.shape == img.shape and (bound > 0).all()
                if E.blur_radius(sigma) == 0:
                    assert np.array_equal(got, img)
                worst = max(worst, float((np.abs(got - ref) / bound).max()))
    print(f"blur {H}x{W}: fp32 restatement / bound {worst:.3f}")
    assert worst <= E.ROOM


def test_blur_bound_follows_the_image_and_notices_a_clamped_border():
    """away from the spot the per-pixel bound is orders below the max|img|-wide one, and a clamp in place of the reflection is
    many bounds off wherever the radius passes the edge"""
    from reni_amd.resample import gaussian_weights
    img = E.blur_image(3, 40, 40, 0)
    b = E.blur_bound(img, 1)
    assert b.min() < 1e-3 * b.max()
    for (H, W), sigma in (((5, 52), 3), ((1, 7), 5), ((2, 3), 12.3)):
        img = E.blur_image(3, H, W, 1).astype(np.float64)
        w, r = gaussian_weights(sigma)
        iy = np.clip(np.arange(H)[:, None] + np.arange(-r, r + 1)[None, :], 0, H - 1)
        ix = np.clip(np.arange(W)[:, None] + np.arange(-r, r + 1)[None, :], 0, W - 1)
        mid = sum(img[iy[:, t]] * w[t] for t in range(2 * r + 1))
        clamped = sum(mid[:, ix[:, t]] * w[t] for t in range(2 * r + 1))
        off = np.abs(clamped - np_gaussian_blur(img, sigma, fp32_intermediate=False)) / E.blur_bound(img, sigma)
        assert off.max() > 100, (H, W, sigma)


# ------------------------------------------------------------------------------------------------ rotation
@pytest.mark.parametrize("shape", E.ROTATE_SHAPES)
def test_rotation_cases_leave_room_for_the_kernel(shape):
    H, W = shape
    worst = 0.0
    for C in ((3, 1, 5) if shape == E.ROTATE_CHANNEL_SHAPE else (3,)):
        x = E.rotate_input(H, W, C)
        for name, R32, yaw in E.bilinear_rotations(H, W):
            ref = np_rotate_envmap(x, R32)
            bound, keep = rotate_bound(x, R32)
            if yaw:
                assert keep.all(), name  # the polar angle is kept: nothing is left out, at any H
            else:
                assert (~keep).sum() <= W and (~keep).sum() * H <= 2 * H * W, name
            got = emulate_kernel_fp32(x, R32)
            assert np.isfinite(got).all()
            worst = max(worst, float((np.abs(got - ref) / bound)[..., keep].max()))
    print(f"rotate {H}x{W}: fp32 restatement / bound {worst:.3f}")
    assert worst <= E.ROOM


@pytest.mark.parametrize("shape", [s for s in E.ROTATE_SHAPES if s[0] >= E.GENERAL_MIN_H])
def test_no_listed_rotation_has_a_pixel_where_nearest_may_differ(shape):
    """the permitted set of nearest_permitted is empty for every case, so the GPU test's comparison is an equality outside the
    caps; the fp32 restatement's coordinates pick the oracle's tap there"""
    H, W = shape
    x = E.rotate_input(H, W)
    least = np.inf
    for name, R in E.nearest_rotations():
        R32 = R.astype(np.float32)
        permitted, keep, margin = E.nearest_permitted(H, W, R32)
        least = min(least, margin)
        assert not permitted.any(), (name, int(permitted.sum()))
        row, col = emulate_coordinates_fp32(H, W, R32)
        got = fetch(x, np.floor(row + np.float32(0.5)).astype(np.int64), np.floor(col + np.float32(0.5)).astype(np.int64))
        assert np.array_equal(got[..., keep], np_rotate_envmap(x, R32, "nearest")[..., keep]), name
    print(f"rotate nearest {H}x{W}: smallest distance to a half-integer / threshold {least:.1f}")


@pytest.mark.parametrize("shape", [s for s in E.ROTATE_SHAPES if s[0] >= E.GENERAL_MIN_H])
def test_taps_beyond_a_pole_are_compared_somewhere(shape):
    """every shape has pixels inside E.pole_pixels under rotation_list(); the fp32 restatement keeps half of the bound there,
    and the same sum with the top-left tap left on the near side of the pole misses it by far"""
    from tests.test_rotate_cpu import rotation_list, source_coordinates
    H, W = shape
    x = E.rotate_input(H, W)
    count, worst, near_side = 0, 0.0, 0.0
    for name, R in rotation_list():
        R32 = R.astype(np.float32)
        pole = E.pole_pixels(H, W, R32)
        if not pole.any():
            continue
        count += int(pole.sum())
        ref = np_rotate_envmap(x, R32)
        bound, _ = rotate_bound(x, R32)
        worst = max(worst, float((np.abs(emulate_kernel_fp32(x, R32) - ref) / bound)[..., pole].max()))
        row, col, _ = source_coordinates(H, W, R32)
        i, j = np.floor(row).astype(np.int64), np.floor(col).astype(np.int64)
        t00 = np.where(i < 0, x[..., np.clip(-1 - i, 0, H - 1), np.mod(j, W)] - fetch(x, i, j), 0.0)  # the tap's error
        near_side = max(near_side, float((np.abs((1 - (row - i)) * (1 - (col - j)) * t00) / bound)[..., pole].max()))
    print(f"rotate {H}x{W}: {count} pixels reach beyond a pole; fp32 restatement / bound {worst:.3f}; near-side tap / bound {near_side:.0f}")
    assert count >= 8 and worst <= E.ROOM and near_side > 100


@pytest.mark.parametrize("shape", E.ROTATE_SHAPES)
def test_oracle_nearest_identities_hold_at_the_edge_shapes(shape):
    x = E.rotate_input(*shape).astype(np.float64)
    for name, R, want in E.nearest_exact_cases(x):
        assert np.array_equal(np_rotate_envmap(x, R.astype(np.float32), "nearest"), want), name
