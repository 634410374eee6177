"""GPU tests of the resampler, the blur (reni_tu_resample.hip) and the environment-map rotation (reni_tu_rotate.hip) at the
shapes where their guards, tails, wraps and clamps act: the cases of tests/map_edge_cases.py against the float64 oracles and
bounds of tests/test_resample_cpu.py and tests/test_rotate_cpu.py, bit-equality across layouts and addressing, guard bands
around outputs written through the C entry points, and a poisoned workspace.  tests/test_map_edges_cpu.py shows that plain
fp32 arithmetic stays within half of each bound at every case.

Each parity test prints its worst figure before it asserts (pytest -s or -rA shows them)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import map_edge_cases as E
from tests.test_gpu_baseline_edges import Carved, _dev, _lib, _stream, _workspace
from tests.test_resample_cpu import np_gaussian_blur, np_resample, resample_bound
from tests.test_rotate_cpu import np_rotate_envmap, rotate_bound

pytestmark = pytest.mark.gpu

RESAMPLE_IDS = [f"{N}x{C}-{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}" for N, C, p in E.RESAMPLE_CASES]


def _t(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(_dev())  # (a copy: the builders' arrays are read-only)


def _shape_id(s):
    return f"{s[0]}x{s[1]}"


# ================================================================================================ 1. resampler
def c_resample(x, tables, size, out_ptr):
    """reni_resample through the C entry point: x [N, C, Hs, Ws] on the device with any strides, tables (ri, rw, ci, cw) numpy"""
    ri, rw, ci, cw = tables
    dev = [_t(ri, np.int32), _t(rw, np.float32), _t(ci, np.int32), _t(cw, np.float32)]
    N, C, Hs, Ws = x.shape
    lib = _lib()
    rc = lib.reni_resample(N, C, Hs, Ws, size[0], size[1], x.data_ptr(), (ctypes.c_int64 * 4)(*x.stride()), dev[0].data_ptr(),
                           dev[1].data_ptr(), ri.shape[1], dev[2].data_ptr(), dev[3].data_ptr(), ci.shape[1], out_ptr, _stream())
    assert rc == 0, lib.reni_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", E.RESAMPLE_CASES, ids=RESAMPLE_IDS)
def test_resample_edge_shapes_match_float64(case):
    from reni_amd import ops
    N, C, pair = case
    size = pair[1]
    x = E.resample_input(N, C, pair)
    xd = _t(x)
    worst = 0.0
    for mode in E.MODES:
        got = ops.resample(xd, size, mode)
        assert got.dtype == torch.float32 and tuple(got.shape) == (N, C) + tuple(size)
        err = np.abs(got.double().cpu().numpy() - np_resample(x, size, mode))
        bound = resample_bound(x, size, mode)
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print(f"resample {N}x{C} {pair[0]} -> {size} {mode}: largest err / bound {ratio:.3f}")
        assert np.all(err <= bound), mode
        assert torch.equal(got, ops.resample(xd, size, mode))
        if pair == E.IDENTITY_PAIR:
            assert torch.equal(got, xd), mode  # weights (.., 1, 0, ..) and the index d itself: the source's bits
    print(f"resample {N}x{C} {pair[0]} -> {size}: worst {worst:.3f}")


@pytest.mark.parametrize("sizes", E.TABLE_SIZES, ids=["37x91-50x23", "1x2-3x257"])
def test_tap_counts_with_real_weights_match_the_float64_table_sum(sizes):
    """every tap of every (ty, tx) carries a weight that matters: tx = 3, 5, 6, 7 through the generic instance, each register
    instance with a row count other than its own"""
    (hs, ws), size = sizes
    x = E.resample_input(2, 3, sizes)
    xd = _t(x)
    for ty, tx in E.GENERIC_TAPS + E.REGISTER_TAPS:
        tables = E.random_tables(hs, size[0], ty, 100 + ty) + E.random_tables(ws, size[1], tx, 200 + tx)
        out = torch.empty(2, 3, *size, device=_dev())
        c_resample(xd, tables, size, out.data_ptr())
        err = np.abs(out.double().cpu().numpy() - E.table_sum(x, *tables))
        bound = E.table_bound(x, *tables)
        print(f"tables ({ty}, {tx}) {hs}x{ws} -> {size}: largest err / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound), (ty, tx)


@pytest.mark.parametrize("sizes", E.TABLE_SIZES, ids=["37x91-50x23", "1x2-3x257"])
def test_a_table_is_trusted_for_weights_never_for_addresses(sizes):
    """indices from -3 to n_in + 4 give the bits of the same table clamped on the host (the kernel clamps every index it reads:
    in the register instances' preload, in the shared row loop and in the generic instance's column loop)"""
    (hs, ws), size = sizes
    xd = _t(E.resample_input(2, 3, sizes))
    for ty, tx in ((3, 5), (5, 3), (4, 2), (2, 8), (1, 1)):
        ri, rw = E.random_tables(hs, size[0], ty, 300 + ty, wild=True)
        ci, cw = E.random_tables(ws, size[1], tx, 400 + tx, wild=True)
        assert ri.min() == -3 and ri.max() == hs + 4 and ci.min() == -3 and ci.max() == ws + 4
        a, b = torch.empty(2, 3, *size, device=_dev()), torch.empty(2, 3, *size, device=_dev())
        c_resample(xd, (ri, rw, ci, cw), size, a.data_ptr())
        c_resample(xd, (np.clip(ri, 0, hs - 1), rw, np.clip(ci, 0, ws - 1), cw), size, b.data_ptr())
        assert torch.equal(a, b), (ty, tx)


@pytest.mark.parametrize("mode", E.MODES)
def test_resample_reads_a_stride_zero_channel_like_its_copy(mode):
    from reni_amd import ops
    x = _t(E.maps(2, 3, 8, 8, 16))[:, :1].expand(-1, 3, -1, -1)
    assert x.stride(1) == 0
    for size in ((7, 9), (17, 15)):
        got = ops.resample(x, size, mode)
        assert torch.equal(got, ops.resample(x.contiguous(), size, mode))
        assert torch.equal(got[:, 0], got[:, 2])


@pytest.mark.parametrize("target", E.CARVED_TARGETS, ids=_shape_id)
def test_resample_stores_nothing_beyond_its_output(target):
    """255, 256 and 257 output pixels between guard bands: the lanes of the last block beyond the image store nothing"""
    from reni_amd import ops
    src = (5, 9)
    xd = _t(E.maps(2, 3, *src, 14))
    for mode in ("bilinear", "lanczos4"):
        tables = E.mode_tables((src, target), mode)
        out = Carved(2, 3, *target)
        c_resample(xd, tables, target, out.ptr)
        out.check(ops.resample(xd, target, mode), f"resample {mode} -> {target}")
    tables = E.random_tables(src[0], target[0], 3, 1) + E.random_tables(src[1], target[1], 5, 2)
    out, plain = Carved(2, 3, *target), torch.empty(2, 3, *target, device=_dev())
    c_resample(xd, tables, target, out.ptr)
    c_resample(xd, tables, target, plain.data_ptr())
    out.check(plain, f"resample (3, 5) taps -> {target}")


# ================================================================================================ 2. blur
@pytest.mark.parametrize("shape", E.BLUR_SHAPES, ids=_shape_id)
def test_blur_edge_shapes_match_float64_per_pixel(shape):
    """against np_gaussian_blur with a float64 intermediate, within E.blur_bound at every pixel (its docstring derives it);
    radius 0 returns the image's bits; the three layouts give the same bits"""
    from reni_amd import ops
    H, W = shape
    worst, where = 0.0, None
    for C in E.BLUR_CHANNELS:
        for n in range(2):
            img = E.blur_image(C, H, W, n)
            t = _t(img)
            planar = t.permute(2, 0, 1).contiguous()
            for sigma in E.BLUR_SIGMAS:
                got = ops.gaussian_blur(t, sigma, layout="hwc")
                assert got.shape == t.shape and got.dtype == torch.float32
                err = np.abs(got.double().cpu().numpy() - np_gaussian_blur(img, sigma, fp32_intermediate=False))
                bound = E.blur_bound(img, sigma)
                ratio = float((err / bound).max())
                if ratio > worst:
                    worst, where = ratio, (C, n, sigma)
                assert np.all(err <= bound), (C, n, sigma, ratio)
                if E.blur_radius(sigma) == 0:
                    assert torch.equal(got, t)
                assert torch.equal(ops.gaussian_blur(planar, sigma, layout="chw"), got.permute(2, 0, 1)), (C, n, sigma)
                assert torch.equal(ops.gaussian_blur(planar[C - 1], sigma), got[:, :, C - 1]), (C, n, sigma)  # [H, W]
    print(f"blur {H}x{W}: largest err / bound {worst:.3f} at (C, map, sigma) = {where}")


@pytest.mark.parametrize("shape", E.BLUR_WORKSPACE_SHAPES, ids=_shape_id)
def test_blur_with_a_poisoned_workspace_and_a_carved_output(shape):
    """the intermediate is written before it is read, whatever the workspace held (0xFF bytes: NaN), and the last block's lanes
    beyond the image store nothing"""
    from reni_amd import ops
    from reni_amd.resample import gaussian_weights
    H, W = shape
    t = _t(E.blur_image(3, H, W, 1))  # [H, W, 3]
    lib = _lib()
    for sigma in (0.1, 3, 12.3):
        w, r = gaussian_weights(sigma)
        wd = _t(w, np.float32)
        ws, wp, wn = _workspace(int(lib.reni_blur_workspace_bytes(3, H, W)), 0xFF)
        out = Carved(H, W, 3)
        rc = lib.reni_gaussian_blur(3, H, W, t.data_ptr(), (ctypes.c_int64 * 3)(1, 3 * W, 3), wd.data_ptr(), r, out.ptr, wp, wn,
                                    _stream())
        assert rc == 0, lib.reni_last_error()
        out.check(ops.gaussian_blur(t, sigma, layout="hwc"), f"blur {H}x{W} sigma {sigma}")


# ================================================================================================ 3. rotation
def _rot(R):
    return _t(R, np.float32)


@pytest.mark.parametrize("shape", E.ROTATE_SHAPES, ids=_shape_id)
def test_rotate_bilinear_edge_shapes_match_float64(shape):
    from reni_amd import ops
    H, W = shape
    worst, where = 0.0, None
    for C in ((3, 1, 5) if shape == E.ROTATE_CHANNEL_SHAPE else (3,)):
        x = E.rotate_input(H, W, C)
        xd = _t(x)
        for name, R32, yaw in E.bilinear_rotations(H, W):
            got = ops.rotate_envmap(xd, _rot(R32)).double().cpu().numpy()
            ref = np_rotate_envmap(x, R32)
            bound, keep = rotate_bound(x, R32)
            assert got.shape == ref.shape == (2, C, H, W)
            left = int((~keep).sum())
            assert left == 0 if yaw else left * H <= 2 * H * W, (name, left)
            ratio = float((np.abs(got - ref) / bound)[..., keep].max())
            if ratio > worst:
                worst, where = ratio, (C, name)
            assert ratio <= 1.0, (C, name, ratio)
            assert np.isfinite(got).all()
            for n in range(2):  # every pixel, the caps included: a convex combination of source pixels
                assert got[n].min() >= x[n].min() and got[n].max() <= x[n].max(), (C, name)
    print(f"rotate bilinear {H}x{W}: largest err / bound {worst:.3f} at (C, rotation) = {where}")


@pytest.mark.parametrize("shape", [s for s in E.ROTATE_SHAPES if s[0] >= E.GENERAL_MIN_H], ids=_shape_id)
def test_rotate_bilinear_taps_beyond_a_pole_are_compared(shape):
    """rotate_bound's keep leaves out the half row round each pole, which is where a tap read on the far side carries weight;
    E.pole_pixels (its docstring gives the reason) compares those cells down to a quarter of that distance, with the same bound"""
    from reni_amd import ops
    from tests.test_rotate_cpu import rotation_list
    H, W = shape
    x = E.rotate_input(H, W)
    xd = _t(x)
    count, worst, where = 0, 0.0, None
    for name, R in rotation_list():
        R32 = R.astype(np.float32)
        pole = E.pole_pixels(H, W, R32)
        if not pole.any():
            continue
        count += int(pole.sum())
        got = ops.rotate_envmap(xd, _rot(R32)).double().cpu().numpy()
        bound, _ = rotate_bound(x, R32)
        ratio = float((np.abs(got - np_rotate_envmap(x, R32)) / bound)[..., pole].max())
        if ratio > worst:
            worst, where = ratio, name
        assert ratio <= 1.0, (name, ratio)
    print(f"rotate bilinear {H}x{W}, {count} pixels beyond a pole: largest err / bound {worst:.3f} at {where}")
    assert count >= 8


@pytest.mark.parametrize("shape", E.ROTATE_SHAPES, ids=_shape_id)
def test_rotate_nearest_half_turns_and_pixel_yaws_are_exact(shape):
    from reni_amd import ops
    x = E.rotate_input(*shape)
    xd = _t(x)
    for name, R, want in E.nearest_exact_cases(x):
        assert torch.equal(ops.rotate_envmap(xd, _rot(R), "nearest"), _t(want)), name


@pytest.mark.parametrize("shape", [s for s in E.ROTATE_SHAPES if s[0] >= E.GENERAL_MIN_H], ids=_shape_id)
def test_rotate_nearest_against_the_oracle(shape):
    """outside the polar caps a tap may differ from the float64 oracle's only where E.nearest_permitted allows it, which is
    nowhere at the listed cases (tests/test_map_edges_cpu.py): an equality.  Inside the caps (at most W pixels) the column is
    ill-conditioned; there the result is only required to be a source pixel of its map."""
    from reni_amd import ops
    H, W = shape
    x = E.rotate_input(H, W)
    xd = _t(x)
    in_caps = 0
    for name, R in E.nearest_rotations():
        R32 = R.astype(np.float32)
        got = ops.rotate_envmap(xd, _rot(R32), "nearest").cpu().numpy()
        ref = np_rotate_envmap(x, R32, "nearest")
        permitted, keep, _ = E.nearest_permitted(H, W, R32)
        differ = (got != ref).any(axis=(0, 1))
        assert not (differ & keep & ~permitted).any(), (name, np.argwhere(differ & keep & ~permitted)[:5].tolist())
        in_caps += int((differ & ~keep).sum())
        for n in range(2):
            assert np.isin(got[n], x[n]).all(), name
    print(f"rotate nearest {H}x{W}: pixels inside the caps that differ from the oracle, over all rotations: {in_caps}")


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("shape", ((1, 2), (3, 10), (9, 30)), ids=_shape_id)
def test_rotate_addressing_changes_no_bit(shape, mode):
    from reni_amd import ops
    from tests.test_rotate_cpu import rotation_list
    H, W = shape
    xd = _t(E.rotate_input(H, W))
    Rs = torch.stack([_rot(R) for _, R in rotation_list()[:7]])
    full = ops.rotate_envmap(xd, Rs[:2], mode)
    last = xd.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(ops.rotate_envmap(last, Rs[:2], mode, layout="hwc"), full)
    zero = xd[:, :1].expand(-1, 3, -1, -1)
    assert zero.stride(1) == 0
    assert torch.equal(ops.rotate_envmap(zero, Rs[:2], mode), ops.rotate_envmap(zero.contiguous(), Rs[:2], mode))
    idx = torch.tensor(E.INDEX_B7, device=_dev())
    via = ops.rotate_envmap(xd, Rs, mode, index=idx)  # B = 7 from N = 2
    assert via.shape == (7, 3, H, W)
    for b, n in enumerate(E.INDEX_B7):
        assert torch.equal(via[b], ops.rotate_envmap(xd[n], Rs[b], mode, layout="chw")), b


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_rotate_stores_nothing_beyond_its_output(mode):
    """7 x 36 = 252 pixels: the last four lanes of the block store nothing"""
    from reni_amd import _lib as L, ops
    from tests.test_rotate_cpu import rotation_list
    H, W = E.ROTATE_CARVED_SHAPE
    xd = _t(E.rotate_input(H, W))
    Rs = torch.stack([_rot(R) for _, R in rotation_list()[1:3]])
    rt, ct = ops._rotate_trig(H, W, xd.device)
    out = Carved(2, 3, H, W)
    lib = _lib()
    rc = lib.reni_rotate_envmap(2, 3, H, W, xd.data_ptr(), (ctypes.c_int64 * 4)(*xd.stride()), None, 2, Rs.data_ptr(), 9,
                                rt.data_ptr(), ct.data_ptr(), L.ROTATE_MODE[mode], out.ptr, _stream())
    assert rc == 0, lib.reni_last_error()
    out.check(ops.rotate_envmap(xd, Rs, mode), f"rotate {mode} {H}x{W}")


def test_a_non_finite_matrix_never_becomes_an_address():
    """NaN, inf, overflow and the zero matrix: the row and column are clamped before they are taps (fminf / fmaxf drop a NaN),
    sph_taps' fold and wraps keep every tap inside the map.  The output is finite and every value lies
    within its source map's range."""
    from reni_amd import ops
    for H, W in E.NONFINITE_SHAPES:
        x = E.rotate_input(H, W)
        xd = _t(x)
        for mode in ("bilinear", "nearest"):
            for name, R in E.NONFINITE:
                got = ops.rotate_envmap(xd, _rot(R), mode)
                torch.cuda.synchronize()
                got = got.cpu().numpy()
                assert np.isfinite(got).all(), (H, W, mode, name)
                for n in range(2):
                    assert got[n].min() >= x[n].min() and got[n].max() <= x[n].max(), (H, W, mode, name)
