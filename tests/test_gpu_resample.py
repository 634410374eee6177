"""GPU parity of the resampler, the batched normalise and the blur (reni_tu_resample.hip, reni_tu_image.hip) against the
float64 oracles of tests/test_resample_cpu.py, with bounds derived from the number formats (see resample_bound, blur_bound),
and bit-equality across calls and across batch positions."""
import os

import numpy as np
import pytest
import torch

from tests.test_resample_cpu import G25, SIGMAS, blur_bound, np_gaussian_blur, np_resample, resample_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("nearest", "bilinear", "bicubic", "lanczos4")
# (source H, W) -> (target H, W): a large shrink, a portrait shrink, a large upsample, a ragged pair, an identity
PAIRS = (((1024, 2048), (64, 128)), ((600, 300), (32, 16)), ((16, 32), (300, 600)), ((37, 91), (50, 23)), ((16, 32), (16, 32)))


def _maps(n, hs, ws, seed):
    """[n, 3, hs, ws] float32: positive sky-like maps with a bright spot (five decades of range) and, in map 1, negatives"""
    g = np.random.default_rng(seed)
    x = 0.05 + g.random((n, 3, hs, ws))
    x[:, :, hs // 3, (2 * ws) // 3] = 2000.0
    if n > 1:
        x[1] -= 0.5
    return x.astype(np.float32)


def _check(got, x, size, mode, what):
    ref = np_resample(x.astype(np.float64), size, mode)  # float64 weights: the bound covers their rounding to fp32 too
    bound = resample_bound(x, size, mode)
    err = np.abs(got.double().cpu().numpy() - ref)
    rel = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what} {mode} {x.shape[-2:]} -> {size}: max err {float(err.max()):.3e}, largest err / bound {rel:.3f}")
    assert got.dtype == torch.float32 and tuple(got.shape[-2:]) == tuple(size)
    assert np.all(err <= bound)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pair", PAIRS)
def test_resample_against_the_float64_table_oracle(mode, pair):
    from reni_amd import ops
    (hs, ws), size = pair
    x = _maps(2, hs, ws, hs + ws)
    planar = torch.from_numpy(x).to(DEV)
    a = ops.resample(planar, size, mode)
    assert a.shape == (2, 3) + tuple(size)
    _check(a, x, size, mode, "planar")
    assert torch.equal(a, ops.resample(planar, size, mode))  # two calls, the same bits
    last = planar.permute(0, 2, 3, 1).contiguous()  # [N, H, W, 3]
    b = ops.resample(last, size, mode, layout="hwc")
    assert torch.equal(a, b)  # the layout changes addresses, not arithmetic
    one = ops.resample(last[1], size, mode, layout="hwc")  # [H, W, 3] -> [3, Hd, Wd]
    assert one.shape == (3,) + tuple(size) and torch.equal(one, a[1])
    ch = ops.resample(planar[0, 2], size, mode)  # [H, W] -> [Hd, Wd]
    assert ch.shape == tuple(size) and torch.equal(ch, a[0, 2])
    if tuple(size) == (hs, ws) and mode != "nearest":
        assert torch.equal(a, planar)  # weights (.., 1, 0, ..): an identity


@pytest.mark.parametrize("mode", MODES)
def test_an_image_gives_the_same_bits_alone_and_inside_a_batch(mode):
    from reni_amd import ops
    x = torch.from_numpy(_maps(5, 64, 128, 5)).to(DEV)
    for size in ((16, 32), (100, 200)):
        full = ops.resample(x, size, mode)
        for n in (0, 3, 4):
            assert torch.equal(ops.resample(x[n:n + 1], size, mode)[0], full[n])
            assert torch.equal(ops.resample(x[n], size, mode), full[n])
    strided = x[:, :, ::2, 1::3]  # any non-negative strides are read in place
    assert torch.equal(ops.resample(strided, (16, 32), mode), ops.resample(strided.contiguous(), (16, 32), mode))


def test_tap_counts_without_an_instance_of_their_own_take_the_generic_one():
    """reni_resample accepts 1..8 taps per axis; 1, 2, 4 and 8 have register instances.  Bilinear tables padded with a
    zero-weight tap (3 per axis) and with three (5 per axis) go through the generic instance and add exact zeros: same bits."""
    import ctypes
    from reni_amd import _lib, ops
    from reni_amd.resample import resample_tables
    x = torch.from_numpy(_maps(2, 37, 91, 9)).to(DEV)
    size = (50, 23)
    want = ops.resample(x, size, "bilinear")
    lib = _lib.load()
    for pad in (1, 3):
        tabs = []
        for n_in, n_out in ((37, size[0]), (91, size[1])):
            idx, w = resample_tables(n_in, n_out, "bilinear")
            idx = np.concatenate([idx, np.repeat(idx[:, :1], pad, 1)], 1).astype(np.int32)
            w = np.concatenate([w, np.zeros((n_out, pad))], 1).astype(np.float32)
            tabs += [torch.from_numpy(idx).to(DEV), torch.from_numpy(w).to(DEV)]
        out = torch.empty(2, 3, *size, device=DEV)
        st = (ctypes.c_int64 * 4)(*x.stride())
        rc = lib.reni_resample(2, 3, 37, 91, size[0], size[1], x.data_ptr(), st, tabs[0].data_ptr(), tabs[1].data_ptr(), 2 + pad,
                               tabs[2].data_ptr(), tabs[3].data_ptr(), 2 + pad, out.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(out, want), pad


def test_bilinear_bound_on_positive_maps_is_what_the_formats_give():
    """on a positive map A equals the result itself, so the bound is (2 + 2 + 4) 2^-24 = 4.8e-7 relative"""
    from reni_amd import ops
    x = np.random.default_rng(3).random((1, 3, 128, 256)).astype(np.float32) + 0.1
    got = ops.resample(torch.from_numpy(x).to(DEV), (16, 32), "bilinear").double().cpu().numpy()
    ref = np_resample(x.astype(np.float64), (16, 32), "bilinear")
    rel = float((np.abs(got - ref) / ref).max())
    print(f"bilinear 128x256 -> 16x32 on a positive map: max relative error {rel:.3e} (bound 4.77e-7)")
    assert rel <= 8 * 2.0 ** -24
    t = torch.nn.functional.interpolate(torch.from_numpy(x).double(), size=(16, 32), mode="bilinear", align_corners=False).numpy()
    assert float((np.abs(got - t) / t).max()) <= 8 * 2.0 ** -24 + 1e-12


@pytest.mark.parametrize("sidelen", [32, 64, 128, 256, 48, 100, 200])
def test_nearest_equals_mask_from_array_on_the_golden_masks(sidelen, golden):
    from reni_amd import ops
    from reni_amd.utils import mask_from_array
    masks = golden("masks.npz")
    assert len(masks) >= 5
    for name, m in masks.items():
        assert m.shape[:2] == (256, 512)
        want = mask_from_array(sidelen, m)  # [1, P, 3]
        src = torch.from_numpy(np.asarray(m).astype(np.float32) / 255.0).to(DEV)  # [256, 512, 3], read channel-last in place
        got = ops.resample(src, (sidelen // 2, sidelen), "nearest", layout="hwc")  # [3, Hd, Wd]
        got = got.permute(1, 2, 0).reshape(-1, 3).unsqueeze(0)
        assert torch.equal(got.cpu(), want), (name, sidelen)


def test_gaussian_blur_against_the_reference_golden():
    from reni_amd import ops
    g = np.load(G25)
    for k in range(2):
        img = g[f"blur_img{k}"]
        t = torch.from_numpy(img).to(DEV)
        for s in SIGMAS:
            got = ops.gaussian_blur(t, s)
            assert got.shape == t.shape and got.dtype == torch.float32 and got.stride() == t.stride()
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - g[f"blur_img{k}_s{s}"]).max())
            bound = 2 * blur_bound(img, s)  # scipy's own fp32 intermediate, and this kernel's fp32 accumulation
            print(f"blur map {k} sigma {s}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound
            assert float(np.abs(got.cpu().numpy() - np_gaussian_blur(img, s)).max()) <= bound
            assert torch.equal(got, ops.gaussian_blur(t, s))
            planar = t.permute(2, 0, 1).contiguous()
            assert torch.equal(ops.gaussian_blur(planar, s, layout="chw"), got.permute(2, 0, 1))
            assert torch.equal(ops.gaussian_blur(t[:, :, 1].contiguous(), s), got[:, :, 1])


def test_minmax_normalise_batch_is_the_single_image_transform_per_image():
    from reni_amd import ops
    g = torch.Generator().manual_seed(7)
    x = torch.exp(torch.randn(4, 3, 16, 32, generator=g) * 2.0)
    x[0, 0, 0, 0] = 0.0
    x[1, 1, 2, 3] = -0.5
    x[2, 2, 4, 5] = float("inf")
    x[3, 0, 7, 9] = 4.0e4  # a spike: image 3's own upper clip bound
    x = x.to(DEV)
    mm = (-12.0, 11.0)
    for flag in (False, True):
        out = ops.minmax_normalise_batch(x, mm, nan_to_num=flag)
        assert out.shape == x.shape and out.dtype == torch.float32
        for n in range(4):
            assert torch.equal(out[n], ops.minmax_normalise(x[n], mm)), n
        assert torch.equal(out, ops.minmax_normalise_batch(x, mm, nan_to_num=flag))
    assert bool(torch.isfinite(out).all())
    x[1, 0, 1, 1] = float("nan")
    raw = ops.minmax_normalise_batch(x, mm, nan_to_num=False)
    out = ops.minmax_normalise_batch(x, mm, nan_to_num=True)
    assert bool(torch.isnan(raw[1, 0, 1, 1])) and int(torch.isnan(raw).sum()) == 1
    assert float(out[1, 0, 1, 1]) == 0.0 and not bool(torch.isnan(out).any())
    keep = ~torch.isnan(raw)
    assert torch.equal(out[keep], raw[keep])
    host = torch.nan_to_num(torch.stack([2 * (torch.clip(i, i[i > 0].min(), i[i < torch.inf].max()).log() - mm[0]) / (mm[1] - mm[0]) - 1
                                         for i in x.cpu()]))
    assert float((out.cpu() - host).abs().max()) <= 1e-5


def test_resize_image_and_blur_ibl_keep_the_references_call_shapes():
    from reni_amd import baselines
    g = np.random.default_rng(11)
    img = (0.05 + g.random((30, 60, 3))).astype(np.float32)
    for interp, mode in ((baselines.INTER_CUBIC, "bicubic"), (baselines.INTER_LANCZOS4, "lanczos4")):
        for (w, h) in ((20, 10), (150, 75)):
            out = baselines.resizeImage(img, w, h, interpolation=interp)
            assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (h, w, 3)
            x = np.ascontiguousarray(img.transpose(2, 0, 1))
            ref = np_resample(x.astype(np.float64), (h, w), mode).transpose(1, 2, 0)
            assert np.all(np.abs(out - ref) <= resample_bound(x, (h, w), mode).transpose(1, 2, 0))
    assert np.array_equal(baselines.resizeImage(img, 20, 10), baselines.resizeImage(img, 20, 10, baselines.INTER_CUBIC))
    assert baselines.resizeImage(img[:, :, 0], 20, 10).shape == (10, 20)
    ref = torch.nn.functional.interpolate(torch.from_numpy(img).double().permute(2, 0, 1)[None], size=(75, 150), mode="bicubic",
                                          align_corners=False)[0].permute(1, 2, 0).numpy()
    assert float(np.abs(baselines.resizeImage(img, 150, 75) - ref).max()) <= 12 * 2.0 ** -24 * 2.5  # sum |w| |w| |x| <= 1.6^2 max|x|
    with pytest.raises(NotImplementedError):
        baselines.resizeImage(img, 20, 10, interpolation="max_pooling")
    gold = np.load(G25)
    for s in SIGMAS:
        out = baselines.blurIBL(gold["blur_img1"], amount=s)
        assert out.dtype == np.float32 and out.shape == gold["blur_img1"].shape
        assert float(np.abs(out - gold[f"blur_img1_s{s}"]).max()) <= 2 * blur_bound(gold["blur_img1"], s)
    assert np.array_equal(baselines.blurIBL(gold["blur_img0"]), baselines.blurIBL(gold["blur_img0"], amount=5))


def test_a_2048_wide_map_reaches_the_sh_projection_through_resize_image():
    """getCoefficientsFromImage refuses maps wider than 1000 and says "resize the map first": resizeImage is that step"""
    from reni_amd import baselines
    yy, xx = np.meshgrid(np.linspace(0, 1, 1024), np.linspace(0, 1, 2048), indexing="ij")
    big = np.stack([1.0 + 0.5 * np.cos(2 * np.pi * xx), 0.8 + 0.2 * yy, 0.5 + 0.4 * np.sin(np.pi * yy)], -1).astype(np.float32)
    with pytest.raises(ValueError, match="resize the map first"):
        baselines.getCoefficientsFromImage(big, lmax=2)
    small = baselines.resizeImage(big, 1000, 500)
    assert small.shape == (500, 1000, 3)
    c = baselines.getCoefficientsFromImage(small, lmax=2)
    assert c.shape == (9, 3) and np.all(np.isfinite(c))
    # a smooth map: the coefficients of the resized map are those of a map sampled at 1000 x 500 directly
    yy, xx = np.meshgrid((np.arange(500) + 0.5) / 500 * (1024 / 1023) - 0.5 / 1023, (np.arange(1000) + 0.5) / 1000 * (2048 / 2047) - 0.5 / 2047,
                         indexing="ij")
    direct = np.stack([1.0 + 0.5 * np.cos(2 * np.pi * xx), 0.8 + 0.2 * yy, 0.5 + 0.4 * np.sin(np.pi * yy)], -1).astype(np.float32)
    c2 = baselines.getCoefficientsFromImage(direct, lmax=2)
    assert float(np.abs(c - c2).max()) <= 1e-3 * float(np.abs(c2).max())
