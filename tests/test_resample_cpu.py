"""CPU tests of the resampling / blur tables (reni_amd/resample.py), the C ABI argument checks of reni_tu_resample.hip and
the batched normalise, and the unit's ISA audit.

Holds the float64 oracles tests/test_gpu_resample.py and tests/test_gpu_resident.py compare the HIP kernels against: the
separable table sum (np_resample), the weighted-sum error bound (resample_bound) and scipy's gaussian_filter restated from
its table and reflect indices (np_gaussian_blur), checked here against torch's float64 F.interpolate, utils.mask_from_array,
the Lanczos closed form, the golden made from the reference's blurIBL (tests/golden/make_g25_resample.py) and scipy itself."""
import ctypes
import math
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import isa_audit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G25 = os.path.join(ROOT, "tests", "golden", "g25_resample.npz")
SIZE_PAIRS = (((50, 100), (16, 32)), ((64, 128), (16, 32)), ((37, 91), (64, 128)), ((16, 32), (300, 600)),
              ((1024, 2048), (64, 128)))
SIGMAS = (1, 3, 5)
EPS32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------ float64 oracles
def np_resample(src, size, mode, fp32_weights=False, absolute=False):
    """src [..., Hs, Ws] float64 -> [..., Hd, Wd]: the separable table sum in float64.  fp32_weights: the weights rounded to
    fp32 first, as the device holds them.  absolute: sum |w| |w| |src| instead (the magnitude the rounding errors scale with)."""
    from reni_amd.resample import resample_tables
    src = np.asarray(src, np.float64)
    ri, rw = resample_tables(src.shape[-2], size[0], mode)
    ci, cw = resample_tables(src.shape[-1], size[1], mode)
    if fp32_weights:
        rw, cw = rw.astype(np.float32).astype(np.float64), cw.astype(np.float32).astype(np.float64)
    if absolute:
        src, rw, cw = np.abs(src), np.abs(rw), np.abs(cw)
    rows = sum(src[..., ri[:, j], :] * rw[:, j][:, None] for j in range(ri.shape[1]))      # [..., Hd, Ws]
    return sum(rows[..., :, ci[:, k]] * cw[:, k] for k in range(ci.shape[1]))             # [..., Hd, Wd]


def resample_bound(src, size, mode):
    """Elementwise bound on |fp32 device result - float64 table sum|: (taps_y + taps_x + 4) 2^-24 A with A the same double sum
    over |w| |w| |src|.  Each weight is rounded to fp32 once (2 relative errors of 2^-24 per term), the inner chain of taps_x
    fmaf and the outer chain of taps_y fmaf add one rounding per step, and two more cover the products' second-order terms."""
    from reni_amd.resample import TAPS
    return (2 * TAPS[mode] + 4) * EPS32 * np_resample(src, size, mode, absolute=True)


def np_gaussian_blur(img, sigma, fp32_intermediate=True):
    """scipy.ndimage.gaussian_filter(channel, sigma) of img [H, W] or [H, W, C] restated: table + reflect indices, axis 0 then
    axis 1, float64 sums; scipy stores the intermediate in the input's dtype (fp32 for an fp32 map)."""
    from reni_amd.resample import gaussian_weights, reflect_indices
    x = np.asarray(img, np.float64)
    w, r = gaussian_weights(sigma)
    H, W = x.shape[:2]
    iy, ix = reflect_indices(H, r), reflect_indices(W, r)
    mid = sum(x[iy[:, t]] * w[t] for t in range(2 * r + 1))
    if fp32_intermediate:
        mid = mid.astype(np.float32).astype(np.float64)
    return sum(mid[:, ix[:, t]] * w[t] for t in range(2 * r + 1))


def blur_bound(img, sigma):
    """(2 r + 3) 2^-24 max|img|: scipy keeps its intermediate (and its result) in fp32"""
    r = int(4.0 * sigma + 0.5)
    return (2 * r + 3) * EPS32 * float(np.abs(np.asarray(img, np.float64)).max())


def exact_coordinate(d, n_in, n_out):
    return Fraction((2 * d + 1) * n_in - n_out, 2 * n_out)


# ------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
@pytest.mark.parametrize("pair", SIZE_PAIRS)
def test_tables_match_torch_float64_interpolate(mode, pair):
    (hs, ws), (hd, wd) = pair
    g = np.random.default_rng(hs * 7 + wd)
    x = g.random((2, 3, hs, ws)) + 0.05
    ref = torch.nn.functional.interpolate(torch.from_numpy(x), size=(hd, wd), mode=mode, align_corners=False).numpy()
    got = np_resample(x, (hd, wd), mode)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"{mode} {hs}x{ws} -> {hd}x{wd}: rel err vs torch float64 {err:.3e}")
    assert err <= 1e-12


def test_bilinear_and_bicubic_tables_follow_the_exact_rational_coordinate():
    from reni_amd.resample import cubic_weights, resample_tables
    for n_in, n_out in ((50, 16), (37, 64), (16, 300), (2048, 128), (5, 5), (1, 7), (7, 1)):
        bi, bw = resample_tables(n_in, n_out, "bilinear")
        ci, cw = resample_tables(n_in, n_out, "bicubic")
        assert bi.shape == (n_out, 2) and ci.shape == (n_out, 4)
        for d in range(n_out):
            x = exact_coordinate(d, n_in, n_out)
            xb = max(x, Fraction(0))
            i0 = math.floor(xb)
            assert tuple(bi[d]) == (min(i0, n_in - 1), min(i0 + 1, n_in - 1))
            assert abs(bw[d, 1] - float(xb - i0)) <= 1e-15 and abs(bw[d].sum() - 1.0) <= 1e-15
            i0 = math.floor(x)
            assert tuple(ci[d]) == tuple(min(max(i0 - 1 + k, 0), n_in - 1) for k in range(4))
            assert np.abs(cw[d] - cubic_weights(float(x - i0))).max() <= 1e-15 and abs(cw[d].sum() - 1.0) <= 1e-14
    assert np.array_equal(cubic_weights(0.0), [0.0, 1.0, 0.0, 0.0])


def test_nearest_indices_equal_mask_from_array_for_every_size():
    """source sizes 1 .. 599, targets {8, 12, 16, 32, 64, 100, 128, 256}: the fp32 product rule, including the pairs where it
    differs from the exact integer floor"""
    from reni_amd.resample import resample_tables
    from reni_amd.utils import mask_from_array
    differ = 0
    for n_out in (8, 12, 16, 32, 64, 100, 128, 256):
        for n_in in range(1, 600):
            idx, w = resample_tables(n_in, n_out, "nearest")
            assert idx.shape == (n_out, 1) and np.all(w == 1.0)
            # a source whose pixel value is its own column index (mod 256), one row: mask_from_array's gather shows its indices
            ramp = (np.arange(n_in) % 256).astype(np.uint8)[None, :].repeat(2, 0)
            m = mask_from_array(n_out, ramp)[0].reshape(n_out // 2, n_out, 3)[0, :, 0].numpy()
            assert np.array_equal(np.round(m * 255).astype(np.int64), idx[:, 0] % 256), (n_in, n_out)
            exact = np.minimum(np.arange(n_out) * n_in // n_out, n_in - 1)
            differ += int(not np.array_equal(exact, idx[:, 0]))
    print(f"pairs where the fp32 product differs from the exact floor: {differ} of {8 * 599}")
    assert differ > 0  # the rule is not the exact floor; a builder that used it would pass the loop above only by luck


def test_lanczos4_weights():
    from reni_amd.resample import lanczos4_weights, resample_tables
    assert np.array_equal(lanczos4_weights(0.0), [0, 0, 0, 1, 0, 0, 0, 0])
    for t in (0.125, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.999):
        w = lanczos4_weights(t)
        x = t + 3.0 - np.arange(8)
        closed = np.sinc(x) * np.sinc(x / 4.0)
        closed = closed / closed.sum()
        assert abs(w.sum() - 1.0) <= 1e-15
        assert np.abs(w - closed).max() <= 1e-15
    for n_in, n_out in ((32, 600), (16, 300), (600, 32), (37, 91), (8, 8)):
        idx, w = resample_tables(n_in, n_out, "lanczos4")
        assert idx.shape == (n_out, 8) and np.abs(w.sum(1) - 1.0).max() <= 1e-15
        assert idx.min() >= 0 and idx.max() <= n_in - 1
        for d in range(n_out):
            x = exact_coordinate(d, n_in, n_out)
            i0 = math.floor(x)
            assert tuple(idx[d]) == tuple(min(max(i0 - 3 + k, 0), n_in - 1) for k in range(8))
            assert np.abs(w[d] - lanczos4_weights(float(x - i0))).max() <= 1e-15
    idx, w = resample_tables(8, 8, "lanczos4")  # same size: every output sits on a sample
    assert np.array_equal(w, np.tile([0, 0, 0, 1, 0, 0, 0, 0], (8, 1))) and np.array_equal(idx[:, 3], np.arange(8))


def test_table_builder_rejects_bad_arguments():
    from reni_amd.resample import gaussian_weights, resample_tables
    with pytest.raises(ValueError):
        resample_tables(0, 4, "bilinear")
    with pytest.raises(ValueError):
        resample_tables(4, 0, "bilinear")
    with pytest.raises(ValueError):
        resample_tables(4, 4, "area")
    for s in (0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gaussian_weights(s)


# ------------------------------------------------------------------------------------------ blur
def test_blur_restatement_matches_the_reference_golden():
    g = np.load(G25)
    for k in range(2):
        img = g[f"blur_img{k}"]
        assert img.dtype == np.float32 and img.ndim == 3
        for s in SIGMAS:
            ref = g[f"blur_img{k}_s{s}"]
            got = np_gaussian_blur(img, s)
            err, bound = float(np.abs(got - ref).max()), blur_bound(img, s)
            print(f"blur map {k} sigma {s}: err {err:.3e} bound {bound:.3e}")
            assert ref.shape == img.shape and err <= bound


def test_blur_restatement_matches_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(25)
    for shape, s in (((16, 32), 1), ((16, 32), 3), ((5, 9), 5), ((32, 64), 2.5)):  # 5 x 9 at sigma 5: radius 20 > the image
        img = g.random(shape).astype(np.float32)
        ref = ndimage.gaussian_filter(img, sigma=s)
        got = np_gaussian_blur(img, s)
        assert float(np.abs(got - ref).max()) <= blur_bound(img, s)


def test_reflect_indices_and_gaussian_weights():
    from reni_amd.resample import gaussian_weights, reflect_indices
    idx = reflect_indices(4, 6)
    assert list(idx[0]) == [2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1]  # ... d c b a | a b c d | d c b a ...
    w, r = gaussian_weights(5)
    assert r == 20 and w.shape == (41,) and abs(w.sum() - 1) <= 1e-15 and np.array_equal(w, w[::-1])
    assert gaussian_weights(0.1)[1] == 0 and gaussian_weights(1)[1] == 4 and gaussian_weights(3)[1] == 12


# ------------------------------------------------------------------------------------------ ISA audit, C ABI checks
def test_resample_translation_unit_isa_audit():
    """reni_tu_resample.hip with build.sh's flags: kernels present, no hazard, no scratch"""
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "resample.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_resample.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    for k in ("k_resample", "k_blur_axis"):
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.valu_to_mfma(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) >= 6 and all(int(x) == 0 for x in sizes)  # five k_resample instances and k_blur_axis


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    from reni_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 255) & ~255
    st4 = (ctypes.c_int64 * 4)(0, 1, 24, 3)

    def rs(N=1, C=3, Hs=4, Ws=8, Hd=2, Wd=4, ptrs=(p,) * 6, strides=st4, ty=2, tx=2):
        return lib.reni_resample(N, C, Hs, Ws, Hd, Wd, ptrs[0], strides, ptrs[1], ptrs[2], ty, ptrs[3], ptrs[4], tx, ptrs[5], None)

    for kw in (dict(N=0), dict(C=0), dict(Hs=0), dict(Ws=0), dict(Hd=0), dict(Wd=-1), dict(N=1 << 17), dict(Hd=1 << 16, Wd=1 << 16),
               dict(Hs=1 << 16, Ws=1 << 16), dict(ty=0), dict(ty=9), dict(tx=0), dict(tx=9), dict(tx=-1)):
        assert rs(**kw) == -1, kw
    for k in range(6):
        ptrs = [p] * 6
        ptrs[k] = None
        assert rs(ptrs=ptrs) == -1 and b"NULL" in lib.reni_last_error()
    assert rs(strides=None) == -1
    assert rs(strides=(ctypes.c_int64 * 4)(0, 1, -24, 3)) == -1

    st3 = (ctypes.c_int64 * 3)(1, 24, 3)

    def blur(C=3, H=4, W=8, ptrs=(p,) * 3, strides=st3, radius=4, ws=p, wsb=4096):
        return lib.reni_gaussian_blur(C, H, W, ptrs[0], strides, ptrs[1], radius, ptrs[2], ws, wsb, None)

    for kw in (dict(C=0), dict(H=0), dict(W=0), dict(C=1 << 17), dict(H=1 << 16, W=1 << 16), dict(radius=-1), dict(radius=1 << 21),
               dict(strides=None), dict(strides=(ctypes.c_int64 * 3)(1, -24, 3))):
        assert blur(**kw) == -1, kw
    for k in range(3):
        ptrs = [p] * 3
        ptrs[k] = None
        assert blur(ptrs=ptrs) == -1 and b"NULL" in lib.reni_last_error()
    assert lib.reni_blur_workspace_bytes(3, 4, 8) >= 3 * 4 * 8 * 4 and lib.reni_blur_workspace_bytes(0, 4, 8) == 0
    assert blur(ws=None, wsb=0) == -2 and blur(ws=p + 4) == -2 and blur(wsb=16) == -2

    def norm(N=2, n=16, ptrs=(p, p), m0=-1.0, m1=1.0, ws=p, wsb=4096):
        return lib.reni_minmax_normalise_batch(N, n, ptrs[0], m0, m1, 1, ptrs[1], ws, wsb, None)

    for kw in (dict(N=0), dict(n=0), dict(N=1 << 17), dict(n=1 << 31), dict(ptrs=(None, p)), dict(ptrs=(p, None)),
               dict(m0=1.0, m1=1.0), dict(m0=2.0, m1=1.0), dict(m1=float("nan"))):
        assert norm(**kw) == -1, kw
    assert lib.reni_minmax_batch_workspace_bytes(4) >= 32 and lib.reni_minmax_batch_workspace_bytes(0) == 0
    assert norm(ws=None, wsb=0) == -2 and norm(ws=p + 4) == -2 and norm(wsb=8) == -2


def test_new_ops_have_no_cpu_fallback(tmp_path):
    from reni_amd import _lib, baselines, ops
    from reni_amd.custom_transforms import transform_builder
    from reni_amd.data import RENIDatasetHDR, ResidentDataset
    from reni_amd import exr
    x = torch.ones(3, 8, 16)
    with pytest.raises(_lib.RENILibraryError):
        ops.resample(x, (4, 8), "bilinear")
    with pytest.raises(_lib.RENILibraryError):
        ops.minmax_normalise_batch(x[None], (-1.0, 1.0))
    with pytest.raises(_lib.RENILibraryError):
        ops.gaussian_blur(x, 1.0)
    exr.write_exr(str(tmp_path / "a.exr"), np.ones((8, 16, 3), np.float32) * 2, pixel_type="half", compression="zip")
    exr.write_exr(str(tmp_path / "b.exr"), np.ones((8, 16, 3), np.float32), pixel_type="half", compression="zip")
    ds = RENIDatasetHDR(str(tmp_path), transform_builder([["resize", [4, 8]], ["minmaxnormalise", []]]))
    with pytest.raises(_lib.RENILibraryError):
        ResidentDataset(ds, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RENILibraryError):
            ResidentDataset(ds)
        with pytest.raises(_lib.RENILibraryError):
            baselines.resizeImage(np.ones((8, 16, 3), np.float32), 8, 4)
        with pytest.raises(_lib.RENILibraryError):
            baselines.blurIBL(np.ones((8, 16, 3), np.float32), 1)
    with pytest.raises(NotImplementedError):
        baselines.resizeImage(np.ones((8, 16, 3), np.float32), 8, 4, interpolation="max_pooling")
    assert baselines.INTER_CUBIC == 2 and baselines.INTER_LANCZOS4 == 4
