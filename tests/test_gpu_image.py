"""SURVEY.md section 8 row f3 on the GPU: the HDR epilogue reni_unnormalise_srgb / reni_minmax_normalise (reni_tu_image.hip)
against the reference's own outputs (golden G12: src/utils/custom_transforms.py:4-21 and src/utils/utils.py:30-42 run in
the build container) and, at BASELINE's image sizes, against the torch expressions of the same chain."""
import numpy as np
import pytest
import torch

from reni_amd import ops, utils
from reni_amd.custom_transforms import MinMaxNormalise, UnMinMaxNormlise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _srgb_torch(x):  # the reference chain on the host, fp32 (utils.py:30-42)
    q = torch.quantile(torch.quantile(torch.quantile(x, 0.98, dim=1), 0.98, dim=1), 0.98, dim=1)
    y = torch.clamp(x / q.view(-1, 1, 1, 1), 0.0, 1.0)
    return torch.where(y <= 0.0031308, 12.92 * y, 1.055 * torch.pow(torch.abs(y), 1 / 2.4) - 0.055)


def test_g12_unnormalise_and_srgb_match_the_reference(golden):
    g = golden("g12_transforms.npz")
    mm = [float(g["minmax"][0]), float(g["minmax"][1])]
    n = torch.from_numpy(g["normalised"]).to(DEV)                       # [3,16,32] log-normalised
    lin = UnMinMaxNormlise(mm)(n)
    assert lin.shape == n.shape and lin.is_cuda
    np.testing.assert_allclose(lin.cpu().numpy(), g["unnormalised"], rtol=3e-6, atol=0)
    # the fused call: un-normalise + nested 0.98 quantile + clamp + gamma == sRGB(UnMinMaxNormlise(x)) of the reference
    srgb, lin2 = ops.unnormalise_srgb(n, mm, srgb=True, want_linear=True)
    assert torch.equal(lin2[0], lin)
    np.testing.assert_allclose(srgb.cpu().numpy(), g["srgb1"], rtol=0, atol=2e-6)
    # plain sRGB of a linear batch (two images: per-image quantiles)
    x2 = (torch.rand(2, 3, 8, 16, generator=torch.Generator().manual_seed(13)) * 3.0).to(DEV)
    np.testing.assert_allclose(utils.sRGB(x2).cpu().numpy(), g["srgb2"], rtol=0, atol=2e-6)


def test_g12_minmax_normalise_matches_the_reference(golden):
    g = golden("g12_transforms.npz")
    mm = [float(g["minmax"][0]), float(g["minmax"][1])]
    img = torch.from_numpy(g["img"]).to(DEV)                            # holds a zero, an inf and a 1e4 spike
    n = MinMaxNormalise(mm)(img)
    np.testing.assert_allclose(n.cpu().numpy(), g["normalised"], rtol=0, atol=3e-7)


@pytest.mark.parametrize("B,H,W", [(3, 128, 256), (1, 512, 1024), (2, 33, 70)])
def test_model_output_layout_full_size(B, H, W):
    """A model output [B, H*W, 3] (channel-last) read in place, at BASELINE's grids and a ragged one."""
    g = torch.Generator().manual_seed(B * 1000 + H)
    out = (torch.rand(B, H * W, 3, generator=g) * 2 - 1)
    mm = [-18.0536, 11.4633]
    view = out.to(DEV).view(B, H, W, 3).permute(0, 3, 1, 2)              # strided [B,3,H,W], never copied
    srgb, lin = ops.unnormalise_srgb(view, mm, srgb=True, want_linear=True)
    lin_ref = torch.exp(0.5 * (out + 1) * (mm[1] - mm[0]) + mm[0]).view(B, H, W, 3).permute(0, 3, 1, 2)
    np.testing.assert_allclose(lin.cpu().numpy(), lin_ref.numpy(), rtol=3e-6, atol=0)
    # the quantile of the DEVICE's linear image (exp differs from the host's in the last bit, and a quantile picks elements)
    ref = _srgb_torch(lin.cpu())
    np.testing.assert_allclose(srgb.cpu().numpy(), ref.numpy(), rtol=0, atol=2e-6)
    # [B,P,3] through the transform class (the FIT_INVERSE call site, RENI_module.py:108)
    y = UnMinMaxNormlise(mm)(out.to(DEV))
    assert y.shape == (B, H * W, 3)
    assert torch.equal(y.view(B, H, W, 3).permute(0, 3, 1, 2), lin)


def test_unnormalise_is_differentiable_on_the_device():
    """FIT_INVERSE back-propagates through the un-normalisation (RENI_module.py:108-112)."""
    mm = [-18.0536, 11.4633]
    x = (torch.rand(2, 50, 3, generator=torch.Generator().manual_seed(5)) * 2 - 1)
    xd = x.to(DEV).requires_grad_(True)
    w = torch.rand(2, 50, 3, generator=torch.Generator().manual_seed(6))
    (UnMinMaxNormlise(mm)(xd) * w.to(DEV)).sum().backward()
    xc = x.clone().requires_grad_(True)
    (torch.exp(0.5 * (xc + 1) * (mm[1] - mm[0]) + mm[0]) * w).sum().backward()
    np.testing.assert_allclose(xd.grad.cpu().numpy(), xc.grad.numpy(), rtol=5e-6)


def test_ties_and_constant_images():
    """Order statistics with many equal values (a masked / saturated image): ranks are broken by index, as a sort does."""
    x = torch.ones(2, 3, 16, 24)
    x[1, :, :4] = 5.0
    x[1, 0, 8:, 3] = 0.25
    got = utils.sRGB(x.to(DEV)).cpu()
    np.testing.assert_allclose(got.numpy(), _srgb_torch(x).numpy(), rtol=0, atol=2e-6)


# ---------------------------------------------------------------------------------------------------------------------
# Edge cases of the epilogue against the reference's own chain (custom_transforms.py:4-21, utils.py:30-42) restated in torch
# and evaluated on the host in float64 from the same float32 values.  Where a quantile picks elements the chain starts from
# the DEVICE's linear image, as test_model_output_layout_full_size does.  NaN positions must be the reference's exactly.
# The linear image itself is held against the fp32 host expression (rtol 3e-6, the number of the tests above): the device
# rounds the exponent after every operation as the reference's fp32 tensor ops do, and a float64 exponent would measure
# that shared rounding (1 ulp of 18 is 1.9e-6, and it is exponentiated), not the kernel.
# ---------------------------------------------------------------------------------------------------------------------
from reni_amd._lib import RENILibraryError  # noqa: E402

MM = [-18.0536, 11.4633]
FLT_MAX = float(np.finfo(np.float32).max)
INF, NAN = float("inf"), float("nan")
PROBE = 2.0 ** -20   # a pixel this dark lies on the linear segment of the sRGB curve: out = 12.92 * PROBE / q


def _srgb_ref(lin, dtype=torch.float64):
    """utils.py:30-42 on the host in `dtype` -> (image [B,3,H,W], exposure q [B])."""
    x = lin.to(dtype)
    q = torch.quantile(torch.quantile(torch.quantile(x, 0.98, dim=1), 0.98, dim=1), 0.98, dim=1)
    y = torch.clamp(x / q.view(-1, 1, 1, 1), 0.0, 1.0)
    return torch.where(y <= 0.0031308, 12.92 * y, 1.055 * torch.pow(torch.abs(y), 1 / 2.4) - 0.055), q


def _norm_ref(img, mm, dtype=torch.float64):
    """custom_transforms.py:4-12 on the host in `dtype`, of ONE image."""
    img = img.to(dtype)
    img = torch.clip(img, img[img > 0.0].min(), img[img < torch.inf].max())
    return 2 * (torch.log(img) - mm[0]) / (mm[1] - mm[0]) - 1


def _norm_ref_batch(imgs, mm, dtype=torch.float64):
    """_norm_ref of every row of imgs [N, n] at once (a NaN fails both masks, as it does in the reference's indexing)."""
    x = imgs.to(dtype)
    lo = torch.where(x > 0.0, x, torch.full_like(x, INF)).amin(1, keepdim=True)
    hi = torch.where(x < INF, x, torch.full_like(x, -INF)).amax(1, keepdim=True)
    return 2 * (torch.log(torch.clip(x, lo, hi)) - mm[0]) / (mm[1] - mm[0]) - 1


def _ulp32(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _check(got, ref, rtol=0.0, atol=2e-6, what=""):
    """values within the tolerance AND NaNs exactly where the reference has them."""
    got = got.detach().cpu().double().numpy()
    ref = ref.detach().cpu().double().numpy()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN at {int(gn.sum())} places, the reference has {int(rn.sum())} (of {gn.size})"
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, equal_nan=True, err_msg=what)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _randexp(g, *shape, s=2.0):
    return torch.exp(s * torch.randn(*shape, generator=g))


# ------------------------------------------------------------------------------------------------ A. the quantile kernel

@pytest.mark.parametrize("axis", ["H", "W"])
@pytest.mark.parametrize("n", [1, 2, 3, 51, 101, 255, 256, 257, 511, 513, 4096])
def test_quantile_axis_sweep(n, axis):
    """The rank-by-counting quantile over an axis of n values (fp32 0.98f * 50 and 0.98f * 100 are exactly 49 and 98: floor ==
    ceil at n = 51 and 101; 4096 is the LDS limit), B = 1 and 3, the other axis 2 or 3 long, data exp(2 randn).

    Besides the image, the exposure q itself is read back through a probe pixel of value 2^-20 (it lies on the linear segment,
    so q = 12.92 * probe / out[probe]) and held against the float64 q.  Bound: twice the error of the torch fp32 chain on the
    host, read through the same probe, against the float64 chain, plus one fp32 ulp of q (a different but valid rounding
    order).  Measured on an MI355X over the 44 (n, axis, B) cases
    (profiles/r09_gpu_image_tests.log): the device's q read the same as the host fp32 chain's to every printed digit; its error
    against float64 ran from 8.4e-9 relative (n = 255) to 3.4e-6 (n = 256, B = 3: the fp32 rank 0.98f * 255 is 1.2e-5 from
    the float64 rank, and order statistics of exp(2 randn) that high lie far apart), under bounds of 1.2e-7 to 6.9e-6."""
    for B in (1, 3):
        other = 2 + (n + B) % 2
        H, W = (n, other) if axis == "H" else (other, n)
        x = _randexp(torch.Generator().manual_seed(100 * n + 10 * B + (axis == "W")), B, 3, H, W)
        x[:, :, 0, 0] = PROBE
        got = ops.unnormalise_srgb(x.to(DEV), None, srgb=True).cpu()
        ref, q64 = _srgb_ref(x)
        _check(got, ref, what=f"n={n} {axis} B={B}")
        ref32, _ = _srgb_ref(x, torch.float32)
        assert bool((ref[:, :, 0, 0] < 0.04).all()), "the probe left the linear segment"
        q_dev = 12.92 * PROBE / got[:, 0, 0, 0].double()
        q_f32 = 12.92 * PROBE / ref32[:, 0, 0, 0].double()
        bound = 2 * (q_f32 - q64).abs().numpy() + _ulp32(q64.numpy())
        err = (q_dev - q64).abs().numpy()
        worst = int(np.argmax(err / bound))
        print(f"q probe n={n} axis={axis} B={B}: device rel err {err[worst] / float(q64[worst]):.3e}  "
              f"bound rel {bound[worst] / float(q64[worst]):.3e}  host fp32 rel err {float((q_f32 - q64).abs()[worst] / q64[worst]):.3e}")
        assert (err <= bound).all(), (n, axis, B, q_dev.tolist(), q64.tolist(), bound.tolist())


def test_quantile_axis_limit():
    """4096 is the longest axis a quantile is taken over (the sweep above runs it); 4097 is refused, not truncated; without
    the sRGB view there is no limit: the [B,P,3] route of UnMinMaxNormlise is a [B,3,1,P] image."""
    for shape in ((1, 3, 1, 4097), (1, 3, 4097, 2)):
        x = torch.rand(*shape, generator=torch.Generator().manual_seed(1)).to(DEV)
        with pytest.raises(RENILibraryError, match="longer than 4096"):
            ops.unnormalise_srgb(x, None, srgb=True)
        with pytest.raises(RENILibraryError, match="longer than 4096"):
            utils.sRGB(x)
    t = torch.rand(2, 3, 1, 32768, generator=torch.Generator().manual_seed(2)) * 2 - 1
    lin = ops.unnormalise_srgb(t.to(DEV), MM, srgb=False)
    np.testing.assert_allclose(lin.cpu().numpy(), torch.exp(0.5 * (t + 1) * (MM[1] - MM[0]) + MM[0]).numpy(), rtol=3e-6, atol=0)
    assert _same_bits(ops.unnormalise_srgb(t.to(DEV), None, srgb=False).cpu(), t)
    model_out = t[:, :, 0].permute(0, 2, 1).contiguous()                 # [B, P, 3] with P = 32768
    assert _same_bits(UnMinMaxNormlise(MM)(model_out.to(DEV)).permute(0, 2, 1), lin[:, :, 0])


def _special_columns():
    g = torch.Generator().manual_seed(31)
    col = lambda: _randexp(g, 101)  # noqa: E731
    two, three, one = col(), col(), col()
    two[13] = two[77] = INF
    three[0] = three[50] = three[100] = INF   # the exact rank 98 of 101 values now picks an inf
    one[40] = INF
    return {
        "all equal": torch.full((101,), 1.7),
        "half +0 half -0": torch.cat([torch.zeros(50), -torch.zeros(51)]),
        "two +inf": two,
        "three +inf": three,
        "one +inf": one,
        "subnormal": torch.randint(1, 1 << 20, (101,), generator=g, dtype=torch.int32).view(torch.float32),
    }


@pytest.mark.parametrize("name", list(_special_columns()))
def test_quantile_ties_and_specials(name):
    """One 101-long column of ties, signed zeros, infinities or subnormals, alone (W = 1: its quantile IS the exposure) and
    beside two ordinary columns.  (An inf in a pixel's largest channel makes the channel quantile NaN already -- ATen's lerp
    forms inf - inf * 0.04 -- and a NaN column makes the exposure NaN: the kernel has to agree, NaN for NaN.)"""
    col = _special_columns()[name]
    assert name != "subnormal" or bool((col < 1.2e-38).all() and (col > 0).all())
    for W in (1, 3):
        x = _randexp(torch.Generator().manual_seed(W), 2, 3, 101, W)
        x[0, :, :, W // 2] = col
        x[1, 1, :, 0] = col     # in one channel only: the other two decide what the channel quantile is
        srgb, lin = ops.unnormalise_srgb(x.to(DEV), None, srgb=True, want_linear=True)
        assert _same_bits(lin.cpu(), x)
        _check(srgb, _srgb_ref(x)[0], what=f"{name} W={W}")


def test_quantile_of_an_overflowing_exponential():
    """A stored value of 20 un-normalises to exp(291) = inf: the infinity is made by the kernel's own exp."""
    g = torch.Generator().manual_seed(32)
    xn = torch.rand(2, 3, 101, 3, generator=g) * 2 - 1
    xn[0, :, 7, 1] = 20.0
    xn[0, 2, 60, 1] = 20.0
    srgb, lin = ops.unnormalise_srgb(xn.to(DEV), MM, srgb=True, want_linear=True)
    lin_ref = torch.exp(0.5 * (xn + 1) * (MM[1] - MM[0]) + MM[0])
    assert bool(torch.isinf(lin_ref[0, :, 7, 1]).all()) and int(torch.isinf(lin_ref).sum()) == 4
    np.testing.assert_allclose(lin.cpu().numpy(), lin_ref.numpy(), rtol=3e-6, atol=0)
    _check(srgb, _srgb_ref(lin.cpu())[0], what="exp overflow")


def test_strided_and_typed_inputs_sweep():
    """40 seeded small cases (H, W <= 40, B <= 4) over the layouts a caller can hand in, every one read in place: contiguous,
    channel-last, a batch expanded with stride 0, [:, :, ::2, 1:] slices, and float64 / half tensors through utils.sRGB, which
    returns the caller's dtype.  Every other round of the six layouts un-normalises first, so each of the four fp32 layouts
    runs both ways.  A half result is the fp32 result rounded to half, so it may
    sit half a half-ulp from the float64 reference on top of the 2e-6."""
    kinds = ["contiguous", "channel_last", "expand", "slices", "float64", "half"]
    rng = np.random.RandomState(5)
    for case in range(40):
        kind = kinds[case % len(kinds)]
        B, H, W = int(rng.randint(1, 5)), int(rng.randint(1, 41)), int(rng.randint(1, 41))
        g = torch.Generator().manual_seed(1000 + case)
        unnorm = (case // len(kinds)) % 2 == 1 and kind not in ("float64", "half")
        make = (lambda *s: torch.rand(*s, generator=g) * 2 - 1) if unnorm else (lambda *s: _randexp(g, *s))
        if kind == "channel_last":
            base = make(B, H, W, 3)
            view = lambda t: t.permute(0, 3, 1, 2)  # noqa: E731
        elif kind == "expand":
            base = make(1, 3, H, W)
            view = lambda t: t.expand(B, 3, H, W)  # noqa: E731
        elif kind == "slices":
            base = make(B, 3, 2 * H, W + 1)
            view = lambda t: t[:, :, ::2, 1:]  # noqa: E731
        else:
            base = make(B, 3, H, W)
            base = base.double() * (1 + 2.0 ** -30) if kind == "float64" else base.half() if kind == "half" else base
            view = lambda t: t  # noqa: E731
        host, dev = view(base), view(base.to(DEV))
        assert dev.stride() == host.stride()          # the device view keeps the layout: nothing was made contiguous
        what = f"case {case} {kind} B={B} H={H} W={W} unnorm={unnorm}"
        if kind in ("float64", "half"):
            got = utils.sRGB(dev)
            assert got.dtype == base.dtype and got.shape == (B, 3, H, W), what
            ref = _srgb_ref(host.float())[0]          # the fp32 values the device sees
            if kind == "half":
                atol = 2e-6 + 0.5 * np.spacing(ref.numpy().astype(np.float16)).astype(np.float64)
                d = np.abs(got.cpu().double().numpy() - ref.numpy())
                assert not np.isnan(d).any() and (d <= atol).all(), (what, float(d.max()))
            else:
                _check(got, ref, what=what)
        elif unnorm:
            srgb, lin = ops.unnormalise_srgb(dev, MM, srgb=True, want_linear=True)
            lin_ref = torch.exp(0.5 * (host + 1) * (MM[1] - MM[0]) + MM[0])
            np.testing.assert_allclose(lin.cpu().numpy(), lin_ref.numpy(), rtol=3e-6, atol=0, err_msg=what)
            _check(srgb, _srgb_ref(lin.cpu())[0], what=what)
        else:
            _check(ops.unnormalise_srgb(dev, None, srgb=True), _srgb_ref(host)[0], what=what)


# ------------------------------------------------------------------------ B. NaN and zero-exposure semantics of the sRGB view

@pytest.mark.parametrize("channel", [0, 1, 2])
def test_one_nan_pixel_makes_its_image_nan_and_no_other(channel):
    """torch.quantile propagates NaN, so the exposure of the image holding it is NaN and the whole picture with it -- it must
    not come out as a plausible picture whose quantile skipped the pixel.  The NaN as first, second and third channel covers
    the three positions of the sorting network: compare-exchanges alone leave a NaN in the first position where it is and the
    lerp then takes its two neighbours, and a clamp by fminf / fmaxf turns a NaN exposure into a black picture."""
    x = _randexp(torch.Generator().manual_seed(40 + channel), 2, 3, 9, 14)
    x[0, channel, 4, 6] = NAN
    srgb, lin = ops.unnormalise_srgb(x.to(DEV), None, srgb=True, want_linear=True)
    ref = _srgb_ref(x)[0]
    assert bool(torch.isnan(ref[0]).all()) and not bool(torch.isnan(ref[1]).any())
    _check(srgb, ref, what=f"NaN in channel {channel}")
    assert torch.equal(srgb[1], ops.unnormalise_srgb(x[1].to(DEV), None, srgb=True)[0])   # untouched by its neighbour
    assert _same_bits(lin.cpu(), x)
    # the same through the un-normalising call
    xn = torch.rand(2, 3, 9, 14, generator=torch.Generator().manual_seed(50 + channel)) * 2 - 1
    xn[1, channel, 0, 0] = NAN
    srgb, lin = ops.unnormalise_srgb(xn.to(DEV), MM, srgb=True, want_linear=True)
    assert int(torch.isnan(lin).sum()) == 1 and bool(torch.isnan(lin[1, channel, 0, 0]))
    _check(srgb, _srgb_ref(lin.cpu())[0], what=f"NaN in channel {channel}, un-normalised")


def test_zero_exposure_is_not_a_black_picture():
    """H = 101 with only the last two rows lit: every column's 0.98-quantile (rank exactly 98 of 99 zeros and 2 values) is 0,
    so q == 0.  The reference divides by it: lit pixels are inf -> clamp -> 1.0, zero pixels are 0 / 0 = NaN.  An all-zero
    image is NaN everywhere.  Neither may come out as 0.0, a valid black picture."""
    x = torch.zeros(3, 3, 101, 4)
    x[0, :, 99:, :] = _randexp(torch.Generator().manual_seed(60), 3, 2, 4)
    x[2] = _randexp(torch.Generator().manual_seed(61), 3, 101, 4)        # an ordinary image beside them
    srgb, lin = ops.unnormalise_srgb(x.to(DEV), None, srgb=True, want_linear=True)
    ref, q = _srgb_ref(x)
    assert q[0] == 0 and q[1] == 0 and q[2] > 0
    assert bool(((ref[0, :, 99:, :] - 1.0).abs() < 1e-15).all()) and bool(torch.isnan(ref[0, :, :99, :]).all()) and bool(torch.isnan(ref[1]).all())
    _check(srgb, ref, what="q == 0")
    assert _same_bits(lin.cpu(), x)
    _check(utils.sRGB(x[1].to(DEV)), ref[1:2], what="all-zero image")


# ------------------------------------------------------------------------------------ C. MinMaxNormalise, single and batched

def _single_and_batch(x2d, mm=MM, nan_to_num=False):
    """ops.minmax_normalise of every row and ops.minmax_normalise_batch of all rows (which must agree bit for bit)."""
    xd = x2d.to(DEV)
    batch = ops.minmax_normalise_batch(xd, mm, nan_to_num=nan_to_num)
    if not nan_to_num:
        for n in range(x2d.shape[0]):
            assert _same_bits(batch[n], ops.minmax_normalise(xd[n], mm)), f"image {n}: batch and single differ"
    return batch


def test_minmax_negative_zero_is_a_zero_not_a_bound():
    """-0.0 passes `x >= 0` and its bits, 0x80000000, are above those of every positive float: taken as the upper clip bound it
    would turn every pixel into log(-0.0) = -inf (-FLT_MAX after nan_to_num).  The reference's maximum over img < inf is the
    true maximum."""
    x = _randexp(torch.Generator().manual_seed(70), 3, 5, 7)
    xp, xn = x.clone(), x.clone()
    xp.view(-1)[17] = 0.0
    xn.view(-1)[17] = -0.0
    assert xn.view(-1)[17].view(torch.int32).item() == -(1 << 31)
    ref = _norm_ref(xp, MM)
    a, b = ops.minmax_normalise(xp.to(DEV), MM), ops.minmax_normalise(xn.to(DEV), MM)
    print("single: with -0.0 min/max", float(b.min()), float(b.max()), " with +0.0", float(a.min()), float(a.max()))
    _check(a, ref, atol=3e-7, what="+0.0")
    _check(b, ref, atol=3e-7, what="-0.0")
    assert _same_bits(a, b)
    for flag in (False, True):
        out = ops.minmax_normalise_batch(torch.stack([xn, xp, x]).to(DEV), MM, nan_to_num=flag)
        print("batch: with -0.0 min/max", float(out[0].min()), float(out[0].max()))
        _check(out[0], ref, atol=3e-7, what="batch -0.0")
        assert _same_bits(out[0], out[1]) and _same_bits(out[1], a)
        _check(out[2], _norm_ref(x, MM), atol=3e-7, what="batch, no zero")


@pytest.mark.parametrize("where", ["tail", "head"])
def test_minmax_grid_stride_tails(where):
    """k_img_minmax runs at most 2048 workgroups and k_img_minmax_batch 128 per image: beyond 2048 * 256 (128 * 256) elements
    the bounds come out of the stride loop.  The image's smallest positive and largest finite value sit in the last 200
    elements (then at elements 0 and 1), with a +inf, a negative value and a -inf as decoys earlier on."""
    def image(n, seed, scale):
        x = _randexp(torch.Generator().manual_seed(seed), n, s=1.0) * scale
        x[1000], x[2000], x[3000] = INF, -3.0, -INF
        imin, imax = (n - 150, n - 7) if where == "tail" else (0, 1)
        x[imin], x[imax] = float(x[x > 0].min()) * 1e-2, float(x[x < INF].max()) * 1e2
        return x
    n = 2048 * 256 + 257
    x = image(n, 80, 1.0)
    _check(ops.minmax_normalise(x.to(DEV), MM), _norm_ref(x, MM), atol=3e-7, what=f"single {where}")
    n = 128 * 256 + 257
    xb = torch.stack([image(n, 81, 1.0), image(n, 82, 10.0), image(n, 83, 0.1)])
    _check(_single_and_batch(xb), _norm_ref_batch(xb, MM), atol=3e-7, what=f"batch {where}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257])
def test_minmax_partial_waves_and_blocks(n):
    """Sizes that leave a wave or a workgroup partly empty; the bounds sit at both ends; a constant image has lo == hi."""
    x = _randexp(torch.Generator().manual_seed(90 + n), 3, n, s=1.0)
    x[0, 0], x[0, -1] = float(x[0].min()) * 0.1, float(x[0].max()) * 10.0
    x[1, -1], x[1, 0] = float(x[1].min()) * 0.1, float(x[1].max()) * 10.0
    x[2] = 0.37
    _check(_single_and_batch(x), _norm_ref_batch(x, MM), atol=3e-7, what=f"n={n}")
    for i in range(3):
        _check(MinMaxNormalise(MM)(x[i].to(DEV)), _norm_ref(x[i], MM), atol=3e-7, what=f"n={n} image {i}")


def test_minmax_value_range_extremes():
    """Smallest positive value a subnormal (1e-40), largest finite FLT_MAX beside a +inf, a zero clipped up to the subnormal.
    There |log x| reaches 92 and the output 6: one output ulp (4.8e-7) is above the 3e-7 of ordinary radiance, so those
    elements (|reference| > 1.5) are held to twice the error of the torch fp32 chain on the host against float64 plus one
    fp32 ulp of the output; ordinary elements keep 3e-7.  Measured on an MI355X
    (profiles/r09_gpu_image_tests.log): host fp32 3.8e-7, device 3.8e-7, bound 1.24e-6; ordinary elements 1.8e-7."""
    x = _randexp(torch.Generator().manual_seed(95), 2, 1000, s=1.0)
    x[0, 3], x[0, 500], x[0, 700], x[0, 20] = 1e-40, FLT_MAX, INF, 0.0
    x[1, 999], x[1, 0], x[1, 1], x[1, 2] = 1e-40, FLT_MAX, INF, -INF
    assert 0 < float(x[0, 3]) < 1.2e-38
    ref, ref32 = _norm_ref_batch(x, MM), _norm_ref_batch(x, MM, torch.float32).double()
    extreme = ref.abs() > 1.5
    assert int(extreme.sum()) == 8
    e32 = float((ref32 - ref).abs()[extreme].max())
    atol = torch.where(extreme, 2 * e32 + torch.from_numpy(_ulp32(ref.numpy())), torch.full_like(ref, 3e-7))
    got = _single_and_batch(x).cpu().double()
    err = (got - ref).abs()
    print(f"extremes: host fp32 err {e32:.3e}, device err {float(err[extreme].max()):.3e}, bound {float(atol[extreme].min()):.3e}; "
          f"ordinary: device err {float(err[~extreme].max()):.3e}")
    assert not bool(torch.isnan(got).any())
    assert bool((err <= atol).all()), (float(err[extreme].max()), float(err[~extreme].max()))


def test_minmax_batch_bookkeeping():
    """N = 257 needs a second workgroup of k_img_minmax_init_batch; every image has its own bounds; image n of the batch is
    bit-equal to the single-image call and a second call to the first.  65535 images is the grid's limit, 65536 is refused."""
    g = torch.Generator().manual_seed(96)
    x = _randexp(g, 257, 6, s=1.0) * (2.0 ** (torch.arange(257) % 21 - 10)).view(-1, 1)
    out = _single_and_batch(x)
    _check(out, _norm_ref_batch(x, MM), atol=3e-7, what="N=257")
    for flag in (False, True):
        a = ops.minmax_normalise_batch(x.to(DEV), MM, nan_to_num=flag)
        assert _same_bits(a, ops.minmax_normalise_batch(x.to(DEV), MM, nan_to_num=flag)) and _same_bits(a, out)
    x = _randexp(g, 65535, 4, s=1.0) * (2.0 ** (torch.arange(65535) % 21 - 10)).view(-1, 1)
    _check(ops.minmax_normalise_batch(x.to(DEV), MM), _norm_ref_batch(x, MM), atol=3e-7, what="N=65535")
    with pytest.raises(RENILibraryError, match="65535"):
        ops.minmax_normalise_batch(torch.ones(65536, 4, device=DEV), MM)


def test_minmax_nan_and_nan_to_num():
    """The bounds ignore a NaN (it fails both of the reference's masks); the pixel itself stays NaN, or becomes 0 under
    nan_to_num, which also turns +-inf outputs into +-FLT_MAX (datasets.py:72)."""
    x = _randexp(torch.Generator().manual_seed(97), 2, 40, s=1.0)
    x[0, 5], x[0, 6], x[0, 7], x[0, 8] = NAN, INF, -INF, 0.0
    ref = _norm_ref_batch(x, MM)
    assert int(torch.isnan(ref).sum()) == 1
    np.testing.assert_array_equal(ref[0].numpy(), _norm_ref(x[0], MM).numpy())
    raw = _single_and_batch(x)
    _check(raw, ref, atol=3e-7, what="NaN kept")
    _check(MinMaxNormalise(MM)(x[0].to(DEV)), ref[0], atol=3e-7, what="NaN kept, transform class")
    out = ops.minmax_normalise_batch(x.to(DEV), MM, nan_to_num=True)
    _check(out, torch.nan_to_num(ref), atol=3e-7, what="NaN -> 0")
    assert float(out[0, 5]) == 0.0
    # infinite outputs: a range so small that the affine map overflows fp32 on either side of log x = 0 ...
    tiny = [0.0, 2e-38]
    y = torch.tensor([[1e-30, 1.0, 1e30, 1e35]])
    want = _norm_ref_batch(y, tiny).float()       # float64 holds 7e39; rounding it to fp32 gives the infinities
    assert want.tolist() == [[-INF, -1.0, INF, INF]]
    assert _single_and_batch(y, tiny).cpu().tolist() == want.tolist()
    assert ops.minmax_normalise_batch(y.to(DEV), tiny, nan_to_num=True).cpu().tolist() == [[-FLT_MAX, -1.0, FLT_MAX, FLT_MAX]]
    # ... and an image whose only positive value is +inf: the reference clips to [inf, 0], which is 0, and log 0 = -inf
    z = torch.zeros(1, 8)
    z[0, 3] = INF
    want = _norm_ref(z[0], MM).float()
    assert bool((want == -INF).all())
    assert torch.equal(_single_and_batch(z).cpu()[0], want)
    assert bool((ops.minmax_normalise_batch(z.to(DEV), MM, nan_to_num=True) == -FLT_MAX).all())


# ---------------------------------------------------------------------------------------------------------- D. the wrappers

def test_unminmaxnormlise_shapes_and_views():
    """UnMinMaxNormlise of a 1-D, a 2-D and a [B,P,3] tensor and of non-contiguous [B,P,3] slices, against the reference's
    expression in fp32 on the host.  _unnormalise_device tells a model output [B,P,3] from an image [3,H,W] by shape[-3] != 3,
    so the model-output cases use B = 2 and 4: they go through its `.view(B, 1, P, 3)`, which has to read the slices in place.
    A [3,P,3] tensor goes the image way and has to give the same numbers."""
    g = torch.Generator().manual_seed(98)
    f = UnMinMaxNormlise(MM)
    cases = {
        "1-D": (torch.rand(301, generator=g) * 2 - 1, lambda t: t),
        "2-D": (torch.rand(37, 5, generator=g) * 2 - 1, lambda t: t),
        "2-D [P,3]": (torch.rand(37, 3, generator=g) * 2 - 1, lambda t: t),
        "[B,P,3]": (torch.rand(2, 257, 3, generator=g) * 2 - 1, lambda t: t),
        "[B,P,3] every other pixel, inner channels": (torch.rand(4, 2 * 257, 5, generator=g) * 2 - 1, lambda t: t[:, ::2, 1:4]),
        "[B,P,3] of a transpose": (torch.rand(2, 3, 257, generator=g) * 2 - 1, lambda t: t.transpose(1, 2)),
        "[B,P,3] every other image": (torch.rand(4, 257, 3, generator=g) * 2 - 1, lambda t: t[::2]),
        "[3,P,3] (an image [3,H,W])": (torch.rand(3, 2 * 257, 5, generator=g) * 2 - 1, lambda t: t[:, ::2, 1:4]),
    }
    for what, (base, view) in cases.items():
        host, dev = view(base), view(base.to(DEV))
        if what.startswith("[B,P,3]"):   # the model-output branch, not the image one
            assert dev.dim() == 3 and dev.shape[-1] == 3 and dev.shape[-3] != 3, what
            assert what == "[B,P,3]" or not dev.is_contiguous(), what
        y = f(dev)
        assert y.shape == host.shape and y.dtype == torch.float32 and y.is_cuda, what
        np.testing.assert_allclose(y.cpu().numpy(), torch.exp(0.5 * (host + 1) * (MM[1] - MM[0]) + MM[0]).numpy(), rtol=3e-6,
                                   atol=0, err_msg=what)


def test_unminmaxnormlise_gradient_of_a_model_output():
    """FIT_INVERSE's gradient through the [B,P,3] form, P = 257 (a second workgroup with one pixel in it)."""
    x = torch.rand(2, 257, 3, generator=torch.Generator().manual_seed(99)) * 2 - 1
    w = torch.rand(2, 257, 3, generator=torch.Generator().manual_seed(100))
    xd = x.to(DEV).requires_grad_(True)
    (UnMinMaxNormlise(MM)(xd) * w.to(DEV)).sum().backward()
    xc = x.clone().requires_grad_(True)
    (torch.exp(0.5 * (xc + 1) * (MM[1] - MM[0]) + MM[0]) * w).sum().backward()
    assert xd.grad.shape == x.shape
    np.testing.assert_allclose(xd.grad.cpu().numpy(), xc.grad.numpy(), rtol=5e-6)


def test_image_calls_launch_what_the_design_says():
    """four launches for the sRGB view, one for the linear image alone, three for either normaliser.  The library
    counts at every launch site of reni_tu_image.hip (reni_launch_count), so a launch added to one of these calls shows here."""
    x = torch.rand(2, 3, 8, 16, generator=torch.Generator().manual_seed(101)).to(DEV) + 0.1
    ops.launch_count(reset=True)
    ops.unnormalise_srgb(x, MM, srgb=True, want_linear=True)
    assert ops.launch_count(reset=True) == 4
    ops.unnormalise_srgb(x, MM, srgb=False)
    assert ops.launch_count(reset=True) == 1
    ops.minmax_normalise(x, MM)
    assert ops.launch_count(reset=True) == 3
    ops.minmax_normalise_batch(x, MM)
    assert ops.launch_count(reset=True) == 3
