"""GPU tests of diffuse irradiance (reni_tu_diffuse.hip through reni_amd.baselines / reni_amd.ops) against the golden made
from the reference (tests/golden/make_g24_diffuse.py) and float64 restatements."""
import numpy as np
import pytest
import torch

from tests.test_baselines_cpu import rel
from tests.test_diffuse_cpu import DM_SHAPES, G24, SR_LMAX, SR_WIDTHS, np_sh_render_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5  # fp32 against float64, relative to the map's maximum


def _dev():
    return torch.device("cuda")


def _unit(g, n):
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return (d / d.norm(dim=1, keepdim=True)).float()


def _ref64(src, in_dirs, w, out_dirs, scale=1 / np.pi):
    """float64 E [N, P, 3] on the device, 256 output rows at a time"""
    d, w64, s = in_dirs.double(), w.double(), src.double()
    out = []
    for o0 in range(0, out_dirs.shape[0], 256):
        A = torch.clamp(out_dirs[o0:o0 + 256].double() @ d.T, min=0) * w64
        out.append(torch.einsum("pq,nqc->npc", A, s))
    return torch.cat(out, 1) * scale


@pytest.mark.parametrize("W,wl", DM_SHAPES)
def test_diffuse_map_matches_the_reference(W, wl):
    from reni_amd import baselines
    g = np.load(G24)
    for i, img in enumerate(g[f"dm_w{W}_imgs"]):
        ref = g[f"dm_w{W}_l{wl}"][i]
        out = baselines.getDiffuseMap(img, width=W, widthLowRes=wl, outputWidth=wl)
        assert out.dtype == np.float32 and out.shape == ref.shape
        assert rel(out, ref) <= TOL, (W, wl, i, rel(out, ref))
        out_t = baselines.getDiffuseMap(torch.from_numpy(img).to(_dev()), width=W, widthLowRes=wl, outputWidth=wl)
        assert np.array_equal(out_t, out)


def test_sh_renders_match_the_reference():
    from reni_amd import baselines
    g = np.load(G24)
    for lmax in SR_LMAX:
        for W in SR_WIDTHS:
            ref = g[f"sr_l{lmax}_w{W}"]
            out = baselines.shRender(g[f"sr_l{lmax}_coeffs"], W)
            assert out.shape == ref.shape and rel(out, ref) <= TOL, (lmax, W)
            if lmax != 2:  # shReconstructDiffuseMap takes shRender for every count but 9
                assert rel(baselines.shReconstructDiffuseMap(g[f"sr_l{lmax}_coeffs"], W), ref) <= TOL
    c9 = g["sr_l2_coeffs"]
    for W in SR_WIDTHS:
        out = baselines.shReconstructDiffuseMap(c9, W)
        assert out.dtype == np.float32 and rel(out, g[f"srd_w{W}"]) <= TOL, W
    out = baselines.shReconstructDiffuseNormalMap(c9, g["srn_normals"])
    assert out.shape == (8, 12, 3) and rel(out, g["srn_out"]) <= TOL
    # the batched form: map n of sh_irradiance is the single-map result
    for lmax in (2, 5):
        cs = torch.from_numpy(np.stack([g[f"sr_l{lmax}_coeffs"], -g[f"sr_l{lmax}_coeffs"]])).float().to(_dev())
        maps = baselines.sh_irradiance(cs, 32)
        ref = g[f"srd_w32"] if lmax == 2 else g["sr_l5_w32"]
        assert rel(maps[0].cpu().numpy(), ref) <= TOL and rel(maps[1].cpu().numpy(), -ref) <= TOL


@pytest.mark.parametrize("P,Q", [(777, 5003), (2000, 1001)])
def test_diffuse_convolve_matches_float64(P, Q):
    """P, Q not multiples of any tile; (777, 5003) splits the i range, (2000, 1001) does not"""
    from reni_amd import baselines
    dev = _dev()
    gen = torch.Generator().manual_seed(P + Q)
    in_dirs, out_dirs = _unit(gen, Q).to(dev), _unit(gen, P).to(dev)
    w = (torch.rand(Q, generator=gen) * 4 * np.pi / Q).to(dev)
    for N in (1, 2, 5, 64):
        src = (torch.rand(N, Q, 3, generator=gen) * 3).to(dev)
        ref = _ref64(src, in_dirs, w, out_dirs)
        out = baselines.diffuse_convolve(src, in_dirs, w, out_dirs)
        assert out.shape == (N, P, 3)
        assert rel(out.cpu().numpy(), ref.cpu().numpy()) <= TOL, (N, P, Q)
        planar = src.permute(0, 2, 1).contiguous()  # [N, 3, Q]
        assert torch.equal(baselines.diffuse_convolve(planar, in_dirs, w, out_dirs), out)
        assert torch.equal(baselines.diffuse_convolve(planar.permute(0, 2, 1), in_dirs, w, out_dirs), out)
    out2 = baselines.diffuse_convolve(src, in_dirs, w, out_dirs, scale=2.0)
    assert rel(out2.cpu().numpy(), (ref * 2 * np.pi).cpu().numpy()) <= TOL


def test_sh_irradiance_l2_matches_float64():
    from reni_amd import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(3)
    N, P = 5, 1234
    coeffs = torch.randn(N, 9, 3, generator=gen, dtype=torch.float64)
    shared = _unit(gen, P).double()
    per_map = torch.stack([_unit(gen, P) for _ in range(N)]).double()
    for nrm in (shared, per_map):
        out = ops.sh_irradiance_l2(coeffs.float().to(dev), nrm.float().to(dev)).cpu().numpy()
        c32, n32 = coeffs.float().double().numpy(), nrm.float().double().numpy()
        for n in range(N):
            ref = np_sh_render_l2(c32[n], n32 if nrm.dim() == 2 else n32[n])
            assert rel(out[n], ref) <= TOL, n


@pytest.mark.parametrize("P,Q", [(777, 5003), (300, 2 * 2048 + 3)])
def test_diffuse_convolve_is_deterministic_and_batch_independent(P, Q):
    from reni_amd import _lib, ops
    dev = _dev()
    lib = _lib.load()
    assert lib.reni_diffuse_workspace_bytes(1, P, Q) > 0  # the i split is active at these shapes
    gen = torch.Generator().manual_seed(11)
    in_dirs, out_dirs = _unit(gen, Q).to(dev), _unit(gen, P).to(dev)
    w = torch.rand(Q, generator=gen).to(dev)
    big = (torch.rand(64, Q, 3, generator=gen) * 2 - 0.5).to(dev)
    full = ops.diffuse_convolve(big, in_dirs, w, out_dirs, 1 / np.pi)
    assert torch.equal(ops.diffuse_convolve(big, in_dirs, w, out_dirs, 1 / np.pi), full)
    for n in (0, 1, 4, 33, 63):
        alone = ops.diffuse_convolve(big[n:n + 1], in_dirs, w, out_dirs, 1 / np.pi)
        assert torch.equal(alone[0], full[n]), n
    for B in (2, 5):
        for s in (0, 64 - B):
            part = ops.diffuse_convolve(big[s:s + B], in_dirs, w, out_dirs, 1 / np.pi)
            assert torch.equal(part, full[s:s + B]), (B, s)


def test_irradiance_map_constant_map_convention():
    """A constant map of 1 on RENI's grid: float64 deviation from 1 is 1.78e-3 / 4.7e-4 / 1.20e-4 at W = 32 / 64 / 128."""
    from reni_amd import baselines
    for W, bound in ((32, 2e-3), (64, 6e-4), (128, 2e-4)):
        ones = torch.ones(2, W // 2, W, 3, device=_dev())
        E = baselines.irradiance_map(ones)
        assert E.shape == ones.shape
        assert float((E - 1).abs().max()) <= bound, (W, float((E - 1).abs().max()))
        E2 = baselines.irradiance_map(ones.reshape(2, -1, 3), out_width=W // 2)
        assert E2.shape == (2, W * W // 8, 3) and float((E2 - 1).abs().max()) <= 2 * bound


def test_reference_shape_and_batch_without_a_pq_tensor():
    """One 600-wide map to 32 x 16 (the reference's default grid) and 64 maps of 64 x 128 at full resolution, with the
    peak memory beyond inputs and outputs under 64 MB."""
    from reni_amd import baselines
    from reni_amd.utils import get_directions
    dev = _dev()
    gen = torch.Generator().manual_seed(5)
    img = (torch.rand(300, 600, 3, generator=gen) + 0.1).to(dev)
    baselines.getDiffuseMap(img[:2, :4], width=4, widthLowRes=4)  # warm the library up outside the measurement
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = baselines.getDiffuseMap(img, width=600, widthLowRes=32, outputWidth=32)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < (64 << 20)
    d, sa, od = baselines.diffuse_map_tables(600, 32)
    t = lambda x: torch.from_numpy(x).float().to(dev)  # noqa: E731
    ref = _ref64(img.reshape(1, -1, 3), t(d), t(sa), t(od))[0].view(16, 32, 3)
    assert rel(out, ref.cpu().numpy()) <= TOL
    envs = (torch.rand(64, 64 * 128, 3, generator=gen) * 2).to(dev)
    baselines.irradiance_map(envs[:1, :128].reshape(1, 8, 16, 3))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    E = baselines.irradiance_map(envs)
    torch.cuda.synchronize()
    out_bytes = E.numel() * 4
    assert torch.cuda.max_memory_allocated() - before - out_bytes < (64 << 20)
    dirs = get_directions(128)[0].to(dev)
    w = torch.from_numpy(baselines.reni_grid_weights(128)).float().to(dev)
    ref = _ref64(envs[[0, 63]], dirs, w, dirs)
    assert rel(E[[0, 63]].cpu().numpy(), ref.cpu().numpy()) <= TOL
