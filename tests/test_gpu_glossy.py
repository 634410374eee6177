"""GPU tests of glossy lighting (reni_tu_glossy.hip through reni_amd.glossy / reni_amd.ops) against the float64 restatements
of tests/test_glossy_cpu.py and against the project's own diffuse convolution and Blinn-Phong shader.

The tolerance of the convolution is derived, not measured (tests/test_glossy_cpu.py::lobe_tol): per lobe
1e-5 + S 2^-22 relative to max |reference| of that lobe's output."""
import os

import numpy as np
import pytest
import torch

from reni_amd import glossy
from tests.test_glossy_cpu import (FH_LOBES, fh_case, fh_field, lobe_tol, np_lobe_convolve, np_lookup_chain, random_dirs)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")
# phong 1, 8, 64, 500; blinn 20, 500; ggx alpha 1, 0.25, 0.0625 (ggx() takes the roughness, alpha = roughness^2)
LOBES = [glossy.phong(1), glossy.phong(8), glossy.phong(64), glossy.phong(500), glossy.blinn(20), glossy.blinn(500),
         glossy.ggx(1.0), glossy.ggx(0.5), glossy.ggx(0.25)]
SHAPES = [(777, 5003), (2000, 1001)]  # (P, Q): the first splits the i range and has an odd Q
NMAX = 22


def _dev():
    return torch.device("cuda")


def _unit(g, n):
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return (d / d.norm(dim=1, keepdim=True)).float()


def _lobe64(lobe, t):
    """f(t) in float64 on the device, from the header's definitions"""
    tc, m = t.clamp(0, 1), ((1 + t) / 2).clamp(0, 1)
    if lobe.kind == "phong":
        return tc ** lobe.param
    if lobe.kind == "blinn":
        return m ** (lobe.param / 2)
    a2 = lobe.param * lobe.param
    return tc * a2 / (m * (a2 - 1) + 1) ** 2


def _ref64(src, in_dirs, w, out_dirs, lobes):
    """(num [N, Lv, P, 3], den [Lv, P]) float64 on the device, 256 output rows at a time"""
    d, w64, s = in_dirs.double(), w.double(), src.double()
    num, den = [], []
    for o0 in range(0, out_dirs.shape[0], 256):
        t = out_dirs[o0:o0 + 256].double() @ d.T
        A = torch.stack([_lobe64(l, t) for l in lobes]) * w64  # [Lv, p, Q]
        num.append(torch.einsum("lpq,nqc->nlpc", A, s))
        den.append(A.sum(2))
    return torch.cat(num, 2), torch.cat(den, 1)


_CASES = {}


def _case(P, Q):
    """inputs and the float64 reference of a shape, computed once and shared"""
    if (P, Q) not in _CASES:
        dev = _dev()
        gen = torch.Generator().manual_seed(P + Q)
        in_dirs, out_dirs = _unit(gen, Q).to(dev), _unit(gen, P).to(dev)
        w = (torch.rand(Q, generator=gen) * 4 * np.pi / Q).to(dev)
        src = (torch.rand(NMAX, Q, 3, generator=gen) * 3).to(dev)
        num, den = _ref64(src, in_dirs, w, out_dirs, LOBES)
        _CASES[(P, Q)] = (in_dirs, out_dirs, w, src, num.cpu().numpy(), den.cpu().numpy())
    return _CASES[(P, Q)]


def _check_lobes(out, ref, lobes, what):
    """out, ref [N, Lv, P, 3]: every lobe within its tolerance, relative to max |reference| of that lobe's output"""
    out = out.double().cpu().numpy() if isinstance(out, torch.Tensor) else np.asarray(out, np.float64)
    assert out.shape == ref.shape and np.isfinite(out).all(), what
    for k, lobe in enumerate(lobes):
        err = np.abs(out[:, k] - ref[:, k]).max() / np.abs(ref[:, k]).max()
        print(f"{what} {lobe.kind}({lobe.param:g}): error / tolerance {err / lobe_tol(tuple(lobe)):.3f}")
        assert err <= lobe_tol(tuple(lobe)), (what, lobe, err, lobe_tol(tuple(lobe)))


# ------------------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("P,Q", SHAPES)
def test_lobe_convolve_matches_float64(P, Q):
    in_dirs, out_dirs, w, src, num, den = _case(P, Q)
    for N in (1, 11, NMAX):  # 3, 33, 66 colour columns (plus the column of ones): across the 32- and 64-column group edges
        s = src[:N]
        out = glossy.lobe_convolve(s, in_dirs, w, out_dirs, LOBES)
        assert out.shape == (N, len(LOBES), P, 3)
        _check_lobes(out, num[:N] / den[None, :, :, None], LOBES, f"normalised N={N} P={P} Q={Q}")
        raw = glossy.lobe_convolve(s, in_dirs, w, out_dirs, LOBES, normalise=False, scale=0.75)
        _check_lobes(raw, 0.75 * num[:N], LOBES, f"unnormalised N={N} P={P} Q={Q}")
        planar = s.permute(0, 2, 1).contiguous()  # [N, 3, Q]
        assert torch.equal(glossy.lobe_convolve(planar, in_dirs, w, out_dirs, LOBES), out)
        assert torch.equal(glossy.lobe_convolve(planar.permute(0, 2, 1), in_dirs, w, out_dirs, LOBES), out)
        assert torch.equal(glossy.lobe_convolve(planar, in_dirs, w, out_dirs, LOBES, normalise=False, scale=0.75), raw)


@pytest.mark.parametrize("normalise", [True, False])
def test_lobe_convolve_is_deterministic_lobe_and_batch_independent(normalise):
    from reni_amd import _lib
    P, Q = SHAPES[0]
    lib = _lib.load()
    one, two = lib.reni_lobe_workspace_bytes(1, P, 2048, 1), lib.reni_lobe_workspace_bytes(1, P, Q, 1)
    assert two - 256 >= 2 * (one - 256)  # the i split is active at this shape
    in_dirs, out_dirs, w, src, _, _ = _case(P, Q)
    kw = dict(normalise=normalise, scale=1.0 / np.pi)
    full = glossy.lobe_convolve(src, in_dirs, w, out_dirs, LOBES, **kw)
    assert torch.equal(glossy.lobe_convolve(src, in_dirs, w, out_dirs, LOBES, **kw), full)
    for k, lobe in enumerate(LOBES):  # a lobe alone
        assert torch.equal(glossy.lobe_convolve(src, in_dirs, w, out_dirs, [lobe], **kw)[:, 0], full[:, k]), lobe
    assert torch.equal(glossy.lobe_convolve(src, in_dirs, w, out_dirs, LOBES[::-1], **kw), full.flip(1))
    for n in (0, 10, 11, 21):  # a map alone, and inside a smaller batch
        assert torch.equal(glossy.lobe_convolve(src[n:n + 1], in_dirs, w, out_dirs, LOBES, **kw)[0], full[n]), n
    assert torch.equal(glossy.lobe_convolve(src[5:16], in_dirs, w, out_dirs, LOBES, **kw), full[5:16])


def test_empty_lobe_gives_zero():
    """phong(1e6) sees no texel among 64 random directions: numerator and denominator are 0, the result is 0, not NaN"""
    dev = _dev()
    gen = torch.Generator().manual_seed(29)
    in_dirs, out_dirs = _unit(gen, 64), _unit(gen, 300)
    assert float((out_dirs.double() @ in_dirs.double().T).max()) < 1 - 2e-4  # 1e6 log2(t) < -288: below fp32's range
    w = torch.rand(64, generator=gen) + 0.5
    src = torch.rand(3, 64, 3, generator=gen) + 1
    for normalise in (True, False):
        out = glossy.lobe_convolve(src.to(dev), in_dirs.to(dev), w.to(dev), out_dirs.to(dev), [glossy.phong(1e6)],
                                   normalise=normalise)
        assert out.shape == (3, 1, 300, 3) and torch.equal(out, torch.zeros_like(out))
    # next to a lobe that is not empty, which stays what it is alone
    both = glossy.lobe_convolve(src.to(dev), in_dirs.to(dev), w.to(dev), out_dirs.to(dev), [glossy.phong(1e6), glossy.phong(2)])
    alone = glossy.lobe_convolve(src.to(dev), in_dirs.to(dev), w.to(dev), out_dirs.to(dev), [glossy.phong(2)])
    assert torch.equal(both[:, 0], torch.zeros_like(both[:, 0])) and torch.equal(both[:, 1], alone[:, 0])
    assert float(alone.min()) >= 1 and float(alone.max()) <= 2  # a normalised lobe averages: the maps lie in [1, 2]


def test_phong_one_is_the_diffuse_convolution():
    from reni_amd import baselines
    P, Q = SHAPES[0]
    in_dirs, out_dirs, w, src, _, _ = _case(P, Q)
    ref = baselines.diffuse_convolve(src[:5], in_dirs, w, out_dirs)
    out = glossy.lobe_convolve(src[:5], in_dirs, w, out_dirs, [glossy.phong(1)], normalise=False, scale=1 / np.pi)[:, 0]
    err = float((out - ref).abs().max() / ref.abs().max())
    print(f"phong(1) against diffuse_convolve: {err:.3g}")
    assert err <= 2 * 1e-5


@pytest.mark.parametrize("s,shader_tol", [(20.0, 2e-5), (500.0, 2e-4)])
def test_blinn_is_the_shader_seen_along_the_normal(s, shader_tol):
    """positions = camera - k normals: the view direction is the normal, and the shader's specular term is norm(s) times the
    BLINN(s) convolution at the normals (weight 1: the shader sums the colours as they are)"""
    from reni_amd import ops
    from reni_amd.utils import get_directions
    dev = _dev()
    gen = torch.Generator().manual_seed(int(s))
    nrm = _unit(gen, 200)
    cam = torch.tensor([0.3, -0.2, 2.0])
    pos = cam[None] - nrm * (0.5 + torch.rand(200, 1, generator=gen))
    dirs = get_directions(32)[0]  # J = 16 x 32 texels
    colors = torch.rand(2, dirs.shape[0], 3, generator=gen) * 2
    shaded = ops.envmap_shade(nrm.to(dev), pos.to(dev), cam, dirs.to(dev), colors.to(dev), s, 0.0, 1.0)
    conv = glossy.lobe_convolve(colors.to(dev), dirs.to(dev), torch.ones(dirs.shape[0], device=dev), nrm.to(dev),
                                [glossy.blinn(s)], normalise=False)[:, 0]
    want = glossy.blinn_phong_norm(s) * conv
    err = float((shaded - want).abs().max() / want.abs().max())
    tol = shader_tol + lobe_tol(("blinn", s))
    print(f"blinn({s:g}) against the shader: {err:.3g} of {tol:.3g}")
    assert err <= tol


def test_prefilter_funk_hecke_on_the_device():
    """prefilter at W = 64 -> 16 x 8 deviates from the analytic field by at most the float64 restatement's deviation at that
    shape plus the kernel's tolerance"""
    from reni_amd.utils import get_directions
    ref, ana = fh_case(64)
    src = torch.from_numpy(fh_field(get_directions(64)[0].numpy()).astype(np.float32))[None].to(_dev())
    out = glossy.prefilter(src, FH_LOBES, out_width=16)
    assert out.shape == (1, len(FH_LOBES), 128, 3)
    out4 = glossy.prefilter(src.view(1, 32, 64, 3), FH_LOBES, out_width=16)
    assert out4.shape == (1, len(FH_LOBES), 8, 16, 3) and torch.equal(out4.view_as(out), out)
    assert glossy.prefilter(src, FH_LOBES).shape == (1, len(FH_LOBES), 32 * 64, 3)
    got = out[0].double().cpu().numpy()
    for k, lobe in enumerate(FH_LOBES):
        dev64 = np.abs(ref[k] - ana[k]).max()
        d = np.abs(got[k] - ana[k]).max()
        print(f"Funk-Hecke {lobe.kind}({lobe.param:g}): device {d:.3g}, float64 {dev64:.3g}")
        assert d <= dev64 + lobe_tol(tuple(lobe)) * np.abs(ref[k]).max(), lobe
    _check_lobes(out, ref[None], FH_LOBES, "prefilter W=64")
    # a constant map stays that constant under every lobe: numerator and denominator are the same sum up to its fp32 rounding
    c = glossy.prefilter(torch.full((1, 32 * 64, 3), 0.37, device=_dev()), LOBES, out_width=16)
    assert float((c - 0.37).abs().max()) <= 0.37 * 1e-5


# ------------------------------------------------------------------------------------------ lookup
def _check_lookup(out, chain, dirs, level, what):
    """out [N, P, 3] against the oracle, per map; dirs [P, 3] or [N, P, 3], level None, a number, [P] or [N, P] (numpy)"""
    out = out.double().cpu().numpy()
    N, Lv = chain.shape[:2]
    worst = 0.0
    for n in range(N):
        d = dirs if dirs.ndim == 2 else dirs[n]
        lv = np.zeros(len(d), np.float32) if level is None else np.broadcast_to(
            np.asarray(level, np.float32) if np.ndim(level) < 2 else np.asarray(level[n], np.float32), (len(d),))
        val, bound, keep = np_lookup_chain(chain[n], d, lv)
        assert (~keep).mean() <= 0.03, what
        assert np.isfinite(out[n]).all(), what
        worst = max(worst, float((np.abs(out[n] - val) / bound)[keep].max()))
        assert (np.abs(out[n] - val)[keep] <= bound[keep]).all(), (what, n)
        # inside the caps too the value is a mix of the levels' texels (up to the three lerps' rounding)
        l0 = np.floor(np.clip(lv, 0, Lv - 1)).astype(int)
        lo = np.minimum(chain[n].reshape(Lv, -1).min(1)[l0], chain[n].reshape(Lv, -1).min(1)[np.minimum(l0 + 1, Lv - 1)])
        hi = np.maximum(chain[n].reshape(Lv, -1).max(1)[l0], chain[n].reshape(Lv, -1).max(1)[np.minimum(l0 + 1, Lv - 1)])
        slack = 8 * 2.0 ** -24 * np.abs(chain[n]).max()
        assert (out[n] >= lo[:, None] - slack).all() and (out[n] <= hi[:, None] + slack).all(), (what, n)
    print(f"lookup {what}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("H,W", [(8, 16), (16, 32)])
def test_lookup_matches_the_oracle(H, W):
    dev = _dev()
    g = np.random.default_rng(H)
    chain = g.random((3, 3, H, W, 3)).astype(np.float32)
    ct = torch.from_numpy(chain).to(dev)
    shared = random_dirs(4096, 7 + H)
    per_map = np.stack([random_dirs(4096, 100 + n + H) for n in range(3)])
    lv_p = g.uniform(-0.5, 2.5, 4096).astype(np.float32)
    lv_np = g.uniform(-0.5, 2.5, (3, 4096)).astype(np.float32)
    for dirs, dname in ((shared, "shared"), (per_map, "per map")):
        dt = torch.from_numpy(dirs).to(dev)
        for level, lname in ((None, "no level"), (1.3, "level 1.3"), (lv_p, "level [P]"), (lv_np, "level [N, P]")):
            lt = torch.from_numpy(level).to(dev) if isinstance(level, np.ndarray) else level
            out = glossy.lookup(ct, dt, lt)
            assert out.shape == (3, 4096, 3)
            _check_lookup(out, chain, dirs, level, f"{H} x {W} {dname}, {lname}")
            assert torch.equal(glossy.lookup(ct, dt, lt), out)
    # plain maps are a chain of one level; a strided view is read in place
    maps = ct[:, 1]
    assert torch.equal(glossy.lookup(maps, torch.from_numpy(shared).to(dev)), glossy.lookup(ct, torch.from_numpy(shared).to(dev), 1.0))
    planar = ct.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)  # [N, Lv, H, W, 3] over planar memory
    assert not planar.is_contiguous()
    assert torch.equal(glossy.lookup(planar, torch.from_numpy(shared).to(dev), torch.from_numpy(lv_p).to(dev)),
                       glossy.lookup(ct, torch.from_numpy(shared).to(dev), torch.from_numpy(lv_p).to(dev)))
    # map n does not depend on the batch
    one = glossy.lookup(ct[1:2], torch.from_numpy(per_map[1:2]).to(dev), torch.from_numpy(lv_np[1:2]).to(dev))
    assert torch.equal(one[0], glossy.lookup(ct, torch.from_numpy(per_map).to(dev), torch.from_numpy(lv_np).to(dev))[1])


@pytest.mark.parametrize("H,W", [(8, 16), (16, 32)])
def test_lookup_special_directions_and_pixel_centres(H, W):
    from reni_amd.utils import get_directions
    dev = _dev()
    g = np.random.default_rng(50 + H)
    chain = g.random((3, 3, H, W, 3)).astype(np.float32)
    ct = torch.from_numpy(chain).to(dev)
    eps = 1e-4
    special = np.asarray([[0, 1, 0], [0, -1, 0], [0, 5, 0], [0, -0.01, 0], [0, 0, 0], [-0.0, 0.0, -0.0],  # poles, zero
                          [0, 0, 1], [0, 0.5, 1], [1e-7, 0, 1], [-1e-7, 0, 1], [0, -0.5, 3], [-0.0, 0.2, 1],  # the +-pi seam
                          [eps, 1, 0], [-eps, 1, eps], [0, -1, eps], [eps, -1, -eps], [1e-3, 1, 1e-3], [3e-2, -1, 1e-2],  # caps
                          [0, 0, -1], [1, 0, 0], [-1, 0, 0]], np.float32)
    lo, hi = chain.reshape(3, 3, -1).min(2), chain.reshape(3, 3, -1).max(2)
    for level in (None, 0.5, 2.0, 7.0, -3.0, float("nan")):
        out = glossy.lookup(ct, torch.from_numpy(special).to(dev), level).cpu().numpy()
        assert np.isfinite(out).all(), level
        lv = 0.0 if level is None or level != level else min(max(level, 0.0), 2.0)
        l0, l1 = int(np.floor(lv)), min(int(np.floor(lv)) + 1, 2)
        slack = 8 * 2.0 ** -24
        for n in range(3):
            assert (out[n] >= min(lo[n, l0], lo[n, l1]) - slack).all() and (out[n] <= max(hi[n, l0], hi[n, l1]) + slack).all()
    # every pixel-centre direction reproduces the map, at every level, within the oracle's bound at those directions
    cd = get_directions(W)[0]
    for l in range(3):
        out = glossy.lookup(ct, cd.to(dev), float(l)).double().cpu().numpy()
        for n in range(3):
            val, bound, keep = np_lookup_chain(chain[n], cd.numpy(), np.full(H * W, float(l), np.float32))
            assert keep.all()
            assert (np.abs(out[n] - chain[n, l].reshape(-1, 3)) <= bound).all(), (l, n)


# ------------------------------------------------------------------------------------------ consumers
def _envmap(B, W, seed):
    from reni_amd.envmap_shader import EnvironmentMap
    from reni_amd.utils import get_directions, get_sineweight
    g = torch.Generator().manual_seed(seed)
    D, Sw = get_directions(W), get_sineweight(W)
    C = torch.rand(B, D.shape[1], 3, generator=g) * 2
    return EnvironmentMap(environment_map=C.to(_dev()), directions=D.expand(B, -1, -1).to(_dev()), sineweight=Sw.to(_dev()))


def test_shade_prefiltered_is_its_composition_and_zero_on_the_background():
    from reni_amd.mesh import build_hip_renderer
    from reni_amd.utils import get_directions
    dev = _dev()
    renderer, R, T, mesh = build_hip_renderer(TEAPOT, 0, 32, 0.5, "cuda")
    _, nrm, pos = renderer.rasterizer.gbuffer(mesh, R, T)
    cam = renderer.camera_center
    env = _envmap(2, 32, 3)
    background = ~(nrm != 0).any(-1)
    assert 100 < int(background.sum()) < 32 * 32 - 100
    for s, Wo in ((20.0, 16), (500.0, 32)):
        out = glossy.shade_prefiltered(env, nrm, pos, cam, s, 0.3, 0.7, Wo)
        assert out.shape == (2, 32 * 32, 3) and torch.isfinite(out).all()
        assert torch.equal(out[:, background], torch.zeros_like(out[:, background]))
        assert float(out[:, ~background].min()) > 0
        # its own composition: one unnormalised two-lobe call with weight 1, two lookups, the shader's factors
        odirs = get_directions(Wo)[0].to(dev)
        ones = torch.ones(env.directions.shape[1], device=dev)
        chain = glossy.lobe_convolve(env.environment_map, env.directions[0], ones, odirs, [glossy.phong(1), glossy.blinn(s)],
                                     normalise=False).view(2, 2, Wo // 2, Wo, 3)
        n, r, mask = glossy.shading_dirs(nrm, pos, cam)
        want = (0.3 * glossy.lookup(chain, n, 0.0) + (glossy.blinn_phong_norm(s) * 0.7) * glossy.lookup(chain, r, 1.0)) * mask
        assert torch.equal(out, want)
        # r is the view direction mirrored at the normal: n . r = n . v, |r| = 1
        v = torch.nn.functional.normalize(cam.to(dev)[None] - pos, dim=-1)
        ok = ~background
        assert float(((n * r).sum(-1) - (n * v).sum(-1))[ok].abs().max()) < 1e-5 and float((r.norm(dim=-1) - 1)[ok].abs().max()) < 1e-5


def test_evaluate_glossy_adds_a_column_and_changes_no_other():
    from reni_amd import metrics
    from reni_amd.data import SyntheticEnvMapDataset
    from reni_amd.models import RENIAutoDecoder
    torch.manual_seed(0)
    model = RENIAutoDecoder(2, 9, "SO2", 64, 3, 3, True, "tanh", 30, 30, False)
    model.set_compute_dtype("f32").to(_dev())
    ds = SyntheticEnvMapDataset(2, 16, 32)
    plain, _ = metrics.evaluate(model, ds)
    table, means = metrics.evaluate(model, ds, glossy=[glossy.ggx(0.5)])
    assert set(table) == set(plain) | {"glossy_psnr_0"} and set(means) == set(table)
    assert table["glossy_psnr_0"].shape == (2,) and torch.isfinite(table["glossy_psnr_0"]).all()
    assert all(torch.equal(plain[k], table[k]) for k in plain)
    two, _ = metrics.evaluate(model, ds, diffuse=True, glossy=[glossy.ggx(1.0), glossy.ggx(0.5)])
    assert torch.equal(two["glossy_psnr_1"], table["glossy_psnr_0"])  # a lobe scores the same among others
    # ggx(1) is the clamped cosine, normalised: the irradiance times 1 / (1 + d), |d| <= 1.78e-3 at W = 32 (the grid's quadrature
    # error), for prediction and target alike: the error and the peak move by at most 0.4 % each, 0.04 dB together
    assert float((two["glossy_psnr_0"] - two["diffuse_psnr"]).abs().max()) < 0.1


def test_sh_glossy_agrees_with_the_prefiltered_reconstruction():
    """sh_glossy(c, phong(8), 32) against prefilter(sh_reconstruct(c, 64), out_width 32).  The two differ by quadrature and by
    the half-pixel offset between the SH grid and RENI's grid, which prefilter is handed here; that deviation is computed in
    float64 from the same fp32 numbers.  On top of it: the convolution's tolerance, and 1e-5 for each of the two fp32 SH
    reconstructions (tests/test_gpu_diffuse.py's figure for that kernel)."""
    from reni_amd import baselines
    from reni_amd.utils import get_directions
    from tests.test_baselines_cpu import np_sh_basis
    dev = _dev()
    lobe = glossy.phong(8)
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(2, 32, 64, 3, generator=g) + torch.linspace(0, 2, 64)[None, None, :, None]).to(dev)
    c = baselines.sh_project(x, 3)
    a = glossy.sh_glossy(c, lobe, 32)
    rec = baselines.sh_reconstruct(c, 64)
    b = glossy.prefilter(rec, [lobe], out_width=32)[:, 0]
    assert a.shape == b.shape == (2, 16, 32, 3)
    c64 = c.double().cpu().numpy()
    lam = glossy.lobe_band_scale(lobe, 3)[[int(np.sqrt(t)) for t in range(16)]]
    a64 = np.einsum("yxt,ntc->nyxc", np_sh_basis(32, 3), c64 * lam[None, :, None])
    b64 = np_lobe_convolve(rec.cpu().numpy().reshape(2, -1, 3), get_directions(64)[0].numpy(),
                           baselines.reni_grid_weights(64).astype(np.float32), get_directions(32)[0].numpy(),
                           [tuple(lobe)])[:, 0].reshape(2, 16, 32, 3)
    dev64 = np.abs(a64 - b64).max()
    got = float((a - b).abs().max())
    scale = np.abs(b64).max()
    print(f"sh_glossy against prefilter: device {got:.4g}, float64 {dev64:.4g} (max {scale:.3g})")
    assert got <= dev64 + (lobe_tol(tuple(lobe)) + 2e-5) * scale
    # each side against its own float64 value
    assert np.abs(a.double().cpu().numpy() - a64).max() <= 1e-5 * np.abs(a64).max()
    assert np.abs(b.double().cpu().numpy() - b64).max() <= lobe_tol(tuple(lobe)) * scale
