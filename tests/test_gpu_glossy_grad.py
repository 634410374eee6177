"""GPU tests of differentiable glossy lighting: the transposed lobe convolution and the transposed lookup
(reni_tu_glossy_bwd.hip through reni_amd.ops), the autograd functions of reni_amd.glossy, and FIT_INVERSE through
``glossy.PrefilteredRenderer``.

The tolerances are derived, not measured: tests/test_glossy_cpu.py::lobe_tol per lobe for the convolution (twice it when
the call normalises: once for the sums, once for the fp32 denominators they are divided by), and
tests/test_glossy_grad_cpu.py::lookup_transpose_check's (8 + n_t) EPS32 (|J|^T |g|) for the lookup."""
import json
import os

import numpy as np
import pytest
import torch

from reni_amd import glossy, ops
from tests.test_glossy_cpu import lobe_tol
from tests.test_glossy_grad_cpu import lookup_transpose_case, lookup_transpose_check
from tests.test_gpu_glossy import LOBES, NMAX, TEAPOT, _lobe64, _unit
from tests.test_rotate_cpu import EPS32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
SHAPES = [(5003, 777), (1001, 2000)]  # (P, Q): the first splits the o range, has an odd P and a Q that is no multiple of 256
SCALE = 0.75
# what ops.launch_count() rises by for a call whose input requires no grad -- measured on the commit before this feature and
# after it: the forward entries of reni_tu_glossy.hip do not count their launches
LAUNCHES_NO_GRAD = {"lobe_convolve": 0, "prefilter": 0, "lookup": 0, "shade_prefiltered": 0}


def _kp(lobes):
    return [l.kind for l in lobes], [l.param for l in lobes]


# ------------------------------------------------------------------------------------------ convolution transpose
_CASES = {}


def _case(P, Q):
    """inputs and the float64 reference of a shape, computed once and shared: refN / refU [Lv, NMAX, Q, 3] =
    w_q sum_p A_l[p, q] g[n, l, p, c] r_l[p] with r = 1 / den_l[p] (normalised) and r = SCALE, 256 rows p at a time"""
    if (P, Q) not in _CASES:
        gen = torch.Generator().manual_seed(P + Q + 1)
        in_dirs, out_dirs = _unit(gen, Q).to(DEV), _unit(gen, P).to(DEV)
        w = (torch.rand(Q, generator=gen) * 4 * np.pi / Q).to(DEV)
        g = torch.randn(NMAX, len(LOBES), P, 3, generator=gen).to(DEV)
        d, w64 = in_dirs.double(), w.double()
        refN = torch.zeros(len(LOBES), NMAX, Q, 3, dtype=torch.float64, device=DEV)
        refU = torch.zeros_like(refN)
        for o0 in range(0, P, 256):
            t = out_dirs[o0:o0 + 256].double() @ d.T
            A = torch.stack([_lobe64(l, t) for l in LOBES]) * w64  # [Lv, p, Q]
            den = A.sum(2)
            assert bool((den > 0).all())
            gg = g[:, :, o0:o0 + 256].double()
            refN += torch.einsum("lpq,nlpc->lnqc", A, gg / den[None, :, :, None])
            refU += SCALE * torch.einsum("lpq,nlpc->lnqc", A, gg)
        kinds, params = _kp(LOBES)
        den32 = ops.lobe_denominators(in_dirs, w, out_dirs, kinds, params)
        _CASES[(P, Q)] = (in_dirs, out_dirs, w, g, den32, refN.cpu().numpy(), refU.cpu().numpy())
    return _CASES[(P, Q)]


@pytest.mark.parametrize("P,Q", SHAPES)
def test_lobe_convolve_backward_matches_float64(P, Q):
    in_dirs, out_dirs, w, g, den, refN, refU = _case(P, Q)
    kinds, params = _kp(LOBES)
    for N in (1, 11, NMAX):  # 3, 33, 66 colour columns: across the 32- and 64-column group edges
        bound = {True: 0.0, False: 0.0}
        for k, lobe in enumerate(LOBES):
            gk = g[:N, k:k + 1].contiguous()
            for normalise, ref, factor in ((True, refN[k, :N], 2.0), (False, refU[k, :N], 1.0)):
                out = ops.lobe_convolve_backward(gk, in_dirs, w, out_dirs, [lobe.kind], [lobe.param], normalise, SCALE,
                                                 den=den[k:k + 1] if normalise else None)
                assert out.shape == (N, Q, 3) and bool(torch.isfinite(out).all())
                err = np.abs(out.double().cpu().numpy() - ref).max()
                tol = factor * lobe_tol(tuple(lobe)) * np.abs(ref).max()
                bound[normalise] += tol
                print(f"transpose N={N} P={P} Q={Q} {'normalised' if normalise else 'unnormalised'} {lobe.kind}({lobe.param:g}): "
                      f"error / tolerance {err / tol:.3f}")
                assert err <= tol, (N, lobe, normalise, err, tol)
        gN = g[:N].contiguous()
        for normalise, ref in ((True, refN[:, :N].sum(0)), (False, refU[:, :N].sum(0))):
            out = ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, kinds, params, normalise, SCALE, den=den if normalise else None)
            err = np.abs(out.double().cpu().numpy() - ref).max()
            print(f"transpose N={N} P={P} Q={Q} all nine lobes, {'normalised' if normalise else 'unnormalised'}: "
                  f"error / sum of the lobes' tolerances {err / bound[normalise]:.3f}")
            assert err <= bound[normalise], (N, normalise, err, bound[normalise])
            planar = ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, kinds, params, normalise, SCALE,
                                                den=den if normalise else None, planar=True)
            assert planar.shape == (N, 3, Q) and torch.equal(planar.permute(0, 2, 1), out)
        # the denominators are computed inside when they are not handed in: the same bits
        assert torch.equal(ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, kinds, params, True),
                           ops.lobe_convolve_backward(gN, in_dirs, w, out_dirs, kinds, params, True, den=den))


def test_denominators_are_the_forwards():
    P, Q = SHAPES[0]
    in_dirs, out_dirs, w, _, den, _, _ = _case(P, Q)
    ones = torch.ones(1, Q, 3, device=DEV)
    raw = glossy.lobe_convolve(ones, in_dirs, w, out_dirs, LOBES, normalise=False, scale=1.0)
    for c in range(3):
        assert torch.equal(raw[0, :, :, c], den)
    norm = glossy.lobe_convolve(ones, in_dirs, w, out_dirs, LOBES, normalise=True)
    assert float(((raw / norm)[0, :, :, 0] - den).abs().div(den).max()) <= 2 * 2 * EPS32  # 2 ulp
    # a shape whose forward splits the i range: (P, Q) = (777, 5003) of tests/test_gpu_glossy.py
    gen = torch.Generator().manual_seed(5)
    d2, o2 = _unit(gen, 5003).to(DEV), _unit(gen, 777).to(DEV)
    w2 = (torch.rand(5003, generator=gen) * 4 * np.pi / 5003).to(DEV)
    kinds, params = _kp(LOBES)
    den2 = ops.lobe_denominators(d2, w2, o2, kinds, params)
    raw2 = glossy.lobe_convolve(torch.ones(1, 5003, 3, device=DEV), d2, w2, o2, LOBES, normalise=False, scale=1.0)
    assert den2.shape == (len(LOBES), 777) and torch.equal(raw2[0, :, :, 1], den2)
    # a lobe's denominators do not depend on the lobes around it
    assert torch.equal(ops.lobe_denominators(d2, w2, o2, kinds[4:5], params[4:5])[0], den2[4])


def test_transpose_is_deterministic_and_batch_independent():
    P, Q = SHAPES[0]
    in_dirs, out_dirs, w, g, den, _, _ = _case(P, Q)
    lib = ops._lib.load()
    slabs = [lib.reni_lobe_backward_workspace_bytes(1, p, Q, 1) - 256 - ((4 * p + 255) & ~255) for p in (2048, P)]
    assert slabs[1] == 2 * slabs[0]  # the o range is split in two at this shape
    kinds, params = _kp(LOBES)
    for normalise in (True, False):
        kw = dict(normalise=normalise, scale=SCALE, den=den if normalise else None)
        full = ops.lobe_convolve_backward(g, in_dirs, w, out_dirs, kinds, params, **kw)
        assert torch.equal(ops.lobe_convolve_backward(g, in_dirs, w, out_dirs, kinds, params, **kw), full)
        for n in (0, 10, 21):  # a map alone
            assert torch.equal(ops.lobe_convolve_backward(g[n:n + 1], in_dirs, w, out_dirs, kinds, params, **kw)[0], full[n]), n
        assert torch.equal(ops.lobe_convolve_backward(g[5:16], in_dirs, w, out_dirs, kinds, params, **kw), full[5:16])


def test_empty_lobe_contributes_zero():
    """phong(1e6) sees no texel among 64 random directions (tests/test_gpu_glossy.py::test_empty_lobe_gives_zero): its
    denominators are 0, its r is 0, and it adds exactly nothing -- no NaN -- alone or next to a lobe that is not empty"""
    gen = torch.Generator().manual_seed(29)
    in_dirs, out_dirs = _unit(gen, 64).to(DEV), _unit(gen, 300).to(DEV)
    w = (torch.rand(64, generator=gen) + 0.5).to(DEV)
    g = torch.randn(3, 2, 300, 3, generator=gen).to(DEV)
    empty, full = glossy.phong(1e6), glossy.phong(2)
    den = ops.lobe_denominators(in_dirs, w, out_dirs, *_kp([empty, full]))
    assert torch.equal(den[0], torch.zeros_like(den[0])) and float(den[1].min()) > 0
    for normalise in (True, False):
        alone = ops.lobe_convolve_backward(g[:, :1].contiguous(), in_dirs, w, out_dirs, *_kp([empty]), normalise=normalise)
        assert torch.equal(alone, torch.zeros_like(alone))
        both = ops.lobe_convolve_backward(g, in_dirs, w, out_dirs, *_kp([empty, full]), normalise=normalise)
        other = ops.lobe_convolve_backward(g[:, 1:].contiguous(), in_dirs, w, out_dirs, *_kp([full]), normalise=normalise)
        assert bool(torch.isfinite(both).all()) and torch.equal(both, other) and float(other.abs().max()) > 0


# ------------------------------------------------------------------------------------------ lookup transpose
def _device_J(Lv, H, W, dirs, level):
    """J [P, E] from the device forward itself on the E = Lv H W one-hot chains, shared directions"""
    E = Lv * H * W
    chains = torch.zeros(E, E, 3, device=DEV)
    chains[torch.arange(E), torch.arange(E)] = 1.0
    out = glossy.lookup(chains.view(E, Lv, H, W, 3), dirs, level)  # [E, P, 3]
    assert torch.equal(out[:, :, 0], out[:, :, 1]) and torch.equal(out[:, :, 0], out[:, :, 2])
    return out[:, :, 0].T.contiguous().cpu().numpy()


@pytest.mark.parametrize("H,W", [(8, 16), (16, 32)])
def test_lookup_backward_matches_the_forwards_matrix(H, W):
    Lv, E = 3, 3 * H * W
    cases = [lookup_transpose_case(H, W, seed) for seed in range(3)]
    dirs = torch.from_numpy(np.stack([c[0] for c in cases])).to(DEV)    # [3, P, 3]
    level = torch.from_numpy(np.stack([c[1] for c in cases])).to(DEV)  # [3, P]
    g = torch.randn(3, 4096, 3, generator=torch.Generator().manual_seed(H)).to(DEV)
    g64 = g.double().cpu().numpy()
    J = [_device_J(Lv, H, W, dirs[n], level[n]) for n in range(3)]
    # shared directions and levels: one table serves the three maps
    out = ops.envmap_lookup_backward(g, Lv, H, W, dirs[0], level[0])
    assert out.shape == (3, Lv, H, W, 3)
    table = ops.envmap_lookup_table(3, Lv, H, W, dirs[0], level[0])
    assert table[0].shape == (1, 4096, 8) and table[1].shape == (1, 8 * 4096) and table[2].shape == (1, E + 1)
    for n in range(3):
        lookup_transpose_check(out[n].reshape(E, 3).cpu().numpy(), J[0], g64[n], f"{H} x {W} shared, map {n}")
    assert torch.equal(ops.envmap_lookup_backward(g, Lv, H, W, dirs[0], level[0]), out)
    assert torch.equal(ops.envmap_lookup_backward(g, Lv, H, W, table=table), out)
    assert torch.equal(ops.envmap_lookup_backward(g[1:2], Lv, H, W, dirs[0], level[0])[0], out[1])  # a map alone
    # per-map directions [N, P, 3] and per-map levels [N, P]: a table a map
    per = ops.envmap_lookup_backward(g, Lv, H, W, dirs, level)
    assert ops.envmap_lookup_table(3, Lv, H, W, dirs, level)[0].shape == (3, 4096, 8)
    for n in range(3):
        lookup_transpose_check(per[n].reshape(E, 3).cpu().numpy(), J[n], g64[n], f"{H} x {W} per map, map {n}")
    assert torch.equal(per[0], out[0])
    assert torch.equal(ops.envmap_lookup_backward(g, Lv, H, W, dirs, level), per)
    # per-map directions with a shared level, and the other way round
    mixed = ops.envmap_lookup_backward(g, Lv, H, W, dirs, level[0])
    assert torch.equal(mixed[0], out[0])
    assert torch.equal(ops.envmap_lookup_backward(g, Lv, H, W, dirs[0], level)[0], out[0])
    # a strided chain (a view with a non-unit column stride), through autograd: the gradient lands in the view's columns
    base = torch.rand(3, Lv, H, 2 * W, 3, device=DEV).requires_grad_()
    view = base[:, :, :, ::2]
    assert view.stride(3) == 6
    glossy.lookup(view, dirs[0], level[0]).backward(g)
    assert torch.equal(base.grad[:, :, :, ::2], out) and float(base.grad[:, :, :, 1::2].abs().max()) == 0.0
    # plain maps [N, H, W, 3] are a chain of one level
    maps = torch.rand(3, H, W, 3, device=DEV).requires_grad_()
    glossy.lookup(maps, dirs[0]).backward(g)
    assert maps.grad.shape == (3, H, W, 3)
    assert torch.equal(maps.grad, ops.envmap_lookup_backward(g, 1, H, W, dirs[0]).view(3, H, W, 3))


# ------------------------------------------------------------------------------------------ autograd
def _env(x, W):
    """EnvironmentMap whose environment_map IS x (no sine weight), on RENI's W grid"""
    from reni_amd.envmap_shader import EnvironmentMap
    from reni_amd.utils import get_directions
    env = EnvironmentMap.__new__(EnvironmentMap)
    env.directions = get_directions(W).to(DEV).expand(x.shape[0], -1, -1)
    env.environment_map = x
    return env


def _hand_shade_backward(gcolors, B, W, nrm, pos, cam, s, kd, ks, Wo):
    """d loss / d environment_map [B, H W, 3] of glossy.shade_prefiltered for the upstream gcolors [B, NP, 3], chained by hand
    from ops.envmap_lookup_backward and ops.lobe_convolve_backward"""
    from reni_amd.utils import get_directions
    n, r, mask = glossy.shading_dirs(nrm, pos, cam)
    gm = gcolors * mask
    gchain = (ops.envmap_lookup_backward(gm * float(kd), 2, Wo // 2, Wo, n, 0.0)
              + ops.envmap_lookup_backward(gm * (glossy.blinn_phong_norm(s) * float(ks)), 2, Wo // 2, Wo, r, 1.0))
    grid = get_directions(W)[0].to(DEV)
    return ops.lobe_convolve_backward(gchain.view(B, 2, -1, 3), grid, torch.ones(grid.shape[0], device=DEV),
                                      get_directions(Wo)[0].to(DEV), ["phong", "blinn"], [1.0, s], normalise=False, scale=1.0)


def _teapot(kd, size=32):
    from reni_amd.mesh import build_hip_renderer
    renderer, R, T, mesh = build_hip_renderer(TEAPOT, 0, size, kd, "cuda")
    return renderer, dict(meshes_world=mesh, R=R, T=T)


def test_autograd_wiring_and_nothing_extra_without_grad():
    """x.grad of the four public functions equals the ops.*_backward results; without requires_grad there is no grad_fn and
    the launch counter rises by what it rose before the feature.  Before the feature ``.backward()`` raised here."""
    from reni_amd.baselines import reni_grid_weights
    from reni_amd.utils import get_directions
    gen = torch.Generator().manual_seed(3)
    Q, P = 700, 300
    in_dirs, out_dirs = _unit(gen, Q).to(DEV), _unit(gen, P).to(DEV)
    w = (torch.rand(Q, generator=gen) * 4 * np.pi / Q).to(DEV)
    lobes = [glossy.phong(8), glossy.blinn(20), glossy.ggx(0.5)]
    kinds, params = _kp(lobes)
    x0 = torch.rand(2, Q, 3, generator=gen).to(DEV)
    y = torch.randn(2, 3, P, 3, generator=gen).to(DEV)
    # ---- lobe_convolve, interleaved and planar, normalised and not
    for normalise in (True, False):
        want = ops.lobe_convolve_backward(y, in_dirs, w, out_dirs, kinds, params, normalise, 0.5)
        x = x0.clone().requires_grad_()
        out = glossy.lobe_convolve(x, in_dirs, w, out_dirs, lobes, normalise=normalise, scale=0.5)
        assert out.requires_grad and torch.equal(out, glossy.lobe_convolve(x0, in_dirs, w, out_dirs, lobes, normalise=normalise, scale=0.5))
        out.backward(y)
        assert torch.equal(x.grad, want)
        xp = x0.permute(0, 2, 1).contiguous().requires_grad_()  # [N, 3, Q]
        glossy.lobe_convolve(xp, in_dirs, w, out_dirs, lobes, normalise=normalise, scale=0.5).backward(y)
        assert xp.grad.shape == (2, 3, Q) and torch.equal(xp.grad.permute(0, 2, 1), want)
    # ---- prefilter, flat and [N, H, W, 3]; the denominators come from the cache the second time
    W, Wo = 16, 8
    e0 = torch.rand(2, 8 * 16, 3, generator=gen).to(DEV)
    yp = torch.randn(2, 3, 4 * 8, 3, generator=gen).to(DEV)
    d16, w16 = get_directions(W)[0].to(DEV), torch.from_numpy(reni_grid_weights(W).astype(np.float32)).to(DEV)
    want = ops.lobe_convolve_backward(yp, d16, w16, get_directions(Wo)[0].to(DEV), kinds, params, True)
    counts = []
    for shape in ((2, 8 * 16, 3), (2, 8, 16, 3)):
        e = e0.clone().view(shape).requires_grad_()
        before = ops.launch_count()
        out = glossy.prefilter(e, lobes, out_width=Wo)
        out.backward(yp.view(out.shape))
        counts.append(ops.launch_count() - before)
        assert e.grad.shape == shape and torch.equal(e.grad.view(2, -1, 3), want)
    assert counts[0] == counts[1] + 4 and counts[1] == 5  # three kinds + finish for the denominators; recip, three kinds, finish
    # ---- lookup
    c0 = torch.rand(2, 3, 8, 16, 3, generator=gen).to(DEV)
    dirs = torch.randn(500, 3, generator=gen).to(DEV)
    level = (torch.rand(500, generator=gen) * 2.4).to(DEV)
    yl = torch.randn(2, 500, 3, generator=gen).to(DEV)
    c = c0.clone().requires_grad_()
    out = glossy.lookup(c, dirs, level)
    assert torch.equal(out, glossy.lookup(c0, dirs, level))
    out.backward(yl)
    assert torch.equal(c.grad, ops.envmap_lookup_backward(yl, 3, 8, 16, dirs, level))
    # ---- shade_prefiltered
    renderer, kw = _teapot(0.5)
    _, nrm, pos = renderer.rasterizer.gbuffer(kw["meshes_world"], kw["R"], kw["T"])
    cam = torch.tensor([0.0, 0.0, 2.0])
    m0 = (torch.rand(2, 8 * 16, 3, generator=gen) * 2).to(DEV)
    ys = torch.randn(2, 32 * 32, 3, generator=gen).to(DEV)
    m = m0.clone().requires_grad_()
    out = glossy.shade_prefiltered(_env(m, 16), nrm, pos, cam, 20.0, 0.3, 0.7, 8)
    assert torch.equal(out, glossy.shade_prefiltered(_env(m0, 16), nrm, pos, cam, 20.0, 0.3, 0.7, 8))
    out.backward(ys)
    assert torch.equal(m.grad, _hand_shade_backward(ys, 2, 16, nrm, pos, cam, 20.0, 0.3, 0.7, 8))
    assert float(m.grad.abs().max()) > 0
    # ---- nothing requires grad: no grad_fn, and not one launch more than before the feature
    calls = {"lobe_convolve": lambda: glossy.lobe_convolve(x0, in_dirs, w, out_dirs, lobes),
             "prefilter": lambda: glossy.prefilter(e0, lobes, out_width=Wo),
             "lookup": lambda: glossy.lookup(c0, dirs, level),
             "shade_prefiltered": lambda: glossy.shade_prefiltered(_env(m0, 16), nrm, pos, cam, 20.0, 0.3, 0.7, 8)}
    for name, fn in calls.items():
        before = ops.launch_count()
        out = fn()
        rose = ops.launch_count() - before
        print(f"{name} without grad: {rose} counted launches")
        assert out.grad_fn is None and not out.requires_grad and rose == LAUNCHES_NO_GRAD[name], name
    with torch.no_grad():  # a map that requires grad under no_grad: the plain path too
        assert glossy.lookup(c, dirs, level).grad_fn is None
    with pytest.raises(ValueError, match="dirs requires grad"):
        glossy.lookup(c0, dirs.clone().requires_grad_(), level)


# ------------------------------------------------------------------------------------------ the public renderer
def diffuse_parity(Wo, size=32, W=16):
    """max |PrefilteredRenderer - HipMeshRenderer| over the covered pixels relative to the latter's largest value, kd = 1, the
    teapot at size x size, two random maps of width W times the sine weight: the figure profiles/glossy_time.jsonl records as
    "diffuse only" (profiles/tools/gpu_glossy_grad_time.py --only parity writes the line)"""
    from reni_amd.envmap_shader import EnvironmentMap
    from reni_amd.utils import get_directions, get_sineweight
    renderer, kw = _teapot(1.0, size)
    pr = glossy.PrefilteredRenderer(renderer.rasterizer, kd=1.0, out_width=Wo)
    assert torch.equal(pr.camera_center, renderer.camera_center)
    g = torch.Generator().manual_seed(16)
    C = (torch.rand(2, W * W // 2, 3, generator=g) * 2).to(DEV)
    env = EnvironmentMap(environment_map=C, directions=get_directions(W).expand(2, -1, -1).to(DEV), sineweight=get_sineweight(W).to(DEV))
    with torch.no_grad():
        ref, nref = renderer(envmap=env, **kw)
        out, nout = pr(envmap=env, **kw)
    assert out.shape == ref.shape == (2, size, size, 3) and torch.equal(nout, nref)
    covered = (nref[0] != 0).any(-1)
    assert float(out[:, ~covered].abs().max()) == 0.0
    return float((out - ref)[:, covered].abs().max() / ref[:, covered].max())


def _largest_segment(table):
    """the largest number of taps of non-zero weight that one texel gathers"""
    wgt, order, offsets = table
    nz = torch.cat([torch.zeros(1, dtype=torch.int64, device=wgt.device), (wgt.reshape(-1)[order[0]] != 0).long().cumsum(0)])
    return int((nz[offsets[0][1:]] - nz[offsets[0][:-1]]).max())


def _recorded_parity(Wo, W=16):
    rows = [json.loads(l) for l in open(os.path.join(ROOT, "profiles", "glossy_time.jsonl")) if l.strip()]
    rows = [r for r in rows if r.get("teapot") == "diffuse only" and r.get("out_width") == Wo and r.get("map_width") == W]
    assert len(rows) == 1, f"profiles/glossy_time.jsonl has no 'diffuse only' line for out_width {Wo} on a width-{W} map"
    return rows[0]["max_rel"]


@pytest.mark.parametrize("Wo", [8, 16])
def test_prefiltered_renderer_adjoint_identity_and_diffuse_parity(Wo):
    """<A x, y> = <x, A^T y> through the public renderer up to tol_A max|A x| sum|y| + tol_T max|A^T y| sum|x|.  The tolerances
    are the max-relative ones of the two operators for the two lobes involved, phong(1) and blinn(500), both unnormalised:
    lobe_tol of each, plus the lookup's -- forward 8 + 4 roundings (a tap's weights and value, four taps summed), transposed
    8 + n_t with n_t the largest number of taps that land on one texel of this G-buffer."""
    gen = torch.Generator().manual_seed(Wo)
    renderer, kw = _teapot(0.6)
    pr = glossy.PrefilteredRenderer(renderer.rasterizer, kd=0.6, out_width=Wo)
    assert pr.ks == pytest.approx(0.4) and pr.shininess == 500.0
    x = (torch.rand(2, 8 * 16, 3, generator=gen) * 2).to(DEV).requires_grad_()
    y = torch.randn(2, 32, 32, 3, generator=gen).to(DEV)
    Ax, normals = pr(envmap=_env(x, 16), **kw)
    assert Ax.shape == (2, 32, 32, 3) and normals.shape == (2, 32, 32, 3)
    (ATy,) = torch.autograd.grad(Ax, x, y)
    _, nrm, pos = renderer.rasterizer.gbuffer(kw["meshes_world"], kw["R"], kw["T"])
    n, r, _ = glossy.shading_dirs(nrm, pos, pr.camera_center)
    nt = max(_largest_segment(ops.envmap_lookup_table(2, 2, Wo // 2, Wo, d, lv)) for d, lv in ((n, 0.0), (r, 1.0)))
    conv = lobe_tol(("phong", 1.0)) + lobe_tol(("blinn", 500.0))
    tol_A, tol_T = conv + (8 + 4) * EPS32, conv + (8 + nt) * EPS32
    lhs = float((Ax.detach().double() * y.double()).sum())
    rhs = float((x.detach().double() * ATy.double()).sum())
    bound = tol_A * float(Ax.abs().max()) * float(y.abs().sum()) + tol_T * float(ATy.abs().max()) * float(x.detach().abs().sum())
    print(f"adjoint out_width {Wo}: <Ax, y> = {lhs:.6g}, <x, A^T y> = {rhs:.6g}, difference / bound {abs(lhs - rhs) / bound:.4f}, n_t {nt}")
    assert abs(lhs - rhs) <= bound
    # the gradient is the hand-chained one, and a G-buffer gives the same renderer
    from reni_amd.envmap_shader import GBuffer
    assert torch.equal(ATy, _hand_shade_backward(y.view(2, -1, 3), 2, 16, nrm, pos, pr.camera_center, 500.0, 0.6, 0.4, Wo))
    gb = glossy.PrefilteredRenderer(GBuffer(nrm.clone(), pos.clone(), pr.camera_center, 32), kd=0.6, out_width=Wo)
    assert torch.equal(gb(envmap=_env(x.detach(), 16))[0], Ax.detach())
    # kd = 1: the two renderers differ only by the lookup's interpolation
    got, rec = diffuse_parity(Wo), _recorded_parity(Wo)
    print(f"diffuse parity out_width {Wo}: max_rel {got:.5f}, recorded {rec:.5f}")
    assert got <= 2 * rec


def test_fit_inverse_with_the_prefiltered_renderer():
    """One FIT_INVERSE step with set_renderer(PrefilteredRenderer): a finite loss, a latent gradient that is non-zero for the
    batch's images and equals the one obtained by chaining ops.*_backward by hand behind the decoder; then a short fit ends
    with a lower loss than it started."""
    from reni_amd import trainer
    from reni_amd.data import SyntheticEnvMapDataset
    from reni_amd.lightning_module import RENI
    from tests.test_gpu_raster import _inverse_cfg
    ds = SyntheticEnvMapDataset(4, 16, 32)
    renderer, kw = _teapot(0.6)
    pr = glossy.PrefilteredRenderer(renderer.rasterizer, kd=0.6, out_width=16)
    torch.manual_seed(2)
    m = RENI(_inverse_cfg(TEAPOT, 0.6), "FIT_INVERSE", dataset=ds)
    m.setup()
    m.model.to(DEV)
    with torch.no_grad():
        m.model.mu.normal_()
    m.set_renderer(pr, kw)
    assert m.gt_renders.shape == (4, 32, 32, 3)
    idx = torch.tensor([0, 2]).to(DEV)
    imgs = torch.stack([ds[int(i)][0] for i in idx]).to(DEV)
    out = m.training_step((imgs, idx), 0)
    out["loss"].backward()
    lat = m.model.mu
    grad = lat.grad.clone()
    assert torch.isfinite(out["loss"]) and bool(torch.isfinite(grad).all())
    assert float(grad[idx].abs().max()) > 0 and float(grad[1].abs().max()) == 0.0  # image 1 was not in the batch
    # by hand: decoder -> unnormalise under autograd, the render's two operators through ops.*_backward
    lat.grad = None
    directions, sineweight = m._grids(imgs)
    Z = lat[idx]
    mo = m.dataset.unnormalise(m.model(Z, directions))
    with torch.no_grad():
        render = m.get_render(mo.detach(), directions, sineweight)
    render.requires_grad_()
    loss = m.criterion(render, m.gt_renders[idx], Z)[0]
    assert torch.equal(loss.detach(), out["loss"].detach())
    loss.backward(inputs=[render, lat], retain_graph=True)  # (Z = mu[idx] is part of the decoder's graph too)
    _, nrm, pos = renderer.rasterizer.gbuffer(kw["meshes_world"], kw["R"], kw["T"])
    genv = _hand_shade_backward(render.grad.reshape(2, -1, 3), 2, 32, nrm, pos, pr.camera_center, 500.0, 0.6, 0.4, 16)
    mo.backward(genv * sineweight, inputs=[lat])
    # (the latent's terms are added in another order than autograd adds them in one pass: a few ulp of the largest entry)
    diff = float((lat.grad - grad).abs().max())
    print(f"latent gradient by hand against autograd: largest difference {diff:.3g} of {float(grad.abs().max()):.3g}")
    assert diff <= 8 * EPS32 * float(grad.abs().max())
    # a short fit moves downhill
    torch.manual_seed(0)
    f = RENI(_inverse_cfg(TEAPOT, 0.6), "FIT_INVERSE", dataset=ds)
    f.setup()
    f.set_renderer(glossy.PrefilteredRenderer(renderer.rasterizer, kd=0.6, out_width=16), kw)
    hist = trainer.fit(f, max_epochs=8, device=DEV)
    assert isinstance(f.renderer, glossy.PrefilteredRenderer)
    print(f"FIT_INVERSE through PrefilteredRenderer: loss {hist[0]['loss']:.6g} -> {hist[-1]['loss']:.6g}")
    assert np.isfinite(hist[-1]["loss"]) and hist[-1]["loss"] < hist[0]["loss"]
