"""CPU tests of importance-sampled light lists (reni_amd.lighting, reni_tu_lights.hip).

Holds the float64 numpy restatement of include/reni_hip.h's definitions -- the luminance x solid-angle distribution
(np_light_table), inverse-CDF sampling (np_sample) and the diffuse sum over a light list (np_irradiance) -- that
tests/test_gpu_lighting.py compares the HIP kernels against.  The feature has no reference counterpart, so the restatement
is checked against itself (normalisation, the searchsorted rule, the estimator property) and the host side of the library
(argument checks, uniforms, the C ABI's validation) against the restatement."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import reni_oracle as O
from reni_amd import _lib, lighting, ops
from reni_amd.baselines import reni_grid_weights
from reni_amd.utils import get_directions, get_sineweight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUMA = np.asarray([0.2126, 0.7152, 0.0722])


# ------------------------------------------------------------------------------------------ numpy restatement
def np_omega(W):
    """[H] float64: the per-texel solid angle of every row as the library is handed it (the exact band value rounded to
    float32 once)"""
    return reni_grid_weights(W)[::W].astype(np.float32).astype(np.float64)


def np_row_cos(W):
    H = W // 2
    return np.cos(np.arange(H + 1, dtype=np.float64) * np.pi / H)


def np_unnormalise(x, minmax):
    """UnMinMaxNormlise as the device computes it: 0.5 (x + 1) in float32, then t * range + m0 as ONE fused multiply-add (the
    library is built with hipcc's default contraction, which fuses the last two operations of reni_dev_image.inc's expression:
    one rounding, the product is exact in float64); the exponential itself is exact here"""
    x = np.asarray(x, np.float32)
    rng, m0 = np.float32(minmax[1] - minmax[0]), np.float32(minmax[0])
    t = np.float32(0.5) * (x + np.float32(1.0))
    arg = (t.astype(np.float64) * np.float64(rng) + np.float64(m0)).astype(np.float32)
    return np.exp(arg.astype(np.float64))


def np_light_table(maps, omega, mask=None, eps=0.0):
    """maps [B, H, W, 3] radiance, omega [H], mask broadcastable to [B, H, W] -> (pmf [B, H, W], cond [B, H, W], marg [B, H]),
    float64"""
    maps = np.asarray(maps, np.float64)
    B, H, W, _ = maps.shape
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.maximum(maps @ LUMA, 0.0) * omega[None, :, None]
        if mask is not None:
            f = f * np.broadcast_to(np.asarray(mask, np.float64), (B, H, W))
        f = np.where(f > 0, f, 0.0)  # (a NaN fails the comparison)
        F = f.sum((1, 2))
    Om = (W * omega).sum()
    ok = np.isfinite(F) & (F > 0)
    e = np.where(ok, eps, 1.0)[:, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        imp = np.where(ok[:, None, None], f / np.where(ok, F, 1.0)[:, None, None], 0.0)
    pmf = (1.0 - e) * np.where(e < 1.0, imp, 0.0) + e * omega[None, :, None] / Om
    cs = np.cumsum(pmf, 2)
    rows = cs[:, :, -1]
    flat = (np.arange(W, dtype=np.float64) + 1.0) / W
    with np.errstate(invalid="ignore", divide="ignore"):
        cond = np.where(rows[:, :, None] > 0, cs / rows[:, :, None], flat[None, None, :])
    cm = np.cumsum(rows, 1)
    return pmf, cond, cm / cm[:, -1:]


def np_select(cond, marg, u):
    """The selection rule on given tables: (row, column) [B, S] for u [S, 2] or [B, S, 2]; searchsorted(side="right"),
    clamped"""
    B, H, W = cond.shape
    u = np.broadcast_to(u, (B,) + u.shape[-2:])
    rows = np.empty(u.shape[:2], np.int64)
    cols = np.empty(u.shape[:2], np.int64)
    for b in range(B):
        rows[b] = np.minimum(np.searchsorted(marg[b], u[b, :, 0], side="right"), H - 1)
        # (the rule as the header words it -- the number of entries <= u -- which is searchsorted on an ascending row)
        cols[b] = np.minimum((cond[b, rows[b]] <= u[b, :, 1, None]).sum(1), W - 1)
    return rows, cols


def np_sample(pmf, cond, marg, radiance, omega, u, dirs_table, texel_weight=None, jitter=False, row_cos=None):
    """Everything reni_light_sample returns, float64 (index int64), from GIVEN tables (any dtype: they are used as they are) and
    the radiance [B, H, W, 3] of the maps"""
    B, H, W = cond.shape
    i, j = np_select(cond, marg, u)
    S = i.shape[1]
    index = i * W + j
    bb = np.arange(B)[:, None]
    pm = np.asarray(pmf, np.float64)[bb, i, j]
    rad = np.asarray(radiance, np.float64)[bb, i, j]
    tw = 1.0 if texel_weight is None else np.asarray(texel_weight, np.float64)[index]
    with np.errstate(divide="ignore", invalid="ignore"):
        colors = rad * (tw / (S * pm))[..., None]
    if jitter:
        uu = np.broadcast_to(np.asarray(u, np.float64), (B, S, 2))
        mg, cd = np.asarray(marg, np.float64), np.asarray(cond, np.float64)
        lo_r = np.where(i > 0, mg[bb, np.maximum(i - 1, 0)], 0.0)
        lo_c = np.where(j > 0, cd[bb, i, np.maximum(j - 1, 0)], 0.0)
        tr = np.clip((uu[..., 0] - lo_r) / (mg[bb, i] - lo_r), 0.0, 1.0)
        tc = np.clip((uu[..., 1] - lo_c) / (cd[bb, i, j] - lo_c), 0.0, 1.0)
        cp = row_cos[i] - tr * (row_cos[i] - row_cos[i + 1])
        sp = np.sqrt(np.maximum(1.0 - cp * cp, 0.0))
        th = 2.0 * np.pi * (j + tc) / W - np.pi
        dirs = np.stack([sp * np.sin(th), cp, -sp * np.cos(th)], -1)
    else:
        dirs = np.asarray(dirs_table, np.float64)[index]
    return dict(index=index, dirs=dirs, pdf=pm / omega[i], radiance=rad, colors=colors)


def np_irradiance(normals, dirs, colors, scale=1.0 / np.pi):
    """[B, P, 3] = scale sum_s max(0, n_p . d_bs) colors_bs, float64; normals [P, 3] or [B, P, 3]"""
    n = np.asarray(normals, np.float64)
    n = np.broadcast_to(n, (dirs.shape[0],) + n.shape[-2:])
    A = np.maximum(np.einsum("bpk,bsk->bps", n, np.asarray(dirs, np.float64)), 0.0)
    return scale * np.einsum("bps,bsc->bpc", A, np.asarray(colors, np.float64))


def np_dirs(W):
    return get_directions(W)[0].double().numpy()


# ------------------------------------------------------------------------------------------ shared cases
def sky_maps(B, W, seed, zero_row=True):
    """[B, H, W, 3] float32 radiance over five decades, smooth plus noise; row 1 is black where there is one"""
    H = W // 2
    rng = np.random.default_rng(seed)
    d = np_dirs(W).reshape(H, W, 3)
    base = np.exp(3.0 * d[..., 1] + 1.5 * d[..., 0])[None, :, :, None]
    m = base * np.exp(rng.normal(0.0, 1.0, (B, H, W, 3)))
    m[rng.random((B, H, W)) < 0.01] *= 500.0
    if zero_row and H > 1:
        m[:, 1] = 0.0
    return m.astype(np.float32)


def lattice(n=64):
    """the n x n midpoint lattice of uniforms, [n n, 2] float32"""
    g = (np.arange(n, dtype=np.float64) + 0.5) / n
    return np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2).astype(np.float32)


SUN_SEED = 7


@functools.lru_cache(maxsize=None)
def sun_case():
    """The estimator case of both test files: a 32 x 64 map of smooth sky plus a 3-texel sun 3000 x brighter, 48 random
    normals, the 64 x 64 midpoint lattice.  Returns a dict with the map [1, H, W, 3] float32, normals [48, 3] float32, u,
    the exact irradiance (the full sum over texels), per uniform_mix the oracle's estimate and its largest error relative to the largest irradiance."""
    W, H = 64, 32
    rng = np.random.default_rng(SUN_SEED)
    d = np_dirs(W).reshape(H, W, 3)
    sky = (0.6 + 0.4 * d[..., 1])[..., None] * np.asarray([0.5, 0.7, 1.0]) + 0.05
    m = sky.copy()
    m[9, 40:43] = 3000.0 * sky[9, 40:43] * np.asarray([1.0, 0.9, 0.7])
    m = m[None].astype(np.float32)
    n = rng.normal(size=(48, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    u = lattice(64)
    omega = np_omega(W)
    tw = np.repeat(omega, W)
    rad = m.astype(np.float64)
    exact = np_irradiance(n, np_dirs(W)[None], rad.reshape(1, -1, 3) * tw[None, :, None])
    out = dict(W=W, H=H, maps=m, normals=n, u=u, exact=exact, estimate={}, error={})
    for eps in (0.0, 0.25, 1.0):
        pmf, cond, marg = np_light_table(rad, omega, eps=eps)
        s = np_sample(pmf, cond, marg, rad, omega, u, np_dirs(W), tw)
        est = np_irradiance(n, s["dirs"], s["colors"])
        out["estimate"][eps] = est
        out["error"][eps] = float(np.abs(est - exact).max() / exact.max())  # relative to the largest irradiance, as tests' `rel`
    # the FIT_INVERSE shader's diffuse sum (kd = 1, ks = 0) over the sine-weighted map, all texels against the sampled lights
    sw = get_sineweight(W)[0, :, 0].double().numpy()
    cosines = lambda dirs: np.clip(np.einsum("pk,bsk->bps", n.astype(np.float64), dirs), 0.0, 1.0)  # noqa: E731
    full = np.einsum("bps,bsc->bpc", cosines(np_dirs(W)[None]), rad.reshape(1, -1, 3) * sw[None, :, None])
    pmf, cond, marg = np_light_table(rad, omega)
    s = np_sample(pmf, cond, marg, rad, omega, u, np_dirs(W), sw)
    out["shade_error"] = float(np.abs(np.einsum("bps,bsc->bpc", cosines(s["dirs"]), s["colors"]) - full).max() / full.max())
    return out


# ------------------------------------------------------------------------------------------ 1. the restatement against itself
@pytest.mark.parametrize("W", [2, 8, 66])
def test_oracle_tables_are_normalised(W):
    m = sky_maps(3, W, W).astype(np.float64)
    for eps in (0.0, 0.25, 1.0):
        pmf, cond, marg = np_light_table(m, np_omega(W), eps=eps)
        assert np.abs(pmf.sum((1, 2)) - 1.0).max() < 1e-13
        assert np.all(cond[:, :, -1] == 1.0) and np.all(marg[:, -1] == 1.0)
        assert np.all(np.diff(cond, axis=2) >= 0) and np.all(np.diff(marg, axis=1) >= 0)
        if eps == 0.0 and W > 2:  # the black row: a flat conditional, no marginal mass
            assert np.allclose(cond[:, 1], (np.arange(W) + 1.0) / W) and np.all(marg[:, 1] == marg[:, 0])
        if eps == 1.0:
            assert np.allclose(pmf, (np_omega(W) / (4 * np.pi))[None, :, None], rtol=1e-6)
    # an image without finite positive importance falls back to the uniform table
    bad = m.copy()
    bad[0] = 0.0
    bad[1, 0, 0, 0] = np.inf
    bad[2, 0, 0, 1] = np.nan
    got = np_light_table(bad, np_omega(W))
    uni = np_light_table(m, np_omega(W), eps=1.0)
    for g, r in zip(got, uni):
        assert np.array_equal(g[:2], r[:2])
    assert np.isfinite(got[0][2]).all() and abs(got[0][2].sum() - 1.0) < 1e-13  # the NaN texel alone counts as 0


def test_oracle_never_selects_a_masked_texel():
    W, H = 66, 33
    m = sky_maps(2, W, 3, zero_row=False).astype(np.float64)
    mask = np.ones((H, W))
    mask[:, W // 2:] = 0.0
    pmf, cond, marg = np_light_table(m, np_omega(W), mask=mask)
    rng = np.random.default_rng(5)
    u = rng.random((4096, 2)).astype(np.float32)
    edge = np.asarray([0.0, np.nextafter(np.float32(1.0), np.float32(0.0))], np.float32)
    u = np.concatenate([u, np.stack(np.meshgrid(edge, edge), -1).reshape(-1, 2)])
    i, j = np_select(cond, marg, u)
    assert j.max() < W // 2 and np.all(pmf[np.arange(2)[:, None], i, j] > 0)
    assert i.min() == 0 and i.max() == H - 1  # the edge values reach the first and the last row


def test_importance_estimator_beats_uniform_sampling():
    """Largest irradiance error over 48 normals x 3 channels, relative to the largest irradiance, with 4096 lattice samples,
    float64 oracle alone: importance sampling 5.1e-3 (uniform_mix 0) and 8.2e-3 (0.25), uniform solid-angle sampling 2.0e-1 --
    a factor of 24 to 38 where the assertion asks for 2 (and, of this seed, for 4)."""
    c = sun_case()
    print("largest relative irradiance error:", c["error"], "of the shader's diffuse sum:", c["shade_error"])
    for eps in (0.0, 0.25):
        assert c["error"][eps] < 0.5 * c["error"][1.0], c["error"]
    assert c["error"][1.0] >= 4.0 * max(c["error"][0.0], c["error"][0.25]), c["error"]  # the seed's margin over the factor of 2
    assert c["shade_error"] < 0.5 * c["error"][1.0]


# ------------------------------------------------------------------------------------------ 2. uniforms
def test_uniforms():
    g = lambda: torch.Generator().manual_seed(11)  # noqa: E731
    for kind, S in (("random", 1000), ("stratified", 4096), ("stratified", 12), ("stratified", 6 * 35)):
        u = lighting.uniforms(S, kind, g())
        assert u.shape == (S, 2) and u.dtype == torch.float32 and u.device.type == "cpu"
        assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
        assert torch.equal(u, lighting.uniforms(S, kind, g()))
        assert not torch.equal(u, lighting.uniforms(S, kind, torch.Generator().manual_seed(12)))
        if kind == "stratified":
            a, b = lighting._stratum_sides(S)
            assert a * b == S and 2 <= a <= b
            cell = np.floor(u.double().numpy() * [a, b]).astype(int)
            assert np.array_equal(cell[:, 0] * b + cell[:, 1], np.arange(S))  # sample k in stratum k: one per stratum
    assert lighting._stratum_sides(4096) == (64, 64) and lighting._stratum_sides(1024) == (32, 32)
    for S in (2, 3, 7, 4099):
        with pytest.raises(ValueError, match="factorisation"):
            lighting.uniforms(S, "stratified")
    with pytest.raises(ValueError):
        lighting.uniforms(0)
    with pytest.raises(ValueError):
        lighting.uniforms(16, "sobol")


def test_stratified_values_stay_inside_their_stratum_after_rounding():
    # the largest float32 below 1 as the jitter: (k + r) / a rounds onto the next stratum's edge without the correction
    r = np.float32(1.0) - np.float32(2.0 ** -24)
    a = 64
    k = np.arange(a, dtype=np.float64)
    raw = ((k + float(r)) / a).astype(np.float32)
    assert (raw.astype(np.float64) >= (k + 1) / a).any()
    u = lighting.uniforms(4096, "stratified", torch.Generator().manual_seed(3)).double().numpy()
    assert np.array_equal(np.floor(u[:, 0] * 64), np.arange(4096) // 64)


# ------------------------------------------------------------------------------------------ 3. argument errors, no GPU touched
def _cpu_table(B=2, W=8):
    H = W // 2
    return lighting.LightTable(torch.zeros(B, H, W), torch.zeros(B, H, W), torch.zeros(B, H), H, W, "stored", None)


def test_argument_errors_raise_before_any_gpu_call():
    maps = torch.ones(2, 4, 8, 3)
    for bad in (torch.ones(4, 8), torch.ones(2, 4, 8, 4), torch.ones(2, 4, 7, 3), torch.ones(2, 4, 6, 3), torch.ones(2, 33, 3),
                torch.ones(2, 3, 4, 10), torch.ones(0, 4, 8, 3), np.ones((2, 4, 8, 3))):
        with pytest.raises(ValueError):
            lighting.build_light_table(bad, space="stored")
    with pytest.raises(ValueError, match="W <= 4096"):
        lighting.build_light_table(torch.ones(1, 1, 1, 3).expand(1, 2049, 4098, 3), space="stored")
    with pytest.raises(ValueError):
        lighting.build_light_table(torch.ones(2, 32, 3), space="stored", size=(4, 9))
    for mix in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="uniform_mix"):
            lighting.build_light_table(maps, space="stored", uniform_mix=mix)
    with pytest.raises(ValueError, match="space"):
        lighting.build_light_table(maps, space="srgb", minmax=O.MINMAX)
    with pytest.raises(ValueError, match="minmax"):
        lighting.build_light_table(maps)  # "linear" without minmax
    with pytest.raises(ValueError, match="minmax"):
        lighting.build_light_table(maps, minmax=(1.0, 1.0))
    with pytest.raises(ValueError, match="broadcast"):
        lighting.build_light_table(maps, space="stored", mask=torch.ones(2, 4, 7))
    t = _cpu_table()
    u = torch.rand(16, 2)
    for kw in (dict(u=None), dict(u=torch.rand(16, 3)), dict(u=torch.rand(3, 16, 2)), dict(u=torch.rand(16)), dict(u=u, n_samples=8),
               dict(u=u, texel_weight="area"), dict(u=u, texel_weight=torch.ones(31)), dict(u=u, model=object()),
               dict(u=u, model=object(), latents=torch.zeros(2))):
        with pytest.raises(ValueError):
            lighting.sample_lights(t, maps, **kw)
    with pytest.raises(ValueError):
        lighting.sample_lights((t.pmf, t.cond, t.marg), maps, u=u)
    with pytest.raises(ValueError, match="table is of"):
        lighting.sample_lights(_cpu_table(B=3), maps, u=u)
    with pytest.raises(ValueError):
        lighting.sample_lights(t, torch.ones(2, 8, 16, 3), u=u)
    s = lighting.LightSamples(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5, 3), torch.zeros(2, 5), torch.zeros(2, 5, 3),
                              torch.zeros(2, 5, 3))
    for nrm in (torch.zeros(7), torch.zeros(7, 2), torch.zeros(3, 7, 3), torch.zeros(0, 3)):
        with pytest.raises(ValueError, match="normals"):
            lighting.sampled_irradiance(s, nrm)
    with pytest.raises(ValueError):
        lighting.sampled_irradiance((s.dirs, s.colors), torch.zeros(7, 3))
    with pytest.raises(ValueError):
        lighting.shade_sampled(None, torch.zeros(7, 3), torch.zeros(7, 3), [0, 0, 2.0], 500.0, 0.5, 0.5)
    s.colors = torch.zeros(2, 4, 3)
    with pytest.raises(ValueError, match="dirs and colors"):
        lighting.sampled_irradiance(s, torch.zeros(7, 3))


def test_lighting_has_no_cpu_fallback():
    import reni_amd
    assert reni_amd.lighting is lighting
    maps = torch.ones(2, 4, 8, 3)
    with pytest.raises(_lib.RENILibraryError, match="no CPU fallback"):
        lighting.build_light_table(maps, space="stored")
    with pytest.raises(_lib.RENILibraryError, match="no CPU fallback"):
        lighting.build_light_table(maps.reshape(2, 32, 3), minmax=O.MINMAX, mask=torch.ones(4, 1), uniform_mix=0.25)
    with pytest.raises(_lib.RENILibraryError, match="no CPU fallback"):
        lighting.sample_lights(_cpu_table(), maps, n_samples=16, generator=torch.Generator().manual_seed(0))
    s = lighting.LightSamples(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5, 3), torch.zeros(2, 5), torch.zeros(2, 5, 3),
                              torch.zeros(2, 5, 3))
    with pytest.raises(_lib.RENILibraryError, match="no CPU fallback"):
        lighting.sampled_irradiance(s, torch.zeros(7, 3))
    with pytest.raises(_lib.RENILibraryError):
        lighting.shade_sampled(s, torch.zeros(7, 3), torch.zeros(7, 3), [0.0, 0.0, 2.0], 500.0, 0.5, 0.5)


def test_host_tables_are_the_grids():
    for W in (8, 66):
        sa, rc, dt = ops.light_grid(W, "cpu")
        assert sa.dtype == torch.float32 and np.array_equal(sa.double().numpy(), np_omega(W))
        assert rc.dtype == torch.float64 and np.array_equal(rc.numpy(), np_row_cos(W))
        assert torch.equal(dt, get_directions(W)[0])
        assert abs(float(sa.double().sum()) * W - 4 * np.pi) < 1e-5
        # the band of row i is what its two cosines span
        assert np.allclose((2 * np.pi / W) * -np.diff(rc.numpy()), reni_grid_weights(W)[::W], rtol=1e-12)
        assert torch.equal(lighting.texel_weights("sineweight", W, "cpu"), get_sineweight(W)[0, :, 0])
        assert np.array_equal(lighting.texel_weights("solid_angle", W, "cpu").numpy(), reni_grid_weights(W).astype(np.float32))


# ------------------------------------------------------------------------------------------ 4. build: header, unit, C ABI
def test_header_build_and_binding_name_the_unit():
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    for name in ("reni_light_table_workspace_bytes", "reni_light_table_build", "reni_light_sample", "reni_lights_irradiance"):
        assert re.search(r"^(int|size_t) " + name + r"\(", header, re.M) and name in _lib.EXPORTS
    build = open(os.path.join(ROOT, "reni_amd", "csrc", "build.sh")).read()
    assert re.search(r"for tu in [^;]*\blights\b", build) and "_build/lights.o" in build


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 255) & ~255
    st4 = (ctypes.c_int64 * 4)(3 * 4 * 8, 4 * 8, 8, 1)
    neg4 = (ctypes.c_int64 * 4)(3 * 4 * 8, 4 * 8, -8, 1)
    st3 = (ctypes.c_int64 * 3)(0, 8, 1)
    neg3 = (ctypes.c_int64 * 3)(0, -8, 1)
    wsb = lib.reni_light_table_workspace_bytes
    assert wsb(2, 4, 8) >= 2 * 4 * 8 and wsb(3, 256, 512) > wsb(1, 256, 512) > 0
    bad_shapes = ((0, 4, 8), (1 << 16, 4, 8), (1, 4, 7), (1, 3, 8), (1, 0, 0), (1, 1, 1), (1, 4098 // 2, 4098), (1, -4, -8))
    for B, H, W in bad_shapes:
        assert wsb(B, H, W) == 0, (B, H, W)

    def table(B=1, H=4, W=8, img=p, st=st4, mask=None, mst=None, space=0, m0=-1.0, m1=1.0, sa=p, mix=0.0, pmf=p, cond=p, marg=p,
              ws=p, nws=4096):
        return lib.reni_light_table_build(B, H, W, img, st, mask, mst, space, m0, m1, sa, mix, pmf, cond, marg, ws, nws, None)

    def sample(B=1, H=4, W=8, S=16, pmf=p, cond=p, marg=p, img=p, st=st4, space=0, m0=-1.0, m1=1.0, u=p, ub=0, dt=p, sa=p, rc=p,
               tw=None, jitter=0, index=p, dirs=p, pdf=p, rad=p, col=p):
        return lib.reni_light_sample(B, H, W, S, pmf, cond, marg, img, st, space, m0, m1, u, ub, dt, sa, rc, tw, jitter, index, dirs,
                                     pdf, rad, col, None)

    def irr(B=1, P=8, S=16, nrm=p, ns=0, dirs=p, col=p, scale=1.0, out=p):
        return lib.reni_lights_irradiance(B, P, S, nrm, ns, dirs, col, scale, out, None)

    shapes = [dict(B=B, H=H, W=W) for B, H, W in bad_shapes]
    image = [dict(img=None), dict(st=None), dict(st=neg4), dict(space=2), dict(space=3), dict(space=-1), dict(space=1, m0=1.0, m1=1.0)]
    for kw in shapes + image + [dict(sa=None), dict(pmf=None), dict(cond=None), dict(marg=None), dict(mask=p, mst=None),
                                dict(mask=p, mst=neg3), dict(mix=-0.5), dict(mix=1.5), dict(mix=float("nan"))]:
        assert table(**kw) == -1, kw
        assert lib.reni_last_error().startswith(b"light table:"), (kw, lib.reni_last_error())
    assert b"RENI_SPACE_SRGB" in (table(space=2), lib.reni_last_error())[1]
    assert table(mask=p, mst=st3, ws=None) == -2 and b"workspace" in lib.reni_last_error()
    for kw in (dict(ws=None), dict(nws=8), dict(ws=p + 8)):
        assert table(**kw) == -2, kw
    nulls = [{k: None} for k in ("pmf", "cond", "marg", "u", "dt", "sa", "index", "dirs", "pdf", "rad", "col")]
    for kw in shapes + image + nulls + [dict(S=0), dict(S=-1), dict(S=1 << 29), dict(B=1 << 14, S=1 << 15), dict(ub=1), dict(ub=16),
                                        dict(jitter=2), dict(jitter=-1), dict(jitter=1, rc=None)]:
        assert sample(**kw) == -1, kw
        assert lib.reni_last_error().startswith(b"light sample:"), (kw, lib.reni_last_error())
    for kw in (dict(B=0), dict(B=1 << 16), dict(P=0), dict(S=0), dict(P=1 << 29), dict(S=1 << 29), dict(B=1 << 14, P=1 << 15),
               dict(ns=3), dict(ns=25), dict(nrm=None), dict(dirs=None), dict(col=None), dict(out=None)):
        assert irr(**kw) == -1, kw
        assert lib.reni_last_error().startswith(b"lights irradiance:"), (kw, lib.reni_last_error())
