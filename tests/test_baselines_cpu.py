"""CPU tests of the spherical-Gaussian and spherical-harmonic baselines (reni_amd.baselines, reni_tu_baselines.hip).

Holds the float64 numpy restatement of the reference's conventions (SGEnvOptim's lobe grid, hemisphere pixel grid,
reparametrisation, render, WeightedMSE and its gradient; the SH basis, solid angle, projection and reconstruction) that
tests/test_gpu_baselines.py compares the HIP kernels against, and checks it against the goldens made from the reference
(tests/golden/make_g22_baselines.py)."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import isa_audit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G22 = os.path.join(ROOT, "tests", "golden", "g22_sg.npz")
G23 = os.path.join(ROOT, "tests", "golden", "g23_sh.npz")
SH_WIDTHS = (16, 32, 64)
SH_LMAX = (0, 2, 5, 9, 15)


# ------------------------------------------------------------------------------------------ numpy restatement: SG
def np_sg_grid(R, C, H, W):
    """(theta_c [K], phi_c [K] as float32 of float64, theta_range, phi_range, dirs [H*W, 3] as float32 of float64)"""
    phi = ((np.arange(C) + 0.5) / C - 0.5) * np.pi * 2
    theta = (np.arange(R) + 0.5) / R * np.pi / 2.0
    phi, theta = np.meshgrid(phi, theta)
    az = ((np.arange(W) + 0.5) / W - 0.5) * 2 * np.pi
    el = ((np.arange(H) + 0.5) / H) * np.pi / 2.0
    az, el = np.meshgrid(az, el)
    dirs = np.stack([np.sin(el) * np.cos(az), np.sin(el) * np.sin(az), np.cos(el)], -1).reshape(-1, 3)
    return (theta.reshape(-1).astype(np.float32).astype(np.float64), phi.reshape(-1).astype(np.float32).astype(np.float64),
            (np.pi / 2 / R) * 1.5, (2 * np.pi / C) * 1.5, dirs.astype(np.float32).astype(np.float64))


def np_sg_lobes(raw, R, C):
    """raw [N, K, 6] -> (tanh theta~, tanh phi~, theta, phi, w [N,K,3], lambda [N,K], axis [N,K,3])"""
    tc, pc, tr, pr, _ = np_sg_grid(R, C, 1, 1)
    raw = np.asarray(raw, np.float64)
    tt, tp = np.tanh(raw[..., 3]), np.tanh(raw[..., 4])
    th, ph = tr * tt + tc, pr * tp + pc
    axis = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1)
    return tt, tp, th, ph, np.exp(raw[..., 0:3]), np.exp(raw[..., 5]), axis


def np_sg_render(raw, R, C, H, W):
    """rec [N, 3, H, W] = sum_k w_kc exp(lambda_k (a_k . l_p - 1))"""
    *_, dirs = np_sg_grid(R, C, H, W)
    _, _, _, _, w, lam, axis = np_sg_lobes(raw, R, C)
    e = np.exp(lam[:, :, None] * (np.einsum("nkd,pd->nkp", axis, dirs) - 1.0))  # [N, K, P]
    return np.einsum("nkc,nkp->ncp", w, e).reshape(len(raw), 3, H, W)


def np_sg_loss_grad(raw, env, sw, R, C):
    """(total, per-map [N], d total / d raw [N, K, 6]) of WeightedMSE(log(rec + 1), log(env + 1), sw)"""
    raw = np.asarray(raw, np.float64)
    N, K = raw.shape[:2]
    H, W = env.shape[2:]
    P = H * W
    tc, pc, tr, pr, dirs = np_sg_grid(R, C, H, W)
    tt, tp, th, ph, w, lam, axis = np_sg_lobes(raw, R, C)
    dm1 = np.einsum("nkd,pd->nkp", axis, dirs) - 1.0
    e = np.exp(lam[:, :, None] * dm1)
    rec = np.einsum("nkc,nkp->ncp", w, e)
    s = np.broadcast_to(np.asarray(sw, np.float64), env.shape).reshape(N, 3, P)
    d = np.log(rec + 1) - np.log(np.asarray(env, np.float64).reshape(N, 3, P) + 1)
    per = (s * d * d).mean(axis=(1, 2))
    g = 2.0 / (3 * P) * s * d / (rec + 1)  # d loss / d rec
    G = np.einsum("ncp,nkc->nkp", g, w)
    grad = np.zeros((N, K, 6))
    grad[..., 0:3] = w * np.einsum("ncp,nkp->nkc", g, e)
    grad[..., 5] = lam * (G * e * dm1).sum(-1)
    da = lam[:, :, None] * np.einsum("nkp,pd->nkd", G * e, dirs)
    dth = da[..., 0] * np.cos(th) * np.cos(ph) + da[..., 1] * np.cos(th) * np.sin(ph) - da[..., 2] * np.sin(th)
    dph = -da[..., 0] * np.sin(th) * np.sin(ph) + da[..., 1] * np.sin(th) * np.cos(ph)
    grad[..., 3] = dth * tr * (1 - tt * tt)
    grad[..., 4] = dph * pr * (1 - tp * tp)
    return per.sum(), per, grad


# ------------------------------------------------------------------------------------------ numpy restatement: SH
def np_legendre(l, m, x):
    """associated Legendre P_l^m with the Condon-Shortley phase, by the standard three-term recursion"""
    pmm = np.ones_like(x)
    if m > 0:
        s = np.sqrt((1.0 - x) * (1.0 + x))
        for i in range(1, m + 1):
            pmm = pmm * -(2 * i - 1) * s
    if l == m:
        return pmm
    p1 = x * (2 * m + 1) * pmm
    for ll in range(m + 2, l + 1):
        pmm, p1 = p1, ((2 * ll - 1) * x * p1 - (ll + m - 1) * pmm) / (ll - m)
    return p1


def np_sh_basis(W, lmax):
    """Y [H, W, T] of the pixel's top-left corner: theta = y pi / H, phi = x 2 pi / W, t = l^2 + l + m, real SH"""
    H = W // 2
    th = (np.arange(H) / (H / np.pi))[:, None]
    ph = (np.arange(W) / (W / (2 * np.pi)))[None, :]
    Y = np.zeros((H, W, (lmax + 1) ** 2))
    for l in range(lmax + 1):
        for m in range(-l, l + 1):
            am = abs(m)
            k = math.sqrt((2 * l + 1) * math.factorial(l - am) / (4 * math.pi * math.factorial(l + am)))
            p = np_legendre(l, am, np.cos(th))
            trig = 1.0 if m == 0 else math.sqrt(2) * (np.cos(m * ph) if m > 0 else np.sin(am * ph))
            Y[:, :, l * l + l + m] = k * p * trig
    return Y


def np_solid_angle(W):
    """[H]: 2 pi / W (cos(theta - pi / 2H) - cos(theta + pi / 2H)), theta = (1 - (y + 0.5) / H) pi"""
    H = W // 2
    th = (1.0 - (np.arange(H) + 0.5) / H) * np.pi
    return 2 * np.pi / W * (np.cos(th - np.pi / H / 2) - np.cos(th + np.pi / H / 2))


def np_sh_project(img, lmax):
    W = img.shape[1]
    return np.einsum("yxc,yxt,y->tc", np.asarray(img, np.float64), np_sh_basis(W, lmax), np_solid_angle(W))


def np_sh_reconstruct(coeffs, W):
    lmax = int(round(math.sqrt(coeffs.shape[0]))) - 1
    return np.einsum("yxt,tc->yxc", np_sh_basis(W, lmax), np.asarray(coeffs, np.float64))


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------------------------------ restatement vs goldens
@pytest.mark.parametrize("s", [1, 2])
def test_sg_restatement_reproduces_the_reference(s):
    g = np.load(G22)
    N, H, W, R, C = (int(x) for x in g[f"s{s}_shape"])
    raw = g[f"s{s}_param"].reshape(N, R * C, 6)
    assert rel(np_sg_render(raw, R, C, H, W), g[f"s{s}_render"]) < 1e-6
    total, per, grad = np_sg_loss_grad(raw, g[f"s{s}_env"], g[f"s{s}_sineweight"], R, C)
    assert abs(total - float(g[f"s{s}_loss"])) / abs(total) < 1e-6
    assert rel(per, g[f"s{s}_loss_per_map"]) < 1e-6
    assert rel_l2(g[f"s{s}_grad"].reshape(N, R * C, 6), grad) < 1e-6


def test_sg_restatement_gradient_is_the_derivative():
    """central differences of the float64 loss at a random point, including lobes near tanh saturation"""
    rng = np.random.default_rng(5)
    N, H, W, R, C = 2, 6, 10, 2, 3
    raw = rng.normal(0, 0.6, (N, R * C, 6))
    raw[0, 0, 3], raw[1, 2, 4] = 3.5, -4.0
    env = rng.random((N, 3, H, W)) * 3
    sw = rng.random((1, 1, H, W))
    _, _, grad = np_sg_loss_grad(raw, env, sw, R, C)
    num = np.zeros_like(raw)
    for idx in np.ndindex(*raw.shape):
        for sgn in (1, -1):
            r2 = raw.copy()
            r2[idx] += sgn * 1e-6
            num[idx] += sgn * np_sg_loss_grad(r2, env, sw, R, C)[0] / 2e-6
    assert rel_l2(num, grad) < 1e-6


def test_g22_optimize_record_is_complete():
    g = np.load(G22)
    for s in (1, 2):
        N, H, W, R, C = (int(x) for x in g[f"s{s}_shape"])
        K = R * C
        assert g[f"s{s}_opt_theta"].shape == (N, K, 1) and g[f"s{s}_opt_weight"].shape == (N, K, 3)
        assert g[f"s{s}_opt_rec"].shape == (N, 3, H, W) and g[f"s{s}_opt_rec"].dtype == np.float32
        assert len(g[f"s{s}_opt_losses"]) == 2 and g[f"s{s}_opt_losses"][1] <= g[f"s{s}_opt_losses"][0]


@pytest.mark.parametrize("W", SH_WIDTHS)
def test_sh_restatement_reproduces_the_reference(W):
    g = np.load(G23)
    imgs = g[f"w{W}_imgs"]
    for lmax in SH_LMAX:
        ref_c, ref_r = g[f"w{W}_l{lmax}_coeffs"], g[f"w{W}_l{lmax}_rec"]
        for i, img in enumerate(imgs):
            c = np_sh_project(img, lmax)
            assert np.abs(c - ref_c[i]).max() <= 1e-12 * np.linalg.norm(ref_c[i]), (W, lmax, i)
            # the reference's reconstruction is float32 of the float64 result
            r = np_sh_reconstruct(ref_c[i], W)
            assert rel(r.astype(np.float32), ref_r[i]) == 0.0 or rel(r, ref_r[i]) < 1e-7, (W, lmax, i)
            assert rel(r, ref_r[i].astype(np.float64)) < 1e-6


def test_sh_restatement_matches_the_library_tables():
    """reni_amd.baselines.sh_tables (the kernels' float64 tables) are the separable form of the restated basis"""
    from reni_amd import baselines
    for W, lmax in ((16, 2), (32, 9), (64, 15)):
        Y = np_sh_basis(W, lmax)
        row, col = baselines.sh_tables(W, lmax, False)
        assert np.abs(row[:, None, :] * col[None, :, :] - Y).max() <= 1e-12 * np.abs(Y).max()
        row_s, _ = baselines.sh_tables(W, lmax, True)
        assert np.allclose(row_s, row * np_solid_angle(W)[:, None], rtol=1e-14, atol=0)
    sg = baselines.sg_lobe_centres(2, 6)
    tc, pc, tr, pr, _ = np_sg_grid(2, 6, 1, 1)
    assert np.array_equal(sg[0].numpy().astype(np.float64), tc) and np.array_equal(sg[1].numpy().astype(np.float64), pc)
    assert (sg[2], sg[3]) == (tr, pr)


def test_sh_small_helpers_match_the_reference():
    from reni_amd import baselines
    g = np.load(G23)
    assert [baselines.calc_num_sh_coeffs(o) for o in range(8)] == list(g["num_coeffs"])
    assert [baselines.get_sh_order(d) for d in range(1, 40)] == list(g["sh_order"])
    assert baselines.shTerms(15) == 256 and baselines.shIndex(3, -2) == 10
    r = np_sh_reconstruct(np_sh_project(g["w32_imgs"][1], 3), 32)
    assert rel(r, g["rep_w32_nb3"]) < 1e-6


def test_sh_wrappers_refuse_what_needs_cv2_or_scipy():
    from reni_amd import baselines
    img = np.zeros((8, 16, 3), np.float32)
    with pytest.raises(NotImplementedError):
        baselines.getCoefficientsFromImage(img, 2, resizeWidth=8)
    with pytest.raises(NotImplementedError):
        baselines.getCoefficientsFromImage(img, 2, filterAmount=3)
    with pytest.raises(ValueError):
        baselines.getCoefficientsFromImage(np.zeros((501, 1002, 3), np.float32), 2)
    with pytest.raises(NotImplementedError):
        baselines.shReconstructSignal(np.zeros((9, 3)), sh_basis_matrix=np.zeros((8, 16, 9)))


def test_sg_optim_has_no_cpu_fallback():
    from reni_amd import _lib, baselines
    with pytest.raises(_lib.RENILibraryError):
        baselines.SGEnvOptim(isCuda=False, envNum=2)
    with pytest.raises(ValueError):
        baselines.SGEnvOptim(ch=4, envNum=2)


# ------------------------------------------------------------------------------------------ ISA audit, C ABI checks
def test_baselines_translation_unit_isa_audit():
    """reni_tu_baselines.hip with build.sh's flags: no MFMA / transcendental / SDWA hazard, no scratch, MFMAs in the SH
    kernels."""
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "baselines.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_baselines.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    for k in ("k_sg_render", "k_sg_loss_grad", "k_sg_total", "k_sh_project", "k_sh_reconstruct"):
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.valu_to_mfma(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert sizes and all(int(x) == 0 for x in sizes)
    mf = isa_audit.mfma_functions(text)
    assert any("k_sh_project" in f for f in mf) and any("k_sh_reconstruct" in f for f in mf)
    assert not any("k_sg_" in f for f in mf)


def test_c_abi_rejects_bad_shapes_and_null_pointers():
    """Argument checks run before any device work, so they hold without a GPU."""
    from reni_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    sg = lambda N, K, H, W, par=p, wt=p: lib.reni_sg_loss_grad(N, K, H, W, par, p, p, 1.0, 1.0, p, wt, 0, 0, 0, 0,  # noqa: E731
                                                                p, p, p, p, 4096, None)
    for N, K, H, W in ((1, 65, 4, 4), (0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0)):
        assert sg(N, K, H, W) == -1
        assert lib.reni_sg_render(N, K, H, W, p, p, p, 1.0, 1.0, p, None) == -1
        assert lib.reni_sg_workspace_bytes(N, K, H, W) == 0
    assert sg(1, 4, 4, 4, par=None) == -1 and b"NULL" in lib.reni_last_error()
    assert sg(1, 4, 4, 4, wt=None) == -1
    assert lib.reni_sg_loss_grad(1, 4, 4, 4, p, p, p, 1.0, 1.0, p, p, -1, 0, 0, 0, p, p, p, p, 4096, None) == -1
    assert lib.reni_sg_render(1, 4, 4, 4, p, None, p, 1.0, 1.0, p, None) == -1
    assert lib.reni_sg_workspace_bytes(19200, 12, 16, 32) == 0 and lib.reni_sg_workspace_bytes(2, 5, 32, 64) > 0
    assert lib.reni_sg_loss_grad(2, 5, 32, 64, p, p, p, 1.0, 1.0, p, p, 0, 0, 0, 0, p, p, p, None, 0, None) == -2
    for fn in (lib.reni_sh_project, lib.reni_sh_reconstruct):
        for N, H, W, lmax in ((1, 8, 16, 16), (1, 8, 16, -1), (1, 9, 16, 2), (1, 8, 15, 2), (0, 8, 16, 2), (1, 4096, 8192, 2)):
            assert fn(N, H, W, lmax, p, p, p, p, None) == -1, (N, H, W, lmax)
        for k in range(4):
            ptrs = [p] * 4
            ptrs[k] = None
            assert fn(1, 8, 16, 2, *ptrs, None) == -1 and b"NULL" in lib.reni_last_error()
