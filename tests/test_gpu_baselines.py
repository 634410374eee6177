"""GPU tests of the spherical-Gaussian and spherical-harmonic baselines (reni_tu_baselines.hip through reni_amd.baselines)
against the goldens made from the reference (tests/golden/make_g22_baselines.py) and float64 restatements."""
import numpy as np
import pytest
import torch

from tests.test_baselines_cpu import G22, G23, SH_LMAX, SH_WIDTHS, np_sg_grid, rel, rel_l2

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda")


def _g22(s):
    g = np.load(G22)
    N, H, W, R, C = (int(x) for x in g[f"s{s}_shape"])
    return g, N, H, W, R, C


def torch_sg_loss(raw, env, sw, R, C, dtype):
    """the reference's closure (reparametrise, renderSG, WeightedMSE) in torch autograd; materialises [N, K, 3, P]"""
    tc, pc, tr, pr, dirs = np_sg_grid(R, C, env.shape[2], env.shape[3])
    d = dict(device=raw.device, dtype=dtype)
    tc, pc, dirs = (torch.as_tensor(x, **d) for x in (tc, pc, dirs))
    N, K = raw.shape[0], R * C
    p = raw.view(N, K, 6).to(dtype)
    th = tr * torch.tanh(p[..., 3]) + tc
    ph = pr * torch.tanh(p[..., 4]) + pc
    axis = torch.stack([torch.sin(th) * torch.cos(ph), torch.sin(th) * torch.sin(ph), torch.cos(th)], -1)
    e = torch.exp(torch.exp(p[..., 5])[..., None] * (axis @ dirs.T - 1))  # [N, K, P]
    rec = (torch.exp(p[..., 0:3])[..., None] * e[:, :, None, :]).sum(1).view(env.shape)
    return ((torch.log(rec + 1) - torch.log(env.to(dtype) + 1)) ** 2 * sw.to(dtype)).view(N, -1).mean(1).sum()


@pytest.mark.parametrize("s", [1, 2])
def test_sg_kernels_match_the_reference(s):
    from reni_amd import baselines, ops
    g, N, H, W, R, C = _g22(s)
    dev = _dev()
    raw = torch.from_numpy(g[f"s{s}_param"]).to(dev)
    rec = baselines.sg_render(raw, R, C, H, W)
    assert rel(rec.cpu().numpy(), g[f"s{s}_render"]) <= 2e-6
    env = torch.from_numpy(g[f"s{s}_env"]).to(dev)
    sw = torch.from_numpy(g[f"s{s}_sineweight"]).to(dev)
    tc, pc, tr, pr = baselines.sg_lobe_centres(R, C, dev)
    total, per, grad = ops.sg_loss_grad(raw.view(N, R * C, 6), tc, pc, tr, pr, torch.log(env + 1), sw)
    assert abs(total.item() - float(g[f"s{s}_loss"])) <= 1e-5 * abs(float(g[f"s{s}_loss"]))
    assert rel(per.cpu().numpy(), g[f"s{s}_loss_per_map"]) <= 1e-5
    assert rel_l2(grad.cpu().numpy().reshape(N, -1), g[f"s{s}_grad"].astype(np.float64)) <= 1e-5
    # the autograd Function hands the same gradient to param.grad
    p = raw.clone().requires_grad_()
    loss = baselines.sg_loss(p, torch.log(env + 1), sw, R, C)
    loss.backward()
    assert torch.equal(loss.detach(), total) and torch.equal(p.grad.view(N, R * C, 6), grad)


def test_sg_gradient_against_float64_autograd():
    from reni_amd import baselines, ops
    dev = _dev()
    gen = torch.Generator().manual_seed(7)
    for N, H, W, R, C, swshape in ((5, 16, 32, 2, 6, (1, 3, 16, 32)), (3, 8, 24, 3, 4, (3, 1, 1, 24)),
                                   (2, 32, 64, 1, 5, (2, 1, 32, 64)), (2, 5, 7, 8, 8, (1, 1, 1, 1))):
        K = R * C
        raw = torch.randn(N, K, 6, generator=gen) * 0.7
        raw[0, 0, 3], raw[-1, K - 1, 4], raw[0, K // 2, 3] = 3.0, -3.5, -2.5  # near tanh saturation
        raw[..., 5] += float(np.log(np.pi / R))
        env = torch.rand(N, 3, H, W, generator=gen) * 4
        sw = torch.rand(*swshape, generator=gen) + 0.1
        raw, env, sw = raw.to(dev), env.to(dev), sw.to(dev)
        r64 = raw.double().requires_grad_()
        ref = torch_sg_loss(r64, env, sw, R, C, torch.float64)
        ref.backward()
        tc, pc, tr, pr = baselines.sg_lobe_centres(R, C, dev)
        total, _, grad = ops.sg_loss_grad(raw, tc, pc, tr, pr, torch.log(env + 1), sw)
        assert abs(total.item() - ref.item()) <= 1e-5 * abs(ref.item()), (N, H, W, R, C)
        assert rel_l2(grad.double().cpu().numpy(), r64.grad.cpu().numpy()) <= 1e-5, (N, H, W, R, C)


def test_sg_loss_grad_is_deterministic_and_batch_independent():
    from reni_amd import baselines, ops
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    for H, W in ((16, 32), (32, 64)):  # LDS path and workspace path
        N, R, C = 64, 2, 6
        raw = (torch.randn(N, R * C, 6, generator=gen) * 0.5).to(dev)
        lt = torch.log(torch.rand(N, 3, H, W, generator=gen) * 3 + 1).to(dev)
        sw = torch.rand(1, 1, H, W, generator=gen).to(dev)
        tc, pc, tr, pr = baselines.sg_lobe_centres(R, C, dev)
        a = ops.sg_loss_grad(raw, tc, pc, tr, pr, lt, sw)
        b = ops.sg_loss_grad(raw, tc, pc, tr, pr, lt, sw)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        for n in (0, 37, 63):
            one = ops.sg_loss_grad(raw[n:n + 1].contiguous(), tc, pc, tr, pr, lt[n:n + 1].contiguous(), sw)
            assert torch.equal(one[1][0], a[1][n]) and torch.equal(one[2][0], a[2][n])


def _psnr(x, ref):
    return 10 * np.log10(float(np.abs(ref).max()) ** 2 / float(((x.astype(np.float64) - ref) ** 2).mean()))


@pytest.mark.parametrize("s", [1, 2])
def test_sg_env_optim_matches_the_reference(s):
    from reni_amd import baselines
    g, N, H, W, R, C = _g22(s)
    K = R * C
    env, sw = torch.from_numpy(g[f"s{s}_env"]), torch.from_numpy(g[f"s{s}_sineweight"])
    m = baselines.SGEnvOptim(niter=2, envNum=N, envWidth=W, envHeight=H, SGRow=R, SGCol=C)
    th, ph, la, we, im = m.optimize(env.to(_dev()), sw.to(_dev()))
    for x, name, shape in ((th, "theta", (N, K, 1)), (ph, "phi", (N, K, 1)), (la, "lamb", (N, K, 1)),
                           (we, "weight", (N, K, 3)), (im, "rec", (N, 3, H, W))):
        ref = g[f"s{s}_opt_{name}"]
        assert isinstance(x, np.ndarray) and x.dtype == ref.dtype == np.float32 and x.shape == ref.shape == shape
    ref_loss = float(g[f"s{s}_opt_losses"][-1])
    assert abs(m.loss.item() - ref_loss) <= 0.01 * ref_loss
    assert _psnr(im, g[f"s{s}_opt_rec"].astype(np.float64)) >= 40.0


def test_lbfgs_kernel_closure_agrees_with_torch_autograd():
    """the same LBFGS driven by the kernel's closure and by an fp32 torch-autograd closure: first 5 closure evaluations"""
    from reni_amd import baselines
    g, N, H, W, R, C = _g22(1)
    dev = _dev()
    env, sw = torch.from_numpy(g["s1_env"]).to(dev), torch.from_numpy(g["s1_sineweight"]).to(dev)
    runs = []
    for use_kernel in (True, False):
        m = baselines.SGEnvOptim(niter=1, envNum=N, envWidth=W, envHeight=H, SGRow=R, SGCol=C)
        p = m.param
        opt = torch.optim.LBFGS([p], lr=0.2, max_iter=6)
        losses = []

        def closure():
            opt.zero_grad()
            if use_kernel:
                loss = baselines.sg_loss(p, torch.log(env + 1), sw, R, C)
            else:
                loss = torch_sg_loss(p, env, sw, R, C, torch.float32)
            loss.backward()
            losses.append(loss.item())
            return loss

        opt.step(closure)
        runs.append(losses)
    assert len(runs[0]) >= 5 and len(runs[1]) >= 5
    assert np.allclose(runs[0][:5], runs[1][:5], rtol=1e-4, atol=0), runs


def test_sg_env_optim_default_shape_stays_small():
    from reni_amd import baselines
    dev = _dev()
    N, H, W = 19200, 16, 32
    gen = torch.Generator().manual_seed(3)
    env = (torch.rand(N, 3, 1, 1, generator=gen) + 0.2 * torch.rand(N, 3, H, W, generator=gen)).to(dev)
    El = (torch.arange(H, dtype=torch.float64) + 0.5) / H * np.pi / 2
    sw = torch.sin(El.float()).view(1, 1, H, 1).expand(1, 1, H, W).contiguous().to(dev)
    m = baselines.SGEnvOptim(niter=1)
    first = baselines.sg_loss(m.param, torch.log(env + 1), sw, 2, 6).item()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = m.optimize(env, sw)
    torch.cuda.synchronize()
    # torch's LBFGS keeps up to history_size = 100 pairs of flat [N * K * 6] vectors (~1.1 GB here): its own state, which the
    # reference's optimizer holds too, is not counted; everything else (targets, kernel outputs, workspace) must stay < 1 GB
    st = m.optEnv.state[m.optEnv._params[0]]
    lbfgs = sum(t.numel() * t.element_size() for t in st.get("old_dirs", []) + st.get("old_stps", []))
    lbfgs += sum(v.numel() * v.element_size() for v in st.values() if torch.is_tensor(v) and v.is_cuda)
    assert torch.cuda.max_memory_allocated() - before - lbfgs < (1 << 30)
    # one closure alone (loss, backward) stays far below a single materialised [N, K, 3, H, W] tensor (1.4 GB)
    p = m.param.detach().clone().requires_grad_()
    lt = torch.log(env + 1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    baselines.sg_loss(p, lt, sw, 2, 6).backward()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < (64 << 20)
    assert out[4].shape == (N, 3, H, W) and m.iterCount >= 1
    assert m.loss.item() < first


@pytest.mark.parametrize("W", SH_WIDTHS)
def test_sh_kernels_match_the_reference(W):
    from reni_amd import baselines
    g = np.load(G23)
    dev = _dev()
    imgs = torch.from_numpy(g[f"w{W}_imgs"]).to(dev)
    for lmax in SH_LMAX:
        ref_c, ref_r = g[f"w{W}_l{lmax}_coeffs"], g[f"w{W}_l{lmax}_rec"]
        c = baselines.sh_project(imgs, lmax)
        assert torch.equal(c, baselines.sh_project(imgs, lmax))
        cn = c.cpu().numpy()
        for i in range(len(ref_c)):
            assert np.abs(cn[i] - ref_c[i]).max() <= 1e-5 * np.linalg.norm(ref_c[i]), (W, lmax, i)
        r = baselines.sh_reconstruct(torch.from_numpy(ref_c).float().to(dev), W)
        assert torch.equal(r, baselines.sh_reconstruct(torch.from_numpy(ref_c).float().to(dev), W))
        assert rel(r.cpu().numpy(), ref_r.astype(np.float64)) <= 1e-5, (W, lmax)
        # the reference-named wrappers
        c1 = baselines.getCoefficientsFromImage(g[f"w{W}_imgs"][1], lmax)
        assert c1.dtype == np.float64 and c1.shape == ref_c[1].shape
        assert np.abs(c1 - ref_c[1]).max() <= 1e-5 * np.linalg.norm(ref_c[1])
        r1 = baselines.shReconstructSignal(ref_c[1], width=W)
        assert r1.dtype == np.float32 and r1.shape == (W // 2, W, 3)
        assert rel(r1, ref_r[1].astype(np.float64)) <= 1e-5
    rep = baselines.get_spherical_harmonic_representation(g["w32_imgs"][1], 3)
    assert isinstance(rep, torch.Tensor) and rep.dtype == torch.float32
    assert rel(rep.numpy(), g["rep_w32_nb3"].astype(np.float64)) <= 1e-5


def test_sh_batch_is_per_map_and_large_batches_work():
    from reni_amd import baselines
    dev = _dev()
    gen = torch.Generator().manual_seed(9)
    imgs = torch.rand(70, 16, 32, 3, generator=gen).to(dev)
    c = baselines.sh_project(imgs, 9)
    for n in (0, 33, 69):
        assert torch.equal(baselines.sh_project(imgs[n:n + 1], 9)[0], c[n])
    r = baselines.sh_reconstruct(c, 32)
    for n in (0, 69):
        assert torch.equal(baselines.sh_reconstruct(c[n:n + 1], 32)[0], r[n])
