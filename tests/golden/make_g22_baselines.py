"""G22 / G23: the spherical-Gaussian and spherical-harmonic environment-map baselines, by IMPORTING the reference.

Run in the build container only (imports the reference from /root/reference, like make_golden.py):

    python tests/golden/make_g22_baselines.py

G22 (src/models/spherical_gaussians.py, SGEnvOptim on the CPU, fp32 torch) for two shapes:
  shape 1: N = 3, 16 x 32, 2 x 6 lobes, sineweight [1, 1, H, W]
  shape 2: N = 2, 32 x 64, 1 x 5 lobes, sineweight [N, 1, H, W]
  stored: the env maps, the sineweight, one random raw-parameter point with the render, the loss and the autograd gradient
  there, and optimize(niter = 2)'s outputs with the loss after each outer iteration.
G23 (src/models/spherical_harmonics.py, float64 numpy): random and structured maps at W in {16, 32, 64}, projected with
  getCoefficientsFromImage at lmax in {0, 2, 5, 9, 15} and reconstructed with shReconstructSignal.
Outputs: tests/golden/g22_sg.npz, tests/golden/g23_sh.npz (plain arrays, well under 1 MB each)."""
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (stubs gdown / torchvision, puts the reference on sys.path)

# spherical_harmonics.py imports cv2, imageio, scipy.ndimage and matplotlib at module top; none of the functions used
# here needs them.  Stub whichever is absent.
for name in ("cv2", "imageio", "scipy", "scipy.ndimage", "matplotlib", "matplotlib.pyplot", "matplotlib.colors"):
    try:
        __import__(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
sys.modules["matplotlib.colors"].__dict__.setdefault("LinearSegmentedColormap", object)
sys.modules["cv2"].__dict__.setdefault("INTER_CUBIC", 2)  # a default argument value at module level
sys.modules["scipy"].__dict__.setdefault("ndimage", sys.modules["scipy.ndimage"])
sys.modules["matplotlib"].__dict__.setdefault("pyplot", sys.modules["matplotlib.pyplot"])

# spherical_gaussians.py imports `utils.loss_functions` (no `src.` prefix): seed it with the real module
from src.utils import loss_functions as ref_loss  # noqa: E402

sys.modules.setdefault("utils", types.ModuleType("utils"))
sys.modules["utils.loss_functions"] = ref_loss
sys.modules["utils"].loss_functions = ref_loss

from src.models import spherical_gaussians as ref_sg  # noqa: E402
from src.models import spherical_harmonics as ref_sh  # noqa: E402

SG_SHAPES = ((3, 16, 32, 2, 6, "one"), (2, 32, 64, 1, 5, "batch"))
SH_WIDTHS = (16, 32, 64)
SH_LMAX = (0, 2, 5, 9, 15)


def reparam(m):
    theta, phi, weight, lamb = m.deparameterize()
    theta = m.thetaRange * torch.tanh(theta) + m.thetaCenter
    phi = m.phiRange * torch.tanh(phi) + m.phiCenter
    return theta, phi, torch.exp(weight), torch.exp(lamb)


def g22():
    out = {}
    for s, (N, H, W, R, C, sw_kind) in enumerate(SG_SHAPES, 1):
        g = torch.Generator().manual_seed(220 + s)
        K = R * C
        # HDR-like maps: a smooth sky term plus a bright lobe plus per-pixel noise, all positive
        yy = torch.linspace(0, 1, H).view(1, 1, H, 1)
        xx = torch.linspace(0, 1, W).view(1, 1, 1, W)
        env = (0.3 + 0.7 * torch.rand(N, 3, 1, 1, generator=g)) * (1.5 - yy) \
            + 4.0 * torch.rand(N, 3, 1, 1, generator=g) * torch.exp(-((xx - torch.rand(N, 1, 1, 1, generator=g)) ** 2
                                                                       + (yy - 0.3) ** 2) / 0.02) \
            + 0.2 * torch.rand(N, 3, H, W, generator=g)
        env = env.float().contiguous()
        El = ((np.arange(H) + 0.5) / H) * np.pi / 2.0
        sw1 = np.repeat(np.sin(El.astype(np.float32))[:, None], W, axis=1)[None, None]  # [1,1,H,W] like SGEnvOptim.W
        if sw_kind == "one":
            sw = torch.from_numpy(np.ascontiguousarray(sw1))
        else:
            sw = torch.from_numpy(np.ascontiguousarray(sw1)).repeat(N, 1, 1, 1) \
                * (0.5 + torch.rand(N, 1, 1, 1, generator=g))
        sw = sw.float().contiguous()

        m = ref_sg.SGEnvOptim(isCuda=False, niter=2, envNum=N, envWidth=W, envHeight=H, SGRow=R, SGCol=C)
        # one random raw-parameter point: render, loss, autograd gradient
        p = torch.randn(N, K, 6, generator=g) * 0.6
        p[:, :, 5] += float(np.log(np.pi / R))
        p = p.reshape(N, K * 6).float()
        m.param.data.copy_(p)
        m.param.grad = None
        theta, phi, weight, lamb = reparam(m)
        rec = m.renderSG(theta, phi, lamb, weight)
        per_map = (((torch.log(rec + 1) - torch.log(env + 1)) ** 2) * sw).view(N, -1).mean(1)
        loss = ref_loss.WeightedMSE(torch.log(rec + 1), torch.log(env + 1), sw)
        loss.backward()
        pre = f"s{s}_"
        out.update({pre + "shape": np.array([N, H, W, R, C]), pre + "env": env.numpy(), pre + "sineweight": sw.numpy(),
                    pre + "param": p.numpy(), pre + "render": rec.detach().numpy(), pre + "loss": np.float32(loss.item()),
                    pre + "loss_per_map": per_map.detach().numpy(), pre + "grad": m.param.grad.numpy().copy()})

        # optimize(niter = 2) from the constructor's initial point, recording the loss after each outer iteration
        m = ref_sg.SGEnvOptim(isCuda=False, niter=2, envNum=N, envWidth=W, envHeight=H, SGRow=R, SGCol=C)
        losses = []
        step = m.optEnv.step

        def rec_step(closure, _step=step, _m=m):
            r = _step(closure)
            losses.append(float(_m.loss.item()))
            return r

        m.optEnv.step = rec_step
        th, ph, la, we, im = m.optimize(env.clone(), sw)
        out.update({pre + "opt_theta": th, pre + "opt_phi": ph, pre + "opt_lamb": la, pre + "opt_weight": we,
                    pre + "opt_rec": im, pre + "opt_losses": np.array(losses, np.float64),
                    pre + "opt_evals": np.int64(m.iterCount)})
        print(f"G22 shape {s}: loss {loss.item():.6g}, optimize losses {losses}, closures {m.iterCount}")
    np.savez_compressed(os.path.join(HERE, "g22_sg.npz"), **out)


def g23():
    out = {}
    rng = np.random.default_rng(23)
    for W in SH_WIDTHS:
        H = W // 2
        th = (np.arange(H) + 0.5)[:, None] / H * np.pi
        ph = (np.arange(W) + 0.5)[None, :] / W * 2 * np.pi
        structured = np.stack([1.0 + np.cos(th) + 0 * ph, 0.5 + 0.4 * np.sin(2 * ph) * np.sin(th),
                               np.exp(-((th - 0.8) ** 2 + (ph - 2.0) ** 2) / 0.1) * 5.0], axis=-1)
        imgs = np.stack([rng.random((H, W, 3)) * 2.0, structured]).astype(np.float32)
        out[f"w{W}_imgs"] = imgs
        for lmax in SH_LMAX:
            co = np.stack([ref_sh.getCoefficientsFromImage(im, lmax) for im in imgs])
            rec = np.stack([ref_sh.shReconstructSignal(c, width=W) for c in co])
            assert co.dtype == np.float64 and rec.dtype == np.float32
            out[f"w{W}_l{lmax}_coeffs"] = co
            out[f"w{W}_l{lmax}_rec"] = rec
    # get_spherical_harmonic_representation passes nBands as lmax and returns a torch tensor
    r = ref_sh.get_spherical_harmonic_representation(out["w32_imgs"][1], 3)
    assert isinstance(r, torch.Tensor)
    out["rep_w32_nb3"] = r.numpy()
    out["num_coeffs"] = np.array([ref_sh.calc_num_sh_coeffs(o) for o in range(8)])
    out["sh_order"] = np.array([ref_sh.get_sh_order(d) for d in range(1, 40)])
    np.savez_compressed(os.path.join(HERE, "g23_sh.npz"), **out)
    print("G23:", len(out), "arrays")


if __name__ == "__main__":
    torch.set_num_threads(4)
    g22()
    g23()
