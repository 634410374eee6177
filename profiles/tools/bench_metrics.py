"""Time metrics.score_maps (fused: reni_pair_stats / reni_ssim) against the torch composition a user would have written
before it existed, in one process on one GPU.  Usage: python profiles/tools/bench_metrics.py [--iters N] [--warmup N]

Both paths score the same pair (a model-output prediction [B, P, 3] against a dataset batch [B, 3, H, W]) with minmax and an
inpainting mask: stored-space weighted MSE and cosine, linear and sRGB PSNR, sRGB SSIM, each over the whole map, the seen and
the hidden pixels.  The composition: ops.unnormalise_srgb for both images (linear + sRGB for the target, linear for the
prediction, whose sRGB view under the target's exposure is torch), torch reductions, and an SSIM from two separable
F.conv2d passes over a column-circular, row-replicated padding.  The two are alternated inside the timed loop, each call
between device events; medians are reported, and beside them the wall time per call of back-to-back calls, where a host
read-back inside a path would show.  The launch counts are the library's (reni_launch_count): the composition's torch
kernels are not in them.  Prints one JSON line per size and the achieved bytes/s of reni_pair_stats.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from reni_amd import metrics, ops  # noqa: E402
from reni_amd.data import MINMAX  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth


def composition(pred, target, minmax, mask_hw, sin_h1, window):
    """the scores of metrics.score_maps from existing ops and torch"""
    B, _, H, W = target.shape
    p4 = pred.view(B, H, W, 3).permute(0, 3, 1, 2)
    lin_p = ops.unnormalise_srgb(p4, minmax, srgb=False)
    srgb_t, lin_t = ops.unnormalise_srgb(target, minmax, srgb=True, want_linear=True)
    q = torch.quantile(torch.quantile(torch.quantile(lin_t, 0.98, dim=1), 0.98, dim=1), 0.98, dim=1)
    y = torch.clamp(lin_p / q.view(B, 1, 1, 1), 0.0, 1.0)
    srgb_p = torch.where(y <= 0.0031308, 12.92 * y, 1.055 * torch.pow(y, 1 / 2.4) - 0.055)
    # SSIM map: five moments through two separable passes
    x = torch.stack((srgb_p, srgb_t, srgb_p * srgb_p, srgb_t * srgb_t, srgb_p * srgb_t), 1).reshape(B * 15, 1, H, W)
    x = F.pad(F.pad(x, (5, 5, 0, 0), mode="circular"), (0, 0, 5, 5), mode="replicate")
    x = F.conv2d(F.conv2d(x, window.view(1, 1, 1, 11)), window.view(1, 1, 11, 1)).reshape(B, 5, 3, H, W)
    mp, mt, epp, ett, ept = x.unbind(1)
    vp, vt, cov = epp - mp * mp, ett - mt * mt, ept - mp * mt
    smap = (((2 * mp * mt + 1e-4) * (2 * cov + 9e-4)) / ((mp * mp + mt * mt + 1e-4) * (vp + vt + 9e-4))).mean(1)
    peak = lin_t.amax((1, 2, 3))
    out = {}
    for suffix, w in (("", sin_h1.expand(H, W)), ("_seen", mask_hw * sin_h1), ("_hidden", (1 - mask_hw) * sin_h1)):
        sw = w.sum()
        out["wmse_stored" + suffix] = (w * ((p4 - target) ** 2).sum(1)).sum((1, 2)) / (3 * sw)
        out["cosine_stored" + suffix] = (w * F.cosine_similarity(p4, target, dim=1, eps=1e-20)).sum((1, 2)) / sw
        mse_l = (w * ((lin_p - lin_t) ** 2).sum(1)).sum((1, 2)) / (3 * sw)
        out["psnr_linear" + suffix] = 10 * torch.log10(peak * peak / mse_l)
        mse_s = (w * ((srgb_p - srgb_t) ** 2).sum(1)).sum((1, 2)) / (3 * sw)
        out["psnr_srgb" + suffix] = 10 * torch.log10(1.0 / mse_s)
        out["ssim_srgb" + suffix] = (w * smap).sum((1, 2)) / sw
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def host_timed(fn, n):
    """wall time per call of n back-to-back calls behind one synchronise: what a host read-back inside fn costs shows here, not
    between device events"""
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    window = torch.from_numpy(metrics.gaussian_window().astype(np.float32)).to(dev)
    for B, H, W in ((64, 128, 256), (16, 512, 1024)):
        g = torch.Generator(device=dev).manual_seed(B + H)
        target = (torch.randn(B, 3, H, W, device=dev, generator=g) * 0.12 - 0.05).clamp(-1, 1)
        pred = (target + 0.03 * torch.randn(B, 3, H, W, device=dev, generator=g)).permute(0, 2, 3, 1).reshape(B, H * W, 3).contiguous()
        mask_hw = torch.ones(H, W, device=dev)
        mask_hw[:, W // 4:W // 2] = 0.0
        sin_h1 = metrics.solid_angle_weight(H, dev)
        fused = lambda: metrics.score_maps(pred, target, MINMAX, mask_hw, size=(H, W))  # noqa: E731
        comp = lambda: composition(pred, target, MINMAX, mask_hw, sin_h1, window)  # noqa: E731
        for _ in range(args.warmup):
            fused(), comp()
        torch.cuda.synchronize()
        ops.launch_count(reset=True)
        fused()
        launches_fused = ops.launch_count(reset=True)
        comp()
        launches_comp_lib = ops.launch_count(reset=True)
        tf, tc = [], []
        for _ in range(args.iters):
            tf.append(timed(fused)[0])
            tc.append(timed(comp)[0])
        wall_f, wall_c = host_timed(fused, args.iters), host_timed(comp, args.iters)
        rf, rc = fused(), comp()
        worst = max(float(((rf[k] - rc[k]).abs() / rc[k].abs().clamp_min(1e-6)).max()) for k in rf if not k.startswith("ssim"))
        # reni_pair_stats alone: bytes the algorithm needs (both images once + the weight row) over its time
        expo = metrics.exposure(target, MINMAX)
        stats = lambda: ops.pair_stats(pred, target, sin_h1, "srgb", MINMAX, expo, size=(H, W))  # noqa: E731
        for _ in range(args.warmup):
            stats()
        ts = [timed(stats)[0] for _ in range(args.iters)]
        nbytes = 2 * B * 3 * H * W * 4
        rec = {"B": B, "H": H, "W": W, "fused_ms_median": float(np.median(tf)), "fused_ms_min": float(np.min(tf)),
               "composition_ms_median": float(np.median(tc)), "composition_ms_min": float(np.min(tc)),
               "speedup_median": float(np.median(tc) / np.median(tf)), "fused_wall_ms_per_call": wall_f,
               "composition_wall_ms_per_call": wall_c, "library_launches_fused": launches_fused,
               "library_launches_composition_without_its_torch_kernels": launches_comp_lib, "largest_relative_difference_non_ssim": worst,
               "ssim_srgb_fused": float(rf["ssim_srgb"].mean()), "ssim_srgb_composition": float(rc["ssim_srgb"].mean()),
               "pair_stats_srgb_ms_median": float(np.median(ts)), "pair_stats_bytes": nbytes,
               "pair_stats_bytes_per_s": nbytes / (float(np.median(ts)) * 1e-3),
               "pair_stats_share_of_hbm_peak": nbytes / (float(np.median(ts)) * 1e-3) / HBM_BYTES_PER_S}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
