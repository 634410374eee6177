"""Time reni_amd.lighting (reni_light_table_build / reni_light_sample / reni_lights_irradiance) against the torch restatement a
user would have written before it existed, in one process on one GPU.
Usage: python profiles/tools/bench_lighting.py [--iters N] [--warmup N]

64 maps of 128 x 256, stored normalised, read in linear space:
    table       lighting.build_light_table          against  exp + luminance + two cumsums + normalisation in torch
    sample      lighting.sample_lights, S = 1024 and 4096  against  two torch.searchsorted + gathers
    irradiance  lighting.sampled_irradiance at P = 2048 normals (the 32 x 64 grid), S = 1024 and 4096, against
                baselines.irradiance_map of the whole maps at the same output width (all 32 768 texels per normal), and against
                the torch bmm that materialises [B, P, S]
The two sides of a pair are alternated inside the timed loop, each call between device events; medians are reported.  The
launch counts are the library's (reni_launch_count): torch's own kernels are not in them.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from reni_amd import baselines, lighting, ops  # noqa: E402
from reni_amd.data import MINMAX  # noqa: E402
from reni_amd.utils import get_directions  # noqa: E402


def torch_table(x, minmax, omega):
    """pmf, cond, marg of maps x [B, H, W, 3] (stored normalised), float32 throughout"""
    rad = torch.exp(0.5 * (x + 1) * (minmax[1] - minmax[0]) + minmax[0])
    f = (0.2126 * rad[..., 0] + 0.7152 * rad[..., 1] + 0.0722 * rad[..., 2]).clamp_min(0) * omega[None, :, None]
    pmf = f / f.sum((1, 2), keepdim=True)
    cs = pmf.cumsum(2)
    rows = cs[:, :, -1]
    cm = rows.cumsum(1)
    return pmf, cs / rows[:, :, None], cm / cm[:, -1:]


def torch_sample(pmf, cond, marg, x, minmax, u, dirs, omega, tw):
    B, H, W = pmf.shape
    S = u.shape[0]
    i = torch.searchsorted(marg, u[None, :, 0].expand(B, S).contiguous(), right=True).clamp_max(H - 1)
    rows = cond.gather(1, i[:, :, None].expand(B, S, W))
    j = torch.searchsorted(rows, u[None, :, 1, None].expand(B, S, 1).contiguous(), right=True)[..., 0].clamp_max(W - 1)
    idx = i * W + j
    pm = pmf.reshape(B, -1).gather(1, idx)
    rad = torch.exp(0.5 * (x.reshape(B, -1, 3).gather(1, idx[..., None].expand(B, S, 3)) + 1) * (minmax[1] - minmax[0]) + minmax[0])
    return idx, dirs[idx], pm / omega[i], rad, rad * (tw[idx] / (S * pm))[..., None]


def torch_irradiance(normals, dirs, colors):
    return torch.bmm(torch.clamp(normals[None].expand(dirs.shape[0], -1, 3) @ dirs.transpose(1, 2), min=0), colors) / np.pi


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def pair(ours, theirs, iters, warmup):
    """medians [ms] of the two alternated, and the library launches of one call of each"""
    for _ in range(warmup):
        ours(), theirs()
    torch.cuda.synchronize()
    ops.launch_count(reset=True)
    ours()
    n_ours = ops.launch_count(reset=True)
    theirs()
    n_theirs = ops.launch_count(reset=True)
    to, tt = [], []
    for _ in range(iters):
        to.append(timed(ours)[0])
        tt.append(timed(theirs)[0])
    return {"ms_median": float(np.median(to)), "ms_min": float(np.min(to)), "other_ms_median": float(np.median(tt)),
            "other_ms_min": float(np.min(tt)), "library_launches": n_ours, "other_library_launches": n_theirs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lighting needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    B, H, W, P_W = 64, 128, 256, 64
    g = torch.Generator(device=dev).manual_seed(B + H)
    x = (torch.randn(B, H, W, 3, device=dev, generator=g) * 0.12 - 0.05).clamp(-1, 1)
    x[:, 40, 100:103] = 0.9  # a sun
    omega, _, dirs = ops.light_grid(W, dev)
    tw = lighting.texel_weights("solid_angle", W, dev)
    normals = get_directions(P_W)[0].to(dev)
    rec = {"B": B, "H": H, "W": W, "P": int(normals.shape[0])}
    rec["table"] = pair(lambda: lighting.build_light_table(x, minmax=MINMAX), lambda: torch_table(x, MINMAX, omega), args.iters, args.warmup)
    table = lighting.build_light_table(x, minmax=MINMAX)
    tt = torch_table(x, MINMAX, omega)
    rec["table"]["largest_cdf_difference"] = max(float((table.cond - tt[1]).abs().max()), float((table.marg - tt[2]).abs().max()))
    lin = ops.unnormalise_srgb(x.permute(0, 3, 1, 2), MINMAX, srgb=False).permute(0, 2, 3, 1).reshape(B, H * W, 3).contiguous()
    full = baselines.irradiance_map(lin, out_width=P_W)
    for S in (1024, 4096):
        u = lighting.uniforms(S, "stratified", torch.Generator().manual_seed(S), dev)
        r = pair(lambda: lighting.sample_lights(table, x, u=u),
                 lambda: torch_sample(table.pmf, table.cond, table.marg, x, MINMAX, u, dirs, omega, tw), args.iters, args.warmup)
        s = lighting.sample_lights(table, x, u=u)
        r["index_agreement"] = float((s.index.long() == torch_sample(table.pmf, table.cond, table.marg, x, MINMAX, u, dirs, omega, tw)[0]).float().mean())
        rec[f"sample_S{S}"] = r
        r = pair(lambda: lighting.sampled_irradiance(s, normals), lambda: baselines.irradiance_map(lin, out_width=P_W), args.iters, args.warmup)
        r["other"] = "baselines.irradiance_map (every texel)"
        E = lighting.sampled_irradiance(s, normals)
        r["largest_error_of_the_estimate_relative_to_the_largest_irradiance"] = float(((E - full).abs().amax((1, 2)) / full.amax((1, 2))).max())
        rec[f"irradiance_S{S}"] = r
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        r = pair(lambda: lighting.sampled_irradiance(s, normals), lambda: torch_irradiance(normals, s.dirs, s.colors), args.iters, args.warmup)
        r["other"] = "torch bmm over a [B, P, S] tensor"
        r["peak_bytes_of_both"] = int(torch.cuda.max_memory_allocated() - before)
        r["largest_difference_relative_to_the_largest_irradiance"] = float((E - torch_irradiance(normals, s.dirs, s.colors)).abs().max() / E.max())
        rec[f"irradiance_vs_bmm_S{S}"] = r
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
