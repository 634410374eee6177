"""Diffuse irradiance timings: 50 calls timed with CUDA events after warm-up, one JSON line per shape.

  (a) one 600-wide map to 32 x 16 (getDiffuseMap's default grid, reni_diffuse_convolve)
  (b) 64 maps of 64 x 128 to 64 x 128 (irradiance_map)
  (c) one 128 x 256 map to 128 x 256 (irradiance_map)
  sh_irradiance of 64 maps at lmax 2 (the L2 closed form) and lmax 9 (shRender) at 64 x 128

FLOP counts the GEMM only (2 P Q 3 N); the fraction is against the 157 TF fp32 matrix peak."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reni_amd import baselines  # noqa: E402

PEAK = 157.3e12


def timed(fn, warmup=10, iters=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # us per call


def main():
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    img = (torch.rand(300, 600, 3, generator=g) + 0.1).to(dev)
    d, sa, od = (torch.from_numpy(x).float().to(dev) for x in baselines.diffuse_map_tables(600, 32))
    src = img.reshape(1, -1, 3)
    rows = [("a: 1 x 600w -> 32x16", lambda: baselines.diffuse_convolve(src, d, sa, od), 512, 180000, 1)]
    envs = (torch.rand(64, 64 * 128, 3, generator=g) * 2).to(dev)
    rows.append(("b: 64 x 64x128 -> 64x128", lambda: baselines.irradiance_map(envs), 8192, 8192, 64))
    one = (torch.rand(1, 128 * 256, 3, generator=g) * 2).to(dev)
    rows.append(("c: 1 x 128x256 -> 128x256", lambda: baselines.irradiance_map(one), 32768, 32768, 1))
    for name, fn, P, Q, N in rows:
        us = timed(fn)
        flop = 2.0 * P * Q * 3 * N
        print(json.dumps({"shape": name, "us": round(us, 2), "gflop": round(flop / 1e9, 3),
                          "tflops": round(flop / us / 1e6, 2), "frac_of_157tf": round(flop / us / 1e6 / (PEAK / 1e12), 4)}))
    for lmax in (2, 9):
        c = torch.randn(64, (lmax + 1) ** 2, 3, generator=g).to(dev)
        us = timed(lambda: baselines.sh_irradiance(c, 128))
        print(json.dumps({"shape": f"sh_irradiance lmax {lmax}: 64 x -> 64x128", "us": round(us, 2)}))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
