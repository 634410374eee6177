"""Timings of the normals' gradient of the shader's terms beside the terms forward and backward of the same build.

The workloads of shade_materials_time.py: a 64 x 64 render under a 64 x 128 map with B = 1, and 128 x 128 under 64 x 128 with
B = 3, on the random G-buffer of the shader's tests (20 % background), shininess 500, a shared grid (the BC = 4 instances).
Variants, alternated round by round in one process so that clock and box drift hit all of them alike:

  terms forward          ops.envmap_shade_terms, D and S
  terms forward + T      ... with dS/ds: by instruction count the nearest relative of the new kernel
  terms backward         ops.envmap_shade_terms_backward
  terms dnormals         ops.envmap_shade_terms_dnormals: one launch per image chunk and the reduce
  terms dnormals, masked ... with an all-ones visibility mask (the MASKED instance)

Each round times `chunk` calls of one variant between two device events after a warm-up; rounds go on until every variant
has at least `--window` seconds of timed calls.  One JSON line per (shape, variant): median, fastest and slowest round in
microseconds per call and the ratio of the medians to the terms forward and to the terms backward.  Per pair the new kernel
does the forward's geometry and three transcendentals and 6 BC + 6 accumulate multiply-adds against the forward's 6 BC (9 BC
with T).  `--out FILE` also appends the lines to FILE."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reni_amd import ops  # noqa: E402
from reni_amd.utils import get_directions, get_sineweight  # noqa: E402


def problem(B, S, W, dev):
    g = torch.Generator().manual_seed(7)
    NP = S * S
    nrm = torch.randn(NP, 3, generator=g) * 0.7
    pos = torch.randn(NP, 3, generator=g) * 0.4
    bg = torch.rand(NP, generator=g) < 0.2
    nrm[bg] = 0.0
    pos[bg] = 0.0
    D = get_directions(W)[0]
    C = torch.exp(torch.randn(B, D.shape[0], 3, generator=g)) * get_sineweight(W)[0]
    w = torch.randn(B, NP, 3, generator=g)
    w2 = torch.randn(B, NP, 3, generator=g)
    return [t.to(dev) for t in (nrm, pos, D, C, w, w2)]


def round_us(fn, chunk):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(chunk):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / chunk * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed calls per variant, at least")
    ap.add_argument("--chunk", type=int, default=20, help="calls per round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    cam = torch.tensor([0.0, 0.0, 2.0])
    lines = []
    for name, B, S, W in (("64x64 render, 64x128 map, B=1", 1, 64, 128), ("128x128 render, 64x128 map, B=3", 3, 128, 128)):
        nrm, pos, D, C, w, w2 = problem(B, S, W, dev)
        shin = torch.full((1,), 500.0, device=dev)
        ones = torch.full((1, S * S, (D.shape[0] + 31) // 32), -1, dtype=torch.int32, device=dev)
        variants = {
            "terms forward": lambda: ops.envmap_shade_terms(nrm, pos, cam, D, C, shin),
            "terms forward + T": lambda: ops.envmap_shade_terms(nrm, pos, cam, D, C, shin, need_ds=True),
            "terms backward": lambda: ops.envmap_shade_terms_backward(nrm, pos, cam, D, w, w2, shin),
            "terms dnormals": lambda: ops.envmap_shade_terms_dnormals(nrm, pos, cam, D, C, w, w2, shin),
            "terms dnormals, masked": lambda: ops.envmap_shade_terms_dnormals(nrm, pos, cam, D, C, w, w2, shin, vis=ones),
        }
        for fn in variants.values():  # warm-up: code objects, allocator, clocks
            for _ in range(a.chunk):
                fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in variants}
        while min(sum(v) * a.chunk for v in rounds.values()) < a.window * 1e6:
            for k, fn in variants.items():
                rounds[k].append(round_us(fn, a.chunk))
        med = {k: statistics.median(v) for k, v in rounds.items()}
        for k, v in rounds.items():
            lines.append(json.dumps({"shape": name, "variant": k, "us_median": round(med[k], 2), "us_min": round(min(v), 2),
                                     "us_max": round(max(v), 2), "rounds": len(v), "calls_per_round": a.chunk,
                                     "over_terms_forward": round(med[k] / med["terms forward"], 3),
                                     "over_terms_backward": round(med[k] / med["terms backward"], 3),
                                     "device": torch.cuda.get_device_name(0)}))
            print(lines[-1])
        sys.stdout.flush()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
