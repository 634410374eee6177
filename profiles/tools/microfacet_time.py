"""Timings of the microfacet (GGX) terms beside the Blinn-Phong terms of the same build.

The workloads of shade_materials_time.py and normal_map_time.py: a 64 x 64 render under a 64 x 128 map with B = 1, and 128 x 128
under 64 x 128 with B = 3, on the random G-buffer of the shader's tests (20 % background), a shared grid (the BC = 4 instances);
shininess 500 for the Blinn-Phong terms, roughness 0.5 (alpha 0.25) for the microfacet ones -- neither kernel's time depends on
the value.  Variants, alternated round by round in one process so that clock and box drift hit all of them alike:

  terms forward + T      ops.envmap_shade_terms with dS/ds: 9 BC accumulators, the GGX forward's nearest relative
  terms backward         ops.envmap_shade_terms_backward
  terms dnormals         ops.envmap_shade_terms_dnormals
  ggx forward            ops.envmap_shade_ggx                        (ratio to terms forward + T)
  ggx backward           ops.envmap_shade_ggx_backward               (ratio to terms backward)
  ggx dpixel             ops.envmap_shade_ggx_dpixel, d alpha only   (ratio to terms dnormals)
  ggx dpixel + dn        ... with the normals' gradient              (ratio to terms dnormals)

Each round times `chunk` calls of one variant between two device events after a warm-up; rounds go on until every variant
has at least `--window` seconds of timed calls.  One JSON line per (shape, variant): median, fastest and slowest round in
microseconds per call and, for the ggx variants, the ratio of the medians to the Blinn-Phong sibling.  `--out FILE` also appends
the lines to FILE."""
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

SIBLING = {"ggx forward": "terms forward + T", "ggx backward": "terms backward", "ggx dpixel": "terms dnormals",
           "ggx dpixel + dn": "terms dnormals"}


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
    ups = [torch.randn(B, NP, 3, generator=g) for _ in range(3)]
    return [t.to(dev) for t in (nrm, pos, D, C, *ups)]


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
        nrm, pos, D, C, w, w2, w3 = problem(B, S, W, dev)
        shin = torch.full((1,), 500.0, device=dev)
        al = torch.full((1,), 0.25, device=dev)
        variants = {
            "terms forward + T": lambda: ops.envmap_shade_terms(nrm, pos, cam, D, C, shin, need_ds=True),
            "terms backward": lambda: ops.envmap_shade_terms_backward(nrm, pos, cam, D, w, w2, shin),
            "terms dnormals": lambda: ops.envmap_shade_terms_dnormals(nrm, pos, cam, D, C, w, w2, shin),
            "ggx forward": lambda: ops.envmap_shade_ggx(nrm, pos, cam, D, C, al),
            "ggx backward": lambda: ops.envmap_shade_ggx_backward(nrm, pos, cam, D, w, w2, w3, al),
            "ggx dpixel": lambda: ops.envmap_shade_ggx_dpixel(nrm, pos, cam, D, C, w, w2, w3, al),
            "ggx dpixel + dn": lambda: ops.envmap_shade_ggx_dpixel(nrm, pos, cam, D, C, w, w2, w3, al, need_dn=True),
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
            rec = {"shape": name, "variant": k, "us_median": round(med[k], 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                   "rounds": len(v), "calls_per_round": a.chunk, "device": torch.cuda.get_device_name(0)}
            if k in SIBLING:
                rec["sibling"] = SIBLING[k]
                rec["over_sibling"] = round(med[k] / med[SIBLING[k]], 3)
            lines.append(json.dumps(rec))
            print(lines[-1])
        sys.stdout.flush()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
