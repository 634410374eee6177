"""Timings of the cloud-neighbourhood unit: ``knn_points`` and ``estimate_normals`` beside ``nearest_points`` and
plain-torch compositions of the same definitions, in points_time.py's protocol (its ``measure``: variants alternated round by
round in one process, `chunk` calls between two device events, at least `--window` seconds of timed calls per variant; median,
fastest and slowest round, launches, peak device memory).

Clouds: N = M points uniform in [-1, 1]^3 from a seed, N = 5 000, 20 000 and 100 000.  Variants per size:

  hip nearest           ops.nearest_points(x, y): the 1-nearest search of reni_tu_points.hip, two queries per lane
  hip knn K             ops.knn_points(x, y, K), K = 1, 8, 16, 32: its pair rate N M / time stands beside the VALU issue bound
                        of the COMPARE path alone (7 instructions a pair in the emitted ISA); how far below it a K falls is
                        what the insertions cost
  torch topk 16         torch.cdist(x, y) ** 2 -> topk(16, largest=False): it materialises the N x M matrix; below 100 000 only
  hip normals 16        mesh_losses.estimate_normals(y, 16): one search and reni_cloud_normals
  torch normals 16      cdist -> topk -> covariance -> torch.linalg.eigh; below 100 000 only

`--out FILE` also appends the JSON lines to FILE."""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from points_time import CLOCK_HZ, CUS, CYCLES_PER_VALU, SIMDS, measure  # noqa: E402
from reni_amd import mesh_losses, ops  # noqa: E402

SIZES = (5000, 20000, 100000)
KS = (1, 8, 16, 32)
TORCH_MAX = 20000
# k_knn_search's compare path in the emitted ISA (isa_core.sh knn): per staged target and lane 3 v_sub_f32 + 1 v_mul_f32 +
# 2 v_fma_f32 + 1 v_cmp_lt_f32 = 7 VALU instructions a pair (the ballot's branch is scalar)
VALU_PER_PAIR = 7.0
ISSUE_BOUND_PAIRS_PER_S = 64.0 / (VALU_PER_PAIR * CYCLES_PER_VALU) * SIMDS * CUS * CLOCK_HZ


def torch_topk(x, y, k):
    return (torch.cdist(x, y) ** 2).topk(k, dim=1, largest=False)


def torch_normals(y, k):
    idx = torch_topk(y, y, k)[1]
    pts = y[idx]
    e = pts - pts.mean(1, keepdim=True)
    return torch.linalg.eigh(torch.einsum("nka,nkb->nab", e, e) / k)[1][:, :, 0]


def variants_of(n, dev):
    g = torch.Generator(device=dev).manual_seed(n)
    x = torch.rand(n, 3, device=dev, generator=g) * 2 - 1
    y = torch.rand(n, 3, device=dev, generator=g) * 2 - 1
    v = {"hip nearest": lambda: ops.nearest_points(x, y)}
    for k in KS:
        v[f"hip knn {k}"] = lambda k=k: ops.knn_points(x, y, k)
    v["hip normals 16"] = lambda: mesh_losses.estimate_normals(y, 16)
    skipped = {}
    if n <= TORCH_MAX:
        v["torch topk 16"] = lambda: torch_topk(x, y, 16)
        v["torch normals 16"] = lambda: torch_normals(y, 16)
    else:
        msg = f"not run: the N x M matrix alone is {4 * n * n / 2 ** 30:.0f} GiB"
        skipped = {"torch topk 16": msg, "torch normals 16": msg}
    return v, skipped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed calls per variant, at least")
    ap.add_argument("--chunk", type=int, default=5, help="calls per round")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_time.py measures on a GPU; none is available")
    dev = torch.device("cuda")
    name = torch.cuda.get_device_name(0)
    lines = []
    for n in a.sizes:
        variants, skipped = variants_of(n, dev)
        res = measure(variants, a.window, a.chunk)
        for k, r in res.items():
            line = {"what": "knn", "N": n, "M": n, "variant": k, **r, "device": name}
            if k.startswith("hip knn") or k == "hip nearest":
                rate = n * n / (r["us_median"] * 1e-6)
                line.update(pairs_per_s=rate)
                if k.startswith("hip knn"):
                    line.update(compare_path_issue_bound_pairs_per_s=ISSUE_BOUND_PAIRS_PER_S,
                                share_of_compare_path_bound=rate / ISSUE_BOUND_PAIRS_PER_S, valu_per_pair_compare_path=VALU_PER_PAIR)
            lines.append(line)
        for k, why in skipped.items():
            lines.append({"what": "knn", "N": n, "M": n, "variant": k, "result": why, "device": name})
        del variants
        torch.cuda.empty_cache()
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
