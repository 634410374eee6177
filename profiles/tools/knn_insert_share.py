"""The share of targets at which k_knn_search runs its insertion, counted on the CPU from the kernel's own rule:
a wave of 64 consecutive queries walks the targets in ascending j, and target j triggers the insertion iff, for SOME lane,
d(i, j) is below that lane's K-th smallest distance over the targets before j.  knn_time.py's clouds (uniform in [-1, 1]^3,
seeded by N), one slice, the first `--waves` waves of queries.  One JSON line per (N, K): the share of targets with an event,
the mean number of lanes that improve at an event, and the issue's estimate 64 K ln(M / K) / M beside it.  No device."""
import argparse
import heapq
import json
import math

import numpy as np
import torch


def lane_events(d, K):
    """bool [M]: d[t] < the K-th smallest of d[:t] (+inf while fewer than K came)"""
    out = np.zeros(d.shape[0], dtype=bool)
    heap = []  # the K smallest so far, negated: -heap[0] is the K-th smallest
    for t, v in enumerate(d.tolist()):
        if len(heap) < K:
            heapq.heappush(heap, -v)
            out[t] = True
        elif v < -heap[0]:
            heapq.heapreplace(heap, -v)
            out[t] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[5000, 20000, 100000])
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 8, 16, 32])
    ap.add_argument("--waves", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for n in a.sizes:
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, 3, generator=g) * 2 - 1).numpy().astype(np.float64)
        y = (torch.rand(n, 3, generator=g) * 2 - 1).numpy().astype(np.float64)
        for K in a.ks:
            events = lanes = 0
            for w in range(a.waves):
                q = x[64 * w:64 * w + 64]
                D = ((q[:, None, :] - y[None, :, :]) ** 2).sum(-1)
                imp = np.stack([lane_events(D[l], K) for l in range(q.shape[0])])
                events += int(imp.any(0).sum())
                lanes += int(imp.sum())
            line = {"what": "knn insertion share", "N": n, "M": n, "K": K, "waves": a.waves, "share_of_targets": events / (a.waves * n),
                    "lanes_per_event": lanes / max(events, 1), "issue_estimate": min(1.0, 64 * K * math.log(n / K) / n)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
