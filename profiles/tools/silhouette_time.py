"""Timings of the soft silhouette and its backward beside the hard rasteriser and the G-buffer backward of the same
build.

The scene is the teapot fixture (1292 vertices, 2464 faces) from look_at_view_transform(2, 0, 0) at 128 x 128 and 256 x 256,
sigma = 1e-4 and the default blur_radius log(1 / 1e-4 - 1) sigma.  Variants, alternated round by round in one process so that
clock and box drift hit all of them alike:

  silhouette forward   ops.soft_silhouette: face set-up + tile kernel
  silhouette backward  ops.soft_silhouette_backward with the vertex -> corner lists kept: set-up, wave per face, vertex gather
  raster forward       ops.rasterize_mesh
  gbuffer backward     ops.gbuffer_backward with the pixel table and the lists kept

Each round times `chunk` calls of one variant between two device events after a warm-up; rounds go on until every variant has
at least `--window` seconds of timed calls of its own.  One JSON line per variant and size: median, fastest and slowest round in
microseconds per call, and the pixels of the faces' grown boxes (what the backward's waves walk: the largest box, the mean, the
sum).  `--out FILE` also appends the lines to FILE."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reni_amd import ops  # noqa: E402
from reni_amd.mesh import load_obj, look_at_view_transform  # noqa: E402

TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")
SIGMA = 1e-4
TANF = 0.5773502691896258


def round_us(fn, chunk):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(chunk):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / chunk * 1e3


def box_pixels(v, f, R, T, S, r):
    """pixels of every face's NDC box grown by sqrt(r) and clipped to the view (an estimate from the box's sides)"""
    q = v[f] @ R[0] + T[0]
    x, y = q[..., 0] / (q[..., 2] * TANF), q[..., 1] / (q[..., 2] * TANF)
    g = math.sqrt(r)

    def side(c):
        lo, hi = (c.min(dim=1).values - g).clamp(-1, 1), (c.max(dim=1).values + g).clamp(-1, 1)
        return (hi - lo) * S / 2.0

    n = side(x) * side(y)
    return {"box_pixels_max": round(float(n.max()), 1), "box_pixels_mean": round(float(n.mean()), 1), "box_pixels_sum": round(float(n.sum()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed calls per variant, at least")
    ap.add_argument("--chunk", type=int, default=20, help="calls per round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    v, f = load_obj(TEAPOT)
    v, f = v.to(dev), f.to(dev)
    R, T = look_at_view_transform(2.0, 0.0, 0.0, device=dev)
    r = math.log(1.0 / 1e-4 - 1.0) * SIGMA
    vn = ops.vertex_normals(v, f)
    vf = ops.vertex_face_lists(f, v.shape[0])
    lines = []
    for S in (128, 256):
        p2f = ops.rasterize_mesh(v, f, vn, R, T, S)[0]
        g = torch.Generator().manual_seed(1)
        gA, gN, gX = torch.randn(S * S, generator=g).to(dev), torch.randn(S * S, 3, generator=g).to(dev), torch.randn(S * S, 3, generator=g).to(dev)
        table = ops.face_pixel_table(p2f, f.shape[0])
        alpha, trans = ops.soft_silhouette(v, f, R, T, S, TANF, SIGMA, r)
        variants = {
            "silhouette forward": lambda: ops.soft_silhouette(v, f, R, T, S, TANF, SIGMA, r),
            "silhouette backward": lambda: ops.soft_silhouette_backward(v, f, R, T, S, TANF, SIGMA, r, trans, gA, vf=vf),
            "raster forward": lambda: ops.rasterize_mesh(v, f, vn, R, T, S),
            "gbuffer backward": lambda: ops.gbuffer_backward(v, f, vn, R, T, S, p2f, gN, gX, table=table, vf=vf),
        }
        for fn in variants.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        todo = set(variants)
        while todo:
            for k, fn in variants.items():
                if k in todo:
                    times[k].append(round_us(fn, a.chunk))
                    if sum(times[k]) * a.chunk >= a.window * 1e6:
                        todo.discard(k)
        boxes = box_pixels(v, f, R, T, S, r)
        for k, t in times.items():
            line = {"scene": f"teapot V={v.shape[0]} F={f.shape[0]}, {S}x{S}, covered {int((p2f >= 0).sum())}, soft {int((alpha > 0).sum())}",
                    "sigma": SIGMA, "blur_radius": r, "variant": k, "us_median": round(statistics.median(t), 2),
                    "us_min": round(min(t), 2), "us_max": round(max(t), 2), "rounds": len(t), "calls_per_round": a.chunk,
                    "device": torch.cuda.get_device_name(0)}
            line.update(boxes)
            lines.append(line)
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
