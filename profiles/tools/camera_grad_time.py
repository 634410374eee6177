"""Timings of the camera gradients beside the backward calls they extend, in one process.

The scene is the teapot fixture (1292 vertices, 2464 faces) from look_at_view_transform(2, 0, 0) at 128 x 128 and 256 x 256,
sigma = 1e-4 and the default blur_radius log(1 / 1e-4 - 1) sigma, as profiles/tools/silhouette_time.py.  Variants, alternated
round by round so that clock and box drift hit all of them alike:

  silhouette backward              ops.soft_silhouette_backward (the existing call: set-up, wave per face, vertex gather)
  silhouette backward + camera     ops.soft_silhouette_backward_camera: the camera instance of the face kernel and the reducer
  silhouette camera only           ... with need_verts=False: no vertex gather
  gbuffer backward                 ops.gbuffer_backward with the pixel table and the lists kept
  gbuffer backward + camera        ops.gbuffer_backward_camera
  gbuffer camera only              ... with need_verts=False: no vertex gather, no vertex-normal chain
  pose-fit step                    one step of a camera-position fit through MeshRasterizer.silhouette: camera_from_position,
                                   the soft IoU, backward, Adam (a new R every step re-rasterises: forward + camera-only backward)

Each round times `chunk` calls of one variant between two device events after a warm-up; rounds go on until every variant has
at least `--window` seconds of timed calls of its own.  One JSON line per variant and size: median, fastest and slowest round in
microseconds per call.  `--out FILE` also appends the lines to FILE."""
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
from reni_amd.mesh import (FoVPerspectiveCameras, MeshRasterizer, Meshes, RasterizationSettings, camera_from_position,  # noqa: E402
                           load_obj, look_at_view_transform, silhouette_iou)

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
    mesh = Meshes(verts=[v], faces=[f])
    lines = []
    for S in (128, 256):
        p2f = ops.rasterize_mesh(v, f, vn, R, T, S)[0]
        g = torch.Generator().manual_seed(1)
        gA, gN, gX = torch.randn(S * S, generator=g).to(dev), torch.randn(S * S, 3, generator=g).to(dev), torch.randn(S * S, 3, generator=g).to(dev)
        table = ops.face_pixel_table(p2f, f.shape[0])
        alpha, trans = ops.soft_silhouette(v, f, R, T, S, TANF, SIGMA, r)
        mask = (alpha > 0.5).reshape(S, S)
        rast = MeshRasterizer(FoVPerspectiveCameras(device=dev), RasterizationSettings(image_size=S))
        pos = torch.tensor([0.3, 0.2, 2.2], device=dev, requires_grad=True)
        opt = torch.optim.Adam([pos], lr=1e-3)

        def fit_step():
            Rp, Tp = camera_from_position(pos)
            loss = silhouette_iou(rast.silhouette(mesh, Rp, Tp, sigma=SIGMA, blur_radius=r), mask)
            opt.zero_grad()
            loss.backward()
            opt.step()

        sil = (v, f, R, T, S, TANF, SIGMA, r, trans, gA)
        gb = (v, f, vn, R, T, S, p2f, gN, gX)
        variants = {
            "silhouette backward": lambda: ops.soft_silhouette_backward(*sil, vf=vf),
            "silhouette backward + camera": lambda: ops.soft_silhouette_backward_camera(*sil, vf=vf),
            "silhouette camera only": lambda: ops.soft_silhouette_backward_camera(*sil, need_verts=False),
            "gbuffer backward": lambda: ops.gbuffer_backward(*gb, table=table, vf=vf),
            "gbuffer backward + camera": lambda: ops.gbuffer_backward_camera(*gb, table=table, vf=vf),
            "gbuffer camera only": lambda: ops.gbuffer_backward_camera(*gb, table=table, need_verts=False),
            "pose-fit step": fit_step,
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
        for k, t in times.items():
            lines.append({"scene": f"teapot V={v.shape[0]} F={f.shape[0]}, {S}x{S}, covered {int((p2f >= 0).sum())}, soft {int((alpha > 0).sum())}",
                          "sigma": SIGMA, "blur_radius": r, "variant": k, "us_median": round(statistics.median(t), 2),
                          "us_min": round(min(t), 2), "us_max": round(max(t), 2), "rounds": len(t), "calls_per_round": a.chunk,
                          "device": torch.cuda.get_device_name(0)})
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
