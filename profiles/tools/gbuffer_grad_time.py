"""Timings of the G-buffer's backward beside the forward rasteriser of the same build, and of a geometry-fit step
beside the same step with constant vertices.

The scene is the teapot fixture (1292 vertices, 2464 faces) at 128 x 128 from look_at_view_transform(2, 0, 0); the steps render it
with kd = 1 under a 64 x 128 map (B = 1), take an MSE against a fixed image and step torch.optim.Adam.  Variants, alternated round
by round in one process so that clock and box drift hit all of them alike:

  vertex normals          ops.vertex_normals (its vertex -> corner sort included, as Meshes calls it)
  raster forward          ops.rasterize_mesh: face set-up + tile rasteriser + interpolation
  pixel table             ops.face_pixel_table: the stable sort of pix_to_face and the searchsorted (per step in a fit: the
                          vertices move, so the assignment is new)
  gbuffer backward        ops.gbuffer_backward with the table and the vertex -> corner lists kept: its three kernels
  vertex normals backward ops.vertex_normals_backward with the lists kept
  step, map only          forward + backward + Adam on the map; constant vertices (the G-buffer is cached)
  step, map + vertices    the same with the vertices a second parameter: normals, raster, table and the backward every step

Each round times `chunk` calls of one variant between two device events after a warm-up; rounds go on until every variant has
at least `--window` seconds of timed calls of its own.  One JSON line per variant: median, fastest and slowest round in microseconds per
call.  `--out FILE` also appends the lines to FILE."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reni_amd import ops  # noqa: E402
from reni_amd.envmap_shader import EnvironmentMap  # noqa: E402
from reni_amd.mesh import (FoVPerspectiveCameras, HipMeshRenderer, MeshRasterizer, Meshes, RasterizationSettings, load_obj,  # noqa: E402
                           look_at_view_transform)
from reni_amd.utils import get_directions, get_sineweight  # noqa: E402

TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")
S, W = 128, 128


def round_us(fn, chunk):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(chunk):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / chunk * 1e3


def make_step(verts, faces, R, T, learn_verts, dev):
    g = torch.Generator().manual_seed(3)
    D, Sw = get_directions(W).to(dev), get_sineweight(W).to(dev)
    C = torch.nn.Parameter((torch.rand(1, D.shape[1], 3, generator=g) + 0.5).to(dev))
    v = verts.clone().requires_grad_(learn_verts)
    mesh = Meshes(verts=[v], faces=[faces])
    renderer = HipMeshRenderer(MeshRasterizer(FoVPerspectiveCameras(device=dev), RasterizationSettings(image_size=S)), kd=1.0)
    target = torch.rand(1, S, S, 3, generator=g).to(dev)
    opt = torch.optim.Adam([C, v] if learn_verts else [C], lr=1e-6)  # (timing only: the scene stays what it is)

    def step():
        col, _ = renderer(meshes_world=mesh, R=R, T=T, envmap=EnvironmentMap(environment_map=C, directions=D, sineweight=Sw))
        loss = ((col - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


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
    vn = ops.vertex_normals(v, f)
    p2f = ops.rasterize_mesh(v, f, vn, R, T, S)[0]
    g = torch.Generator().manual_seed(1)
    gN, gX, gn = (torch.randn(n, 3, generator=g).to(dev) for n in (S * S, S * S, v.shape[0]))
    table, vf = ops.face_pixel_table(p2f, f.shape[0]), ops.vertex_face_lists(f, v.shape[0])
    variants = {
        "vertex normals": lambda: ops.vertex_normals(v, f),
        "raster forward": lambda: ops.rasterize_mesh(v, f, vn, R, T, S),
        "pixel table": lambda: ops.face_pixel_table(p2f, f.shape[0]),
        "gbuffer backward": lambda: ops.gbuffer_backward(v, f, vn, R, T, S, p2f, gN, gX, table=table, vf=vf),
        "vertex normals backward": lambda: ops.vertex_normals_backward(v, f, gn, vf=vf),
        "step, map only": make_step(v, f, R, T, False, dev),
        "step, map + vertices": make_step(v, f, R, T, True, dev),
    }
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    todo = set(variants)
    while todo:  # (a variant leaves the rotation when its own window is full: they differ by two orders of magnitude)
        for k, fn in variants.items():
            if k in todo:
                times[k].append(round_us(fn, a.chunk))
                if sum(times[k]) * a.chunk >= a.window * 1e6:
                    todo.discard(k)
    lines = []
    for k, t in times.items():
        lines.append({"scene": f"teapot V={v.shape[0]} F={f.shape[0]}, {S}x{S}, covered {int((p2f >= 0).sum())}", "variant": k,
                      "us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                      "rounds": len(t), "calls_per_round": a.chunk, "device": torch.cuda.get_device_name(0)})
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
