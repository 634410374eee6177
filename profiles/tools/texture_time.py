"""Timings of the UV-texture path -> profiles/texture_time.jsonl.

Workload: a latitude / longitude sphere (64 x 32 segments, duplicated seam) rendered at 128 x 128 from
look_at_view_transform(2.7, 10, 30), a 512 x 512 three-channel texture with its full pyramid (10 levels).  Variants,
alternated round by round in one process so that clock and box drift hit all of them alike:

  once per scene               pixel_uv; taps; the table's sort + searchsorted (ops.texture_table)
  per step                     pyramid; fetch; fetch backward; pyramid backward; textures.sample forward + backward (all four)
  yardstick                    torch.nn.functional.grid_sample (bilinear, border, one level) forward, and forward + backward
                               through its own autograd (float atomics) on the same uv
  long range                   the backward of every pixel on a 1 x 1 texture at P = 128^2 (one texel owns all P weighted taps):
                               the chunked form against the plain one-lane-per-texel form of the same kernel (plain = 1)

Each round times a few calls of one variant (about --round-us of work, at most --chunk calls) between two device events
after a warm-up; rounds go on until every variant has at least `--window` seconds of timed calls.  One JSON line per
variant: median, fastest and slowest round in microseconds per call.  `--out FILE` also appends the lines to FILE."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reni_amd import ops, textures  # noqa: E402
from reni_amd.mesh import (FoVPerspectiveCameras, Meshes, MeshRasterizer, RasterizationSettings,  # noqa: E402
                           look_at_view_transform)


def uv_sphere(n_lon, n_lat):
    verts, uvs, faces, fuv = [], [], [], []
    for j in range(n_lat + 1):
        th = math.pi * j / n_lat
        for i in range(n_lon + 1):
            ph = 2 * math.pi * i / n_lon
            if i < n_lon:
                verts.append([math.sin(th) * math.sin(ph), math.cos(th), math.sin(th) * math.cos(ph)])
            uvs.append([i / n_lon, 1.0 - j / n_lat])
    for j in range(n_lat):
        for i in range(n_lon):
            a, b = j * n_lon + i, j * n_lon + (i + 1) % n_lon
            c, d = a + n_lon, b + n_lon
            ta, tb = j * (n_lon + 1) + i, j * (n_lon + 1) + i + 1
            tc, td = ta + n_lon + 1, tb + n_lon + 1
            if j > 0:
                faces.append([a, c, b]); fuv.append([ta, tc, tb])
            if j < n_lat - 1:
                faces.append([b, c, d]); fuv.append([tb, tc, td])
    return torch.tensor(verts), torch.tensor(faces), torch.tensor(uvs), torch.tensor(fuv)


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
    ap.add_argument("--chunk", type=int, default=200, help="calls per round, at most")
    ap.add_argument("--round-us", type=float, default=2000.0, help="microseconds of calls per round and variant, about")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    S, H, C = 128, 512, 3
    v, f, vt, ft = (t.to(dev) for t in uv_sphere(64, 32))
    mesh = Meshes(verts=[v], faces=[f], verts_uvs=[vt], faces_uvs=[ft])
    R, T = look_at_view_transform(2.7, 10.0, 30.0, device=dev)
    cams = FoVPerspectiveCameras(device=dev)
    ras = MeshRasterizer(cameras=cams, raster_settings=RasterizationSettings(image_size=S))
    frags = ras.gbuffer(mesh, R, T)[0]
    uv, jac, valid = ras.pixel_uv(mesh, R, T)
    taps = ras.texture_taps(mesh, R, T, size=(H, H))
    L, E = taps.levels, taps.elements
    g = torch.Generator().manual_seed(3)
    tex = torch.rand(H, H, C, generator=g).to(dev)
    buf = torch.zeros(E, C, device=dev)
    buf[: H * H] = tex.reshape(-1, C)
    gout = torch.randn(S * S, C, generator=g).to(dev)
    gbuf = torch.randn(E, C, generator=g).to(dev)
    texp = tex.clone().requires_grad_(True)
    # the yardstick: grid_sample on the same uv
    grid = torch.stack([2 * uv[:, 0] - 1, 1 - 2 * uv[:, 1]], 1).reshape(1, 1, -1, 2)
    img = tex.permute(2, 0, 1)[None].contiguous()
    imgp = img.clone().requires_grad_(True)
    gs_g = gout.t().reshape(1, C, 1, -1).contiguous()

    def gs_fwd():
        return torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=False)

    def gs_fwd_bwd():
        imgp.grad = None
        torch.nn.functional.grid_sample(imgp, grid, mode="bilinear", padding_mode="border", align_corners=False).backward(gs_g)

    def sample_fwd_bwd():
        texp.grad = None
        textures.sample(texp, taps).backward(gout)

    # the long range: every pixel on a 1 x 1 texture
    taps1 = textures.make_taps(uv, (1, 1))
    table1 = (taps1.order, taps1.offsets)
    variants = {
        "scene: pixel_uv": lambda: ops.mesh_pixel_uv(v, f, vt, ft, R, T, S, frags.pix_to_face, frags.bary_coords, cams.tan_half_fov()),
        "scene: taps": lambda: ops.texture_taps(uv, (H, H), L, jac=jac, pix_valid=valid),
        "scene: table (sort + searchsorted)": lambda: ops.texture_table(taps.index, E, taps.weight),
        "step: pyramid": lambda: ops.texture_pyramid(buf, L, H, H),
        "step: fetch": lambda: ops.texture_fetch(buf, taps.index, taps.weight),
        "step: fetch backward": lambda: ops.texture_fetch_backward(gout, taps.weight, (taps.order, taps.offsets), E),
        "step: fetch backward, plain": lambda: ops.texture_fetch_backward(gout, taps.weight, (taps.order, taps.offsets), E, plain=True),
        "step: pyramid backward": lambda: ops.texture_pyramid_backward(gbuf, L, H, H),
        "step: sample forward + backward": sample_fwd_bwd,
        "yardstick: grid_sample forward": gs_fwd,
        "yardstick: grid_sample forward + backward": gs_fwd_bwd,
        "long range (1x1, P=128^2): chunked": lambda: ops.texture_fetch_backward(gout, taps1.weight, table1, 1),
        "long range (1x1, P=128^2): plain": lambda: ops.texture_fetch_backward(gout, taps1.weight, table1, 1, plain=True),
    }
    for fn in variants.values():  # warm-up: code objects, allocator, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # calls per round and variant: about --round-us of work each (at least 1, at most --chunk), so that a 100 ms call and a 10 us
    # call share the rounds; the rounds still alternate the variants
    chunk = {k: max(1, min(a.chunk, int(a.round_us / max(round_us(fn, 2), 1e-3)))) for k, fn in variants.items()}
    rounds = {k: [] for k in variants}
    while min(sum(r) * chunk[k] for k, r in rounds.items()) < a.window * 1e6:
        for k, fn in variants.items():
            rounds[k].append(round_us(fn, chunk[k]))
    lines = []
    for k, r in rounds.items():
        lines.append(json.dumps({"workload": f"sphere {S}x{S}, texture {H}x{H}x{C}, {L} levels, E={E}, covered pixels={int((valid >= 0).sum())}",
                                 "variant": k, "us_median": round(statistics.median(r), 2), "us_min": round(min(r), 2),
                                 "us_max": round(max(r), 2), "rounds": len(r), "calls_per_round": chunk[k],
                                 "device": torch.cuda.get_device_name(0)}))
        print(lines[-1])
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
