"""Glossy prefilter and lookup timings: 50 calls timed with CUDA events after warm-up, one JSON line per row.

  64 maps of 64 x 128 to 64 x 128 with 1 and with 5 lobes, per kind (glossy.prefilter), and irradiance_map at the same shape
  one 128 x 256 map to 128 x 256, likewise
  a lookup of 64 x 16 384 directions in a 5-level chain of 64 x 128 maps, with a per-direction level
  the error of glossy.shade_prefiltered against ops.envmap_shade on the teapot G-buffer (64 x 64 pixels, a 32 x 64 map),
  out_width 32, 64, 128 at shininess 20 and 500: largest and mean absolute difference over the covered pixels, relative to
  the shader's largest value

Time per lobe is reported as a ratio to diffuse_convolve (irradiance_map) at the same shape in the same process.
`--only NAME` runs one row family (conv64, conv1, lookup, teapot): a profiler run wants one."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reni_amd import baselines, glossy, ops  # noqa: E402


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


CHAINS = {"phong": [glossy.phong(n) for n in (1, 8, 64, 500, 4096)],
          "blinn": [glossy.blinn(s) for s in (4, 20, 100, 500, 2000)],
          "ggx": [glossy.ggx(r) for r in (1.0, 0.8, 0.6, 0.4, 0.2)]}


def conv_rows(name, envs, iters):
    base = timed(lambda: baselines.irradiance_map(envs), iters=iters)
    print(json.dumps({"shape": name, "call": "irradiance_map (diffuse_convolve)", "us": round(base, 2)}))
    for kind, chain in CHAINS.items():
        for lobes in (chain[1:2], chain):
            us = timed(lambda: glossy.prefilter(envs, lobes), iters=iters)
            print(json.dumps({"shape": name, "call": f"prefilter {kind} x {len(lobes)}", "us": round(us, 2),
                              "us_per_lobe": round(us / len(lobes), 2), "per_lobe_over_diffuse": round(us / len(lobes) / base, 3)}))
    mixed = [CHAINS["phong"][2], CHAINS["blinn"][1], CHAINS["ggx"][2]]
    us = timed(lambda: glossy.prefilter(envs, mixed), iters=iters)
    print(json.dumps({"shape": name, "call": "prefilter phong + blinn + ggx", "us": round(us, 2),
                      "per_lobe_over_diffuse": round(us / 3 / base, 3)}))
    sys.stdout.flush()


def teapot_rows():
    from reni_amd.envmap_shader import EnvironmentMap
    from reni_amd.mesh import build_hip_renderer
    from reni_amd.utils import get_directions, get_sineweight
    dev = torch.device("cuda")
    renderer, R, T, mesh = build_hip_renderer(os.path.join(ROOT, "tests", "golden", "teapot.obj"), 0, 64, 0.5, "cuda")
    _, nrm, pos = renderer.rasterizer.gbuffer(mesh, R, T)
    # the renderer's shader keeps the reference's quirk, the centre of the DEFAULT camera (the world origin, inside the mesh):
    # there n . v < 0 on most pixels, the shader has no highlight and the n = v = r lobe has one.  The rendering camera's own
    # centre is the sane case; both are reported
    cams = (("rendering camera", renderer.rasterizer.cameras.get_camera_center(R, T).reshape(3).cpu()),
            ("world origin (shader's quirk)", renderer.camera_center))
    g = torch.Generator().manual_seed(0)
    W = 64
    D, Sw = get_directions(W), get_sineweight(W)
    sky = 0.2 + torch.rand(2, D.shape[1], 3, generator=g)
    sky[:, (W // 4) * W + W // 3] += 200.0  # a sun of one texel
    env = EnvironmentMap(environment_map=sky.to(dev), directions=D.expand(2, -1, -1).to(dev), sineweight=Sw.to(dev))
    covered = (nrm != 0).any(-1)
    for cname, cam in cams:
        n, r, _ = glossy.shading_dirs(nrm, pos, cam)
        v = 2.0 * (n * r).sum(-1, keepdim=True) * n - r
        facing = float(((n * v).sum(-1)[covered] > 0).float().mean())
        for s in (20.0, 500.0):
            for kd in (1.0, 0.0):
                if kd == 1.0 and (s != 20.0 or cname != cams[0][0]):
                    continue  # the diffuse term depends on neither
                ref = ops.envmap_shade(nrm, pos, cam, env.directions[0], env.environment_map, s, kd, 1.0 - kd)[:, covered]
                for Wo in (32, 64, 128):
                    out = glossy.shade_prefiltered(env, nrm, pos, cam, s, kd, 1.0 - kd, Wo)[:, covered]
                    d = (out - ref).abs()
                    print(json.dumps({"teapot": "diffuse only" if kd == 1.0 else "specular only", "camera": cname,
                                      "facing": round(facing, 3), "shininess": s, "out_width": Wo,
                                      "max_rel": round(float(d.max() / ref.max()), 5),
                                      "mean_rel": round(float(d.mean() / ref.max()), 6),
                                      "ref_max": round(float(ref.max()), 4), "ref_mean": round(float(ref.mean()), 5)}))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    if a.only in (None, "conv64"):
        conv_rows("64 x 64x128 -> 64x128", (torch.rand(64, 64 * 128, 3, generator=g) * 2).to(dev), a.iters)
    if a.only in (None, "conv1"):
        conv_rows("1 x 128x256 -> 128x256", (torch.rand(1, 128 * 256, 3, generator=g) * 2).to(dev), a.iters)
    if a.only in (None, "lookup"):
        chain = torch.rand(64, 5, 64, 128, 3, generator=g).to(dev)
        dirs = torch.randn(64, 16384, 3, generator=g).to(dev)
        level = (torch.rand(64, 16384, generator=g) * 4).to(dev)
        for name, fn in (("lookup 64 x 16384, level [N, P]", lambda: glossy.lookup(chain, dirs, level)),
                         ("lookup 64 x 16384, level 0", lambda: glossy.lookup(chain, dirs)),
                         ("lookup 64 x 16384 shared directions, level 2.5", lambda: glossy.lookup(chain, dirs[0], 2.5))):
            us = timed(fn, iters=a.iters)
            print(json.dumps({"call": name, "us": round(us, 2), "gdirs_per_s": round(64 * 16384 / us / 1e3, 2)}))
        sys.stdout.flush()
    if a.only in (None, "teapot"):
        teapot_rows()


if __name__ == "__main__":
    main()
