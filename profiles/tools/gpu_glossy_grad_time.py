"""Backward against forward for glossy lighting, the companion of gpu_glossy_time.py: calls timed with CUDA
events after warm-up, one JSON line per row (kept in profiles/glossy_grad_time.jsonl).

  conv64, conv1   64 maps of 64 x 128 to 64 x 128 and one 128 x 256 map to 128 x 256, one and five lobes per kind: prefilter
                  forward, the transposed convolution with the denominators handed in, and the denominators pass alone
  lookup          64 x 16 384 directions in a 5-level chain of 64 x 128 maps, shared and per-map directions: the forward, the
                  table (taps, stable sort, searchsorted) and the gather, shown separately
  step            the render of FIT_INVERSE at the config's shapes (128 x 128 pixels, a 64 x 128 map, batch 3), forward +
                  backward to the map, HipMeshRenderer against PrefilteredRenderer(out_width=64)
  parity          not a timing: max |PrefilteredRenderer - HipMeshRenderer| at kd = 1 on the G-buffer of
                  tests/test_gpu_glossy_grad.py, as a "diffuse only" line for profiles/glossy_time.jsonl

`--only NAME` runs one row family."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_glossy_time import CHAINS, timed  # noqa: E402
from reni_amd import glossy, ops  # noqa: E402


def row(**kw):
    print(json.dumps(kw))
    sys.stdout.flush()


def conv_rows(name, envs, W, iters):
    from reni_amd.baselines import reni_grid_weights
    from reni_amd.utils import get_directions
    dev = envs.device
    dirs = get_directions(W)[0].to(dev)
    w = torch.as_tensor(reni_grid_weights(W), dtype=torch.float32).to(dev)
    for kind, chain in CHAINS.items():
        for lobes in (chain[1:2], chain):
            kinds, params = [l.kind for l in lobes], [l.param for l in lobes]
            fwd = timed(lambda: glossy.prefilter(envs, lobes), iters=iters)
            den = ops.lobe_denominators(dirs, w, dirs, kinds, params)
            g = torch.randn(envs.shape[0], len(lobes), dirs.shape[0], 3, device=dev)
            bwd = timed(lambda: ops.lobe_convolve_backward(g, dirs, w, dirs, kinds, params, True, den=den), iters=iters)
            dn = timed(lambda: ops.lobe_denominators(dirs, w, dirs, kinds, params), iters=iters)
            row(shape=name, call=f"{kind} x {len(lobes)}", forward_us=round(fwd, 2), backward_us=round(bwd, 2),
                denominators_us=round(dn, 2), backward_over_forward=round(bwd / fwd, 3),
                backward_us_per_lobe=round(bwd / len(lobes), 2))


def lookup_rows(iters):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    chain = torch.rand(64, 5, 64, 128, 3, generator=g).to(dev)
    dirs = torch.randn(64, 16384, 3, generator=g).to(dev)
    level = (torch.rand(64, 16384, generator=g) * 4).to(dev)
    up = torch.randn(64, 16384, 3, generator=g).to(dev)
    for name, d, lv in (("shared directions, level 2.5", dirs[0], 2.5), ("per-map directions, level [N, P]", dirs, level)):
        fwd = timed(lambda: glossy.lookup(chain, d, lv), iters=iters)
        table = ops.envmap_lookup_table(64, 5, 64, 128, d, lv)
        tab = timed(lambda: ops.envmap_lookup_table(64, 5, 64, 128, d, lv), iters=iters)
        gat = timed(lambda: ops.envmap_lookup_backward(up, 5, 64, 128, table=table), iters=iters)
        row(call=f"lookup 64 x 16384, {name}", forward_us=round(fwd, 2), table_us=round(tab, 2), gather_us=round(gat, 2),
            backward_over_forward=round((tab + gat) / fwd, 2), gather_over_forward=round(gat / fwd, 2))


def step_rows(iters):
    from reni_amd.envmap_shader import EnvironmentMap
    from reni_amd.mesh import build_hip_renderer
    from reni_amd.utils import get_directions, get_sineweight
    dev = torch.device("cuda")
    renderer, R, T, mesh = build_hip_renderer(os.path.join(ROOT, "tests", "golden", "teapot.obj"), 0, 128, 0.5, "cuda")
    kw = dict(meshes_world=mesh, R=R, T=T)
    W = 128
    g = torch.Generator().manual_seed(0)
    D, Sw = get_directions(W).expand(3, -1, -1).to(dev), get_sineweight(W).to(dev)
    x = (torch.rand(3, D.shape[1], 3, generator=g) * 2).to(dev).requires_grad_()
    y = torch.randn(3, 128, 128, 3, generator=g).to(dev)
    times = {}
    for name, r in (("HipMeshRenderer", renderer), ("PrefilteredRenderer(out_width=64)",
                                                    glossy.PrefilteredRenderer(renderer.rasterizer, kd=0.5, out_width=64))):
        def fwd():
            with torch.no_grad():
                return r(envmap=EnvironmentMap(environment_map=x, directions=D, sineweight=Sw), **kw)[0]

        def both():
            x.grad = None
            (r(envmap=EnvironmentMap(environment_map=x, directions=D, sineweight=Sw), **kw)[0] * y).sum().backward()

        times[name] = (timed(fwd, iters=iters), timed(both, iters=iters))
        row(call=f"FIT_INVERSE render 3 x 128x128 from a 64x128 map, {name}", forward_us=round(times[name][0], 2),
            forward_backward_us=round(times[name][1], 2))
    a, b = times.values()
    row(call="FIT_INVERSE render, PrefilteredRenderer over HipMeshRenderer", forward=round(b[0] / a[0], 3),
        forward_backward=round(b[1] / a[1], 3))


def parity_rows():
    from tests.test_gpu_glossy_grad import diffuse_parity
    for Wo in (8, 16):
        row(teapot="diffuse only", camera="world origin (shader's quirk)", render=32, map_width=16, out_width=Wo,
            max_rel=round(diffuse_parity(Wo), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    if a.only in (None, "conv64"):
        conv_rows("64 x 64x128 -> 64x128", (torch.rand(64, 64 * 128, 3, generator=g) * 2).to(dev), 128, a.iters)
    if a.only in (None, "conv1"):
        conv_rows("1 x 128x256 -> 128x256", (torch.rand(1, 128 * 256, 3, generator=g) * 2).to(dev), 256, a.iters)
    if a.only in (None, "lookup"):
        lookup_rows(a.iters)
    if a.only in (None, "step"):
        step_rows(a.iters)
    if a.only == "parity":
        parity_rows()


if __name__ == "__main__":
    main()
