"""Timings of the split-sum path beside the existing calls it stands next to, on the same box and in one process.

  query: glossy.sample forward + backward with d_dirs and d_level against glossy.lookup forward + backward (the maps'
         gradient alone) on the same queries: a chain [1, 8, 32, 64, 3], 128 x 128 queries with a per-query level.
           lookup fwd+bwd (maps)            the sibling: forward, tap table, gather
           sample fwd+bwd (dirs, level)     forward + the dquery kernel
           sample fwd+bwd (maps, dirs, level)  forward + gather + dquery
  fit:   one FIT step -- render, squared error against a target, backward to the map and to a per-pixel roughness -- of
         PrefilteredRenderer(materials=MicrofacetMaterials) against HipMeshRenderer with the same materials, on the teapot, at
         64 x 64 and 128 x 128 pixels under 64 x 128 and 128 x 256 maps (out_width 64, the default chain, B = 1).

Variants alternate round by round so that clock and box drift hit all of them alike.  Each round times `chunk` calls between two
device events after a warm-up; rounds go on until every variant has at least `--window` seconds of timed calls.  One JSON line per
(shape, variant): median, fastest and slowest round in microseconds per call and the ratio of the medians to the sibling.  `--out
FILE` also appends the lines to FILE."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reni_amd import glossy  # noqa: E402
from reni_amd.envmap_shader import EnvironmentMap, MicrofacetMaterials  # noqa: E402
from reni_amd.mesh import build_hip_renderer  # noqa: E402
from reni_amd.utils import get_directions, get_sineweight  # noqa: E402

TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")


def round_us(fn, chunk):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(chunk):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / chunk * 1e3


def measure(name, variants, sibling, chunk, window):
    for fn in variants.values():  # warm-up: code objects, allocator, cached tables, clocks
        for _ in range(max(chunk // 2, 2)):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    while min(sum(v) * chunk for v in rounds.values()) < window * 1e6:
        for k, fn in variants.items():
            rounds[k].append(round_us(fn, chunk))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    lines = []
    for k, v in rounds.items():
        rec = {"shape": name, "variant": k, "us_median": round(med[k], 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
               "rounds": len(v), "calls_per_round": chunk, "device": torch.cuda.get_device_name(0)}
        if k != sibling:
            rec["sibling"] = sibling
            rec["over_sibling"] = round(med[k] / med[sibling], 3)
        lines.append(json.dumps(rec))
        print(lines[-1])
    sys.stdout.flush()
    return lines


def query_variants(dev):
    g = torch.Generator().manual_seed(3)
    chain = torch.rand(1, 8, 32, 64, 3, generator=g).to(dev)
    P = 128 * 128
    dirs = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1).to(dev)
    level = (torch.rand(P, generator=g) * 7.0).to(dev)
    up = torch.randn(1, P, 3, generator=g).to(dev)

    def step(fn, m, d, l):
        m, d, l = m.detach().requires_grad_(m.requires_grad), d.detach().requires_grad_(d.requires_grad), l.detach().requires_grad_(l.requires_grad)
        (fn(m, d, l) * up).sum().backward()

    cg, dg, lg = chain.clone().requires_grad_(True), dirs.clone().requires_grad_(True), level.clone().requires_grad_(True)
    return {
        "lookup fwd+bwd (maps)": lambda: step(glossy.lookup, cg, dirs, level),
        "sample fwd+bwd (dirs, level)": lambda: step(glossy.sample, chain, dg, lg),
        "sample fwd+bwd (maps, dirs, level)": lambda: step(glossy.sample, cg, dg, lg),
    }, "lookup fwd+bwd (maps)"


def fit_variants(S, W, dev):
    g = torch.Generator().manual_seed(11)
    NP = S * S
    D, Sw = get_directions(W).to(dev), get_sineweight(W).to(dev)
    L = torch.exp(torch.randn(1, D.shape[1], 3, generator=g)).to(dev).requires_grad_(True)
    rough = 0.2 + 0.7 * torch.rand(NP, generator=g)
    steps = {}
    for kind in ("exact", "prefiltered"):
        mat = MicrofacetMaterials(torch.rand(NP, 3, generator=g), rough.clone(), 0.5, learn=("roughness",))
        exact, R, T, mesh = build_hip_renderer(TEAPOT, 0, S, None, "cuda", materials=mat)
        r = exact if kind == "exact" else glossy.PrefilteredRenderer(exact.rasterizer, materials=mat, out_width=64)
        with torch.no_grad():
            target = r(meshes_world=mesh, R=R, T=T, envmap=EnvironmentMap(L.detach() * 0.5, D, Sw))[0]

        def step(r=r, mat=mat, R=R, T=T, mesh=mesh, target=target):
            L.grad = None
            mat.roughness.grad = None
            col = r(meshes_world=mesh, R=R, T=T, envmap=EnvironmentMap(L, D, Sw))[0]
            ((col - target) ** 2).mean().backward()

        steps[kind] = step
    return {"HipMeshRenderer FIT step (exact sums)": steps["exact"],
            "PrefilteredRenderer FIT step (split-sum)": steps["prefiltered"]}, "HipMeshRenderer FIT step (exact sums)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed calls per variant, at least")
    ap.add_argument("--chunk", type=int, default=10, help="calls per round")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, choices=("query", "fit"), help="one row family")
    a = ap.parse_args()
    dev = torch.device("cuda")
    lines = []
    if a.only in (None, "query"):
        variants, sibling = query_variants(dev)
        lines += measure("chain 8x32x64, 16384 queries, per-query level", variants, sibling, a.chunk, a.window)
    shapes = ((64, 128), (64, 256), (128, 128), (128, 256), (256, 256))  # (the last: where pixels x texels outgrows the chain)
    for S, W in shapes if a.only in (None, "fit") else ():
        variants, sibling = fit_variants(S, W, dev)
        lines += measure(f"teapot {S}x{S} render, {W // 2}x{W} map, B=1", variants, sibling, a.chunk, a.window)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
