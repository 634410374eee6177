"""Timings of the mesh regularisers: the fused HIP call beside a plain-torch composition of the same definitions.

The mesh is the teapot fixture (1292 vertices, 2464 faces); weights edge 1, laplacian 1, normal 1, target_length 0.05.
Variants, alternated round by round in one process so that clock and box drift hit all of them alike:

  hip value <method>        ops.mesh_regularizers(need_grad=False), the topology lists kept
  hip value+grad <method>   ops.mesh_regularizers, the lists kept: the gradient comes with the forward
  torch fwd+bwd <method>    float32 torch on the device: gathers, norms, index_add scatters over the same lists (kept), autograd's
                            backward.  Its scatter-adds are float atomics: the gradient's bits depend on the run.

for <method> in uniform, cot.  Each round times `chunk` calls of one variant between two device events after a warm-up; rounds go
on until every variant has at least `--window` seconds of timed calls of its own.  One JSON line per variant: median, fastest
and slowest round in microseconds per call, and the number of kernel launches of one call (counted by the torch profiler; null
where it is not available).  `--out FILE` also appends the lines to FILE."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reni_amd import ops  # noqa: E402
from reni_amd.mesh import load_obj  # noqa: E402

TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")
WEIGHTS, TARGET = (1.0, 1.0, 1.0), 0.05


def round_us(fn, chunk):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(chunk):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / chunk * 1e3


def torch_tables(faces, L):
    """the index tensors of the composition, built once: the edges' ends, the directed neighbour entries, the faces taking
    part with the edge opposite each corner, the pairs (edge, c, d)"""
    E = L["E"]
    edges = L["edges"][:E]
    a, b = edges[:, 0], edges[:, 1]
    ce = L["corner_edges"].reshape(-1, 3)
    part = (ce >= 0).all(dim=1).nonzero()[:, 0]
    off, cor = L["ef_offsets"].tolist(), L["ef_corners"].tolist()
    flat = faces.reshape(-1).tolist()
    pairs = [(e, flat[cor[i]], flat[cor[j]]) for e in range(E) for i in range(off[e], off[e + 1]) for j in range(i + 1, off[e + 1])]
    pairs = torch.tensor(pairs, dtype=torch.int64, device=faces.device).reshape(-1, 3)
    v = torch.cat([a, b])
    deg = torch.zeros(int(L["V"]), dtype=torch.float32, device=a.device).index_add(0, v, torch.ones(2 * E, device=a.device))
    return {"a": a, "b": b, "v": v, "j": torch.cat([b, a]), "e2": torch.cat([torch.arange(E, device=a.device)] * 2),
            "tri": faces[part], "tri_edge": ce[part], "pairs": pairs, "E": E, "deg": deg,  # deg: a constant of the topology
            "n_uniform": torch.where(deg > 0, 1.0 / deg.clamp_min(1.0), deg), "ones": torch.ones(2 * E, device=a.device)}


def torch_objective(x, t, method):
    V, E = x.shape[0], t["E"]
    ln = (x[t["a"]] - x[t["b"]]).norm(dim=1)
    Le = ((ln - TARGET) ** 2).sum() / E
    deg = t["deg"].to(x.dtype)
    if method == "uniform":  # weights 1: s_v = deg and n_v = 1 / deg are constants of the topology, kept with the lists
        w, n = t["ones"].to(x.dtype), t["n_uniform"].to(x.dtype)
    else:
        with torch.no_grad():
            x0, x1, x2 = (x[t["tri"][:, k]] for k in range(3))
            A, B, C = (x1 - x2).norm(dim=1), (x0 - x2).norm(dim=1), (x0 - x1).norm(dim=1)
            s = 0.5 * (A + B + C)
            area = (s * (s - A) * (s - B) * (s - C)).clamp_min(0.0).sqrt().clamp_min(1e-12)
            cot = torch.stack([B * B + C * C - A * A, A * A + C * C - B * B, A * A + B * B - C * C], 1) / (4.0 * area)[:, None]
            w = torch.zeros(E, dtype=x.dtype, device=x.device).index_add(0, t["tri_edge"].reshape(-1), cot.reshape(-1))[t["e2"]]
        with torch.no_grad():
            s_v = torch.zeros(V, dtype=x.dtype, device=x.device).index_add(0, t["v"], w)
            n = torch.where(s_v > 0, 1.0 / s_v.clamp_min(1e-30), s_v)
    S = torch.zeros_like(x).index_add(0, t["v"], w[:, None] * x[t["j"]])
    r = torch.where((deg > 0)[:, None], S * n[:, None] - x, torch.zeros_like(x))
    Ll = r.norm(dim=1).sum() / V
    p = t["pairs"]
    xa, xb = x[t["a"][p[:, 0]]], x[t["b"][p[:, 0]]]
    e, c, d = xb - xa, x[p[:, 1]] - xa, x[p[:, 2]] - xa
    n0, n1 = torch.cross(e, c, dim=1), -torch.cross(e, d, dim=1)
    cs = (n0 * n1).sum(1) / (n0.norm(dim=1).clamp_min(1e-8) * n1.norm(dim=1).clamp_min(1e-8))
    Ln = (1.0 - cs).sum() / max(p.shape[0], 1)
    return WEIGHTS[0] * Le + WEIGHTS[1] * Ll + WEIGHTS[2] * Ln


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in ev.name.lower()
                   and "memset" not in ev.name.lower())
    except Exception:  # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed calls per variant, at least")
    ap.add_argument("--chunk", type=int, default=20, help="calls per round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    v, f = load_obj(TEAPOT)
    v, f = v.to(dev), f.to(dev)
    L = ops.mesh_edge_lists(f, v.shape[0])
    t = torch_tables(f, L)
    x = v.clone().requires_grad_(True)

    def torch_call(method):
        def call():
            x.grad = None
            torch_objective(x, t, method).backward()
        return call

    variants = {}
    for method in ("uniform", "cot"):
        variants[f"hip value {method}"] = lambda m=method: ops.mesh_regularizers(v, f, *WEIGHTS, target_length=TARGET, method=m, lists=L,
                                                                                 need_grad=False)
        variants[f"hip value+grad {method}"] = lambda m=method: ops.mesh_regularizers(v, f, *WEIGHTS, target_length=TARGET, method=m, lists=L)
        variants[f"torch fwd+bwd {method}"] = torch_call(method)
    agree = {}
    for method in ("uniform", "cot"):  # the two paths compute the same thing
        values, g = ops.mesh_regularizers(v, f, *WEIGHTS, target_length=TARGET, method=method, lists=L)
        torch_call(method)()
        agree[method] = {"value_rel": abs(float(values[0]) - float(torch_objective(x, t, method).detach())) / abs(float(values[0])),
                         "grad_rel_l2": float((g - x.grad).norm() / g.norm())}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    launches = {k: count_launches(fn) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    todo = set(variants)
    while todo:
        for k, fn in variants.items():
            if k in todo:
                times[k].append(round_us(fn, a.chunk))
                if sum(times[k]) * a.chunk >= a.window * 1e6:
                    todo.discard(k)
    lines = []
    for k, tm in times.items():
        lines.append({"scene": f"teapot V={v.shape[0]} F={f.shape[0]} E={L['E']} P={L['P']}", "weights": WEIGHTS, "target_length": TARGET,
                      "variant": k, "us_median": round(statistics.median(tm), 2), "us_min": round(min(tm), 2), "us_max": round(max(tm), 2),
                      "rounds": len(tm), "calls_per_round": a.chunk, "launches": launches[k], "agreement": agree[k.split()[-1]],
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
