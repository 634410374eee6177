"""Timings of the point-cloud unit: ``chamfer_distance`` and ``sample_points_from_meshes`` beside plain-torch
compositions of the same definitions.

Clouds: N = M points uniform in [-1, 1]^3 from a seed, N = 5 000, 20 000 and 100 000.  Variants per size, alternated round by
round in one process so that clock and box drift hit all of them alike:

  hip nearest         ops.nearest_points(x, y): ONE search; its pair rate N M / time stands beside the VALU issue bound
  hip fwd             chamfer_distance under no_grad: two searches and two means
  hip fwd+bwd         chamfer_distance with both clouds requiring grad, then backward: + two stable sorts and two gathers
  torch fwd           D = torch.cdist(x, y) ** 2;  D.min(1).values.mean() + D.min(0).values.mean()
  torch fwd+bwd       the same through autograd.  It materialises the N x M matrix (and its gradient), and its backward
                      scatter-adds with float atomics: the gradient's bits depend on the run.

The composition needs about 4 N M 4 bytes for forward and backward; where the device does not have them free, where they are more
than half of the device (it is shared), or where the allocation fails, that is recorded as the result ("cannot allocate").  Sampling: the teapot fixture, 10 000 samples, ``sample_points_from_meshes``
(area table kept by the Meshes) forward and forward + backward to the vertices, beside areas -> ``torch.multinomial`` ->
index -> barycentrics in torch.

Each round times `chunk` calls of one variant between two device events after a warm-up; rounds go on until every variant has
at least `--window` seconds of timed calls of its own.  One JSON line per variant: median, fastest and slowest round in
microseconds per call, the kernel launches of one call (torch profiler; null where it is not available) and the peak device
memory one call adds.  `--out FILE` also appends the lines to FILE."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reni_amd import mesh_losses, ops  # noqa: E402
from reni_amd.mesh import Meshes, load_obj  # noqa: E402

TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")
SIZES = (5000, 20000, 100000)
SAMPLES = 10000
# k_np_search's inner loop in the emitted ISA (isa_core.sh points): per staged target and lane, for the lane's TWO queries,
# 3 v_pk_add_f32 + 1 v_pk_mul_f32 + 2 v_pk_fma_f32 + 2 v_cmp_lt_f32 + 4 v_cndmask_b32 = 12 VALU instructions, 6 per pair; a
# wave64 VALU instruction occupies its SIMD for 4 cycles; 4 SIMDs per CU, 256 CUs, 2.4 GHz peak clock.
VALU_PER_PAIR, CYCLES_PER_VALU, SIMDS, CUS, CLOCK_HZ = 6.0, 4.0, 4, 256, 2.4e9
ISSUE_BOUND_PAIRS_PER_S = 64.0 / (VALU_PER_PAIR * CYCLES_PER_VALU) * SIMDS * CUS * CLOCK_HZ


def round_us(fn, chunk):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(chunk):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / chunk * 1e3


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def torch_chamfer(x, y):
    D = torch.cdist(x, y) ** 2
    return D.min(dim=1).values.mean() + D.min(dim=0).values.mean()


def torch_sample(verts, faces, n, gen):
    tri = verts[faces]
    with torch.no_grad():
        area = 0.5 * torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1).norm(dim=1)
        f = torch.multinomial(area, n, replacement=True, generator=gen)
        u = torch.rand(n, 2, device=verts.device, generator=gen)
        r = u[:, 0].sqrt()
        w = torch.stack([1 - r, r * (1 - u[:, 1]), r * u[:, 1]], 1)
    return (w[:, :, None] * tri[f]).sum(1)


def cloud_variants(n, dev):
    g = torch.Generator(device=dev).manual_seed(n)
    x = torch.rand(n, 3, device=dev, generator=g) * 2 - 1
    y = torch.rand(n, 3, device=dev, generator=g) * 2 - 1
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)

    def hip_fwd():
        with torch.no_grad():
            return mesh_losses.chamfer_distance(x, y)

    def hip_both():
        xg.grad = yg.grad = None
        mesh_losses.chamfer_distance(xg, yg).backward()

    def torch_fwd():
        with torch.no_grad():
            return torch_chamfer(x, y)

    def torch_both():
        xg.grad = yg.grad = None
        torch_chamfer(xg, yg).backward()

    variants = {"hip nearest": lambda: ops.nearest_points(x, y), "hip fwd": hip_fwd, "hip fwd+bwd": hip_both}
    skipped = {}
    need = 4 * n * n * 4
    free, total = torch.cuda.mem_get_info()
    if need * 1.1 > free or need > total // 2:  # (a device is shared: more than half of it is not taken for a comparison)
        msg = (f"cannot allocate: the composition needs about {need / 2 ** 30:.0f} GiB (4 N M floats); {free / 2 ** 30:.0f} GiB free of "
               f"{total / 2 ** 30:.0f} GiB, and no more than half the device is asked for")
        skipped = {"torch fwd": msg, "torch fwd+bwd": msg}
    else:
        try:
            torch_both()
            torch.cuda.synchronize()
            variants.update({"torch fwd": torch_fwd, "torch fwd+bwd": torch_both})
        except torch.cuda.OutOfMemoryError as e:
            skipped = {"torch fwd": f"cannot allocate: {str(e)[:120]}", "torch fwd+bwd": f"cannot allocate: {str(e)[:120]}"}
        xg.grad = yg.grad = None
        torch.cuda.empty_cache()
    agree = None
    if "torch fwd" in variants:  # the two paths compute the same thing
        a, b = float(hip_fwd()), float(torch_fwd())
        hip_both()
        gx = xg.grad.clone()
        torch_both()
        agree = {"value_rel": abs(a - b) / abs(b), "grad_rel_l2": float((gx - xg.grad).norm() / xg.grad.norm())}
    return variants, skipped, agree


def measure(variants, window, chunk):
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    launches = {k: count_launches(fn) for k, fn in variants.items()}
    peaks = {k: peak_bytes(fn) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    todo = set(variants)
    while todo:
        for k, fn in variants.items():
            if k in todo:
                times[k].append(round_us(fn, chunk))
                if sum(times[k]) * chunk >= window * 1e6:
                    todo.discard(k)
    return {k: {"us_median": round(statistics.median(tm), 2), "us_min": round(min(tm), 2), "us_max": round(max(tm), 2), "rounds": len(tm),
                "calls_per_round": chunk, "launches": launches[k], "peak_bytes": peaks[k]} for k, tm in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed calls per variant, at least")
    ap.add_argument("--chunk", type=int, default=10, help="calls per round")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("points_time.py measures on a GPU; none is available")
    dev = torch.device("cuda")
    name = torch.cuda.get_device_name(0)
    lines = []
    for n in a.sizes:
        variants, skipped, agree = cloud_variants(n, dev)
        res = measure(variants, a.window, a.chunk)
        for k, r in res.items():
            line = {"what": "chamfer", "N": n, "M": n, "variant": k, **r, "agreement": agree, "device": name}
            if k == "hip nearest":
                rate = n * n / (r["us_median"] * 1e-6)
                line.update(pairs_per_s=rate, issue_bound_pairs_per_s=ISSUE_BOUND_PAIRS_PER_S, share_of_issue_bound=rate / ISSUE_BOUND_PAIRS_PER_S,
                            valu_per_pair=VALU_PER_PAIR)
            lines.append(line)
        for k, why in skipped.items():
            lines.append({"what": "chamfer", "N": n, "M": n, "variant": k, "result": why, "device": name})
        del variants
        torch.cuda.empty_cache()
    v, f = load_obj(TEAPOT)
    v, f = v.to(dev), f.to(dev)
    mesh = Meshes(verts=[v.clone().requires_grad_(True)], faces=[f])
    vg = mesh.verts_packed()
    tv = v.clone().requires_grad_(True)
    gen = torch.Generator(device=dev).manual_seed(0)

    def hip_fwd():
        with torch.no_grad():
            return mesh_losses.sample_points_from_meshes(mesh, SAMPLES, generator=gen)

    def hip_both():
        vg.grad = None
        mesh_losses.sample_points_from_meshes(mesh, SAMPLES, generator=gen).sum().backward()

    def hip_table():
        return ops.mesh_sample_table(v, f)

    def torch_fwd():
        with torch.no_grad():
            return torch_sample(v, f, SAMPLES, gen)

    def torch_both():
        tv.grad = None
        torch_sample(tv, f, SAMPLES, gen).sum().backward()

    res = measure({"hip table": hip_table, "hip fwd": hip_fwd, "hip fwd+bwd": hip_both, "torch fwd": torch_fwd, "torch fwd+bwd": torch_both},
                  a.window, a.chunk)
    for k, r in res.items():
        lines.append({"what": "sample", "scene": f"teapot V={v.shape[0]} F={f.shape[0]}", "samples": SAMPLES, "variant": k, **r, "device": name})
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
