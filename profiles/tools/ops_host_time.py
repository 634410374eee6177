"""Host time of the wrappers in ``reni_amd.ops``: what a launch-bound call pays per call, at tests/test_gpu_launch_counts.py's
shapes (2 maps of 8 x 16, 64 directions, a four-face mesh at 16 x 16).  Toy shapes are the point: the kernels take a few
microseconds, so the time of a call is the wrapper's checks, casts, allocations and the launches.

Six wrappers, two of them from the shader family: envmap_shade_terms, envmap_shade_ggx, soft_silhouette_backward,
gbuffer_backward (both with the lists the caller keeps), envmap_lookup, pair_stats.  Each round times `--chunk` calls with the
host clock, ending in a device synchronise; the figure of a wrapper is the median round, in microseconds per call.

    ops_host_time.py                         one run of the package beside this file
    ops_host_time.py --package DIR           one run of DIR/reni_amd (Python only: RENI_HIP_LIB names the library to load)
    ops_host_time.py --compare DIR --out F   DIR/reni_amd against this tree's, both on this tree's library: four fresh child
                                             processes, DIR, here, DIR, here; appends one JSON line per wrapper to F

The comparison's bound is not fixed in advance: a wrapper passes when the median of this tree's rounds exceeds the median of
DIR's rounds by no more than the distance between the medians of DIR's own two runs."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, H, W, P, S = 2, 8, 16, 64, 16


def measure(package, chunk, rounds):
    sys.path.insert(0, package)
    import torch
    from reni_amd import ops
    assert os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__))) == os.path.abspath(package), ops.__file__
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)

    def unit(*shape):
        return torch.nn.functional.normalize(torch.randn(*shape, 3, generator=g), dim=-1).to(dev)

    verts = torch.tensor([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]).to(dev) * 0.5
    faces = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=torch.int64).to(dev)
    R, T, tan = torch.eye(3), torch.tensor([0.0, 0.0, 3.0]), 0.5773502691896258
    vn = ops.vertex_normals(verts, faces)
    p2f, _, _, _, pnrm, ppos = ops.rasterize_mesh(verts, faces, vn, R, T, S)
    vf, table = ops.vertex_face_lists(faces, 4), ops.face_pixel_table(p2f, 4)
    _, trans = ops.soft_silhouette(verts, faces, R, T, S, tan, 1e-2, 1e-3)
    galpha, gN, gX = (torch.rand(*s, generator=g).to(dev) for s in ((S * S,), (S * S, 3), (S * S, 3)))
    sdirs, colors, cam = unit(P), torch.rand(B, P, 3, generator=g).to(dev), torch.tensor([0.0, 0.0, 3.0])
    maps, out_dirs = torch.rand(B, H, W, 3, generator=g).to(dev), unit(P)
    pred, target = torch.rand(B, 3, H, W, generator=g).to(dev), torch.rand(B, 3, H, W, generator=g).to(dev)
    calls = {
        "envmap_shade_terms": lambda: ops.envmap_shade_terms(pnrm, ppos, cam, sdirs, colors, 50.0),
        "envmap_shade_ggx": lambda: ops.envmap_shade_ggx(pnrm, ppos, cam, sdirs, colors, 0.25),
        "soft_silhouette_backward": lambda: ops.soft_silhouette_backward(verts, faces, R, T, S, tan, 1e-2, 1e-3, trans, galpha, vf=vf),
        "gbuffer_backward": lambda: ops.gbuffer_backward(verts, faces, vn, R, T, S, p2f, gN, gX, table=table, vf=vf),
        "envmap_lookup": lambda: ops.envmap_lookup(maps, out_dirs),
        "pair_stats": lambda: ops.pair_stats(pred, target),
    }
    for fn in calls.values():
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):  # the wrappers take turns round by round: clock and machine drift hit all of them alike
        for k, fn in calls.items():
            t0 = time.perf_counter()
            for _ in range(chunk):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / chunk * 1e6)
    return {"package": os.path.abspath(package), "chunk": chunk, "device": torch.cuda.get_device_name(0), "us_rounds": times}


def compare(parent, chunk, rounds, out):
    env = dict(os.environ, RENI_HIP_LIB=os.environ.get("RENI_HIP_LIB") or os.path.join(ROOT, "reni_amd", "lib", "libreni_hip.so"))
    runs = []
    for label, package in (("parent", parent), ("new", ROOT)) * 2:
        # a fresh process per run; a run that fails ends the comparison (nothing more is started on the device)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--package", package, "--chunk", str(chunk), "--rounds", str(rounds),
                            "--json"], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"the {label} run ended with status {r.returncode}")
        runs.append((label, json.loads(r.stdout.strip().splitlines()[-1])))
    lines, ok = [], True
    for k in runs[0][1]["us_rounds"]:
        per_run = [(label, r["us_rounds"][k]) for label, r in runs]
        med = [round(statistics.median(t), 2) for _, t in per_run]
        parent_us = statistics.median(per_run[0][1] + per_run[2][1])
        new_us = statistics.median(per_run[1][1] + per_run[3][1])
        spread = abs(med[0] - med[2])
        within = new_us - parent_us <= spread
        ok = ok and within
        lines.append({"wrapper": k, "us_parent": round(parent_us, 2), "us_new": round(new_us, 2), "us_runs_parent_new_parent_new": med,
                      "us_parent_spread": round(spread, 2), "within_spread": within, "calls_per_run": chunk * rounds,
                      "shapes": f"B={B} {H}x{W} P={P} mesh 4 faces at {S}x{S}", "device": runs[0][1]["device"]})
    for line in lines:
        print(json.dumps(line))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=ROOT, help="the directory that holds the reni_amd package to time")
    ap.add_argument("--compare", default=None, metavar="DIR", help="time DIR/reni_amd against this tree's, alternating fresh processes")
    ap.add_argument("--chunk", type=int, default=200, help="calls per round")
    ap.add_argument("--rounds", type=int, default=15, help="rounds per wrapper and run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", action="store_true", help="print the run's rounds as one JSON line (what --compare reads)")
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(0 if compare(a.compare, a.chunk, a.rounds, a.out) else 1)
    r = measure(a.package, a.chunk, a.rounds)
    if a.json:
        print(json.dumps(r))
    else:
        for k, t in r["us_rounds"].items():
            print(f"{k:28s} {statistics.median(t):8.2f} us per call (median of {len(t)} rounds of {a.chunk}; {min(t):.2f} .. {max(t):.2f})")


if __name__ == "__main__":
    main()
