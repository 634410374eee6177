"""Cast shadows at FIT_INVERSE's shapes: the teapot at 128 x 128 pixels, a 64 x 128 grid, batch 3.  Calls timed
with CUDA events after warm-up, one JSON line per row (kept in profiles/visibility_time.jsonl).

  prepare   the acceleration record (Morton sort on the torch side + reni_mesh_visibility_prepare)
  pass      the visibility pass, culled and RENI_VIS_NO_CULL, alternated call by call in the same process (the median of each)
  shader    the masked shader forward and backward, alternated with the unmasked shader the same way
  lights    the visibility pass for per-image lists of 1 024 lights (batch 3)
  stats     not a timing: clusters a wave enters out of those it could, counted on the host from the float64 restatement on
            the 32 x 32 teapot with the 8 x 16 grid (tests/visibility_ref.py) -- the ballot statistics of the culled pass

`--only NAME` runs one row family."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from reni_amd import ops  # noqa: E402

TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")


def row(**kw):
    print(json.dumps(kw))
    sys.stdout.flush()


def alternated(fa, fb, warmup=2, rounds=10):
    """a, b, a, b, ... each call between its own pair of events -> (median us of a, median us of b, their spreads)."""
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        for fn, acc in ((fa, ta), (fb, tb)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record()
            torch.cuda.synchronize()
            acc.append(s.elapsed_time(e) * 1e3)
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


def scene(S=128, W=128):
    from reni_amd.mesh import build_hip_renderer
    from reni_amd.utils import get_directions
    renderer, R, T, mesh = build_hip_renderer(TEAPOT, 0, S, 0.5, "cuda", shadows=True)
    frag, nrm, pos = renderer.rasterizer.gbuffer(mesh, R, T)
    D = get_directions(W)[0].cuda().contiguous()
    v, f = mesh.verts_packed(), mesh.faces_packed()
    diag = float((v.max(0).values - v.min(0).values).norm())
    return renderer, v, f, frag.pix_to_face, nrm, pos, D, 1e-4 * diag


def prepare_rows(rounds):
    _, v, f, *_ = scene()
    a, b, sa, _ = alternated(lambda: ops.mesh_visibility_prepare(v, f), lambda: None, rounds=rounds)
    order = ops._morton_order(v, f)
    c, _, sc, _ = alternated(lambda: ops.mesh_visibility_prepare(v, f, order=order), lambda: None, rounds=rounds)
    row(call="prepare, teapot", faces=int(f.shape[0]), clusters=(int(f.shape[0]) + 63) // 64, with_morton_sort_us=round(a, 1),
        kernel_only_us=round(c, 1), spread_us=[round(x, 1) for x in sa + sc])


def pass_rows(rounds):
    _, v, f, p2f, nrm, pos, D, t_min = scene()
    accel = ops.mesh_visibility_prepare(v, f)
    a, b, sa, sb = alternated(lambda: ops.mesh_visibility(pos, p2f, D, accel, t_min),
                              lambda: ops.mesh_visibility(pos, p2f, D, accel, t_min, no_cull=True), warmup=1, rounds=rounds)
    fg = int((p2f >= 0).sum())
    assert torch.equal(ops.mesh_visibility(pos, p2f, D, accel, t_min), ops.mesh_visibility(pos, p2f, D, accel, t_min, no_cull=True))
    row(call="visibility pass, teapot 128x128 x 64x128 grid", pixels=int(pos.shape[0]), foreground=fg, directions=int(D.shape[0]),
        faces=int(f.shape[0]), ray_face_tests_brute_force=fg * int(D.shape[0]) * ((int(f.shape[0]) + 63) // 64) * 64,
        culled_us=round(a, 1), no_cull_us=round(b, 1), culled_over_brute_force=round(a / b, 4),
        culled_spread_us=[round(x, 1) for x in sa], no_cull_spread_us=[round(x, 1) for x in sb])


def shader_rows(rounds):
    renderer, v, f, p2f, nrm, pos, D, t_min = scene()
    vis = ops.mesh_visibility(pos, p2f, D, ops.mesh_visibility_prepare(v, f), t_min)
    g = torch.Generator().manual_seed(0)
    C = torch.rand(3, D.shape[0], 3, generator=g).cuda()
    dcol = torch.randn(3, pos.shape[0], 3, generator=g).cuda()
    cam = renderer.camera_center
    for name, fn, src in (("forward", ops.envmap_shade, C), ("backward", ops.envmap_shade_backward, dcol)):
        a, b, sa, sb = alternated(lambda: fn(nrm, pos, cam, D, src, 500.0, 0.5, 0.5, vis=vis),
                                  lambda: fn(nrm, pos, cam, D, src, 500.0, 0.5, 0.5), rounds=rounds)
        row(call=f"shader {name}, 3 x 128x128 from a 64x128 map", masked_us=round(a, 1), unmasked_us=round(b, 1),
            masked_over_unmasked=round(a / b, 4), masked_spread_us=[round(x, 1) for x in sa],
            unmasked_spread_us=[round(x, 1) for x in sb])


def light_rows(rounds):
    _, v, f, p2f, nrm, pos, D, t_min = scene()
    accel = ops.mesh_visibility_prepare(v, f)
    g = torch.Generator().manual_seed(1)
    dirs = torch.nn.functional.normalize(torch.randn(3, 1024, 3, generator=g), dim=-1).cuda()
    a, b, sa, sb = alternated(lambda: ops.mesh_visibility(pos, p2f, dirs, accel, t_min),
                              lambda: ops.mesh_visibility(pos, p2f, dirs, accel, t_min, no_cull=True), warmup=1, rounds=rounds)
    row(call="visibility pass, teapot 128x128, per-image lists of 1024 lights, batch 3", culled_us=round(a, 1),
        no_cull_us=round(b, 1), culled_over_brute_force=round(a / b, 4), culled_spread_us=[round(x, 1) for x in sa])


def stats_rows():
    """What the culled kernel's ballots do, restated on the host in float64: per wave (one pixel x 64 consecutive directions)
    the clusters whose box some still-unoccluded ray touches, walking the clusters in the record's order."""
    from tests import visibility_ref as VR
    sc = VR.teapot_scene()
    verts, faces = sc["verts"].astype(np.float64), sc["faces"]
    order = ops._morton_order(torch.from_numpy(sc["verts"]), torch.from_numpy(faces)).numpy()
    F = len(faces)
    NC = (F + 63) // 64
    fg = np.flatnonzero(sc["own"] >= 0)
    dirs = sc["dirs"].astype(np.float64)
    entered = possible = 0
    occluded_exit = 0
    for p in fg:
        o = sc["origins"][p].astype(np.float64)
        for j0 in range(0, len(dirs), 64):
            d = dirs[j0:j0 + 64]
            occ = np.zeros(len(d), bool)
            for c in range(NC):
                possible += 1
                if occ.all():
                    occluded_exit += 1
                    continue
                ids = order[c * 64:(c + 1) * 64]
                tri = verts[faces[ids]]
                lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
                m = max(float((hi - lo).max()), float(np.abs(np.concatenate([lo, hi])).max())) / 1024.0
                with np.errstate(divide="ignore", invalid="ignore"):
                    t0, t1 = (lo - m - o) / d, (hi + m - o) / d
                tn, tf = np.nanmax(np.minimum(t0, t1), axis=1), np.nanmin(np.maximum(t0, t1), axis=1)
                touch = (tf >= 0) & (tf >= tn) & ~occ
                if not touch.any():
                    continue
                entered += 1
                own = np.flatnonzero(ids == sc["own"][p])  # the pixel's own face, if this cluster holds it
                o_, _ = VR.visibility_ref(o[None], [int(own[0]) if len(own) else len(ids)], d, sc["verts"], faces[ids], sc["t_min"])
                occ |= o_[0]
    row(call="ballot statistics, teapot 32x32 x 8x16 grid (host, float64)", waves=possible // NC, clusters=NC,
        clusters_entered_share=round(entered / possible, 4), skipped_because_all_occluded_share=round(occluded_exit / possible, 4),
        skipped_by_the_box_test_share=round(1 - (entered + occluded_exit) / possible, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--rounds", type=int, default=10)
    a = ap.parse_args()
    if a.only in (None, "prepare"):
        prepare_rows(a.rounds)
    if a.only in (None, "pass"):
        pass_rows(min(a.rounds, 5))
    if a.only in (None, "shader"):
        shader_rows(a.rounds)
    if a.only in (None, "lights"):
        light_rows(min(a.rounds, 5))
    if a.only == "stats":
        stats_rows()


if __name__ == "__main__":
    main()
