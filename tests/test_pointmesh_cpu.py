"""CPU tests of the point-against-mesh unit (reni_tu_pointmesh.hip; ops.nearest_faces, ops.faces_nearest_points;
mesh_losses.nearest_surface, point_mesh_distance, geometry_scores(surface=True)): the float64 reference of tests/pointmesh_ref.py
against an independent evaluation and against autograd, the cases, the error-budget constants, and everything of the new entry
points that holds without a GPU (declarations, argument checks, the workspace's bound, no CPU path, the unit's emitted code)."""
import ctypes
import os

import pytest
import torch

from tests import pointmesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reni_nearest_faces_workspace_bytes", "reni_nearest_faces", "reni_faces_nearest_points_workspace_bytes",
         "reni_faces_nearest_points")
KERNELS = ("k_pm_searchILb0", "k_pm_searchILb1", "k_pm_combineILb0", "k_pm_combineILb1")


# ---------------------------------------------------------------------------------------------------------- the reference
def _independent(p, a, b, c):
    """float64 squared distance from p to the triangle without the region form: the plane projection where it falls inside the
    triangle, else the smallest distance to the three edges' segments"""
    def segment(p, x, y):
        e = y - x
        t = ((p - x) * e).sum(-1) / (e * e).sum(-1).clamp_min(1e-300)
        q = x + t.clamp(0.0, 1.0)[:, None] * e
        return ((p - q) ** 2).sum(-1)

    d = torch.minimum(torch.minimum(segment(p, a, b), segment(p, b, c)), segment(p, c, a))
    n = torch.linalg.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    t = ((p - a) * n).sum(-1) / nn.clamp_min(1e-300)
    proj = p - t[:, None] * n
    inside = nn > 0
    for x, y in ((a, b), (b, c), (c, a)):  # the projection is on the inner side of every edge
        inside = inside & ((torch.linalg.cross(y - x, proj - x) * n).sum(-1) >= 0)
    return torch.where(inside, t * t * nn, d)


def _check_against_independent(points, verts, faces, pi, fi, label):
    row = R.pair_rows(points, verts, faces, pi, fi)
    a, b, c = (t.double()[fi] for t in R.corners(verts, faces))
    want = _independent(points.double()[pi], a, b, c)
    worst = float(((row["d"] - want).abs() / row["s"].clamp_min(1e-300)).max())
    print(f"{label}: worst |d_ref - d_independent| / s = {worst:.3g} over {pi.numel()} pairs")
    assert worst <= 1e-12
    assert (row["u"] >= 0).all() and (row["v"] >= 0).all() and (row["w"] >= 0).all()
    assert float((row["u"] + row["v"] + row["w"] - 1).abs().max()) <= 1e-15
    assert float((row["q"] - (row["u"][:, None] * a + row["v"][:, None] * b + row["w"][:, None] * c)).abs().max()) <= 1e-12 * float(row["s"].max() ** 0.5 + a.abs().max())


def test_reference_agrees_with_an_independent_evaluation():
    gen = torch.Generator().manual_seed(1)
    for key in R.SEARCH_CASES:
        p, v, f = R.search_inputs(key)
        ref = R.search_of(key)
        keep = ref["idx"] >= 0
        qi = torch.arange(ref["idx"].numel())[keep]
        pi, fi = (ref["idx"][keep], qi) if key[1] == "fp" else (qi, ref["idx"][keep])
        _check_against_independent(p, v, f, pi, fi, R.case_id(key) + " matches")
        n = min(2000, p.shape[0] * f.shape[0])  # and pairs that are no matches: every region far from the triangle too
        _check_against_independent(p, v, f, torch.randint(0, p.shape[0], (n,), generator=gen), torch.randint(0, f.shape[0], (n,), generator=gen),
                                   R.case_id(key) + " random pairs")
    for name in R.PMD_CASES:
        p, v, f = R.pmd_inputs(name)
        part = torch.nonzero(R.take_part(f, v.shape[0]))[:, 0]
        pi = torch.randint(0, p.shape[0], (3000,), generator=gen)
        fi = part[torch.randint(0, part.numel(), (3000,), generator=gen)]
        area2 = R.pair_rows(p, v, f, pi, fi)["cross2"]
        ok = area2 > 1e-12  # (the collinear face of "bad_faces": its weights are noise over noise, its point still of the triangle)
        _check_against_independent(p, v, f, pi[ok], fi[ok], name)
    p, v, f = R.region_case()
    _check_against_independent(p, v, f, torch.arange(p.shape[0]), torch.zeros(p.shape[0], dtype=torch.int64), "regions")


def test_reference_gradients_match_autograd():
    """the closed form against autograd through the same expression, the weights and matches constant"""
    for name in ("ico1", "bad_faces", "star320"):
        p, v, f = R.pmd_inputs(name)
        for weights in R.WEIGHTS:
            ref = R.pmd_of(name, weights)
            bary = R.own_bary(p, v, f, ref["matches"])
            P, X = p.double().requires_grad_(True), v.double().requires_grad_(True)
            L = torch.zeros((), dtype=R.F64)
            for wt, pi, fi, w in ((weights[0], torch.arange(p.shape[0]), ref["matches"][0], bary[0]),
                                  (weights[1], ref["matches"][1], torch.arange(f.shape[0]), bary[1])):
                keep = (pi >= 0) & (fi >= 0)
                if wt > 0 and keep.any():
                    q = (w[keep][:, :, None] * X[f[fi[keep]]]).sum(1)
                    L = L + wt * ((P[pi[keep]] - q) ** 2).sum(1).mean()
            if L.requires_grad:
                L.backward()
            gp, gv = (torch.zeros_like(t) if t.grad is None else t.grad for t in (P, X))
            assert abs(float(L.detach() - ref["value"])) <= 1e-12 * max(float(ref["value"]), 1e-300)
            assert R.M.error_ratio(gp, ref["gp"], ref["gp_terms"]) < 1e-6 and R.M.error_ratio(gv, ref["gv"], ref["gv_terms"]) < 1e-6
            if weights == (0.0, 0.0):
                assert float(ref["value"]) == 0.0 and (ref["gp"] == 0).all() and (ref["gv"] == 0).all()
    ref = R.pmd_of("on_vertices")
    assert float(ref["value"]) == 0.0 and (ref["gp"] == 0).all() and (ref["gv"] == 0).all()  # points on vertices: distance 0


def test_the_cases_are_what_they_claim():
    shapes = {(k[2], k[3]) for k in R.SEARCH_CASES if k[0] == "big"}
    for want in ((1, 1), (1, R.TILE * 4 + 1), (R.QUERIES * 8 + 1, 1), (300, R.TILE - 1), (300, R.TILE), (300, R.TILE + 1),
                 (R.QUERIES - 1, 700), (R.QUERIES, 700), (R.QUERIES + 1, 700), (64, 20000)):
        assert want in shapes
    assert {k[1] for k in R.SEARCH_CASES} == {"pf", "fp"} and {k[4] for k in R.SEARCH_CASES} == {1e-3, 1.0, 1e3}
    assert {k[0] for k in R.SEARCH_CASES} == {"big", "small", "near", "ico"}
    for key in R.SEARCH_CASES:
        ref = R.search_of(key)
        assert (ref["idx"] >= 0).all() and torch.isfinite(ref["d"]).all(), key
    # the grid lands in every region on both sides of the plane
    p, v, f = R.region_case()
    ref = R.nearest_faces(p, v, f)
    for side in (p[:, 2] > 0, p[:, 2] < 0):
        assert sorted(set(ref["region"][side].tolist())) == list(range(7))
    # exact ties: both faces of the split square give every tie point the same float32 bits, exactly the float64 value
    p = R.tie_points()
    for swapped in (False, True):
        f = R.tie_faces(swapped)
        rows = [R.pair_rows(p, R.SQUARE, f, torch.arange(12), torch.full((12,), k), R.F32)["d"] for k in (0, 1)]
        exact = R.pair_rows(p, R.SQUARE, f, torch.arange(12), torch.zeros(12, dtype=torch.int64))["d"]
        assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0].double(), exact)
        assert (R.nearest_faces(p, R.SQUARE, f)["idx"] == 0).all()
    # the stars: every face is nearest to point 0
    for name, F in (("star80", 80), ("star320", 320)):
        ref = R.pmd_of(name)
        assert (ref["matches"][1] == 0).all() and ref["matches"][1].numel() == F and (F > R.SHORT) == (name == "star320")
    # points on vertices: exactly 0 in the float32 evaluation too (some face has the vertex as its corner a, or b - a is exact)
    p, v, f = R.pmd_inputs("on_vertices")
    assert (R.nearest_faces(p, v, f, R.F32)["d"] == 0).all() and (R.faces_nearest_points(p, v, f, R.F32)["d"] == 0).all()
    # the regions' grid against the unit triangle is exact in float32
    p, v, f = R.region_case()
    assert torch.equal(R.nearest_faces(p, v, f, R.F32)["d"], R.nearest_faces(p, v, f)["d"])
    p, v, f = R.pmd_inputs("bad_faces")
    assert int((~R.take_part(f, v.shape[0])).sum()) == 4 and (R.pmd_of("bad_faces")["matches"][1] < 0).sum() == 4
    v, f = R.degenerate_mesh()
    assert R.take_part(f, v.shape[0]).all()
    a, b, c = (t.double() for t in R.corners(v, f))
    area2 = (torch.linalg.cross(b - a, c - a) ** 2).sum(1)
    assert (area2[8:20] == 0).all() and (area2[:8] > 0).all() and float(area2[:8].max()) < 1e-10 and (area2[20:] > 1e-3).all()


def test_error_budget_constants_are_the_measured_ones():
    """K = 4 x the worst ratio of the float32 CPU evaluation, hard-coded in the case file: still what is measured."""
    rd, rw, rv, rp, rg = R.float32_ratios()
    print(f"float32 CPU evaluation, worst ratios: dist2 / (2^-23 s) {rd:.4g}, weights / (2^-23 s^2 / |ab x ac|^2) {rw:.4g}; "
          f"point_mesh_distance / (2^-23 sum |terms|): value {rv:.4g}, points.grad {rp:.4g}, verts.grad {rg:.4g}")
    for k, r in ((R.K_D, rd), (R.K_W, rw), (R.K_VALUE, rv), (R.K_GP, rp), (R.K_GV, rg)):
        assert k / 2 <= 4 * r <= k * 1.001, (k, r)


# ----------------------------------------------------------------------------------------------------------- entry points
def test_header_integration_build_and_binding_name_the_entry_points():
    from reni_amd import _lib
    h = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name in NAMES:
        assert name + "(" in h and name in _lib.EXPORTS and name in doc and hasattr(lib, name)
    build = open(os.path.join(ROOT, "reni_amd", "csrc", "build.sh")).read()
    isa = open(os.path.join(ROOT, "reni_amd", "csrc", "isa_core.sh")).read()
    assert " pointmesh " in build and "_build/pointmesh.o" in build and " pointmesh " in isa
    for word in ("points against a mesh", "fmaf(d1, d4, -(d3 * d2))", "the FIRST of these regions", "(va + vb) + vc", "LOWEST f",
                 "LOWEST i", "lexicographic", "never N x F", "TAKES PART", "2^31 - 257", "fmaf(w, ac, fmaf(v, ab, a))"):
        assert word in h, word
    src = open(os.path.join(ROOT, "reni_amd", "csrc", "reni_tu_pointmesh.hip")).read()
    assert f"PM_TILE = {R.TILE};" in src and "PM_Q = 2;" in src and "PM_BLOCK = 256;" in src and R.QUERIES == 512


def test_cpu_tensors_raise():
    from reni_amd import _lib, mesh_losses, ops
    from reni_amd.mesh import ico_sphere
    m = ico_sphere(0)
    p = torch.rand(5, 3)
    calls = (lambda: ops.nearest_faces(p, m.verts_packed(), m.faces_packed()),
             lambda: ops.faces_nearest_points(p, m.verts_packed(), m.faces_packed()),
             lambda: mesh_losses.nearest_surface(p, m), lambda: mesh_losses.point_mesh_distance(p, m),
             lambda: mesh_losses.point_mesh_distance(p, m, weights=(0.0, 0.0)),
             lambda: mesh_losses.geometry_scores(m, m, n=4, surface=True))
    for call in calls:
        with pytest.raises(_lib.RENILibraryError):
            call()


def test_bad_arguments_raise_value_errors_before_the_device_check():
    from reni_amd import mesh_losses, ops
    from reni_amd.mesh import ico_sphere
    m = ico_sphere(0)
    v, f, p = m.verts_packed(), m.faces_packed(), torch.rand(5, 3)
    bad = (lambda: ops.nearest_faces(torch.rand(5, 2), v, f), lambda: ops.nearest_faces(torch.rand(0, 3), v, f),
           lambda: ops.nearest_faces([1.0, 2.0, 3.0], v, f), lambda: ops.nearest_faces(p, v, f, slices=-1),
           lambda: ops.nearest_faces(p, v[:, :2], f), lambda: ops.nearest_faces(p, v, f[:0]),
           lambda: ops.faces_nearest_points(p, v, f, slices=-1), lambda: ops.faces_nearest_points(torch.rand(5), v, f),
           lambda: mesh_losses.point_mesh_distance(torch.rand(5), m), lambda: mesh_losses.point_mesh_distance(p, m, weights=(-1.0, 1.0)),
           lambda: mesh_losses.point_mesh_distance(p, m, weights=(1.0, float("nan"))),
           lambda: mesh_losses.point_mesh_distance(p, m, weights=(float("inf"), 1.0)),
           lambda: mesh_losses.point_mesh_distance(p, m, weights=(1.0,)))
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} did not raise")


def test_wrappers_behind_the_device_check(monkeypatch):
    """with the device check and the launch taken out: what reaches the library"""
    from reni_amd import _lib, ops
    from reni_amd.mesh import ico_sphere
    lib = _lib.load()
    seen = []
    monkeypatch.setattr(ops, "_require_cuda", lambda *t: None)
    monkeypatch.setattr(ops, "_call", lambda fn, device, *args: seen.append((fn, args)))
    m = ico_sphere(1)
    v, f, p = m.verts_packed(), m.faces_packed(), torch.rand(600, 3)
    for fn_py, fn_c, n in ((ops.nearest_faces, lib.reni_nearest_faces, 600), (ops.faces_nearest_points, lib.reni_faces_nearest_points, 80)):
        d, i, ti, tw = fn_py(p.double(), v, f.int(), slices=3)  # (casts: float32 points, int64 faces)
        fn, a = seen.pop()
        assert fn is fn_c and a[:3] == (600, 42, 80) and a[6] == 3 and a[4] == v.data_ptr()
        assert a[7:11] == (d.data_ptr(), i.data_ptr(), ti.data_ptr(), tw.data_ptr()) and a[9] % 16 == 0 and a[10] % 16 == 0
        need = getattr(lib, fn_c.__name__ + "_workspace_bytes")(600, 42, 80)
        assert a[11] % 256 == 0 and a[12] >= need > 0  # aligned by the wrapper
        assert (d.dtype, i.dtype, ti.dtype, tw.dtype) == (torch.float32, torch.int64, torch.int32, torch.float32)
        assert tuple(d.shape) == (n,) == tuple(i.shape) and tuple(ti.shape) == (n, 8) == tuple(tw.shape)
    assert not seen


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Argument checks run before any device work, so they hold without a GPU."""
    from reni_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(3 * 2 ** 20)
    p = (ctypes.addressof(buf) + 255) & ~255
    big = 2 ** 31 - 256
    for name, who in (("reni_nearest_faces", b"nearest faces:"), ("reni_faces_nearest_points", b"faces nearest points:")):
        fn, wsb = getattr(lib, name), getattr(lib, name + "_workspace_bytes")

        def call(N=4, V=4, F=4, pts=p, v=p, f=p, slices=0, d=p, i=p, ti=p, tw=p, wsp=p, wsn=2 ** 21 + 1024):
            return fn(N, V, F, pts, v, f, slices, d, i, ti, tw, wsp, wsn, None)

        for kw in (dict(N=0), dict(V=0), dict(F=0), dict(N=-1), dict(N=big), dict(F=big), dict(V=2 ** 30), dict(slices=-1), dict(pts=None),
                   dict(v=None), dict(f=None), dict(d=None), dict(i=None), dict(ti=None), dict(tw=None), dict(ti=p + 8), dict(tw=p + 4)):
            assert call(**kw) == -1 and lib.reni_last_error().startswith(who), kw
        assert b"16-byte" in (call(tw=p + 4), lib.reni_last_error())[1] and b"slices" in (call(slices=-1), lib.reni_last_error())[1]
        assert b"2^31 - 257" in (call(N=big), lib.reni_last_error())[1] and b"NULL" in (call(v=None), lib.reni_last_error())[1]
        need = wsb(4, 4, 4)
        assert call(wsp=None, wsn=0) == -2 and call(wsn=need - 1) == -2 and call(wsp=p + 8) == -2  # RENI_EWORKSPACE
        assert lib.reni_last_error().startswith(who) and b"workspace" in lib.reni_last_error()
        assert wsb(0, 4, 4) == 0 and wsb(4, 0, 4) == 0 and wsb(4, 4, 0) == 0 and wsb(big, 4, 4) == 0 and wsb(4, 4, big) == 0
        assert wsb(4, 2 ** 30, 4) == 0 and wsb(big - 1, 2 ** 30 - 1, big - 1) > 0


def test_search_workspace_is_bounded_and_independent_of_the_targets():
    from reni_amd import _lib
    lib = _lib.load()
    counts = (1, 64, 511, 512, 513, 5000, 20000, 100000, 10 ** 6, 10 ** 8)
    for Q in counts:
        by_point = {lib.reni_nearest_faces_workspace_bytes(Q, V, T) for T in (1, 1000, 81920, 10 ** 9) for V in (3, 10 ** 6)}
        by_face = {lib.reni_faces_nearest_points_workspace_bytes(T, V, Q) for T in (1, 1000, 81920, 10 ** 9) for V in (3, 10 ** 6)}
        assert len(by_point) == 1 and by_point == by_face, Q  # the queries alone decide
        need = by_point.pop()
        assert 0 < need <= 8 * 512 * Q + 768 and need <= 2 * 2 ** 20 + 768  # at most 512 slices of two 4-byte partials per query


# -------------------------------------------------------------------------------------------------------------- the build
def test_pointmesh_unit_has_no_float_atomics_and_launches_through_the_host_path():
    src = open(os.path.join(ROOT, "reni_amd", "csrc", "reni_tu_pointmesh.hip")).read()
    assert "atomic" not in src.replace("no float atomic", "")
    assert "hipDeviceSynchronize" not in src and "hipStreamSynchronize" not in src and "hipMemcpy" not in src
    assert '#include "reni_tu_host.inc"' in src and "hipLaunchKernelGGL" not in src and "<<<" not in src
    assert src.count("tu_launch(TU_COUNTED") == 2 and "TU_PLAIN" not in src
    assert "#pragma clang fp contract(off)" in src


def test_pointmesh_translation_unit_isa_audit():
    """reni_tu_pointmesh.hip with build.sh's flags: it compiles; no MFMA / transcendental / SDWA hazard, no scratch; the targets
    come from LDS in 16-byte reads."""
    import re
    import subprocess
    import tempfile
    from tests import isa_audit
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "pointmesh.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_pointmesh.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    for k in KERNELS:
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text and "atomic" not in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) >= len(KERNELS) and all(int(n) == 0 for n in sizes)  # one per kernel
    for inst in ("k_pm_searchILb0", "k_pm_searchILb1"):
        start = text.index("_ZN4reni11" + inst)
        body = text[start:text.index("s_endpgm", start)]
        # 16-byte records, written whole; the fourth word is padding, so the compiler reads the three it uses (ds_read_b96)
        assert ("ds_read_b128" in body or "ds_read_b96" in body) and "ds_write_b128" in body, inst
        assert not re.search(r"ds_read_b(32|64)\b", body) and "ds_read2" not in body, inst
    assert "v_mfma" not in text
