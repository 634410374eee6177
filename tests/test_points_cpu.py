"""CPU tests of the point-cloud unit (reni_tu_points.hip; ops.nearest_points, chamfer_grad, mesh_sample_table,
mesh_sample_points; reni_amd/mesh_losses.py; mesh.ico_sphere): the float64 reference of tests/points_ref.py against central
differences and against autograd, the cases, the share of undecided elements, the error-budget constants, ico_sphere, and
everything of the new entry points that holds without a GPU (declarations, argument checks, the workspace's growth, no CPU
path, the unit's emitted code)."""
import ctypes
import os

import pytest
import torch

from tests import points_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reni_nearest_points_workspace_bytes", "reni_nearest_points", "reni_chamfer_grad",
         "reni_mesh_sample_table_workspace_bytes", "reni_mesh_sample_table", "reni_mesh_sample_points")
KERNELS = ("k_np_search", "k_np_combine", "k_ch_grad", "k_ps_area", "k_ps_chunks", "k_ps_cdf", "k_ps_sample")


# ---------------------------------------------------------------------------------------------------------- the reference
def test_reference_gradient_matches_central_differences():
    h = 1e-6
    ran = 0
    for name in ("cube", "r129", "spheres"):
        x, y = P.ch_clouds(name)
        for weights in ((1.0, 1.0), (0.3, 1.7), (1.0, 0.0)):
            ref = P.chamfer_of(name, weights)
            X, Y = x.to(P.F64), y.to(P.F64)
            gen = torch.Generator().manual_seed(3)
            for _ in range(2):
                dx = torch.randn(X.shape, generator=gen, dtype=P.F64)
                dy = torch.randn(Y.shape, generator=gen, dtype=P.F64)
                vals = []
                for s in (1.0, -1.0):  # the true objective: the matches are searched again at the moved points
                    D = P.dist_matrix(X + s * h * dx, Y + s * h * dy)
                    vals.append(float(weights[0] * D.min(1).values.mean() + weights[1] * D.min(0).values.mean()))
                fd = (vals[0] - vals[1]) / (2 * h)
                an = float((ref["gx"] * dx).sum() + (ref["gy"] * dy).sum())
                scale = float((ref["gx_terms"] * dx.abs()).sum() + (ref["gy_terms"] * dy.abs()).sum())
                assert abs(fd - an) <= 1e-6 * scale + 1e-12, (name, weights, fd, an)
                ran += 1
    assert ran == 18


def test_reference_closed_form_matches_autograd():
    for name in P.CH_CASES:
        x, y = P.ch_clouds(name)
        for weights in P.WEIGHTS:
            ref = P.chamfer_of(name, weights)
            L, gx, gy = P.chamfer_autograd(x, y, weights)
            assert abs(float(L - ref["value"])) <= 1e-12 * max(float(ref["value"]), 1e-300)
            assert P.M.error_ratio(gx, ref["gx"], ref["gx_terms"]) < 1e-6 and P.M.error_ratio(gy, ref["gy"], ref["gy_terms"]) < 1e-6
            assert (ref["gx_terms"] >= ref["gx"].abs() * (1 - 1e-9)).all() and (ref["gy_terms"] >= ref["gy"].abs() * (1 - 1e-9)).all()
    ref = P.chamfer_of("coincident")
    assert float(ref["value"]) == 0.0 and (ref["gx"] == 0).all() and (ref["gy"] == 0).all()
    for w in ((1.0, 0.0), (0.0, 1.0), (0.0, 0.0)):
        ref = P.chamfer_of("cube", w)
        if w == (0.0, 0.0):
            assert float(ref["value"]) == 0.0 and (ref["gx"] == 0).all() and (ref["gy"] == 0).all()


def test_the_cases_are_what_they_claim():
    assert P.longest_range("star") == 5000 and P.ch_clouds("star")[0].shape[0] == 300
    assert (P.nearest(*reversed(P.ch_clouds("star")))["idx"] == 0).all()  # every y nearest to x_0
    assert 65 <= P.longest_range("r100") <= P.SHORT and P.longest_range("r128") == P.SHORT and P.longest_range("r129") == P.SHORT + 1
    assert all(P.longest_range(n) <= 64 for n in ("cube", "uneven", "spheres", "coincident"))
    shapes = {(k[1], k[2]) for k in P.NN_CASES}
    for want in ((1, 1), (1, 4097), (4097, 1), (255, 257), (257, 255), (64, 20000), (1000, 4097)):
        assert want in shapes
    assert {m for _, m in shapes} >= {P.TILE - 1, P.TILE, P.TILE + 1} and {n for n, _ in shapes} >= {P.QUERIES - 1, P.QUERIES, P.QUERIES + 1}
    assert {k[3] for k in P.NN_CASES} == {1e-3, 1.0, 1e3} and {k[0] for k in P.NN_CASES} == {"cube", "spheres"}
    x, y = P.lattice()
    r = P.nearest(x, y)
    assert x.shape[0] == 729 and (r["d"] == 0.75).all()
    D = P.dist_matrix(x.double(), y.double())
    ties = (D == 0.75).sum(1)
    assert int(ties.max()) == 8 and int((ties == 8).sum()) == 512  # the 8^3 queries with a full cell round them
    a, part = P.areas(*P.sample_mesh(("two", 0)))
    assert a.tolist() == [1.0, 3.0]
    a, part = P.areas(*P.sample_mesh(("bad_faces", 16)))
    assert int((~part).sum()) == 4 and int((part & (a == 0)).sum()) == 1  # four faces take no part, one more is collinear
    u = P.sample_u()
    assert float(u.min()) == 0.0 and float(u.max()) < 1.0 and (u[:, 1] == 0).any() and float(u.max()) == 1.0 - 2.0 ** -24


def test_undecided_elements_stay_under_the_cap():
    worst = 0.0
    for key in P.NN_CASES:
        r = P.nearest_of(key)
        share = float(r["und"].float().mean())
        print(f"nearest {P.case_id(key)}: {int(r['und'].sum())} undecided of {r['und'].numel()} queries")
        assert share == 0.0, key  # the random cases have none
        worst = max(worst, share)
    for name in P.CH_CASES:
        for weights in P.WEIGHTS:
            ref = P.chamfer_of(name, weights)
            u, n = int(ref["und_x"].sum() + ref["und_y"].sum()), ref["und_x"].numel() + ref["und_y"].numel()
            if name != "coincident":  # (x is y there: d = 0 is decided exactly, d_second > 0)
                assert u == 0, (name, weights)
            assert u / n <= P.UNDECIDED_CAP, (name, weights, u, n)
    u = P.sample_u()
    up = P.sample_upstream(u.shape[0])
    for key in P.SAMPLE_MESHES:
        v, f = P.sample_mesh(key)
        s = P.sample(v, f, u, up)
        share = float(s["und"].float().mean())
        print(f"sampling {P.case_id(key)}: {int(s['und'].sum())} undecided of {u.shape[0]} samples ({100 * share:.2f} %)")
        assert share <= P.UNDECIDED_CAP, key
        assert (s["area"][s["face"]] > 0).all() and s["part"][s["face"]].all()  # the reference never names a face without area


def test_error_budget_constants_are_the_measured_ones():
    """K = 4 x the worst ratio of the float32 CPU evaluation, hard-coded in the case file: still what is measured."""
    rv, rg, rp, rq = P.float32_ratios()
    print(f"float32 CPU evaluation, worst error / (2^-23 sum |terms|): value {rv:.4g}, gradients {rg:.4g}, points {rp:.4g}, "
          f"vertex gradient {rq:.4g}")
    for k, r in ((P.K_VALUE, rv), (P.K_GRAD, rg), (P.K_POINTS, rp), (P.K_VGRAD, rq)):
        assert k / 2 <= 4 * r <= k * 1.001, (k, r)


# ------------------------------------------------------------------------------------------------------------- ico_sphere
def test_ico_sphere_counts_edges_and_radii():
    from reni_amd import ops
    from reni_amd.mesh import Meshes, ico_sphere
    for level in range(4):
        m = ico_sphere(level)
        assert isinstance(m, Meshes)
        v, f = m.verts_packed(), m.faces_packed()
        V, F = 10 * 4 ** level + 2, 20 * 4 ** level
        assert tuple(v.shape) == (V, 3) and tuple(f.shape) == (F, 3) and v.dtype == torch.float32 and f.dtype == torch.int64
        L = ops.mesh_edge_lists(f, V)
        assert L["E"] == 30 * 4 ** level and V - L["E"] + F == 2
        mult = L["ef_offsets"][1:] - L["ef_offsets"][:-1]
        assert (mult == 2).all()  # a closed surface: every edge on exactly two faces
        assert float((v.double().norm(dim=1) - 1).abs().max()) <= 1e-6
        tri = v.double()[f]
        n = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
        assert ((n * tri.mean(1)).sum(1) > 0).all()  # outward winding
        assert torch.unique(f).numel() == V
    with pytest.raises(ValueError):
        ico_sphere(-1)


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
    assert " points " in build and "_build/points.o" in build and " points " in isa
    for word in ("fmaf(dz, dz, fmaf(dy, dy, dx * dx))", "LOWEST j", "lexicographic", "never N x M", "CONSTANTS of the gradient",
                 "r (1 - u2)", "never chosen", "TAKE PART", "2^31 - 1025"):
        assert word in h, word


def test_cpu_tensors_raise():
    from reni_amd import _lib, mesh_losses, ops
    from reni_amd.mesh import ico_sphere
    x, y = torch.rand(5, 3), torch.rand(7, 3)
    m = ico_sphere(0)
    calls = (lambda: ops.nearest_points(x, y), lambda: mesh_losses.nearest_points(x, y), lambda: mesh_losses.chamfer_distance(x, y),
             lambda: ops.chamfer_grad(x, y, torch.zeros(5, dtype=torch.int64), ops.chamfer_table(torch.zeros(7, dtype=torch.int64), 5)),
             lambda: ops.mesh_sample_table(m.verts_packed(), m.faces_packed()),
             lambda: ops.mesh_sample_points(m.faces_packed(), torch.zeros(2, 20), torch.rand(4, 3), 12),
             lambda: mesh_losses.sample_points_from_meshes(m, 4), lambda: mesh_losses.sample_points_from_meshes(m, 4, u=torch.rand(4, 3)),
             lambda: mesh_losses.geometry_scores(m, m, n=4))
    for call in calls:
        with pytest.raises(_lib.RENILibraryError):
            call()


def test_bad_arguments_raise_value_errors_before_the_device_check():
    from reni_amd import mesh_losses, ops
    from reni_amd.mesh import ico_sphere
    x, y = torch.rand(5, 3), torch.rand(7, 3)
    i5, t75 = torch.zeros(5, dtype=torch.int64), ops.chamfer_table(torch.zeros(7, dtype=torch.int64), 5)
    m = ico_sphere(0)
    bad = (lambda: ops.nearest_points(torch.rand(5, 2), y), lambda: ops.nearest_points(x, torch.rand(0, 3)),
           lambda: ops.nearest_points(x, [1.0, 2.0, 3.0]), lambda: ops.nearest_points(x, y, slices=-1),
           lambda: mesh_losses.chamfer_distance(torch.rand(5), y), lambda: mesh_losses.chamfer_distance(x, y, weights=(-1.0, 1.0)),
           lambda: mesh_losses.chamfer_distance(x, y, weights=(1.0, float("nan"))),
           lambda: mesh_losses.chamfer_distance(x, y, weights=(float("inf"), 1.0)), lambda: mesh_losses.chamfer_distance(x, y, weights=(1.0,)),
           lambda: ops.chamfer_grad(x, y, i5, t75, weights=(-1.0, 1.0)), lambda: ops.chamfer_grad(x, y, i5[:4], t75),
           lambda: ops.chamfer_grad(x, y, i5.int(), t75), lambda: ops.chamfer_grad(x, y, i5, (t75[0], t75[1][:-1])),
           lambda: ops.chamfer_grad(x, y, i5, None), lambda: ops.chamfer_table(torch.zeros(7), 5),
           lambda: ops.chamfer_table(torch.zeros(7, dtype=torch.int64), 0),
           lambda: ops.mesh_sample_table(torch.rand(4, 2), m.faces_packed()),
           lambda: ops.mesh_sample_points(m.faces_packed(), torch.zeros(2, 19), torch.rand(4, 3), 12),
           lambda: ops.mesh_sample_points(m.faces_packed(), torch.zeros(2, 20), torch.rand(4, 2), 12),
           lambda: ops.mesh_sample_points(m.faces_packed(), torch.zeros(2, 20), torch.rand(4, 3), 0),
           lambda: mesh_losses.sample_points_from_meshes(m, 0), lambda: mesh_losses.sample_points_from_meshes(m, 4, u=torch.rand(5, 3)))
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} did not raise")
    # a weight of 0 needs no list
    with pytest.raises(Exception) as e:
        ops.chamfer_grad(x, y, None, None, weights=(0.0, 0.0))
    assert not isinstance(e.value, ValueError)  # (the device check, not an argument error)


def test_wrappers_behind_the_device_check(monkeypatch):
    """with the device check and the launch taken out: what reaches the library, and the errors raised behind the check"""
    from reni_amd import _lib, ops
    from reni_amd.mesh import ico_sphere
    lib = _lib.load()
    seen = []
    monkeypatch.setattr(ops, "_require_cuda", lambda *t: None)
    monkeypatch.setattr(ops, "_call", lambda fn, device, *args: seen.append((fn, args)))
    x, y = torch.rand(600, 3), torch.rand(7, 3)
    d, i = ops.nearest_points(x.double(), y, slices=3)
    fn, a = seen.pop()
    assert fn is lib.reni_nearest_points and a[:2] == (600, 7) and a[4] == 3 and a[5] == d.data_ptr() and a[6] == i.data_ptr()
    assert a[7] % 256 == 0 and a[8] >= lib.reni_nearest_points_workspace_bytes(600, 7) > 0  # aligned by the wrapper
    assert d.dtype == torch.float32 and tuple(d.shape) == (600,) and i.dtype == torch.int64 and tuple(i.shape) == (600,)
    t = ops.chamfer_table(torch.tensor([2, 0, 2, 599, -1, 600, 0]), 600)
    assert t[0].tolist() == [4, 1, 6, 0, 2, 3, 5] and t[1][:4].tolist() == [1, 3, 3, 5] and int(t[1][600]) == 6
    g = ops.chamfer_grad(x, y, torch.zeros(600, dtype=torch.int64), t, (0.5, 0.0), torch.tensor(2.0))
    fn, a = seen.pop()
    assert fn is lib.reni_chamfer_grad and a[:2] == (600, 7) and a[4] is not None and a[5] is None and a[6] is None
    assert a[7:9] == (0.5, 0.0) and a[10] == g.data_ptr() and tuple(g.shape) == (600, 3)
    ops.chamfer_grad(x, y, None, t, (0.0, 1.0))
    fn, a = seen.pop()
    assert a[4] is None and a[5] == t[0].data_ptr() and a[6] == t[1].data_ptr()
    with pytest.raises(ValueError):
        ops.chamfer_grad(x, y, None, t, (0.0, 1.0), torch.ones(2))  # g must hold one value
    m = ico_sphere(1)
    table = ops.mesh_sample_table(m.verts_packed(), m.faces_packed().int())
    fn, a = seen.pop()
    assert fn is lib.reni_mesh_sample_table and a[:2] == (42, 80) and a[4] == table.data_ptr() and tuple(table.shape) == (2, 80)
    assert a[5] % 256 == 0 and a[6] >= lib.reni_mesh_sample_table_workspace_bytes(80) > 0
    idx, wgt, face = ops.mesh_sample_points(m.faces_packed(), table, torch.rand(9, 3), 42)
    fn, a = seen.pop()
    assert fn is lib.reni_mesh_sample_points and a[:3] == (42, 80, 9) and a[6] % 16 == 0 and a[7] % 16 == 0
    assert (idx.dtype, wgt.dtype, face.dtype) == (torch.int32, torch.float32, torch.int64) and tuple(idx.shape) == (9, 8) == tuple(wgt.shape)
    assert not seen


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Argument checks run before any device work, so they hold without a GPU."""
    from reni_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(3 * 2 ** 20)
    p = (ctypes.addressof(buf) + 255) & ~255
    big = 2 ** 31 - 1024

    def nn(N=4, M=4, x=p, y=p, slices=0, d=p, i=p, wsp=p, wsn=2 ** 21 + 256):
        return lib.reni_nearest_points(N, M, x, y, slices, d, i, wsp, wsn, None)

    who = b"nearest points:"
    for kw in (dict(N=0), dict(M=0), dict(N=-1), dict(N=big), dict(M=big), dict(slices=-1), dict(x=None), dict(y=None), dict(d=None),
               dict(i=None)):
        assert nn(**kw) == -1 and lib.reni_last_error().startswith(who), kw
    need = lib.reni_nearest_points_workspace_bytes(4, 4)
    assert nn(wsp=None, wsn=0) == -2 and nn(wsn=need - 1) == -2 and nn(wsp=p + 8) == -2  # RENI_EWORKSPACE
    assert lib.reni_last_error().startswith(who) and b"workspace" in lib.reni_last_error()
    wsb = lib.reni_nearest_points_workspace_bytes
    assert wsb(0, 4) == 0 and wsb(4, 0) == 0 and wsb(big, 4) == 0 and wsb(4, big) == 0 and wsb(big - 1, big - 1) > 0

    def cg(N=4, M=4, x=p, y=p, ixy=p, order=p, off=p, wx=1.0, wy=1.0, g=p, out=p):
        return lib.reni_chamfer_grad(N, M, x, y, ixy, order, off, wx, wy, g, out, None)

    who = b"chamfer grad:"
    for kw in (dict(N=0), dict(M=0), dict(N=big), dict(x=None), dict(y=None), dict(g=None), dict(out=None), dict(ixy=None),
               dict(order=None), dict(off=None), dict(wx=-1.0), dict(wy=float("nan")), dict(wx=float("inf"))):
        assert cg(**kw) == -1 and lib.reni_last_error().startswith(who), kw
    assert b"idx_xy" in (cg(ixy=None), lib.reni_last_error())[1] and b"weights" in (cg(wy=-0.5), lib.reni_last_error())[1]

    def st(V=4, F=4, v=p, f=p, t=p, wsp=p, wsn=4096):
        return lib.reni_mesh_sample_table(V, F, v, f, t, wsp, wsn, None)

    who = b"mesh sample table:"
    for kw in (dict(V=0), dict(F=0), dict(V=2 ** 30), dict(F=2 ** 30), dict(v=None), dict(f=None), dict(t=None)):
        assert st(**kw) == -1 and lib.reni_last_error().startswith(who), kw
    need = lib.reni_mesh_sample_table_workspace_bytes(4)
    assert 0 < need <= 4096 and st(wsp=None, wsn=0) == -2 and st(wsn=need - 1) == -2 and st(wsp=p + 8) == -2
    assert lib.reni_mesh_sample_table_workspace_bytes(0) == 0 and lib.reni_mesh_sample_table_workspace_bytes(2 ** 30) == 0

    def sp(V=4, F=4, S=4, f=p, t=p, u=p, ti=p, tw=p, fi=p):
        return lib.reni_mesh_sample_points(V, F, S, f, t, u, ti, tw, fi, None)

    who = b"mesh sample points:"
    for kw in (dict(V=0), dict(F=0), dict(S=0), dict(S=2 ** 28), dict(V=2 ** 30), dict(f=None), dict(t=None), dict(u=None), dict(ti=None),
               dict(tw=None), dict(fi=None)):
        assert sp(**kw) == -1 and lib.reni_last_error().startswith(who), kw


def test_search_workspace_is_never_n_times_m():
    """linear in N at most (in fact bounded), and independent of M: the partials of the slices, never a distance matrix"""
    from reni_amd import _lib
    ws = _lib.load().reni_nearest_points_workspace_bytes
    for N in (1, 64, 511, 512, 513, 5000, 20000, 100000, 10 ** 6, 10 ** 8):
        sizes = {ws(N, M) for M in (1, 1000, 20000, 10 ** 6, 10 ** 9)}
        assert len(sizes) == 1, N  # independent of M
        assert 0 < ws(N, 1) <= 8 * 512 * N + 768  # at most 512 slices of two 4-byte partials per query
        assert ws(N, 1) <= 2 * 2 ** 20 + 256
    for a, b in ((64, 128), (1000, 2000), (5000, 10000), (20000, 100000)):
        assert ws(b, 1) - 768 <= (b / a) * ws(a, 1)  # no faster than linearly
    assert ws(20000, 20000) < 20000 * 20000 // 100


# -------------------------------------------------------------------------------------------------------------- the build
def test_points_unit_has_no_float_atomics():
    src = open(os.path.join(ROOT, "reni_amd", "csrc", "reni_tu_points.hip")).read()
    assert "atomic" not in src.replace("no float atomic", "")
    assert "hipDeviceSynchronize" not in src and "hipStreamSynchronize" not in src and "hipMemcpy" not in src
    assert '#include "reni_tu_host.inc"' in src and "hipLaunchKernelGGL" not in src  # the shared host path launches


def test_points_translation_unit_isa_audit():
    """reni_tu_points.hip with build.sh's flags: it compiles; no MFMA / transcendental / SDWA hazard, no scratch."""
    import re
    import subprocess
    import tempfile
    from tests import isa_audit
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "points.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_points.hip"), "-o", out], capture_output=True, text=True)
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
    search = text[text.index("k_np_searchENS"):text.index("k_np_combineENS")]
    assert "ds_read_b96" in search or "ds_read_b128" in search  # the targets come from LDS in wide reads
    assert "v_mfma" not in text
