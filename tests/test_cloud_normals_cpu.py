"""CPU tests of the cloud-neighbourhood unit (reni_tu_knn.hip; ops.knn_points, ops.cloud_normals; mesh_losses.knn_points,
estimate_normals, the normals of chamfer_distance, sample_points_from_meshes and geometry_scores): the float64 reference of
tests/cloud_normals_ref.py against independent evaluations and autograd, the error-budget constants, the caps on undecided
rows (they hold for the reference alone), and everything of the new entry points that holds without a GPU (declarations,
argument checks, the workspace bound, no CPU path, the unit's emitted code)."""
import ctypes
import os

import pytest
import torch

from tests import cloud_normals_ref as C
from tests import points_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reni_knn_points_workspace_bytes", "reni_knn_points", "reni_cloud_normals")
KERNELS = ("k_knn_search", "k_knn_combine", "k_cn_normals")


# ---------------------------------------------------------------------------------------------------------- the reference
def test_knn_reference_matches_an_independent_sort():
    for key in (("cube", 1, 1, 1, 1.0), ("cube", 5, 3, 8, 1.0), ("cube", 257, 255, 8, 1.0), ("spheres", 257, 1023, 16, 1e-3)):
        x, y = C.knn_clouds(key)
        K = key[3]
        r = C.knn_of(key)
        d, j = C.knn_independent(x[:40], y, K)
        assert torch.equal(r["idx"][:40, :K], j) and torch.equal(r["d"][:40, :K], d), key
    r = C.knn_of(("cube", 5, 3, 8, 1.0))
    assert (r["idx"][:, 3:] == -1).all() and torch.isinf(r["d"][:, 3:]).all() and (r["idx"][:, :3] >= 0).all()
    x, y = C.lattice()
    r = C.knn(x, y, 8)
    assert (r["d"] == r["d"].round()).all() and (r["d"][:, 0] == 0).all() and torch.equal(r["idx"][:, 0], torch.arange(729))
    centre = 4 * 81 + 4 * 9 + 4  # six neighbours at 1, then the twelve at 2 by ascending index
    assert r["d"][centre, :8].tolist() == [0, 1, 1, 1, 1, 1, 1, 2]
    assert r["idx"][centre, :8].tolist() == [centre, centre - 81, centre - 9, centre - 1, centre + 1, centre + 9, centre + 81,
                                             centre - 81 - 9]
    nan_y = y.clone()
    nan_y[7] = float("nan")
    assert not (C.knn(x[:20], nan_y, 8)["idx"] == 7).any()
    big = torch.full((4, 3), 3e38)
    assert (C.knn(big, -big, 4)["idx"] == -1).all()


def test_undecided_rows_stay_under_the_cap():
    for key in C.KNN_CASES:
        r = C.knn_of(key)
        share = float(r["und"].float().mean())
        print(f"knn {C.case_id(key)}: {int(r['und'].sum())} undecided of {r['und'].numel()} rows")
        assert share <= C.UNDECIDED_CAP, key


def test_normals_reference_solves_the_eigenproblem_and_gaps_are_open():
    for key in C.NORMAL_CASES:
        y, idx, ref = C.normal_case(key)
        assert (idx[:, 0] == torch.arange(y.shape[0])).all()  # the point itself is its first neighbour
        pts = y.double()[idx]
        e = pts - pts.mean(1, keepdim=True)
        cov = torch.einsum("nka,nkb->nab", e, e) / idx.shape[1]
        res = torch.einsum("nab,nb->na", cov, ref["normal"]) - ref["eig"][:, :1] * ref["normal"]
        assert float(res.abs().max()) <= 1e-12 * float(ref["eig"].max())
        assert float((ref["normal"].norm(dim=1) - 1).abs().max()) <= 1e-12
        assert (ref["eig"][:, 0] <= ref["eig"][:, 1]).all() and (ref["eig"][:, 1] <= ref["eig"][:, 2]).all()
        n32, e32 = C.normals32(y, idx)
        re, ra, left_out, gap = C.normal_ratios(n32, e32, ref)
        print(f"normals {C.case_id(key)}: smallest gap ratio {gap:.4g}, left out {100 * left_out:.2f} %")
        assert left_out <= C.UNDECIDED_CAP, key
    kind = {k[0] for k in C.NORMAL_CASES}
    assert kind == {"sphere", "cubesurf", "ellipsoid", "plane"} and {k[2] for k in C.NORMAL_CASES} == {8, 16, 32}
    assert all(1000 <= k[1] <= 2000 for k in C.NORMAL_CASES)
    # degenerate lists by the definition: fewer than 3 usable slots
    y = C.normal_cloud("sphere", 1500)
    ref = C.normals(y, torch.tensor([[0, 1, -1], [0, -1, -1], [3, 4, 5]]))
    assert (ref["normal"][:2] == 0).all() and (ref["eig"][:2] == 0).all() and float(ref["normal"][2].norm()) > 0.99


def test_normal_term_closed_form_matches_autograd():
    for name in C.NT_CASES:
        nx, ny = C.nt_normals(name)
        ch = P.chamfer_of(name, (1.0, 1.0))
        ix, iy = ch["matches"][0]["idx"], ch["matches"][1]["idx"]
        for weights in C.NT_WEIGHTS:
            for ac in (True, False):
                ref = C.nt_of(name, weights, ac)
                L, gx, gy = C.normal_term_autograd(nx, ny, ix, iy, weights, ac)
                assert abs(float(L - ref["value"])) <= 1e-12 * max(float(ref["value_terms"]), 1e-300)
                assert C.M.error_ratio(gx, ref["gx"], ref["gx_terms"]) < 1e-6 and C.M.error_ratio(gy, ref["gy"], ref["gy_terms"]) < 1e-6
    # a zero normal: a finite value and gradient
    nx, ny = (t.clone() for t in C.nt_normals("cube"))
    nx[0] = 0.0
    ch = P.chamfer_of("cube", (1.0, 1.0))
    ref = C.normal_term(nx, ny, ch["matches"][0]["idx"], ch["matches"][1]["idx"])
    assert all(bool(torch.isfinite(ref[k]).all()) for k in ("value", "gx", "gy"))


def test_face_normals_closed_form_matches_autograd():
    for key in C.FN_MESHES:
        v, f, u, up, s, ref = C.fn_case(key)
        n, g = C.face_normals_autograd(v, f, s["face"], up)
        assert C.M.error_ratio(n, ref["n"], ref["n_terms"]) < 1e-6 and C.M.error_ratio(g, ref["gv"], ref["gv_terms"]) < 1e-6
        assert float((ref["n"].norm(dim=1) - 1).abs().max()) <= 1e-12
    v, f = (t for t in P.sample_mesh(("ico", 16)))
    assert 0.0 < C.max_dihedral_cos(v, f) < 1.0


def test_consistency_references_on_known_answers():
    """a mesh against itself: every sample's nearest triangle has its own normal or a tied neighbour's; a cube inside a cube:
    the match is the parallel face or a tie"""
    from reni_amd.mesh import ico_sphere
    u = torch.rand(300, 3, generator=torch.Generator().manual_seed(2))
    m = ico_sphere(1)
    v, f = m.verts_packed(), m.faces_packed()
    floor = C.max_dihedral_cos(v, f)
    for c, bound, tied in C.consistency_surface(v, f, v, f, u):
        assert floor <= c <= 1.0 + 1e-12 and 1.0 - c <= bound
    small, big = C.cube_mesh(0.6), C.cube_mesh(1.2)
    (cp, bp, tp), (ct, bt, tt) = C.consistency_surface(*small, *big, u)
    assert abs(cp - 1.0) <= 1e-12 and bp < 1e-5  # every inner sample is nearest to the parallel outer face (ties share its normal)
    assert 0.0 < ct < 1.0 and ct - bt <= 1.0
    (sp, bsp), (st, bst) = C.consistency(*small, *small, u)
    assert abs(sp - 1.0) <= 1e-12 and abs(st - 1.0) <= 1e-12  # the same u: every sample matches its twin


def test_error_budget_constants_are_the_measured_ones():
    """K = 4 x the worst ratio of the float32 CPU evaluation, hard-coded in the case file: still what is measured."""
    r = C.float32_ratios()
    print("float32 CPU evaluation, worst ratios: eigenvalues %.4g, angle %.4g; face normals %.4g, their gradient %.4g; "
          "term %.4g, its gradients %.4g" % r)
    for k, v in zip((C.K_E, C.K_N, C.K_FN, C.K_FNG, C.K_NT, C.K_NTG), r):
        assert k / 2 <= 4 * v <= k * 1.001, (k, v)


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
    assert " knn " in build and "_build/knn.o" in build and " knn " in isa
    for word in ("cloud neighbourhoods", "LEXICOGRAPHIC", "+inf and -1", "[-1, M)", "ANY slicing", "cyclic Jacobi", "6 sweeps",
                 "ASCENDING", "exactly (0, 0, 0)", "Never a NaN", "independent of M", "2^31 - 1025"):
        assert word in h, word


def test_cpu_tensors_raise():
    from reni_amd import _lib, mesh_losses, ops
    from reni_amd.mesh import ico_sphere
    x, y = torch.rand(5, 3), torch.rand(7, 3)
    idx = torch.zeros(5, 4, dtype=torch.int64)
    m = ico_sphere(0)
    calls = (lambda: ops.knn_points(x, y, 3), lambda: mesh_losses.knn_points(x, y, 3), lambda: ops.cloud_normals(y, idx),
             lambda: ops.cloud_normals(y, idx, viewpoint=(0.0, 0.0, 1.0)), lambda: mesh_losses.estimate_normals(y, 4),
             lambda: mesh_losses.chamfer_distance(x, y, x_normals=x, y_normals=y),
             lambda: mesh_losses.sample_points_from_meshes(m, 4, return_normals=True),
             lambda: mesh_losses.geometry_scores(m, m, n=4, normals=True))
    for call in calls:
        with pytest.raises(_lib.RENILibraryError):
            call()


def test_bad_arguments_raise_value_errors_before_the_device_check():
    from reni_amd import mesh_losses, ops
    x, y = torch.rand(5, 3), torch.rand(7, 3)
    idx = torch.zeros(5, 4, dtype=torch.int64)
    bad = (lambda: ops.knn_points(x, y, 0), lambda: ops.knn_points(x, y, 33), lambda: ops.knn_points(x, y, 2.0),
           lambda: ops.knn_points(x, y, True), lambda: ops.knn_points(x, y, "3"), lambda: ops.knn_points(torch.rand(5, 2), y, 3),
           lambda: ops.knn_points(x, torch.rand(0, 3), 3), lambda: ops.knn_points(x, y, 3, slices=-1),
           lambda: mesh_losses.knn_points(x, y, 0), lambda: mesh_losses.estimate_normals(y, 0),
           lambda: mesh_losses.estimate_normals(y, 50), lambda: mesh_losses.estimate_normals(torch.rand(5), 4),
           lambda: ops.cloud_normals(torch.rand(7, 2), idx), lambda: ops.cloud_normals(y, idx.int()),
           lambda: ops.cloud_normals(y, idx[:, 0]), lambda: ops.cloud_normals(y, torch.zeros(5, 33, dtype=torch.int64)),
           lambda: ops.cloud_normals(y, idx, viewpoint=(0.0, 1.0)),
           lambda: ops.cloud_normals(y, torch.zeros(8, 4, dtype=torch.int64), viewpoint=(0.0, 0.0, 1.0)),
           lambda: mesh_losses.chamfer_distance(x, y, x_normals=x), lambda: mesh_losses.chamfer_distance(x, y, y_normals=y),
           lambda: mesh_losses.chamfer_distance(x, y, x_normals=y, y_normals=y),
           lambda: mesh_losses.chamfer_distance(x, y, x_normals=x, y_normals=y[:, :2]))
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} did not raise")


def test_wrappers_behind_the_device_check(monkeypatch):
    """with the device check and the launch taken out: what reaches the library"""
    from reni_amd import _lib, ops
    lib = _lib.load()
    seen = []
    monkeypatch.setattr(ops, "_require_cuda", lambda *t: None)
    monkeypatch.setattr(ops, "_call", lambda fn, device, *args: seen.append((fn, args)))
    x, y = torch.rand(600, 3), torch.rand(7, 3)
    d, i = ops.knn_points(x.double(), y, 5, slices=3)
    fn, a = seen.pop()
    assert fn is lib.reni_knn_points and a[:3] == (600, 7, 5) and a[5] == 3 and a[6] == d.data_ptr() and a[7] == i.data_ptr()
    assert a[8] % 256 == 0 and a[9] >= lib.reni_knn_points_workspace_bytes(600, 7, 5) > 0  # aligned by the wrapper
    assert d.dtype == torch.float32 and tuple(d.shape) == (600, 5) and i.dtype == torch.int64 and tuple(i.shape) == (600, 5)
    n, e = ops.cloud_normals(y, torch.zeros(4, 6, dtype=torch.int64))
    fn, a = seen.pop()
    assert fn is lib.reni_cloud_normals and a[:3] == (4, 7, 6) and a[5] is None and a[6] == n.data_ptr() and a[7] == e.data_ptr()
    assert tuple(n.shape) == (4, 3) == tuple(e.shape) and n.dtype == torch.float32
    ops.cloud_normals(y, torch.zeros(4, 6, dtype=torch.int64), viewpoint=torch.tensor([0.0, 0.0, 2.0]))
    fn, a = seen.pop()
    assert a[5] is not None
    assert not seen


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Argument checks run before any device work, so they hold without a GPU."""
    from reni_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(2 ** 20)
    p = (ctypes.addressof(buf) + 255) & ~255
    big = 2 ** 31 - 1024

    def kn(N=4, M=4, K=3, x=p, y=p, slices=0, d=p, i=p, wsp=p, wsn=2 ** 19):
        return lib.reni_knn_points(N, M, K, x, y, slices, d, i, wsp, wsn, None)

    who = b"knn points:"
    for kw in (dict(N=0), dict(M=0), dict(N=-1), dict(N=big), dict(M=big), dict(K=0), dict(K=33), dict(K=-1), dict(slices=-1),
               dict(x=None), dict(y=None), dict(d=None), dict(i=None)):
        assert kn(**kw) == -1 and lib.reni_last_error().startswith(who), kw
    need = lib.reni_knn_points_workspace_bytes(4, 4, 3)
    assert 0 < need <= 2 ** 19
    assert kn(wsp=None, wsn=0) == -2 and kn(wsn=need - 1) == -2 and kn(wsp=p + 8) == -2  # RENI_EWORKSPACE
    assert lib.reni_last_error().startswith(who) and b"workspace" in lib.reni_last_error()
    wsb = lib.reni_knn_points_workspace_bytes
    assert wsb(0, 4, 3) == 0 and wsb(4, 0, 3) == 0 and wsb(big, 4, 3) == 0 and wsb(4, big, 3) == 0 and wsb(4, 4, 0) == 0
    assert wsb(4, 4, 33) == 0 and wsb(big - 1, big - 1, 32) > 0

    def cn(N=4, M=4, K=3, y=p, i=p, view=None, n=p, e=p):
        return lib.reni_cloud_normals(N, M, K, y, i, view, n, e, None)

    who = b"cloud normals:"
    for kw in (dict(N=0), dict(M=0), dict(N=big), dict(M=big), dict(K=0), dict(K=33), dict(y=None), dict(i=None), dict(n=None),
               dict(e=None), dict(N=5, view=p)):
        assert cn(**kw) == -1 and lib.reni_last_error().startswith(who), kw


def test_knn_workspace_is_bounded_and_never_n_times_m():
    """the partials of cap N K pairs with np_slices' cap rule: N cap <= 512 * 256, independent of M"""
    from reni_amd import _lib
    ws = _lib.load().reni_knn_points_workspace_bytes
    for K in (1, 4, 5, 8, 16, 32):
        for N in (1, 64, 255, 256, 257, 5000, 20000, 100000, 10 ** 6, 10 ** 8):
            sizes = {ws(N, M, K) for M in (1, 1000, 20000, 10 ** 6, 10 ** 9)}
            assert len(sizes) == 1, (N, K)  # independent of M
            assert 0 < ws(N, 1, K) <= 8 * 512 * 256 * K + 768  # at most K MiB + 768
            blocks = (N + 255) // 256
            cap = max(1, 512 // blocks)
            assert ws(N, 1, K) <= 8 * cap * N * K + 768
    assert ws(10 ** 6, 1, 32) == 256  # the queries alone fill the device: one slice, no partials
    assert ws(20000, 20000, 32) < 20000 * 20000 * 4 // 10


# -------------------------------------------------------------------------------------------------------------- the build
def test_knn_unit_uses_the_shared_host_path_and_no_atomics():
    src = open(os.path.join(ROOT, "reni_amd", "csrc", "reni_tu_knn.hip")).read()
    assert "atomic" not in src.replace("no float atomic", "")
    assert "hipDeviceSynchronize" not in src and "hipStreamSynchronize" not in src and "hipMemcpy" not in src
    assert '#include "reni_tu_host.inc"' in src and "hipLaunchKernelGGL" not in src  # the shared host path launches


def test_knn_translation_unit_compiles_without_private_memory():
    """reni_tu_knn.hip with build.sh's flags: it compiles, every kernel's private segment is 0 (the register lists stay in
    registers), and the existing hazard checks of tests/isa_audit.py return nothing.  Resource metadata and the existing
    helper only."""
    import re
    import subprocess
    import tempfile
    from tests import isa_audit
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "knn.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_knn.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    for k in KERNELS:
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 9 and all(int(n) == 0 for n in sizes)  # four search and four combine instances, the normals kernel
    lds = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text)
    assert sorted(int(n) for n in lds) == [0] * 5 + [16384] * 4
