"""CPU tests of the G-buffer's gradient with respect to the vertices (reni_tu_raster_bwd.hip, ops.gbuffer_backward,
ops.vertex_normals_backward): the float64 reference of tests/gbuffer_grad_ref.py against central differences with the face
assignment fixed, its hand-written closed form against its autograd, the error-budget constants, and everything of the new
entry points that holds without a GPU (declarations, argument checks, no CPU path)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import gbuffer_grad_ref as G
from tests import raster_edge_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reni_mesh_vertex_normals_backward", "reni_gbuffer_backward_workspace_bytes", "reni_gbuffer_backward")


def test_the_cases_are_what_they_claim():
    v, f, *_ = G.case("tetra", 8)
    assert v.shape == (4, 3) and f.shape == (4, 3)
    v, f, *_ = G.case("ico", 16)
    assert v.shape == (42, 3) and f.shape == (80, 3)
    assert int((G.cpu_pix_to_face(("cover", 33)) == 0).sum()) == 33 * 33  # one face under 1089 pixels
    v, f, *_ = G.case("fan", 16)
    assert int((f == 0).sum()) == 300
    assert [G.case("strip", V)[0].shape[0] for V in (255, 256, 257)] == [255, 256, 257]
    v, f, *_ = G.case("soup", 17)
    p2f = G.cpu_pix_to_face(("soup", 17))
    assert f.shape[0] == 60 and len(set(p2f[p2f >= 0].tolist())) < 60  # faces that win no pixel
    v, f, *_ = G.case("unreferenced", 16)
    assert not (f == G.UNREFERENCED).any()
    assert int((G.cpu_pix_to_face(("behind", 16)) >= 0).sum()) == 0
    v, f, *_ = G.case("tiny_normal", 16)
    u = np.zeros(3)
    for a, b, c in f[(f == 0).any(axis=1)]:
        u += np.cross(v[b].astype(np.float64) - v[a], v[c].astype(np.float64) - v[a])
    assert np.linalg.norm(u) < 1e-6  # vertex 0 takes the max branch
    for key in G.CASES:
        if key[0] not in ("behind",):
            assert int((G.cpu_pix_to_face(key) >= 0).sum()) > 0, key


@pytest.mark.parametrize("key", G.CASES, ids=G.case_id)
def test_reference_autograd_matches_central_differences(key):
    """<g, d> against (f(v + h d) - f(v - h d)) / 2h for random directions d, the face assignment fixed.  h = 1e-7 keeps the
    tiny-normal vertex inside the max branch; the difference quotient of a float64 f of size sum |terms| is then good to
    ~1e-16 sum |terms| / h plus the O(h^2) term."""
    v, f, R, T, S = G.case(*key)
    p2f = G.cpu_pix_to_face(key)
    faces = torch.from_numpy(f)
    h = 1e-7
    for variant in G.VARIANTS:
        gN, gX = G.upstream(key, variant)
        g = G.reference(key, p2f, gN, gX)
        _, terms = G.scales(key, variant)
        gen = torch.Generator().manual_seed(7)
        for _ in range(4):
            d = torch.randn(v.shape[0], 3, generator=gen, dtype=torch.float64)
            vals = [float(G.objective(torch.from_numpy(v).double() + s * h * d, faces, R[0].double(), T[0].double(), S, E.TANF,
                                      p2f, gN, gX)) for s in (1.0, -1.0)]
            fd = (vals[0] - vals[1]) / (2 * h)
            scale = float((terms * d.abs()).sum())
            assert abs(fd - float((g * d).sum())) <= 1e-6 * scale + 1e-12, (key, variant)


@pytest.mark.parametrize("key", G.CASES, ids=G.case_id)
def test_closed_form_matches_autograd_in_float64(key):
    """the hand-written chain (the kernels' structure) is the autograd gradient, far below the float32 budget"""
    p2f = G.cpu_pix_to_face(key)
    for variant in G.VARIANTS:
        gN, gX = G.upstream(key, variant)
        ref = G.reference(key, p2f, gN, gX)
        got, terms = G.scales(key, variant)
        assert (terms >= ref.abs() * (1 - 1e-9)).all()
        assert G.error_ratio(got, ref, terms) < 1e-6
    v, f, *_ = G.case(*key)
    gn = G.normals_upstream(key)
    got, terms = G.vn_closed_form(torch.from_numpy(v).double(), torch.from_numpy(f), gn)
    assert G.error_ratio(got, G.vertex_normals_reference(v, f, gn), terms) < 1e-6


def test_exact_zeros_of_the_reference():
    key = ("unreferenced", 16)
    gN, gX = G.upstream(key, "both")
    g = G.reference(key, G.cpu_pix_to_face(key), gN, gX)
    assert (g[G.UNREFERENCED] == 0).all() and (g != 0).any()
    key = ("behind", 16)
    assert (G.reference(key, G.cpu_pix_to_face(key), *G.upstream(key, "both")) == 0).all()


def test_error_budget_constants_are_the_measured_ones():
    """K = 4 x the worst ratio of the float32 CPU evaluation, hard-coded in the case file: still what is measured."""
    rg, rn = G.float32_ratios()
    print(f"float32 closed form, worst error / (2^-23 sum |terms|): g_verts {rg:.4g}, vertex-normal backward {rn:.4g}")
    assert G.K_GVERTS / 2 <= 4 * rg <= G.K_GVERTS * 1.001
    assert G.K_VNORMALS / 2 <= 4 * rn <= G.K_VNORMALS * 1.001


def test_header_and_integration_name_the_entry_points():
    from reni_amd import _lib
    h = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name + "(" in h and name in _lib.EXPORTS and name in doc
    build = open(os.path.join(ROOT, "reni_amd", "csrc", "build.sh")).read()
    assert " raster_bwd " in build and "_build/raster_bwd.o" in build
    for word in ("1e-8", "max(|u_v|, 1e-6)", "pix_to_face", "face_pixel_offsets"):
        assert word in h


def test_cpu_tensors_raise():
    from reni_amd import _lib, ops
    v, f = torch.rand(3, 3), torch.tensor([[0, 1, 2]])
    with pytest.raises(_lib.RENILibraryError):
        ops.vertex_normals_backward(v, f, torch.rand(3, 3))
    with pytest.raises(_lib.RENILibraryError):
        ops.gbuffer_backward(v, f, v, torch.eye(3), torch.zeros(3), 4, torch.zeros(16, dtype=torch.int64), torch.rand(16, 3), None)


def test_bad_shapes_raise_value_errors():
    from reni_amd import ops
    v, f, n = torch.rand(3, 3), torch.tensor([[0, 1, 2]]), torch.rand(3, 3)
    p2f, g = torch.zeros(16, dtype=torch.int64), torch.rand(16, 3)
    I, Z = torch.eye(3), torch.zeros(3)
    with pytest.raises(ValueError):
        ops.vertex_normals_backward(torch.rand(3, 2), f, n)
    with pytest.raises(ValueError):
        ops.vertex_normals_backward(v, torch.tensor([0, 1, 2]), n)
    with pytest.raises(ValueError):
        ops.vertex_normals_backward(v, f, torch.rand(4, 3))
    for args in ((torch.rand(3, 4), f, n, I, Z, 4, p2f, g, g), (v, torch.zeros(0, 3, dtype=torch.int64), n, I, Z, 4, p2f, g, g),
                 (v, f, torch.rand(2, 3), I, Z, 4, p2f, g, g), (v, f, n, torch.eye(2), Z, 4, p2f, g, g),
                 (v, f, n, I, torch.zeros(2), 4, p2f, g, g), (v, f, n, I, Z, 0, p2f, g, g), (v, f, n, I, Z, 4, p2f[:15], g, g),
                 (v, f, n, I, Z, 4, p2f.to(torch.int32), g, g), (v, f, n, I, Z, 4, p2f, torch.rand(15, 3), g),
                 (v, f, n, I, Z, 4, p2f, g, torch.rand(16, 2)), (v, f, n, I, Z, 4, p2f, None, None)):
        with pytest.raises(ValueError):
            ops.gbuffer_backward(*args)


def test_c_abi_rejects_bad_sizes_null_pointers_and_short_workspaces():
    """Argument checks run before any device work, so they hold without a GPU."""
    from reni_amd import _lib
    lib = _lib.load()
    R, T = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (ctypes.c_float * 3)()
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 255) & ~255
    need = lib.reni_gbuffer_backward_workspace_bytes(3, 1, 8, 8)
    assert 18 * 4 + 3 * 12 <= need <= 4096 and lib.reni_gbuffer_backward_workspace_bytes(0, 1, 8, 8) == 0
    assert lib.reni_gbuffer_backward_workspace_bytes(3, 0, 8, 8) == 0

    def call(V=3, F=1, tanh=0.5, H=8, W=8, ptrs=None, gN=p, gX=p, ws=p, wsn=4096, Rp=R):
        ptrs = [p] * 8 if ptrs is None else ptrs
        return lib.reni_gbuffer_backward(V, F, ptrs[0], ptrs[1], ptrs[2], Rp, T, tanh, H, W, ptrs[3], ptrs[4], ptrs[5], ptrs[6],
                                         ptrs[7], gN, gX, p, ws, wsn, None)

    for kw in (dict(V=0), dict(F=0), dict(H=8, W=9), dict(H=0, W=0), dict(tanh=0.0), dict(tanh=-1.0), dict(tanh=float("nan"))):
        assert call(**kw) == -1 and lib.reni_last_error().startswith(b"gbuffer backward:")
    for i in range(8):
        ptrs = [p] * 8
        ptrs[i] = None
        assert call(ptrs=ptrs) == -1 and b"NULL" in lib.reni_last_error()
    assert call(gN=None, gX=None) == -1 and b"both" in lib.reni_last_error()
    assert call(ws=None, wsn=0) == -2 and call(wsn=64) == -2 and call(ws=p + 8) == -2  # RENI_EWORKSPACE
    assert lib.reni_mesh_vertex_normals_backward(0, 1, p, p, p, p, p, p, None) == -1
    assert lib.reni_mesh_vertex_normals_backward(3, 0, p, p, p, p, p, p, None) == -1
    for i in range(6):
        ptrs = [p] * 6
        ptrs[i] = None
        assert lib.reni_mesh_vertex_normals_backward(3, 1, *ptrs, None) == -1 and b"NULL" in lib.reni_last_error()


def test_raster_backward_unit_has_no_float_atomics():
    for name in ("reni_tu_raster_bwd.hip", "reni_mesh.inc"):  # the unit and the header its projection and list walks live in
        src = open(os.path.join(ROOT, "reni_amd", "csrc", name)).read()
        assert "atomic" not in src.replace("no float atomic", "")


def test_raster_backward_translation_unit_isa_audit():
    """reni_tu_raster_bwd.hip with build.sh's flags: no MFMA / transcendental / SDWA hazard, no scratch."""
    import re
    import subprocess
    import tempfile
    from tests import isa_audit
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "raster_bwd.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_raster_bwd.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    for k in ("k_gb_face", "k_gb_vertex", "k_vn_bwd"):
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text and "atomic" not in text
    for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", text):
        assert int(m.group(1)) == 0
