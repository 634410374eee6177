"""CPU tests of the mesh regularisers (reni_tu_meshreg.hip, ops.mesh_regularizers, reni_amd/mesh_losses.py): the cases, the
topology lists against their definition, the float64 reference of tests/mesh_reg_ref.py against central differences, its
hand-written closed form against its autograd, the share of undecided elements, the error-budget constants, and everything of
the new entry points that holds without a GPU (declarations, argument checks, no CPU path, the unit's emitted code)."""
import ctypes
import os

import pytest
import torch

from tests import mesh_reg_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reni_mesh_regularizers_workspace_bytes", "reni_mesh_regularizers")


def test_the_cases_are_what_they_claim():
    def sizes(key):
        T = M.topology(key)
        return T.V, T.E, T.P

    assert sizes(("tetra", 8)) == (4, 6, 6)
    assert sizes(("ico", 16)) == (42, 120, 120)
    T = M.topology(("fan", 16))
    assert (T.E, T.P) == (600, 300) and T.mult.count(1) == 300 and int((T.nb[:, 0] == 0).sum()) == 300  # degree 300 at vertex 0
    assert sizes(("cover", 33)) == (3, 3, 0)
    T = M.topology(("soup", 17))
    assert T.P == 0 and max(T.mult) == 1 and T.part.numel() == T.F - 1  # no shared edge, one bad-index face
    assert T.V - int(torch.unique(T.nb[:, 0]).numel()) == 3  # ... whose three vertices have no neighbour
    T = M.topology(("unreferenced", 16))
    assert not (T.nb[:, 0] == M.G.UNREFERENCED).any() and T.E == 120
    T = M.topology(("bad_faces", 16))
    assert (T.F, T.part.numel()) == (85, 81) and T.nb[T.nb[:, 0] == 43][:, 1].tolist() == [42, 44]
    x = M.verts(("bad_faces", 16), torch.float32)
    assert ((x[42] + x[44]) * 0.5 == x[43]).all()  # the exact midpoint, in float32 too
    assert sizes(("tiny_normal", 16))[2] == 1
    for V in M.STRIPS:
        assert sizes(("strip", V)) == (V, 2 * V - 3, V - 3)
    for n in (256, 512):
        for col in range(3):
            vals = [sizes(("strip", V))[col] for V in M.STRIPS]
            assert min(vals) <= n < max(vals) and any(v <= n for v in vals) and any(v > n for v in vals)
    assert any(2 * V - 3 <= 4096 for V in M.STRIPS) and any(2 * V - 3 > 4096 for V in M.STRIPS)  # the reducer's chunk
    T = M.topology(("book", 0))
    assert max(T.mult) == 3 and T.P == 3
    T = M.topology(("double", 0))
    assert T.mult == [2, 2, 2] and T.P == 3
    assert abs(M.reference(("double", 0), "normal")[0] - 2.0) < 1e-12   # a repeated face: cos = -1
    assert abs(M.reference(("hinge", 90), "normal")[0] - 1.0) < 1e-7
    assert M.reference(("hinge", 0), "normal")[0] == 0.0 and M.reference(("cover", 33), "normal")[0] == 0.0
    # independent of the winding
    key = ("ico", 16)
    v, f = M.mesh(key)
    flipped = f.copy()
    flipped[1::2] = flipped[1::2][:, [0, 2, 1]]  # every other face turned round
    a = M.losses(M.verts(key), M.topology(key))[2]
    b = M.losses(M.verts(key), M.build_topology(v.shape[0], flipped))[2]
    assert abs(float(a) - float(b)) < 1e-15


@pytest.mark.parametrize("key", M.CASES, ids=M.case_id)
def test_edge_lists_are_the_definition(key):
    """ops.mesh_edge_lists (stable sorts, plain torch) against the lists built by their definition with Python loops"""
    from reni_amd import ops
    v, f = M.mesh(key)
    T = M.topology(key)
    L = ops.mesh_edge_lists(torch.from_numpy(f), v.shape[0])
    assert (L["E"], L["P"], L["H"], L["V"], L["F"]) == (T.E, T.P, T.H, T.V, T.F)
    assert all(L[k].dtype == torch.int64 for k in ops._EDGE_LIST_NAMES)
    assert torch.equal(L["edges"][:T.E], T.edges)
    assert torch.equal(L["ef_corners"][:T.H], 3 * T.half[:, 1] + T.half[:, 2])
    off = torch.searchsorted(T.half[:, 0].contiguous(), torch.arange(T.E + 1))
    assert torch.equal(L["ef_offsets"], off)
    assert torch.equal(L["ve_edges"][:2 * T.E], T.nb[:, 2])
    assert torch.equal(L["ve_offsets"], torch.searchsorted(T.nb[:, 0].contiguous(), torch.arange(T.V + 1)))
    ce = torch.full((3 * T.F,), -1, dtype=torch.int64)
    ce[3 * T.half[:, 1] + T.half[:, 2]] = T.half[:, 0]
    assert torch.equal(L["corner_edges"], ce)
    vo, vc = ops.vertex_face_lists(torch.from_numpy(f), v.shape[0])
    assert torch.equal(L["vf_offsets"], vo) and torch.equal(L["vf_corners"], vc)


def test_meshes_keeps_the_lists_and_hands_out_the_edges():
    from reni_amd.mesh import Meshes
    v, f = M.mesh(("bad_faces", 16))
    m = Meshes(verts=[torch.from_numpy(v).clone()], faces=[torch.from_numpy(f).clone()])  # (the case's arrays are shared: copies)
    e = m.edges_packed()
    assert torch.equal(e, M.topology(("bad_faces", 16)).edges)
    first = m._edge_lists()
    with torch.no_grad():
        m.verts_packed().mul_(1.5)  # the vertices move: the lists stay
    assert m._edge_lists() is first
    m.faces_packed()[0] = torch.tensor([0, 0, 1])  # the faces change in place: new lists
    assert m._edge_lists() is not first


def test_undecided_elements_stay_under_the_cap():
    worst = 0.0
    for loss in M.LOSSES:
        for key in M.parity_cases(loss):
            u, n = M.undecided_share(key, loss)
            worst = max(worst, u / n)
            print(f"{M.case_id(key)}-{loss}: {u} undecided of {n} elements ({100 * u / n:.2f} %)")
            assert u / n <= M.UNDECIDED_CAP, (key, loss, u, n)
            if loss != "cot":
                assert u == 0, (key, loss)
    # the collinear face of "bad_faces" sits at the area floor: under "cot" it reaches the rows of 42, 43, 44 and the value
    u, n = M.undecided_share(("bad_faces", 16), "cot")
    print(f"bad_faces-16-cot: {u} undecided of {n} elements ({100 * u / n:.2f} %): over the cap, bounded on bad_faces_cot instead")
    assert u / n > M.UNDECIDED_CAP and M.scales(("bad_faces", 16), "cot")["und_rows"].nonzero()[:, 0].tolist() == [42, 43, 44]
    assert ("bad_faces", 16) not in M.parity_cases("cot") and ("bad_faces_cot", 16) in M.parity_cases("cot")
    print(f"worst share over the parity cases {100 * worst:.2f} %")


@pytest.mark.parametrize("loss", M.LOSSES)
def test_closed_form_matches_autograd_in_float64(loss):
    """the hand-written chain is the autograd gradient, far below the float32 budget, and its terms dominate it"""
    for key in M.parity_cases(loss):
        s = M.scales(key, loss)
        val, g = M.reference(key, loss, M.target_of(loss))
        keep = ~s["und_rows"]
        assert M.error_ratio(s["g"], g, s["g_terms"], keep) < 1e-6, key
        assert abs(float(s["value"]) - val) <= 1e-6 * M.U * float(s["value_terms"]) + 1e-300, key
        assert (s["g_terms"][keep] >= g.abs()[keep] * (1 - 1e-9)).all() and float(s["value_terms"]) >= abs(val) * (1 - 1e-9)


def test_reference_autograd_matches_central_differences():
    h = 1e-6
    ran = 0
    for loss in M.LOSSES:
        for key in (("tetra", 8), ("ico", 16), ("fan", 16), ("book", 0), ("hinge", 90), ("strip", 129), ("bad_faces_cot", 16)):
            T = M.topology(key)
            x = M.verts(key)
            val, g = M.reference(key, loss, M.target_of(loss))
            terms = M.scales(key, loss)["g_terms"]
            pick = {"edge": 0, "uniform": 1, "cot": 1, "normal": 2}[loss]
            method = "cot" if loss == "cot" else "uniform"
            gen = torch.Generator().manual_seed(7)
            for _ in range(2):
                d = torch.randn(T.V, 3, generator=gen, dtype=torch.float64)
                if loss == "cot":  # the weights are constants of the gradient: differentiate with them frozen
                    w0 = M._cot_weights(x, T)
                    orig = M._cot_weights
                    M._cot_weights = lambda *_: w0
                try:
                    with torch.no_grad():
                        vals = [float(M.losses(x + s * h * d, T, M.target_of(loss), method)[pick]) for s in (1.0, -1.0)]
                finally:
                    if loss == "cot":
                        M._cot_weights = orig
                fd = (vals[0] - vals[1]) / (2 * h)
                scale = float((terms * d.abs()).sum())
                assert abs(fd - float((g * d).sum())) <= 1e-6 * scale + 1e-12, (key, loss, fd, float((g * d).sum()))
                ran += 1
    assert ran == 56


def test_exact_zeros_of_the_reference():
    for loss in M.LOSSES:
        val, g = M.reference(("unreferenced", 16), loss)
        assert (g[M.G.UNREFERENCED] == 0).all() and (g != 0).any()
    s = M.scales(("bad_faces", 16), "uniform")
    x = M.verts(("bad_faces", 16))
    assert ((x[42] + x[44]) * 0.5 - x[43] == 0).all()  # r_43 = 0: its own share -u_43 of the Laplacian gradient is exactly 0
    assert M.scales(("cover", 33), "normal")["value"] == 0 and (M.scales(("cover", 33), "normal")["g"] == 0).all()
    assert s["value"] > 0


def test_error_budget_constants_are_the_measured_ones():
    """K = 4 x the worst ratio of the float32 CPU evaluation, hard-coded in the case file: still what is measured."""
    ratios = M.float32_ratios()
    for loss in M.LOSSES:
        rv, rg = ratios[loss]
        print(f"{loss}: float32 closed form, worst error / (2^-23 sum |terms|): value {rv:.4g}, grad_verts {rg:.4g}")
        assert M.K[loss][0] / 2 <= 4 * rv <= M.K[loss][0] * 1.001, loss
        assert M.K[loss][1] / 2 <= 4 * rg <= M.K[loss][1] * 1.001, loss


def test_fit_reference_is_the_recorded_one():
    losses = M.fit_reference()
    print(f"float64 fit: loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert abs(losses[0] - M.FIT_START) < 1e-9 and abs(losses[-1] - M.FIT_END) < 1e-9
    assert losses[-1] < 0.75 * losses[0]


def test_header_integration_build_and_binding_name_the_entry_points():
    from reni_amd import _lib
    h = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name + "(" in h and name in _lib.EXPORTS and name in doc
    build = open(os.path.join(ROOT, "reni_amd", "csrc", "build.sh")).read()
    assert " meshreg " in build and "_build/meshreg.o" in build
    for word in ("TAKES PART", "m (m - 1) / 2", "WITHOUT NEIGHBOURS", "CONSTANTS of the gradient", "1e-12", "RENI_LAPLACIAN_COT",
                 "corner_edges"):
        assert word in h, word
    assert _lib.LAPLACIAN == {"uniform": 0, "cot": 1}


def _mesh_cpu():
    from reni_amd.mesh import Meshes
    v, f = M.mesh(("tetra", 8))
    return Meshes(verts=[torch.from_numpy(v)], faces=[torch.from_numpy(f)])


def test_cpu_tensors_raise():
    from reni_amd import _lib, mesh_losses, ops
    m = _mesh_cpu()
    for fn in (mesh_losses.mesh_edge_loss, mesh_losses.mesh_laplacian_smoothing, mesh_losses.mesh_normal_consistency):
        with pytest.raises(_lib.RENILibraryError):
            fn(m)
    with pytest.raises(_lib.RENILibraryError):
        mesh_losses.mesh_regularizer(m, edge=1.0)
    with pytest.raises(_lib.RENILibraryError):
        ops.mesh_regularizers(m.verts_packed(), m.faces_packed(), 1.0, 1.0, 1.0)


def test_bad_arguments_raise_value_errors():
    from reni_amd import mesh_losses, ops
    m = _mesh_cpu()
    v, f = m.verts_packed(), m.faces_packed()
    for method in ("cotcurv", "COT", "", None):
        with pytest.raises(ValueError):
            mesh_losses.mesh_laplacian_smoothing(m, method=method)
        with pytest.raises(ValueError):
            mesh_losses.mesh_regularizer(m, laplacian=1.0, method=method)
        with pytest.raises(ValueError):
            ops.mesh_regularizers(v, f, 0.0, 1.0, 0.0, method=method)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mesh_losses.mesh_edge_loss(m, target_length=bad)
        for kw in ({"edge": bad}, {"laplacian": bad}, {"normal": bad}, {"target_length": bad}):
            with pytest.raises(ValueError):
                mesh_losses.mesh_regularizer(m, **kw)
            with pytest.raises(ValueError):
                ops.mesh_regularizers(v, f, **kw)
    with pytest.raises(ValueError):
        ops.mesh_regularizers(torch.rand(3, 2), f, 1.0)
    with pytest.raises(ValueError):
        ops.mesh_edge_lists(torch.tensor([0, 1, 2]), 3)
    with pytest.raises(ValueError):
        ops.mesh_edge_lists(f, 0)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Argument checks run before any device work, so they hold without a GPU."""
    from reni_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(16384)
    p = (ctypes.addressof(buf) + 255) & ~255
    need = lib.reni_mesh_regularizers_workspace_bytes(4, 4, 6)
    assert 256 <= need <= 8192
    ws = lib.reni_mesh_regularizers_workspace_bytes
    assert ws(0, 4, 6) == 0 and ws(4, 0, 6) == 0 and ws(4, 4, -1) == 0 and ws(4, 4, 0) > 0 and ws(2 ** 31, 4, 6) == 0

    def call(V=4, F=4, E=6, H=12, NC=12, ptrs=None, w=(1.0, 1.0, 1.0), target=0.0, method=0, values=p, grad=p, wsp=p, wsn=8192):
        ptrs = [p] * 10 if ptrs is None else ptrs
        return lib.reni_mesh_regularizers(V, F, E, H, NC, *ptrs, w[0], w[1], w[2], target, method, values, grad, wsp, wsn, None)

    who = b"mesh regularizers:"
    for kw in (dict(V=0), dict(F=0), dict(E=-1), dict(H=-1), dict(H=13), dict(NC=-1), dict(NC=13), dict(method=2), dict(method=-1),
               dict(values=None)):
        assert call(**kw) == -1 and lib.reni_last_error().startswith(who), kw
    for i in range(10):
        ptrs = [p] * 10
        ptrs[i] = None
        assert call(ptrs=ptrs) == -1 and lib.reni_last_error().startswith(who) and b"NULL" in lib.reni_last_error()
    for bad in (-1.0, float("nan"), float("inf")):
        for i in range(3):
            w = [1.0, 1.0, 1.0]
            w[i] = bad
            assert call(w=w) == -1 and b"weights" in lib.reni_last_error(), (bad, i)
        assert call(target=bad) == -1 and b"target_length" in lib.reni_last_error()
    assert call(wsp=None, wsn=0) == -2 and call(wsn=need - 1) == -2 and call(wsp=p + 8) == -2  # RENI_EWORKSPACE
    assert lib.reni_last_error().startswith(who) and b"workspace" in lib.reni_last_error()


def test_meshreg_unit_has_no_float_atomics():
    src = open(os.path.join(ROOT, "reni_amd", "csrc", "reni_tu_meshreg.hip")).read()
    assert "atomic" not in src.replace("no float atomic", "")


def test_meshreg_translation_unit_isa_audit():
    """reni_tu_meshreg.hip with build.sh's flags: it compiles; no MFMA / transcendental / SDWA hazard, no scratch."""
    import re
    import subprocess
    import tempfile
    from tests import isa_audit
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "meshreg.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_meshreg.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    for k in ("k_mr_face", "k_mr_edge", "k_mr_lap", "k_mr_reduce", "k_mr_gather"):
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text and "atomic" not in text
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) >= 5 and all(int(n) == 0 for n in sizes)  # one per kernel
