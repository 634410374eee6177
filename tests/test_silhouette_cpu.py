"""CPU tests of the soft silhouette (reni_tu_silhouette.hip, ops.soft_silhouette, ops.soft_silhouette_backward): the float64
reference of tests/silhouette_ref.py against central differences, its hand-written closed form against its autograd, the
share of undecided pairs, the error-budget constants, and everything of the new entry points that holds without a GPU
(declarations, argument checks, no CPU path, the unit's emitted code)."""
import ctypes
import os

import pytest
import torch

from tests import silhouette_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reni_soft_silhouette_workspace_bytes", "reni_soft_silhouette", "reni_soft_silhouette_backward_workspace_bytes",
         "reni_soft_silhouette_backward")
COMBOS = tuple((key, name) for key in R.CASES for name in R.SETTINGS)
FD_REL = 1e-4  # a pair this close to a flip may flip within the step of the central differences (its effect: below 1e-5)


def _combo_id(c):
    return R.case_id(c[0]) + "-" + c[1]


def _members(key, name):
    v, f, Rm, T, S, tanh = R.inputs(key)
    sigma, r = R.setting(name, S)
    with torch.no_grad():
        idx, x, y, _ = R.taking_part(v, f, Rm, T, tanh)
        return idx, R.pairs(x, y, S, r)["either"]


def _on_edge(key, name):
    v, f, Rm, T, S, tanh = R.inputs(key)
    sigma, r = R.setting(name, S)
    with torch.no_grad():
        _, x, y, _ = R.taking_part(v, f, Rm, T, tanh)
        return int(R.pairs(x, y, S, r)["on_edge"].sum())


def test_the_cases_are_what_they_claim():
    assert len(R.CASES) == 14 and ("tiny_normal", 16) not in R.CASES
    assert R.count_pairs(("tetra", 8), "sharp")[0] == 86
    assert R.count_pairs(("ico", 33), "sharp")[0] == 2129
    assert R.count_pairs(("fan", 16), "sharp")[0] == 15396
    assert R.count_pairs(("ico", 16), "sharp") == (1240, 6)
    _, m = _members(("fan", 16), "sharp")
    assert int(m.sum(dim=1).max()) == 300  # every face of the fan takes part at one pixel: the product crosses the 256-face chunk
    idx, _ = _members(("soup", 17), "sharp")
    assert idx.numel() == 54 and R.case("soup", 17)[1].shape[0] == 60
    for name in R.SETTINGS:
        assert R.count_pairs(("behind", 16), name) == (0, 0)  # nothing takes part
        idx, m = _members(("cover", 33), name)
        assert idx.tolist() == [0] and bool(m.all())  # one face under everything
    for name in ("sharp", "inside_only", "short_cut"):
        out = R.reference_lo(("cover", 33), name)
        assert (out["trans"] == 0).all() and (out["alpha"] == 1).all()
    v, f, *_ = R.case("unreferenced", 16)
    assert not (f == R.UNREFERENCED).any()
    assert [R.case("strip", V)[0].shape[0] for V in (255, 256, 257)] == [255, 256, 257]
    # wide: the footprint sqrt(r) is more than a tile, so a face reaches tiles that its own box does not touch
    S = 33
    sigma, r = R.setting("wide", S)
    assert r ** 0.5 / (2.0 / S) > 16 and 1.0 < R.setting("sharp", S)[1] ** 0.5 / (2.0 / S) < 2.0
    sigma, r = R.setting("short_cut", S)
    assert r == sigma and abs(1.0 / (1.0 + 2.718281828) - 0.27) < 0.01  # the cut-off sits where prob is about 0.27
    assert R.setting("inside_only", S)[1] == 0.0


def test_undecided_pairs_stay_under_the_cap():
    worst = 0.0
    for key, name in COMBOS:
        n, u = R.count_pairs(key, name)
        share = u / n if n else 0.0
        worst = max(worst, share)
        print(f"{_combo_id((key, name))}: {u} undecided of {n} participating pairs ({100 * share:.2f} %)")
        assert share <= R.UNDECIDED_CAP, (key, name, u, n)
    print(f"worst share {100 * worst:.2f} %")


def test_reference_autograd_matches_central_differences():
    """<g, d> against (f(v + h d) - f(v - h d)) / 2h for random directions d, on every case and setting with no pair within
    FD_REL of a flip and no pixel centre on an edge's line beyond r (the function is smooth across the step there)."""
    ran = 0
    h = 1e-7
    for key, name in COMBOS:
        n, u = R.count_pairs(key, name, FD_REL)
        if n == 0 or u > 0 or _on_edge(key, name) or key[0] == "bad_faces":  # (its collinear face crosses |area| = 1e-8 within the step)
            continue
        ran += 1
        v, f, Rm, T, S, tanh = R.inputs(key)
        sigma, r = R.setting(name, S)
        gA = R.upstream(key, name)
        g = R.reference(key, name, gA)
        terms = R.reference_lo(key, name, gA)["terms_g"]
        gen = torch.Generator().manual_seed(7)
        for _ in range(3):
            d = torch.randn(v.shape[0], 3, generator=gen, dtype=torch.float64)
            with torch.no_grad():
                vals = [float((R.soft_alpha(v + s * h * d, f, Rm, T, S, tanh, sigma, r)[0] * gA).sum()) for s in (1.0, -1.0)]
            fd = (vals[0] - vals[1]) / (2 * h)
            scale = float((terms * d.abs()).sum())
            assert abs(fd - float((g * d).sum())) <= 1e-6 * scale + 1e-12, (key, name, fd, float((g * d).sum()))
    print(f"central differences on {ran} of {len(COMBOS)} cases x settings")
    assert ran >= 12


@pytest.mark.parametrize("combo", COMBOS, ids=_combo_id)
def test_closed_form_matches_autograd_in_float64(combo):
    """the hand-written chain (the kernels' structure) is the autograd gradient, far below the float32 budget, under either
    choice of the undecided pairs"""
    key, name = combo
    gA = R.upstream(key, name)
    v, f, Rm, T, S, tanh = R.inputs(key)
    sigma, r = R.setting(name, S)
    for choice, fn in (("lo", R.reference_lo), ("hi", R.reference_hi)):
        ref = R.reference(key, name, gA, choice)
        out = fn(key, name, gA)
        with torch.no_grad():
            alpha, trans = R.soft_alpha(v, f, Rm, T, S, tanh, sigma, r, choice)
        assert float((out["alpha"] - alpha).abs().max()) <= 1e-12 and float((out["trans"] - trans).abs().max()) <= 1e-12
        assert (out["terms_g"] >= ref.abs() * (1 - 1e-9)).all()
        # (autograd's product rule divides by the factors of a 300-face product: a few 1e-12 of the scale in float64)
        assert R.error_ratio(out["g"], ref, ref, out["terms_g"], True) < 1e-3


def test_exact_zeros_of_the_reference():
    key = ("unreferenced", 16)
    g = R.reference(key, "sharp", R.upstream(key, "sharp"))
    assert (g[R.UNREFERENCED] == 0).all() and (g != 0).any()
    for name in R.SETTINGS:
        key = ("behind", 16)
        out = R.reference_lo(key, name, R.upstream(key, name))
        assert (out["g"] == 0).all() and (out["alpha"] == 0).all() and (out["trans"] == 1).all()
    for name in ("sharp", "inside_only", "short_cut"):  # alpha = 1 everywhere: trans = 0 and the gradient is exactly 0
        key = ("cover", 33)
        assert (R.reference_lo(key, name, R.upstream(key, name))["g"] == 0).all()


def test_error_budget_constants_are_the_measured_ones():
    """K = 4 x the worst ratio of the float32 CPU evaluation, hard-coded in the case file: still what is measured."""
    ra, rg = R.float32_ratios()
    print(f"float32 closed form, worst error / (2^-23 sum |terms|): alpha {ra:.4g}, g_verts {rg:.4g}")
    assert R.K_ALPHA / 2 <= 4 * ra <= R.K_ALPHA * 1.001
    assert R.K_GVERTS / 2 <= 4 * rg <= R.K_GVERTS * 1.001


def test_fit_reference_is_the_recorded_one():
    iou0, iou1, losses = R.fit_reference()
    print(f"float64 fit: hard IoU {iou0:.4f} -> {iou1:.4f}, loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert abs(iou0 - R.FIT_IOU_START) < 1e-9 and abs(iou1 - R.FIT_IOU_END) < 1e-9
    assert iou1 > iou0 + 0.1 and losses[-1] < losses[0]


def test_silhouette_iou_is_the_soft_iou():
    from reni_amd.mesh import silhouette_iou
    g = torch.Generator().manual_seed(1)
    a, m = torch.rand(8, 8, generator=g), (torch.rand(8, 8, generator=g) > 0.5)
    want = 1.0 - (a * m).sum() / (a + m - a * m).sum()
    assert abs(float(silhouette_iou(a, m)) - float(want)) < 1e-6
    assert abs(float(silhouette_iou(a, m.float().reshape(-1))) - float(R.soft_iou_loss(a.reshape(-1), m.reshape(-1)))) < 1e-6
    assert float(silhouette_iou(m.float(), m)) < 1e-6
    with pytest.raises(ValueError):
        silhouette_iou(a, m[:4])


def test_header_integration_build_and_binding_name_the_entry_points():
    from reni_amd import _lib
    h = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name + "(" in h and name in _lib.EXPORTS and name in doc
    build = open(os.path.join(ROOT, "reni_amd", "csrc", "build.sh")).read()
    assert " silhouette " in build and "_build/silhouette.o" in build
    for word in ("blur_radius", "K-nearest", "straddles", "ascending face order", "-trans_p prob_f / sigma"):
        assert word in h, word


def test_cpu_tensors_raise():
    from reni_amd import _lib, ops
    from reni_amd.mesh import FoVPerspectiveCameras, MeshRasterizer, Meshes, RasterizationSettings
    v, f = torch.rand(3, 3), torch.tensor([[0, 1, 2]])
    I, Z = torch.eye(3), torch.zeros(3)
    with pytest.raises(_lib.RENILibraryError):
        ops.soft_silhouette(v, f, I, Z, 4, 0.5, 1e-3, 1e-2)
    with pytest.raises(_lib.RENILibraryError):
        ops.soft_silhouette_backward(v, f, I, Z, 4, 0.5, 1e-3, 1e-2, torch.ones(16), torch.ones(16))
    with pytest.raises(_lib.RENILibraryError):
        MeshRasterizer(FoVPerspectiveCameras(), RasterizationSettings(image_size=4)).silhouette(Meshes(verts=[v], faces=[f]))
    with pytest.raises(ValueError):  # the hard rasteriser keeps its settings
        RasterizationSettings(image_size=4, blur_radius=1e-3)


def test_bad_arguments_raise_value_errors():
    from reni_amd import ops
    v, f = torch.rand(3, 3), torch.tensor([[0, 1, 2]])
    I, Z, one = torch.eye(3), torch.zeros(3), torch.ones(16)
    for args in ((torch.rand(3, 2), f, I, Z, 4, 0.5, 1e-3, 1e-2), (v, torch.tensor([0, 1, 2]), I, Z, 4, 0.5, 1e-3, 1e-2),
                 (v, f, torch.eye(2), Z, 4, 0.5, 1e-3, 1e-2), (v, f, I, Z, 0, 0.5, 1e-3, 1e-2), (v, f, I, Z, 4, 0.5, 0.0, 1e-2),
                 (v, f, I, Z, 4, 0.5, float("nan"), 1e-2), (v, f, I, Z, 4, 0.5, 1e-3, -1.0), (v, f, I, Z, 4, 0.5, 1e-3, float("inf"))):
        with pytest.raises(ValueError):
            ops.soft_silhouette(*args)
        with pytest.raises(ValueError):
            ops.soft_silhouette_backward(*args, one, one)
    for tr, gA in ((one[:15], one), (one, torch.ones(17)), (None, one)):
        with pytest.raises(ValueError):
            ops.soft_silhouette_backward(v, f, I, Z, 4, 0.5, 1e-3, 1e-2, tr, gA)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Argument checks run before any device work, so they hold without a GPU."""
    from reni_amd import _lib
    lib = _lib.load()
    Rm, T = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (ctypes.c_float * 3)()
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 255) & ~255
    need_f = lib.reni_soft_silhouette_workspace_bytes(3, 1, 8, 8)
    need_b = lib.reni_soft_silhouette_backward_workspace_bytes(3, 1, 8, 8)
    assert 64 <= need_f <= 4096 and 64 + 36 <= need_b <= 4096 and need_b > need_f
    for fn in (lib.reni_soft_silhouette_workspace_bytes, lib.reni_soft_silhouette_backward_workspace_bytes):
        assert fn(0, 1, 8, 8) == 0 and fn(3, 0, 8, 8) == 0

    def fwd(V=3, F=1, tanh=0.5, H=8, W=8, sigma=1e-3, r=1e-2, ptrs=None, Rp=Rm, Tp=T, ws=p, wsn=4096):
        ptrs = [p] * 4 if ptrs is None else ptrs
        return lib.reni_soft_silhouette(V, F, ptrs[0], ptrs[1], Rp, Tp, tanh, H, W, sigma, r, ptrs[2], ptrs[3], ws, wsn, None)

    def bwd(V=3, F=1, tanh=0.5, H=8, W=8, sigma=1e-3, r=1e-2, ptrs=None, Rp=Rm, Tp=T, ws=p, wsn=4096):
        ptrs = [p] * 7 if ptrs is None else ptrs
        return lib.reni_soft_silhouette_backward(V, F, ptrs[0], ptrs[1], Rp, Tp, tanh, H, W, sigma, r, *ptrs[2:], ws, wsn, None)

    for call, who, n in ((fwd, b"soft silhouette:", 4), (bwd, b"soft silhouette backward:", 7)):
        for kw in (dict(V=0), dict(F=0), dict(H=8, W=9), dict(H=0, W=0), dict(tanh=0.0), dict(tanh=float("nan"))):
            assert call(**kw) == -1 and lib.reni_last_error().startswith(who), kw
        for kw in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("inf")), dict(sigma=float("nan"))):
            assert call(**kw) == -1 and lib.reni_last_error().startswith(who) and b"sigma" in lib.reni_last_error(), kw
        for kw in (dict(r=-1e-9), dict(r=float("inf")), dict(r=float("nan"))):
            assert call(**kw) == -1 and b"blur_radius" in lib.reni_last_error(), kw
        for i in range(n):
            ptrs = [p] * n
            ptrs[i] = None
            assert call(ptrs=ptrs) == -1 and b"NULL" in lib.reni_last_error()
        assert call(Rp=None) == -1 and b"NULL" in lib.reni_last_error()
        assert call(Tp=None) == -1 and b"NULL" in lib.reni_last_error()
        assert call(ws=None, wsn=0) == -2 and call(wsn=32) == -2 and call(ws=p + 8) == -2  # RENI_EWORKSPACE
        assert lib.reni_last_error().startswith(who) and b"workspace" in lib.reni_last_error()
    assert bwd(wsn=64) == -2  # enough for the forward's records, short of the backward's


def test_silhouette_unit_has_no_float_atomics():
    src = open(os.path.join(ROOT, "reni_amd", "csrc", "reni_tu_silhouette.hip")).read()
    assert "atomic" not in src.replace("no float atomic", "")


def test_silhouette_translation_unit_isa_audit():
    """reni_tu_silhouette.hip with build.sh's flags: it compiles; no MFMA / transcendental / SDWA hazard, no scratch."""
    import re
    import subprocess
    import tempfile
    from tests import isa_audit
    csrc = os.path.join(ROOT, "reni_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "silhouette.s")
        pr = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm",
                             "-amdgpu-spill-vgpr-to-agpr=0", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                             os.path.join(csrc, "reni_tu_silhouette.hip"), "-o", out], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stderr[-2000:]
        text = open(out).read()
    for k in ("k_sil_setup", "k_sil_tile", "k_sil_face", "k_sil_vertex"):
        assert k in text
    assert isa_audit.violations(text) == []
    assert isa_audit.trans_to_valu(text) == []
    assert isa_audit.sdwa_partial_dst(text) == []
    assert "scratch_" not in text and "atomic" not in text
    for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", text):
        assert int(m.group(1)) == 0
