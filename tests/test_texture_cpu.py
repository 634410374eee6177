"""CPU tests of the UV-texture path (no GPU is touched): the float64 restatement (tests/texture_ref.py) against
torch's grid_sample, its own invariants, the fp32 emulation the GPU tolerance comes from, ``load_obj_uv`` and ``Meshes``
UVs, every argument error of the new C entry points through ctypes, and the Python layer's validation."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import texture_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reni_mesh_pixel_uv", "reni_texture_taps", "reni_texture_pyramid", "reni_texture_pyramid_backward", "reni_texture_fetch",
         "reni_texture_fetch_backward")
F64 = torch.float64


def _uv_set(n, seed):
    g = torch.Generator().manual_seed(seed)
    uv = torch.rand(n, 2, generator=g, dtype=F64) * 1.6 - 0.3
    uv[:4] = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0]], dtype=F64)
    return uv


@pytest.mark.parametrize("size", [(1, 1), (1, 4), (2, 2), (3, 5), (8, 16)])
@pytest.mark.parametrize("align", [False, True])
def test_restatement_is_grid_sample_with_border_padding(size, align):
    H, W = size
    uv = _uv_set(300, 3)
    tex = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(4), dtype=F64)
    got = TR.sample_ref(tex, uv, 1, align_corners=align)
    grid = torch.stack([2 * uv[:, 0] - 1, 1 - 2 * uv[:, 1]], 1).reshape(1, 1, -1, 2)
    want = torch.nn.functional.grid_sample(tex.permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="border",
                                           align_corners=align)[0, :, 0].t()
    assert float((got - want).abs().max()) <= 1e-14


def test_repeat_is_periodic_and_continuous_across_the_seam():
    tex = torch.rand(8, 4, 2, generator=torch.Generator().manual_seed(5), dtype=F64)
    uv = _uv_set(200, 6)
    base = TR.sample_ref(tex, uv, 3, wrap="repeat", lod_bias=0.6)
    for k in ((1.0, 0.0), (-2.0, 3.0), (5.0, -7.0)):
        moved = TR.sample_ref(tex, uv + torch.tensor(k, dtype=F64), 3, wrap="repeat", lod_bias=0.6)
        assert float((moved - base).abs().max()) <= 1e-13
    e = 1e-9
    a = TR.sample_ref(tex, torch.tensor([[1.0 - e, 0.3], [0.2, 1.0 - e]], dtype=F64), 1, wrap="repeat")
    b = TR.sample_ref(tex, torch.tensor([[e, 0.3], [0.2, e]], dtype=F64), 1, wrap="repeat")
    assert float((a - b).abs().max()) <= 1e-7


def test_weights_sum_to_one_on_valid_pixels_and_are_zero_on_invalid_ones():
    for c in TR.lookup_cases()[::5]:
        idx, wgt = TR.taps_ref(c["uv"], c["H0"], c["W0"], c["L"], jac=c["jac"], valid=c["valid"], wrap=c["wrap"],
                               align_corners=c["align"], lod_bias=c["lod_bias"])
        ok = torch.isfinite(c["uv"]).all(1) & (c["valid"] >= 0)
        E = TR.level_offsets(c["H0"], c["W0"], c["L"])[-1]
        assert int(idx.min()) >= 0 and int(idx.max()) < E
        assert float((wgt[ok].sum(1) - 1).abs().max()) <= 1e-14 and float(wgt.min()) >= 0.0
        if bool((~ok).any()):
            assert float(wgt[~ok].abs().max()) == 0.0 and int(idx[~ok].abs().max()) == 0
            out = TR.fetch_ref(TR.pyramid_ref(c["tex"].to(F64), c["L"]), idx, wgt)
            assert float(out[~ok].abs().max()) == 0.0


def test_pyramid_of_a_constant_is_constant_and_its_transpose_is_the_autograd():
    for H, W in ((16, 4), (1, 8), (8, 1), (64, 64), (2, 2)):
        L = TR.full_levels(H, W)
        pyr = TR.pyramid_ref(torch.full((H, W, 2), 0.7, dtype=F64), L)
        assert pyr.shape[0] == TR.level_offsets(H, W, L)[-1] and float((pyr - 0.7).abs().max()) <= 1e-15
        assert TR.level_sizes(H, W, L)[-1] == (1, 1)
        # every level keeps the mean
        tex = torch.rand(H, W, 1, generator=torch.Generator().manual_seed(H + W), dtype=F64)
        assert abs(float(TR.pyramid_ref(tex, L)[-1, 0]) - float(tex.mean())) <= 1e-14


@pytest.mark.parametrize("k", [-2, -1, 0, 1, 2, 3])
def test_lambda_of_an_analytic_quad(k):
    """A unit quad whose u runs over the image's columns and v over its rows, seen so that one texel of a 64 x 64 texture
    covers 2^-k ... i.e. one pixel step moves 2^k texels: lambda = k (clamped at 0), from the Jacobian of pixel_uv_ref."""
    S, H0 = 16, 64
    tan = math.tan(math.radians(30.0))
    texels_per_pixel = 2.0 ** k
    # the quad spans NDC [-a, a]^2 at z = 1 / tan (so NDC = x, y); it carries uv [0, 1]^2: du/dNDC = 1 / (2a), one pixel is
    # 2 / S in NDC -> du/dcol = 1 / (a S) (in size), times H0 texels = texels_per_pixel
    a = H0 / (S * texels_per_pixel)
    z = 1.0 / tan
    verts = torch.tensor([[-a, -a, z], [a, -a, z], [a, a, z], [-a, a, z]], dtype=torch.float32)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]])
    vt = torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    P = S * S
    p2f = torch.zeros(P, dtype=torch.int64)
    bary = torch.full((P, 3), 1.0 / 3.0)
    uv, jac, valid = TR.pixel_uv_ref(verts, faces, vt, faces, torch.eye(3), torch.zeros(3), tan, S, p2f, bary)
    assert bool(valid.all())
    # +x is left in NDC: u falls with the column; v falls with the row
    want = torch.tensor([-1.0 / (a * S), 0.0, 0.0, -1.0 / (a * S)], dtype=F64)
    assert float((jac - want).abs().max()) <= 1e-6 * float(want.abs().max())
    lam = TR.lod_ref(jac.float(), P, H0, H0, 7, 0.0)
    assert float((lam - max(k, 0)).abs().max()) <= 1e-5
    assert float((TR.lod_ref(jac.float(), P, H0, H0, 7, 1.5) - min(max(k + 1.5, 0), 6)).abs().max()) <= 1e-5
    # no footprint, zero and non-finite footprints
    assert TR.lod_ref(None, 3, 8, 8, 4, 2.25).tolist() == [2.25] * 3 and TR.lod_ref(None, 1, 8, 8, 4, 9.0).tolist() == [3.0]
    bad = torch.tensor([[0.0, 0, 0, 0], [float("nan"), 0, 0, 1], [float("inf"), 0, 0, 1]])
    assert TR.lod_ref(bad, 3, 8, 8, 4, 1.0).tolist() == [0.0, 0.0, 0.0]


def test_pixel_uv_reference_marks_invalid_pixels():
    verts = torch.tensor([[-1.0, -1, 3], [1, -1, 3], [1, 1, 3], [-1, 1, 3]])
    faces = torch.tensor([[0, 1, 2], [0, 2, 3], [0, 1, 3]])
    vt = torch.tensor([[0.0, 0], [1, 0], [1, 1], [0, 1], [float("nan"), 0.5]])
    ft = torch.tensor([[0, 1, 2], [0, 2, -1], [0, 1, 4]])
    p2f = torch.tensor([0, 1, 2, -1])
    bary = torch.tensor([[0.2, 0.3, 0.5]] * 4)
    uv, jac, valid = TR.pixel_uv_ref(verts, faces, vt, ft, torch.eye(3), torch.zeros(3), 0.5, 2, p2f, bary)
    assert valid.tolist() == [True, False, False, False]
    assert float(uv[1:].abs().max()) == 0.0 and float(jac[1:].abs().max()) == 0.0
    assert torch.allclose(uv[0], torch.tensor([0.8, 0.5], dtype=F64), atol=1e-7)


def test_fp32_emulation_gives_the_tolerance_constants():
    """K and K' of the GPU test: four times the worst ratio of the fp32 emulation's error to the unit bounds over the GPU
    test's own cases.  The emulation rounds every product and sum on its own, so it is no better than the device."""
    K, Kp, worst_f, worst_g = TR.emulation_constants()
    print(f"texture emulation: worst fetch ratio {worst_f:.4f} (K = {K:.4f}), worst gradient ratio {worst_g:.4f} (K' = {Kp:.4f})")
    assert 0.0 < worst_f < 1e3 and 0.0 < worst_g < 1e3 and K == 4 * worst_f and Kp == 4 * worst_g
    # the emulation's taps are the restatement's up to rounding: same indices wherever no coordinate sits on a border
    c = TR.make_case(16, 4, 3, 257, 3, "clamp", False, 7)
    ri, rw = TR.taps_ref(c["uv"], 16, 4, 3, jac=c["jac"], valid=c["valid"])
    ei, ew = TR.taps_emulated(c["uv"].numpy(), 16, 4, 3, jac=c["jac"].numpy(), valid=c["valid"].numpy())
    assert float(np.abs(ew.astype(np.float64) - rw.numpy()).max()) <= 1e-4 or (ei != ri.numpy()).any()
    assert (ei == ri.numpy()).mean() > 0.99


# ---- OBJ files and Meshes ---------------------------------------------------------------------------------------------
def test_load_obj_uv_mixed_corners_negative_indices_and_fans(tmp_path):
    from reni_amd.mesh import load_obj, load_obj_uv
    p = tmp_path / "m.obj"
    p.write_text("""# a quad, a textured triangle, corners of every kind
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0 0
vt 1 0 0.5
vt 1 1
vt 0 1
vt 0.5 0.5
vt 0.25 0.75
vn 0 0 1
f 1/1 2/2 3/3 4/4
f 1/1/1 2/2/1 3/5/1
f 1//1 2//1 3//1
f 1 2 4
f -4/-6 -3/-5 -1/-1
v 2 2 2
vt 0.9 0.1
f -1/-1 1/1 2/7
""")
    v, f, vt, ft = load_obj_uv(str(p))
    v0, f0 = load_obj(str(p))
    assert torch.equal(v, v0) and torch.equal(f, f0)            # load_obj's geometry, unchanged
    assert v.shape == (5, 3) and vt.shape == (7, 2) and f.shape == ft.shape == (7, 3)   # Tn differs from V
    assert vt.dtype == torch.float32 and ft.dtype == torch.int64
    assert ft.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [-1, -1, -1], [-1, -1, -1], [0, 1, 5], [6, 0, 6]]
    assert f.tolist()[5] == [0, 1, 3] and f.tolist()[6] == [4, 0, 1]
    assert vt[1].tolist() == [1.0, 0.0]                          # a third vt value is ignored
    q = tmp_path / "bad.obj"
    q.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/0 2/1 3/1\n")
    with pytest.raises(ValueError, match="start at 1"):
        load_obj_uv(str(q))
    q.write_text("v 0 0 0\nvt 0\n")
    with pytest.raises(ValueError, match="two values"):
        load_obj_uv(str(q))
    with pytest.raises(FileNotFoundError):
        load_obj_uv(str(tmp_path / "none.obj"))
    # the teapot has no vt lines: geometry as before, no UVs, every face untextured
    v, f, vt, ft = load_obj_uv(os.path.join(ROOT, "tests", "golden", "teapot.obj"))
    assert vt.shape == (0, 2) and ft.shape == f.shape and int(ft.max()) == -1


def test_meshes_with_and_without_uvs():
    from reni_amd.mesh import Meshes, MeshRasterizer
    v, f = torch.rand(4, 3), torch.tensor([[0, 1, 2], [0, 2, 3]])
    m = Meshes(verts=[v], faces=[f])
    assert m.verts_uvs_packed() is None and m.faces_uvs_packed() is None and torch.equal(m.verts_packed(), v)
    vt, ft = torch.rand(5, 2), torch.tensor([[0, 1, 2], [0, 4, -1]])
    m = Meshes(verts=[v], faces=[f], verts_uvs=[vt], faces_uvs=[ft])
    assert torch.equal(m.verts_uvs_packed(), vt) and torch.equal(m.faces_uvs_packed(), ft)
    for bad in ({"verts_uvs": [vt]}, {"faces_uvs": [ft]}, {"verts_uvs": [vt[:, :1]], "faces_uvs": [ft]},
                {"verts_uvs": [vt], "faces_uvs": [ft[:1]]}, {"verts_uvs": [vt, vt], "faces_uvs": [ft]}):
        with pytest.raises(ValueError):
            Meshes(verts=[v], faces=[f], **bad)
    with pytest.raises(ValueError, match="no texture coordinates"):
        MeshRasterizer().pixel_uv(Meshes(verts=[v], faces=[f]))
    with pytest.raises(ValueError, match="no texture coordinates"):
        MeshRasterizer().texture_taps(Meshes(verts=[v], faces=[f]), size=(4, 4))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_declared_and_documented():
    from reni_amd import _lib
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"^int " + n + r"\(", header, re.M) and n in _lib.EXPORTS and n in integration, n
        assert getattr(lib, n) is not None
    assert re.search(r"#define\s+RENI_TEX_CLAMP\s+0\b", header) and re.search(r"#define\s+RENI_TEX_REPEAT\s+1\b", header)
    assert _lib.TEX_WRAP == {"clamp": 0, "repeat": 1}


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from reni_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    p = 1 << 20  # a non-NULL, aligned address: nothing dereferences it before the checks are through
    R, T = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (ctypes.c_float * 3)(0, 0, 0)

    def rejected(rc, keyword):
        return rc == EINVAL and keyword in lib.reni_last_error()

    def puv(V=4, F=2, Tn=4, verts=p, faces=p, vt=p, ft=p, R=R, T=T, tan=0.5, S=8, p2f=p, bary=p, uv=p, jac=p, valid=None):
        return lib.reni_mesh_pixel_uv(V, F, Tn, verts, faces, vt, ft, R, T, tan, S, p2f, bary, uv, jac, valid, None)

    for size in ({"V": 0}, {"F": 0}, {"Tn": 0}, {"S": 0}, {"S": -3}):
        assert rejected(puv(**size), b">= 1")
    assert rejected(puv(S=1 << 14), b"too large") and rejected(puv(F=1 << 30), b"too large")
    for name in ("verts", "faces", "vt", "ft", "R", "T", "p2f", "bary", "uv", "jac"):
        assert rejected(puv(**{name: None}), b"NULL"), name
    for tan in (0.0, -1.0, float("nan"), float("inf")):
        assert rejected(puv(tan=tan), b"tan_half_fov")

    def taps(P=10, uv=p, jac=None, valid=None, L=1, H0=8, W0=8, bias=0.0, wrap=0, align=0, idx=p, wgt=p):
        return lib.reni_texture_taps(P, uv, jac, valid, L, H0, W0, bias, wrap, align, idx, wgt, None)

    assert rejected(taps(P=0), b">= 1") and rejected(taps(P=1 << 28), b"too large")
    for size in ({"L": 0}, {"H0": 0}, {"W0": -1}):
        assert rejected(taps(**size), b">= 1")
    assert rejected(taps(H0=1 << 16, W0=1 << 15), b"E < 2^31") and rejected(taps(H0=1 << 40, W0=1), b"E < 2^31")
    assert rejected(taps(H0=3, W0=5, L=2), b"powers of two") and rejected(taps(H0=8, W0=6, L=2), b"powers of two")
    assert rejected(taps(H0=8, W0=16, L=6), b"log2") and rejected(taps(H0=1, W0=1, L=2), b"log2")
    assert rejected(taps(wrap=2), b"wrap") and rejected(taps(wrap=-1), b"wrap") and rejected(taps(align=2), b"align_corners")
    assert rejected(taps(align=1, L=2), b"align_corners") and rejected(taps(align=1, wrap=1), b"align_corners")
    for bias in (float("nan"), float("inf")):
        assert rejected(taps(bias=bias), b"lod_bias")
    for name in ("uv", "idx", "wgt"):
        assert rejected(taps(**{name: None}), b"NULL"), name
    assert rejected(taps(idx=p + 4), b"16-byte aligned") and rejected(taps(wgt=p + 8), b"16-byte aligned")

    for fn in (lib.reni_texture_pyramid, lib.reni_texture_pyramid_backward):
        assert rejected(fn(0, 8, 8, 3, p, None), b">= 1") and rejected(fn(2, 8, 0, 3, p, None), b">= 1")
        assert rejected(fn(2, 3, 5, 3, p, None), b"powers of two") and rejected(fn(5, 8, 8, 3, p, None), b"log2")
        assert rejected(fn(1, 1 << 16, 1 << 15, 3, p, None), b"E < 2^31")
        assert rejected(fn(2, 8, 8, 0, p, None), b"C must be") and rejected(fn(2, 8, 8, 9, p, None), b"C must be")
        assert rejected(fn(2, 8, 8, 3, None, None), b"NULL")

    def fetch(P=10, E=64, C=3, tex=p, idx=p, wgt=p, out=p):
        return lib.reni_texture_fetch(P, E, C, tex, idx, wgt, out, None)

    def fbwd(P=10, E=64, C=3, g=p, wgt=p, order=p, offsets=p, plain=0, out=p):
        return lib.reni_texture_fetch_backward(P, E, C, g, wgt, order, offsets, plain, out, None)

    for fn in (fetch, fbwd):
        for size in ({"P": 0}, {"E": 0}, {"C": 0}):
            assert rejected(fn(**size), b">= 1")
        assert rejected(fn(C=9), b"C must be <= 8")
        assert rejected(fn(E=1 << 31), b"too large") and rejected(fn(P=1 << 28), b"too large")
    for name in ("tex", "idx", "wgt", "out"):
        assert rejected(fetch(**{name: None}), b"NULL"), name
    assert rejected(fetch(idx=p + 4), b"16-byte aligned")
    for name in ("g", "wgt", "order", "offsets", "out"):
        assert rejected(fbwd(**{name: None}), b"NULL"), name
    assert rejected(fbwd(plain=2), b"plain")


# ---- the Python layer -------------------------------------------------------------------------------------------------
def test_python_argument_errors_come_before_the_library():
    from reni_amd import _lib, ops, textures
    assert ops.texture_levels(16, 4)[:2] == (5, 64 + 16 + 4 + 2 + 1) and ops.texture_levels(3, 5)[0] == 1
    assert ops.texture_levels(64, 64, 3) == (3, 64 * 64 + 32 * 32 + 16 * 16, [(64, 64), (32, 32), (16, 16)])
    assert ops.texture_levels(1, 8)[2] == [(1, 8), (1, 4), (1, 2), (1, 1)]
    for bad in ((3, 5, 2), (16, 4, 6), (0, 4, None), (8, 8, 0), (1 << 16, 1 << 15, 1)):
        with pytest.raises(ValueError):
            ops.texture_levels(*bad)
    uv = torch.rand(6, 2)
    with pytest.raises(ValueError, match="wrap"):
        ops.texture_taps(uv, (4, 4), wrap="mirror")
    with pytest.raises(ValueError, match="align_corners"):
        ops.texture_taps(uv, (4, 4), align_corners=True)            # the full pyramid of 4 x 4 has 3 levels
    with pytest.raises(ValueError, match="align_corners"):
        ops.texture_taps(uv, (4, 4), 1, wrap="repeat", align_corners=True)
    with pytest.raises(ValueError, match="lod_bias"):
        ops.texture_taps(uv, (4, 4), lod_bias=float("nan"))
    with pytest.raises(ValueError, match=r"\[P, 2\]"):
        ops.texture_taps(torch.rand(6, 3), (4, 4))
    with pytest.raises(ValueError, match="jac"):
        ops.texture_taps(uv, (4, 4), jac=torch.rand(6, 3))
    with pytest.raises(ValueError, match="pix_valid"):
        ops.texture_taps(uv, (4, 4), pix_valid=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="uv.*require grad"):
        ops.texture_taps(uv.clone().requires_grad_(True), (4, 4))
    with pytest.raises(ValueError, match="jac.*require grad"):
        ops.texture_taps(uv, (4, 4), jac=torch.rand(6, 4, requires_grad=True))
    with pytest.raises(ValueError, match="lod_bias.*require grad"):
        textures.make_taps(uv, (4, 4), lod_bias=torch.tensor(0.5, requires_grad=True))
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        ops.texture_taps(uv, (4, 4))                                 # well-formed on the CPU: there is no CPU path
    idx, wgt = torch.zeros(6, 8, dtype=torch.int32), torch.zeros(6, 8)
    order, offsets = ops.texture_table(idx, 21)                      # plain torch: works on the CPU
    assert order.tolist() == list(range(48)) and offsets.tolist() == [0] + [48] * 21 and offsets.dtype == torch.int64
    # with the weights, taps of weight 0 sit behind offsets[E]: outside every texel's range
    w2, i2 = wgt.clone(), idx.clone()
    w2[1, 0], w2[4, 3], i2[4, 3] = 0.5, 0.25, 7
    order, offsets = ops.texture_table(i2, 21, w2)
    assert order[:2].tolist() == [8, 35] and offsets.tolist() == [0] + [1] * 7 + [2] * 14 and sorted(order.tolist()) == list(range(48))
    with pytest.raises(ValueError, match="tap_weight"):
        ops.texture_table(idx, 21, wgt[:5])
    order, offsets = ops.texture_table(idx, 21)
    with pytest.raises(ValueError, match="int32"):
        ops.texture_table(idx.long(), 21)
    with pytest.raises(ValueError, match="tap_index"):
        ops.texture_fetch(torch.rand(21, 3), idx.long(), wgt)
    with pytest.raises(ValueError, match="C <= 8"):
        ops.texture_fetch(torch.rand(21, 9), idx, wgt)
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        ops.texture_fetch(torch.rand(21, 3), idx, wgt)
    with pytest.raises(ValueError, match="grad_out"):
        ops.texture_fetch_backward(torch.rand(5, 3), wgt, (order, offsets), 21)
    with pytest.raises(ValueError, match="table"):
        ops.texture_fetch_backward(torch.rand(6, 3), wgt, (order[:-1], offsets), 21)
    with pytest.raises(ValueError, match="table"):
        ops.texture_fetch_backward(torch.rand(6, 3), wgt, (order, offsets), 22)
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        ops.texture_fetch_backward(torch.rand(6, 3), wgt, (order, offsets), 21)
    for bad in (torch.rand(20, 3), torch.rand(21, 9), torch.rand(21, 3).double()):
        with pytest.raises(ValueError):
            ops.texture_pyramid(bad, 3, 4, 4)
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        ops.texture_pyramid(torch.rand(21, 3), 3, 4, 4)
    # sample
    taps = textures.Taps(idx, wgt, order, offsets, 3, 4, 4, 21)
    with pytest.raises(ValueError, match="Taps"):
        textures.sample(torch.rand(4, 4, 3), (idx, wgt))
    with pytest.raises(ValueError, match="4 x 4"):
        textures.sample(torch.rand(4, 8, 3), taps)
    with pytest.raises(ValueError, match="channels"):
        textures.sample(torch.rand(4, 4, 9), taps)
    with pytest.raises(ValueError, match="float32"):
        textures.sample(torch.rand(4, 4, 3).double(), taps)
    with pytest.raises(ValueError, match="tensor"):
        textures.sample(torch.rand(4), taps)
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        textures.sample(torch.rand(4, 4), taps)


def test_textured_materials_shapes_parameters_and_validation():
    from reni_amd.mesh import HipMeshRenderer, MeshRasterizer
    from reni_amd.textures import TexturedMaterials
    m = TexturedMaterials()
    assert list(m.parameters()) == [] and set(dict(m.named_buffers())) == {"albedo", "ks", "shininess"}
    a, k, s = m.values(None, None)                                    # all scalars: no rasteriser is asked
    assert float(a) == 1.0 and float(k) == 0.0 and float(s) == 500.0
    assert float(TexturedMaterials(shininess=1e6, shininess_max=100.0).values(None, None)[2]) == 100.0
    m = TexturedMaterials(albedo=torch.rand(8, 16, 3), ks=torch.rand(4, 4), shininess=40.0, learn=("albedo", "ks"), lod_bias=0.5)
    assert set(dict(m.named_parameters())) == {"albedo", "ks"} and set(dict(m.named_buffers())) == {"shininess"}
    assert m.levels is None and m.wrap == "clamp" and not m.align_corners and m.lod_bias == 0.5
    TexturedMaterials(albedo=torch.rand(3, 5, 3), align_corners=True)      # one level: legal
    TexturedMaterials(albedo=torch.rand(4, 4, 3), levels=1, align_corners=True)
    for bad in ({"albedo": torch.rand(4, 4)}, {"albedo": torch.rand(4, 4, 2)}, {"albedo": torch.rand(4)}, {"ks": torch.rand(4)},
                {"shininess": torch.rand(2, 2, 2)}, {"learn": ("kd",)}, {"wrap": "mirror"}, {"shininess_min": 0.0},
                {"albedo": torch.rand(3, 5, 3), "levels": 2}, {"ks": torch.rand(4, 4), "levels": 4},
                {"albedo": torch.rand(4, 4, 3), "align_corners": True}, {"ks": torch.rand(3, 3), "wrap": "repeat", "align_corners": True}):
        with pytest.raises(ValueError):
            TexturedMaterials(**bad)
    r = HipMeshRenderer(MeshRasterizer(), materials=m)
    assert r.textured and not r.spatial and sorted(n for n, _ in r.named_parameters()) == ["materials.albedo", "materials.ks"]
    assert not HipMeshRenderer(MeshRasterizer(), kd=0.5).textured
    two = HipMeshRenderer(MeshRasterizer(), materials=m)              # a second renderer shares the same Parameters
    assert two.materials.albedo is r.materials.albedo
