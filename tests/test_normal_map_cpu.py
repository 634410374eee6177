"""CPU tests of the normal-mapped materials: the new entry points' names, prototypes and argument checks (no GPU is touched
before them), the float64 restatement of d loss / d normals (tests/normal_map_ref.py) against autograd through
tests/shade_materials_ref.py and against a central difference of its own D and S, the tangent frames, ``perturb_normals``,
``TexturedMaterials(normal=)`` and the Python layer's argument errors."""
import math
import os
import re

import pytest
import torch

from tests import normal_map_ref as NR
from tests import shade_materials_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reni_envmap_shade_terms_dnormals_workspace_bytes", "reni_envmap_shade_terms_dnormals")
F64 = torch.float64


def test_entry_points_are_exported_declared_and_documented():
    from reni_amd import _lib
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.EXPORTS and getattr(lib, n) is not None
        assert n in integration, n
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    geometry = ("int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x, float cam_y, "
                "float cam_z, const float* light_dirs, int64_t dirs_batch_stride, ")
    materials = "const float* shininess, int64_t shininess_stride, const uint32_t* vis, int64_t vis_batch_stride, "
    assert "size_t reni_envmap_shade_terms_dnormals_workspace_bytes(int64_t B, int64_t NP, int64_t J);" in flat
    assert ("int reni_envmap_shade_terms_dnormals(" + geometry + "const float* light_colors, " + materials +
            "const float* d_diffuse, const float* d_specular, float* d_normals, void* ws, size_t ws_bytes, void* stream);") in flat
    for n in ("envmap_shade_terms_dnormals", "shade_terms_normals", "pixel_tangents", "perturb_normals", "shading_normals"):
        assert n in integration, n


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from reni_amd import _lib
    lib = _lib.load()
    ws_bytes = lib.reni_envmap_shade_terms_dnormals_workspace_bytes
    assert ws_bytes(0, 4, 4) == 0 and ws_bytes(1, 0, 4) == 0 and ws_bytes(1, 4, -1) == 0
    assert ws_bytes(1, 4, 4) == 1 * 1 * 4 * 3 * 4 + 256                      # one slot per (image chunk, split), always
    assert ws_bytes(2, 1000, 515) == 2 * 5 * 1000 * 3 * 4 + 256              # 515 texels = 5 stages = 5 splits
    EINVAL, EWORKSPACE = -1, -2
    p = 1 << 20  # a non-NULL, 16-byte aligned address: nothing dereferences it before the checks are through

    def dn(B=2, NP=4, J=40, nrm=p, pos=p, dirs=p, dstride=0, C=p, shin=p, sstride=0, vis=None, vstride=0, gD=p, gS=p, out=p,
           ws=p, nbytes=1 << 30):
        return lib.reni_envmap_shade_terms_dnormals(B, NP, J, nrm, pos, 0.0, 0.0, 0.0, dirs, dstride, C, shin, sstride, vis,
                                                    vstride, gD, gS, out, ws, nbytes, None)

    def rejected(rc, keyword, code=EINVAL):
        return rc == code and keyword in lib.reni_last_error() and b"dnormals" in lib.reni_last_error()

    for size in ({"B": 0}, {"NP": 0}, {"J": -1}):
        assert rejected(dn(**size), b">= 1")
    assert rejected(dn(NP=1 << 30), b"too large") and rejected(dn(J=1 << 30), b"too large") and rejected(dn(B=1 << 16), b"too large")
    for name in ("nrm", "pos", "dirs", "C", "shin", "gD", "gS", "out"):
        assert rejected(dn(**{name: None}), b"NULL"), name
    assert rejected(dn(dstride=119), b"direction batch stride")
    for bad in (2, -1, 4):
        assert rejected(dn(sstride=bad), b"shininess stride")
    assert rejected(dn(vis=p + 4), b"16-byte aligned")
    assert rejected(dn(vis=p, vstride=8), b"mask batch stride")                 # per-image masks on a shared grid
    assert rejected(dn(dstride=120, vis=p, vstride=7), b"mask batch stride")    # below NP JW = 8 words
    assert rejected(dn(J=512, dstride=1536, vis=p, vstride=66), b"mask batch stride")  # JW = 16: rows are read 16 bytes at a time
    # the workspace is always needed: a slot per (chunk, split), then the reduce applies the normalisation's Jacobian
    assert rejected(dn(ws=None, nbytes=0), b"workspace too small", EWORKSPACE)
    assert rejected(dn(ws=None), b"workspace too small", EWORKSPACE)
    assert rejected(dn(NP=4, J=40, nbytes=4 * 3 * 4 - 1), b"workspace too small", EWORKSPACE)
    assert rejected(dn(NP=1000, J=515, nbytes=5 * 1000 * 3 * 4 - 1), b"workspace too small", EWORKSPACE)               # one chunk of 2 images
    assert rejected(dn(NP=1000, J=515, dstride=1545, nbytes=2 * 5 * 1000 * 3 * 4 - 1), b"workspace too small", EWORKSPACE)  # two chunks


CPU_CASES = [(3, 130, 97, False), (2, 50, 33, True), (5, 40, 129, False), (3, 1, 1, False)]


@pytest.mark.parametrize("kind", NR.SHININESS)
def test_restatement_is_float64_autograd_except_on_background_pixels(kind):
    """On every pixel with a normal the written-out formula equals autograd through shade_terms_ref to 1e-12 of the largest
    value; on background pixels it is exactly 0 (autograd gives L a / 1e-6 there)."""
    for (B, NP, J, per_image) in CPU_CASES:
        c = NR.case(B, NP, J, per_image, kind)
        for vis in (None, c["vis"]):
            d = NR.dnormals_ref(c["nrm"], c["pos"], c["cam"], c["L"], c["C"], c["gD"], c["gS"], c["shin"], vis=vis)
            n = c["nrm"].to(F64).requires_grad_(True)
            D, S, _ = MR.shade_terms_ref(n, c["pos"], c["cam"], c["L"], c["C"], c["shin"], vis=vis)
            (g,) = torch.autograd.grad((D * c["gD"].to(F64)).sum() + (S * c["gS"].to(F64)).sum(), n)
            fg = ~c["bg"]
            assert float(d.abs().max()) > 0 and torch.isfinite(d).all()
            assert float((g[fg] - d[fg]).abs().max()) <= 1e-12 * float(d.abs().max())
            if bool(c["bg"].any()):
                assert float(d[c["bg"]].abs().max()) == 0.0
                if vis is None and NP > 1:
                    assert float(g[c["bg"]].abs().max()) > 1.0   # what the strict gates are there to avoid


@pytest.mark.parametrize("kind", ["s20", "per_pixel", "s1"])
def test_restatement_matches_a_central_difference_of_its_own_terms(kind):
    """sum d_normals . dn against (F(n + e dn) - F(n - e dn)) / 2e with F = sum gD D + sum gS S in float64.  Pixels with a
    pair within 2e of a gate are left out of this check (the diffuse term has a kink there, the s = 1 lobe a step); on the
    others F is smooth and the difference's own error is e^2 / 6 times a third derivative of size s^3 |S|: with e = 1e-6
    that is far below its rounding error, 2^-52 |F| / e ~ 2e-10 |F|.  1e-6 of the largest value is asked."""
    B, NP, J = 2, 120, 97
    c = NR.case(B, NP, J, False, kind)
    s = c["shin"].clamp(max=60.0)   # (per pixel: keep s^3 e^2 small)
    g = torch.Generator().manual_seed(3)
    dn = torch.randn(NP, 3, generator=g, dtype=F64)
    e = 1e-6
    for vis in (None, c["vis"]):
        d = NR.dnormals_ref(c["nrm"], c["pos"], c["cam"], c["L"], c["C"], c["gD"], c["gS"], s, vis=vis)

        def F(n):
            D, S, _ = MR.shade_terms_ref(n, c["pos"], c["cam"], c["L"], c["C"], s, vis=vis)
            return (D * c["gD"].to(F64)).sum(dim=(0, 2)) + (S * c["gS"].to(F64)).sum(dim=(0, 2))   # per pixel

        n0 = c["nrm"].to(F64)
        fd = (F(n0 + e * dn) - F(n0 - e * dn)) / (2 * e)
        _, _, x_l, x_h, _ = NR._pairs(c["nrm"], c["pos"], c["cam"], c["L"])
        margin = 4 * e * float(dn.norm(dim=1).max()) / float(n0.norm(dim=1)[~c["bg"]].min())
        smooth = ~c["bg"] & (x_l.abs() > margin).all(dim=(0, 2)) & (x_h.abs() > margin).all(dim=(0, 2))
        assert int(smooth.sum()) > NP // 2
        got = (d * dn).sum(1)
        assert float((got - fd)[smooth].abs().max()) <= 1e-6 * float(got.abs().max())


def _quad_scene(mirror=False, degenerate=False):
    """Two triangles in the plane z = 0, UVs u = x / 2, v = y / 4 (so T = +x, B = +y), seen by six 'pixels'."""
    verts = torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 4.0, 0.0], [0.0, 4.0, 0.0]], dtype=F64)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]])
    vt = verts[:, :2] / torch.tensor([2.0, 4.0], dtype=F64)
    if mirror:
        vt = vt * torch.tensor([-1.0, 1.0], dtype=F64) + torch.tensor([1.0, 0.0], dtype=F64)   # u runs towards -x
    ft = faces.clone()
    if degenerate:
        vt = torch.cat([vt, vt[:1]])
        ft[1] = torch.tensor([0, 4, 0])   # the second face's three UVs coincide: det = 0
    pix_valid = torch.tensor([0, 1, -1, 0, 1, 0])
    nrm = torch.tensor([[0.0, 0.0, 0.9], [0.3, 0.0, 0.8], [0.0, 0.0, 0.0], [0.0, -0.4, 0.5], [0.2, 0.1, -0.7], [0.1, 0.2, 0.6]], dtype=F64)
    return verts, faces, vt, ft, pix_valid, nrm


def test_tangent_frames_of_a_uv_mapped_quad():
    from reni_amd.textures import tangent_frames
    parts = _quad_scene()
    t, b, ok = tangent_frames(*parts)
    assert ok.tolist() == [True, True, False, True, True, True]
    nrm = parts[5]
    N = torch.nn.functional.normalize(nrm, dim=-1)
    # analytic: T_f = +x, B_f = +y on both faces; t is +x projected off N, b = N x t up to the sign that follows +y
    x = torch.tensor([1.0, 0.0, 0.0], dtype=F64)
    want_t = torch.nn.functional.normalize(x[None] - N * N[:, 0:1], dim=-1)
    cr = torch.linalg.cross(N, want_t)
    want_b = torch.sign(cr[:, 1:2]) * cr
    assert torch.allclose(t[ok], want_t[ok], atol=1e-14) and torch.allclose(b[ok], want_b[ok], atol=1e-14)
    assert torch.equal(t[0], x) and torch.equal(b[0], torch.tensor([0.0, 1.0, 0.0], dtype=F64))
    assert float(t[2].abs().max()) == 0.0 and float(b[2].abs().max()) == 0.0
    assert float((t * N).sum(1).abs().max()) <= 1e-15 and float((b * N).sum(1).abs().max()) <= 1e-15
    assert torch.allclose(t[ok].norm(dim=1), torch.ones(5, dtype=F64), atol=1e-15)
    assert torch.allclose(b[ok].norm(dim=1), torch.ones(5, dtype=F64), atol=1e-15)
    assert float((t * b).sum(1).abs().max()) <= 1e-15
    # pixel 4 looks at the back of the surface: N x t points to -y there, and h flips it so that b still follows +y
    assert float(b[4, 1]) > 0 and float(torch.linalg.cross(N[4], t[4])[1]) < 0
    # the float64 pixel-by-pixel restatement says the same
    rt, rb, rok = NR.tangent_frames_ref(*parts)
    assert torch.equal(rok, ok) and torch.allclose(rt, t, atol=1e-15) and torch.allclose(rb, b, atol=1e-15)
    # float32 inputs give float32 frames
    t32, b32, ok32 = tangent_frames(parts[0].float(), parts[1], parts[2].float(), parts[3], parts[4], parts[5].float())
    assert t32.dtype == torch.float32 and torch.equal(ok32, ok) and torch.allclose(t32.double(), t, atol=1e-6)


def test_tangent_frames_mirrored_and_degenerate_uvs():
    from reni_amd.textures import tangent_frames
    t0, b0, ok0 = tangent_frames(*_quad_scene())
    t1, b1, ok1 = tangent_frames(*_quad_scene(mirror=True))
    assert torch.equal(ok0, ok1)
    # mirrored u: the tangent turns round, the bitangent (growing v) stays: h = sign((N x t).B_f) has flipped
    assert torch.allclose(t1, -t0, atol=1e-15) and torch.allclose(b1, b0, atol=1e-15)
    N = torch.nn.functional.normalize(_quad_scene()[5], dim=-1)
    h0 = (torch.linalg.cross(N, t0) * b0).sum(1)[ok0]
    h1 = (torch.linalg.cross(N, t1) * b1).sum(1)[ok1]
    assert torch.allclose(h0, -h1, atol=1e-15) and torch.allclose(h0.abs(), torch.ones_like(h0), atol=1e-15)
    t2, b2, ok2 = tangent_frames(*_quad_scene(degenerate=True))
    assert ok2.tolist() == [True, False, False, True, False, True]
    assert float(t2[~ok2].abs().max()) == 0.0 and float(b2[~ok2].abs().max()) == 0.0 and torch.equal(t2[ok2], t0[ok2])
    rt, rb, rok = NR.tangent_frames_ref(*_quad_scene(degenerate=True))
    assert torch.equal(rok, ok2) and torch.allclose(rt, t2, atol=1e-15)
    # a normal along the face tangent leaves nothing to project: invalid
    verts, faces, vt, ft, pv, nrm = _quad_scene()
    nrm = nrm.clone()
    nrm[0] = torch.tensor([0.5, 0.0, 0.0], dtype=F64)
    assert tangent_frames(verts, faces, vt, ft, pv, nrm)[2].tolist() == [False, True, False, True, True, True]
    # non-finite UVs: invalid, and nothing non-finite comes out
    vt_bad = vt.clone()
    vt_bad[3, 0] = float("nan")
    tb, bb, okb = tangent_frames(verts, faces, vt_bad, ft, pv, _quad_scene()[5])
    assert okb.tolist() == [True, False, False, True, False, True] and torch.isfinite(tb).all() and torch.isfinite(bb).all()


def test_perturb_normals_flat_is_the_identity_and_invalid_pixels_are_untouched():
    from reni_amd.textures import perturb_normals, tangent_frames
    for dtype in (torch.float32, F64):
        verts, faces, vt, ft, pv, nrm = _quad_scene()
        nrm = nrm.to(dtype)
        t, b, ok = tangent_frames(verts.to(dtype), faces, vt.to(dtype), ft, pv, nrm)
        P = nrm.shape[0]
        flat = torch.tensor([0.0, 0.0, 1.0], dtype=dtype).expand(P, 3)
        for strength in (1.0, 2.5):
            assert torch.equal(perturb_normals(nrm, t, b, ok, flat, strength), nrm)        # bit for bit, not normalised
        g = torch.Generator().manual_seed(5)
        m = (torch.rand(P, 3, generator=g, dtype=dtype) * 2 - 1).requires_grad_(True)
        out = perturb_normals(nrm, t, b, ok, m, 0.7)
        assert torch.equal(out[~ok], nrm[~ok])
        N = torch.nn.functional.normalize(nrm, dim=-1)
        want = 0.7 * m[:, 0:1] * t + 0.7 * m[:, 1:2] * b + m[:, 2:3] * N                    # the direction the issue states
        cosine = (torch.nn.functional.normalize(out, dim=-1) * torch.nn.functional.normalize(want, dim=-1)).sum(1)
        assert float((cosine[ok] - 1).detach().abs().max()) <= (1e-6 if dtype == torch.float32 else 1e-14)
        assert torch.allclose(out[ok].norm(dim=1), (nrm.norm(dim=1, keepdim=True) * want).norm(dim=1)[ok], rtol=1e-5)
        ref = NR.perturb_normals_ref(nrm, t, b, ok, m.detach().to(F64), 0.7)
        assert float((out.detach().to(F64) - ref).abs().max()) <= (1e-6 if dtype == torch.float32 else 1e-15)
        (out * torch.randn(P, 3, generator=g, dtype=dtype)).sum().backward()
        assert float(m.grad[~ok].abs().max()) == 0.0 and float(m.grad[ok].abs().min()) > 0   # no gradient from invalid pixels
    for bad in ({"tangent": t[:-1]}, {"m": m[:, :2]}, {"valid": ok.to(torch.int64)}, {"valid": ok[:-1]}, {"pixel_normals": nrm[0]}):
        kw = dict(pixel_normals=nrm, tangent=t, bitangent=b, valid=ok, m=m)
        kw.update(bad)
        with pytest.raises(ValueError):
            perturb_normals(**kw)


def test_emulation_follows_the_definition_and_sets_the_gpu_tests_constant():
    """The fp32 emulation in kernel order against the float64 definition over the GPU test's own cases: every pixel within
    its bound's unit times a constant of order 1 -- K, which the GPU test uses, is four times the worst ratio."""
    K, worst = NR.emulation_constant()
    print("emulation: worst error / unit", worst, "K", K)
    assert K == 4.0 * worst and 0.25 < worst < 16.0
    # exact zeros where the definition has them
    c = NR.case(3, 1000, 515, False, "s20")
    emu = NR.dnormals_emulated(c["nrm"], c["pos"], c["cam"], c["L"], c["C"], c["gD"], c["gS"], c["shin"], vis=c["vis"])
    assert float(abs(emu[c["bg"].numpy()]).max()) == 0.0 and emu.dtype.name == "float32"
    assert NR.n_splits(1000, 515) == 5 and NR.n_splits(300, 200) == 2 and NR.n_splits(64, 129) == 2


def test_textured_materials_take_a_normal_texture():
    from reni_amd.mesh import HipMeshRenderer, MeshRasterizer
    from reni_amd.textures import TexturedMaterials
    m = TexturedMaterials(albedo=torch.rand(4, 8, 3), normal=torch.rand(8, 16, 3), learn=("albedo", "normal"), normal_strength=2.0)
    assert TexturedMaterials.NAMES == ("albedo", "ks", "shininess")
    assert set(dict(m.named_parameters())) == {"albedo", "normal"} and m.normal.shape == (8, 16, 3) and m.normal_strength == 2.0
    m = TexturedMaterials(normal=torch.rand(2, 2, 3))
    assert list(m.parameters()) == [] and "normal" in dict(m.named_buffers())
    plain = TexturedMaterials(albedo=torch.rand(4, 8, 3))
    assert plain.normal is None and "normal" not in dict(plain.named_buffers())
    nrm = torch.rand(5, 3)
    assert plain.shading_normals(None, None, pixel_normals=nrm) is nrm          # nothing new runs without a normal texture
    for bad in (torch.rand(4, 4), torch.rand(4, 4, 2), torch.rand(3), 0.5):
        with pytest.raises(ValueError, match="normal"):
            TexturedMaterials(normal=bad)
    with pytest.raises(ValueError, match="normal"):
        TexturedMaterials(learn=("normal",))
    with pytest.raises(ValueError, match="learn"):
        TexturedMaterials(learn=("bump",))
    with pytest.raises(ValueError, match="align_corners"):
        TexturedMaterials(normal=torch.rand(4, 4, 3), align_corners=True)
    r = HipMeshRenderer(MeshRasterizer(), materials=TexturedMaterials(normal=torch.rand(4, 4, 3), learn=("normal",)))
    assert r.textured and [n for n, _ in r.named_parameters()] == ["materials.normal"]


def test_python_argument_errors_come_before_the_library():
    from reni_amd import _lib, ops
    from reni_amd.envmap_shader import EnvironmentMap, blinn_phong_shading_materials, shade_terms, shade_terms_normals
    NP, J = 6, 40
    nrm, pos, cam = torch.randn(NP, 3), torch.randn(NP, 3), torch.zeros(3)
    dirs, C = torch.randn(J, 3), torch.rand(2, J, 3)
    gD = torch.rand(2, NP, 3)
    good = torch.zeros(1, NP, 2, dtype=torch.int32)

    def call(**k):
        return ops.envmap_shade_terms_dnormals(k.get("nrm", nrm), pos, cam, k.get("dirs", dirs), k.get("C", C), k.get("gD", gD), gD,
                                               k.get("s", 10.0), vis=k.get("vis"))

    for bad in (torch.rand(NP + 1), torch.rand(NP, 1), torch.rand(2), "ten"):
        with pytest.raises(ValueError, match="shininess"):
            call(s=bad)
    with pytest.raises(ValueError, match="int32"):
        call(vis=good.to(torch.int64))
    with pytest.raises(ValueError, match=r"\[NB, 6, 2\]"):
        call(vis=torch.zeros(1, NP, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="require grad"):
        call(vis=torch.zeros(1, NP, 2, requires_grad=True))
    with pytest.raises(ValueError, match="per-image directions"):
        call(vis=torch.zeros(2, NP, 2, dtype=torch.int32))
    for bad_dirs in (torch.randn(J), torch.randn(J, 4), torch.randn(1, 2, J, 3)):
        with pytest.raises(ValueError, match=r"\[J, 3\]"):
            call(dirs=bad_dirs)
    with pytest.raises(ValueError, match="normals"):
        call(nrm=torch.randn(NP))
    for kw in ({}, {"vis": good}, {"s": torch.full((NP,), 10.0)}):   # well-formed calls on CPU tensors: there is no CPU path
        with pytest.raises(_lib.RENILibraryError, match="GPU"):
            call(**kw)
    env = EnvironmentMap(environment_map=C, directions=dirs.expand(2, J, 3), sineweight=torch.ones(1, J, 1))
    n_g = nrm.clone().requires_grad_(True)
    # the old function keeps its contract; the new one lets the normals through, and only the normals
    with pytest.raises(ValueError, match="normals.*require grad"):
        shade_terms(n_g, pos, cam, env, 10.0)
    with pytest.raises(ValueError, match="normals.*require grad"):
        blinn_phong_shading_materials(n_g, pos, cam, env, 0.5, 0.3, 10.0)
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        shade_terms_normals(n_g, pos, cam, env, 10.0)
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        blinn_phong_shading_materials(n_g, pos, cam, env, 0.5, 0.3, 10.0, differentiable_normals=True)
    with pytest.raises(ValueError, match="positions.*require grad"):
        shade_terms_normals(n_g, pos.clone().requires_grad_(True), cam, env, 10.0)
    with pytest.raises(ValueError, match="camera.*require grad"):
        shade_terms_normals(n_g, pos, cam.clone().requires_grad_(True), env, 10.0)
    with pytest.raises(ValueError, match="require grad"):
        shade_terms_normals(n_g, pos, cam, env, 10.0, vis=torch.zeros(1, NP, 2, requires_grad=True))
    assert math.isfinite(float(n_g.sum())) and n_g.grad is None
