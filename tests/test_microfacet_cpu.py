"""CPU tests of the microfacet (GGX) materials: the new entry points' names, prototypes and argument checks (no GPU is touched
before them), the float64 reference tests/microfacet_ref.py (white furnace, central differences of its own sums, exact zeros
on background pixels), ``compose_microfacet``, the two material classes and the Python layer's argument errors."""
import math
import os
import re

import pytest
import torch

from tests import microfacet_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reni_envmap_shade_ggx_workspace_bytes", "reni_envmap_shade_ggx", "reni_envmap_shade_ggx_backward",
         "reni_envmap_shade_ggx_dpixel_workspace_bytes", "reni_envmap_shade_ggx_dpixel")
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
    materials = "const float* alpha, int64_t alpha_stride, const uint32_t* vis, int64_t vis_batch_stride, "
    tail = "void* ws, size_t ws_bytes, void* stream);"
    assert "size_t reni_envmap_shade_ggx_workspace_bytes(int64_t B, int64_t NP, int64_t J);" in flat
    assert "size_t reni_envmap_shade_ggx_dpixel_workspace_bytes(int64_t B, int64_t NP, int64_t J);" in flat
    assert ("int reni_envmap_shade_ggx(" + geometry + "const float* light_colors, " + materials +
            "float* diffuse, float* spec0, float* spec1, " + tail) in flat
    assert ("int reni_envmap_shade_ggx_backward(" + geometry + materials +
            "const float* d_diffuse, const float* d_spec0, const float* d_spec1, float* dlight_colors, " + tail) in flat
    assert ("int reni_envmap_shade_ggx_dpixel(" + geometry + "const float* light_colors, " + materials +
            "const float* d_diffuse, const float* d_spec0, const float* d_spec1, float* d_alpha, float* d_normals, " + tail) in flat
    for n in ("envmap_shade_ggx", "envmap_shade_ggx_backward", "envmap_shade_ggx_dpixel", "shade_terms_ggx", "compose_microfacet",
              "microfacet_shading_materials", "MicrofacetMaterials", "TexturedMicrofacetMaterials"):
        assert n in integration, n


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from reni_amd import _lib
    lib = _lib.load()
    for ws_bytes in (lib.reni_envmap_shade_ggx_workspace_bytes, lib.reni_envmap_shade_ggx_dpixel_workspace_bytes):
        assert ws_bytes(0, 4, 4) == 0 and ws_bytes(1, 0, 4) == 0 and ws_bytes(1, 4, -1) == 0
    assert lib.reni_envmap_shade_ggx_workspace_bytes(1, 4, 4) == 256                                  # one split: no partial sums
    assert lib.reni_envmap_shade_ggx_workspace_bytes(2, 1000, 515) == 5 * 3 * 2 * 1000 * 3 * 4 + 256  # 5 splits of three terms
    assert lib.reni_envmap_shade_ggx_dpixel_workspace_bytes(1, 4, 4) == 1 * 1 * 4 * 4 * 4 + 256       # 1 + 3 floats per slot, always
    assert lib.reni_envmap_shade_ggx_dpixel_workspace_bytes(2, 1000, 515) == 2 * 5 * 1000 * 4 * 4 + 256
    EINVAL, EWORKSPACE = -1, -2
    p = 1 << 20  # a non-NULL, 16-byte aligned address: nothing dereferences it before the checks are through

    def fwd(B=2, NP=4, J=40, nrm=p, pos=p, dirs=p, dstride=0, C=p, al=p, astride=0, vis=None, vstride=0, D=p, S0=p, S1=p, ws=p,
            nbytes=1 << 30):
        return lib.reni_envmap_shade_ggx(B, NP, J, nrm, pos, 0.0, 0.0, 0.0, dirs, dstride, C, al, astride, vis, vstride, D, S0, S1,
                                         ws, nbytes, None)

    def bwd(B=2, NP=4, J=40, nrm=p, pos=p, dirs=p, dstride=0, al=p, astride=0, vis=None, vstride=0, gD=p, gS0=p, gS1=p, dC=p,
            ws=p, nbytes=1 << 30):
        return lib.reni_envmap_shade_ggx_backward(B, NP, J, nrm, pos, 0.0, 0.0, 0.0, dirs, dstride, al, astride, vis, vstride, gD,
                                                  gS0, gS1, dC, ws, nbytes, None)

    def dpx(B=2, NP=4, J=40, nrm=p, pos=p, dirs=p, dstride=0, C=p, al=p, astride=0, vis=None, vstride=0, gD=p, gS0=p, gS1=p,
            da=p, dn=p, ws=p, nbytes=1 << 30):
        return lib.reni_envmap_shade_ggx_dpixel(B, NP, J, nrm, pos, 0.0, 0.0, 0.0, dirs, dstride, C, al, astride, vis, vstride,
                                                gD, gS0, gS1, da, dn, ws, nbytes, None)

    def rejected(rc, keyword, code=EINVAL, who=b"envmap shade ggx"):
        return rc == code and keyword in lib.reni_last_error() and who in lib.reni_last_error()

    pointers = {fwd: ("nrm", "pos", "dirs", "C", "al", "D", "S0", "S1"), bwd: ("nrm", "pos", "dirs", "al", "gD", "gS0", "gS1", "dC"),
                dpx: ("nrm", "pos", "dirs", "C", "al", "gD", "gS0", "gS1", "da")}   # (dn = NULL: "not wanted")
    for call, names in pointers.items():
        who = b"envmap shade ggx dpixel" if call is dpx else b"envmap shade ggx:"
        for size in ({"B": 0}, {"NP": 0}, {"J": -1}):
            assert rejected(call(**size), b">= 1", who=who)
        for size in ({"NP": 1 << 30}, {"J": 1 << 30}, {"B": 1 << 16}):
            assert rejected(call(**size), b"too large", who=who)
        for name in names:
            assert rejected(call(**{name: None}), b"NULL", who=who), name
        assert rejected(call(dstride=119), b"direction batch stride", who=who)
        for bad in (2, -1, 4):
            assert rejected(call(astride=bad), b"alpha stride", who=who)
        assert rejected(call(vis=p + 4), b"16-byte aligned", who=who)
        assert rejected(call(vis=p, vstride=8), b"mask batch stride", who=who)                 # per-image masks on a shared grid
        assert rejected(call(dstride=120, vis=p, vstride=7), b"mask batch stride", who=who)    # below NP JW = 8 words
        assert rejected(call(J=512, dstride=1536, vis=p, vstride=66), b"mask batch stride", who=who)  # JW = 16: 16-byte row loads
    # forward and backward need a workspace only when the other axis is split
    assert rejected(fwd(NP=1000, J=515, ws=None), b"workspace too small", EWORKSPACE)
    assert rejected(fwd(NP=1000, J=515, nbytes=5 * 3 * 2 * 1000 * 3 * 4 - 1), b"workspace too small", EWORKSPACE)
    assert rejected(bwd(NP=1000, J=515, nbytes=8 * 2 * 515 * 3 * 4 - 1), b"workspace too small", EWORKSPACE)   # 1000 pixels = 8 stages
    # the dpixel call always needs one: a slot per (chunk, split), a quarter of it when the normals' gradient is not wanted
    who = b"envmap shade ggx dpixel"
    assert rejected(dpx(ws=None, nbytes=0), b"workspace too small", EWORKSPACE, who)
    assert rejected(dpx(ws=None), b"workspace too small", EWORKSPACE, who)
    assert rejected(dpx(NP=4, J=40, nbytes=4 * 4 * 4 - 1), b"workspace too small", EWORKSPACE, who)
    assert rejected(dpx(NP=4, J=40, dn=None, nbytes=4 * 4 - 1), b"workspace too small", EWORKSPACE, who)
    assert rejected(dpx(NP=1000, J=515, nbytes=5 * 1000 * 4 * 4 - 1), b"workspace too small", EWORKSPACE, who)                # one chunk
    assert rejected(dpx(NP=1000, J=515, dstride=1545, nbytes=2 * 5 * 1000 * 4 * 4 - 1), b"workspace too small", EWORKSPACE, who)  # two


def test_python_argument_errors_come_before_the_library():
    from reni_amd import _lib, ops
    from reni_amd.envmap_shader import EnvironmentMap, microfacet_shading_materials, shade_terms_ggx
    NP, J = 6, 40
    nrm, pos, cam = torch.randn(NP, 3), torch.randn(NP, 3), torch.zeros(3)
    dirs, C = torch.randn(J, 3), torch.rand(2, J, 3)
    g = torch.rand(2, NP, 3)
    good = torch.zeros(1, NP, 2, dtype=torch.int32)

    def calls(**k):
        a = (k.get("nrm", nrm), pos, cam, k.get("dirs", dirs))
        al, vis = k.get("al", 0.25), k.get("vis")
        return (lambda: ops.envmap_shade_ggx(*a, k.get("C", C), al, vis=vis),
                lambda: ops.envmap_shade_ggx_backward(*a, k.get("g", g), g, g, al, vis=vis),
                lambda: ops.envmap_shade_ggx_dpixel(*a, k.get("C", C), k.get("g", g), g, g, al, vis=vis, need_dn=True))

    def raises(exc, match, **k):
        for call in calls(**k):
            with pytest.raises(exc, match=match):
                call()

    for bad in (torch.rand(NP + 1), torch.rand(NP, 1), torch.rand(2), "rough"):
        raises(ValueError, "alpha", al=bad)
    raises(ValueError, "int32", vis=good.to(torch.int64))
    raises(ValueError, r"\[NB, 6, 2\]", vis=torch.zeros(1, NP, 3, dtype=torch.int32))
    raises(ValueError, "require grad", vis=torch.zeros(1, NP, 2, requires_grad=True))
    raises(ValueError, "per-image directions", vis=torch.zeros(2, NP, 2, dtype=torch.int32))
    for bad_dirs in (torch.randn(J), torch.randn(J, 4), torch.randn(1, 2, J, 3)):
        raises(ValueError, r"\[J, 3\]", dirs=bad_dirs)
    raises(ValueError, "normals", nrm=torch.randn(NP))
    for kw in ({}, {"vis": good}, {"al": torch.full((NP,), 0.3)}):   # well-formed calls on CPU tensors: there is no CPU path
        raises(_lib.RENILibraryError, "GPU", **kw)
    env = EnvironmentMap(environment_map=C, directions=dirs.expand(2, J, 3), sineweight=torch.ones(1, J, 1))
    n_g = nrm.clone().requires_grad_(True)
    with pytest.raises(_lib.RENILibraryError, match="GPU"):   # the normals may require grad
        shade_terms_ggx(n_g, pos, cam, env, 0.25)
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        microfacet_shading_materials(n_g, pos, cam, env, 0.5, torch.tensor(0.5, requires_grad=True), 0.1)
    with pytest.raises(ValueError, match="positions.*require grad"):
        shade_terms_ggx(nrm, pos.clone().requires_grad_(True), cam, env, 0.25)
    with pytest.raises(ValueError, match="camera.*require grad"):
        shade_terms_ggx(nrm, pos, cam.clone().requires_grad_(True), env, 0.25)
    env_g = EnvironmentMap(environment_map=C, directions=dirs.expand(2, J, 3).clone().requires_grad_(True), sineweight=torch.ones(1, J, 1))
    with pytest.raises(ValueError, match="directions.*require grad"):
        shade_terms_ggx(nrm, pos, cam, env_g, 0.25)
    with pytest.raises(ValueError, match="require grad"):
        shade_terms_ggx(nrm, pos, cam, env, 0.25, vis=torch.zeros(1, NP, 2, requires_grad=True))
    with pytest.raises(ValueError, match="alpha"):
        shade_terms_ggx(nrm, pos, cam, env, torch.rand(NP + 1))
    with pytest.raises(ValueError, match="roughness_min"):
        microfacet_shading_materials(nrm, pos, cam, env, 0.5, 0.5, 0.0, roughness_min=0.0)
    assert n_g.grad is None


# ------------------------------------------------------------------------------------------------ the float64 reference
def _furnace(alpha, cos_v, P=512, Q=1024, rows=256):
    """(1 / pi) sum_j k(N, V, L_j) omega_j over an equirectangular P x Q grid of directions (midpoint rule), N = +z,
    N.V = cos_v; ``rows`` rows of the grid at a time."""
    ph = (torch.arange(Q, dtype=F64) + 0.5) * (2 * math.pi / Q)
    V = torch.tensor([math.sqrt(1 - cos_v * cos_v), 0.0, cos_v], dtype=F64)
    nrm, pos = torch.tensor([[0.0, 0.0, 1.0]], dtype=F64), torch.zeros(1, 3, dtype=F64)
    total = 0.0
    for r0 in range(0, P, rows):
        th = (torch.arange(r0, min(P, r0 + rows), dtype=F64) + 0.5) * (math.pi / P)
        n = th.numel()
        st, ct = torch.sin(th)[:, None], torch.cos(th)[:, None]
        L = torch.stack([st * torch.cos(ph)[None], st * torch.sin(ph)[None], ct.expand(n, Q)], dim=-1).reshape(1, n * Q, 3)
        omega = (st * (math.pi / P) * (2 * math.pi / Q)).expand(n, Q).reshape(1, n * Q, 1)
        _, S0, _ = GR.shade_terms_ggx_ref(nrm, pos, V, L, omega.expand(1, n * Q, 3), torch.tensor(alpha, dtype=F64))
        total += float(S0[0, 0, 0])
    return total / math.pi


def test_white_furnace_of_the_reference():
    """k carries the GGX distribution, the separable Smith visibility and nl: under white light it reflects 1 - ln 2 at
    alpha = 1, N = V (the closed form, on a 512 x 1024 grid), and never more than everything: <= 1.001 at every alpha and
    angle.  At alpha = 0.01 the lobe is 0.02 rad wide in L and a 512 x 1024 grid has cells of 0.006 rad: its midpoint rule
    alone is off by 0.8 % there (1.0080 at N = V), so that alpha is integrated on the 2000 x 4000 grid the definition was
    checked on."""
    assert abs(_furnace(1.0, 1.0) - (1.0 - math.log(2.0))) <= 1e-4
    for alpha in (0.01, 0.25, 1.0):
        for cos_v in (1.0, 0.5, 0.1):
            e = _furnace(alpha, cos_v, *((2000, 4000) if alpha < 0.1 else (512, 1024)))
            print(f"furnace alpha {alpha} N.V {cos_v}: {e:.6f}")
            assert 0.0 < e <= 1.001, (alpha, cos_v, e)


CPU_CASES = [(3, 130, 97, False, "per_pixel"), (2, 50, 33, True, "r02"), (5, 40, 129, False, "r07"), (3, 1, 1, False, "r07")]


@pytest.mark.parametrize("B,NP,J,per_image,kind", CPU_CASES)
def test_reference_gradients_match_central_differences_of_its_own_sums(B, NP, J, per_image, kind):
    """d alpha and d normals of the reference (autograd with strict gates) against (F(x + e dx) - F(x - e dx)) / 2e per pixel,
    F = sum gD D + sum gS0 S0 + sum gS1 S1 in float64.  Pixels with a pair within the step's reach of a gate are left out (k has
    a step at x_h = 0 and kinks at x_l = 0 and x_v = 0); on the others F is smooth and e = 1e-6 leaves a rounding error of
    2^-52 |F| / e ~ 2e-10 |F|.  The sharpest lobe here (alpha = 0.01) has third derivatives of order alpha^-3 |F|, so the
    difference's own error, e^2 / 6 of that, is ~ 2e-7 |F|: 2e-6 of the largest value is asked."""
    c = GR.case(B, NP, J, per_image, kind)
    g = torch.Generator().manual_seed(5)
    dn = torch.randn(NP, 3, generator=g, dtype=F64)
    da = torch.rand(NP, generator=g, dtype=F64) + 0.5
    e = 1e-6
    for vis in (None, c.vis):
        ref = GR.evaluate(c, vis)

        def F(n, al):
            D, S0, S1 = GR.shade_terms_ggx_ref(n, c.pos, c.cam, c.L, c.C, al, vis=vis)
            return sum((T * g_.to(F64)).sum(dim=(0, 2)) for T, g_ in ((D, c.gD), (S0, c.gS0), (S1, c.gS1)))   # per pixel

        n0, a0 = c.nrm.to(F64), c.alpha.to(F64).expand(NP)
        q = GR.pairs(c.nrm, c.pos, c.cam, c.L, c.alpha)
        fg = ~c.bg
        margin = 4 * e * float(dn.norm(dim=1).max()) / float(n0.norm(dim=1)[fg].min())
        smooth = fg & (q.x_l.abs() > margin).all(dim=(0, 2)) & (q.x_h.abs() > margin).all(dim=(0, 2)) & (q.x_v.abs() > margin).all(dim=(0, 2))
        assert int(smooth.sum()) > NP // 2
        fd_n = (F(n0 + e * dn, a0) - F(n0 - e * dn, a0)) / (2 * e)
        got_n = (ref["dn"] * dn).sum(1)
        assert float((got_n - fd_n)[smooth].abs().max()) <= 2e-6 * float(got_n.abs().max())
        h = e * a0   # a relative step: alpha spans two decades
        fd_a = (F(n0, a0 + h * da) - F(n0, a0 - h * da)) / (2 * h)
        got_a = ref["dalpha"] * da
        assert float((got_a - fd_a)[fg].abs().max()) <= 2e-6 * float(got_a.abs().max())


def test_background_pixels_are_exact_zeros_in_the_reference():
    for (B, NP, J, per_image, kind) in CPU_CASES[:3]:
        c = GR.case(B, NP, J, per_image, kind)
        assert bool(c.bg.any())
        for vis in (None, c.vis):
            ref = GR.evaluate(c, vis)
            for name in ("D", "S0", "S1", "colours"):
                assert float(ref[name][:, c.bg].abs().max()) == 0.0, name
            for name in ("dalpha", "dn", "d_base_color", "d_metallic") + (("d_roughness",) if c.rough.numel() > 1 else ()):
                assert float(ref[name][c.bg].abs().max()) == 0.0, name
            assert all(bool(torch.isfinite(v).all()) for v in ref.values())
            assert float(ref["S0"].abs().max()) > 0 and float(ref["dn"].abs().max()) > 0 and float(ref["dalpha"].abs().max()) > 0


def test_float32_evaluation_sets_the_gpu_tests_factors():
    """The definition in float32 torch against float64 over the GPU test's 42 cases: the worst ratio per quantity, of which
    the GPU test allows four times (and never less than the scalar shader's 2e-5 of the largest reference value)."""
    ratios, factors = GR.float32_ratios(), GR.factors()
    for k in GR.QUANTITIES:
        print(f"float32 ratio {k}: {ratios[k]:.3e}  factor {factors[k]:.3e}")
        assert factors[k] == 4.0 * ratios[k] and 0.0 < ratios[k] < 1e-3
    assert len(GR.all_cases()) * len(GR.MASKS) == 42 and GR.FLOOR == 2e-5


# ------------------------------------------------------------------------------------------------ composition and classes
def test_compose_microfacet_limits_and_gradients():
    from reni_amd.envmap_shader import compose_microfacet
    g = torch.Generator().manual_seed(1)
    B, NP = 2, 7
    D, S0, S1 = (torch.rand(B, NP, 3, generator=g, dtype=F64) for _ in range(3))
    bc = torch.rand(NP, 3, generator=g, dtype=F64)
    assert torch.equal(compose_microfacet(D, S0, S1, bc, 0.0, f0_dielectric=0.0), bc * D + S1)        # F0 = 0: all of S1 ...
    assert torch.equal(compose_microfacet(D, torch.zeros_like(S0), torch.zeros_like(S1), bc, 0.0, f0_dielectric=0.0), bc * D)
    assert torch.allclose(compose_microfacet(D, S0, S1, bc, 1.0), bc * S0 + (1 - bc) * S1, rtol=0, atol=1e-15)
    m = torch.rand(NP, generator=g, dtype=F64)
    want = GR.compose_microfacet_ref(D, S0, S1, bc, m)
    assert torch.allclose(compose_microfacet(D, S0, S1, bc, m), want, rtol=0, atol=1e-15)
    for c in (0.3, torch.tensor([0.2, 0.5, 0.7], dtype=F64)):
        assert torch.allclose(compose_microfacet(D, S0, S1, c, 0.25), GR.compose_microfacet_ref(D, S0, S1, c, 0.25), rtol=0, atol=1e-15)
    bc_g, m_g = bc.clone().requires_grad_(True), m.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: compose_microfacet(D, S0, S1, a, b), (bc_g, m_g))
    for bad in ({"base_color": torch.rand(NP + 1, 3)}, {"base_color": torch.rand(2)}, {"metallic": torch.rand(NP + 1)},
                {"S0": S0[:, :-1]}, {"D": D[0]}):
        kw = dict(D=D, S0=S0, S1=S1, base_color=bc, metallic=m)
        kw.update(bad)
        with pytest.raises(ValueError):
            compose_microfacet(**kw)


def test_microfacet_materials_shapes_learn_and_clamps():
    from reni_amd.envmap_shader import MicrofacetMaterials
    from reni_amd.mesh import HipMeshRenderer, MeshRasterizer
    S = 4
    m = MicrofacetMaterials(torch.rand(S, S, 3), torch.linspace(-0.5, 1.5, S * S).reshape(S, S), torch.linspace(-1, 2, S * S),
                            learn=("base_color", "roughness"))
    assert MicrofacetMaterials.NAMES == ("base_color", "roughness", "metallic")
    assert set(dict(m.named_parameters())) == {"base_color", "roughness"} and "metallic" in dict(m.named_buffers())
    c, r, me = m.values()
    assert c.shape == (S * S, 3) and r.shape == (S * S,) and me.shape == (S * S,)
    assert float(r.min()) == pytest.approx(0.1) and float(r.max()) == 1.0 and float(me.min()) == 0.0 and float(me.max()) == 1.0
    assert m.roughness_min == 0.1 and m.f0_dielectric == 0.04
    r.sum().backward()   # the clamp passes gradients inside the range only
    assert int((m.roughness.grad != 0).sum()) == int(((m.roughness > 0.1) & (m.roughness < 1.0)).sum())
    d = MicrofacetMaterials()
    assert list(d.parameters()) == [] and d.values()[0].dim() == 0
    assert MicrofacetMaterials([0.2, 0.4, 0.6], 0.3, 0.0, roughness_min=0.25).values()[1] == pytest.approx(0.3)
    for bad in ({"base_color": torch.rand(5, 4)}, {"base_color": torch.rand(2)}, {"roughness": torch.rand(2, 3, 4)},
                {"metallic": torch.rand(2, 3)}, {"learn": ("albedo",)}, {"roughness_min": 0.0}, {"roughness_min": -1.0},
                {"base_color": torch.rand(16, 3), "roughness": torch.rand(9)}):
        with pytest.raises(ValueError):
            MicrofacetMaterials(**bad)
    r = HipMeshRenderer(MeshRasterizer(), materials=m)   # no kd needed
    assert r.microfacet and not r.textured and not r.spatial
    assert sorted(n for n, _ in r.named_parameters()) == ["materials.base_color", "materials.roughness"]


def test_textured_microfacet_materials_share_the_lookup_with_textured_materials():
    from reni_amd.mesh import HipMeshRenderer, MeshRasterizer
    from reni_amd.textures import TexturedMaterials, TexturedMicrofacetMaterials, _UVMaterials
    assert issubclass(TexturedMicrofacetMaterials, _UVMaterials) and issubclass(TexturedMaterials, _UVMaterials)
    assert TexturedMicrofacetMaterials.NAMES == ("base_color", "roughness", "metallic")
    assert TexturedMaterials.NAMES == ("albedo", "ks", "shininess")
    for shared in ("_fetched", "_taps", "shading_normals", "tangent_space_normals", "is_texture"):   # one fetch, not a copy
        assert getattr(TexturedMicrofacetMaterials, shared) is getattr(TexturedMaterials, shared)
    m = TexturedMicrofacetMaterials(base_color=torch.rand(4, 8, 3), roughness=torch.rand(16, 16), metallic=0.2,
                                    normal=torch.rand(8, 16, 3), learn=("roughness", "normal"), normal_strength=2.0, lod_bias=0.5)
    assert set(dict(m.named_parameters())) == {"roughness", "normal"} and m.normal_strength == 2.0 and m.lod_bias == 0.5
    assert set(dict(m.named_buffers())) == {"base_color", "metallic"}
    assert m.is_texture(m.base_color) and m.is_texture(m.roughness) and not m.is_texture(m.metallic)
    scalars = TexturedMicrofacetMaterials(base_color=[0.2, 0.4, 0.6], roughness=0.05, metallic=1.5)
    c, r, me = scalars.values(None, None)    # nothing is fetched for scalars; the clamps apply
    assert c.tolist() == pytest.approx([0.2, 0.4, 0.6]) and float(r) == pytest.approx(0.1) and float(me) == 1.0
    nrm = torch.rand(5, 3)
    assert scalars.normal is None and scalars.shading_normals(None, None, pixel_normals=nrm) is nrm
    flat = torch.tensor([0.5, 0.5, 1.0]).expand(4, 4, 3)
    assert TexturedMicrofacetMaterials(normal=flat).normal.shape == (4, 4, 3)
    for bad in ({"base_color": torch.rand(4, 4)}, {"roughness": torch.rand(4, 4, 3)}, {"metallic": torch.rand(3)},
                {"normal": torch.rand(4, 4)}, {"learn": ("normal",)}, {"learn": ("shininess",)}, {"wrap": "mirror"},
                {"roughness_min": 0.0}, {"roughness": torch.rand(4, 4), "align_corners": True}):
        with pytest.raises(ValueError):
            TexturedMicrofacetMaterials(**bad)
    r = HipMeshRenderer(MeshRasterizer(), materials=m)
    assert r.microfacet and r.textured and not r.spatial
    old = HipMeshRenderer(MeshRasterizer(), materials=TexturedMaterials(albedo=torch.rand(4, 4, 3)))
    assert old.textured and not old.microfacet
