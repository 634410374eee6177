"""CPU tests of the shader's per-pixel materials: the entry points' names, prototypes and argument checks (no GPU is
touched before them), the float64 reference itself (tests/shade_materials_ref.py: its composition against the oracle's
scalar shader, its analytic dS/ds against a finite difference), ``compose_materials`` and ``SpatialMaterials``."""
import os
import re

import pytest
import torch

from oracle import reni_oracle as O
from tests import shade_materials_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reni_envmap_shade_terms_workspace_bytes", "reni_envmap_shade_terms", "reni_envmap_shade_terms_backward")


def _problem(B, NP, J, seed, per_image_dirs=False):
    g = torch.Generator().manual_seed(seed)
    nrm = torch.randn(NP, 3, generator=g) * 0.7
    pos = torch.randn(NP, 3, generator=g) * 0.4
    bg = torch.rand(NP, generator=g) < 0.2
    nrm[bg] = 0.0
    pos[bg] = 0.0
    cam = torch.tensor([0.0, 0.0, 2.0])
    L = torch.nn.functional.normalize(torch.randn((B if per_image_dirs else 1, J, 3), generator=g), dim=-1)
    C = torch.exp(torch.randn(B, J, 3, generator=g)) * torch.rand(1, J, 1, generator=g)
    return nrm, pos, cam, L, C


def test_entry_points_are_exported_declared_and_documented():
    from reni_amd import _lib
    header = open(os.path.join(ROOT, "include", "reni_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert n in _lib.EXPORTS
        assert n in integration, n
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    geometry = ("int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x, float cam_y, "
                "float cam_z, const float* light_dirs, int64_t dirs_batch_stride, ")
    materials = "const float* shininess, int64_t shininess_stride, const uint32_t* vis, int64_t vis_batch_stride, "
    tail = "void* ws, size_t ws_bytes, void* stream);"
    assert "size_t reni_envmap_shade_terms_workspace_bytes(int64_t B, int64_t NP, int64_t J, uint32_t flags);" in flat
    assert ("int reni_envmap_shade_terms(" + geometry + "const float* light_colors, " + materials +
            "float* diffuse, float* specular, float* dspecular_ds, " + tail) in flat
    assert ("int reni_envmap_shade_terms_backward(" + geometry + materials +
            "const float* d_diffuse, const float* d_specular, float* dlight_colors, " + tail) in flat
    assert re.search(r"#define\s+RENI_SHADE_TERMS_DS\s+1u", header) and _lib.SHADE_TERMS_DS == 1


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from reni_amd import _lib
    lib = _lib.load()
    ws_bytes = lib.reni_envmap_shade_terms_workspace_bytes
    assert ws_bytes(0, 4, 4, 0) == 0 and ws_bytes(1, 4, 0, 0) == 0 and ws_bytes(1, 4, 4, 2) == 0
    assert ws_bytes(1, 4, 4, 0) == 256                                       # one split: no partial sums
    # (2, 1000, 515): 5 splits forward (515 texels = 5 stages), 3 terms with dS/ds
    assert ws_bytes(2, 1000, 515, 0) == 5 * 2 * 2 * 1000 * 3 * 4 + 256
    assert ws_bytes(2, 1000, 515, 1) == 5 * 3 * 2 * 1000 * 3 * 4 + 256
    EINVAL, EWORKSPACE = -1, -2
    p = 1 << 20  # a non-NULL, 16-byte aligned address: nothing dereferences it before the checks are through

    def fwd(B=2, NP=4, J=40, nrm=p, pos=p, dirs=p, dstride=0, C=p, shin=p, sstride=0, vis=None, vstride=0, D=p, S=p, T=None,
            ws=None, nbytes=0):
        return lib.reni_envmap_shade_terms(B, NP, J, nrm, pos, 0.0, 0.0, 0.0, dirs, dstride, C, shin, sstride, vis, vstride,
                                           D, S, T, ws, nbytes, None)

    def bwd(B=2, NP=4, J=40, nrm=p, pos=p, dirs=p, dstride=0, shin=p, sstride=0, vis=None, vstride=0, gD=p, gS=p, dC=p,
            ws=None, nbytes=0):
        return lib.reni_envmap_shade_terms_backward(B, NP, J, nrm, pos, 0.0, 0.0, 0.0, dirs, dstride, shin, sstride, vis,
                                                    vstride, gD, gS, dC, ws, nbytes, None)

    def rejected(rc, keyword, code=EINVAL):
        return rc == code and keyword in lib.reni_last_error()

    for fn in (fwd, bwd):
        for size in ({"B": 0}, {"NP": 0}, {"J": -1}):
            assert rejected(fn(**size), b">= 1")
        assert rejected(fn(NP=1 << 30), b"too large") and rejected(fn(B=1 << 16), b"too large")
        for name in ("nrm", "pos", "dirs", "shin"):
            assert rejected(fn(**{name: None}), b"NULL"), name
        assert rejected(fn(dstride=119), b"direction batch stride")
        for bad in (2, -1, 4):
            assert rejected(fn(sstride=bad), b"shininess stride")
        assert rejected(fn(vis=p + 4), b"16-byte aligned")
        assert rejected(fn(vis=p, vstride=8), b"mask batch stride")                 # per-image masks on a shared grid
        assert rejected(fn(dstride=120, vis=p, vstride=7), b"mask batch stride")    # below NP JW = 8 words
        assert rejected(fn(J=512, dstride=1536, vis=p, vstride=66), b"mask batch stride")  # JW = 16: rows are read 16 bytes at a time
        assert rejected(fn(NP=1000, J=515), b"workspace too small", EWORKSPACE)
        assert rejected(fn(NP=1000, J=515, ws=p, nbytes=1024), b"workspace too small", EWORKSPACE)
    for name in ("C", "D", "S"):
        assert rejected(fwd(**{name: None}), b"NULL"), name
    for name in ("gD", "gS", "dC"):
        assert rejected(bwd(**{name: None}), b"NULL"), name
    # dS/ds needs the third term's partial sums: the size without the flag is too small for it
    assert rejected(fwd(NP=1000, J=515, T=p, ws=p, nbytes=ws_bytes(2, 1000, 515, 0) - 256), b"workspace too small", EWORKSPACE)


@pytest.mark.parametrize("shin", [500.0, 20.0])
def test_reference_composition_is_the_oracles_scalar_shader(shin):
    from reni_amd.envmap_shader import compose_materials
    B, NP, J = 3, 130, 97
    nrm, pos, cam, L, C = _problem(B, NP, J, seed=5)
    D, S, _ = MR.shade_terms_ref(nrm, pos, cam, L, C, shin)
    want = O.blinn_phong_gbuffer(nrm, pos, cam, L.expand(B, -1, -1), C, shin, 0.4, 0.6)
    for got in (compose_materials(D, S, 0.4, 0.6, shin), MR.compose_ref(D, S, 0.4, 0.6, shin)):
        assert got.dtype == torch.float64
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # ... and per-image directions, a per-pixel shininess that happens to be constant, an albedo per channel
    nrm, pos, cam, L, C = _problem(2, 50, 33, seed=6, per_image_dirs=True)
    f64 = torch.float64
    D, S, _ = MR.shade_terms_ref(nrm, pos, cam, L, C, torch.full((50,), shin, dtype=f64))
    want = O.blinn_phong_gbuffer(nrm, pos, cam, L, C, shin, 0.4, 0.6)
    got = compose_materials(D, S, torch.full((50, 3), 0.4, dtype=f64), torch.full((50,), 0.6, dtype=f64), torch.full((50,), shin, dtype=f64))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("shin", [500.0, 20.0, None])
def test_reference_dS_ds_matches_a_central_difference_of_its_own_S(shin):
    """The yardstick, not the kernel: T against (S(s + h) - S(s - h)) / 2h in float64.  The difference's own error is
    h^2 / 6 times the third derivative sum nh^s ln^3 nh C, below 1e-6 of T's size for h = 1e-3 at these s; 1e-5 is asked."""
    B, NP, J = 2, 257, 129
    nrm, pos, cam, L, C = _problem(B, NP, J, seed=8)
    s = torch.rand(NP, generator=torch.Generator().manual_seed(9), dtype=torch.float64) * 495 + 5 if shin is None else shin
    vis = torch.rand(1, NP, J, generator=torch.Generator().manual_seed(10)) < 0.6
    for v in (None, vis):
        _, S0, T = MR.shade_terms_ref(nrm, pos, cam, L, C, s, vis=v)
        h = 1e-3
        fd = (MR.shade_terms_ref(nrm, pos, cam, L, C, s + h, vis=v)[1] - MR.shade_terms_ref(nrm, pos, cam, L, C, s - h, vis=v)[1]) / (2 * h)
        assert torch.isfinite(T).all() and float(T.abs().max()) > 0 and float(T.max()) <= 0.0
        assert float((T - fd).abs().max()) <= 1e-5 * float(T.abs().max())
        # the autograd of S, which the GPU tests use for the shininess gradient, is the same derivative
        sp = torch.as_tensor(s, dtype=torch.float64).clone().requires_grad_(True)
        S1 = MR.shade_terms_ref(nrm, pos, cam, L, C, sp, vis=v)[1]
        w = torch.randn(B, NP, 3, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
        (gs,) = torch.autograd.grad((S1 * w).sum(), sp)
        want = (w * T).sum(dim=(0, 2)) if sp.numel() > 1 else (w * T).sum()
        assert float((gs - want).abs().max()) <= 1e-12 * float((w.abs() * T.abs()).sum(dim=(0, 2)).max()) * (NP if sp.numel() == 1 else 1)
        bgp = (nrm == 0).all(-1)
        assert float(S0[:, bgp].abs().max()) == 0.0 and float(T[:, bgp].abs().max()) == 0.0


def test_compose_materials_shapes_and_gradients():
    from reni_amd.envmap_shader import compose_materials, specular_norm
    g = torch.Generator().manual_seed(3)
    B, NP = 2, 7
    D, S = torch.rand(B, NP, 3, generator=g, dtype=torch.float64), torch.rand(B, NP, 3, generator=g, dtype=torch.float64)
    a = torch.rand(NP, 3, generator=g, dtype=torch.float64, requires_grad=True)
    k = torch.rand(NP, generator=g, dtype=torch.float64, requires_grad=True)
    s = (torch.rand(NP, generator=g, dtype=torch.float64) * 100 + 2).requires_grad_(True)
    col = compose_materials(D, S, a, k, s)
    assert col.shape == (B, NP, 3)
    assert torch.allclose(col, MR.compose_ref(D, S, a.detach(), k.detach(), s.detach()), rtol=1e-14, atol=0)
    ga, gk, gs = torch.autograd.grad(col.sum(), (a, k, s))
    n = MR.specular_norm_ref(s.detach())
    assert torch.allclose(ga, D.sum(0), rtol=1e-13) and torch.allclose(gk, (n[:, None] * S).sum(dim=(0, 2)), rtol=1e-13)
    assert torch.allclose(gs, (k.detach() * MR.specular_norm_ds_ref(s.detach()))[:, None].mul(S).sum(dim=(0, 2)), rtol=1e-12)
    assert torch.allclose(specular_norm(torch.tensor(500.0, dtype=torch.float64)), torch.tensor(502.0 / 8.0, dtype=torch.float64), rtol=1e-12)
    # scalars, one albedo per channel, float32 terms
    col = compose_materials(D.float(), S.float(), torch.tensor([0.1, 0.2, 0.3]), 0.5, torch.tensor(20.0))
    assert col.dtype == torch.float32 and col.shape == (B, NP, 3)
    for bad in (torch.rand(NP + 1, 3), torch.rand(NP, 2), torch.rand(4), torch.rand(1, NP, 3)):
        with pytest.raises(ValueError, match="albedo"):
            compose_materials(D, S, bad, 0.5, 20.0)
    for bad in (torch.rand(NP + 1), torch.rand(NP, 1), torch.rand(2, NP)):
        with pytest.raises(ValueError, match="ks"):
            compose_materials(D, S, 0.5, bad, 20.0)
        with pytest.raises(ValueError, match="shininess"):
            compose_materials(D, S, 0.5, 0.5, bad + 1.0)
    with pytest.raises(ValueError):
        compose_materials(D, S[:, :-1], 0.5, 0.5, 20.0)


def test_python_argument_errors_come_before_the_library():
    from reni_amd import _lib, lighting, ops
    from reni_amd.envmap_shader import (EnvironmentMap, SpatialMaterials, blinn_phong_shading_materials, shade_terms)
    NP, J = 6, 40
    nrm, pos, cam = torch.randn(NP, 3), torch.randn(NP, 3), torch.zeros(3)
    dirs, C = torch.randn(J, 3), torch.rand(2, J, 3)
    gD = torch.rand(2, NP, 3)
    good = torch.zeros(1, NP, 2, dtype=torch.int32)
    calls = (lambda **k: ops.envmap_shade_terms(k.get("nrm", nrm), pos, cam, k.get("dirs", dirs), C, k.get("s", 10.0), vis=k.get("vis")),
             lambda **k: ops.envmap_shade_terms_backward(k.get("nrm", nrm), pos, cam, k.get("dirs", dirs), gD, gD, k.get("s", 10.0),
                                                         vis=k.get("vis")))
    for call in calls:
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
        # well-formed calls on CPU tensors: there is no CPU path
        for kw in ({}, {"vis": good}, {"s": torch.full((NP,), 10.0)}):
            with pytest.raises(_lib.RENILibraryError, match="GPU"):
                call(**kw)
    # the autograd layer: the geometry, the directions and the mask are constants
    env = EnvironmentMap(environment_map=C, directions=dirs.expand(2, J, 3), sineweight=torch.ones(1, J, 1))
    with pytest.raises(ValueError, match="normals.*require grad"):
        shade_terms(nrm.clone().requires_grad_(True), pos, cam, env, 10.0)
    with pytest.raises(ValueError, match="positions.*require grad"):
        shade_terms(nrm, pos.clone().requires_grad_(True), cam, env, 10.0)
    with pytest.raises(ValueError, match="camera.*require grad"):
        shade_terms(nrm, pos, cam.clone().requires_grad_(True), env, 10.0)
    env_g = EnvironmentMap(environment_map=C, directions=dirs.expand(2, J, 3).clone().requires_grad_(True), sineweight=torch.ones(1, J, 1))
    with pytest.raises(ValueError, match="directions.*require grad"):
        shade_terms(nrm, pos, cam, env_g, 10.0)
    with pytest.raises(ValueError, match="require grad"):
        shade_terms(nrm, pos, cam, env, 10.0, vis=torch.zeros(1, NP, 2, requires_grad=True))
    with pytest.raises(ValueError, match="shininess"):
        shade_terms(nrm, pos, cam, env, torch.rand(NP + 1) + 1)
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        shade_terms(nrm, pos, cam, env, torch.full((NP,), 10.0, requires_grad=True))
    with pytest.raises(_lib.RENILibraryError, match="GPU"):
        blinn_phong_shading_materials(nrm, pos, cam, env, torch.rand(NP, 3), 0.3, 40.0, vis=good)
    with pytest.raises(ValueError, match="SpatialMaterials"):
        lighting.shade_sampled(lighting.LightSamples.__new__(lighting.LightSamples), nrm, pos, cam, materials="shiny")
    with pytest.raises(ValueError, match="required without materials"):
        lighting.shade_sampled(lighting.LightSamples.__new__(lighting.LightSamples), nrm, pos, cam)


def test_spatial_materials_shapes_parameters_and_clamp():
    from reni_amd.envmap_shader import SpatialMaterials, compose_materials
    m = SpatialMaterials(albedo=0.5, ks=0.3, shininess=40.0)
    assert list(m.parameters()) == [] and set(dict(m.named_buffers())) == {"albedo", "ks", "shininess"}
    a, k, s = m.values()
    assert a.shape == () and k.shape == () and float(s) == 40.0
    S_ = 4
    m = SpatialMaterials(albedo=torch.rand(S_, S_, 3), ks=torch.rand(S_, S_), shininess=torch.rand(S_ * S_) * 100 + 1,
                         learn=("albedo", "shininess"))
    assert set(dict(m.named_parameters())) == {"albedo", "shininess"} and set(dict(m.named_buffers())) == {"ks"}
    a, k, s = m.values()
    assert a.shape == (16, 3) and k.shape == (16,) and s.shape == (16,)
    D, S = torch.rand(2, 16, 3), torch.rand(2, 16, 3)
    compose_materials(D, S, a, k, s).sum().backward()
    assert m.albedo.grad.shape == (16, 3) and m.shininess.grad.shape == (16,) and torch.isfinite(m.shininess.grad).all()
    for alb in (torch.tensor([0.2, 0.4, 0.6]), torch.rand(16, 3)):
        assert compose_materials(D, S, *SpatialMaterials(alb, 0.5, 20.0).values()).shape == (2, 16, 3)
    # the clamp: an optimiser that walks the raw value out of [1, 2000] never hands the kernels s <= 0
    m = SpatialMaterials(shininess=torch.tensor([-3.0, 0.0, 0.5, 40.0, 5000.0]), learn="shininess")
    assert m.values()[2].tolist() == [1.0, 1.0, 1.0, 40.0, 2000.0]
    assert SpatialMaterials(shininess=1e6, shininess_max=100.0).values()[2].item() == 100.0
    assert m.shininess_min == 1.0 and m.shininess_max == 2000.0
    for bad in ({"albedo": torch.rand(4)}, {"albedo": torch.rand(5, 2)}, {"albedo": torch.rand(2, 3, 3)}, {"ks": torch.rand(3, 4)},
                {"shininess": torch.rand(2, 2, 2)}, {"learn": ("kd",)}, {"albedo": torch.rand(9, 3), "ks": torch.rand(8)},
                {"shininess_min": 0.0}):
        with pytest.raises(ValueError):
            SpatialMaterials(**bad)
    # a renderer takes it in place of the scalars (nothing is rendered here: that needs the GPU)
    from reni_amd.mesh import HipMeshRenderer, MeshRasterizer
    r = HipMeshRenderer(MeshRasterizer(), materials=SpatialMaterials(albedo=torch.rand(16, 3), learn=("albedo",)))
    assert r.spatial and [n for n, _ in r.named_parameters()] == ["materials.albedo"]
    assert not HipMeshRenderer(MeshRasterizer(), kd=0.5).spatial
    with pytest.raises(ValueError, match="kd"):
        HipMeshRenderer(MeshRasterizer())
