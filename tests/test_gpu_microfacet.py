"""GPU tests of the microfacet (GGX) materials (reni_envmap_shade_ggx[_backward|_dpixel], envmap_shader.shade_terms_ggx /
compose_microfacet / MicrofacetMaterials, textures.TexturedMicrofacetMaterials, HipMeshRenderer(materials=)) against the float64
reference tests/microfacet_ref.py, whose autograd is the reference for every gradient.

Tolerances (tests/microfacet_ref.py: ``factors``, ``over_bound``).  The reference's own definition is evaluated in float32 torch on
the CPU over the 42 cases below; a quantity's factor is four times the worst error ratio of that evaluation against float64, and
its bound is max(factor x scale, 2e-5 x largest reference value) plus the allowance of the pairs within 1e-6 of a gate (x_l, x_h,
x_v: k has a step at x_h = 0, the normals' gradient steps at all three).  The scale is the largest reference value for the sums,
dC, the colours, d base_color and d metallic; d alpha, d normals and d roughness are held per pixel against the sum of the
absolute values of their parts (``grad_scales``): the 2 / alpha term of d ln k / d alpha and its three negative terms cancel, as
the parts of ds did in the Blinn-Phong terms.  Measured ratios and the device's worst error over bound: DESIGN 4.4m.
"""
import functools
import math
import os
import types

import pytest
import torch

from tests import microfacet_ref as GR
from tests import normal_map_ref as NR
from tests import texture_ref as TR
from tests import visibility_ref as VR
from tests.util import uv_sphere

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")
F64 = torch.float64
EPS24 = 2.0 ** -24

CASES = GR.all_cases()                                           # 7 shapes x 3 roughnesses
PAIRS = [(s, k) for s in GR.SHAPES for k in GR.ROUGHNESS]


def _pack(vis_bool):
    return torch.from_numpy(VR.pack_bits(vis_bool.numpy())).to(DEV)


@functools.lru_cache(maxsize=None)
def _dev(B, NP, J, per_image, kind):
    c = GR.case(B, NP, J, per_image, kind)
    d = types.SimpleNamespace(**{k: getattr(c, k).to(DEV) for k in ("nrm", "pos", "C", "alpha", "rough", "gD", "gS0", "gS1", "w")})
    d.L = (c.L if per_image else c.L[0]).to(DEV)
    d.vis = _pack(c.vis)
    return c, d


def _fwd(c, d, vis=None, alpha=None, C=None, nrm=None):
    from reni_amd import ops
    return ops.envmap_shade_ggx(d.nrm if nrm is None else nrm, d.pos, c.cam, d.L, d.C if C is None else C,
                                d.alpha if alpha is None else alpha, vis=vis)


def _bwd(c, d, vis=None, alpha=None):
    from reni_amd import ops
    return ops.envmap_shade_ggx_backward(d.nrm, d.pos, c.cam, d.L, d.gD, d.gS0, d.gS1, d.alpha if alpha is None else alpha, vis=vis)


def _dpx(c, d, vis=None, alpha=None, need_dn=True):
    from reni_amd import ops
    return ops.envmap_shade_ggx_dpixel(d.nrm, d.pos, c.cam, d.L, d.C, d.gD, d.gS0, d.gS1, d.alpha if alpha is None else alpha,
                                       vis=vis, need_dn=need_dn)


def _held(name, got, entry):
    """One quantity against its float64 entry: print the figure, then assert."""
    fac = GR.factors()[name]
    r = GR.over_bound(got, entry, fac)
    print(f"{name}: error over bound {r:.3f} (factor {fac:.3e}, largest reference {float(entry[0].abs().max()):.3e})")
    assert torch.isfinite(torch.as_tensor(got)).all(), name
    assert r <= 1.0, (name, r)
    return r


@pytest.mark.parametrize("B,NP,J,per_image,kind", CASES)
@pytest.mark.parametrize("mask", GR.MASKS)
def test_terms_and_every_gradient_match_float64(B, NP, J, per_image, kind, mask):
    from reni_amd.envmap_shader import EnvironmentMap, MicrofacetMaterials
    c, d = _dev(B, NP, J, per_image, kind)
    ref = GR.reference(B, NP, J, per_image, kind, mask)
    vis = None if mask == "none" else d.vis
    D, S0, S1 = _fwd(c, d, vis)
    dC = _bwd(c, d, vis)
    da, dn = _dpx(c, d, vis)
    for name, got in (("D", D), ("S0", S0), ("S1", S1), ("dC", dC), ("dalpha", da), ("dn", dn)):
        _held(name, got, ref[name])
    # the autograd path: map, base colour, roughness and metallic through shade_terms_ggx + compose_microfacet
    Cg = d.C.clone().requires_grad_(True)
    env = EnvironmentMap(environment_map=Cg, directions=d.L if per_image else d.L.expand(B, -1, -1),
                         sineweight=torch.ones(1, J, 1, device=DEV))
    m = MicrofacetMaterials(c.base_color, c.rough, c.metallic, learn=("base_color", "roughness", "metallic")).to(DEV)
    col = m.shade(d.nrm, d.pos, c.cam, env, vis=vis)
    _held("colours", col, ref["colours"])
    (col * d.w).sum().backward()
    _held("dC_col", Cg.grad, ref["dC_col"])
    _held("d_base_color", m.base_color.grad, ref["d_base_color"])
    _held("d_roughness", m.roughness.grad, ref["d_roughness"])
    _held("d_metallic", m.metallic.grad, ref["d_metallic"])
    # background pixels: exact zeros in every term and every per-pixel gradient
    if bool(c.bg.any()):
        bg = c.bg.to(DEV)
        for t in (D, S0, S1, col.detach()):
            assert float(t[:, bg].abs().max()) == 0.0
        per_pixel = [da, dn, m.base_color.grad, m.metallic.grad] + ([m.roughness.grad] if c.rough.numel() > 1 else [])
        for t in per_pixel:
            assert float(t[bg].abs().max()) == 0.0


@pytest.mark.parametrize("shape,kind", PAIRS)
def test_bit_properties(shape, kind):
    from reni_amd import ops
    B, NP, J, per_image = shape
    c, d = _dev(B, NP, J, per_image, kind)
    NB, JW = c.L.shape[0], (J + 31) // 32
    ones = _pack(torch.ones(NB, NP, J, dtype=torch.bool))
    zeros = torch.zeros(NB, NP, JW, dtype=torch.int32, device=DEV)
    plain = list(_fwd(c, d)) + [_bwd(c, d)] + list(_dpx(c, d))
    # an all-ones mask gives the unmasked instance's bits, an all-zeros mask exact zeros
    for a, b in zip(plain, list(_fwd(c, d, ones)) + [_bwd(c, d, ones)] + list(_dpx(c, d, ones))):
        assert torch.equal(a, b)
    for t in list(_fwd(c, d, zeros)) + [_bwd(c, d, zeros)] + list(_dpx(c, d, zeros)):
        assert float(t.abs().max()) == 0.0
    # repeatability, under the random mask too
    for vis in (None, d.vis):
        first = list(_fwd(c, d, vis)) + [_bwd(c, d, vis)] + list(_dpx(c, d, vis))
        again = list(_fwd(c, d, vis)) + [_bwd(c, d, vis)] + list(_dpx(c, d, vis))
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        # D is the Blinn-Phong terms' diffuse sum, bit for bit
        assert torch.equal(first[0], ops.envmap_shade_terms(d.nrm, d.pos, c.cam, d.L, d.C, 20.0, vis=vis)[0])
        # asking for the normals' gradient does not move the roughness's
        da_only, none = _dpx(c, d, vis, need_dn=False)
        assert none is None and torch.equal(da_only, first[4])
        # exact zeros on background pixels
        if bool(c.bg.any()):
            bg = c.bg.to(DEV)
            assert all(float(t[:, bg].abs().max()) == 0.0 for t in first[:3]) and all(float(t[bg].abs().max()) == 0.0 for t in first[4:])
    # a stride-1 alpha of one value is the stride-0 result
    if c.alpha.numel() == 1:
        per_pixel = d.alpha.expand(NP).contiguous()
        for a, b in zip(plain, list(_fwd(c, d, alpha=per_pixel)) + [_bwd(c, d, alpha=per_pixel)] + list(_dpx(c, d, alpha=per_pixel))):
            assert torch.equal(a, b)


ADJOINT = [((3, 1000, 515, False), "r07"), ((3, 1000, 515, False), "r02"), ((2, 500, 300, True), "r07"), ((9, 64, 129, False), "per_pixel")]


@pytest.mark.parametrize("shape,kind", ADJOINT)
@pytest.mark.parametrize("mask", GR.MASKS)
def test_backward_is_the_adjoint_of_the_forward_kernel(shape, kind, mask):
    """<dC, dC'> against <g, terms(dC')>: the forward kernel is linear in the colours.  Both sides are fp32 results; each is
    allowed its own float64-parity bound (the quantity's factor, at least 2e-5, of its largest value, times the l1 norm of what
    it is paired with)."""
    B, NP, J, per_image = shape
    c, d = _dev(B, NP, J, per_image, kind)
    vis = None if mask == "none" else d.vis
    g = torch.Generator().manual_seed(23)
    dCp = torch.rand(B, J, 3, generator=g).to(DEV)
    fac = {k: max(v, GR.FLOOR) for k, v in GR.factors().items()}
    terms = _fwd(c, d, vis, C=dCp)
    dC = _bwd(c, d, vis)
    lhs = float((dC.double() * dCp.double()).sum())
    rhs = sum(float((t.double() * u.double()).sum()) for t, u in zip(terms, (d.gD, d.gS0, d.gS1)))
    tol = fac["dC"] * float(dC.abs().max()) * float(dCp.abs().sum()) + sum(
        fac[n] * float(t.abs().max()) * float(u.abs().sum()) for n, t, u in zip(("D", "S0", "S1"), terms, (d.gD, d.gS0, d.gS1)))
    print(f"adjointness {shape} {kind} {mask}: {lhs:.8e} vs {rhs:.8e}, |difference| / tol {abs(lhs - rhs) / tol:.3e}")
    assert abs(lhs - rhs) <= tol and abs(lhs) > 0


@pytest.mark.parametrize("shape,kind", ADJOINT)
@pytest.mark.parametrize("mask", GR.MASKS)
def test_dpixel_matches_a_central_difference_of_the_forward_kernel(shape, kind, mask):
    """Per pixel: d_normals . dn and d_alpha da against (F(x + e dx) - F(x - e dx)) / 2e with F = sum gD D + gS0 S0 + gS1 S1 of
    the DEVICE's forward kernel.  The tolerance has three parts: (i) the difference's own truncation error, taken from the
    float64 reference evaluated at the very same fp32 inputs (|analytic - difference| there); (ii) the forward's rounding
    through the difference, 2 (J + 8 + 2 / alpha_p) 2^-24 sum |g| |term| / 2e -- J accumulations, and a pair's k carries the
    rounding of d twice, where the cross product's absolute error 2 sin(t) 2^-24 meets d >= alpha^2 + sin^2(t): 2^-24 / alpha at
    worst; (iii) the analytic side's own bound (its factor on the per-pixel scale, plus the gate allowance).  The step is a
    power of two per pixel.  For the normals (i) grows with e -- the diffuse sum has a kink wherever a texel crosses the horizon,
    and with hundreds of texels nearly every pixel has one inside the step -- and (ii) with 1 / e: e = 2^-6 where alpha >= 1/4,
    2^-7 below, near their crossing.  Alpha has no kinks and its step is relative: e = 2^-5.  The median of tolerance / |value|
    is asserted below 1/4, so the comparison means something."""
    B, NP, J, per_image = shape
    c, d = _dev(B, NP, J, per_image, kind)
    ref = GR.reference(B, NP, J, per_image, kind, mask)
    vis, vis64 = (None, None) if mask == "none" else (d.vis, c.vis)
    fac = GR.factors()
    g = torch.Generator().manual_seed(17)
    dn = torch.nn.functional.normalize(torch.randn(NP, 3, generator=g), dim=-1) * c.nrm.norm(dim=1, keepdim=True)
    dal = (torch.rand(NP, generator=g) + 0.5) * c.alpha.expand(NP)
    a0 = c.alpha.expand(NP).contiguous()
    e_n = torch.where(a0 >= 0.25, torch.tensor(2.0 ** -6), torch.tensor(2.0 ** -7))
    e_a = torch.full((NP,), 2.0 ** -5)
    got_a, got_n = _dpx(c, d, vis)
    ups = (c.gD.double(), c.gS0.double(), c.gS1.double())

    def F(nrm, alpha):
        return sum((u * t.double().cpu()).sum(dim=(0, 2)) for u, t in zip(ups, _fwd(c, d, vis, alpha=alpha.to(DEV), nrm=nrm.to(DEV))))

    def F64_(nrm, alpha):
        return sum((u * t).sum(dim=(0, 2)) for u, t in zip(ups, GR.shade_terms_ggx_ref(nrm, c.pos, c.cam, c.L, c.C, alpha, vis=vis64)))

    T0 = _fwd(c, d, vis, alpha=a0.to(DEV))
    size = sum((u.abs() * t.double().cpu().abs()).sum(dim=(0, 2)) for u, t in zip(ups, T0))
    noise = 2 * (J + 8 + 2 / a0.double()) * EPS24 * size
    fg = ~c.bg
    for name, got, e, x_plus, x_minus, scale, allow in (
            ("d_normals", (got_n.double().cpu() * dn.double()).sum(1), e_n.double(), (c.nrm + e_n[:, None] * dn, a0),
             (c.nrm - e_n[:, None] * dn, a0), ref["dn"][1][:, 0] * dn.double().abs().sum(1), ref["dn"][2][:, 0] * dn.double().abs().sum(1)),
            ("d_alpha", got_a.double().cpu() * dal.double(), e_a.double(), (c.nrm, a0 + e_a * dal), (c.nrm, a0 - e_a * dal),
             ref["dalpha"][1] * dal.double(), ref["dalpha"][2] * dal.double())):
        rhs = (F(*x_plus) - F(*x_minus)) / (2 * e)          # (float32 inputs: the very values the kernel is given)
        fd_ii = noise / (2 * e)
        key = "dn" if name == "d_normals" else "dalpha"
        lhs64 = (ref["dn"][0] * dn.double()).sum(1) if key == "dn" else ref["dalpha"][0] * dal.double()
        rhs64 = (F64_(x_plus[0].double(), x_plus[1].double()) - F64_(x_minus[0].double(), x_minus[1].double())) / (2 * e)
        fd_i = (lhs64 - rhs64).abs()
        own = fac[key] * scale + allow
        tol = fd_i + fd_ii + own
        rel = float((tol[fg] / got[fg].abs().clamp_min(1e-300)).median())
        worst = float(((got - rhs).abs()[fg] / tol[fg].clamp_min(1e-300)).max())
        print(f"{name} vs central difference {shape} {kind} {mask}: worst |lhs - rhs| / tol {worst:.3f}; median tol / |lhs| {rel:.3e} "
              f"(difference's own share {float((fd_i[fg] / tol[fg].clamp_min(1e-300)).median()):.2f})")
        assert rel < 0.25
        assert bool(((got - rhs).abs() <= tol).all())
        assert float(got[c.bg].abs().max() if bool(c.bg.any()) else 0.0) == 0.0


def test_dpixel_runs_only_when_asked_for(monkeypatch):
    from reni_amd import ops
    from reni_amd.envmap_shader import EnvironmentMap, shade_terms_ggx
    B, NP, J = 3, 1000, 515
    c, d = _dev(B, NP, J, False, "per_pixel")

    def env(grad=True):  # (a fresh graph per backward)
        return EnvironmentMap(environment_map=d.C.clone().requires_grad_(grad), directions=d.L.expand(B, -1, -1),
                              sineweight=torch.ones(1, J, 1, device=DEV))

    want_a, want_n = _dpx(c, d, need_dn=False)[0], _dpx(c, d)[1]
    calls, real = [], ops.envmap_shade_ggx_dpixel
    monkeypatch.setattr(ops, "envmap_shade_ggx_dpixel", lambda *a, **k: calls.append(k.get("need_dn")) or real(*a, **k))
    sum(t.sum() for t in shade_terms_ggx(d.nrm, d.pos, c.cam, env(), d.alpha)).backward()   # the map alone: no dpixel call
    assert calls == []
    al = d.alpha.clone().requires_grad_(True)
    T = shade_terms_ggx(d.nrm, d.pos, c.cam, env(False), al)
    ((T[0] * d.gD).sum() + (T[1] * d.gS0).sum() + (T[2] * d.gS1).sum()).backward()
    assert calls == [False] and torch.equal(al.grad, want_a)
    n = d.nrm.clone().requires_grad_(True)
    T = shade_terms_ggx(n, d.pos, c.cam, env(False), d.alpha)
    ((T[0] * d.gD).sum() + (T[1] * d.gS0).sum() + (T[2] * d.gS1).sum()).backward()
    assert calls == [False, True] and torch.equal(n.grad, want_n)


# ------------------------------------------------------------------------------------------------- renderer
@functools.lru_cache(maxsize=None)
def _sphere_mesh():
    from reni_amd.mesh import Meshes
    v, f, vt, ft = (t.to(DEV) for t in uv_sphere())
    return Meshes(verts=[v], faces=[f], verts_uvs=[vt], faces_uvs=[ft])


def _envmap(C, W=32):
    from reni_amd.envmap_shader import EnvironmentMap
    from reni_amd.utils import get_directions, get_sineweight
    D, Sw = get_directions(W).to(DEV), get_sineweight(W).to(DEV)
    return EnvironmentMap(environment_map=C, directions=D.expand(C.shape[0], -1, -1), sineweight=Sw), D[0], Sw


def _view(azim, S, shadows, materials):
    from reni_amd.mesh import FoVPerspectiveCameras, HipMeshRenderer, MeshRasterizer, RasterizationSettings, look_at_view_transform
    R, T = look_at_view_transform(2.7, 10.0, azim, device=DEV)
    ras = MeshRasterizer(cameras=FoVPerspectiveCameras(device=DEV), raster_settings=RasterizationSettings(image_size=S))
    r = HipMeshRenderer(ras, materials=materials, shader_cameras=FoVPerspectiveCameras(R=R, T=T, device=DEV), shadows=shadows)
    return r, R, T


def _bumps(H, W, amp, seed):
    g = torch.Generator().manual_seed(seed)
    xy = (torch.rand(H, W, 2, generator=g) * 2 - 1) * amp
    z = torch.sqrt(1 - (xy ** 2).sum(-1, keepdim=True))
    return (torch.cat([xy, z], -1) + 1) / 2   # encoded in [0, 1]


def _transpose_lookup(tex, taps, upstream):
    """float64: d (sum upstream . fetch(pyramid(tex))) / d tex through the DEVICE's taps."""
    t64 = tex.to(F64).requires_grad_(True)
    t3 = t64 if t64.dim() == 3 else t64.unsqueeze(-1)
    val = TR.fetch_ref(TR.pyramid_ref(t3, taps.levels), taps.index.cpu().long(), taps.weight.cpu().double())
    return torch.autograd.grad((val * upstream).sum(), t64)[0]


@pytest.mark.parametrize("shadows", [False, True])
def test_textured_microfacet_renderer_matches_float64(shadows):
    """The UV sphere at 32 x 32 under a 16 x 32 map, B = 2; base colour, roughness, metallic and normal textures of four sizes.

    The float64 chain starts at the device's taps: every texture is fetched through them in float64 and the device's fetch
    is held to that first (32 2^-24 of the fetched value: at most five box levels of three roundings each and the fetch's nine,
    all terms >= 0).  From the device's own per-pixel values (so that the shader's parity is not charged with the fetch's
    rounding) the chain goes on in float64: clamps, perturb_normals, the definition, compose_microfacet.  Colours are held to
    the 42 cases' bound plus the fp32 rounding of the bent normal (8 2^-24, relative) times the colours'
    sensitivity to it, |d colour / d n|_1 |n| from float64 autograd.  A texture's gradient, texel by texel, is held to the
    gather bound of DESIGN 4.4k on the float64 upstream gradient plus the per-pixel upstream bound (the 42 cases' rule on this
    scene's scales; for the normal texture pushed through perturb_normals and the decoding as in 4.4l) times the texel's coverage."""
    from reni_amd.mesh import unpack_visibility
    from reni_amd.textures import TexturedMicrofacetMaterials
    mesh = _sphere_mesh()
    S, B, J = 32, 2, 512
    NP = S * S
    g = torch.Generator().manual_seed(71)
    tex = {"base_color": 0.2 + 0.6 * torch.rand(16, 32, 3, generator=g), "roughness": 0.2 + 0.6 * torch.rand(8, 16, generator=g),
           "metallic": torch.rand(4, 8, generator=g), "normal": _bumps(8, 16, 0.4, 72)}
    strength = 1.5
    mat = TexturedMicrofacetMaterials(tex["base_color"], tex["roughness"], tex["metallic"], normal=tex["normal"],
                                      normal_strength=strength, learn=tuple(tex)).to(DEV)
    r, R, T = _view(25.0, S, shadows, mat)
    ras = r.rasterizer
    C = torch.rand(B, J, 3, generator=g) * 4.0
    env, Dirs, Sw = _envmap(C.to(DEV))
    wcol = torch.randn(B, S, S, 3, generator=g)
    col, _ = r(meshes_world=mesh, R=R, T=T, envmap=env)
    (col * wcol.to(DEV)).sum().backward()
    assert torch.equal(r(meshes_world=mesh, R=R, T=T, envmap=env)[0], col)
    _, nrm, pos = ras.gbuffer(mesh, R, T)
    seen = ~(nrm.cpu() == 0).all(-1)
    # the device's per-pixel values against the float64 fetch through its own taps
    taps = {k: ras.texture_taps(mesh, R, T, size=tuple(v.shape[:2])) for k, v in tex.items()}
    dev_vals = dict(zip(mat.NAMES, (v.detach().cpu() for v in mat.values(ras, mesh, R, T))))
    m_dev = mat.tangent_space_normals(ras, mesh, R, T).detach().cpu()
    for k in mat.NAMES:
        t3 = tex[k].to(F64) if tex[k].dim() == 3 else tex[k].to(F64).unsqueeze(-1)
        f64 = TR.fetch_ref(TR.pyramid_ref(t3, taps[k].levels), taps[k].index.cpu().long(), taps[k].weight.cpu().double())
        f64 = f64 if tex[k].dim() == 3 else f64[:, 0]
        err = (dev_vals[k].double() - f64)[seen].abs()
        assert bool((err <= 32 * EPS24 * f64[seen].abs()).all()), k
    rf = dev_vals["roughness"][seen]
    assert float(rf.min()) > 0.1 and float(rf.max()) < 1.0   # the clamp is the identity on the pixels that are shaded
    # float64 from the device's per-pixel values
    t, b, valid = (x.cpu() for x in ras.pixel_tangents(mesh, R, T))
    m64 = m_dev.double().requires_grad_(True)
    n_bent = NR.perturb_normals_ref(nrm.cpu(), t, b, valid, m64, strength)
    vis = unpack_visibility(ras.visibility(mesh, R, T, Dirs), J).cpu() if shadows else None
    Cw = env.environment_map.detach().cpu()   # (the map times the sine weight, as the device holds it)
    prob = types.SimpleNamespace(B=B, NP=NP, J=J, nrm=n_bent.detach(), pos=pos.cpu(), cam=r.camera_center, L=Dirs.cpu()[None], C=Cw,
                                 rough=dev_vals["roughness"], alpha=dev_vals["roughness"] ** 2, base_color=dev_vals["base_color"],
                                 metallic=dev_vals["metallic"], w=wcol.reshape(B, NP, 3))
    prob.gD, prob.gS0, prob.gS1 = (u.float() for u in GR.composed_upstreams(prob))
    ent = GR.entries(prob, vis)
    fac = GR.factors()
    # colours: the cases' bound plus the bent normal's rounding times the colours' sensitivity to the normal
    nb = n_bent.detach().clone().requires_grad_(True)
    terms = GR.shade_terms_ggx_ref(nb, prob.pos, prob.cam, prob.L, prob.C, prob.rough.double() ** 2, vis=vis)
    col64 = GR.compose_microfacet_ref(*terms, prob.base_color.double(), prob.metallic.double())
    sens = torch.zeros(B, NP, 3, dtype=F64)
    for bi in range(B):
        for ci in range(3):
            (gn,) = torch.autograd.grad(col64[bi, :, ci].sum(), nb, retain_graph=True)   # (a pixel's colour depends on its own normal only)
            sens[bi, :, ci] = gn.abs().sum(1) * nb.detach().norm(dim=1)
    ref_c, scale_c, allow_c = ent["colours"]
    assert float((col64.detach() - ref_c).abs().max()) <= 1e-12 * float(ref_c.abs().max())
    rc = GR.over_bound(col.detach().reshape(B, NP, 3), (ref_c, scale_c, allow_c + 8 * EPS24 * sens), fac["colours"])
    print(f"renderer colours (shadows {shadows}): error over bound {rc:.3f}, largest colour {float(ref_c.abs().max()):.3e}")
    assert rc <= 1.0 and float(ref_c.abs().max()) > 0
    # texture gradients
    _, Kp, _, _ = TR.emulation_constants()
    uv = ras.pixel_uv(mesh, R, T)[0].cpu()
    (um,) = torch.autograd.grad((n_bent * ent["dn"][0]).sum(), m64)
    utol = {"base_color": GR.bound(ent["d_base_color"], fac["d_base_color"]).max(1).values,
            "roughness": GR.bound(ent["d_roughness"], fac["d_roughness"]), "metallic": GR.bound(ent["d_metallic"], fac["d_metallic"]),
            "normal": 2 * math.sqrt(3.0) * max(1.0, strength) * nrm.cpu().double().norm(dim=1)
                      * GR.bound(ent["dn"], fac["dn"]).max(1).values * valid.to(F64)}
    ups = {"base_color": ent["d_base_color"][0], "roughness": ent["d_roughness"][0][:, None], "metallic": ent["d_metallic"][0][:, None],
           "normal": 2 * um}
    for k in tex:
        want = _transpose_lookup(tex[k], taps[k], ups[k])
        C_ = 3 if tex[k].dim() == 3 else 1
        cover = _transpose_lookup(tex[k], taps[k], utol[k][:, None].expand(NP, C_))
        cover = cover[:, :, 0] if tex[k].dim() == 3 else cover
        cc = {"H0": tex[k].shape[0], "W0": tex[k].shape[1], "L": taps[k].levels, "uv": uv, "g": ups[k].detach(), "wrap": "clamp"}
        bound = TR.level0_grad_bound(Kp, cc, taps[k].index.cpu().long(), taps[k].weight.cpu().double()) + cover
        got = getattr(mat, k).grad.cpu().double()
        err = (got - want).abs()
        err = err.max(2).values if err.dim() == 3 else err
        nz = bound > 0
        print(f"{k} texture gradient (shadows {shadows}): error over bound {float((err[nz] / bound[nz]).max()):.3f}, "
              f"largest gradient {float(want.abs().max()):.3e}")
        assert float(want.abs().max()) > 0 and bool((err <= bound).all()), k


def test_two_views_share_a_roughness_texture_and_a_short_fit():
    """Two views share one material: the shared gradient is bit-equal to the sum of the single-view ones; 15 Adam steps on base
    colour, roughness and normal texture together, towards a rougher, bumpier, differently coloured target, lower the loss."""
    from reni_amd.textures import TexturedMicrofacetMaterials
    mesh = _sphere_mesh()
    S, B, J = 32, 2, 512
    g = torch.Generator().manual_seed(81)
    C = (torch.rand(B, J, 3, generator=g) * 4.0).to(DEV)
    env, _, _ = _envmap(C)
    gt = TexturedMicrofacetMaterials(base_color=0.2 + 0.6 * torch.rand(16, 32, 3, generator=g), roughness=0.3 + 0.5 * torch.rand(8, 16, generator=g),
                                     metallic=0.3, normal=_bumps(16, 32, 0.5, 82)).to(DEV)
    flat = torch.tensor([0.5, 0.5, 1.0]).expand(16, 32, 3)
    mat = TexturedMicrofacetMaterials(base_color=torch.full((16, 32, 3), 0.5), roughness=torch.full((8, 16), 0.5), metallic=0.3,
                                      normal=flat, learn=("base_color", "roughness", "normal")).to(DEV)
    names = ("base_color", "roughness", "normal")
    for shadows in (False, True):
        views = [_view(az, S, shadows, mat) for az in (0.0, 180.0)]
        with torch.no_grad():
            targets = [_view(az, S, shadows, gt)[0](meshes_world=mesh, R=R, T=T, envmap=env)[0] for az, (_, R, T) in zip((0.0, 180.0), views)]

        def loss_of(i):
            r, R, T = views[i]
            return ((r(meshes_world=mesh, R=R, T=T, envmap=env)[0] - targets[i]) ** 2).mean()

        def clear():
            for n in names:
                getattr(mat, n).grad = None

        single = []
        for i in (0, 1):
            clear()
            loss_of(i).backward()
            single.append([getattr(mat, n).grad.clone() for n in names])
        clear()
        (loss_of(0) + loss_of(1)).backward()
        for k, n in enumerate(names):
            assert float(single[0][k].abs().max()) > 0 and float(single[1][k].abs().max()) > 0, n
            assert torch.equal(getattr(mat, n).grad, single[0][k] + single[1][k]), n
    # a flat normal texture renders the bits of the material without one
    plain = TexturedMicrofacetMaterials(base_color=torch.full((16, 32, 3), 0.5), roughness=torch.full((8, 16), 0.5), metallic=0.3).to(DEV)
    ra, Ra, Ta = _view(25.0, S, True, plain)
    rb, Rb, Tb = _view(25.0, S, True, mat)
    assert torch.equal(ra(meshes_world=mesh, R=Ra, T=Ta, envmap=env)[0], rb(meshes_world=mesh, R=Rb, T=Tb, envmap=env)[0])
    opt = torch.optim.Adam([getattr(mat, n) for n in names], lr=0.03)
    losses = []
    for _ in range(15):
        opt.zero_grad()
        loss = loss_of(0) + loss_of(1)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("two-view base colour + roughness + normal fit: loss", losses[0], "->", losses[-1])
    assert all(torch.isfinite(getattr(mat, n)).all() for n in names) and losses[-1] < losses[0]


def test_spatial_microfacet_materials_through_build_hip_renderer():
    """MicrofacetMaterials (one value per render pixel) on the teapot, shadows off and on: the renderer's colours are
    microfacet_shading_materials' on its G-buffer, and every learnt input gets a finite, non-zero gradient."""
    from reni_amd.envmap_shader import MicrofacetMaterials, microfacet_shading_materials
    from reni_amd.mesh import build_hip_renderer
    S = 32
    g = torch.Generator().manual_seed(91)
    C = (torch.rand(2, 512, 3, generator=g) * 4.0).to(DEV)
    env, Dirs, _ = _envmap(C)
    for shadows in (False, True):
        m = MicrofacetMaterials(torch.rand(S, S, 3, generator=g), 0.15 + 0.8 * torch.rand(S, S, generator=g), torch.rand(S * S, generator=g),
                                learn=MicrofacetMaterials.NAMES)
        r, R, T, teapot = build_hip_renderer(TEAPOT, 0, S, None, "cuda", shadows=shadows, materials=m)
        col = r(meshes_world=teapot, R=R, T=T, envmap=env)[0]
        _, nrm, pos = r.rasterizer.gbuffer(teapot, R, T)
        vis = r.rasterizer.visibility(teapot, R, T, Dirs) if shadows else None
        want = microfacet_shading_materials(nrm, pos, r.camera_center, env, *m.values(), vis=vis)
        assert torch.equal(col.reshape(2, S * S, 3), want) and float(col.abs().max()) > 0
        col.sum().backward()
        for n in m.NAMES:
            gr = getattr(m, n).grad
            assert torch.isfinite(gr).all() and float(gr.abs().max()) > 0, n


def test_blinn_phong_paths_keep_their_bits_around_a_microfacet_render():
    from reni_amd import ops
    from reni_amd.envmap_shader import EnvironmentMap, shade_terms
    from reni_amd.textures import TexturedMaterials, TexturedMicrofacetMaterials
    mesh = _sphere_mesh()
    S = 32
    g = torch.Generator().manual_seed(61)
    C = (torch.rand(2, 512, 3, generator=g) * 4.0).to(DEV)
    env, _, _ = _envmap(C)
    tex = TexturedMaterials(albedo=torch.rand(8, 8, 3, generator=g), ks=torch.rand(4, 4, generator=g), normal=_bumps(8, 8, 0.5, 62)).to(DEV)
    c, d = _dev(3, 1000, 515, False, "r02")
    envc = EnvironmentMap(environment_map=d.C, directions=d.L.expand(3, -1, -1), sineweight=torch.ones(1, 515, 1, device=DEV))

    def old():
        outs = [ops.envmap_shade(d.nrm, d.pos, c.cam, d.L, d.C, 40.0, 0.6, 0.4, vis=d.vis)]
        outs += list(shade_terms(d.nrm, d.pos, c.cam, envc, 20.0, vis=d.vis))
        for shadows in (False, True):
            r, R, T = _view(40.0, S, shadows, tex)
            outs.append(r(meshes_world=mesh, R=R, T=T, envmap=env)[0])
        return outs

    before = old()
    mat = TexturedMicrofacetMaterials(base_color=torch.rand(8, 8, 3, generator=g), roughness=0.2 + 0.6 * torch.rand(8, 8, generator=g),
                                      normal=_bumps(8, 8, 0.5, 63), learn=("roughness", "normal")).to(DEV)
    r, R, T = _view(40.0, S, True, mat)
    r(meshes_world=mesh, R=R, T=T, envmap=env)[0].sum().backward()
    assert float(mat.roughness.grad.abs().max()) > 0 and float(mat.normal.grad.abs().max()) > 0
    for a, b in zip(before, old()):
        assert torch.equal(a, b)
