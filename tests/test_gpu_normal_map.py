"""GPU tests of the normal-mapped materials: reni_envmap_shade_terms_dnormals against the float64 definition
(tests/normal_map_ref.py), its bit properties and adjointness, envmap_shader.shade_terms_normals, and the renderer with a
normal texture (tangent frames, perturb_normals, TexturedMaterials(normal=), HipMeshRenderer).

d_normals, per pixel: |device - float64| <= K unit + jump with ``normal_map_ref.dnormals_bound``'s unit and jump and K =
``normal_map_ref.emulation_constant()``: four times the worst ratio an fp32 emulation in kernel order reaches over the same
cases.  At shininess 1 a gate that flips under rounding may add its step: |b'| of a pair with |x_h| < 1e-6, |a| of one with
|x_l| < 1e-6.  No case and no pixel is left out.
"""
import functools
import math
import os

import pytest
import torch

from tests import normal_map_ref as NR
from tests import shade_materials_ref as MR
from tests import texture_ref as TR
from tests import visibility_ref as VR
from tests.util import uv_sphere

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")
CASES = NR.all_cases()


def _pack(vis_bool):
    return torch.from_numpy(VR.pack_bits(vis_bool.numpy())).to(DEV)


@functools.lru_cache(maxsize=None)
def _dev(B, NP, J, per_image, kind):
    c = NR.case(B, NP, J, per_image, kind)
    d = {k: c[k].to(DEV) for k in ("nrm", "pos", "C", "shin", "gD", "gS")}
    d["L"] = (c["L"] if per_image else c["L"][0]).to(DEV)
    d["vis"] = _pack(c["vis"])
    return c, d


def _dn(c, d, vis=None, shin=None, nrm=None):
    from reni_amd import ops
    return ops.envmap_shade_terms_dnormals(d["nrm"] if nrm is None else nrm, d["pos"], c["cam"], d["L"], d["C"], d["gD"], d["gS"],
                                           d["shin"] if shin is None else shin, vis=vis)


@pytest.mark.parametrize("B,NP,J,per_image,kind", CASES)
@pytest.mark.parametrize("mask", NR.MASKS)
def test_dnormals_match_the_float64_definition(B, NP, J, per_image, kind, mask):
    c, d = _dev(B, NP, J, per_image, kind)
    K, worst_emu = NR.emulation_constant()
    got = _dn(c, d, d["vis"] if mask == "random" else None)
    assert got.shape == (NP, 3) and got.dtype == torch.float32 and torch.isfinite(got).all()
    ratio, ref = NR.error_ratio(got.cpu(), c, mask)
    raw = float(((got.cpu().double() - ref["d"]).abs().max(1).values / ref["unit"].clamp_min(1e-300))[ref["unit"] > 0].max())
    print(f"d_normals {B}x{NP}x{J} {kind} {mask}: worst error / unit {ratio:.3f} (K {K:.3f}, emulation's worst {worst_emu:.3f}); "
          f"largest gradient {float(ref['d'].abs().max()):.3e}, pixels with a gate within 1e-6: {int((ref['jump'] > 0).sum())} (ratio without their allowance {raw:.3f})")
    assert float(ref["d"].abs().max()) > 0
    assert ratio <= K
    if bool(c["bg"].any()):
        assert float(got[c["bg"].to(DEV)].abs().max()) == 0.0


@pytest.mark.parametrize("B,NP,J,per_image,kind", CASES)
def test_bit_properties(B, NP, J, per_image, kind):
    c, d = _dev(B, NP, J, per_image, kind)
    plain = _dn(c, d)
    assert torch.equal(_dn(c, d), plain)                                             # repeatable
    assert torch.equal(_dn(c, d, torch.full_like(d["vis"], -1)), plain)              # an all-ones mask: the unmasked bits
    zeros = _dn(c, d, torch.zeros_like(d["vis"]))
    assert float(zeros.abs().max()) == 0.0                                           # an all-zeros mask: exact zeros
    masked = _dn(c, d, d["vis"])
    assert torch.equal(_dn(c, d, d["vis"]), masked)
    bg = c["bg"].to(DEV)
    if bool(bg.any()):
        assert float(plain[bg].abs().max()) == 0.0 and float(masked[bg].abs().max()) == 0.0
    if d["shin"].numel() == 1:                                                       # stride 1 of one value: the stride-0 bits
        assert torch.equal(_dn(c, d, shin=d["shin"].expand(NP).contiguous()), plain)
        if NP > 1:
            assert torch.equal(_dn(c, d, d["vis"], shin=d["shin"].expand(NP).contiguous()), masked)


@pytest.mark.parametrize("B,NP,J,per_image,kind,mask", [(1, 300, 200, False, "s20", "random"), (2, 500, 300, True, "s20", "none"),
                                                         (9, 64, 129, False, "s1", "none")])
def test_adjointness_against_the_forward_kernel(B, NP, J, per_image, kind, mask):
    """Per pixel: lhs = d_normals[p] . dn[p] against rhs = (F_p(n + e dn) - F_p(n - e dn)) / 2e with F_p = sum_{b,c} gD D +
    gS S of the forward kernel, e = 2^-7, |dn_p| = |n_p| (so e is the relative step), differences taken in float64.

    The finite-difference error, as stated here, has two parts.  (i) What a central difference of the exact terms misses:
    truncation (the lobe's third derivative, of relative size (s e)^2 / nh^3) and the kinks of pairs whose gate lies within
    the step.  It is not modelled but computed: |lhs64 - rhs64| with both sides from the float64 references at the same
    n +- e dn.  (ii) The forward kernel's rounding on both sides of the difference: a term is an fmaf chain of J
    non-negative products, error <= J 2^-24 of its value, and the lobe's pow adds 8 (1 + s) 2^-24 (log2 and exp2 at a few
    ulp, amplified by s): 2 (J + 8 (1 + s)) 2^-24 sum |g| (|D| + |S|) / 2e.  The kernel's own bound, K unit + jump, is added.
    The tolerance has to leave something to check: on the median pixel it must be below a fifth of the derivative."""
    from reni_amd import ops
    c, d = _dev(B, NP, J, per_image, kind)
    vis = d["vis"] if mask == "random" else None
    vis64 = c["vis"] if mask == "random" else None
    g = torch.Generator().manual_seed(17)
    dn = torch.nn.functional.normalize(torch.randn(NP, 3, generator=g), dim=-1) * c["nrm"].norm(dim=1, keepdim=True)
    e = 2.0 ** -7
    got = _dn(c, d, vis)
    lhs = (got.double().cpu() * dn.double()).sum(1)
    gD, gS = c["gD"].double(), c["gS"].double()

    def F(n):
        D, S, _ = ops.envmap_shade_terms(n.to(DEV), d["pos"], c["cam"], d["L"], d["C"], d["shin"], vis=vis)
        return D.double().cpu(), S.double().cpu()

    def F64_(n):
        D, S, _ = MR.shade_terms_ref(n, c["pos"], c["cam"], c["L"], c["C"], c["shin"], vis=vis64)
        return (gD * D).sum(dim=(0, 2)) + (gS * S).sum(dim=(0, 2))

    n_plus, n_minus = c["nrm"] + e * dn, c["nrm"] - e * dn        # (float32: the very normals the kernel is given)
    (Dp, Sp), (Dm, Sm), (D0, S0) = F(n_plus), F(n_minus), F(c["nrm"])
    rhs = ((gD * (Dp - Dm)).sum(dim=(0, 2)) + (gS * (Sp - Sm)).sum(dim=(0, 2))) / (2 * e)
    ref = NR.reference(B, NP, J, per_image, kind, mask)
    lhs64 = (ref["d"] * dn.double()).sum(1)
    rhs64 = (F64_(n_plus.double()) - F64_(n_minus.double())) / (2 * e)
    s = float(c["shin"].max())
    aD, aS = (gD.abs() * D0.abs()).sum(dim=(0, 2)), (gS.abs() * S0.abs()).sum(dim=(0, 2))
    K, _ = NR.emulation_constant()
    own = (K * ref["unit"] + ref["jump"]) * dn.double().abs().sum(1)
    fd_i, fd_ii = (lhs64 - rhs64).abs(), 2 * (J + 8 * (1 + s)) * NR.EPS24 * (aD + aS) / (2 * e)
    tol = fd_i + fd_ii + own
    fg = ~c["bg"]
    rel = (tol[fg] / lhs[fg].abs().clamp_min(1e-300)).median()
    worst = float(((lhs - rhs).abs()[fg] / tol[fg]).max())
    print(f"adjointness {B}x{NP}x{J} {kind} {mask}: worst |lhs - rhs| / tol {worst:.3f}; median tol / |lhs| {float(rel):.3e} "
          f"(difference's own share {float((fd_i[fg] / tol[fg]).median()):.2f}); sums {float(lhs.sum()):.6e} {float(rhs.sum()):.6e}")
    assert float(rel) < 0.2
    assert bool(((lhs - rhs).abs() <= tol).all())
    assert float(lhs[c["bg"]].abs().max() if bool(c["bg"].any()) else 0.0) == 0.0


def test_shade_terms_normals_is_shade_terms_plus_the_normals_gradient(monkeypatch):
    from reni_amd.envmap_shader import EnvironmentMap, blinn_phong_shading_materials, shade_terms, shade_terms_normals
    B, NP, J = 3, 1000, 515
    c, d = _dev(B, NP, J, False, "per_pixel")
    for vis in (None, d["vis"]):
        outs = []
        for fn in (shade_terms, shade_terms_normals):
            Cg = d["C"].clone().requires_grad_(True)
            sg = d["shin"].clone().requires_grad_(True)
            n = d["nrm"].clone().requires_grad_(fn is shade_terms_normals)
            env = EnvironmentMap(environment_map=Cg, directions=d["L"].expand(B, -1, -1), sineweight=torch.ones(1, J, 1, device=DEV))
            D, S = fn(n, d["pos"], c["cam"], env, sg, vis=vis)
            ((D * d["gD"]).sum() + (S * d["gS"]).sum()).backward()
            outs.append((D.detach(), S.detach(), Cg.grad, sg.grad, n.grad))
        old, new = outs
        assert all(torch.equal(a, b) for a, b in zip(old[:4], new[:4])) and old[4] is None   # the forward, dC and ds keep their bits
        assert torch.equal(new[4], _dn(c, d, vis))
    # the normals' gradient is computed only when it is asked for
    from reni_amd import ops
    def env():  # (a fresh graph per backward)
        return EnvironmentMap(environment_map=d["C"].clone().requires_grad_(True), directions=d["L"].expand(B, -1, -1),
                              sineweight=torch.ones(1, J, 1, device=DEV))

    calls, real = [], ops.envmap_shade_terms_dnormals
    monkeypatch.setattr(ops, "envmap_shade_terms_dnormals", lambda *a, **k: calls.append(1) or real(*a, **k))
    shade_terms_normals(d["nrm"], d["pos"], c["cam"], env(), d["shin"])[0].sum().backward()
    assert calls == []
    shade_terms_normals(d["nrm"].clone().requires_grad_(True), d["pos"], c["cam"], env(), d["shin"])[0].sum().backward()
    assert calls == [1]
    with pytest.raises(ValueError, match="normals.*require grad"):
        blinn_phong_shading_materials(d["nrm"].clone().requires_grad_(True), d["pos"], c["cam"], env(), 0.5, 0.3, d["shin"])


# ------------------------------------------------------------------------------------------------- renderer
@functools.lru_cache(maxsize=None)
def _sphere_mesh():
    from reni_amd.mesh import Meshes
    parts = uv_sphere()
    v, f, vt, ft = (t.to(DEV) for t in parts)
    return Meshes(verts=[v], faces=[f], verts_uvs=[vt], faces_uvs=[ft]), parts


@functools.lru_cache(maxsize=None)
def _grid(W=32):
    from reni_amd.utils import get_directions, get_sineweight
    return get_directions(W).to(DEV), get_sineweight(W).to(DEV)


def _envmap(C, W=32):
    from reni_amd.envmap_shader import EnvironmentMap
    D, Sw = _grid(W)
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


def _texel_grad_ref(tex64, idx, wgt, L, upstream):
    """The float64 transpose of the lookup: d (sum upstream . fetch(pyramid(tex))) / d tex."""
    val = TR.fetch_ref(TR.pyramid_ref(tex64, L), idx, wgt)
    return torch.autograd.grad((val * upstream).sum(), tex64)[0]


@pytest.mark.parametrize("shadows", [False, True])
def test_normal_mapped_renderer_matches_float64(shadows):
    """The UV sphere at 32 x 32 under a 16 x 32 map, B = 2, an albedo texture and a normal texture of different sizes.

    The float64 chain starts from the device's own decoded m (its parity with the float64 fetch is checked first, within
    the fetch bound of DESIGN 4.4k) and the device's tangent frames (checked against the float64 frames): perturb, terms,
    composition.  Colours: the materials path's 2e-5 of the largest value, plus the albedo's fetch bound times D, plus the
    fp32 rounding of the bent normal (8 2^-24, relative) times the colour's sensitivity to it (albedo sum_j v C for the
    diffuse sum, ks norm(s) s sum_j v nh^(s-1) C for the lobe).  d normal-texture, texel by texel: the gather bound of 4.4k
    on the float64 upstream gradient, plus the upstream tolerance -- 2 sqrt(3) max(1, strength) |n_p| (K unit + jump) of
    the pixel's d_normals, pushed through perturb_normals and the decoding -- times the texel's coverage."""
    from reni_amd.mesh import unpack_visibility
    from reni_amd.textures import TexturedMaterials
    mesh, parts = _sphere_mesh()
    S, B, J = 32, 2, 512
    NP = S * S
    g = torch.Generator().manual_seed(41)
    ta = 0.2 + 0.6 * torch.rand(16, 32, 3, generator=g)
    tn = _bumps(8, 16, 0.5, 42)
    ks, shin, strength = 0.3, 40.0, 1.5
    mat = TexturedMaterials(albedo=ta, ks=ks, shininess=shin, normal=tn, normal_strength=strength, learn=("albedo", "normal")).to(DEV)
    r, R, T = _view(25.0, S, shadows, mat)
    ras = r.rasterizer
    C = torch.rand(B, J, 3, generator=g) * 4.0
    env, D, Sw = _envmap(C.to(DEV))
    wcol = torch.randn(B, S, S, 3, generator=g)
    col, geo_normals = r(meshes_world=mesh, R=R, T=T, envmap=env)
    (col * wcol.to(DEV)).sum().backward()
    assert torch.equal(r(meshes_world=mesh, R=R, T=T, envmap=env)[0], col)
    _, nrm, pos = ras.gbuffer(mesh, R, T)
    assert torch.equal(geo_normals[0].reshape(NP, 3), torch.nn.functional.normalize(nrm, dim=-1, eps=1e-6))   # the geometry's
    # tangent frames
    uv, jac, pvalid = ras.pixel_uv(mesh, R, T)
    t, b, valid = ras.pixel_tangents(mesh, R, T)
    assert ras.pixel_tangents(mesh, R, T)[0] is t
    rt, rb, rvalid = NR.tangent_frames_ref(*parts, pvalid.cpu(), nrm.cpu())
    assert torch.equal(valid.cpu(), rvalid) and int(rvalid.sum()) > 100 and int((~rvalid).sum()) > 100
    ferr = max(float((t.cpu().double() - rt).abs().max()), float((b.cpu().double() - rb).abs().max()))
    print("tangent frame: largest difference from float64", ferr)
    assert ferr <= 1e-5
    N = torch.nn.functional.normalize(nrm, dim=-1)
    assert float((t * N).sum(1).abs().max()) <= 1e-6 and float((t.norm(dim=1)[valid] - 1).abs().max()) <= 1e-6
    # the decoded normal map against the float64 fetch
    K, Kp, _, _ = TR.emulation_constants()
    Ln = TR.full_levels(8, 16)
    idx_n, wgt_n = TR.taps_ref(uv.cpu(), 8, 16, Ln, jac=jac.cpu(), valid=pvalid.cpu())
    m_dev = mat.tangent_space_normals(ras, mesh, R, T).detach()
    m_ref = 2 * TR.fetch_ref(TR.pyramid_ref(tn.to(F64), Ln), idx_n, wgt_n) - 1
    merr = float((m_dev.cpu().double() - m_ref)[rvalid].abs().max())
    mb = 2 * TR.fetch_bound(K, 8, 16, uv.cpu(), tn) + 4 * NR.EPS24
    print("decoded normal map: error / bound", merr / mb)
    unseen = pvalid < 0
    assert merr <= mb and torch.equal(m_dev[unseen], torch.tensor([0.0, 0.0, 1.0], device=DEV).expand(int(unseen.sum()), 3))
    # float64 from there
    m64 = m_dev.cpu().double().requires_grad_(True)
    n_bent = NR.perturb_normals_ref(nrm.cpu(), t.cpu(), b.cpu(), valid.cpu(), m64, strength)
    got_sn = r.shading_normals(mesh, R, T).detach().reshape(NP, 3).cpu().double()
    assert float((got_sn - torch.nn.functional.normalize(n_bent.detach(), dim=-1)).abs().max()) <= 1e-6
    assert float((got_sn - geo_normals[0].reshape(NP, 3).cpu().double())[rvalid].abs().max()) > 0.05              # bent indeed
    La = TR.full_levels(16, 32)
    idx_a, wgt_a = TR.taps_ref(uv.cpu(), 16, 32, La, jac=jac.cpu(), valid=pvalid.cpu())
    ta64 = ta.to(F64).requires_grad_(True)
    a64 = TR.fetch_ref(TR.pyramid_ref(ta64, La), idx_a, wgt_a)
    vis = unpack_visibility(ras.visibility(mesh, R, T, D), J).cpu() if shadows else None
    Cw = C.to(F64) * Sw.cpu().to(F64)
    Dr, Sr, _ = MR.shade_terms_ref(n_bent, pos.cpu(), r.camera_center, D.cpu()[None], Cw, shin, vis=vis)
    col_ref = MR.compose_ref(Dr, Sr, a64, ks, shin)
    norm_s = float(MR.specular_norm_ref(torch.tensor(shin, dtype=F64)))
    vv = torch.ones(1, NP, J, dtype=F64) if vis is None else vis.to(F64)
    lit = (~(nrm.cpu() == 0).all(-1)).to(F64)[None, :, None]
    Dabs = torch.einsum("bjk,bpj->bpk", Cw, vv.expand(B, -1, -1)) * lit
    Spow = MR.shade_terms_ref(n_bent.detach(), pos.cpu(), r.camera_center, D.cpu()[None], Cw, shin - 1.0, vis=vis)[1]
    sens = (TR.fetch_bound(K, 16, 32, uv.cpu(), ta) * Dr.abs()
            + 8 * NR.EPS24 * (a64.abs() * Dabs + ks * norm_s * shin * Spow)).detach()
    cmax = float(col_ref.detach().abs().max())
    cerr = (col.detach().reshape(B, NP, 3).cpu().double() - col_ref.detach()).abs()
    print("colour err/bound", float((cerr / (2e-5 * cmax + sens)).max()))
    assert cmax > 0 and bool((cerr <= 2e-5 * cmax + sens).all())
    # gradients
    gw = wcol.reshape(B, NP, 3).to(F64)
    loss_ref = (col_ref * gw).sum()
    um, ua = torch.autograd.grad(loss_ref, (m64, a64))
    assert float(um[~rvalid].abs().max()) == 0.0 and float(um.abs().max()) > 0
    Kd, _ = NR.emulation_constant()
    gD_up = gw * a64.detach()
    gS_up = gw * (ks * norm_s)
    unit, jump = NR.dnormals_bound(n_bent.detach().float(), pos.cpu(), r.camera_center, D.cpu()[None], Cw.float(), gD_up, gS_up, shin, vis=vis)
    utol_n = 2 * math.sqrt(3.0) * max(1.0, strength) * nrm.cpu().double().norm(dim=1) * (Kd * unit + jump) * rvalid.to(F64)
    for name, got, tex, up, idx, wgt, (H0, W0), L, utol in (
            ("normal", mat.normal.grad, tn, 2 * um, idx_n, wgt_n, (8, 16), Ln, utol_n),
            ("albedo", mat.albedo.grad, ta, ua, idx_a, wgt_a, (16, 32), La, torch.full((NP,), 2e-5 * float(ua.abs().max()), dtype=F64))):
        t64 = tex.to(F64).requires_grad_(True)
        want = _texel_grad_ref(t64, idx, wgt, L, up.detach())
        cover = _texel_grad_ref(t64, idx, wgt, L, utol[:, None].expand(NP, 3))[:, :, 0]
        cc = {"H0": H0, "W0": W0, "L": L, "uv": uv.cpu(), "g": up.detach(), "wrap": "clamp"}
        bound = TR.level0_grad_bound(Kp, cc, idx, wgt) + cover
        err = (got.cpu().double() - want).abs().max(2).values
        nz = bound > 0
        print(name, "texture grad err/bound", float((err[nz] / bound[nz]).max()), "largest gradient", float(want.abs().max()))
        assert float(want.abs().max()) > 0 and bool((err <= bound).all()), name


def test_flat_normal_texture_two_views_and_a_short_fit():
    """A flat normal texture renders the bits of the same material without one; two views share one normal texture and
    the shared gradient is bit-equal to the sum of the single-view ones; 15 Adam steps on albedo and normal texture
    together, towards a bumpy target, lower the loss."""
    from reni_amd.textures import TexturedMaterials
    mesh, _ = _sphere_mesh()
    S, B, J = 32, 2, 512
    g = torch.Generator().manual_seed(51)
    C = (torch.rand(B, J, 3, generator=g) * 4.0).to(DEV)
    env, _, _ = _envmap(C)
    ta = 0.2 + 0.6 * torch.rand(16, 32, 3, generator=g)
    flat = torch.tensor([0.5, 0.5, 1.0]).expand(8, 16, 3)
    for shadows in (False, True):
        a = _view(25.0, S, shadows, TexturedMaterials(albedo=ta, ks=0.3, shininess=40.0).to(DEV))
        b = _view(25.0, S, shadows, TexturedMaterials(albedo=ta, ks=0.3, shininess=40.0, normal=flat, normal_strength=2.0,
                                                     learn=("normal",)).to(DEV))
        ca, cb = (r(meshes_world=mesh, R=R, T=T, envmap=env)[0] for r, R, T in (a, b))
        assert torch.equal(ca, cb)
        assert torch.equal(b[0].shading_normals(mesh, b[1], b[2]), a[0].shading_normals(mesh, a[1], a[2]))
    # two views, one normal texture
    gt = TexturedMaterials(albedo=ta, ks=0.3, shininess=40.0, normal=_bumps(16, 32, 0.6, 52)).to(DEV)
    mat = TexturedMaterials(albedo=torch.full((16, 32, 3), 0.5), ks=0.3, shininess=40.0, normal=torch.tensor([0.5, 0.5, 1.0]).expand(16, 32, 3),
                            learn=("albedo", "normal")).to(DEV)
    views = [_view(az, S, False, mat) for az in (0.0, 180.0)]
    with torch.no_grad():
        targets = [_view(az, S, False, gt)[0](meshes_world=mesh, R=R, T=T, envmap=env)[0] for az, (_, R, T) in zip((0.0, 180.0), views)]

    def loss_of(i):
        r, R, T = views[i]
        return ((r(meshes_world=mesh, R=R, T=T, envmap=env)[0] - targets[i]) ** 2).mean()

    single = []
    for i in (0, 1):
        mat.normal.grad = mat.albedo.grad = None
        loss_of(i).backward()
        single.append((mat.normal.grad.clone(), mat.albedo.grad.clone()))
    mat.normal.grad = mat.albedo.grad = None
    (loss_of(0) + loss_of(1)).backward()
    assert float(single[0][0].abs().max()) > 0 and float(single[1][0].abs().max()) > 0
    assert torch.equal(mat.normal.grad, single[0][0] + single[1][0]) and torch.equal(mat.albedo.grad, single[0][1] + single[1][1])
    opt = torch.optim.Adam([mat.albedo, mat.normal], lr=0.03)
    losses = []
    for _ in range(15):
        opt.zero_grad()
        loss = loss_of(0) + loss_of(1)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("two-view albedo + normal fit: loss", losses[0], "->", losses[-1])
    assert torch.isfinite(mat.normal).all() and torch.isfinite(mat.albedo).all() and losses[-1] < losses[0]


def test_old_paths_keep_their_bits_around_a_normal_mapped_render():
    from reni_amd.envmap_shader import EnvironmentMap, SpatialMaterials, blinn_phong_shading_materials, shade_terms
    from reni_amd.mesh import build_hip_renderer
    from reni_amd.textures import TexturedMaterials
    mesh, _ = _sphere_mesh()
    S = 32
    g = torch.Generator().manual_seed(61)
    C = (torch.rand(2, 512, 3, generator=g) * 4.0).to(DEV)
    env, _, _ = _envmap(C)
    sp = SpatialMaterials(torch.rand(S * S, 3, generator=g), 0.3, 40.0)
    tex = TexturedMaterials(albedo=torch.rand(8, 8, 3, generator=g), ks=torch.rand(4, 4, generator=g)).to(DEV)
    c, d = _dev(3, 1000, 515, False, "s20")
    envc = EnvironmentMap(environment_map=d["C"], directions=d["L"].expand(3, -1, -1), sineweight=torch.ones(1, 515, 1, device=DEV))

    def old():
        outs = list(shade_terms(d["nrm"], d["pos"], c["cam"], envc, d["shin"], vis=d["vis"]))
        outs.append(blinn_phong_shading_materials(d["nrm"], d["pos"], c["cam"], envc, 0.5, 0.3, d["shin"]))
        for shadows in (False, True):
            r, R, T, teapot = build_hip_renderer(TEAPOT, 0, S, 0.5, "cuda", shadows=shadows)
            outs.append(r(meshes_world=teapot, R=R, T=T, envmap=env)[0])
            r, R, T, teapot = build_hip_renderer(TEAPOT, 0, S, None, "cuda", shadows=shadows, materials=sp)
            outs.append(r(meshes_world=teapot, R=R, T=T, envmap=env)[0])
            r, R, T = _view(40.0, S, shadows, tex)
            outs.append(r(meshes_world=mesh, R=R, T=T, envmap=env)[0])
        return outs

    before = old()
    mat = TexturedMaterials(albedo=torch.rand(8, 8, 3, generator=g), normal=_bumps(8, 8, 0.5, 62), learn=("normal",)).to(DEV)
    r, R, T = _view(40.0, S, True, mat)
    r(meshes_world=mesh, R=R, T=T, envmap=env)[0].sum().backward()
    assert mat.normal.grad is not None and float(mat.normal.grad.abs().max()) > 0
    for a, b in zip(before, old()):
        assert torch.equal(a, b)
