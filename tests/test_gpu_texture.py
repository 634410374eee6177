"""GPU tests of the UV-texture path against the float64 restatement (tests/texture_ref.py) on the same fp32 inputs.

Tolerances.  The fetch is continuous in uv and lambda across every floor, clamp, wrap and level border, so every
pixel is compared: |out - ref| <= K 2^-24 (1 + max(H0, W0) max(1, |uv|max)) (max tex - min tex).  A texel's gradient is held
against K' 2^-24 (1 + ...) sum |g| over the float64 reference's taps of that texel, carried to level 0 through the box
transpose of the bounds (texture_ref.grad_bound / level0_grad_bound); a texel that no reference tap names, at any level above
it either, has bound 0 and its gradient must be exactly 0.  K and K' are four times the worst ratio the fp32 numpy emulation
reaches over these very cases (texture_ref.emulation_constants; the margin is for FMA contraction and the device's log2)."""
import functools
import os

import pytest
import torch

from tests import shade_materials_ref as MR
from tests import texture_ref as TR
from tests.util import uv_sphere

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEAPOT = os.path.join(ROOT, "tests", "golden", "teapot.obj")
F64 = torch.float64
CASES = TR.lookup_cases()


def _id(c):
    return (f"{c['H0']}x{c['W0']}-L{c['L']}-P{c['P']}-C{c['C']}-{c['wrap']}" + ("-ac" if c["align"] else "") +
            (f"-b{c['lod_bias']:g}" if c["lod_bias"] else "") + ("" if c["jac"] is not None else "-nojac"))


@functools.lru_cache(maxsize=None)
def _reference(i):
    return TR.case_reference(CASES[i])


def _device_taps(c):
    from reni_amd import textures
    return textures.make_taps(c["uv"].to(DEV), (c["H0"], c["W0"]), c["L"], jac=None if c["jac"] is None else c["jac"].to(DEV),
                              pix_valid=c["valid"].to(DEV), wrap=c["wrap"], align_corners=c["align"], lod_bias=c["lod_bias"])


def _run(c, taps):
    from reni_amd import textures
    tex = c["tex"].to(DEV).requires_grad_(True)
    out = textures.sample(tex, taps)
    out.backward(c["g"].to(DEV))
    return out.detach(), tex.grad


@pytest.mark.parametrize("i", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_fetch_and_texture_gradient_match_float64(i):
    c = CASES[i]
    K, Kp, _, _ = TR.emulation_constants()
    ref_out, ref_g, ref_idx, ref_w = _reference(i)
    taps = _device_taps(c)
    E = TR.level_offsets(c["H0"], c["W0"], c["L"])[-1]
    assert taps.elements == E and taps.levels == c["L"]
    assert int(taps.index.min()) >= 0 and int(taps.index.max()) < E
    ok = torch.isfinite(c["uv"]).all(1) & (c["valid"] >= 0)
    w = taps.weight.cpu()
    assert float((w[ok].double().sum(1) - 1).abs().max() if bool(ok.any()) else 0.0) <= 16 * TR.EPS24
    out, grad = _run(c, taps)
    if bool((~ok).any()):  # background, missing-UV, NaN / Inf pixels: weights, index and fetch exactly 0
        assert float(w[~ok].abs().max()) == 0.0 and int(taps.index.cpu()[~ok].abs().max()) == 0
        assert float(out.cpu()[~ok].abs().max()) == 0.0
    bound = TR.fetch_bound(K, c["H0"], c["W0"], c["uv"], c["tex"])
    err = float((out.cpu().double() - ref_out).abs().max())
    gb = TR.level0_grad_bound(Kp, c, ref_idx, ref_w)
    gerr = (grad.cpu().double() - ref_g).abs().max(2).values
    m = gb > 0
    ratio_g = float((gerr[m] / gb[m]).max()) if bool(m.any()) else 0.0
    print(f"fetch err/bound {err / bound if bound > 0 else 0.0:.4f} grad err/bound {ratio_g:.4f}")
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    assert err <= bound, (err, bound)
    assert float(gerr[~m].max() if bool((~m).any()) else 0.0) == 0.0   # texels with no taps (invalid pixels add exactly 0)
    assert ratio_g <= 1.0, ratio_g
    # every forward and backward call repeated once: bit-equal (taps and table included)
    taps2 = _device_taps(c)
    for a, b in zip(taps[:4], taps2[:4]):
        assert torch.equal(a, b)
    out2, grad2 = _run(c, taps2)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)


@pytest.mark.parametrize("P", [64, 65, 128, 129, 192, 193, 4097])
@pytest.mark.parametrize("C", [1, 3, 8])
def test_every_pixel_on_one_texel(P, C):
    """A 1 x 1 texture: every pixel's one tap of weight 1 belongs to texel 0 (the seven of weight 0 are sorted out of the
    table's ranges).  A range of 128 is the longest one lane walks, 129 the first the wave shares; 192 and 193 sit on and one
    past a 64-entry chunk border.  The chunked and the plain form agree with
    float64 within the sum's own rounding (the number of additions on a lane's path x 2^-24 sum |g|) and repeat bit for bit."""
    from reni_amd import ops, textures
    g = torch.Generator().manual_seed(P * 10 + C)
    uv = torch.rand(P, 2, generator=g)
    gout = torch.randn(P, C, generator=g)
    taps = textures.make_taps(uv.to(DEV), (1, 1))
    assert taps.offsets.tolist() == [0, P] and float((taps.weight.sum(1) - 1).abs().max()) <= 4 * TR.EPS24
    want = gout.double().sum(0)
    for plain in (False, True):
        got = ops.texture_fetch_backward(gout.to(DEV), taps.weight, (taps.order, taps.offsets), 1, plain=plain)
        again = ops.texture_fetch_backward(gout.to(DEV), taps.weight, (taps.order, taps.offsets), 1, plain=plain)
        assert torch.equal(got, again) and got.shape == (1, C)
        # every weight is exactly 1, so the only roundings are the additions': P of them on one lane, or ceil(P / 64) per lane
        # and six butterfly levels in the chunked form of a range longer than 128
        adds = P if plain or P <= 128 else -(-P // 64) + 6
        tol = adds * TR.EPS24 * gout.double().abs().sum(0)
        assert bool(((got.cpu().double()[0] - want).abs() <= tol).all()), (got, want)
    tex = torch.rand(1, 1, C, generator=g)
    out = textures.sample(tex.to(DEV), taps)
    assert float((out.cpu() - tex.reshape(1, C)).abs().max()) <= 4 * TR.EPS24


def test_long_and_short_ranges_in_one_wave_and_a_constant_pyramid():
    """4 x 4 texture, every pixel at level 2 (the 1 x 1 top, a long range) or at level 0 (short ranges), in one table: the
    wave that owns the top texel also owns short ones.  And the pyramid of a constant is that constant at every level."""
    from reni_amd import ops, textures
    P = 600
    g = torch.Generator().manual_seed(1)
    uv = torch.rand(P, 2, generator=g)
    jac = torch.zeros(P, 4)
    jac[::2, 0] = 1.0   # rho = 4 texels: lambda = 2 = L - 1
    jac[::2, 3] = 1.0
    c = {"H0": 4, "W0": 4, "L": 3, "P": P, "C": 3, "wrap": "clamp", "align": False, "lod_bias": 0.0, "uv": uv, "jac": jac,
         "valid": torch.zeros(P, dtype=torch.int64), "tex": torch.rand(4, 4, 3, generator=g), "g": torch.randn(P, 3, generator=g)}
    ref_out, ref_g, ref_idx, ref_w = TR.case_reference(c)
    taps = _device_taps(c)
    assert int(taps.offsets[21] - taps.offsets[20]) > 128     # the top texel's range is long
    out, grad = _run(c, taps)
    K, Kp, _, _ = TR.emulation_constants()
    assert float((out.cpu().double() - ref_out).abs().max()) <= TR.fetch_bound(K, 4, 4, uv, c["tex"])
    # the top texel's sum of n weighted terms: ceil(n / 64) additions per lane and six butterfly levels, folded down by 1/16
    n = int(taps.offsets[21] - taps.offsets[20])
    top = c["g"][::2].abs().max(1).values.double().sum()
    gb = TR.level0_grad_bound(Kp, c, ref_idx, ref_w) + (-(-n // 64) + 6) * TR.EPS24 * top / 16
    assert bool(((grad.cpu().double() - ref_g).abs().max(2).values <= gb).all())
    buf = torch.full((21, 5), 0.3, device=DEV)
    ops.texture_pyramid(buf, 3, 4, 4)
    assert float((buf - 0.3).abs().max()) <= 2 * TR.EPS24
    for H, W in ((1, 8), (8, 1), (16, 4)):
        L, E, _ = ops.texture_levels(H, W)
        tex = torch.rand(H, W, 2, generator=g)
        buf = torch.zeros(E, 2, device=DEV)
        buf[: H * W] = tex.reshape(-1, 2).to(DEV)
        ops.texture_pyramid(buf, L, H, W)
        assert float((buf.cpu().double() - TR.pyramid_ref(tex.double(), L)).abs().max()) <= 4 * L * TR.EPS24


def test_malformed_table_and_indices_stay_inside_guard_bands():
    """Order entries outside [0, 8 P), ranges that run backwards or past the table, fetch indices outside [0, E): skipped or
    clipped, never an address.  The outputs are carved out of larger buffers whose guard bands must stay intact."""
    from reni_amd import _lib, ops
    lib = _lib.load()
    P, E, C, G = 300, 40, 3, 4096
    g = torch.Generator().manual_seed(2)
    gout = torch.randn(P, C, generator=g).to(DEV)
    wgt = torch.rand(P, 8, generator=g).to(DEV)
    order = torch.randint(0, 8 * P, (8 * P,), generator=g)
    order[::7] = -5
    order[3::11] = 8 * P
    order[5::13] = 1 << 40
    offsets = torch.sort(torch.randint(0, 8 * P + 1, (E + 1,), generator=g)).values
    offsets[0], offsets[3], offsets[4], offsets[10], offsets[E] = -(1 << 33), 9 * P, 2, 1 << 45, 1 << 50
    order_d, offsets_d = order.to(DEV), offsets.to(DEV)   # (held: a temporary's memory would be reused by the next one)
    big = torch.full((2 * G + E * C,), 7.5, device=DEV)
    out = big[G:G + E * C]
    stream = torch.cuda.current_stream().cuda_stream
    for plain in (0, 1):
        rc = lib.reni_texture_fetch_backward(P, E, C, gout.data_ptr(), wgt.data_ptr(), order_d.data_ptr(),
                                             offsets_d.data_ptr(), plain, out.data_ptr(), stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((big[:G] == 7.5).all()) and bool((big[G + E * C:] == 7.5).all()) and torch.isfinite(out).all()
        # what a well-behaved reader of the same table sums
        want = torch.zeros(E, C, dtype=F64)
        for e in range(E):
            k0 = min(max(int(offsets[e]), 0), 8 * P)
            k1 = min(max(int(offsets[e + 1]), k0), 8 * P)
            t = order[k0:k1]
            t = t[(t >= 0) & (t < 8 * P)]
            want[e] = (wgt.cpu().double().reshape(-1)[t][:, None] * gout.cpu().double()[t >> 3]).sum(0)
        tol = 8 * P * TR.EPS24 * gout.abs().sum().item()
        assert float((out.reshape(E, C).cpu().double() - want).abs().max()) <= tol
    # the forward: indices beyond the pyramid are clamped
    tex = torch.rand(E, C, generator=g).to(DEV)
    idx = torch.randint(-100, E + 100, (P, 8), generator=g, dtype=torch.int32)
    idx[0, 0], idx[1, 1] = -(1 << 31), (1 << 31) - 1
    bigo = torch.full((2 * G + P * C,), 7.5, device=DEV)
    idx_d = idx.to(DEV)
    got = ops.texture_fetch(tex, idx_d, wgt)
    want = (wgt.cpu().double()[:, :, None] * tex.cpu().double()[idx.long().clamp(0, E - 1)]).sum(1)
    assert float((got.cpu().double() - want).abs().max()) <= 16 * TR.EPS24 * 8
    o = bigo[G:G + P * C]
    assert lib.reni_texture_fetch(P, E, C, tex.data_ptr(), idx_d.data_ptr(), wgt.data_ptr(), o.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert bool((bigo[:G] == 7.5).all()) and bool((bigo[G + P * C:] == 7.5).all()) and torch.equal(o.reshape(P, C), got)


# ------------------------------------------------------------------------------------------------- meshes
def _quad():
    verts = torch.tensor([[-0.9, -0.7, 0.1], [0.8, -0.6, -0.2], [0.7, 0.9, 0.0], [-0.8, 0.6, 0.3]])
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]])
    vt = torch.tensor([[0.1, 0.0], [1.2, 0.1], [0.9, 1.0], [-0.1, 0.8], [0.5, 0.5]])
    ft = torch.tensor([[0, 1, 2], [0, 2, 3]])
    return verts, faces, vt, ft


def _mesh(parts):
    from reni_amd.mesh import Meshes
    v, f, vt, ft = (t.to(DEV) for t in parts)
    return Meshes(verts=[v], faces=[f], verts_uvs=[vt], faces_uvs=[ft])


@pytest.mark.parametrize("S", [1, 15, 17, 33])
@pytest.mark.parametrize("which", ["sphere", "quad", "sphere_missing"])
def test_pixel_uv_and_jacobian_match_float64(S, which):
    from reni_amd.mesh import FoVPerspectiveCameras, MeshRasterizer, RasterizationSettings, look_at_view_transform
    parts = _quad() if which == "quad" else uv_sphere()
    if which == "sphere_missing":   # every third face loses a texture coordinate, one keeps an index past Tn
        ft = parts[3].clone()
        ft[::3, 1] = -1
        ft[1, 2] = parts[2].shape[0]
        parts = parts[:3] + (ft,)
    assert parts[2].shape[0] != parts[0].shape[0]
    mesh = _mesh(parts)
    R, T = look_at_view_transform(2.7, 20.0, 35.0, device=DEV)
    cams = FoVPerspectiveCameras(device=DEV)
    ras = MeshRasterizer(cameras=cams, raster_settings=RasterizationSettings(image_size=S))
    uv, jac, valid = ras.pixel_uv(mesh, R, T)
    assert ras.pixel_uv(mesh, R, T)[0] is uv                      # cached beside the G-buffer
    frags = ras.gbuffer(mesh, R, T)[0]
    from reni_amd import ops
    for _ in range(2):                                            # the kernel itself, run again twice: bit-equal
        again = ops.mesh_pixel_uv(*(t.to(DEV) for t in parts), R, T, S, frags.pix_to_face, frags.bary_coords, cams.tan_half_fov())
        assert all(torch.equal(a, b) for a, b in zip(again, (uv, jac, valid)))
    p2f, bary = frags.pix_to_face.cpu().reshape(-1), frags.bary_coords.cpu().reshape(-1, 3)
    ruv, rjac, rvalid = TR.pixel_uv_ref(*parts, R.cpu(), T.cpu(), cams.tan_half_fov(), S, p2f, bary)
    assert int((p2f >= 0).sum()) > 0 and torch.equal(valid.cpu() >= 0, rvalid) and torch.equal(valid.cpu()[rvalid], p2f[rvalid])
    if which == "sphere_missing":
        assert int(((p2f >= 0) & ~rvalid).sum()) > 0 or S == 1
    inv = ~rvalid
    if bool(inv.any()):
        assert float(uv.cpu()[inv].abs().max()) == 0.0 and float(jac.cpu()[inv].abs().max()) == 0.0
    # uv: a three-term fp32 dot, 3 roundings on sum |b t|
    t_abs = parts[2].abs().max().double()
    tol_uv = 4 * TR.EPS24 * bary.abs().double().sum(1) * t_abs
    assert bool(((uv.cpu().double() - ruv).abs().max(1).values <= tol_uv + 1e-300).all())
    jb = TR.jac_bound(*parts, R.cpu(), T.cpu(), cams.tan_half_fov(), S, p2f)
    jerr = (jac.cpu().double() - rjac).abs().max(1).values
    print("jac err/bound", float((jerr[rvalid] / jb[rvalid]).max()) if bool(rvalid.any()) else 0.0)
    assert bool((jerr[rvalid] <= jb[rvalid]).all())
    # the taps of the cache: one record per argument set, kept
    a = ras.texture_taps(mesh, R, T, size=(8, 8))
    assert ras.texture_taps(mesh, R, T, size=(8, 8)) is a and ras.texture_taps(mesh, R, T, size=(8, 8), lod_bias=1.0) is not a
    assert ras.texture_taps(mesh, R, T, size=(8, 8)) is a and a.levels == 4
    assert float(a.weight.cpu()[inv].abs().max() if bool(inv.any()) else 0.0) == 0.0


# ------------------------------------------------------------------------------------------------- renderer
@functools.lru_cache(maxsize=None)
def _grid(W=32):
    from reni_amd.utils import get_directions, get_sineweight
    return get_directions(W).to(DEV), get_sineweight(W).to(DEV)


def _envmap(C, W=32):
    from reni_amd.envmap_shader import EnvironmentMap
    D, Sw = _grid(W)
    return EnvironmentMap(environment_map=C, directions=D.expand(C.shape[0], -1, -1), sineweight=Sw), D[0], Sw


def _view(azim, S, shadows, materials):
    """A renderer with its own rasteriser, camera and true camera centre, looking at the UV sphere from `azim` degrees."""
    from reni_amd.mesh import FoVPerspectiveCameras, HipMeshRenderer, MeshRasterizer, RasterizationSettings, look_at_view_transform
    R, T = look_at_view_transform(2.7, 10.0, azim, device=DEV)
    ras = MeshRasterizer(cameras=FoVPerspectiveCameras(device=DEV), raster_settings=RasterizationSettings(image_size=S))
    r = HipMeshRenderer(ras, materials=materials, shader_cameras=FoVPerspectiveCameras(R=R, T=T, device=DEV), shadows=shadows)
    return r, R, T


def _material_refs(mat64, ras, R, T, lod_bias=0.0):
    """float64 per-pixel (albedo, ks, shininess) of the restatement from float64 textures (which may require grad)."""
    # the device's own fp32 uv and jac are the lookup's inputs (their parity is the test above): the restatement starts there
    duv, djac, dvalid = ras.pixel_uv(_MESH[0], R, T)
    out = []
    for tex in mat64:
        t = tex if tex.dim() == 3 else tex.unsqueeze(-1)
        L = TR.full_levels(*t.shape[:2])
        idx, wgt = TR.taps_ref(duv.cpu(), t.shape[0], t.shape[1], L, jac=djac.cpu(), valid=dvalid.cpu(), lod_bias=lod_bias)
        v = TR.fetch_ref(TR.pyramid_ref(t, L), idx, wgt)
        out.append((v if tex.dim() == 3 else v[:, 0], (idx, wgt), duv.cpu()))
    return out


_MESH = [None, None]


def _sphere_mesh():
    if _MESH[0] is None:
        _MESH[1] = uv_sphere()
        _MESH[0] = _mesh(_MESH[1])
    return _MESH


@pytest.mark.parametrize("shadows", [False, True])
def test_textured_renderer_matches_the_restatement_and_its_autograd(shadows):
    """HipMeshRenderer(materials=TexturedMaterials) on the UV sphere at 32 x 32 under a 16 x 32 map, B = 2, with an albedo,
    a ks and a shininess texture of three different sizes: colours against compose_ref fed with the restatement's per-pixel
    values, d texture of all three against its autograd.  Colours and upstream gradients carry the materials path's own
    tolerance (2e-5 of the largest reference value, s <= 100: tests/test_gpu_shade_materials.py); the fetch adds its bound
    times the colour's sensitivity to the material; a texel's gradient adds the upstream tolerance times its coverage."""
    from reni_amd.mesh import unpack_visibility
    from reni_amd.textures import TexturedMaterials
    mesh, parts = _sphere_mesh()
    S, B, J = 32, 2, 512
    NP = S * S
    g = torch.Generator().manual_seed(11)
    ta = 0.2 + 0.6 * torch.rand(16, 32, 3, generator=g)
    tk = 0.1 + 0.4 * torch.rand(8, 8, generator=g)
    ts = 10.0 + 60.0 * torch.rand(4, 16, generator=g)
    mat = TexturedMaterials(albedo=ta, ks=tk, shininess=ts, learn=("albedo", "ks", "shininess")).to(DEV)
    r, R, T = _view(25.0, S, shadows, mat)
    C = (torch.rand(B, J, 3, generator=g) * 4.0)
    env, D, Sw = _envmap(C.to(DEV))
    wcol = torch.randn(B, S, S, 3, generator=g)
    col, _ = r(meshes_world=mesh, R=R, T=T, envmap=env)
    (col * wcol.to(DEV)).sum().backward()
    col2, _ = r(meshes_world=mesh, R=R, T=T, envmap=env)
    assert torch.equal(col, col2)
    # float64
    t64 = [t.to(F64).requires_grad_(True) for t in (ta, tk, ts)]
    (a64, ia, uv), (k64, ik, _), (s64raw, is_, _) = _material_refs(t64, r.rasterizer, R, T)
    s64 = s64raw.clamp(1.0, 2000.0)
    _, nrm, pos = r.rasterizer.gbuffer(mesh, R, T)
    vis = unpack_visibility(r.rasterizer.visibility(mesh, R, T, D), J).cpu() if shadows else None
    Dr, Sr, Tr = MR.shade_terms_ref(nrm.cpu(), pos.cpu(), r.camera_center, D.cpu()[None], C.to(F64) * Sw.cpu().to(F64), s64, vis=vis)
    col_ref = MR.compose_ref(Dr, Sr, a64, k64, s64)
    assert float(col_ref.detach().abs().max()) > 0 and int((nrm.abs().sum(1) > 0).sum()) > 100
    K, Kp, _, _ = TR.emulation_constants()
    da = TR.fetch_bound(K, 16, 32, uv, ta)
    dk = TR.fetch_bound(K, 8, 8, uv, tk)
    ds = TR.fetch_bound(K, 4, 16, uv, ts)
    n, dn = MR.specular_norm_ref(s64.detach()), MR.specular_norm_ds_ref(s64.detach())
    kk = k64.detach()
    sens = (da * Dr.abs() + dk * n[:, None] * Sr.abs() + ds * kk[:, None] * (dn.abs()[:, None] * Sr.abs() + n[:, None] * Tr.abs())).detach()
    rtol = 2e-5
    cmax = float(col_ref.detach().abs().max())
    cerr = (col.reshape(B, NP, 3).cpu().double() - col_ref.detach()).abs()
    print("colour err/bound", float((cerr / (rtol * cmax + sens)).detach().max()))
    assert bool((cerr <= rtol * cmax + sens).all())
    # gradients: upstream d loss / d (per-pixel material) from the reference, then texel by texel
    loss_ref = (col_ref * wcol.reshape(B, NP, 3).to(F64)).sum()
    ga, gk, gs = torch.autograd.grad(loss_ref, t64, retain_graph=True)
    ua, uk, us = torch.autograd.grad(loss_ref, (a64, k64, s64raw))
    gw = wcol.reshape(B, NP, 3).to(F64)
    up_tol = (rtol * float(ua.abs().max()), rtol * float(uk.abs().max()),
              rtol * float(MR.shininess_grad_bound(gw, kk, s64.detach(), Sr.detach(), Tr.detach()).max()))
    for name, got, want, up, val, tex, idx, (H0, W0), utol in (
            ("albedo", mat.albedo.grad, ga, ua, a64, t64[0], ia, (16, 32), up_tol[0]),
            ("ks", mat.ks.grad, gk, uk[:, None], k64, t64[1], ik, (8, 8), up_tol[1]),
            ("shininess", mat.shininess.grad, gs, us[:, None], s64raw, t64[2], is_, (4, 16), up_tol[2])):
        L = TR.full_levels(H0, W0)
        c = {"H0": H0, "W0": W0, "L": L, "uv": uv, "g": up.detach(), "wrap": "clamp"}
        # a texel's coverage: the sum of the weights that reach it (through the pyramid), the transpose applied to ones
        cover = torch.autograd.grad(val.sum(), tex, retain_graph=True)[0].reshape(H0, W0, -1)[:, :, 0]
        bound = TR.level0_grad_bound(Kp, c, *idx) + utol * cover
        err = (got.cpu().double().reshape(H0, W0, -1) - want.reshape(H0, W0, -1)).abs().max(2).values
        m = bound > 0
        print(name, "grad err/bound", float((err[m] / bound[m]).max()))
        assert float(want.abs().max()) > 0 and bool((err <= bound).all()), name


def test_two_views_share_one_texture_gradient_and_a_short_fit_lowers_the_loss():
    """Two renderers at azimuth 0 and 180, each with its own rasteriser, camera and camera centre, share one
    TexturedMaterials: the gradient of the summed loss is bit-equal to the sum of the two single-view gradients, texels seen
    only from the second view get a gradient, and 15 Adam steps on the albedo texture over both views lower the loss."""
    from reni_amd.textures import TexturedMaterials
    mesh, _ = _sphere_mesh()
    S, B, J = 32, 1, 512
    g = torch.Generator().manual_seed(21)
    yy, xx = torch.meshgrid(torch.arange(32), torch.arange(64), indexing="ij")
    checker = (((yy // 4) + (xx // 4)) % 2).float()[:, :, None]
    gt = TexturedMaterials(albedo=0.2 + 0.6 * checker * torch.tensor([1.0, 0.6, 0.3]), ks=0.2, shininess=40.0).to(DEV)
    C = (torch.rand(B, J, 3, generator=g) * 4.0).to(DEV)
    env, _, _ = _envmap(C)
    mat = TexturedMaterials(albedo=torch.full((32, 64, 3), 0.5), ks=0.2, shininess=40.0, learn=("albedo",)).to(DEV)
    views = [_view(az, S, False, mat) for az in (0.0, 180.0)]
    assert views[0][0].materials is views[1][0].materials and not torch.equal(views[0][0].camera_center, views[1][0].camera_center)
    with torch.no_grad():
        targets = [_view(az, S, False, gt)[0](meshes_world=mesh, R=R, T=T, envmap=env)[0] for az, (_, R, T) in zip((0.0, 180.0), views)]

    def loss_of(i):
        r, R, T = views[i]
        return ((r(meshes_world=mesh, R=R, T=T, envmap=env)[0] - targets[i]) ** 2).mean()

    single = []
    for i in (0, 1):
        mat.albedo.grad = None
        loss_of(i).backward()
        single.append(mat.albedo.grad.clone())
    mat.albedo.grad = None
    (loss_of(0) + loss_of(1)).backward()
    assert torch.equal(mat.albedo.grad, single[0] + single[1])
    # the level-0 texels directly under a view's pixels (one-level taps of the same G-buffer; the pyramid's coarse levels also
    # carry a little gradient from the polar pixels of either view to every texel, so "seen" is not "gradient != 0")
    seen = []
    for r, R, T in views:
        t1 = r.rasterizer.texture_taps(mesh, R, T, size=(32, 64), levels=1)
        hit = torch.zeros(32 * 64, dtype=torch.bool, device=DEV)
        hit[t1.index[t1.weight > 0].long()] = True
        seen.append(hit.reshape(32, 64))
    only1, only0 = seen[1] & ~seen[0], seen[0] & ~seen[1]
    assert int(only1.sum()) > 50 and int(only0.sum()) > 50 and int((~seen[0] & ~seen[1]).sum()) > 0
    assert bool((mat.albedo.grad.abs().sum(2)[only1] > 0).all()) and bool((single[1].abs().sum(2)[only1] > 0).all())
    # ... and there the second view's share is the larger one (the first reaches them through coarse levels only)
    assert float(single[1].abs().sum(2)[only1].mean()) > 10 * float(single[0].abs().sum(2)[only1].mean())
    opt = torch.optim.Adam([mat.albedo], lr=0.05)
    losses = []
    for _ in range(15):
        opt.zero_grad()
        loss = loss_of(0) + loss_of(1)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("two-view loss", losses[0], "->", losses[-1])
    assert torch.isfinite(mat.albedo).all() and losses[-1] < losses[0]


def test_old_paths_keep_their_bits_around_textured_objects():
    """Scalar and SpatialMaterials renders of the teapot before and after textured objects were built and rendered: bit-equal."""
    from reni_amd.envmap_shader import SpatialMaterials
    from reni_amd.mesh import build_hip_renderer
    from reni_amd.textures import TexturedMaterials
    S = 32
    g = torch.Generator().manual_seed(31)
    C = (torch.rand(2, 512, 3, generator=g) * 4.0).to(DEV)
    env, _, _ = _envmap(C)
    sp = SpatialMaterials(torch.rand(S * S, 3, generator=g), 0.3, 40.0)

    def old():
        outs = []
        for shadows in (False, True):
            r, R, T, mesh = build_hip_renderer(TEAPOT, 0, S, 0.5, "cuda", shadows=shadows)
            outs.append(r(meshes_world=mesh, R=R, T=T, envmap=env)[0])
            r, R, T, mesh = build_hip_renderer(TEAPOT, 0, S, None, "cuda", shadows=shadows, materials=sp)
            outs.append(r(meshes_world=mesh, R=R, T=T, envmap=env)[0])
        return outs

    before = old()
    mesh, _ = _sphere_mesh()
    mat = TexturedMaterials(albedo=torch.rand(8, 8, 3, generator=g), ks=torch.rand(4, 4, generator=g), learn=("albedo",)).to(DEV)
    r, R, T = _view(40.0, S, True, mat)
    r(meshes_world=mesh, R=R, T=T, envmap=env)[0].sum().backward()
    assert mat.albedo.grad is not None and float(mat.albedo.grad.abs().max()) > 0
    for a, b in zip(before, old()):
        assert torch.equal(a, b)
    # a mesh without UVs cannot take the textured path, and says so
    r2, R2, T2, teapot = build_hip_renderer(TEAPOT, 0, S, 0.5, "cuda")
    with pytest.raises(ValueError, match="no texture coordinates"):
        build_hip_renderer(TEAPOT, 0, S, None, "cuda", materials=mat)
