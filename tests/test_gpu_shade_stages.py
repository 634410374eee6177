"""GPU tests of the env-map shader's kernels (reni_tu_shade.hip) at the shapes of tests/shade_stage_cases.py, where a split walks
two or more LDS stages: the stage loop's second iteration, a mask word index w0 that differs from the split's first, the mask
rows of a second stage's pixels, a partial stage after a full one, empty splits, and S from the workgroup branch.  The older
parity files run the same kernels at seven shapes whose splits all walk exactly one stage.

Against float64, with the bounds the quantities already have (tests/test_shade_stages_cpu.py holds the float32 evaluation of
each definition against them at these shapes first): the terms' 2e-4 / 2e-5 of the largest reference value,
``normal_map_ref.emulation_constant()`` units of ``dnormals_bound``, ``microfacet_ref.factors()`` with its floor, the scalar
shader's 2e-4.  The case builders, references and comparisons are the older files' own; they take any shape.  Beside them:
exact properties of every entry point at every shape, and a structural check that needs no large reference -- with only one
stage's texels (or pixels' gradients) nonzero, the full call has to agree with the call on that stage's elements alone.

A new kernel family on the ``shade_walk`` skeleton is to be added to ``_everything`` below and given its float64 test here;
profiles/shade_stage_mutants.md records which mutants of the stage loop these tests catch that the older files do not.
"""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import reni_oracle as O
from tests import microfacet_ref as GR
from tests import normal_map_ref as NR
from tests import shade_materials_ref as MR
from tests import shade_stage_cases as SC
from tests import test_gpu_microfacet as GM
from tests import test_gpu_normal_map as NM
from tests import test_gpu_shade_materials as TM
from tests import test_gpu_visibility as VIS
from tests import visibility_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
RTOL = 2e-4          # the terms' and the scalar shader's bound with a shininess above 100
SCALAR = (500.0, 0.5, 0.5)   # shininess, kd, ks of the scalar shader's calls

TERMS_CASES = [(n, k) for n in SC.REFERENCED for k in SC.terms_kinds(n)]
GGX_CASES = [(n, k) for n in SC.REFERENCED for k in SC.ggx_kinds(n)]


# ----------------------------------------------------------------------------------- float64 parity at F1 .. B3
@pytest.mark.parametrize("name,kind", TERMS_CASES)
@pytest.mark.parametrize("mask", SC.MASKS)
def test_terms_match_float64(name, kind, mask):
    c = TM._case(*SC.SHAPES[name], kind)
    p = SC.terms_problem(*SC.SHAPES[name], kind)   # the problem the CPU file held the bound against is this one
    assert torch.equal(p.C, c.C) and torch.equal(p.shin, c.shin) and torch.equal(p.gS, c.gS) and torch.equal(p.vis, c.vis)
    r = c.ref[mask]
    vis = None if mask == "none" else c.dev.vis
    D, S, T = TM._fwd(c, vis)
    for label, got, ref in (("D", D, r.D), ("S", S, r.S), ("T", T, r.T)):
        TM._close(label, got, ref, c.rtol)
    TM._close("dC", TM._bwd(c, vis), r.dC, c.rtol)
    D2, S2, none = TM._fwd(c, vis, need_ds=False)   # the instances without T: the other two terms keep their bits
    assert none is None and torch.equal(D2, D) and torch.equal(S2, S)
    bg = c.bg.to(DEV)
    for t in (D, S, T):
        assert float(t[:, bg].abs().max()) == 0.0


@pytest.mark.parametrize("name,kind", TERMS_CASES)
@pytest.mark.parametrize("mask", SC.MASKS)
def test_terms_dnormals_match_float64(name, kind, mask):
    c, d = NM._dev(*SC.SHAPES[name], kind)
    K, _ = NR.emulation_constant()
    got = NM._dn(c, d, d["vis"] if mask == "random" else None)
    assert torch.isfinite(got).all()
    ratio, ref = NR.error_ratio(got.cpu(), c, mask)
    print(f"d_normals {name} {kind} {mask}: worst error / unit {ratio:.3f} (K {K:.3f}); largest gradient {float(ref['d'].abs().max()):.3e}")
    assert float(ref["d"].abs().max()) > 0
    assert ratio <= K
    assert float(got[c["bg"].to(DEV)].abs().max()) == 0.0


@pytest.mark.parametrize("name,kind", GGX_CASES)
@pytest.mark.parametrize("mask", SC.MASKS)
def test_ggx_terms_and_gradients_match_float64(name, kind, mask):
    shape = SC.SHAPES[name]
    c, d = GM._dev(*shape, kind)
    ref = GR.reference(*shape, kind, mask)
    vis = None if mask == "none" else d.vis
    D, S0, S1 = GM._fwd(c, d, vis)
    dC = GM._bwd(c, d, vis)
    da, dn = GM._dpx(c, d, vis)
    da_only, none = GM._dpx(c, d, vis, need_dn=False)   # both WANT_DN instances, d alpha bit-equal between them
    assert none is None and torch.equal(da_only, da)
    for label, got in (("D", D), ("S0", S0), ("S1", S1), ("dC", dC), ("dalpha", da), ("dn", dn)):
        GM._held(label, got, ref[label])
    bg = c.bg.to(DEV)
    assert all(float(t[:, bg].abs().max()) == 0.0 for t in (D, S0, S1)) and all(float(t[bg].abs().max()) == 0.0 for t in (da, dn))


@functools.lru_cache(maxsize=None)
def _scalar_reference(name, mask):
    """colours and d colours' adjoint of the scalar shader in float64, as tests/test_gpu_visibility.py::_shader_case has them."""
    c = SC.inputs(name)
    Cd = c.C.double().requires_grad_(True)
    L = c.L.expand(c.B, -1, -1)
    if mask == "none":
        ref = O.blinn_phong_gbuffer(c.nrm, c.pos, c.cam, L, Cd, *SCALAR)
    else:
        ref = VIS._masked_ref(c.nrm, c.pos, c.cam, L, Cd, *SCALAR, torch.from_numpy(c.mask))
    (ref_g,) = torch.autograd.grad((ref * c.gD.double()).sum(), Cd)
    return ref.detach(), ref_g


@pytest.mark.parametrize("name", SC.REFERENCED)
@pytest.mark.parametrize("mask", SC.MASKS)
def test_scalar_shader_matches_float64(name, mask):
    from reni_amd import ops
    c, P = SC.inputs(name), _dev(name)
    ref, ref_g = _scalar_reference(name, mask)
    vis = None if mask == "none" else P.words
    col = ops.envmap_shade(P.nrm, P.pos, P.cam, P.L, P.C, *SCALAR, vis=vis)
    gC = ops.envmap_shade_backward(P.nrm, P.pos, P.cam, P.L, P.gD, *SCALAR, vis=vis)
    TM._close("colours", col, ref, RTOL)
    TM._close("d colours", gC, ref_g, RTOL)
    assert float(col[:, c.bg.to(DEV)].abs().max()) == 0.0


# ----------------------------------------------------------------------------------- every entry point, any shape
@functools.lru_cache(maxsize=None)
def _dev(name):
    c = SC.inputs(name)
    P = types.SimpleNamespace(cam=c.cam, **{k: getattr(c, k).to(DEV) for k in ("nrm", "pos", "C", "shin", "alpha", "gD", "gS0", "gS1", "words")})
    P.L = (c.L if c.per_image else c.L[0]).to(DEV)
    return P


def _sub(P, pix=slice(None), tex=slice(None)):
    """The problem on a slice of the pixels and a slice of the texels (the mask is the caller's)."""
    return types.SimpleNamespace(cam=P.cam, nrm=P.nrm[pix].contiguous(), pos=P.pos[pix].contiguous(), shin=P.shin[pix].contiguous(),
                                 alpha=P.alpha[pix].contiguous(), L=P.L[..., tex, :].contiguous(), C=P.C[:, tex].contiguous(),
                                 gD=P.gD[:, pix].contiguous(), gS0=P.gS0[:, pix].contiguous(), gS1=P.gS1[:, pix].contiguous())


def _forward(P, vis):
    from reni_amd import ops
    geo = (P.nrm, P.pos, P.cam, P.L, P.C)
    out = {"shade": ops.envmap_shade(*geo, *SCALAR, vis=vis)}
    out["terms.D"], out["terms.S"], out["terms.T"] = ops.envmap_shade_terms(*geo, P.shin, vis=vis, need_ds=True)
    out["ggx.D"], out["ggx.S0"], out["ggx.S1"] = ops.envmap_shade_ggx(*geo, P.alpha, vis=vis)
    return out


def _backward(P, vis):
    from reni_amd import ops
    geo = (P.nrm, P.pos, P.cam, P.L)
    return {"shade.dC": ops.envmap_shade_backward(*geo, P.gD, *SCALAR, vis=vis),
            "terms.dC": ops.envmap_shade_terms_backward(*geo, P.gD, P.gS0, P.shin, vis=vis),
            "ggx.dC": ops.envmap_shade_ggx_backward(*geo, P.gD, P.gS0, P.gS1, P.alpha, vis=vis)}


def _pixel_gradients(P, vis):
    from reni_amd import ops
    geo = (P.nrm, P.pos, P.cam, P.L, P.C)
    out = {"terms.dn": ops.envmap_shade_terms_dnormals(*geo, P.gD, P.gS0, P.shin, vis=vis)}
    out["ggx.dalpha"], out["ggx.dn"] = ops.envmap_shade_ggx_dpixel(*geo, P.gD, P.gS0, P.gS1, P.alpha, vis=vis, need_dn=True)
    out["ggx.dalpha only"], _ = ops.envmap_shade_ggx_dpixel(*geo, P.gD, P.gS0, P.gS1, P.alpha, vis=vis, need_dn=False)
    return out


def _everything(P, vis):
    """Every entry point of the unit and every instance switch (T wanted or not, d normals wanted or not)."""
    from reni_amd import ops
    out = {**_forward(P, vis), **_backward(P, vis), **_pixel_gradients(P, vis)}
    out["terms.D without T"], out["terms.S without T"], _ = ops.envmap_shade_terms(P.nrm, P.pos, P.cam, P.L, P.C, P.shin, vis=vis, need_ds=False)
    return out


PER_PIXEL = ("terms.dn", "ggx.dalpha", "ggx.dn", "ggx.dalpha only")                        # [NP, ...]
PER_IMAGE_PIXEL = ("shade", "terms.D", "terms.S", "terms.T", "ggx.D", "ggx.S0", "ggx.S1",  # [B, NP, 3]
                   "terms.D without T", "terms.S without T")


@pytest.mark.parametrize("name", list(SC.SHAPES))
def test_exact_properties_of_every_entry_point(name):
    c, P = SC.inputs(name), _dev(name)
    plain = _everything(P, None)
    assert len(plain) == 16
    ones = torch.from_numpy(VR.pack_bits(np.ones((c.NB, c.NP, c.J), bool))).to(DEV)
    masked = _everything(P, P.words)
    zeroed = _everything(P, torch.zeros_like(P.words))
    bg = c.bg.to(DEV)
    assert int(bg.sum()) > 0
    for k, want in plain.items():
        assert torch.isfinite(want).all() and torch.isfinite(masked[k]).all(), k       # an empty split, a 0 * inf in a store
        assert float(want.abs().max()) > 0 and float(masked[k].abs().max()) > 0, k
        assert float(zeroed[k].abs().max()) == 0.0, k                                   # an all-zero mask: exact zeros
        assert not torch.equal(masked[k], want), k                                      # (the random mask does something)
    for k, got in _everything(P, ones).items():                                         # all-ones: the unmasked bits
        assert torch.equal(got, plain[k]), k
    for k, got in _everything(P, torch.full_like(P.words, -1)).items():                 # the bits past J set as well
        assert torch.equal(got, plain[k]), k
    for first, vis in ((plain, None), (masked, P.words)):
        for k, got in _everything(P, vis).items():                                      # two calls give equal bits
            assert torch.equal(got, first[k]), k
        assert torch.equal(first["terms.D without T"], first["terms.D"]) and torch.equal(first["terms.S without T"], first["terms.S"])
        assert torch.equal(first["ggx.dalpha only"], first["ggx.dalpha"])
        assert torch.equal(first["ggx.D"], first["terms.D"])                            # one diffuse sum, bit for bit
        for k in PER_IMAGE_PIXEL:                                                       # background pixels: exactly 0
            assert float(first[k][:, bg].abs().max()) == 0.0, k
        for k in PER_PIXEL:
            assert float(first[k][bg].abs().max()) == 0.0, k


def _agree(label, full, sub):
    for k, want in sub.items():
        scale = float(want.abs().max())
        err = float((full[k].double() - want.double()).abs().max())
        print(f"{label} {k}: largest difference {err:.3e}, {err / scale if scale > 0 else 0.0:.3e} of the largest value (bound {RTOL:g})")
        assert scale > 0 and torch.isfinite(full[k]).all() and err <= RTOL * scale, (label, k, err / scale)


@pytest.mark.parametrize("name", list(SC.SHAPES))
@pytest.mark.parametrize("mask", SC.MASKS)
def test_a_stage_reads_its_own_elements(name, mask):
    """With the colours of all texels but one stage's zero, the forward sums of the full call are the sums of the call on
    that stage's texels alone (first stage: j < 128; last stage: j >= the last stage's start); with the upstream gradients of
    all pixels but one stage's zero, the same holds for dC on the pixel axis.  The zero terms still go through the partial
    sums, so the bits may differ: the terms' 2e-4 of the largest value is asked (the nonzero terms are the same few hundred
    products in both calls; what a wrong stage, mask word or mask row adds or drops is of the order of the value itself)."""
    c, P = SC.inputs(name), _dev(name)
    words = P.words if mask == "random" else None
    checked = 0
    for which, start in (("first", 0), ("last", SC.last_stage_start(True, c.B, c.NP, c.J, c.per_image))):
        stop = min(c.J, start + SC.SH_TILE)
        if (start, stop) == (0, c.J):
            continue                                      # a walked axis of one stage: nothing to tell apart
        tex = slice(start, stop)
        full = types.SimpleNamespace(**vars(P))
        full.C = torch.zeros_like(P.C)
        full.C[:, tex] = P.C[:, tex]
        vis_sub = None if words is None else words[:, :, start >> 5:(stop + 31) >> 5].contiguous()
        _agree(f"{name} {which} texel stage {start}:{stop}", _forward(full, words), _forward(_sub(P, tex=tex), vis_sub))
        checked += 1
    for which, start in (("first", 0), ("last", SC.last_stage_start(False, c.B, c.NP, c.J, c.per_image))):
        stop = min(c.NP, start + SC.SH_TILE)
        if (start, stop) == (0, c.NP):
            continue
        pix = slice(start, stop)
        full = types.SimpleNamespace(**vars(P))
        for k in ("gD", "gS0", "gS1"):
            g = torch.zeros_like(getattr(P, k))
            g[:, pix] = getattr(P, k)[:, pix]
            setattr(full, k, g)
        vis_sub = None if words is None else words[:, pix].contiguous()
        _agree(f"{name} {which} pixel stage {start}:{stop}", _backward(full, words), _backward(_sub(P, pix=pix), vis_sub))
        checked += 1
    assert checked >= 2


# ----------------------------------------------------------------------------------- G: S from the workgroup branch
@functools.lru_cache(maxsize=None)
def _g_sample(mask):
    """float64 references of G on the pixels sel = 0, 97, 194, ...: the forward sums and the per-pixel gradients are
    independent per pixel."""
    c = SC.inputs("G")
    sel = torch.arange(0, c.NP, 97)
    vis = torch.from_numpy(c.mask[:, sel.numpy()]) if mask == "random" else None
    g = torch.Generator().manual_seed(97)
    s = types.SimpleNamespace(B=c.B, NP=len(sel), J=c.J, per_image=False, nrm=c.nrm[sel], pos=c.pos[sel], cam=c.cam, L=c.L, C=c.C,
                              shin=c.shin[sel], alpha=c.alpha[sel], rough=c.alpha[sel].sqrt(), gD=c.gD[:, sel], gS0=c.gS0[:, sel],
                              gS1=c.gS1[:, sel], gS=c.gS0[:, sel], bg=c.bg[sel], sel=sel)
    s.base_color, s.metallic, s.w = torch.rand(s.NP, 3, generator=g), torch.rand(s.NP, generator=g), torch.randn(c.B, s.NP, 3, generator=g)
    s.terms = MR.shade_terms_ref(s.nrm, s.pos, s.cam, s.L, s.C, s.shin, vis=vis)
    if mask == "none":
        s.colours = O.blinn_phong_gbuffer(s.nrm, s.pos, s.cam, s.L.expand(c.B, -1, -1), s.C, *SCALAR).double()
    else:
        s.colours = VIS._masked_ref(s.nrm, s.pos, s.cam, s.L.expand(c.B, -1, -1), s.C.double(), *SCALAR, vis)
    args = (s.nrm, s.pos, s.cam, s.L, s.C, s.gD, s.gS, s.shin)
    s.dn, (s.unit, s.jump) = NR.dnormals_ref(*args, vis=vis), NR.dnormals_bound(*args, vis=vis)
    s.ggx = GR.entries(s, vis)
    return s


@pytest.mark.parametrize("mask", SC.MASKS)
def test_g_sampled_pixels_match_float64_and_dC_is_the_adjoint(mask):
    c, P = SC.inputs("G"), _dev("G")
    s = _g_sample(mask)
    sel = s.sel.to(DEV)
    vis = P.words if mask == "random" else None
    fwd, bwd, px = _forward(P, vis), _backward(P, vis), _pixel_gradients(P, vis)
    TM._close("colours", fwd["shade"][:, sel], s.colours, RTOL)
    for k, ref in zip(("terms.D", "terms.S", "terms.T"), s.terms):
        TM._close(k, fwd[k][:, sel], ref, RTOL)
    # d normals of the terms, per pixel: K units of dnormals_bound plus the gates' jump (normal_map_ref.error_ratio's rule)
    K, _ = NR.emulation_constant()
    over = ((px["terms.dn"][sel].cpu().double() - s.dn).abs().max(dim=1).values - s.jump).clamp_min(0.0)
    ratio = GR._worst(over, s.unit)
    print(f"G {mask} d normals of the terms: worst error / unit {ratio:.3f} (K {K:.3f})")
    assert float(s.dn.abs().max()) > 0 and ratio <= K
    for k, got in (("D", fwd["ggx.D"][:, sel]), ("S0", fwd["ggx.S0"][:, sel]), ("S1", fwd["ggx.S1"][:, sel]),
                   ("dalpha", px["ggx.dalpha"][sel]), ("dn", px["ggx.dn"][sel])):
        GM._held(k, got, s.ggx[k])
    # the three dC through the adjoint identity: the forward sums are linear in C and dC is their adjoint
    dbl = lambda t: t.double()
    pairs = {"shade.dC": [(P.gD, fwd["shade"])], "terms.dC": [(P.gD, fwd["terms.D"]), (P.gS0, fwd["terms.S"])],
             "ggx.dC": [(P.gD, fwd["ggx.D"]), (P.gS0, fwd["ggx.S0"]), (P.gS1, fwd["ggx.S1"])]}
    for k, terms in pairs.items():
        lhs = sum(float((dbl(g) * dbl(t)).sum()) for g, t in terms)
        size = sum(float((dbl(g).abs() * dbl(t).abs()).sum()) for g, t in terms)
        rhs = float((dbl(bwd[k]) * dbl(P.C)).sum())
        print(f"G {mask} {k}: <g, terms> {lhs:.8e}, <dC, C> {rhs:.8e}, |difference| / absolute sum {abs(lhs - rhs) / size:.3e} (bound 1e-5)")
        assert torch.isfinite(bwd[k]).all() and size > 0 and abs(lhs - rhs) <= 1e-5 * size, k
