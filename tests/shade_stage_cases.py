"""The shapes at which a split of the env-map shader's kernels (reni_tu_shade.hip) walks two or more LDS stages, and a pure-Python
model of the host's plan (``ShadePlan`` / ``n_splits`` there) that says so.

A kernel owns one axis (a thread per pixel forward and in the pixel gradients, a thread per texel backward) and walks the
other in S splits of ``per_split`` elements, 128 (SH_TILE) per stage:

    tiles     = ceil(n_oth / 128)
    S         = max(1, min(ceil(2048 / ceil(n_own / 256)), tiles, 64))
    per_split = ceil(tiles / S) * 128

A split walks a second stage only when tiles > S: the walked axis is longer than 8192 (the cap of 64 bites) or the owned one
is so long that 2048 / wg_x falls below the tiles.  The older parity cases (seven shapes, walked axis <= 1030) have tiles <= S.
tests/test_shade_stages_cpu.py pins what each shape below reaches, so that a change of the constants cannot quietly turn them
back into single-stage cases; tests/test_gpu_shade_stages.py runs the kernels at them.
"""
import functools
import types

import numpy as np
import torch

from tests import normal_map_ref as NR
from tests import visibility_ref as VR

SH_TILE, SHADE_BC = NR.SH_TILE, NR.SHADE_BC

# name -> (B, NP, J, per-image directions); each is the smallest shape with its property
SHAPES = {
    "F1": (5, 40, 8325, False),     # forward: 66 tiles over 64 splits, 33 live (the last 128 + 5), 31 empty; JW = 261; nb = 4 and 1
    "F2": (2, 300, 8420, False),    # as F1 with JW = 264: the 16-byte mask load at w0 = 260; a second workgroup of 44 pixels
    "F3": (2, 33, 16500, True),     # three stages per split, 43 live and 21 empty; BC = 1; per-image masks, JW = 516
    "B1": (5, 8325, 40, False),     # backward: F1's plan on the pixel axis; one workgroup of 40 texels, JW = 2
    "B2": (2, 8325, 260, True),     # backward, BC = 1; a second workgroup of 4 texels with mask word 8 of 9
    "B3": (1, 16500, 129, False),   # backward, three stages; nb = 1 < BC; JW = 5
    "G": (1, 32600, 2100, False),   # S from the workgroup branch: forward wg_x = 128, S = 16 < 17 tiles
}
REFERENCED = ("F1", "F2", "F3", "B1", "B2", "B3")   # a full float64 reference is affordable (G: a sample of pixels)
SCALAR_KIND_AT = ("F1", "B1")                       # one scalar material kind beside "per_pixel"
MASKS = ("none", "random")


def plan(forward, B, NP, J, per_image):
    """The host's plan of one call: forward (and the pixel gradients) owns the pixels and walks the texels, backward the
    reverse.  -> S, per_split, stages (of every live split, ascending), last_count (elements of the last live split's last
    stage), live, empty (splits with t_begin >= n_oth), JW, n_chunks, wg_x."""
    n_own, n_oth = (NP, J) if forward else (J, NP)
    S = NR.n_splits(n_own, n_oth)
    tiles = (n_oth + SH_TILE - 1) // SH_TILE
    per_split = ((tiles + S - 1) // S) * SH_TILE
    live = min(S, (n_oth + per_split - 1) // per_split)
    counts = [min(n_oth, (q + 1) * per_split) - q * per_split for q in range(live)]
    stages = tuple((c + SH_TILE - 1) // SH_TILE for c in counts)
    step = 1 if per_image else SHADE_BC
    return types.SimpleNamespace(n_own=n_own, n_oth=n_oth, S=S, per_split=per_split, stages=stages,
                                 last_count=counts[-1] - (stages[-1] - 1) * SH_TILE, live=live, empty=S - live,
                                 JW=(J + 31) // 32, n_chunks=(B + step - 1) // step, wg_x=(n_own + 255) // 256)


def workspace_bytes(B, NP, J):
    """What the six *_workspace_bytes entry points answer, from ``plan`` (the sizes do not depend on per-image directions: the
    pixel gradients reserve a slot per image)."""
    f, g = plan(True, B, NP, J, False), plan(False, B, NP, J, False)
    partial = lambda p, nt: p.S * nt * B * p.n_own * 3 * 4 if p.S > 1 else 0
    return {"scalar": max(f.S * B * NP * 3 * 4, g.S * B * J * 3 * 4) + 256,
            "terms": max(partial(f, 2), partial(g, 1)) + 256,
            "terms_ds": max(partial(f, 3), partial(g, 1)) + 256,
            "terms_dnormals": B * f.S * NP * 3 * 4 + 256,
            "ggx": max(partial(f, 3), partial(g, 1)) + 256,
            "ggx_dpixel": B * f.S * NP * 4 * 4 + 256}


def last_stage_start(forward, B, NP, J, per_image):
    """First element of the walked axis's last stage (a multiple of 128)."""
    p = plan(forward, B, NP, J, per_image)
    return (p.live - 1) * p.per_split + (p.stages[-1] - 1) * SH_TILE


# ------------------------------------------------------------------------------------------------------------- cases
def terms_kinds(name):
    return ("per_pixel", "s20") if name in SCALAR_KIND_AT else ("per_pixel",)


def ggx_kinds(name):
    return ("per_pixel", "r02") if name in SCALAR_KIND_AT else ("per_pixel",)


@functools.lru_cache(maxsize=None)
def terms_problem(B, NP, J, per_image, kind):
    """The CPU half of tests/test_gpu_shade_materials.py::_case (its generator, seeds and order of draws): what the float32
    evaluation of the terms is given where there is no GPU."""
    from tests import test_gpu_shade_materials as TM
    nrm, pos, cam, L, C = TM._problem(B, NP, J, seed=100 + B + NP, per_image_dirs=per_image)
    g = torch.Generator().manual_seed(7 * NP + J)
    shin = {"s500": torch.tensor(500.0), "s20": torch.tensor(20.0)}.get(kind)
    if shin is None:
        shin = torch.rand(NP, generator=g) * 495.0 + 5.0
    c = types.SimpleNamespace(B=B, NP=NP, J=J, nrm=nrm, pos=pos, cam=cam, L=L, C=C, shin=shin, per_image=per_image,
                              rtol=2e-4 if float(shin.max()) > 100 else 2e-5, bg=(nrm == 0).all(-1))
    c.albedo = torch.rand(NP, 3, generator=g)
    c.ks = torch.rand(NP, generator=g) * 0.8 + 0.1
    c.gD, c.gS, c.w = (torch.randn(B, NP, 3, generator=g) for _ in range(3))
    c.vis = torch.rand(L.shape[0], NP, J, generator=g) < 0.6
    return c


def terms_eval(c, vis, dtype):
    """D, S, T and dC = d (<gD, D> + <gS, S>) / dC of one terms problem by the definition and its autograd in ``dtype``."""
    from tests import shade_materials_ref as MR
    C = c.C.to(dtype).clone().requires_grad_(True)
    D, S, T = MR.shade_terms_ref(c.nrm, c.pos, c.cam, c.L, C, c.shin.to(dtype), vis=vis, dtype=dtype)
    (dC,) = torch.autograd.grad((D * c.gD.to(dtype)).sum() + (S * c.gS.to(dtype)).sum(), C)
    return {"D": D.detach(), "S": S.detach(), "T": T.detach(), "dC": dC}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """One problem per shape for the exact properties and the structural checks, which need no reference: the shared
    generator's geometry and colours, a per-pixel shininess and alpha, three upstream gradients, and a 60 % mask drawn as
    numpy booleans and packed (``mask`` bool [NB, NP, J], ``words`` int32 [NB, NP, JW]).  CPU tensors."""
    B, NP, J, per_image = SHAPES[name]
    nrm, pos, cam, L, C = NR.problem(B, NP, J, seed=300 + B + NP, per_image_dirs=per_image)
    g = torch.Generator().manual_seed(11 * NP + J)
    c = types.SimpleNamespace(name=name, B=B, NP=NP, J=J, per_image=per_image, nrm=nrm, pos=pos, cam=cam, L=L, C=C,
                              bg=(nrm == 0).all(-1), JW=(J + 31) // 32, NB=L.shape[0])
    c.shin = torch.rand(NP, generator=g) * 495.0 + 5.0
    rough = torch.rand(NP, generator=g) * 0.9 + 0.1
    c.alpha = rough * rough
    c.gD, c.gS0, c.gS1 = (torch.randn(B, NP, 3, generator=g) for _ in range(3))
    rng = np.random.default_rng([B, NP, J, int(per_image)])
    c.mask = rng.integers(0, 5, size=(c.NB, NP, J), dtype=np.uint8) < 3
    c.words = torch.from_numpy(VR.pack_bits(c.mask))
    return c
