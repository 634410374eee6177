"""CPU tests of the env-map shader's multi-stage cases (tests/shade_stage_cases.py): the model of the host's plan says of
every shape what it is there to reach, the six *_workspace_bytes entry points agree with the model, and the existing
tolerances of the three kernel families are checked against the float64 references at the new shapes before a GPU is: the
definition evaluated in float32 on the CPU has to lie inside them.

Measured (float32 evaluation's worst error over the bound in use, F1 - B3, masks "none" and "random"): terms D 0.015, S 0.10,
T 0.14, dC 0.13 of 2e-4 / 2e-5 of the largest reference value; d normals of the terms 2.81 units of ``dnormals_bound`` (the old
cases' worst is 2.46, K = 9.83); microfacet D 0.034, S0 0.20, S1 0.16, dC 0.18, d alpha 0.15, d normals 0.09 of
``microfacet_ref.bound``.  No quantity needed a constant of its own: sums of 8 000 to 16 000 terms stay inside the bounds that
were derived at 1 030."""
import pytest
import torch

from tests import microfacet_ref as GR
from tests import normal_map_ref as NR
from tests import shade_stage_cases as SC

# forward / backward: (S, per_split, stages of the first live split, stages of the last, last stage's count, live, empty)
EXPECTED = {
    "F1": {"JW": 261, "n_chunks": 2, True: (64, 256, 2, 2, 5, 33, 31), False: (1, 128, 1, 1, 40, 1, 0)},
    "F2": {"JW": 264, "n_chunks": 1, True: (64, 256, 2, 2, 100, 33, 31), False: (3, 128, 1, 1, 44, 3, 0)},
    "F3": {"JW": 516, "n_chunks": 2, True: (64, 384, 3, 3, 116, 43, 21), False: (1, 128, 1, 1, 33, 1, 0)},
    "B1": {"JW": 2, "n_chunks": 2, True: (1, 128, 1, 1, 40, 1, 0), False: (64, 256, 2, 2, 5, 33, 31)},
    "B2": {"JW": 9, "n_chunks": 2, True: (3, 128, 1, 1, 4, 3, 0), False: (64, 256, 2, 2, 5, 33, 31)},
    "B3": {"JW": 5, "n_chunks": 1, True: (2, 128, 1, 1, 1, 2, 0), False: (64, 384, 3, 3, 116, 43, 21)},
    "G": {"JW": 66, "n_chunks": 1, True: (16, 256, 2, 1, 52, 9, 7), False: (64, 512, 4, 3, 88, 64, 0)},
}


@pytest.mark.parametrize("name", list(SC.SHAPES))
@pytest.mark.parametrize("forward", [True, False])
def test_plan_reaches_what_the_shape_is_there_for(name, forward):
    B, NP, J, per_image = SC.SHAPES[name]
    p = SC.plan(forward, B, NP, J, per_image)
    print(f"{name} {'forward' if forward else 'backward'}: S {p.S}, per_split {p.per_split}, stages {p.stages[0]}..{p.stages[-1]}, "
          f"last stage {p.last_count}, live {p.live}, empty {p.empty}, JW {p.JW} (JW % 4 = {p.JW % 4}), chunks {p.n_chunks}")
    want = EXPECTED[name]
    assert (p.S, p.per_split, p.stages[0], p.stages[-1], p.last_count, p.live, p.empty) == want[forward]
    assert p.JW == want["JW"] and p.n_chunks == want["n_chunks"]
    assert all(s == p.per_split // SC.SH_TILE for s in p.stages[:-1])         # every live split but the last is full
    assert p.live + p.empty == p.S and p.live == len(p.stages) and 1 <= p.last_count <= SC.SH_TILE
    # the model's own consistency: the splits cover the walked axis exactly once
    assert (p.live - 1) * p.per_split < p.n_oth <= p.live * p.per_split
    assert sum(p.stages) == (p.n_oth + SC.SH_TILE - 1) // SC.SH_TILE


def test_every_property_of_the_table_is_reached_in_its_direction():
    multi = lambda name, fwd: SC.plan(fwd, *SC.SHAPES[name]).stages[0] >= 2
    assert all(multi(n, True) for n in ("F1", "F2", "F3", "G")) and all(multi(n, False) for n in ("B1", "B2", "B3", "G"))
    # a partial stage after a full one; empty splits (they need per_split >= 256)
    for name, fwd in (("F1", True), ("F2", True), ("F3", True), ("B1", False), ("B2", False), ("B3", False)):
        p = SC.plan(fwd, *SC.SHAPES[name])
        assert p.stages[-1] >= 2 and p.last_count < SC.SH_TILE and p.empty > 0 and p.per_split >= 256
        assert p.S == 64 and p.wg_x <= 2                                      # the cap of 64 decides
    # guarded mask loads (JW % 4 != 0) and the 16-byte ones (JW % 4 == 0), both with a second stage's w0
    assert SC.plan(True, *SC.SHAPES["F1"]).JW % 4 == 1 and SC.plan(True, *SC.SHAPES["F2"]).JW % 4 == 0
    assert SC.plan(True, *SC.SHAPES["F3"]).JW % 4 == 0 and SC.SHAPES["F3"][3]
    assert SC.last_stage_start(True, *SC.SHAPES["F2"]) >> 5 == 260 and SC.last_stage_start(True, *SC.SHAPES["F1"]) >> 5 == 260
    # chunks of nb = 4 and nb = 1, nb = 1 < BC, BC = 1
    assert SC.SHAPES["F1"][0] % SC.SHADE_BC == 1 and SC.SHAPES["B1"][0] % SC.SHADE_BC == 1 and SC.SHAPES["B3"][0] == 1
    assert SC.SHAPES["B2"][3] and SC.SHAPES["F3"][3]
    # backward workgroups: 40 live texels; a second one with 4 live texels whose first mask word is 8 of 9
    assert SC.plan(False, *SC.SHAPES["B1"]).n_own == 40 and SC.plan(False, *SC.SHAPES["B2"]).n_own == 256 + 4
    assert SC.plan(False, *SC.SHAPES["B2"]).JW == 9 and SC.plan(True, *SC.SHAPES["F2"]).n_own == 256 + 44
    # G: S comes from 2048 / wg_x, below the tiles, with per_split > 128
    g = SC.plan(True, *SC.SHAPES["G"])
    assert g.wg_x == 128 and g.S == 2048 // g.wg_x == 16 < (g.n_oth + 127) // 128 == 17 and g.per_split == 256
    # none of the older cases walks a second stage: that is the gap these shapes close
    for (B, NP, J, per_image) in NR.SHAPES:
        assert SC.plan(True, B, NP, J, per_image).stages[0] == 1 and SC.plan(False, B, NP, J, per_image).stages[0] == 1


@pytest.mark.parametrize("name", list(SC.SHAPES))
def test_workspace_sizes_are_what_the_plan_implies(name):
    from reni_amd import _lib
    lib = _lib.load()
    B, NP, J, _ = SC.SHAPES[name]
    want = SC.workspace_bytes(B, NP, J)
    got = {"scalar": lib.reni_envmap_shade_workspace_bytes(B, NP, J),
           "terms": lib.reni_envmap_shade_terms_workspace_bytes(B, NP, J, 0),
           "terms_ds": lib.reni_envmap_shade_terms_workspace_bytes(B, NP, J, _lib.SHADE_TERMS_DS),
           "terms_dnormals": lib.reni_envmap_shade_terms_dnormals_workspace_bytes(B, NP, J),
           "ggx": lib.reni_envmap_shade_ggx_workspace_bytes(B, NP, J),
           "ggx_dpixel": lib.reni_envmap_shade_ggx_dpixel_workspace_bytes(B, NP, J)}
    print(name, got)
    assert {k: int(v) for k, v in got.items()} == want
    assert SC.workspace_bytes(2, 1000, 515)["terms_ds"] == 5 * 3 * 2 * 1000 * 3 * 4 + 256   # (the model at an older case's figure)


REFERENCED = [(n, k) for n in SC.REFERENCED for k in SC.terms_kinds(n)]
REFERENCED_GGX = [(n, k) for n in SC.REFERENCED for k in SC.ggx_kinds(n)]


@pytest.mark.parametrize("name,kind", REFERENCED)
@pytest.mark.parametrize("mask", SC.MASKS)
def test_float32_terms_lie_inside_the_terms_tolerance(name, kind, mask):
    """D, S, T and dC of ``shade_terms_ref`` in float32 against float64: 2e-4 (a shininess above 100) or 2e-5 of the largest
    reference value, the terms' existing bound."""
    c = SC.terms_problem(*SC.SHAPES[name], kind)
    vis = c.vis if mask == "random" else None
    ref, got = SC.terms_eval(c, vis, torch.float64), SC.terms_eval(c, vis, torch.float32)
    for k in ("D", "S", "T", "dC"):
        scale = float(ref[k].abs().max())
        ratio = float((got[k].double() - ref[k]).abs().max()) / scale
        print(f"{name} {kind} {mask} {k}: float32 error {ratio:.3e} of the largest value, {ratio / c.rtol:.4f} of the bound {c.rtol:g}")
        assert scale > 0 and ratio <= c.rtol, (k, ratio)


@pytest.mark.parametrize("name,kind", REFERENCED)
@pytest.mark.parametrize("mask", SC.MASKS)
def test_emulated_dnormals_lie_inside_the_existing_constant(name, kind, mask):
    """``dnormals_emulated`` (float32, kernel order, with this shape's splits) against the float64 definition in units of
    ``dnormals_bound``: at most K = ``emulation_constant()``, which is four times the worst ratio over the OLDER cases."""
    K, old_worst = NR.emulation_constant()
    c = NR.case(*SC.SHAPES[name], kind)
    vis = c["vis"] if mask == "random" else None
    emu = NR.dnormals_emulated(c["nrm"], c["pos"], c["cam"], c["L"], c["C"], c["gD"], c["gS"], c["shin"], vis=vis)
    ratio, ref = NR.error_ratio(torch.from_numpy(emu), c, mask)
    print(f"{name} {kind} {mask} d normals: emulation's worst error {ratio:.3f} units, {ratio / K:.4f} of K = {K:.3f} "
          f"(older cases' worst {old_worst:.3f})")
    assert float(ref["d"].abs().max()) > 0 and ratio <= K
    assert float(abs(emu[c["bg"].numpy()]).max()) == 0.0


@pytest.mark.parametrize("name,kind", REFERENCED_GGX)
@pytest.mark.parametrize("mask", SC.MASKS)
def test_float32_microfacet_terms_lie_inside_the_existing_factors(name, kind, mask):
    """``microfacet_ref.evaluate`` in float32 against float64 under ``over_bound`` with ``factors()`` (four times the float32
    evaluation's worst ratio over the OLDER cases) and FLOOR."""
    fac = GR.factors()
    shape = SC.SHAPES[name]
    c = GR.case(*shape, kind)
    ref = GR.reference(*shape, kind, mask)
    got = GR.evaluate(c, c.vis if mask == "random" else None, dtype=torch.float32)
    for k in ("D", "S0", "S1", "dC", "dalpha", "dn"):
        over, raw = GR.over_bound(got[k], ref[k], fac[k]), GR.error_ratio(got[k], ref[k])
        print(f"{name} {kind} {mask} {k}: float32 error {over:.4f} of the bound (ratio to its scale {raw:.3e}, factor {fac[k]:.3e}, "
              f"floor {GR.FLOOR:g})")
        assert float(ref[k][0].abs().max()) > 0 and over <= 1.0, (k, over)
