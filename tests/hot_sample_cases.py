"""Hot-sample problems for the decoder's fused forward / loss / backward kernels: cases, float64 reference and bound (no GPU).

The loss weight is data of shape [B, P, 3].  Exactly zero everywhere except at one chosen sample per image, it makes that sample the
whole problem: the float64 oracle's loss, dZ[b] and parameter gradients are that sample's contribution alone, and a sample that a
kernel drops, counts twice, reads from its neighbour's row or leaks from the next image's rows is an error of order one in dZ[b] --
not the 1 / (B P) it is under a dense weight, thirty times below the whole-problem bf16 tolerances.

Positions come from the kernels' structure (`positions`): a tile is 128 consecutive samples of one image, four waves' quarters of
32 rows; the training instances own contiguous tile ranges [g n / G, (g + 1) n / G) that cross images; k_reni_wide256 works on tile
pairs; a ragged last tile masks its tail.  WeightedMSE cases give every cold sample a target of magnitude 1e3: the reference does
not see it (its weight is exactly zero), a kernel that reads a weight row one sample or one image off does.

Reference: O.fwd_loss_bwd / O.film_fwd_loss_bwd on float64 copies of every input.  Bound, one rule for every compared quantity:
    bf16 plans   max(c, 1.5 e_ac)   c: tests/test_gpu_parity.py::TOL (loss 2e-3, gradients 3e-2; FiLM: beside it twice what the
                                    reference's dZ[b] moves by with its hidden and head weights rounded to bf16, the floor of
                                    tests/test_gpu_fuzz.py::_run_case); e_ac: the reference's own error on the same problem with its
                                    linear layers under torch.autocast("cpu", torch.bfloat16), the worst over dZ[b] of the hot
                                    images and every compared parameter (the bf16_bound construction of tests/test_gpu_fuzz.py)
    f32 plans    max(c, 2.5 e_32)   c: loss 2e-6, gradients 1e-5; e_32: the oracle in fp32 against its float64 run
    cap          0.3: the fault this file exists for is an error of 1.0, a bound above 0.3 asserts nothing.  No case may need more
                 (tests/test_hot_sample_cpu.py); the only freedom is the seed, chosen on the CPU.
dZ is compared image by image, never over the whole tensor.  With loss_kind="test" (alpha 1e-3, beta 1e-1) the prior's 2 alpha Z is
all but 0.5 % of dZ[b] and the prior all but 1 % of loss term 0, which would hide the hot sample again: there dZ[b] is compared whole
AND with the prior's exact gradient taken off both sides, and the WeightedMSE term beside term 0 (`errors`, `loss_errors`).  The
cosine term of that loss is multiplied by the weight of PIXEL 0 (O.weighted_cosine): it is live only in the launches whose hot
sample is sample 0 (the first dZ launch, one leak launch), where it spans the whole image with ordinary targets and dominates
dZ[b]; in every other launch of a test-loss case beta contributes exactly nothing."""
import functools
from dataclasses import dataclass, field
from typing import Tuple

import torch

from oracle import reni_oracle as O
from tests.util import random_problem

TILE = 128
CAP = 0.3
C_BF16 = dict(loss=2e-3, grad=3e-2)   # tests/test_gpu_parity.py::TOL["bf16"]
C_F32 = dict(loss=2e-6, grad=1e-5)    # tests/test_gpu_parity.py::TOL["f32"]
MIN_RESIDUAL = 0.25                   # every hot sample's |out - target| in the reference: its loss is no small difference
ALPHA, BETA = 1e-3, 1e-1              # loss_kind="test": prior and cosine term live (the statistics instance runs)


# ---------------------------------------------------------------------------------------------------------------------------
# positions
# ---------------------------------------------------------------------------------------------------------------------------

def tiles_per_image(P):
    return (P + TILE - 1) // TILE


def tile_ranges(B, P, G):
    """The contiguous tile range of each of G workgroups (reni_dev_train.inc: t_first / t_stop)."""
    n = B * tiles_per_image(P)
    return [(g * n // G, (g + 1) * n // G) for g in range(G)]


def _tile_span(P, tin):
    """first and last valid sample of tile `tin` of an image"""
    return tin * TILE, min(P, (tin + 1) * TILE) - 1


def positions(B, P, G):
    """-> sorted list of (image, sample): the samples at which one of the kernels' masks, owner lanes, wave quarters, flushes or
    range / image-run boundaries can go wrong at this shape (the module docstring)."""
    tpi = tiles_per_image(P)
    common = [r for r in (0, 31, 32, 63, 64, 95, 96, 127) if r < P]                 # the wave quarters of the first tile
    whole = P // TILE
    if whole >= 1:
        common += [(whole - 1) * TILE, whole * TILE - 1]                            # rows 0 and 127 of the last whole tile
    if P % TILE:
        common += [whole * TILE, P - 1] + ([P - 2] if P >= 2 else [])               # the ragged tile: row 0, the last valid lanes
    out = set()
    for i, p in enumerate(sorted(set(common))):
        out.add((i % B, p))
    for b in range(B):
        out.add((b, P - 1))                                                         # the end of every image
    for lo, hi in tile_ranges(B, P, G):
        if hi <= lo:
            continue
        for t in (lo, hi - 1):                                                      # tiles that begin or end a workgroup's range
            b, tin = divmod(t, tpi)
            first, last = _tile_span(P, tin)
            out.update({(b, first), (b, last)})
        for b in range(lo // tpi, (hi - 1) // tpi + 1):                             # image runs inside the range
            t0, t1 = max(lo, b * tpi), min(hi, (b + 1) * tpi) - 1
            for t in (t0, t1):
                first, last = _tile_span(P, t - b * tpi)
                out.update({(b, first), (b, last)})
    return sorted(out)


def boundary_samples(B, P, G):
    """Brute force, sample by sample: the first and last sample of every workgroup range and of every image run inside one, and
    every image's P - 1 (what `positions` must contain at the least; tests/test_hot_sample_cpu.py)."""
    tpi = tiles_per_image(P)
    n = B * tpi
    owner = []                                                                      # (workgroup, image, sample) of every valid sample, in tile order
    for t in range(n):
        g = next(g for g in range(G) if g * n // G <= t < (g + 1) * n // G)
        b, tin = divmod(t, tpi)
        owner += [(g, b, p) for p in range(tin * TILE, min(P, (tin + 1) * TILE))]
    need = {(b, P - 1) for b in range(B)}
    for i, (g, b, p) in enumerate(owner):
        if i == 0 or owner[i - 1][:2] != (g, b) or i + 1 == len(owner) or owner[i + 1][:2] != (g, b):
            need.add((b, p))
    return need


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Launch:
    hot: Tuple[Tuple[int, ...], ...]   # per image: its hot samples
    broadcast: bool = False            # the weight is passed as [1, P, 3] (stride 0 over images)


@dataclass(frozen=True)
class Case:
    id: str
    family: str
    film: bool
    nd: int
    eq: str
    H: int
    L: int
    dtype: str
    B: int
    P: int
    wg: object          # RENI_TRAIN_WG, or None
    env: Tuple[str, ...]
    need_dw: bool
    loss: str
    seed: int
    expect: Tuple[Tuple[str, object], ...] = field(default=())   # path_info entries the case is about
    bcast: bool = False                                          # also run with a broadcast weight

    @property
    def G(self):
        return self.wg if self.wg is not None else self.B * tiles_per_image(self.P)

    @property
    def spec(self):
        if self.film:
            return O.FilmSpec(self.nd, self.eq, self.H, self.L + 1, 12, 1, 3, "tanh")
        return O.DecoderSpec(self.nd, self.eq, self.H, self.L, 3, True, "tanh")

    @property
    def alpha(self):
        return ALPHA if self.loss == "test" else 0.0

    @property
    def beta(self):
        return BETA if self.loss == "test" else 0.0


# Seeds chosen on the CPU (tests/test_hot_sample_cpu.py states the conditions): a case not listed takes 7000 + its index.
SEEDS = {
    "wide-train-2x300": 7128,                            # (7028: removing one of dW launch 0's samples moved dW_0 by 0.19 < 3 x 0.082)
    "frozen-nd36-test-3x129": 7125,                      # (7016: the weight rows read one sample off moved a dZ[b] by 0.618 < 3 x 0.207)
    "film-H128-train-2x256": 7141,                      # (7035: a bound of 0.51)
    "film-H128-frozen-2x256": 7140,                      # (7038: 0.45)
    "film-H256-train-advice-regression-3x127": 7140,     # (7040: 0.33)
}


def _build_cases():
    out = []

    def add(family, B, P, wg=None, film=False, nd=36, eq="SO2", H=128, L=5, dtype="bf16", env=(), need_dw=True, loss="mse", expect=(),
            bcast=False, tag=""):
        cid = "%s%s-%dx%d%s" % (family, tag, B, P, "" if wg is None else "-wg%d" % wg)
        assert all(c.id != cid for c in out), cid
        out.append(Case(cid, family, film, nd, eq, H, L, dtype, B, P, wg, tuple(env), need_dw, loss, SEEDS.get(cid, 7000 + len(out)),
                        tuple(sorted(dict(expect).items())), bcast))

    pers = dict(persistent_kernels=True, fragment_stream="none")
    for L in (5, 3):    # the L0X instance + k_reni_l0_ring: the shapes of tests/test_gpu_shared_wimage.py
        for B, P, wg in ((1, 128, None), (2, 256, 3), (3, 384, 2)):
            add("l0x", B, P, wg, L=L, tag="-L%d" % L, expect=dict(pers, dw1_kernel="k_reni_l0_ring"), bcast=(L == 5 and B == 2))
    add("no_l0x", 3, 384, 2, env=("RENI_NO_L0X",), expect=dict(pers, dw1_kernel="k_reni_dw1_ring"))
    add("dw1_old", 3, 384, 2, env=("RENI_DW1_OLD",), expect=dict(pers, dw1_kernel="k_reni_dw1"))
    for B, P, wg in ((3, 129, 2), (2, 300, 3), (3, 127, None), (2, 161, None)):   # ragged: round 4's kernels with no switch set
        add("ragged", B, P, wg, expect=dict(pers, dw1_kernel="k_reni_dw1"), bcast=(P == 129))
    for nd in (36, 9):   # frozen decoder: the strided instance, and with loss_kind="test" the statistics instance in front of it
        for loss in ("mse", "test"):
            for B, P in ((3, 384), (3, 129), (2, 300)):
                add("frozen", B, P, nd=nd, need_dw=False, loss=loss, tag="-nd%d-%s" % (nd, loss), expect=dict(pers, dw1_kernel="none"),
                    bcast=(P == 129 and nd == 36))
    for need_dw in (True, False):   # H = 256: k_reni_wide256<2> + k_dw_frag + k_wide_head_dw, and <1>
        for B, P in ((1, 128), (3, 384), (1, 100), (3, 127), (2, 300)):
            add("wide", B, P, nd=9, H=256, need_dw=need_dw, tag="-train" if need_dw else "-frozen", bcast=(P == 127),
                expect=dict(persistent_kernels=True, dw1_kernel="none", fragment_stream="bf16" if need_dw else "none"))
    for H in (128, 256):   # FiLM through RENIAutoDecoderFiLM.fused_loss; (3, 127) at 256 features: ADVICE's regression case
        for need_dw in (True, False):
            for B, P in ((3, 127), (2, 256), (3, 129)):
                tag = "-H%d-%s" % (H, "train" if need_dw else "frozen")
                if H == 256 and (B, P) == (3, 127):
                    tag += "-advice-regression"
                add("film", B, P, film=True, nd=9, H=H, L=4, need_dw=need_dw, tag=tag, bcast=(P == 129 and need_dw),
                    expect=dict(persistent_kernels=True, dw1_kernel="k_reni_dw1" if H == 128 else "none",
                                fragment_stream="none" if H == 128 else "bf16"))
    for B, P in ((3, 129), (2, 300)):   # the generic chain (reni_dev_main.inc / reni_dev_stream.inc)
        gen = dict(env=("RENI_NO_PERSIST",), expect=dict(persistent_kernels=False, dw1_kernel="none"))
        add("generic", B, P, tag="-bf16", bcast=(P == 129), **gen)
        add("generic", B, P, dtype="f32", tag="-f32", **gen)
        add("generic", B, P, dtype="f32", nd=9, eq="SO3", H=64, L=2, tag="-f32-so3-64x2", **gen)
    return out


CASES = _build_cases()


def dz_launches(c):
    """`positions` packed into launches of one hot sample per image: launch k takes the k-th position of every image that has one
    (the images that have none are all cold in that launch)."""
    per = [[p for b, p in positions(c.B, c.P, c.G) if b == i] for i in range(c.B)]
    return [Launch(tuple((lst[k],) if k < len(lst) else () for lst in per)) for k in range(max(len(lst) for lst in per))]


def dw_launches(c):
    """At most two hot samples in all (FiLM: one -- its bounds leave no room for the condition on two), the other images cold: row
    0 of the first tile, P - 1, the last sample of a workgroup's range and of an image run."""
    if not c.need_dw:
        return []
    B, P = c.B, c.P
    lo, hi = tile_ranges(B, P, c.G)[0]
    b_end, tin_end = divmod(hi - 1, tiles_per_image(P))
    picks = [(0, 0), (B - 1, P - 1), (b_end, _tile_span(P, tin_end)[1]), (0, P - 1)]
    picks = list(dict.fromkeys(picks))
    groups = []
    while picks:
        g = [picks.pop(0)]
        mate = next((x for x in picks if x[0] != g[0][0]), None)   # two hot samples lie in two images
        if mate is not None and not c.film:
            picks.remove(mate)
            g.append(mate)
        groups.append(g)
    return [Launch(tuple(tuple(p for b, p in g if b == i) for i in range(B))) for g in groups]


def leak_launches(c):
    """Image 0 all cold except P - 1 and image 1 hot at samples 0 and 1 -- an unmasked tail lane of image 0's last tile reads image
    1's rows -- and the same with the roles swapped."""
    if c.B < 2:
        return []
    rest = tuple(() for _ in range(c.B - 2))
    return [Launch(((c.P - 1,), (0, 1)) + rest), Launch(((0, 1), (c.P - 1,)) + rest)]


def bcast_launches(c):
    """A [1, P, 3] weight (stride 0 over the images, ops._loss_views): the same sample is hot in every image."""
    return [Launch(tuple((c.P - 1,) for _ in range(c.B)), broadcast=True)] if c.bcast else []


KINDS = {"dz": dz_launches, "dw": dw_launches, "leak": leak_launches, "bcast": bcast_launches}


def groups():
    """(case, kind) of every non-empty launch group: one GPU test each"""
    return [(c, k) for c in CASES for k, fn in KINDS.items() if fn(c)]


# ---------------------------------------------------------------------------------------------------------------------------
# problem, reference, bound
# ---------------------------------------------------------------------------------------------------------------------------

def _forward(c, params, Z, D):
    return O.film_forward(c.spec, params, Z, D) if c.film else O.reni_forward(c.spec, params, Z, D)


@functools.lru_cache(maxsize=None)
def problem(c):
    """-> (params, Z, D, T) in fp32.  T lies in [-1, 1]; at every sample some launch of the case makes hot it is redrawn (from a
    generator of its own) until the float64 reference's output is at least 0.3 away from it."""
    if c.film:   # (the construction of tests/test_gpu_fuzz.py::_run_case)
        gen = torch.Generator().manual_seed(c.seed)
        Z = torch.randn(c.B, c.nd, 3, generator=gen) * 0.6
        D = torch.nn.functional.normalize(torch.randn(c.B, c.P, 3, generator=gen), dim=-1)
        torch.rand(1, c.P, 3, generator=gen)
        T = torch.rand(c.B, c.P, 3, generator=gen) * 2 - 1
        params = O.film_init_params(c.spec, gen)
    else:
        params, Z, D, _, T = random_problem(c.spec, c.B, c.P, seed=c.seed, per_image_dirs=True)
    out = _forward(c, {k: v.double() for k, v in params.items()}, Z.double(), D.double())
    T = T.clone()
    for fn in KINDS.values():
        for l in fn(c):
            for b, hot in enumerate(l.hot):
                for p in hot:
                    g = torch.Generator().manual_seed(c.seed * 100003 + b * c.P + p)
                    while float((out[b, p] - T[b, p].double()).norm()) < 0.3:
                        T[b, p] = torch.rand(3, generator=g) * 2 - 1
    return params, Z, D, T


def weight_of(c, l):
    W = torch.zeros(c.B, c.P, 3)
    for b, hot in enumerate(l.hot):
        for p in hot:
            W[b, p] = 1.0
    return W


def target_of(c, l, cold_scale=1.0):
    """ordinary targets at the hot samples; WeightedMSE: magnitude 1e3 (x cold_scale) at the cold ones"""
    T = problem(c)[3]
    if c.loss != "mse":
        return T
    cold = torch.where(T >= 0, torch.tensor(1e3), torch.tensor(-1e3)) * cold_scale
    return torch.where(weight_of(c, l) > 0, T, cold)


def oracle(c, W, T, dtype=torch.float64, params=None, need_dw=None):
    """-> dict(loss, dZ, grads, out) of the reference on `dtype` copies of every input (need_dw: the case's, unless given)"""
    p0, Z, D, _ = problem(c)
    need_dw = c.need_dw if need_dw is None else need_dw
    ps = {k: v.to(dtype) for k, v in (params or p0).items()}
    if c.film:
        r = O.film_fwd_loss_bwd(c.spec, ps, Z.to(dtype), D.to(dtype), T.to(dtype), W.to(dtype), c.loss, c.alpha, c.beta)
        return dict(loss=r["terms"][0], dZ=r["dZ"], grads=r["grads"] if need_dw else {}, out=r["out"])
    r = O.fwd_loss_bwd(c.spec, ps, Z.to(dtype), D.to(dtype), T.to(dtype), W.to(dtype), c.loss, c.alpha, c.beta, need_dw=need_dw)
    return dict(loss=r["loss_terms"][0], mse=r["loss_terms"][1], dZ=r["dZ"], grads=r["grads"], out=r["out"])


def prior_dz(c):
    """d prior / d Z = 2 alpha Z in float64 (loss_kind="test"; zero for WeightedMSE)"""
    return 2.0 * c.alpha * problem(c)[1].double()


def errors(c, got, ref, hot_images):
    """rel-L2 of every compared gradient of `got` against `ref`: dZ image by image, every parameter.  With the prior live (alpha =
    1e-3) 2 alpha Z is all but 0.5 % of dZ[b] and would hide the hot sample: there dZ[b] is compared whole AND with the prior's
    exact gradient taken off both sides (fp32 rounding of the sum: 1e-7 of 2e-3 against a data term of 1e-5)."""
    e = {"dZ[%d]" % b: O.rel_l2(got["dZ"][b].double().numpy(), ref["dZ"][b].numpy()) for b in hot_images}
    if c.alpha:
        pr = prior_dz(c)
        e.update({"dZ[%d] - 2 alpha Z" % b: O.rel_l2((got["dZ"][b].double() - pr[b]).numpy(), (ref["dZ"][b] - pr[b]).numpy()) for b in hot_images})
    e.update({k: O.rel_l2(got["grads"][k].double().numpy(), v.numpy()) for k, v in ref["grads"].items()})
    return e


def loss_errors(c, got, ref):
    """relative error of loss term 0 and, with the prior live (it is all but 1 % of term 0), of the WeightedMSE term beside it"""
    e = {"loss": abs(got["loss"] - ref["loss"]) / abs(ref["loss"])}
    if c.alpha:
        e["mse term"] = abs(got["mse"] - ref["mse"]) / abs(ref["mse"])
    return e


def _bf16_weights(c, params):
    hit = lambda k: k.endswith("weight") and ((k.startswith("net.") and not k.startswith("net.0.")) or k.startswith("final_layer."))  # noqa: E731
    return {k: (v.bfloat16().float() if hit(k) else v) for k, v in params.items()}


@functools.lru_cache(maxsize=None)
def reference(c, kind, i):
    """-> dict(W, T, ref, hot_images, bound=dict(loss, grad), own=dict(loss, grad)) of launch i of the case's `kind` group: the float64
    reference and the bound, from the reference alone (`own`: its error under autocast -- fp32 for an f32 plan -- before the factor)."""
    l = KINDS[kind](c)[i]
    W, T = weight_of(c, l), target_of(c, l)
    ref = oracle(c, W, T)
    hot_images = [b for b, h in enumerate(l.hot) if h]
    if c.dtype == "bf16":
        with torch.autocast("cpu", dtype=torch.bfloat16):
            low = oracle(c, W, T, torch.float32)
        base, factor = dict(C_BF16), 1.5
        if c.film:
            e_w = errors(c, oracle(c, W, T, torch.float32, _bf16_weights(c, problem(c)[0])), dict(ref, grads={}), hot_images)
            base["grad"] = max(base["grad"], 2.0 * max(e_w.values()))
    else:
        low = oracle(c, W, T, torch.float32)
        base, factor = dict(C_F32), 2.5
    own = dict(loss=max(loss_errors(c, low, ref).values()), grad=max(errors(c, low, ref, hot_images).values()))
    bound = {k: max(base[k], factor * own[k]) for k in base}
    return dict(launch=l, W=W, T=T, ref=ref, hot_images=hot_images, bound=bound, own=own)
