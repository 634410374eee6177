"""The conditions under which tests/test_gpu_hot_samples.py is a test, checked on the CPU from the float64 reference alone
(tests/hot_sample_cases.py): for every committed case and seed
  * every bound is at most 0.3 -- the fault the GPU file exists for is an error of 1.0;
  * every hot sample's |out - target| in the reference is at least 0.25: one sample's loss is no small difference;
  * in a dW launch with two hot samples, removing either moves every compared parameter's gradient by at least 3 x the bound;
  * the bound has teeth: the reference with the weight rows read one sample off (every dZ, leak and broadcast launch), and with the
    hot samples removed or counted twice (exactly 1.0 where the loss is linear in the weight: first and last dZ launch, leak and
    broadcast launches), is off by at least 3 x the case's bound in dZ[b] of every hot image;
  * the reference does not see the cold rows: every cold target x 10 leaves every reference quantity bit-equal;
and the position generator against a brute-force statement of the tiling."""
import pytest
import torch

from oracle import reni_oracle as O
from tests import hot_sample_cases as HS


@pytest.fixture(scope="module", autouse=True)
def _one_reference_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


SHAPES = sorted({(c.B, c.P, c.G) for c in HS.CASES} | {(B, P, G) for B, P in ((3, 384), (2, 300), (3, 129), (5, 257)) for G in (1, 2, 3, 4, 7)})


@pytest.mark.parametrize("B,P,G", SHAPES)
def test_positions_hold_every_boundary_of_the_tiling(B, P, G):
    got = set(HS.positions(B, P, G))
    assert all(0 <= b < B and 0 <= p < P for b, p in got)
    missing = HS.boundary_samples(B, P, G) - got
    assert not missing, sorted(missing)
    rows = {p for b, p in got}
    assert {r for r in (0, 31, 32, 63, 64, 95, 96, 127) if r < P} <= rows
    if P % HS.TILE:
        assert {P // HS.TILE * HS.TILE, P - 1, P - 2} & set(range(P)) <= rows


def test_every_launch_has_one_hot_sample_per_image_and_every_position_is_launched():
    for c in HS.CASES:
        ls = HS.dz_launches(c)
        assert all(len(h) <= 1 for l in ls for h in l.hot)
        assert sorted((b, h[0]) for l in ls for b, h in enumerate(l.hot) if h) == HS.positions(c.B, c.P, c.G)
        for l in HS.dw_launches(c):
            assert 1 <= sum(len(h) for h in l.hot) <= 2
    assert len({c.id for c in HS.CASES}) == len(HS.CASES)
    assert any("advice-regression" in c.id and c.film and c.H == 256 and (c.B, c.P) == (3, 127) for c in HS.CASES)


def _dz_only(c, W, T):
    return HS.oracle(c, W, T, need_dw=False)["dZ"]


def conditions(c):
    """-> the list of violated conditions of one case (empty: the case is a test)"""
    bad = []
    pr = HS.prior_dz(c)
    worst = max(HS.reference(c, kind, i)["bound"]["grad"] for kind, fn in HS.KINDS.items() for i in range(len(fn(c))))
    for kind, fn in HS.KINDS.items():
        for i, l in enumerate(fn(c)):
            r = HS.reference(c, kind, i)
            ref, W, T, bound = r["ref"], r["W"], r["T"], r["bound"]
            where = "%s %s[%d] hot %s" % (c.id, kind, i, l.hot)
            for k, v in bound.items():
                if not v <= HS.CAP:
                    bad.append("%s: %s bound %.3f above the cap (own error %.3f)" % (where, k, v, r["own"][k]))
            for b, hot in enumerate(l.hot):
                for p in hot:
                    res = float((ref["out"][b, p] - T[b, p].double()).norm())
                    if not res >= HS.MIN_RESIDUAL:
                        bad.append("%s: |out - target| = %.3f at (%d, %d)" % (where, res, b, p))
            # the faults, in the reference: removed, counted twice, the neighbour's row in the hot sample's place
            # (the neighbour's row: the weight rows read one sample off -- the hot weight meets the neighbour's target and output.  A
            #  fault that takes ALL of a neighbour's rows, target and direction included, is not in this list: on these smooth random
            #  decoders two samples' gradients under one target differ by 3 % to 15 % only, which no bf16 bound sees.)
            shifted_W = torch.zeros_like(W)
            for b, hot in enumerate(l.hot):
                for p in hot:
                    q = p + 1 if p + 1 < c.P and p + 1 not in hot else p - 1
                    if 0 <= q < c.P and q not in hot:
                        shifted_W[b, q] = 1.0
            # `neighbour`, the informative one, at every dZ, leak and broadcast launch.  `removed` and `twice` are exactly 1.0 wherever the
            # loss is linear in the weight (they then say only that the bound is under 1 / 3): at the first and last dZ launch -- the
            # first has sample 0 hot, where with loss_kind="test" the cosine term is live and the loss is NOT linear -- and at the leak
            # and broadcast launches.  All against the CASE's bound: its worst launch's.
            faults = []
            if kind != "dw":
                faults.append(("neighbour", shifted_W))
                if kind in ("leak", "bcast") or i in (0, len(fn(c)) - 1):
                    faults += [("removed", torch.zeros_like(W)), ("twice", 2 * W)]
            for name, Wm in faults:
                dZ = _dz_only(c, Wm, T)
                for b in r["hot_images"]:   # (with the prior live: the data term, as the GPU file compares it)
                    e = O.rel_l2((dZ[b] - pr[b]).numpy(), (ref["dZ"][b] - pr[b]).numpy())
                    if not e >= 3 * worst:
                        bad.append("%s: %s moves dZ[%d] by %.3f < 3 x %.3f" % (where, name, b, e, worst))
            if kind == "dw" and sum(len(h) for h in l.hot) == 2:
                # (WeightedMSE: the gradient is linear in the weight, so ONE more run -- the first hot image alone -- gives both halves)
                assert c.loss == "mse"
                first = r["hot_images"][0]
                Wm = torch.zeros_like(W)
                Wm[first] = W[first]
                g = HS.oracle(c, Wm, T)["grads"]
                for k, v in ref["grads"].items():
                    n = max(float(v.norm()), 1e-300)
                    for what, e in (("the second", float((v - g[k]).norm()) / n), ("the first", float(g[k].norm()) / n)):
                        if not e >= 3 * bound["grad"]:
                            bad.append("%s: removing %s hot sample moves %s by %.3f < 3 x %.3f" % (where, what, k, e, bound["grad"]))
            if kind == "dw":
                assert set(ref["grads"]) == set(c.spec.param_keys()), "every parameter key is compared"
            if i == 0 and c.loss == "mse":   # cold rows: not seen
                r10 = HS.oracle(c, W, HS.target_of(c, l, cold_scale=10.0))
                same = (r10["loss"] == ref["loss"] and torch.equal(r10["dZ"], ref["dZ"])
                        and all(torch.equal(r10["grads"][k], v) for k, v in ref["grads"].items()))
                if not same or torch.equal(HS.target_of(c, l, cold_scale=10.0), T):
                    bad.append("%s: the reference sees the cold rows" % where)
    return bad


@pytest.mark.parametrize("c", HS.CASES, ids=lambda c: c.id)
def test_case_is_a_test(c):
    bad = conditions(c)
    assert not bad, "\n".join(bad)
