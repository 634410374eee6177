"""Every sample of a tile counted exactly once (pytest -m gpu): the decoder's fused forward / loss / backward kernels on the hot-sample
problems of tests/hot_sample_cases.py -- a loss weight that is exactly zero except at one chosen sample per image, so that a sample
dropped, doubled, read from its neighbour's row or leaked from the next image is an error of 100 % in dZ[b] -- against the float64
oracle, at the bound that file derives from the reference alone.  The kernels: k_reni_train_bf16 in its training, frozen,
statistics, FiLM and L0X instances, k_reni_l0_ring, k_reni_dw1 and k_reni_dw1_ring, k_reni_wide256<1 / 2> with k_dw_frag and
k_wide_head_dw, and the generic chain of reni_dev_main.inc / reni_dev_stream.inc; every case asserts through path_info that the
family it is about is the one in force.

Per launch: loss term 0, dZ[b] of every hot image and every parameter gradient within the bound (with the prior live also the
WeightedMSE term, and dZ[b] with the prior's exact 2 alpha Z taken off both sides: the prior is all but 1 % of either); dZ[b] of every
image without a hot sample exactly what the prior alone gives (WeightedMSE: exactly 0); per group: two calls give equal bits; a frozen concat
decoder also with sparse_weight=True (equal bits) and "pixels" (2e-6 relative), the relations of
test_sparse_weight_leaves_out_only_exact_zeros at the positions its block masks do not reach; an all-cold weight gives loss 0 and
all-zero gradients.  Every figure is printed before it is asserted: case, launch, quantity, error, bound, error / bound."""
import os

import pytest
import torch

from oracle import reni_oracle as O
from tests import hot_sample_cases as HS
from tests.util import flat_params, make_plan, unflatten

pytestmark = pytest.mark.gpu

_PLANS = {}    # (spec, dtype, switches) -> Plan
_MODELS = {}   # FiLM: case id -> module


@pytest.fixture(scope="module", autouse=True)
def _one_reference_thread():
    """(the references are a few hundred small problems: a thread pool only slows them down)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _plan(c):
    key = (c.nd, c.eq, c.H, c.L, c.dtype, c.env, c.wg)
    if key not in _PLANS:
        env = {e: "1" for e in c.env}
        if c.wg is not None:
            env["RENI_TRAIN_WG"] = str(c.wg)
        before = {e: os.environ.get(e) for e in env}   # (whatever the process was started with is put back)
        os.environ.update(env)   # (read once, at plan creation)
        try:
            _PLANS[key] = make_plan(c.spec, c.dtype)
        finally:
            for e, v in before.items():
                os.environ.pop(e, None)
                if v is not None:
                    os.environ[e] = v
    return _PLANS[key]


def _model(c, dev):
    key = c.id   # (a case's parameters come from its own generator)
    if key not in _MODELS:
        from reni_amd.film import RENIAutoDecoderFiLM
        m = RENIAutoDecoderFiLM(c.B, c.nd, c.eq, c.H, c.L + 1, 12, 1, 3, "tanh", not c.need_dw)
        m.load_state_dict({"model." + k: v for k, v in HS.problem(c)[0].items()}, strict=False)
        _MODELS[key] = m.set_compute_dtype(c.dtype).to(dev)
    return _MODELS[key]


def _path_plan(c, dev):
    return _model(c, dev)._plan() if c.film else _plan(c)


def _run(c, W, T, dev, broadcast=False, sparse=False):
    """-> dict(terms, loss, dZ, grads) on the CPU; target and weight go in as contiguous [B, P, 3] tensors (a broadcast weight: [1, P, 3])"""
    params, Z, D, _ = HS.problem(c)
    Wd = (W[:1] if broadcast else W).contiguous().to(dev)
    Td = T.contiguous().to(dev)
    if c.film:
        m = _model(c, dev)
        m.zero_grad()
        Zd = Z.to(dev).requires_grad_(True)
        terms = m.fused_loss(Zd, D.to(dev), Td, Wd)
        terms[0].backward()
        grads = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None and k != "Z"}
        return dict(terms=terms.detach().cpu().clone(), loss=float(terms[0].detach()), dZ=Zd.grad.cpu().clone(), grads=grads)
    plan = _plan(c)
    lt, dZ, dp, _ = plan.forward_loss_backward(Z.to(dev), D.to(dev), flat_params(c.spec, params).to(dev), Td, Wd, loss_kind=c.loss,
                                               alpha=c.alpha, beta=c.beta, need_dw=c.need_dw, sparse_weight=sparse)
    grads = {k: v.clone() for k, v in unflatten(c.spec, dp.cpu()).items()} if c.need_dw else {}
    return dict(terms=lt.cpu().clone(), loss=float(lt[0]), mse=float(lt[1]), dZ=dZ.cpu().clone(), grads=grads)


def _same_bits(a, b):
    return (torch.equal(a["terms"], b["terms"]) and torch.equal(a["dZ"], b["dZ"]) and a["grads"].keys() == b["grads"].keys()
            and all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"]))


@pytest.mark.parametrize("c,kind", HS.groups(), ids=lambda v: v.id if isinstance(v, HS.Case) else v)
def test_hot_samples_against_the_float64_reference(c, kind):
    dev = torch.device("cuda:0")
    info = _path_plan(c, dev).path_info(c.B, c.P, need_dw=c.need_dw)
    print(c.id, kind, info)
    for k, v in c.expect:   # the kernel family the case is about is the one in force
        assert info[k] == v, (k, info)
    assert info["workgroups"] == c.G, info
    assert sorted(info["env_overrides"]) == sorted(c.env + (("RENI_TRAIN_WG",) if c.wg is not None else ())), info
    Z = HS.problem(c)[1]
    bad = []
    for i, l in enumerate(HS.KINDS[kind](c)):
        r = HS.reference(c, kind, i)
        ref, bound = r["ref"], r["bound"]
        got = _run(c, r["W"], r["T"], dev, broadcast=l.broadcast)
        assert torch.isfinite(got["terms"]).all() and torch.isfinite(got["dZ"]).all() and all(torch.isfinite(g).all() for g in got["grads"].values())
        if c.need_dw:
            assert set(ref["grads"]) <= set(got["grads"]), sorted(set(ref["grads"]) - set(got["grads"]))   # every key is compared
        errs = [(q, e, bound["loss"]) for q, e in HS.loss_errors(c, got, ref).items()]
        errs += [(q, e, bound["grad"]) for q, e in HS.errors(c, got, ref, r["hot_images"]).items()]
        for q, e, bnd in errs:
            print("%s %s[%d] hot %s  %-40s err %.3e  bound %.3e  err/bound %.3f" % (c.id, kind, i, l.hot, q, e, bnd, e / bnd))
            if not e <= bnd:
                bad.append((i, q, e, bnd))
        for b in range(c.B):   # an image without a hot sample: what the prior alone gives
            if b in r["hot_images"]:
                continue
            if c.loss == "mse":
                ok = not bool(got["dZ"][b].any())
            else:   # (the data term is an exact 0: what is left is the kernels' own fp32 product fl(2 alpha) z, bit for bit)
                ok = torch.equal(got["dZ"][b], Z[b] * torch.tensor(2 * c.alpha, dtype=torch.float32))
            print("%s %s[%d] cold image %d: max |dZ| %.3e %s" % (c.id, kind, i, b, float(got["dZ"][b].abs().max()), "ok" if ok else "WRONG"))
            if not ok:
                bad.append((i, "cold dZ[%d]" % b, float(got["dZ"][b].abs().max()), 0.0))
        again = _run(c, r["W"], r["T"], dev, broadcast=l.broadcast)
        assert _same_bits(got, again), ("two calls differ", i, l.hot)
        if not c.film and not c.need_dw:   # frozen concat decoder: the tile lists and the packed pixels
            tiles = _run(c, r["W"], r["T"], dev, broadcast=l.broadcast, sparse=True)
            assert _same_bits(got, tiles), ("sparse_weight=True", i, l.hot)
            px = _run(c, r["W"], r["T"], dev, broadcast=l.broadcast, sparse="pixels")
            assert torch.allclose(px["terms"], got["terms"], rtol=2e-6, atol=0), ("pixels: loss terms", i, l.hot, px["terms"], got["terms"])
            for b in range(c.B):
                d, n = float((px["dZ"][b] - got["dZ"][b]).norm()), float(got["dZ"][b].norm())
                assert d <= 2e-6 * n + 1e-12, ("pixels: dZ", i, l.hot, b, d, n)
    if kind == "dz" and c.loss == "mse":   # exact-zero anchor: an all-cold weight
        l = HS.Launch(tuple(() for _ in range(c.B)))
        got = _run(c, HS.weight_of(c, l), HS.target_of(c, l), dev)
        assert float(got["loss"]) == 0.0 and not bool(got["dZ"].any()) and not any(bool(g.any()) for g in got["grads"].values()), "all-cold weight"
    assert not bad, bad
