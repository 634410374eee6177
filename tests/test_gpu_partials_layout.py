"""The quad-row layout of the weight-gradient partials on the config-2 path: the L0X training instance flushes a lane's four
consecutive rows of a column as one 16-byte store, and the 16-byte fixed-order reducer (k_tail_a's extra blocks,
k_reduce_partials_quad) sums those buffers and undoes the permutation where it writes the gradient.  (k_reni_l0_ring's layer-1
partials stay flat.)  The layout moves values and adds no arithmetic, so the checks are bit equalities wherever both sides run the
same arithmetic, and the existing tolerances where the other side is another kernel.

Shapes are chosen for the slot counts the reducer sees (one slot per workgroup, wave g of a block sums slots g, g + 4, ... with
32 slots per trip of its main loop):
    B = 3,  16 x 32:  12 tiles -> 12 slots: only the remainder loop, and the last block's `e < n` guard
    B = 5,  32 x 64:  80 tiles -> 80 slots: main loop plus remainder
    B = 17, 32 x 64: 272 tiles -> more tiles than CUs: every workgroup a range of tiles, a short last range
"""
import os
import subprocess
import sys

import pytest
import torch

from oracle import reni_oracle as O
from tests.util import flat_params, make_plan, random_problem, unflatten

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 32), (5, 64), (17, 64)]  # (images, equirect width; height = width / 2)
SPEC = dict(ndims=36, eq="SO2", H=128, L=5)


def _spec():
    return O.DecoderSpec(SPEC["ndims"], SPEC["eq"], SPEC["H"], SPEC["L"], 3, True, "tanh")


def _problem(B, W):
    return random_problem(_spec(), B, 0, seed=40 + B, grid_w=W)


def _run(plan, B, W, dev):
    params, Z, D, Wt, T = _problem(B, W)
    fp = flat_params(_spec(), params).to(dev)
    lt, dZ, dp, _ = plan.forward_loss_backward(Z.to(dev), D.to(dev), fp, T.to(dev), Wt.to(dev))
    return lt.cpu().clone(), dZ.cpu().clone(), dp.cpu().clone()


# The same calls with layer 0's backward inside the training kernel (RENI_NO_L0X: flat partials, the narrow reducer).  The variable is
# read once, at plan creation, and reni_path_info reports it: a fresh process keeps it out of this one.
_CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
from tests.test_gpu_partials_layout import SHAPES, _run, _spec
from tests.util import make_plan
dev = torch.device("cuda:0")
out = {{}}
for B, W in SHAPES:
    plan = make_plan(_spec(), "bf16")
    info = plan.path_info(B, W * W // 2)
    assert info["dw1_kernel"] == "k_reni_dw1_ring" and "RENI_NO_L0X" in info["env_overrides"], info
    out["%dx%d" % (B, W)] = list(_run(plan, B, W, dev))
torch.save(out, {path!r})
"""


@pytest.fixture(scope="module")
def without_l0x(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("no_l0x") / "grads.pt")
    env = dict(os.environ, RENI_NO_L0X="1")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, path=path)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return torch.load(path)


@pytest.fixture(scope="module")
def with_l0x():
    """(loss terms, dZ, dparams) of the L0X path per shape, computed once: two calls each, which must agree bit for bit."""
    dev = torch.device("cuda:0")
    out = {}
    for B, W in SHAPES:
        plan = make_plan(_spec(), "bf16")
        info = plan.path_info(B, W * W // 2)
        assert info["dw1_kernel"] == "k_reni_l0_ring" and not info["env_overrides"], info  # the L0X instance: quad-row partials
        a, b = _run(plan, B, W, dev), _run(plan, B, W, dev)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (B, W)
        out[(B, W)] = a
    return out


@pytest.mark.parametrize("B,W", SHAPES)
def test_quad_row_partials_against_the_flat_path_and_fp32(with_l0x, without_l0x, B, W):
    """Gradients of the L0X path (quad-row partials of layers >= 2 and the head behind them, summed by k_tail_a's extra blocks)
    against RENI_NO_L0X in a fresh process at the tolerance tests/test_gpu_l0x.py uses for that comparison (1e-6 on the
    loss, 2e-3 rel-L2 on dZ and on the flat decoder gradient), and, tensor by tensor, against the fp32 generic kernels at
    tests/test_gpu_parity.py's bf16 gradient tolerance (3e-2 rel-L2).  A value stored to, or read from, the wrong word of a slice is an
    error of order one in that layer's tensor."""
    dev = torch.device("cuda:0")
    spec = _spec()
    lt, dZ, dp = with_l0x[(B, W)]
    lo, dZo, dpo = without_l0x["%dx%d" % (B, W)]
    assert torch.isfinite(dp).all() and torch.isfinite(dZ).all()
    print("vs RENI_NO_L0X: loss", abs(float(lt[0]) - float(lo[0])) / abs(float(lo[0])), "dZ", O.rel_l2(dZ.numpy(), dZo.numpy()),
          "dparams", O.rel_l2(dp.numpy(), dpo.numpy()))
    assert abs(float(lt[0]) - float(lo[0])) <= 1e-6 * abs(float(lo[0]))
    assert O.rel_l2(dZ.numpy(), dZo.numpy()) <= 2e-3
    assert O.rel_l2(dp.numpy(), dpo.numpy()) <= 2e-3
    gp, gpo = unflatten(spec, dp), unflatten(spec, dpo)
    for k in gp:
        print("vs RENI_NO_L0X", k, O.rel_l2(gp[k].numpy(), gpo[k].numpy()))
    lf, dZf, dpf = _run(make_plan(spec, "f32"), B, W, dev)
    gpf = unflatten(spec, dpf)
    for k in gp:
        e = O.rel_l2(gp[k].numpy(), gpf[k].numpy())
        print("vs fp32", k, e)
        assert e <= 3e-2, (k, e)
    assert O.rel_l2(dZ.numpy(), dZf.numpy()) <= 3e-2


@pytest.mark.parametrize("B,W", SHAPES)
def test_the_early_reduction_of_quad_row_partials_gives_the_same_bits(with_l0x, B, W):
    """With a grad-ready event set (a data-parallel caller's hook) layers >= 2 and the head are reduced by a launch of their own in
    front of k_reni_l0_ring -- k_reduce_partials_quad -- instead of k_tail_a's extra blocks: the same body, the same bits."""
    from reni_amd import _lib
    dev = torch.device("cuda:0")
    ev = torch.cuda.Event()
    ev.record()  # (materialises the event behind the handle)
    plan = make_plan(_spec(), "bf16")
    _lib.check(_lib.load().reni_set_grad_ready_event(ev.cuda_event))
    try:
        got = _run(plan, B, W, dev)
    finally:
        _lib.check(_lib.load().reni_set_grad_ready_event(None))
    for x, y in zip(got, with_l0x[(B, W)]):
        assert torch.equal(x, y), (B, W)


def _engine(N, fused):
    from reni_amd.engine import TrainEngine
    from reni_amd.models import RENIAutoDecoder
    torch.manual_seed(0)
    m = RENIAutoDecoder(N, SPEC["ndims"], SPEC["eq"], SPEC["H"], SPEC["L"], 3, True, "tanh", 30.0, 30.0, False)
    m.set_compute_dtype("bf16").to("cuda:0")
    return m, TrainEngine(m, lr=1e-3, fused_step=fused)


def _data(N, W, dev):
    from reni_amd.utils import get_directions, get_sineweight
    D, S = get_directions(W).to(dev), get_sineweight(W).to(dev)
    T = torch.stack([torch.rand(D.shape[1], 3, generator=torch.Generator().manual_seed(500 + i)) * 2 - 1 for i in range(N)]).to(dev)
    return D, S, T


def _state(m, e):
    return [t.detach().clone() for t in (m._flat_params(), m.Z.data, e.m_dec, e.v_dec, e.m_lat, e.v_lat)]


@pytest.mark.parametrize("B,W", SHAPES)
def test_fused_step_is_bit_equal_to_the_two_calls_on_quad_row_partials(B, W):
    """Three training steps on quad-row partials with the fused call on (a staged prologue, k_adam2 behind the call's work) and off
    (the two calls it replaces): every buffer bit-equal, as tests/test_gpu_train_step.py asks of the flat layout."""
    dev = torch.device("cuda:0")
    N = 2 * B
    D, S, T = _data(N, W, dev)
    batches = [torch.arange(B, device=dev), torch.arange(B, device=dev) + B, torch.arange(B, device=dev)]
    res = {}
    for fused in (False, True):
        m, e = _engine(N, fused)
        assert e.plan.path_info(B, D.shape[1])["dw1_kernel"] == "k_reni_l0_ring"
        terms = []
        for k, idx in enumerate(batches):
            nxt = batches[k + 1] if k + 1 < len(batches) else None
            terms.append(e.step(idx, T[idx], S, D, next_idx=nxt).clone())
        torch.cuda.synchronize()
        res[fused] = (torch.stack(terms), _state(m, e), e)
    assert res[True][2]._stage is not None and res[False][2]._stage is None  # the fused path really ran
    assert bool(torch.isfinite(res[True][0]).all())
    assert torch.equal(res[False][0], res[True][0]), (res[False][0], res[True][0])
    for a, b, name in zip(res[False][1], res[True][1], ("params", "Z", "m_dec", "v_dec", "m_lat", "v_lat")):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


def test_a_skipped_step_leaves_the_parameters_alone_on_quad_row_partials():
    """A staged batch that is not the call's batch, on the path with quad-row partials: loss NaN, parameters, latents and moments
    exactly as they were -- the step is skipped -- and the next step runs."""
    dev = torch.device("cuda:0")
    B, N, W = 3, 9, 32
    D, S, T = _data(N, W, dev)
    m, e = _engine(N, True)
    idx = torch.arange(B, device=dev)
    nxt = torch.arange(B, device=dev) + B
    e.step(idx, T[idx], S, D, next_idx=nxt)
    before = _state(m, e)
    nxt[1] = N - 1  # the announced batch is changed in place behind the engine's back
    t = e.step(nxt, T[nxt], S, D)
    assert bool(torch.isnan(t).all())
    for a, b, name in zip(before, _state(m, e), ("params", "Z", "m_dec", "v_dec", "m_lat", "v_lat")):
        assert torch.equal(a, b), name
    t3 = e.step(idx, T[idx], S, D)
    assert bool(torch.isfinite(t3).all())
