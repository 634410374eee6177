"""One weight image per hidden layer for both passes of the L0X training instance (reni_dev_train.inc: wimg_cell, wimg_tr_base,
make_job; k_pack: PackDesc::swz): the backward step's dX GEMM reads W_l^T out of the forward image with transposing reads, the
images of layers L and L - 1 are still in their buffers when the backward pass needs them, and layer 2's is handed from a tile's
last step to the next tile's forward pass -- six copies per tile instead of nine at L = 5.

The fused forward / loss / backward call on that path against the generic kernels (RENI_NO_PERSIST=1, a fresh process: the
variable is read at plan creation), with the helpers of tests/test_gpu_partials_layout.py and the bf16 tolerances of
tests/test_gpu_parity.py (loss 2e-3 relative, gradients 3e-2 rel-L2: the two sides are different bf16 kernels).  A fragment read
from the wrong cell, an image that is not (or no longer) in its buffer, or a misplaced power of two is an error of order one in at
least one tensor.

Shapes: the smallest at which the image schedule can still go wrong (RENI_TRAIN_WG sets the number of workgroups):
    B = 1, P = 128                   one tile in all: first tile == last tile, nothing handed over
    B = 2, P = 256, 3 workgroups     ranges of 1, 1 and 2 tiles: the range of one tile (the second of them starts in the middle of an
                                     image) beside the shortest range that hands layer 2's image from one tile to the next
    B = 3, P = 384, 2 workgroups     ranges of 4 and 5 tiles (even and odd counts); image runs end inside both ranges, so the image is
                                     handed over across tile boundaries that are also image boundaries
each with L = 5 and with L = 3 (the L0X instance needs an odd L >= 3; at L = 3 no image is loaded in the backward pass at all)."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import reni_oracle as O
from tests.util import flat_params, make_plan, random_problem, unflatten

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (images, samples per image, workgroups of the training kernel or None, workgroups expected)
SHAPES = [(1, 128, None, 1), (2, 256, 3, 3), (3, 384, 2, 2)]
LAYERS = [5, 3]
CASES = [(B, P, wg, n, L) for L in LAYERS for (B, P, wg, n) in SHAPES]


def _spec(L):
    return O.DecoderSpec(36, "SO2", 128, L, 3, True, "tanh")


def _key(B, P, L):
    return "%dx%d_L%d" % (B, P, L)


def _run(plan, B, P, L, dev):
    spec = _spec(L)
    params, Z, D, Wt, T = random_problem(spec, B, P, seed=90 + 7 * B + L)
    fp = flat_params(spec, params).to(dev)
    lt, dZ, dp, _ = plan.forward_loss_backward(Z.to(dev), D.to(dev), fp, T.to(dev), Wt.expand(B, -1, 3).contiguous().to(dev))
    return lt.cpu().clone(), dZ.cpu().clone(), dp.cpu().clone()


def _plan_with_wg(L, wg):
    if wg is None:
        return make_plan(_spec(L), "bf16")
    os.environ["RENI_TRAIN_WG"] = str(wg)  # (read once, at plan creation)
    try:
        return make_plan(_spec(L), "bf16")
    finally:
        del os.environ["RENI_TRAIN_WG"]


_CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
from tests.test_gpu_shared_wimage import CASES, _key, _run, _spec
from tests.util import make_plan
dev = torch.device("cuda:0")
out = {{}}
for B, P, wg, n, L in CASES:
    plan = make_plan(_spec(L), "bf16")
    info = plan.path_info(B, P)
    assert not info["persistent_kernels"] and "RENI_NO_PERSIST" in info["env_overrides"], info
    out[_key(B, P, L)] = list(_run(plan, B, P, L, dev))
torch.save(out, {path!r})
"""


@pytest.fixture(scope="module")
def generic(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("no_persist") / "grads.pt")
    env = dict(os.environ, RENI_NO_PERSIST="1")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, path=path)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return torch.load(path)


@pytest.fixture(scope="module")
def shared():
    """(loss terms, dZ, dparams) of the L0X path per case, the same call made twice on one plan."""
    dev = torch.device("cuda:0")
    out = {}
    for B, P, wg, n, L in CASES:
        plan = _plan_with_wg(L, wg)
        info = plan.path_info(B, P)
        assert info["dw1_kernel"] == "k_reni_l0_ring" and info["workgroups"] == n, info   # the L0X instance, on the grid the case is about
        assert info["env_overrides"] == ([] if wg is None else ["RENI_TRAIN_WG"]), info
        out[_key(B, P, L)] = (_run(plan, B, P, L, dev), _run(plan, B, P, L, dev))
    return out


@pytest.mark.parametrize("B,P,wg,n,L", CASES)
def test_shared_image_path_against_the_generic_kernels(shared, generic, B, P, wg, n, L):
    spec = _spec(L)
    lt, dZ, dp = shared[_key(B, P, L)][0]
    lo, dZo, dpo = generic[_key(B, P, L)]
    assert torch.isfinite(lt).all() and torch.isfinite(dZ).all() and torch.isfinite(dp).all()
    e_loss = abs(float(lt[0]) - float(lo[0])) / abs(float(lo[0]))
    e_dz = O.rel_l2(dZ.numpy(), dZo.numpy())
    print("loss", e_loss, "dZ", e_dz)
    gp, gpo = unflatten(spec, dp), unflatten(spec, dpo)
    errs = {k: O.rel_l2(gp[k].numpy(), gpo[k].numpy()) for k in gp}
    for k, e in errs.items():
        print(k, e)
    assert e_loss <= 2e-3
    assert e_dz <= 3e-2
    for k, e in errs.items():
        assert e <= 3e-2, (k, e)


@pytest.mark.parametrize("B,P,wg,n,L", CASES)
def test_the_same_step_twice_gives_the_same_bits(shared, B, P, wg, n, L):
    """(the second call finds the buffers, the workspace images and the g_1 stream as the first left them)"""
    a, b = shared[_key(B, P, L)]
    for x, y, name in zip(a, b, ("loss terms", "dZ", "dparams")):
        assert torch.equal(x, y), name
