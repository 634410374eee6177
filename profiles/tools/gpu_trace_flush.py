"""Cycles the weight-gradient partial flush takes at the end of the config-2 kernels (wave 0 of workgroup 0, s_memtime).
usage: gpu_trace_flush.py train   -- a -DRENI_TRACE build: k_reni_train_bf16<.., L0X>, stamps 10 (before flush_layer) and 11 (its
                                     stores have left) in trace slots 510 / 511, behind the tile loop's stamps
       gpu_trace_flush.py ring    -- a -DRENI_TRACE_DW1 -DRENI_L0_NSLOT=3 build: k_reni_l0_ring, stamps 101 (loop end) and 102
The library is the one RENI_HIP_LIB names.  Five traced calls; prints every call's figures and the median."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from oracle import reni_oracle as O
from tests.util import flat_params, make_plan, random_problem

which = sys.argv[1] if len(sys.argv) > 1 else "train"
dev = torch.device("cuda:0")
spec = O.DecoderSpec(36, "SO2", 128, 5, 3, True, "tanh")
B = 64
params, Z, D, W, T = random_problem(spec, B, 0, seed=2, grid_w=256)
plan = make_plan(spec, "bf16")
assert plan.path_info(B, D.shape[1])["dw1_kernel"] == "k_reni_l0_ring"
fp = flat_params(spec, params).to(dev)
Zd, Dd, Td, Wd = Z.to(dev), D.to(dev), T.to(dev), W.to(dev)
tr = torch.zeros(1024, dtype=torch.int64, device=dev)
for _ in range(3):
    plan.forward_loss_backward(Zd, Dd, fp, Td, Wd)
torch.cuda.synchronize()
os.environ["RENI_TRACE_PTR"] = str(tr.data_ptr())
flush, whole = [], []
for rep in range(5):
    tr.zero_()
    plan.forward_loss_backward(Zd, Dd, fp, Td, Wd)
    torch.cuda.synchronize()
    ev = [((w >> 48) & 0xffff, w & ((1 << 48) - 1)) for w in tr.cpu().tolist() if w != 0]
    tags = {}
    for tag, clk in ev:
        tags.setdefault(tag, []).append(clk)
    a, b = (10, 11) if which == "train" else (101, 102)
    if a not in tags or b not in tags:
        print("no flush stamps in the trace: is this the right build?", sorted(tags))
        sys.exit(1)
    t0 = min(c for _, c in ev)
    flush.append(tags[b][-1] - tags[a][-1])
    whole.append(tags[b][-1] - t0)
    print(f"{which} call {rep}: flush {flush[-1]} cycles of {whole[-1]} traced ({100.0 * flush[-1] / whole[-1]:.2f} %)")
print(f"{which}: flush median {statistics.median(flush)} cycles, min {min(flush)} max {max(flush)}; traced span median {statistics.median(whole)}")
