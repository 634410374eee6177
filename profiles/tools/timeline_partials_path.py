"""The path of the weight-gradient partials through a config-2 step, from a rocprofv3 rocpd database (kernel trace of bench.py):
per step -- between two launches of the training kernel -- the durations of the training kernel, k_reni_l0_ring, k_tail_a, k_tail_b,
k_adam2, the span from the training kernel's end to the ring's start and the step itself; median and median absolute deviation over the
last N steps (default 20: the timed window).  usage: python profiles/tools/timeline_partials_path.py <results.db> [N]"""
import sqlite3, statistics, sys

c = sqlite3.connect(sys.argv[1])
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rows = c.execute("select name, start, end from kernels order by start").fetchall()
idx = [i for i, r in enumerate(rows) if "k_reni_train_bf16" in r[0]]
steps = list(zip(idx[:-1], idx[1:]))[-N:]
cols = {k: [] for k in ("step", "k_reni_train_bf16", "gap train->ring", "k_reni_l0_ring", "k_tail_a", "k_tail_b", "k_adam2")}
for a, b in steps:
    seg = rows[a:b]
    def first(sub):
        return next((r for r in seg if sub in r[0]), None)
    tr, ring = seg[0], first("k_reni_l0_ring")
    if ring is None:
        continue
    cols["step"].append((rows[b][1] - tr[1]) / 1e3)
    cols["k_reni_train_bf16"].append((tr[2] - tr[1]) / 1e3)
    cols["gap train->ring"].append((ring[1] - tr[2]) / 1e3)
    for k in ("k_reni_l0_ring", "k_tail_a", "k_tail_b", "k_adam2"):
        r = first(k)
        if r is not None:
            cols[k].append((r[2] - r[1]) / 1e3)
print(f"{len(cols['step'])} steps")
for k, v in cols.items():
    if v:
        med = statistics.median(v)
        mad = statistics.median(abs(x - med) for x in v)
        print(f"{k:20s} median {med:9.2f} us   MAD {mad:6.2f}   min {min(v):9.2f}   max {max(v):9.2f}")
