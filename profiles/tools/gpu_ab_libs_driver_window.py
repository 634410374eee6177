"""Same-box alternating A/B of two builds of the library in the DRIVER'S window: bench.py --gpus 1 --steps 20 --warmup 5, a fresh process
per run, A then B, PAIRS times (as gpu_ab_driver_window.sh does for an environment selector; here the library RENI_HIP_LIB names).
usage: python profiles/tools/gpu_ab_libs_driver_window.py PAIRS LIB_A LIB_B [bench arguments ...]
Prints every pair, then: pairs won by B (lower step time), the median of (A - B) and the median absolute deviation of A's own runs.
B counts as a gain only if it wins every pair and the median difference is at least three times A's MAD.
A run that fails, or ends on a signal, ends the whole comparison (nothing more is started on the device)."""
import json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pairs, libs, extra = int(sys.argv[1]), [os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3])], sys.argv[4:]


def run(lib):
    env = dict(os.environ, RENI_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"] + extra, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:])
        sys.exit(r.returncode if r.returncode > 0 else 128 - r.returncode)
    d = json.loads(r.stdout.strip().splitlines()[-1])
    return d["ms_per_step"] * 1e3, d["roofline"]["kernel_avg_ms"] * 1e3


a, b = [], []
for k in range(pairs):
    ra, rb = run(libs[0]), run(libs[1])
    a.append(ra); b.append(rb)
    print(f"pair {k + 1:2d}: A step {ra[0]:8.1f} us kernel {ra[1]:8.1f}   B step {rb[0]:8.1f} us kernel {rb[1]:8.1f}   A - B {ra[0] - rb[0]:+7.1f} us", flush=True)
sa, sb = [x[0] for x in a], [x[0] for x in b]
diff = [x - y for x, y in zip(sa, sb)]
med_a = statistics.median(sa)
mad_a = statistics.median(abs(x - med_a) for x in sa)
wins = sum(d > 0 for d in diff)
print(f"B wins {wins} of {pairs} pairs; median A {med_a:.1f} us, median B {statistics.median(sb):.1f} us, median (A - B) {statistics.median(diff):+.1f} us "
      f"({100 * statistics.median(diff) / med_a:+.2f} %), MAD of A {mad_a:.1f} us, min / max (A - B) {min(diff):+.1f} / {max(diff):+.1f}")
print("gain" if wins == pairs and statistics.median(diff) >= 3 * mad_a else "NOT a gain by the project's bar")
