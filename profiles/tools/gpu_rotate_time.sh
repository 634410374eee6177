#!/bin/bash
# usage: gpu_rotate_time.sh <out dir> [<parent tree>]  -- the rotation's measurements of DESIGN 4.6c, from the repository root:
# call times (device events), a kernel trace in a run of its own, and the resident fit's epoch with DATASET.ROTATE_AUGMENT on
# against off, alternating.  <parent tree>: a built checkout of the parent commit; "off" is then measured there as well.
# Every GPU step has its own time limit and the chain stops at the first step that fails.
set -u
OUT=$1; PARENT=${2:-}
T=profiles/tools/gpu_rotate_time.py
mkdir -p "$OUT"
DATA=$(mktemp -d /tmp/reni_rotate_XXXXXX)
trap 'rm -rf "$DATA" "$OUT/_kt"' EXIT
fit() { timeout -k 10 150 python3 $T fit "$DATA" "$@" >> "$OUT/rotate_fit.txt" 2>> "$OUT/rotate_fit.err"; }
trace() {  # kernel times of thirty calls of one shape, a run of its own
  timeout -k 10 180 rocprofv3 --kernel-trace --stats -d "$OUT/_kt" -o k -- python3 $T trace $1 > "$OUT/rotate_trace_$1.log" 2>&1 &&
  python3 profiles/summarize_rocpd.py "$OUT/_kt/k_results.db" "$OUT/rotate_kernel_stats_$1.md" > /dev/null && rm -rf "$OUT/_kt"
}
export TMPDIR=/tmp
python3 $T write "$DATA" > "$OUT/rotate_fit.txt" &&
timeout -k 10 120 python3 $T kernel > "$OUT/rotate_kernel.txt" 2> "$OUT/rotate_kernel.err" &&
trace 0 && trace 1 &&
for round in 1 2 3; do
  fit SO3 && fit && fit SO2 || exit 1
  if [ -n "$PARENT" ]; then fit --root "$PARENT" || exit 1; fi
done
