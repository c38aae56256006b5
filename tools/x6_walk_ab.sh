#!/bin/bash
# conv_x6's F(2,3) walk against the direct walk, per shape: tools/micro/conv_bench (build it first:
# tools/micro/build_conv_bench.sh) on the 3x3 / stride 1 shapes of the bench workload, DDMI_X6_WALK=0 and 2 alternating,
# REPS processes each; prints the per-shape table of profiles/x6_walk_ab.md. Stops at the first failing run.
#   tools/x6_walk_ab.sh [reps = 5] [shape filter = .3x3]   -> $DDMI_OUT/x6_walk_ab.log (default results/)
set -u
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"; O=${DDMI_OUT:-results}; mkdir -p "$O"
REPS=${1:-5}; FILT=${2:-.3x3}
: > "$O/x6_walk_ab.log"
for rep in $(seq 1 "$REPS"); do
  for w in 0 2; do
    echo "## rep $rep DDMI_X6_WALK=$w" >> "$O/x6_walk_ab.log"
    DDMI_X6_WALK=$w timeout -k 10 120 tools/micro/conv_bench 20 "$FILT" >> "$O/x6_walk_ab.log" 2>&1
    rc=$?; [ $rc -ne 0 ] && { echo "conv_bench rc=$rc (rep $rep, DDMI_X6_WALK=$w)"; tail -5 "$O/x6_walk_ab.log"; exit $rc; }
  done
done
python3 - "$O/x6_walk_ab.log" <<'PY'
import re, statistics as st, sys
d, mode = {}, None
for line in open(sys.argv[1]):
    m = re.match(r"## rep \d+ DDMI_X6_WALK=(\d)", line)
    if m:
        mode = m.group(1)
        continue
    p = line.split()
    if len(p) >= 7 and p[0] != "shape":
        d.setdefault(p[0], {}).setdefault(mode, []).append((float(p[1]), p[5], p[6]))
print("| shape | direct form | walk form | direct ms: median (min-max) | walk ms: median (min-max) | gain | slowest walk < fastest direct |")
print("|---|---|---|---|---|---|---|")
for k, v in d.items():
    a, b = [x[0] for x in v["0"]], [x[0] for x in v["2"]]
    print(f"| {k} | {v['0'][0][1]} | {v['2'][0][1]} {v['2'][0][2]} | {st.median(a):.4f} ({min(a):.4f}-{max(a):.4f}) | "
          f"{st.median(b):.4f} ({min(b):.4f}-{max(b):.4f}) | {100 * (1 - st.median(b) / st.median(a)):.1f} % | "
          f"{'yes' if max(b) < min(a) else 'no'} |")
PY
