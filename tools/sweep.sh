#!/bin/bash
# ONE parameterised sweep instead of a script per experiment (rounds 1-3 left 37 of those; tools/README.md lists the
# command line that replaces each). Runs `bench.py` once per variant and repetition and prints one line per run.
#
#   tools/sweep.sh <tag> [--workload W] [--reps N] [--steps S] [--warmup W] [--field F] [--extra "bench args"] -- VARIANT [VARIANT ...]
#
#   VARIANT   a quoted, space-separated list of KEY=VALUE tunables (kvq_set_tunable keys). "" = no tunables.
#   --field   which record of the line to print: roofline (default) | roofline_quantise | sharded | value
#             (roofline_quantise and the two_phase part of sharded are records of a --full run: the sweep asks for one)
#   -> gpurun_out/<tag>/sweep.txt (+ one JSON line per run in gpurun_out/<tag>/runs.jsonl)
# Example:
#   tools/sweep.sh ring --workload llama3_8b_decode_attn_seq16k_b8 --reps 2 -- "" "attn_lds=0" "attn_stream_tpw=3"
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
TAG=${1:?usage: tools/sweep.sh <tag> [options] -- VARIANT ...}; shift
W=llama3_8b_mixed_seq16k; REPS=1; STEPS=30; WARM=5; FIELD=roofline; EXTRA=""
while [ $# -gt 0 ] && [ "$1" != "--" ]; do
  case "$1" in
    --workload) W=$2; shift 2;; --reps) REPS=$2; shift 2;; --steps) STEPS=$2; shift 2;; --warmup) WARM=$2; shift 2;;
    --field) FIELD=$2; shift 2;; --extra) EXTRA=$2; shift 2;; *) echo "unknown option $1" >&2; exit 2;;
  esac
done
[ "$1" = "--" ] && shift
case "$FIELD" in roofline_quantise|sharded) EXTRA="--full $EXTRA";; esac
[ $# -gt 0 ] || { echo "no variants" >&2; exit 2; }
O=gpurun_out/$TAG; mkdir -p $O
cat > $O/.fmt.py <<'PY'
import json, sys
field, rep, variant = sys.argv[1:4]
try:
    j = json.loads(sys.stdin.read())
except Exception:
    print(f"rep {rep} {variant!r:44s} FAILED")
    sys.exit(1)


def one(r):
    return f"{r['avg_launch_ms'] * 1e3:9.2f} us  frac {r['frac']:.4f}  {r['kernel'][:70]}"


if field == "roofline":
    out = one(j["roofline"])
elif field == "roofline_quantise":
    out = "  |  ".join(f"{k} {one(v)}" for k, v in j["roofline_quantise"].items())
elif field == "sharded":
    out = f"{j['ms_per_step']} ms/step  {j['value']} GB/s  {j.get('kernels')}" + (f"  two_phase {j['two_phase']['ms_per_step']} ms" if j.get("two_phase") else "")
else:
    out = f"{j['value']} {j['unit']}  {j['ms_per_step']} ms/step"
print(f"rep {rep} {variant!r:44s} {out}")
PY
failed=0
for rep in $(seq 1 $REPS); do
  for V in "$@"; do
    args=""
    for kv in $V; do args="$args --tunable $kv"; done
    line=$(timeout -k 10 400 python3 bench.py --workload $W --steps $STEPS --warmup $WARM $EXTRA $args 2>>$O/sweep.err | tail -1)
    echo "$line" >> $O/runs.jsonl
    echo "$line" | python3 $O/.fmt.py "$FIELD" "$rep" "$V" | tee -a $O/sweep.txt || failed=$((failed+1))
  done
done
rm -f $O/.fmt.py
exit $failed
