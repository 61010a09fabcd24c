#!/bin/bash
# The existing bench routes of this tree against a checkout of its parent commit, with no EMA attached anywhere:
#   bench.py --config base            and            bench.py --config micro_k --batch 512 --graph
# alternating parent, tree, parent, tree, ... for ROUNDS rounds (one fresh process per run, each under its own timeout; the
# first failure ends the script), then the --dump-outputs files of the first round compared byte for byte.
#
#   tools/ema_ab.sh PARENT_DIR [LOG]        PARENT_DIR: the parent commit, checked out and built (git worktree + make)
#
# The log (default profiles/ema_ab_bench.log) holds bench.py's JSON line of every run, the medians per route and side, and
# the verdict of the comparison.
set -o pipefail
PARENT=${1:?usage: tools/ema_ab.sh PARENT_DIR [LOG]}
HERE=$(cd "$(dirname "$0")/.." && pwd)
LOG=${2:-$HERE/profiles/ema_ab_bench.log}
ROUNDS=${ROUNDS:-3}
STEPS=${STEPS:-30}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir -p "$(dirname "$LOG")"
: > "$LOG"

run() {  # side dir route round args...
  local side=$1 dir=$2 route=$3 round=$4
  shift 4
  local dump=()
  [ "$round" = 1 ] && dump=(--dump-outputs "$TMP/$side.$route")
  local line
  line=$(cd "$dir" && timeout -k 10 300 python bench.py --gpus 1 --steps "$STEPS" --warmup 5 "$@" "${dump[@]}" 2>"$TMP/err" | grep '^{' | tail -1)
  local rc=$?
  if [ $rc -ne 0 ] || [ -z "$line" ]; then
    echo "$route $side round $round: FAILED (exit $rc)" | tee -a "$LOG"
    tail -20 "$TMP/err" | tee -a "$LOG"
    exit 1
  fi
  echo "$route $side round $round: $line" | tee -a "$LOG"
}

for round in $(seq 1 "$ROUNDS"); do
  for side in parent tree; do
    dir=$PARENT
    [ "$side" = tree ] && dir=$HERE
    run "$side" "$dir" base "$round" --config base || exit 1
    run "$side" "$dir" micro_k_graph "$round" --config micro_k --batch 512 --graph || exit 1
  done
done

python - "$LOG" "$TMP" <<'EOF' | tee -a "$LOG"
import json, os, re, statistics, sys
import numpy as np
log, tmp = sys.argv[1], sys.argv[2]
ms = {}
for ln in open(log):
    m = re.match(r"(\w+) (parent|tree) round \d+: (\{.*\})", ln)
    if m:
        ms.setdefault((m.group(1), m.group(2)), []).append(json.loads(m.group(3))["ms_per_step"])
ok = True
for route in sorted({r for r, _ in ms}):
    med = {s: statistics.median(ms[(route, s)]) for s in ("parent", "tree")}
    spread = {s: (max(ms[(route, s)]) - min(ms[(route, s)])) / med[s] for s in med}
    print(f"{route}: median ms/step parent {med['parent']:.4f} (spread {spread['parent']:.4f}) tree {med['tree']:.4f} "
          f"(spread {spread['tree']:.4f}) tree/parent {med['tree'] / med['parent']:.4f}")
    a, b = os.path.join(tmp, "parent." + route), os.path.join(tmp, "tree." + route)
    names = sorted(os.listdir(a))
    same = names == sorted(os.listdir(b)) and all(
        open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read() for n in names)
    print(f"{route}: --dump-outputs {len(names)} files {'bit-identical' if same else 'DIFFER'}")
    ok = ok and same and len(names) > 0
sys.exit(0 if ok else 1)
EOF
