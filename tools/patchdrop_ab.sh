#!/bin/bash
# The existing bench routes of this tree against a checkout of its parent commit, with no PatchDropout attached anywhere:
# what tools/ema_ab.sh does (bench.py --config base and --config micro_k --batch 512 --graph, parent and tree alternating
# for ROUNDS rounds, the --dump-outputs files of the first round compared byte for byte), logged under this feature's name.
#
#   tools/patchdrop_ab.sh PARENT_DIR [LOG]        PARENT_DIR: the parent commit, checked out and built
#
# The log (default profiles/patchdrop_ab_bench.log) holds bench.py's JSON line of every run, the medians and spreads per
# route and side, and the verdict of the comparison.
HERE=$(cd "$(dirname "$0")/.." && pwd)
exec bash "$HERE/tools/ema_ab.sh" "${1:?usage: tools/patchdrop_ab.sh PARENT_DIR [LOG]}" "${2:-$HERE/profiles/patchdrop_ab_bench.log}"
