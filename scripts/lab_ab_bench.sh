#!/bin/bash
# Same-box alternating A/B of bench.py: scripts/lab_ab_bench.sh product build_lab/libpn2ops_x.so ... -- every library in turn,
# LAB_AB_ROUNDS times over (default 2), one line per run: clouds/s, ms per step, verified. Each run has a time limit of its own
# and the first run that fails ends the script: nothing more is started on a GPU that a run has faulted or hung.
set -o pipefail
for i in $(seq "${LAB_AB_ROUNDS:-2}"); do for lib in "$@"; do [ "$lib" = product ] && lib=""; echo -n "${lib:-product} : "; PN2OPS_LIBRARY=${lib:+$PWD/$lib} timeout -k 10 "${LAB_AB_TIMEOUT:-300}" python bench.py --no-extras --no-cpu-baseline --steps 2000 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.readline()); print(round(d[\"value\"]), d[\"ms_per_step\"], d[\"verified\"])" || { echo "run failed: stopping"; exit 1; }; done; done
