#!/bin/bash
# A/B of the feedback gains on demand on ONE box: UPR_FB_FUSED unset (on demand) against UPR_FB_FUSED=1 (the QP kernel's exit writes
# the array with every advance, as before), alternating pairs in one call.  tools/ab_fb_on_demand.sh [pairs]
#   headline: bench.py --steps 200 --warmup 5 (value, ms_per_step, QP kernel ms)
#   closed loop: bench.py --only config5 / config5s (thrown ball, hard rows / with slacks): ms_per_tick -- the loop that reads the
#   policy every period
# A run that fails or overruns its limit ends the script.
set -o pipefail
export TMPDIR=/tmp
N=${1:-3}
line() { python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); k=d.get('kernel_ms',{}); print('$1', '$2', d.get('ms_per_step', d.get('ms_per_tick')), k.get('qp'))"; }
for r in $(seq $N); do for v in unset 1; do
  if [ $v = unset ]; then E="env -u UPR_FB_FUSED"; else E="env UPR_FB_FUSED=1"; fi
  $E timeout -k 10 300 python bench.py --gpus 1 --steps 200 --warmup 5 2>/dev/null | line headline $v || exit 1
done; done
for W in config5 config5s; do for r in $(seq $N); do for v in unset 1; do
  if [ $v = unset ]; then E="env -u UPR_FB_FUSED"; else E="env UPR_FB_FUSED=1"; fi
  $E timeout -k 10 300 python bench.py --gpus 1 --only $W 2>/dev/null | line $W $v || exit 1
done; done; done
