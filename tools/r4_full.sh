#!/bin/bash
# GPU pass: parity tests + the bench line as the driver runs it (extras and CPU baseline included)
export TMPDIR=/tmp
export OUT=${OUT:-out}
mkdir -p "$OUT"
timeout 1500 python -m pytest tests -m gpu -x -q > "$OUT"/r4_tests.log 2>&1; echo "tests rc $?" >> "$OUT"/r4_tests.log
tail -15 "$OUT"/r4_tests.log
timeout 600 python bench.py --full --steps 20 --warmup 5 > "$OUT"/r4_bench_full.json 2> "$OUT"/r4_bench_full.err; echo "bench rc $?"
python3 - <<'PY'
import json, os
d=json.loads(open(os.environ['OUT'] + '/r4_bench_full.json').read().strip().splitlines()[-1])
print({k:d[k] for k in ('value','ms_per_step','n_gpus')}, d['roofline'], d.get('cpu_baseline'), d['kernel_ms'])
for e in d.get('extra_workloads',[]):
    print(e['workload'][:60], {k:e.get(k) for k in ('value','ms_per_step','ms_per_tick','qp_converged_fraction','qp_iters_mean','qp_status_counts','value_converged_subset','qp_not_converged_fraction','note')}, (e.get('warm') or {}).get('value'), e['kernel_ms'])
PY
tail -3 "$OUT"/r4_bench_full.err
