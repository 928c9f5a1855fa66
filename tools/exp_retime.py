#!/usr/bin/env python3
"""Cost of the retiming on a speed lattice (upr_batch_retime_plan) on one MI355X: the plan form at the headline B = 1024 (pink_bottle, 21
knots, one cold solve) for n_scen in {1, 8, 45} and lattices of M in {8, 16, 32} speeds, linspace(0, 1.5, M).  Per row: device time of
the launches (HIP events, BatchMPC.balance_ms: state kernel, mask kernel, path kernel), beside it the path_accel_margin_plan launch on the
same handle in the same session and the ratio; least-squares solves per (instance, scenario, segment, level) job, mean and max (a job runs
at most 2 M projections); the share of set mask bits; the share of plans with a time law, their median duration against
N h, and the same with common=True and end at rest for n_scen > 1.  Warm-up calls first, then the median of `--reps` repetitions.
    python tools/exp_retime.py [--B 1024] [--reps 21] [--levels 8 16 32] [--scenarios 1 8 45]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import balance_ref as R  # noqa: E402
from upright_amd.engine import BatchMPC  # noqa: E402
from upright_amd.problem import thing_problem  # noqa: E402
from upright_amd.sampling import level_tray_states, waypoints_for  # noqa: E402


def timed(call, mpc, reps):
    for _ in range(3):
        out = call()
    dev = []
    for _ in range(reps):
        out = call()
        dev.append(mpc.balance_ms())
    return float(np.median(dev)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--levels", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--scenarios", type=int, nargs="+", default=[1, 8, 45])
    a = ap.parse_args()
    arrs = json.load(open(ROOT / "tests" / "golden" / "arrangements.json"))
    P = thing_problem(arrs["pink_bottle"])
    x0 = level_tray_states(a.B, seed=3)
    mpc = BatchMPC(P, a.B, way_p=waypoints_for(P, x0))
    mpc.set_observation(0.0, x0)
    mpc.advance()
    sweep = R.study_sweep(P.body_params, [0.02, 0.02, 0.03])
    plan_s = P.N * float(P.dt)
    rows = []
    for ns in a.scenarios:
        prm = None if ns == 1 else sweep[:ns]
        pac_ms, _ = timed(lambda: mpc.path_accel_margin_plan(prm, want_iters=True), mpc, a.reps)
        for M in a.levels:
            speeds = np.linspace(0.0, 1.5, M)
            ms, (dur, level, edges, iters) = timed(lambda: mpc.retime_plan(speeds, prm, want_edges=True, want_iters=True), mpc, a.reps)
            fin = np.isfinite(dur)
            bits = np.unpackbits(edges.view(np.uint8)).sum()
            r = dict(B=a.B, n_scen=ns, M=M, jobs=int(edges.size), retime_device_ms=ms, pathacc_device_ms=pac_ms,
                     ratio_to_pathacc=ms / pac_ms, solves_mean=float(iters.mean()), solves_max=int(iters.max()), share_bits_set=float(bits) / (edges.size * M),
                     share_plans_with_a_law=float(fin.mean()), median_duration_over_plan=float(np.median(dur[fin]) / plan_s) if fin.any() else None)
            if ns > 1:
                cms, (cdur, _) = timed(lambda: mpc.retime_plan(speeds, prm, common=True, end=0.0), mpc, a.reps)
                cf = np.isfinite(cdur)
                r.update(common_to_rest_device_ms=cms, share_plans_with_a_common_law_to_rest=float(cf.mean()),
                         median_common_duration_over_plan=float(np.median(cdur[cf]) / plan_s) if cf.any() else None)
            rows.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    mpc.close()
    print(json.dumps(dict(rows=rows, reps=a.reps)))


if __name__ == "__main__":
    main()
