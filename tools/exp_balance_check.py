#!/usr/bin/env python3
"""Cost of the batched balance check (upr_batch_balance_plan / upr_batch_balance_points) on one MI355X:
    headline      the plan form at B = 1024 (pink_bottle, 21 knots) for n_scen in {1, 8, 45}: device time of the two launches (HIP
                  events around them, BatchMPC.balance_ms), wall time of the call (copies and the synchronisation included), jobs per
                  second, mean and largest iteration count
    robust_8corner, blue_cups   the points form at B = 64 states x 21 knots of a stationary plan pushed sideways, n_scen = 8
    reference     jobs per second of tests/balance_ref.py (the oracle's b and A, scipy's nnls) on one host thread, 1000-job sample
Warm-up calls first, then the median of `--reps` repetitions.
    python tools/exp_balance_check.py [--B 1024] [--reps 21] [--ref-jobs 1000]"""
import argparse
import json
import sys
import time
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
    dev, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        out = call()
        wall.append(1e3 * (time.perf_counter() - t))
        dev.append(mpc.balance_ms())
    return float(np.median(dev)), float(np.median(wall)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--ref-jobs", type=int, default=1000)
    a = ap.parse_args()
    arrs = json.load(open(ROOT / "tests" / "golden" / "arrangements.json"))
    rows = []
    # headline: one cold solve, then the plan form
    P = thing_problem(arrs["pink_bottle"])
    x0 = level_tray_states(a.B, seed=3)
    mpc = BatchMPC(P, a.B, way_p=waypoints_for(P, x0))
    mpc.set_observation(0.0, x0)
    mpc.advance()
    sweep = R.study_sweep(P.body_params, [0.02, 0.02, 0.03])
    for ns in (1, 8, 45):
        prm = None if ns == 1 else sweep[:ns]
        dev, wall, (rho, it) = timed(lambda: mpc.balance_check_plan(prm, want_iters=True), mpc, a.reps)
        jobs = rho.size
        rows.append(dict(shape="headline", B=a.B, n_scen=ns, jobs=jobs, device_ms=dev, wall_ms=wall, jobs_per_s_device=jobs / dev * 1e3,
                         iters_mean=float(it.mean()), iters_max=int(it.max()), outside_fraction=float((rho > 1e-6).mean())))
    _, xs, _ = mpc.solution()
    mpc.close()
    # the reference on one host thread
    rng = np.random.default_rng(0)
    pick = [(int(b), int(k), int(s)) for b, k, s in zip(rng.integers(0, a.B, a.ref_jobs), rng.integers(0, P.N + 1, a.ref_jobs), rng.integers(0, 45, a.ref_jobs))]
    t = time.perf_counter()
    for b, k, s in pick:
        R.reference(P, xs[b, k], sweep[s:s + 1], False)
    ref_s = time.perf_counter() - t
    # the large shapes, points form
    for name in ("robust_8corner", "blue_cups"):
        Pl = R.table_problem(arrs, name)
        kinds = (["inside" if Pl.nf == 3 else "lift", "outside", "down"] * 448)[:64 * 21]
        x = R.points(Pl, kinds, seed=5)
        prm = R.scenarios(Pl, np.random.default_rng(1), 8)
        h = BatchMPC(Pl, 1)
        dev, wall, (rho, it) = timed(lambda: h.balance_check(x, prm, want_iters=True), h, a.reps)
        rows.append(dict(shape=name, B=64, n_scen=8, jobs=rho.size, device_ms=dev, wall_ms=wall, jobs_per_s_device=rho.size / dev * 1e3,
                         iters_mean=float(it.mean()), iters_max=int(it.max()), outside_fraction=float((rho > 1e-6).mean())))
        h.close()
    print(json.dumps(dict(rows=rows, reference_jobs=a.ref_jobs, reference_jobs_per_s=a.ref_jobs / ref_s, reps=a.reps)))


if __name__ == "__main__":
    main()
