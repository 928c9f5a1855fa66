#!/usr/bin/env python3
"""Cost of the batched friction margin (upr_batch_friction_margin_plan / _points) on one MI355X, on the shapes of the balance
check's cost table (tools/exp_balance_check.py):
    headline      the plan form at B = 1024 (pink_bottle, 21 knots) for n_scen in {1, 8, 45}
    robust_8corner, blue_cups   the points form at 64 x 21 states, n_scen = 8
Per shape: device time of the margin launch (HIP events, BatchMPC.balance_ms), beside it the rho launch of the same jobs
(balance_check_plan / balance_check; run the tool on the parent commit with --rho-only for the yardstick of that library), their
ratio, evaluations per job (1 for kappa* = 0; 2 for +inf, 1 without friction; 34 for a finite kappa*) and least-squares solves per
job, mean and max, and the shares of the classes.  Warm-up calls first, then the median of `--reps` repetitions.
    python tools/exp_friction_margin.py [--B 1024] [--reps 21] [--kappa-max 8] [--rho-only]"""
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


def row(shape, B, ns, nf, rho_ms, margin):
    out = dict(shape=shape, B=B, n_scen=ns, rho_device_ms=rho_ms)
    if margin is not None:
        ms, (hi, it) = margin
        fin = np.isfinite(hi) & (hi > 0)
        ev = np.where(hi == 0, 1, np.where(fin, 34, 2 if nf == 3 else 1))
        out.update(jobs=int(hi.size), margin_device_ms=ms, ratio=ms / rho_ms, evaluations_mean=float(ev.mean()), evaluations_max=int(ev.max()),
                   solves_mean=float(it.mean()), solves_max=int(it.max()), share_zero=float((hi == 0).mean()), share_finite=float(fin.mean()),
                   share_below_one=float((fin & (hi < 1)).mean()), share_inf=float(np.isinf(hi).mean()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--kappa-max", type=float, default=8.0)
    ap.add_argument("--rho-only", action="store_true")
    a = ap.parse_args()
    arrs = json.load(open(ROOT / "tests" / "golden" / "arrangements.json"))
    rows = []
    P = thing_problem(arrs["pink_bottle"])
    x0 = level_tray_states(a.B, seed=3)
    mpc = BatchMPC(P, a.B, way_p=waypoints_for(P, x0))
    mpc.set_observation(0.0, x0)
    mpc.advance()
    sweep = R.study_sweep(P.body_params, [0.02, 0.02, 0.03])
    for ns in (1, 8, 45):
        prm = None if ns == 1 else sweep[:ns]
        rho_ms, _ = timed(lambda: mpc.balance_check_plan(prm), mpc, a.reps)
        mar = None if a.rho_only else timed(lambda: mpc.friction_margin_plan(prm, kappa_max=a.kappa_max, want_iters=True), mpc, a.reps)
        rows.append(row("headline", a.B, ns, P.nf, rho_ms, mar))
    mpc.close()
    for name in ("robust_8corner", "blue_cups"):
        Pl = R.table_problem(arrs, name)
        kinds = (["inside" if Pl.nf == 3 else "lift", "outside", "down"] * 448)[:64 * 21]
        x = R.points(Pl, kinds, seed=5)
        prm = R.scenarios(Pl, np.random.default_rng(1), 8)
        h = BatchMPC(Pl, 1)
        rho_ms, _ = timed(lambda: h.balance_check(x, prm), h, a.reps)
        mar = None if a.rho_only else timed(lambda: h.friction_margin(x, prm, kappa_max=a.kappa_max, want_iters=True), h, a.reps)
        rows.append(row(name, 64, 8, Pl.nf, rho_ms, mar))
        h.close()
    print(json.dumps(dict(rows=rows, reps=a.reps, kappa_max=a.kappa_max)))


if __name__ == "__main__":
    main()
