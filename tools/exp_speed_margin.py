#!/usr/bin/env python3
"""Cost of the batched speed margin (upr_batch_speed_margin_plan / _points) on one MI355X, on the shapes of the friction margin's cost
table (tools/exp_friction_margin.py):
    headline      the plan form at B = 1024 (pink_bottle, 21 knots) for n_scen in {1, 8, 45}
    robust_8corner, blue_cups   the points form at 64 x 21 states, n_scen = 8
Per shape: device time of the speed launch (HIP events, BatchMPC.balance_ms), beside it the rho launch of the same jobs in the same
session (balance_check_plan / balance_check) and their ratio, least-squares solves per job, mean and max, the shares of the classes
(all: rest and s_max accepted; upper: rest accepted; window: rest rejected, some speed accepted; none) and an ESTIMATE of the
evaluations per job, implied by the class and not counted by the kernel (2 for all, 2 + 32 for upper, 3 + 32 for none; a window job
seeded by the nominal speed takes 3 + 30 + 32 with s_max = 4, which is the figure used for every window job: one seeded by the descent
search takes up to 3 + 3 * 32, so for windows the figure is a lower bound).  The headline rows
add the window over the knots and the limit speed.  Warm-up calls first, then the median of `--reps` repetitions.
    python tools/exp_speed_margin.py [--B 1024] [--reps 21] [--s-max 4]"""
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


def row(shape, B, ns, s_max, rho_ms, speed):
    ms, (s, it) = speed
    lo, hi = s[..., 0], s[..., 1]
    none = np.isinf(lo)
    rest = lo == 0
    cls_all = rest & (hi == s_max)
    upper = rest & ~cls_all
    window = ~rest & ~none
    ev = np.where(cls_all, 2, np.where(upper, 34, np.where(none, 35, 65)))
    return dict(shape=shape, B=B, n_scen=ns, jobs=int(lo.size), rho_device_ms=rho_ms, speed_device_ms=ms, ratio=ms / rho_ms,
                evaluations_implied_by_class_mean=float(ev.mean()), evaluations_implied_by_class_max=int(ev.max()), solves_mean=float(it.mean()), solves_max=int(it.max()),
                share_all=float(cls_all.mean()), share_upper=float(upper.mean()), share_upper_below_one=float((upper & (hi < 1)).mean()),
                share_window=float(window.mean()), share_none=float(none.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--s-max", type=float, default=4.0)
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
        r = row("headline", a.B, ns, a.s_max, rho_ms, timed(lambda: mpc.speed_margin_plan(prm, s_max=a.s_max, want_iters=True), mpc, a.reps))
        wms, (w, _, lim) = timed(lambda: mpc.speed_margin_plan(prm, s_max=a.s_max, window=True), mpc, a.reps)
        ok = w[..., 0] <= w[..., 1]
        r.update(window_device_ms=wms, share_plans_with_a_window=float(ok.mean()), share_plans_balanced_as_planned=float((ok & (w[..., 0] <= 1) & (w[..., 1] >= 1)).mean()),
                 plan_s_hi_median=float(np.median(w[..., 1])), limit_speed_min=float(lim.min()), limit_speed_median=float(np.median(lim)))
        rows.append(r)
    mpc.close()
    for name in ("robust_8corner", "blue_cups"):
        Pl = R.table_problem(arrs, name)
        kinds = (["inside" if Pl.nf == 3 else "lift", "outside", "down"] * 448)[:64 * 21]
        x = R.points(Pl, kinds, seed=5)
        prm = R.scenarios(Pl, np.random.default_rng(1), 8)
        h = BatchMPC(Pl, 1)
        rho_ms, _ = timed(lambda: h.balance_check(x, prm), h, a.reps)
        rows.append(row(name, 64, 8, a.s_max, rho_ms, timed(lambda: h.speed_margin(x, prm, s_max=a.s_max, want_iters=True), h, a.reps)))
        h.close()
    print(json.dumps(dict(rows=rows, reps=a.reps, s_max=a.s_max)))


if __name__ == "__main__":
    main()
