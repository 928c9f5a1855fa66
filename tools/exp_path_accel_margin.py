#!/usr/bin/env python3
"""Cost of the batched path-acceleration margin (upr_batch_path_accel_margin_plan / _points) on one MI355X, on the shapes of the speed
margin's cost table (tools/exp_speed_margin.py):
    headline      the plan form at B = 1024 (pink_bottle, 21 knots) for n_scen in {1, 8, 45}
    robust_8corner, blue_cups   the points form at 64 x 21 states, n_scen = 8
Per shape: device time of the launch (HIP events, BatchMPC.balance_ms), beside it the rho launch and the speed-margin launch of the same
jobs in the same session and the ratios, least-squares solves per job, mean and max, for both margins, and the shares of the classes
(all: -d_max and d_max accepted; hi: only -d_max; lo: only d_max; both: neither, 0 accepted; window: neither and not 0; none), of the
jobs balanced only while braking (d_hi < 0) and of those that cannot brake at all (d_lo = 0 to the grid).  The headline rows add the
window over the knots and the interval of the acceleration boxes.  Warm-up calls first, then the median of `--reps` repetitions.
With --form-compare the one-body headline is also timed on the wave form (UPR_BAL_FORM=0, a second handle).
    python tools/exp_path_accel_margin.py [--B 1024] [--reps 21] [--d-max 8] [--speed 1] [--form-compare]"""
import argparse
import json
import os
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


def row(shape, B, ns, d_max, rho_ms, speed, acc):
    sms, (_, sit) = speed
    ms, (d, it) = acc
    lo, hi = d[..., 0], d[..., 1]
    none = np.isinf(lo)
    open_lo, open_hi = lo == -d_max, hi == d_max
    zero_in = (lo <= 0) & (0 <= hi)
    bounded = ~none & ~open_lo & ~open_hi
    return dict(shape=shape, B=B, n_scen=ns, jobs=int(lo.size), rho_device_ms=rho_ms, speed_device_ms=sms, accel_device_ms=ms, ratio_to_rho=ms / rho_ms,
                ratio_to_speed=ms / sms, solves_mean=float(it.mean()), solves_max=int(it.max()), speed_solves_mean=float(sit.mean()), speed_solves_max=int(sit.max()),
                share_all=float((open_lo & open_hi).mean()), share_hi=float((open_lo & ~open_hi).mean()), share_lo=float((open_hi & ~open_lo).mean()),
                share_both=float((bounded & zero_in).mean()), share_window=float((bounded & ~zero_in).mean()), share_none=float(none.mean()),
                share_balanced_only_braking=float((~none & (hi < 0)).mean()), share_balanced_now=float((~none & zero_in).mean()),
                d_lo_median_of_balanced=float(np.median(lo[~none & zero_in])) if np.any(~none & zero_in) else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--d-max", type=float, default=8.0)
    ap.add_argument("--speed", type=float, default=1.0)
    ap.add_argument("--s-max", type=float, default=4.0)
    ap.add_argument("--form-compare", action="store_true")
    a = ap.parse_args()
    arrs = json.load(open(ROOT / "tests" / "golden" / "arrangements.json"))
    rows = []
    P = thing_problem(arrs["pink_bottle"])
    x0 = level_tray_states(a.B, seed=3)
    way = waypoints_for(P, x0)
    sweep = R.study_sweep(P.body_params, [0.02, 0.02, 0.03])
    kw = dict(d_max=a.d_max, speed=a.speed)
    for form in (("", "0") if a.form_compare else ("",)):
        if form:
            os.environ["UPR_BAL_FORM"] = form
        mpc = BatchMPC(P, a.B, way_p=way)
        os.environ.pop("UPR_BAL_FORM", None)
        mpc.set_observation(0.0, x0)
        mpc.advance()
        for ns in (1, 8, 45):
            prm = None if ns == 1 else sweep[:ns]
            rho_ms, _ = timed(lambda: mpc.balance_check_plan(prm), mpc, a.reps)
            spd = timed(lambda: mpc.speed_margin_plan(prm, s_max=a.s_max, want_iters=True), mpc, a.reps)
            r = row("headline" + (" (wave form)" if form else ""), a.B, ns, a.d_max, rho_ms, spd,
                    timed(lambda: mpc.path_accel_margin_plan(prm, want_iters=True, **kw), mpc, a.reps))
            wms, (w, _, lim) = timed(lambda: mpc.path_accel_margin_plan(prm, window=True, **kw), mpc, a.reps)
            ok = w[..., 0] <= w[..., 1]
            r.update(window_device_ms=wms, share_plans_with_a_window=float(ok.mean()), share_plans_balanced_as_planned=float((ok & (w[..., 0] <= 0) & (w[..., 1] >= 0)).mean()),
                     plan_d_lo_median=float(np.median(w[..., 0])), limit_lo_median=float(np.median(lim[:, 0])), limit_hi_median=float(np.median(lim[:, 1])),
                     share_limit_empty=float((lim[:, 0] > lim[:, 1]).mean()))
            rows.append(r)
        mpc.close()
    for name in ("robust_8corner", "blue_cups"):
        Pl = R.table_problem(arrs, name)
        kinds = (["inside" if Pl.nf == 3 else "lift", "outside", "down"] * 448)[:64 * 21]
        x = R.points(Pl, kinds, seed=5)
        prm = R.scenarios(Pl, np.random.default_rng(1), 8)
        h = BatchMPC(Pl, 1)
        rho_ms, _ = timed(lambda: h.balance_check(x, prm), h, a.reps)
        spd = timed(lambda: h.speed_margin(x, prm, s_max=a.s_max, want_iters=True), h, a.reps)
        rows.append(row(name, 64, 8, a.d_max, rho_ms, spd, timed(lambda: h.path_accel_margin(x, prm, want_iters=True, **kw), h, a.reps)))
        h.close()
    print(json.dumps(dict(rows=rows, reps=a.reps, d_max=a.d_max, speed=a.speed)))


if __name__ == "__main__":
    main()
