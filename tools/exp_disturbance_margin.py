#!/usr/bin/env python3
"""Cost of the batched disturbance margin (upr_batch_disturbance_margin_plan) on one MI355X: the plan form on the headline handle
(pink_bottle, 21 knots, B = 1024, one cold solve) for n_scen in {1, 8, 45} and n_dir in {3, 6, 32}.
Per shape: device time of the launches (HIP events, BatchMPC.balance_ms: state kernel, job kernel, and for the reductions the plan
kernel), beside it the path_accel_margin_plan launch on the same handle in the same session (the yardstick: n_dir times its jobs with the
same decisions per job is the only expectation that can be derived) and the ratio, also per direction; least-squares solves per job,
mean and max; the shares of the classes; the radius over the plans and which direction binds.  Directions (tray frame): the span
directions of contact 0 and e_z (3), those and their negatives (6), and 32 unit linear directions on a sphere lattice.  Warm-up calls
first, then the median of `--reps` repetitions (of at most 5 for the reductions).  With --form-compare the one-body headline is also
timed on the wave form (UPR_BAL_FORM=0, a second handle).
    python tools/exp_disturbance_margin.py [--B 1024] [--reps 21] [--r-max 8] [--form-compare]"""
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


def directions(P, n):
    span = np.asarray(P.contact_span, dtype=np.float64)[0]
    base = np.stack([span[0], span[1], [0.0, 0.0, 1.0]])
    if n == 3:
        u = base
    elif n == 6:
        u = np.concatenate([base, -base])
    else:   # a Fibonacci lattice on the sphere
        k = np.arange(n) + 0.5
        z, th = 1.0 - 2.0 * k / n, np.pi * (1.0 + 5.0 ** 0.5) * k
        u = np.stack([np.sqrt(1.0 - z * z) * np.cos(th), np.sqrt(1.0 - z * z) * np.sin(th), z], axis=1)
    return np.concatenate([np.zeros((len(u), 3)), u], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--r-max", type=float, default=8.0)
    ap.add_argument("--form-compare", action="store_true")
    a = ap.parse_args()
    arrs = json.load(open(ROOT / "tests" / "golden" / "arrangements.json"))
    rows = []
    P = thing_problem(arrs["pink_bottle"])
    x0 = level_tray_states(a.B, seed=3)
    way = waypoints_for(P, x0)
    sweep = R.study_sweep(P.body_params, [0.02, 0.02, 0.03])
    rm = a.r_max
    for form in (("", "0") if a.form_compare else ("",)):
        if form:
            os.environ["UPR_BAL_FORM"] = form
        mpc = BatchMPC(P, a.B, way_p=way)
        os.environ.pop("UPR_BAL_FORM", None)
        mpc.set_observation(0.0, x0)
        mpc.advance()
        for ns in (1, 8, 45):
            prm = None if ns == 1 else sweep[:ns]
            pac_ms, (_, pit) = timed(lambda: mpc.path_accel_margin_plan(prm, d_max=rm, want_iters=True), mpc, a.reps)
            for nd in (3, 6, 32):
                dirs = directions(P, nd)
                ms, (r, it) = timed(lambda: mpc.disturbance_margin_plan(dirs, prm, r_max=rm, want_iters=True), mpc, a.reps)
                rms, (w, _, rad, bind) = timed(lambda: mpc.disturbance_margin_plan(dirs, prm, r_max=rm, window=True, radius=True), mpc, min(a.reps, 5))
                lo, hi = r[..., 0], r[..., 1]
                none = np.isinf(lo)
                open_lo, open_hi = lo == -rm, hi == rm
                zero_in = (lo <= 0) & (0 <= hi)
                bounded = ~none & ~open_lo & ~open_hi
                fin = np.isfinite(rad)
                rows.append(dict(shape="headline" + (" (wave form)" if form else ""), B=a.B, n_scen=ns, n_dir=nd, jobs=int(lo.size), disturb_device_ms=ms,
                                 pathacc_device_ms=pac_ms, ratio_to_pathacc=ms / pac_ms, ratio_per_direction=ms / pac_ms / nd, reductions_device_ms=rms,
                                 solves_mean=float(it.mean()), solves_max=int(it.max()), pathacc_solves_mean=float(pit.mean()), pathacc_solves_max=int(pit.max()),
                                 share_all=float((open_lo & open_hi).mean()), share_hi=float((open_lo & ~open_hi).mean()),
                                 share_lo=float((open_hi & ~open_lo).mean()), share_both=float((bounded & zero_in).mean()),
                                 share_window=float((bounded & ~zero_in).mean()), share_none=float(none.mean()),
                                 share_plans_radius_positive=float((rad > 0).mean()), share_plans_radius_minus_inf=float(np.isneginf(rad).mean()),
                                 radius_median_of_finite=float(np.median(rad[fin])) if fin.any() else None,
                                 binding_direction_counts=np.bincount(bind[..., 0].ravel(), minlength=nd).tolist(),
                                 window_is_consistent=bool(np.array_equal(np.minimum(-w[..., 0], w[..., 1]).min(axis=0), rad))))
                print("n_scen %d n_dir %d: %.2f ms, path_accel_margin_plan %.2f ms" % (ns, nd, ms, pac_ms), file=sys.stderr, flush=True)
        mpc.close()
    print(json.dumps(dict(rows=rows, reps=a.reps, r_max=rm)))


if __name__ == "__main__":
    main()
