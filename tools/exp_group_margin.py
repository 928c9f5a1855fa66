#!/usr/bin/env python3
"""Cost of the friction margin per contact group (upr_batch_friction_margin_groups_points / _plan) on one MI355X:
    foam_die2, box_arch   groups by pair of objects, the points form at 64 x 21 states, n_scen = 8
    fixture_box           bottom / walls, the plan form at B = 1024 (21 knots), n_scen = 8; the plan call with `worst` only beside
                          the call that downloads kappa_hi of every knot (wall time of the call, copies included)
Per shape: device time of the group launch (HIP events, BatchMPC.balance_ms), beside it the common-margin launch of the same (state,
scenario) jobs, their ratio (the expectation is n_grp: every group is a job of its own), evaluations per (job, group) (1 for
kappa* = 0; 2 for +inf; 34 for a finite kappa*) and least-squares solves, mean and max, and the shares of the classes.  Warm-up calls
first, then the median of `--reps` repetitions.  --common-only runs the common-margin launches alone and uses no entry newer than
the friction margin; with --root it imports the package of another checkout (the yardstick of that library in the same session).
    python tools/exp_group_margin.py [--B 1024] [--reps 21] [--kappa-max 8] [--common-only] [--root DIR]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np


def timed(call, mpc, reps):
    for _ in range(3):
        out = call()
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(mpc.balance_ms())
    return float(np.median(dev)), float(np.median(wall)), out


def stats(hi, it):
    fin = np.isfinite(hi) & (hi > 0)
    ev = np.where(hi == 0, 1, np.where(fin, 34, 2))
    return dict(evaluations_mean=float(ev.mean()), evaluations_max=int(ev.max()), solves_mean=float(it.mean()), solves_max=int(it.max()),
                share_zero=float((hi == 0).mean()), share_finite=float(fin.mean()), share_inf=float(np.isinf(hi).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--kappa-max", type=float, default=8.0)
    ap.add_argument("--common-only", action="store_true")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    a = ap.parse_args()
    root = Path(a.root).resolve()
    sys.path.insert(0, str(root))
    sys.path.insert(0, str(root / "tests"))
    import balance_ref as R
    from upright_amd.engine import BatchMPC
    from upright_amd.problem import thing_problem
    from upright_amd.sampling import level_tray_states, waypoints_for

    arrs = json.load(open(root / "tests" / "golden" / "arrangements.json"))
    km = a.kappa_max
    rows = []
    for name in ("foam_die2", "box_arch"):
        P = R.table_problem(arrs, name)
        kinds = (["inside", "lift", "down"] * 448)[:64 * 21]
        x = R.points(P, kinds, seed=5)
        prm = R.scenarios(P, np.random.default_rng(1), 8)
        h = BatchMPC(P, 1)
        ms, _, (hi, it) = timed(lambda: h.friction_margin(x, prm, kappa_max=km, want_iters=True), h, a.reps)
        r = dict(shape=name, jobs=int(hi.size), common_device_ms=ms, common=stats(hi, it))
        if not a.common_only:
            lab = h.contact_groups()
            gms, _, (ghi, git) = timed(lambda: h.friction_margin(x, prm, kappa_max=km, want_iters=True, groups=lab), h, a.reps)
            r.update(n_grp=int(lab.max() + 1), group_device_ms=gms, ratio=gms / ms, group=stats(ghi, git),
                     per_group_median_finite=[float(np.median(ghi[..., g][np.isfinite(ghi[..., g]) & (ghi[..., g] > 0)])) if
                                              (np.isfinite(ghi[..., g]) & (ghi[..., g] > 0)).any() else None for g in range(ghi.shape[-1])])
        rows.append(r)
        h.close()
    P = thing_problem(arrs["simulation_box_with_fixture"])
    x0 = level_tray_states(a.B, seed=3)
    mpc = BatchMPC(P, a.B, way_p=waypoints_for(P, x0))
    mpc.set_observation(0.0, x0)
    mpc.advance()
    prm = R.scenarios(P, np.random.default_rng(1), 8)
    ms, wall, (hi, it) = timed(lambda: mpc.friction_margin_plan(prm, kappa_max=km, want_iters=True), mpc, a.reps)
    r = dict(shape="fixture_box plan", B=a.B, jobs=int(hi.size), common_device_ms=ms, common_wall_ms=wall, common=stats(hi, it))
    if not a.common_only:
        grp = [[0, 1, 2, 3], [4, 5, 6, 7]]
        gms, gwall, (ghi, git) = timed(lambda: mpc.friction_margin_plan(prm, kappa_max=km, want_iters=True, groups=grp), mpc, a.reps)
        fms, fwall, _ = timed(lambda: mpc.friction_margin_plan(prm, kappa_max=km, groups=grp), mpc, a.reps)
        wms, wwall, (w, kn) = timed(lambda: mpc.friction_margin_plan(prm, kappa_max=km, groups=grp, worst=True), mpc, a.reps)
        assert np.array_equal(w, ghi.max(axis=1)) and np.array_equal(kn, ghi.argmax(axis=1))
        r.update(n_grp=2, group_device_ms=gms, ratio=gms / ms, group=stats(ghi, git), full_download_device_ms=fms, full_download_wall_ms=fwall,
                 worst_only_device_ms=wms, worst_only_wall_ms=wwall, worst_finite_share=float(np.isfinite(w).mean()),
                 worst_by_group=[float(np.max(w[..., g][np.isfinite(w[..., g])])) for g in range(2)])
    rows.append(r)
    mpc.close()
    print(json.dumps(dict(rows=rows, reps=a.reps, kappa_max=km, common_only=a.common_only)))


if __name__ == "__main__":
    main()
