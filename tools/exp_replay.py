#!/usr/bin/env python3
"""Cost of the replay of a time law on a clock (upr_batch_replay_plan) on one MI355X: the headline B = 1024 (pink_bottle, 21 knots, the plan
of one cold SQP iteration), the uniform law at speed 1, a tick that gives K in {21, 201, 2001} samples per plan, n_scen in {1, 8}.  Per row:
device time of the launches (HIP events, BatchMPC.balance_ms: sampler, state kernel on the B K sample states, job kernel, reduction) of the
full call and of the call that asks for the reductions alone, and the yardstick: balance_check (the points entry: state kernel and job kernel
on B K uploaded states) on the very states the call returned, same handle, same session.  The one expectation written down in advance is
derived: the projections are the same jobs, so the job launch should cost about what the yardstick's does; what the sampler and the
reduction add is reported, not targeted.  Also: the share of rejected samples and the least-squares solves per job, which the yardstick
must reproduce.  Warm-up calls first, then the median of `--reps` repetitions.
    python tools/exp_replay.py [--B 1024] [--reps 21] [--samples 21 201 2001] [--scenarios 1 8]"""
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
    ap.add_argument("--samples", type=int, nargs="+", default=[21, 201, 2001])
    ap.add_argument("--scenarios", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args()
    arrs = json.load(open(ROOT / "tests" / "golden" / "arrangements.json"))
    P = thing_problem(arrs["pink_bottle"])
    x0 = level_tray_states(a.B, seed=3)
    mpc = BatchMPC(P, a.B, way_p=waypoints_for(P, x0))
    mpc.set_observation(0.0, x0)
    mpc.advance()
    sweep = R.study_sweep(P.body_params, [0.02, 0.02, 0.03])
    speeds, level = np.array([1.0]), np.zeros((a.B, P.N + 1), dtype=np.int32)
    duration = P.N * float(P.dt)
    rows = []
    for ns in a.scenarios:
        prm = np.asarray(P.body_params)[None] if ns == 1 else sweep[:ns]
        for K in a.samples:
            tick = duration / (K - 1) * (1.0 - 1e-12)    # (the last sample just inside the duration)
            ms, (t, x, excess, iters) = timed(lambda: mpc.replay_plan(level, speeds, tick, prm, n_samples=K, want_iters=True), mpc, a.reps)
            ms_red, (_, count, worst, verdict, _) = timed(lambda: mpc.replay_plan(level, speeds, tick, prm, n_samples=K, reductions=True), mpc, a.reps)
            pts = np.ascontiguousarray(x.reshape(-1, x.shape[-1]))
            ms_pts, (rho, it_pts) = timed(lambda: mpc.balance_check(pts, prm, want_iters=True), mpc, a.reps)
            r = dict(B=a.B, n_scen=ns, K=K, jobs=int(excess.size), all_samples_exist=bool((count == K).all()), replay_device_ms=ms,
                     replay_reductions_device_ms=ms_red, balance_check_device_ms=ms_pts, ratio_to_balance_check=ms / ms_pts,
                     share_rejected=float((excess > 1e-8).mean()), plans_with_a_rejected_sample=float((verdict[..., 2] > 0).any(axis=1).mean()),
                     solves_mean=float(iters.mean()), same_solves_as_balance_check=bool(np.array_equal(iters.reshape(it_pts.shape), it_pts)),
                     worst_excess=float(np.nanmax(worst)))
            rows.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    mpc.close()
    print(json.dumps(dict(rows=rows, reps=a.reps)))


if __name__ == "__main__":
    main()
