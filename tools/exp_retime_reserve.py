#!/usr/bin/env python3
"""Cost of the retiming with a reserve (upr_batch_retime_plan_reserve) on one MI355X: the plan form at the headline B = 1024 (pink_bottle,
21 knots, one cold solve) for n_scen in {1, 8}, lattices of M in {8, 16} speeds, linspace(0, 1.5, M), n_dir in {1, 3} tray-frame
directions (e_z; span_0, span_1, e_z of contact 0) and the reserve 0.25.  Per row: device time of the launches (HIP events,
BatchMPC.balance_ms: state kernel, mask kernel, path kernel) of this call and of retime_plan on the same handle in the same session, and
the ratio; least-squares solves per (instance, scenario, segment, level) job of both, mean and max (a job here runs at most 2 M (1 + 2
n_dir) projections); the share of set mask bits and of plans with a time law, both calls.  The one expectation written down in advance is
the derived bound on the solves: (1 + 2 n_dir) times the projections retime_plan spends on its ACCEPTED end states, and the same cost as
retime_plan for rejected nominal states -- so the ratio of solves lies in [1, 1 + 2 n_dir].  No target ratio is set.  Warm-up calls
first, then the median of `--reps` repetitions.
    python tools/exp_retime_reserve.py [--B 1024] [--reps 21] [--levels 8 16] [--scenarios 1 8] [--dirs 1 3] [--reserve 0.25]"""
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


def summary(dur, edges, iters, M):
    bits = np.unpackbits(edges.view(np.uint8)).sum()
    return dict(solves_mean=float(iters.mean()), solves_max=int(iters.max()), share_bits_set=float(bits) / (edges.size * M),
                share_plans_with_a_law=float(np.isfinite(dur).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--levels", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--scenarios", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--dirs", type=int, nargs="+", default=[1, 3], choices=[1, 3])
    ap.add_argument("--reserve", type=float, default=0.25)
    a = ap.parse_args()
    arrs = json.load(open(ROOT / "tests" / "golden" / "arrangements.json"))
    P = thing_problem(arrs["pink_bottle"])
    x0 = level_tray_states(a.B, seed=3)
    mpc = BatchMPC(P, a.B, way_p=waypoints_for(P, x0))
    mpc.set_observation(0.0, x0)
    mpc.advance()
    sweep = R.study_sweep(P.body_params, [0.02, 0.02, 0.03])
    span = np.asarray(P.contact_span, dtype=np.float64)[0]
    lin = np.stack([span[0], span[1], [0.0, 0.0, 1.0]])
    sets = {1: np.concatenate([np.zeros((1, 3)), lin[2:]], axis=1), 3: np.concatenate([np.zeros((3, 3)), lin], axis=1)}
    rows = []
    for ns in a.scenarios:
        prm = None if ns == 1 else sweep[:ns]
        for M in a.levels:
            speeds = np.linspace(0.0, 1.5, M)
            ms0, (dur0, _, edges0, iters0) = timed(lambda: mpc.retime_plan(speeds, prm, want_edges=True, want_iters=True), mpc, a.reps)
            plain = summary(dur0, edges0, iters0, M)
            for nd in a.dirs:
                ms, (dur, _, edges, iters) = timed(lambda: mpc.retime_plan(speeds, prm, want_edges=True, want_iters=True, reserve=a.reserve, dirs=sets[nd]),
                                                   mpc, a.reps)
                r = dict(B=a.B, n_scen=ns, M=M, n_dir=nd, reserve=a.reserve, jobs=int(edges.size), reserve_device_ms=ms, retime_device_ms=ms0,
                         ratio_to_retime=ms / ms0, solves_ratio=float(iters.mean() / iters0.mean()), bound_on_solves_ratio=1 + 2 * nd,
                         masks_are_subsets=bool(not np.any(edges & ~edges0)), **summary(dur, edges, iters, M),
                         **{"retime_" + k: v for k, v in plain.items()})
                rows.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
    mpc.close()
    print(json.dumps(dict(rows=rows, reps=a.reps)))


if __name__ == "__main__":
    main()
