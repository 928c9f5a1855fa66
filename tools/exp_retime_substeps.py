#!/usr/bin/env python3
"""Cost of the retiming with substeps (upr_batch_retime_plan_substeps) on one MI355X: the plan form at the headline B = 1024 (pink_bottle,
21 knots, one cold solve) for n_scen in {1, 8}, lattices of M in {8, 16} speeds, linspace(0, 1.5, M), and R in {1, 2, 4, 8} substeps.  Per
row: device time of the launches (HIP events, BatchMPC.balance_ms: refinement, state kernel, mask kernel, path kernel) of this call and
of retime_plan on the same handle in the same session, and the ratio; least-squares solves per (instance, scenario, segment, level) job of
both, mean and max (a job here runs at most M (R + 1) projections); the share of set mask bits and of plans with a time law.  R = 1 goes
through the new entry (ctypes: BatchMPC.retime_plan sends it to the plain one).  fixed_ms: the same call on the lattice [0.0], on which
no edge exists and no projection runs -- what the refinement and the state kernel on the B (N R + 1) fine points cost, with the empty
mask rows and the path kernel; retime_fixed_ms the plain call's.  The one expectation written down in advance is derived: interior
points are evaluated only on edges whose two ends pass, so the extra projections are at most (R - 1) x the bits set at R = 1
(extra_projection_bound, per job).  No target ratio is set.  Warm-up calls first, then the median of `--reps` repetitions.
    python tools/exp_retime_substeps.py [--B 1024] [--reps 21] [--levels 8 16] [--scenarios 1 8] [--substeps 1 2 4 8]"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import balance_ref as R  # noqa: E402
from upright_amd._capi import iptr, ptr  # noqa: E402
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


def substeps_call(mpc, speeds, prm, Rs):
    """(duration, edges, iters) of the new entry, R = 1 included"""
    speeds = np.ascontiguousarray(speeds, dtype=np.float64)
    ns = 1 if prm is None else prm.shape[0]
    par = None if prm is None else np.ascontiguousarray(prm, dtype=np.float64)
    dur, level = np.zeros((mpc.B, ns)), np.zeros((mpc.B, ns, mpc.N + 1), dtype=np.int32)
    edges, iters = np.zeros((mpc.B, ns, mpc.N, speeds.size), dtype=np.uint32), np.zeros((mpc.B, ns, mpc.N, speeds.size), dtype=np.int32)
    rc = mpc._lib.upr_batch_retime_plan_substeps(mpc._h, ns, ptr(par), 0, speeds.size, ptr(speeds), -1, -1, 0, 1, int(Rs), ptr(dur), iptr(level), None,
                                                 edges.ctypes.data_as(C.POINTER(C.c_uint)), iptr(iters))
    assert rc == 0, mpc._lib.upr_last_error()
    return dur, edges, iters


def summary(dur, edges, iters, M):
    bits = np.unpackbits(edges.view(np.uint8)).sum()
    return dict(solves_mean=float(iters.mean()), solves_max=int(iters.max()), share_bits_set=float(bits) / (edges.size * M),
                bits_per_job=float(bits) / edges.size, share_plans_with_a_law=float(np.isfinite(dur).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--levels", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--scenarios", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--substeps", type=int, nargs="+", default=[1, 2, 4, 8])
    a = ap.parse_args()
    arrs = json.load(open(ROOT / "tests" / "golden" / "arrangements.json"))
    P = thing_problem(arrs["pink_bottle"])
    x0 = level_tray_states(a.B, seed=3)
    mpc = BatchMPC(P, a.B, way_p=waypoints_for(P, x0))
    mpc.set_observation(0.0, x0)
    mpc.advance()
    sweep = R.study_sweep(P.body_params, [0.02, 0.02, 0.03])
    rest = np.array([0.0])
    rows = []
    for ns in a.scenarios:
        prm = None if ns == 1 else sweep[:ns]
        fixed0, _ = timed(lambda: mpc.retime_plan(rest, prm), mpc, a.reps)
        fixed = {Rs: timed(lambda: substeps_call(mpc, rest, prm, Rs), mpc, a.reps)[0] for Rs in a.substeps}
        for M in a.levels:
            speeds = np.linspace(0.0, 1.5, M)
            ms0, (dur0, _, edges0, iters0) = timed(lambda: mpc.retime_plan(speeds, prm, want_edges=True, want_iters=True), mpc, a.reps)
            plain = summary(dur0, edges0, iters0, M)
            one = None
            for Rs in a.substeps:
                ms, (dur, edges, iters) = timed(lambda: substeps_call(mpc, speeds, prm, Rs), mpc, a.reps)
                if Rs == 1:
                    one = dict(identical_to_retime=bool(np.array_equal(edges, edges0) and np.array_equal(iters, iters0) and np.array_equal(dur, dur0)))
                r = dict(B=a.B, n_scen=ns, M=M, substeps=Rs, jobs=int(edges.size), substeps_device_ms=ms, retime_device_ms=ms0, ratio_to_retime=ms / ms0,
                         fixed_ms=fixed[Rs], retime_fixed_ms=fixed0, solves_ratio=float(iters.mean() / iters0.mean()),
                         extra_projection_bound=(Rs - 1) * plain["bits_per_job"], masks_are_subsets=bool(not np.any(edges & ~edges0)),
                         **summary(dur, edges, iters, M), **{"retime_" + k: v for k, v in plain.items()}, **(one if Rs == 1 else {}))
                rows.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
    mpc.close()
    print(json.dumps(dict(rows=rows, reps=a.reps)))


if __name__ == "__main__":
    main()
