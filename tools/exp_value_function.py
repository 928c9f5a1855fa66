#!/usr/bin/env python3
"""Where the time of a batched value-function update goes, on the headline at B = 1024 (needs the GPU):
    QP launch         device time per QP launch of an advance (HIP events, BatchMPC.kernel_times)
    cost-to-go        device time of upr_value_kernel (HIP events around that launch, BatchMPC.value_function_ms)
    update, host      wall time of value_function_update(): hold statistics, linearise, QP, cost-to-go, restore, synchronise
    query             wall time of value_function() for n points (upload, upr_value_query_kernel, download)
Warm-up launches first, then the median of `--reps` repetitions.
    python tools/exp_value_function.py [--B 1024] [--reps 21] [--points 4096]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, waypoints_for


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--points", type=int, default=4096)
    a = ap.parse_args()
    P = thing_problem(json.load(open(ROOT / "tests" / "golden" / "arrangements.json"))["pink_bottle"])
    x0 = level_tray_states(a.B, seed=3)
    mpc = BatchMPC(P, a.B, way_p=waypoints_for(P, x0))
    mpc.set_observation(0.0, x0)
    for _ in range(3):                                   # warm-up: code objects, allocations
        mpc.advance()
    mpc.enable_timing(1)
    mpc.advance()
    qp_ms = float(mpc.kernel_times()["qp_ms"])
    mpc.enable_timing(0)
    for _ in range(3):
        mpc.value_function_update()
    ctg_ms, upd_ms = [], []
    for _ in range(a.reps):
        t = time.perf_counter()
        mpc.value_function_update()
        upd_ms.append(1e3 * (time.perf_counter() - t))
        ctg_ms.append(mpc.value_function_ms())
    X = mpc.cost_to_go()["X"]
    rng = np.random.default_rng(0)
    inst = rng.integers(0, a.B, a.points)
    t = rng.uniform(0.0, P.N * P.dt, a.points)
    x = X[inst, np.clip((t / P.dt).astype(int), 0, P.N)] + rng.normal(size=(a.points, P.nx)) * 1e-2
    for _ in range(3):
        mpc.value_function(t, x, inst)
    q_ms = []
    for _ in range(a.reps):
        t1 = time.perf_counter()
        mpc.value_function(t, x, inst)
        q_ms.append(1e3 * (time.perf_counter() - t1))
    med = lambda v: float(np.median(v))
    print(json.dumps(dict(B=a.B, reps=a.reps, qp_launch_ms=qp_ms, cost_to_go_kernel_ms=med(ctg_ms), cost_to_go_kernel_ms_min_max=[min(ctg_ms), max(ctg_ms)],
                          update_host_ms=med(upd_ms), query_points=a.points, query_host_ms=med(q_ms))))
    mpc.close()


if __name__ == "__main__":
    main()
