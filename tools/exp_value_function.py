#!/usr/bin/env python3
"""Where the time of a batched value-function update goes, on the headline at B = 1024 (needs the GPU):
    QP launch         device time per QP launch of an advance (HIP events, BatchMPC.kernel_times)
    cost-to-go        device time of upr_value_kernel (HIP events around that launch, BatchMPC.value_function_ms)
    update, host      wall time of value_function_update(): hold statistics, linearise, QP, cost-to-go, restore, synchronise
    query             wall time of value_function() for n points (upload, upr_value_query_kernel, download)
    tracked           wall time of advance() and of tick() with track_value_function() on, next to the same calls without it and to
                      advance() + value_function_update(); device time of the in-stream cost-to-go launch (enable_timing(1))
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

    # tracked row: the same warm loop (a new observation time per period) without tracking, with the explicit update, and tracked
    def loop(call, t_start, observe=False):
        """Median wall time of call(t) over the periods behind the warm-up; observe: set_observation(t, x0) first, outside the timed part."""
        ms = []
        for k in range(3 + a.reps):
            tk = t_start + 0.01 * k
            if observe:
                mpc.set_observation(tk, x0)
            t1 = time.perf_counter()
            call(tk)
            if k >= 3:
                ms.append(1e3 * (time.perf_counter() - t1))
        return med(ms)

    advance_ms = loop(lambda tk: mpc.advance(), 1.0, observe=True)
    advance_update_ms = loop(lambda tk: (mpc.advance(), mpc.value_function_update()), 2.0, observe=True)
    tick_ms = loop(lambda tk: mpc.tick(tk, x0), 3.0)
    mpc.track_value_function()
    tracked_advance_ms = loop(lambda tk: mpc.advance(), 4.0, observe=True)
    tracked_tick_ms = loop(lambda tk: mpc.tick(tk, x0), 5.0)
    replays = mpc.tick_graph_replays()
    mpc.enable_timing(1)
    in_stream = []
    for k in range(5):
        mpc.set_observation(6.0 + 0.01 * k, x0)
        mpc.advance()
        in_stream.append(mpc.value_function_ms())
    mpc.enable_timing(0)
    mpc.track_value_function(False)
    print(json.dumps(dict(B=a.B, reps=a.reps, qp_launch_ms=qp_ms, cost_to_go_kernel_ms=med(ctg_ms), cost_to_go_kernel_ms_min_max=[min(ctg_ms), max(ctg_ms)],
                          update_host_ms=med(upd_ms), query_points=a.points, query_host_ms=med(q_ms),
                          advance_ms=advance_ms, advance_plus_update_ms=advance_update_ms, tracked_advance_ms=tracked_advance_ms, tick_ms=tick_ms,
                          tracked_tick_ms=tracked_tick_ms, tick_graph_replays=replays, tracked_kernel_in_stream_ms=med(in_stream))))
    mpc.close()


if __name__ == "__main__":
    main()
