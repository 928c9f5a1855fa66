"""Cost of the end-effector box constraint on the headline workload (bench.py's configs[1], B = 1024, cold solves, one SQP
iteration): wall time per solve of the batch without the box and with one that the plans touch (tests/test_ee_box.py's
BOX_LO / BOX_HI: the tray may rise 0.1 m above the target, it rises ~0.2 m without the box), alternating, no timing events in the
timed loops; then the average launch of each kernel from the engine's events (upr_batch_enable_timing 1, a separate loop).
    python tools/exp_ee_box.py [--only off|on] [--reps R] [--solves K]
For the launch times as the kernel trace sees them: rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp_ee_box.py --only on
(and --only off)."""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

import bench  # noqa: E402

BOX_LO, BOX_HI = np.array([-0.5, -1.5, -0.1]), np.array([2.5, 0.5, 0.1])   # (tests/test_ee_box.py)


def engine(box):
    w = bench.headline_workload(1024)
    if box:
        P = w["P"]
        P.ee_box, P.ee_box_lower, P.ee_box_upper = True, BOX_LO.copy(), BOX_HI.copy()
    return bench.make_engine(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["off", "on"], default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--solves", type=int, default=40)
    a = ap.parse_args()
    modes = [a.only] if a.only else ["off", "on"]
    eng = {m: engine(m == "on") for m in modes}
    for m in modes:
        mpc = eng[m]
        for _ in range(5):
            mpc.reset_async(); mpc.advance_async()
        mpc.sync()
        st = mpc.stats()
        print("%s: qp kernel %s; qp iterations mean %.2f max %d; qp status 0: %d of %d" % (
            m, mpc.kernel_times()["qp_kernel"], st["qp_iters_last"].mean(), st["qp_iters_last"].max(), (st["qp_status_last"] == 0).sum(), mpc.B))
    for rep in range(a.reps):
        for m in modes:
            mpc = eng[m]
            mpc.enable_timing(0); mpc.sync()
            t0 = time.perf_counter()
            for _ in range(a.solves):
                mpc.reset_async(); mpc.advance_async()
            mpc.sync()
            ms = 1e3 * (time.perf_counter() - t0) / a.solves
            print("rep %d %s: %.4f ms per solve of the batch = %.0f solves/s" % (rep, m, ms, mpc.B / ms * 1e3), flush=True)
    for m in modes:
        mpc = eng[m]
        mpc.enable_timing(1)
        for _ in range(a.solves):
            mpc.reset_async(); mpc.advance_async()
        mpc.sync()
        kt = mpc.kernel_times()
        print("%s events: linearise %.4f ms, QP %.4f ms, line search %.4f ms per launch" % (m, kt["linearize_ms"], kt["qp_ms"], kt["linesearch_ms"]))
        mpc.enable_timing(0)
        mpc.close()


if __name__ == "__main__":
    main()
