"""What the feedback gains cost the headline step: bench.py's timed loop (cold start + one SQP iteration, B = 1024) with
sqp.use_feedback_policy on against the same problem with it off, alternating pairs in one process on one box.  With the policy
off the handle has no gain array and the QP kernel's exit writes none, so the difference is the most that forming the gains on
demand can give the headline.  tools/fb_ceiling.py [pairs] [steps]"""
import argparse
import sys

sys.path.insert(0, ".")
import bench

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
rows = {True: [], False: []}
for r in range(pairs):
    for fb in (True, False):
        w = bench.headline_workload(1024)
        w["P"].use_feedback_policy = fb
        mpc = bench.make_engine(w)
        el, _ = bench.rank_main(argparse.Namespace(gpus=1, steps=steps, warmup=5), mpc, w["P"], events=3)
        qp = mpc.kernel_times()["qp_ms"]
        mpc.close()
        rows[fb].append(1e3 * el / steps)
        print("pair %d use_feedback_policy %-5s ms_per_step %.4f qp_ms %.4f" % (r, fb, 1e3 * el / steps, qp), flush=True)
d = [a - b for a, b in zip(rows[True], rows[False])]
print("difference on - off per pair (ms):", " ".join("%.4f" % x for x in d), " mean %.4f" % (sum(d) / len(d)))
for fb in (True, False):
    print("spread of use_feedback_policy %-5s %.4f ms" % (fb, max(rows[fb]) - min(rows[fb])))
