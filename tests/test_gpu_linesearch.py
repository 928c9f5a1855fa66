"""The line-search plan (upr_launch_select.h, upr_ls_plan) picks one of four forms of upr_linesearch_kernel by the contact structure:
EXACT without rows (the headline's one body on four frictional contacts), EXACT with state rows (collision / projectile rows, the
end-effector box), the small general form (one body, up to twelve force components) and the large form, each staged or not by its
LDS footprint.  kernel_times()["ls_kernel"] names the one the handle's last line search ran.

test_line_search_at_the_device_step compares every form at the device's own QP step with the numpy reference of tests/ls_check.py:
step length, cost, violation, step norms, the iterate afterwards and the convergence flag."""
import sys
from pathlib import Path

import ctypes as C

import numpy as np
import pytest

from upright_amd.engine import BatchMPC

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from test_emu import EMU, _ls_select  # noqa: E402
from test_gpu_qp_screen import _box_arch, _golden, _headline, _obstacles, _robust  # noqa: E402
from test_ls_reference import CPU_CASES, EXACT, LS_FORMS, SMALL, check_against_reference, ls_case  # noqa: E402
from upright_amd.sampling import stationary_guess  # noqa: E402

pytestmark = pytest.mark.gpu

# case -> (builder, kwargs, (NQ, NFM, NBM, EXACT, OBS) of the form the handle must run, STAGE or None: by the LDS footprint)
LS_CASES = {
    "headline": (_headline, {"B": 4}, (9, 12, 1, True, False), None),
    "collision_rows": (_obstacles, {}, (9, 12, 1, True, True), None),
    "arm_only": (_golden, {"name": "full_bottle_arm_only"}, (6, 12, 1, True, False), None),
    "thing_demo": (_golden, {"name": "thing_demo"}, (9, 12, 1, False, True), None),
    "ur10_demo": (_golden, {"name": "ur10_demo", "level": True}, (6, 12, 1, False, True), None),
    "dice": (_golden, {"name": "full_dice_point1", "arr": "foam_die2"}, (9, 96, 8, False, True), None),
    "box_arch_rows": (_box_arch, {}, (9, 96, 8, False, True), None),
    "robust_N100": (_robust, {"N": 100}, (9, 96, 8, False, True), False),
}


def _name(nq, nfm, nbm, exact, obs, stage):
    b = lambda v: "true" if v else "false"   # noqa: E731
    return "upr_linesearch_kernel<%d, 128, %d, %d, %s, %s, %s>" % (nq, nfm, nbm, b(exact), b(obs), b(stage))


@pytest.fixture(scope="module")
def reached():
    seen = {}
    yield seen
    print("line-search kernels reached:", sorted(set(seen.values())))


@pytest.mark.parametrize("case", list(LS_CASES))
def test_line_search_kernel_the_launch_picks(case, reached):
    """One SQP iteration per case: the line-search form the shape selects, and an empty name before the first launch."""
    builder, kw, form, stage = LS_CASES[case]
    c = builder(**kw)
    P, x0, way = c["P"], c["x0"], c["way"]
    B = x0.shape[0]
    bp = c.get("bp")
    if bp is None:
        bp = np.ascontiguousarray(np.broadcast_to(P.body_params, (B,) + np.shape(P.body_params)))
    mpc = BatchMPC(P, B, body_params=bp, way_p=way)
    try:
        assert mpc.kernel_times()["ls_kernel"] == ""
        mpc.set_sqp_iterations(1)
        mpc.set_observation(0.0, x0)
        mpc.advance()
        name = mpc.kernel_times()["ls_kernel"]
        assert np.all(np.isfinite(mpc.solution()[1]))
    finally:
        mpc.close()
    reached[case] = name
    print(case, name)
    if len(reached) == len(LS_CASES):    # both staged and unstaged forms are reached by the table
        assert {n.endswith("true>") for n in reached.values()} == {True, False}, reached
    assert name in (_name(*form, True), _name(*form, False)), name
    if stage is not None:
        assert name == _name(*form, stage), name


def _golden_ls(name, form, **kw):
    c = _golden(name, **kw)
    P, x0 = c["P"], c["x0"]
    xs, us = stationary_guess(x0, P.N, P.nu)
    c.update(t0=np.array([0.0, 0.2, 0.45])[:x0.shape[0]], xs0=np.ascontiguousarray(xs), us0=np.ascontiguousarray(us), bp=None, way_q=None,
             dyn=None, form=form)
    return c


GOLDEN_LS = {
    "thing_demo": ("thing_demo", SMALL, {}),
    "ur10_demo": ("ur10_demo", SMALL, {"level": True}),
    "ur10_demo_N10": ("ur10_demo", SMALL, {"level": True, "override": {
        "mpc.time_horizon": 1.0, "waypoints": [{"time": 0, "position": [0.15, 0.1, 0.05], "orientation": [0, 0, 0, 1]}]}}),
    "arm_only": ("full_bottle_arm_only", EXACT, {}),
}
DEVICE_CASES = CPU_CASES + ["robust_N100"] + list(GOLDEN_LS)
BRANCHES = {}


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_line_search_at_the_device_step(arrangements, name):
    """Per case: the device's QP step (qp_step), then one SQP iteration from the same guess (advance) and, for the convergence flag,
    two (sqp_iters_done == 1 exactly when the first converged); the line search's outcome against tests/ls_check.py at that step:
    alpha equal (a tie -- smallest relative margin below 1e-9 -- is reported, at most one per case), cost and violation to 1e-10
    relative + 1e-13, step norms to 1e-12, the iterate xs + alpha dx to 1e-14 and bitwise unchanged when the step is rejected."""
    if name in GOLDEN_LS:
        cfg, form, kw = GOLDEN_LS[name]
        c = _golden_ls(cfg, form, **kw)
    else:
        c = ls_case(arrangements, name)
    P = c["P"]
    B, nx = c["x0"].shape[0], P.nx
    xs0, us0 = c["xs0"], c["us0"]
    x0 = c["x0"]
    if c["dyn"] is not None:     # the observation and the guess carry the dynamic obstacle's state
        x0 = np.concatenate([x0, c["dyn"]], axis=1)
        xs0 = np.concatenate([xs0, np.repeat(c["dyn"][:, None, :], P.N + 1, axis=1)], axis=2)
    mpc = BatchMPC(P, B, body_params=c["bp"], way_p=c["way"], way_q=c["way_q"])
    try:
        if c["dyn"] is not None:
            mpc.set_projectile_flag(1.0)
        mpc.set_observation(c["t0"], x0)
        mpc.set_guess(xs0, us0)
        dxs, dus = mpc.qp_step()
        qp_status = mpc.stats()["qp_status_last"].copy()
        mpc.set_guess(xs0, us0); mpc.set_sqp_iterations(1); mpc.advance()
        st = {k: v.copy() for k, v in mpc.stats().items()}
        _, xs1, us1 = mpc.solution()
        ls_name = mpc.kernel_times()["ls_kernel"]
        mpc.set_guess(xs0, us0); mpc.set_sqp_iterations(2); mpc.advance()
        done = mpc.stats()["sqp_iters_done"] == 1
    finally:
        mpc.close()
    plan = _ls_select(C.CDLL(str(EMU)), P)     # (the same rules on the host)
    assert ls_name == plan["name"] and plan["form"] == (P.nq,) + LS_FORMS[c["form"]], (ls_name, plan, c["form"])
    report, branches = [], []
    for b in range(B):
        r = check_against_reference(c, b, st["step_alpha_last"][b], st["cost"][b], st["constraint_violation"][b], st["dx_norm"][b],
                                    st["du_norm"][b], xs1[b, :, :nx], us1[b], done[b], dxs[b, :, :nx], dus[b], qp_status[b], report)
        branches.append(r["branch"])
    BRANCHES[name] = branches
    print(name, ls_name, branches, "ties:", report)
    assert len(report) <= 1, report


def test_line_search_table_reaches_every_branch():
    """The table above shows its coverage: full steps, backtracked steps, the Armijo branch (violation below g_min) and convergence
    by the metrics or the primal test, each in at least one instance."""
    assert set(BRANCHES) == set(DEVICE_CASES), "run the whole module"
    flat = [b for v in BRANCHES.values() for b in v]
    counts = {k: sum(k in b for b in flat) for k in ("full", "backtracked", "rejected", "armijo", "metrics", "primal")}
    print("line-search branches over the table:", counts)
    assert counts["full"] and counts["backtracked"] and counts["armijo"] and counts["metrics"] + counts["primal"], counts
