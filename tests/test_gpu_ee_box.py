"""End-effector box constraint on the MI355X: the two linearisation kernels' records against the host emulation of their source,
the headline batch at full size with a box that bites (QP optimality checked in numpy, SQP plans inside the box, the same plans
without it outside), a box that never binds against the oracle, the headline with HPIPM slacks and a box, and the
ControllerInterface / ControllerManager surface of a merged reference config with the box enabled.  The oracle does not know
the box: where it is active the checks are numpy restatements (tests/test_ee_box.py) and KKT residuals."""
import copy
import json
from pathlib import Path

import numpy as np
import pytest

from oracle.oracle import Oracle
from test_ee_box import BOX_HI, BOX_LO, box_rows
from test_emu import Emu
from upright_amd import _capi
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, stationary_guess, waypoints_for

pytestmark = pytest.mark.gpu

HEADLINE_ROWS = "upr_qp3_cfg<9, 1, 4, 3, 20, 256, true, false, false>"


def _setup(arrangements, B, seed, lo=BOX_LO, hi=BOX_HI, **kw):
    P = thing_problem(arrangements["pink_bottle"], **kw)
    P.ee_box, P.ee_box_lower, P.ee_box_upper = True, np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    x0 = level_tray_states(B, seed=seed)
    return P, x0, waypoints_for(P, x0)


def _plan_rows(mpc, xs, t0=0.0):
    """The box rows of every instance's plan at knots 1 .. N-1, through upr_batch_state_rows: (B, N - 1, 6)."""
    B, N = xs.shape[0], xs.shape[1] - 1
    inst = np.repeat(np.arange(B), N - 1)
    t = np.tile(t0 + mpc.problem.dt * np.arange(1, N), B)
    return mpc.state_rows(xs[:, 1:N].reshape(-1, xs.shape[2]), t=t, inst=inst, jac=False).reshape(B, N - 1, -1)[..., -6:]


@pytest.mark.parametrize("form,orientation", [("1", False), ("0", False), ("0", True)])
def test_device_records_equal_the_emulation(arrangements, form, orientation, monkeypatch):
    """Every double of every knot's record of the device kernel -- upr_linearize2_kernel (UPR_LIN2=1), upr_linearize_kernel
    (UPR_LIN2=0; with orientation weights in either form) -- against the host emulation of the same source, on a batch that does
    not fill its last workgroup, with a moving target (two waypoints) and random trajectories."""
    monkeypatch.setenv("UPR_LIN2", form)
    B = 37
    P, x0, way = _setup(arrangements, B, seed=21)
    P.way_t = np.array([0.4, 1.6])
    way = np.ascontiguousarray(np.stack([way[:, 0], way[:, 0] + np.array([0.3, -0.2, 0.1])], axis=1))
    way_q = None
    if orientation:
        P.Wee = np.array([1.0, 1.0, 1.0, 0.3, 0.5, 0.2])
        rng = np.random.default_rng(4)
        q = rng.normal(size=(B, 2, 4)); q[..., 3] += 4.0
        way_q = np.ascontiguousarray(q / np.linalg.norm(q, axis=-1, keepdims=True))
    xs, us = stationary_guess(x0, P.N, P.nu)
    rng = np.random.default_rng(5)
    xs = np.ascontiguousarray(xs + rng.uniform(-0.2, 0.2, xs.shape)); xs[:, 0] = x0
    us = np.ascontiguousarray(rng.uniform(-1, 1, us.shape))
    mpc = BatchMPC(P, B, way_p=way, way_q=way_q)
    mpc.set_observation(0.0, x0)
    mpc.set_guess(xs, us)
    mpc.qp_kkt()                       # (linearises at the guess)
    dev = mpc.lin_records()
    mpc.close()
    e = Emu(P, B)
    try:
        e.E.emu_set_lin_form(int(form))
        if way_q is not None:
            e.E.emu_set_way_q(_capi.ptr(way_q))
        emu = e.linearize(way, np.zeros(B), xs, us)
    finally:
        e.E.emu_set_lin_form(1)
        e.E.emu_set_way_q(None)
    assert dev.shape == emu.shape and dev.shape[2] == e.lin_hess + 45 + 6 * 10
    o = e.lin_hess + 45
    assert np.abs(emu[:, 1:P.N, o:o + 6]).max() > 0.1              # (the box rows are there)
    assert (np.abs(dev - emu) / np.maximum(1.0, np.abs(emu))).max() < 1e-10


def test_full_batch_with_an_active_box(arrangements):
    """The headline batch (B = 1024) with a box that its plans without it leave (the tray rises ~0.2 m on the way): the QP of the
    ROWS instantiation converges and its primal-dual point satisfies the optimality conditions assembled in numpy with the box's
    multipliers in play; converged SQP plans stay in the box at knots 1 .. N-1 on every instance; the same instances without
    the box leave it."""
    from kkt_check import kkt_residuals

    B = 1024
    P, x0, way = _setup(arrangements, B, seed=0, qp_tol=1e-9, qp_iter_max=60)
    xs0, us0 = stationary_guess(x0, P.N, P.nu)
    mpc = BatchMPC(P, B, way_p=way)
    assert mpc.kernel_times()["qp_kernel"].endswith(HEADLINE_ROWS + ">")
    mpc.set_observation(0.0, x0)
    mpc.set_guess(xs0, us0)
    sol = mpc.qp_kkt()
    lin = mpc.lin_records()
    st = mpc.stats()
    conv = st["qp_status_last"] == 0
    assert conv.mean() > 0.99
    view = copy.copy(P); view.proj_sph = np.zeros(6, dtype=np.int32)   # (kkt_check sizes the row block by len(pair_a) + len(proj_sph))
    for b in np.flatnonzero(conv):
        res = kkt_residuals(view, P.body_params, x0[b], xs0[b], us0[b], lin[b], {k: v[b] for k, v in sol.items()})
        assert res.max() < 1e-7, (b, res)
    lam_box = sol["lam"][:, 1:P.N, -6:]
    assert (lam_box.max(axis=(1, 2)) > 1e-3).mean() > 0.9          # the box is active in the QP of most instances
    mpc.close()
    # converged SQP
    P.sqp_iters, P.delta_tol, P.cost_tol = 15, 1e-6, 1e-9
    plans = {}
    for box in (True, False):
        Q = copy.copy(P); Q.ee_box = box
        m = BatchMPC(Q, B, way_p=way)
        m.set_observation(0.0, x0)
        m.advance()
        plans[box] = (m.solution()[1], m.stats())
        m.close()
    mpc = BatchMPC(P, B, way_p=way)   # (the rows of both plans, through the term access of the box problem)
    rows_on, rows_off = _plan_rows(mpc, plans[True][0]), _plan_rows(mpc, plans[False][0])
    for b in range(4):                # upr_batch_state_rows against the numpy restatement
        for k in (1, 7, P.N - 1):
            assert np.abs(rows_on[b, k - 1] - box_rows(P, P.way_t, way[b], k * P.dt, plans[True][0][b, k, :9])).max() < 1e-12
    mpc.close()
    assert np.all(plans[True][1]["qp_status_last"] == 0)
    assert rows_on.min() >= -1e-6, rows_on.min()
    assert (rows_off.min(axis=(1, 2)) < -1e-2).mean() > 0.9, np.sort(rows_off.min(axis=(1, 2)))[-20:]


def test_box_that_never_binds_matches_the_oracle(arrangements):
    """A box of +-100 m: its rows are in every QP (the ROWS instantiation, the line search's EXACT form with rows) and never bind:
    converged SQP plans match the oracle's, which has no box, at the parity tolerances of tests/test_gpu_parity.py."""
    B = 3
    P, x0, way = _setup(arrangements, B, seed=31, lo=[-100.0] * 3, hi=[100.0] * 3, sqp_iters=12)
    xs0, us0 = stationary_guess(x0, P.N, P.nu)
    mpc = BatchMPC(P, B, way_p=way)
    assert mpc.kernel_times()["qp_kernel"].endswith(HEADLINE_ROWS + ">")
    mpc.set_observation(0.0, x0)
    mpc.advance()
    _, xs, us = mpc.solution()
    st = mpc.stats()
    mpc.close()
    Po = copy.copy(P); Po.ee_box = False
    for b in range(B):
        Po.way_p = way[b]
        xo, uo, so, rc = Oracle(Po).solve(0.0, x0[b], xs0[b], us0[b])
        assert st["sqp_iters_done"][b] == so.sqp_iters_done
        assert np.abs(xs[b] - xo).max() < 1e-4 and np.abs(us[b] - uo).max() < 1e-4
        assert abs(np.linalg.norm(xs[b]) - np.linalg.norm(xo)) < 1e-4 and abs(np.linalg.norm(us[b]) - np.linalg.norm(uo)) < 1e-4


def test_headline_with_slacks_and_box(arrangements):
    """HPIPM slacks on the boxes and the polytopic rows (the box rows among them): part 1 of upr_qp3_list.h takes the problem and
    the last QP of every instance's SQP solve ends with status 0."""
    B = 64
    P, x0, way = _setup(arrangements, B, seed=3, sqp_iters=8)
    P.slacks = dict(state_box=True, input_box=True, poly_ineq=True)
    mpc = BatchMPC(P, B, way_p=way)
    assert mpc.kernel_times()["qp_kernel"].endswith("upr_qp3_cfg<9, 1, 4, 3, 20, 256, true, true, false>>")
    mpc.set_observation(0.0, x0)
    mpc.advance()
    st = mpc.stats()
    assert np.all(st["qp_status_last"] == 0) and np.all(np.isfinite(mpc.solution()[1]))
    mpc.close()


def _manager(arrangements):
    from upright_amd import control

    cfg = copy.deepcopy(json.load(open(Path(__file__).parent / "golden" / "configs.json"))["full_bottle_point1"]["controller"])
    cfg["end_effector_box_constraint"] = dict(enabled=True, xyz_lower=BOX_LO.tolist(), xyz_upper=BOX_HI.tolist())
    bodies, contacts = control.objects_from_fixture(arrangements["pink_bottle"])
    return control.ControllerManager.from_config(cfg, bodies=bodies, contacts=contacts)


def test_controller_interface_with_the_box(arrangements):
    """full_bottle_point1 with end_effector_box_constraint enabled: ControllerInterface builds it, the term query
    getStateInputInequalityConstraintValue("end_effector_box_constraint", t, x, u) returns the numpy rows, the obstacle-row access
    keeps its contract (no pairs: an error), ControllerManager runs 20 control steps and valueFunction answers."""
    m = _manager(arrangements)
    ci = m.mpc
    P = ci.problem
    assert P.ee_box
    x0 = np.array(m.settings.initial_state)
    m.warmstart()
    rng = np.random.default_rng(6)
    for t in (0.0, 0.35, 1.2):
        x = x0.copy(); x[:9] += rng.uniform(-0.1, 0.1, 9)
        v = ci.getStateInputInequalityConstraintValue("end_effector_box_constraint", t, x, np.zeros(P.nu))
        assert v.shape == (6,) and np.abs(v - box_rows(P, P.way_t, P.way_p, t, x[:9])).max() < 1e-12
    with pytest.raises(RuntimeError, match="no collision pairs"):
        ci._mpc.obstacle_rows(x0)
    with pytest.raises(RuntimeError):
        ci.getStateInputInequalityConstraintValue("obstacle_avoidance", 0.0, x0, np.zeros(P.nu))
    x, t = x0.copy(), 0.0
    for _ in range(20):
        t += 0.01
        xd, u = m.step(t, x)
        assert np.all(np.isfinite(u)) and np.all(np.isfinite(xd))
        x = xd
    assert ci._mpc.stats()["qp_status_last"][0] == 0
    assert np.isfinite(ci.valueFunction(t, x))
    assert np.all(np.isfinite(ci.valueFunctionStateDerivative(t, x)))
