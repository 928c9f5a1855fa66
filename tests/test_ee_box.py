"""End-effector box constraint ("end_effector_box_constraint": end_effector_box_constraint.h:47-76, registered at
controller_interface.cpp:257-270) on the host: settings -> problem, the linearisation kernels' source through the test-only host
emulation against a numpy restatement, and one emulated SQP iteration with an active box checked through the optimality
conditions of its QP (tests/kkt_check.py).  The oracle does not know the box: where it is active the checks are numpy
restatements and KKT residuals.  The device side is tests/test_gpu_ee_box.py."""
import copy
import json
from pathlib import Path

import numpy as np
import pytest

from kkt_check import kkt_residuals
from test_emu import Emu, _case, _emu_kkt, _obstacle_case
from upright_amd import _capi, control, control_bindings

GOLD = Path(__file__).resolve().parent / "golden"
# Box around the target for the headline plan (start 2 m / -1 m off the target in x / y, the tray rising ~0.2 m on its way
# there, the plan ending on the target): it contains the start and the end and cuts the rise to 0.1 m
BOX_LO, BOX_HI = np.array([-0.5, -1.5, -0.1]), np.array([2.5, 0.5, 0.1])


def box_rows(P, way_t, way_p, t, q):
    """numpy restatement: [p_d(t) + upper - p(q); p(q) - (p_d(t) + lower)], p from robots.py's forward kinematics, p_d the
    waypoints interpolated linearly in time and held outside their interval (ocs2 LinearInterpolation)."""
    p = P.chain.forward(q)[0]
    pd = np.array([np.interp(t, way_t, way_p[:, i]) for i in range(3)])
    return np.concatenate([pd + P.ee_box_upper - p, p - (pd + P.ee_box_lower)])


def box_jacobian(P, way_t, way_p, t, q, h=1e-6):
    J = np.zeros((6, len(q)))
    for j in range(len(q)):
        dq = np.zeros(len(q)); dq[j] = h
        J[:, j] = (box_rows(P, way_t, way_p, t, q + dq) - box_rows(P, way_t, way_p, t, q - dq)) / (2 * h)
    return J


def _with_box(P):
    P.ee_box, P.ee_box_lower, P.ee_box_upper = True, BOX_LO.copy(), BOX_HI.copy()
    return P


def test_settings_enable_the_box(arrangements):
    """controller.yaml:91-94 (off by default; xyz_lower / xyz_upper read at wrappers.py:239-250): enabled, the term becomes six
    state rows per knot of the problem instead of a refusal."""
    g = json.load(open(GOLD / "configs.json"))["full_bottle_point1"]["controller"]
    bodies, contacts = control.objects_from_fixture(arrangements["pink_bottle"])
    s = control.ControllerSettings(g, bodies=bodies, contacts=contacts)
    assert not s.end_effector_box_constraint_enabled and not control_bindings.problem_from_settings(s).ee_box
    s.end_effector_box_constraint_enabled = True
    s.xyz_lower, s.xyz_upper = BOX_LO.copy(), BOX_HI.copy()
    P = control_bindings.problem_from_settings(s)
    assert P.ee_box and np.array_equal(P.ee_box_lower, BOX_LO) and np.array_equal(P.ee_box_upper, BOX_HI)
    assert P.n_state_rows == 6
    cp = _capi.problem_to_c(P)
    assert cp.ee_box == 1 and list(cp.ee_box_lower) == list(BOX_LO) and list(cp.ee_box_upper) == list(BOX_HI)
    e = Emu(P, 1)
    import ctypes as C

    o = (C.c_int * 8)()
    e.E.emu_kkt_offsets(C.byref(e.cp), o)
    lin_obs, no = list(o)[6:8]
    assert no == 6 and e.lin_stride == lin_obs + 6 * (1 + P.nq)
    # the bounds are validated
    s.xyz_lower, s.xyz_upper = BOX_HI.copy(), BOX_LO.copy()
    with pytest.raises(RuntimeError, match="lower <= upper"):
        control_bindings.problem_from_settings(s)
    s.xyz_lower = np.zeros(2)
    with pytest.raises(RuntimeError, match="three values"):
        control_bindings.problem_from_settings(s)


@pytest.mark.parametrize("case", ["headline", "orientation", "collision_rows"])
def test_linearisation_box_rows(arrangements, case):
    """Both forms of the linearisation source (upr_linearize2.h's lane jobs and upr_linearize.h's phases; the orientation-weighted
    shape runs the phases in either form): the six rows equal the numpy restatement to 1e-12 at knots 0 .. N-1 of instances with
    their own time and targets (two waypoints: the target moves), their gradient the central differences of it, and every entry
    of the record in front of the box rows -- for the collision shape also the pairs' gradients behind them -- is bit-identical
    to the record without the box."""
    B = 2
    if case == "collision_rows":
        P, x0, way, xs, us = _obstacle_case(arrangements, B, 5)
    else:
        P, x0, way, xs, us = _case(arrangements, B, 7)
        P.way_t = np.array([0.4, 1.6])
        way = np.ascontiguousarray(np.stack([way[:, 0], way[:, 0] + np.array([0.3, -0.2, 0.1])], axis=1))
    way_q = None
    if case == "orientation":
        P.Wee = np.array([1.0, 1.0, 1.0, 0.3, 0.5, 0.2])
        way_q = np.ascontiguousarray(np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (B, len(P.way_t), 1)))
    rng = np.random.default_rng(3)
    xs = np.ascontiguousarray(xs + rng.uniform(-0.2, 0.2, xs.shape)); us = np.ascontiguousarray(rng.uniform(-1, 1, us.shape))
    t0 = np.array([0.0, 0.35])
    off = Emu(P, B)
    on = Emu(_with_box(copy.copy(P)), B)
    nq, N, nsr = P.nq, P.N, len(P.pair_a) + len(P.proj_sph)
    lin_obs = off.lin_hess + nq * (nq + 1) // 2
    assert on.lin_stride == off.lin_stride + 6 * (1 + nq)
    try:
        if way_q is not None:
            on.E.emu_set_way_q(_capi.ptr(way_q))
        for form in (0, 1):
            on.E.emu_set_lin_form(form)
            r_off = off.linearize(way, t0, xs, us)
            r_on = on.linearize(way, t0, xs, us)
            assert np.array_equal(r_on[..., :lin_obs + nsr], r_off[..., :lin_obs + nsr])
            g_off = r_off[..., lin_obs + nsr:].reshape(B, N + 1, nsr, nq)
            g_on = r_on[..., lin_obs + nsr + 6:].reshape(B, N + 1, nsr + 6, nq)
            assert np.array_equal(g_on[:, :, :nsr], g_off)
            for b in range(B):
                for k in range(N):
                    t, q = t0[b] + k * P.dt, xs[b, k, :nq]
                    ref = box_rows(on.P, P.way_t, way[b], t, q)
                    assert np.abs(r_on[b, k, lin_obs + nsr:lin_obs + nsr + 6] - ref).max() < 1e-12, (form, b, k)
                    assert np.abs(g_on[b, k, nsr:] - box_jacobian(on.P, P.way_t, way[b], t, q)).max() < 1e-8, (form, b, k)
                    assert np.array_equal(g_on[b, k, nsr:nsr + 3], -g_on[b, k, nsr + 3:])
    finally:
        on.E.emu_set_lin_form(1)
        on.E.emu_set_way_q(None)


def test_one_sqp_iteration_with_an_active_box(arrangements):
    """One SQP iteration of the headline shape with the box of BOX_LO / BOX_HI, which the plan without it leaves: the QP's
    primal-dual point satisfies the optimality conditions assembled in numpy (kkt_check treats the record's rows generically and
    sizes the block from len(pair_a) + len(proj_sph): it gets a problem view whose proj_sph counts the six rows) with the box's
    multipliers in play; the production kernel's ROWS instantiation (which exports no multipliers in the emulation) takes the
    same step; the line search's merit counts the box rows, at the trial point (a walk per knot) as out of the records."""
    B = 2
    P, x0, way, xs, us = _case(arrangements, B, 5, qp_tol=1e-9, qp_iter_max=60)
    _with_box(P)
    e = Emu(P, B)
    t0 = np.zeros(B)
    lin = e.linearize(way, t0, xs, us)
    dx, du, stats, ws = e.qp(1, xs, us, x0, lin)
    assert np.all(stats[:, 2] == 0)
    view = copy.copy(P); view.proj_sph = np.zeros(6, dtype=np.int32)
    for b in range(B):
        sol = dict(dx=dx[b], du=du[b], **_emu_kkt(e, ws, b))
        res = kkt_residuals(view, P.body_params, x0[b], xs[b], us[b], lin[b], sol)
        assert res.max() < 1e-7, (b, res)
        assert sol["lam"][1:P.N, -6:].max() > 1e-2            # the box is active
    dx3, du3, st3, ws3 = e.qp(3, xs, us, x0, lin)
    assert np.all(st3[:, 2] == 0)
    assert np.abs(dx3 - dx).max() < 1e-8 * max(1.0, np.abs(dx).max()) and np.abs(du3 - du).max() < 1e-8 * max(1.0, np.abs(du).max())
    xs2, us2, _ = e.linesearch(xs, us, x0, t0, way, lin, ws3, st3)
    assert np.all(st3[:, 3] > 0)
    rows = np.array([[box_rows(P, P.way_t, way[b], k * P.dt, xs2[b, k, :9]) for k in range(1, P.N)] for b in range(B)])
    assert rows.min() < -1e-3                               # (the linearised box: the accepted point violates it a little)
    box_sse = P.dt * (np.minimum(rows, 0.0) ** 2).sum(axis=(1, 2))
    # the same point once more, as the base of a line search (out of its records), with and without the box
    off = Emu(_case(arrangements, B, 5, qp_tol=1e-9, qp_iter_max=60)[0], B)
    viol = {}
    for name, em in (("on", e), ("off", off)):
        lin2 = em.linearize(way, t0, xs2, us2)
        ws0, st0 = np.zeros((B, ws3.shape[1])), np.zeros_like(st3)
        em.linesearch(xs2, us2, x0, t0, way, lin2, ws0, st0)
        viol[name] = st0[:, 5]
    assert np.abs(viol["on"] ** 2 - viol["off"] ** 2 - box_sse).max() < 1e-10
    assert np.abs(st3[:, 5] - viol["on"]).max() < 1e-9
