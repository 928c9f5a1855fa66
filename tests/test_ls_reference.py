"""The line-search reference (tests/ls_check.py) against the line-search kernel's source through the host emulation (tests/emu,
emu_linesearch: the generic form) at the emulation's own QP step, over the case table the device test (tests/test_gpu_linesearch.py)
uses where the shape needs no controller manager.  This checks the reference before any GPU time and gives the generic source CPU
coverage on every one of these shapes."""
import ctypes as C

import numpy as np
import pytest

from ls_check import line_search
from test_emu import Emu, _case, _obstacle_case, _projectile_case
from upright_amd import _capi
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, stationary_guess, waypoints_for

p = _capi.ptr
# the four forms of the line search (upr_launch_select.h, UPR_LS_FORMS) and their (NFM, NBM, EXACT, OBS)
EXACT, EXACT_ROWS, SMALL, LARGE = "exact", "exact_rows", "small", "large"
LS_FORMS = {EXACT: (12, 1, True, False), EXACT_ROWS: (12, 1, True, True), SMALL: (12, 1, False, True), LARGE: (96, 8, False, True)}


def _perturbed(xs, us, seed, s):
    rng = np.random.default_rng(seed)
    xs = xs.copy(); xs[:, 1:, :9] += rng.uniform(-s, s, xs[:, 1:, :9].shape)
    return np.ascontiguousarray(xs), np.ascontiguousarray(us + rng.uniform(-s, s, us.shape))


def ls_case(arrangements, name, **kw):
    """dict(P, x0 [B][nx], way, t0 [B], xs0, us0 (the guess), bp or None, way_q or None, dyn or None, form)"""
    from test_ee_box import _with_box
    c = dict(bp=None, way_q=None, dyn=None, form=EXACT)
    if name in ("headline", "headline_backtrack", "headline_capped", "headline_converged", "orientation", "box_only"):
        qp = dict(qp_iter_max=1) if name == "headline_capped" else {}
        P, x0, way, xs, us = _case(arrangements, 4, 21, **qp, **kw)
        if name == "headline_backtrack":
            xs, us = _perturbed(xs, us, 5, 1.0)
        if name == "headline_converged":     # restart from the oracle's converged plans: tiny steps, violation below g_min
            from oracle.oracle import Oracle
            Pc = thing_problem(arrangements["pink_bottle"], sqp_iters=12)
            for b in range(4):
                Pc.way_p = way[b]
                xs[b], us[b], _, _ = Oracle(Pc).solve(0.0, x0[b], xs[b], us[b])
        if name == "orientation":
            P.Wee = np.array([1.0, 1.0, 1.0, 0.3, 0.5, 0.2])
            rng = np.random.default_rng(2)
            q = rng.normal(size=(4, 1, 4)); q /= np.linalg.norm(q, axis=2, keepdims=True)
            c["way_q"] = np.ascontiguousarray(q)
        if name == "box_only":
            _with_box(P); c["form"] = EXACT_ROWS
        t0 = np.zeros(4) if name == "headline_converged" else np.array([0.0, 0.1, 0.25, 0.5])
        c.update(P=P, x0=x0, way=way, t0=t0, xs0=np.ascontiguousarray(xs), us0=np.ascontiguousarray(us))
    elif name == "collision_rows":
        P, x0, way, xs, us = _obstacle_case(arrangements, 4, 4, **kw)
        c.update(P=P, x0=x0, way=way, t0=np.zeros(4), xs0=xs, us0=us, form=EXACT_ROWS)
    elif name == "thrown_ball":
        P, x0, way, xs, us, dyn = _projectile_case(arrangements, 3, **kw)
        c.update(P=P, x0=x0, way=way, t0=np.zeros(3), xs0=xs, us0=us, dyn=np.ascontiguousarray(dyn), form=EXACT_ROWS)
    elif name in ("dice", "cups", "box_arch_rows"):
        arr = {"dice": "foam_die2", "cups": "blue_cups", "box_arch_rows": "box_arch"}[name]
        P = thing_problem(arrangements[arr], **kw)
        if name == "box_arch_rows":
            from upright_amd import robots
            for k, v in robots.collision_model(P.chain, robots.SIMPLE_COLLISION_PAIRS).items():
                setattr(P, k, v)
        x0 = level_tray_states(3, seed=9)
        way = waypoints_for(P, x0, offset=(-0.5, 0.5, 0.0))
        xs, us = stationary_guess(x0, P.N, P.nu)
        c.update(P=P, x0=x0, way=way, t0=np.zeros(3), xs0=np.ascontiguousarray(xs), us0=np.ascontiguousarray(us), form=LARGE)
    elif name in ("robust", "robust_N100"):
        from test_gpu_parity import _robust_problem
        P, bp, x0, way = _robust_problem(arrangements, 3, N=100 if name == "robust_N100" else 20, **kw)
        xs, us = stationary_guess(x0, P.N, P.nu)
        c.update(P=P, x0=x0, way=way, t0=np.zeros(3), xs0=np.ascontiguousarray(xs), us0=np.ascontiguousarray(us), bp=bp, form=LARGE)
    else:
        raise KeyError(name)
    return c


CPU_CASES = ["headline", "headline_backtrack", "headline_capped", "headline_converged", "orientation", "box_only", "collision_rows", "thrown_ball", "dice", "box_arch_rows",
             "cups", "robust"]


def check_against_reference(c, b, alpha, cost, viol, dxn, dun, xs1, us1, done, dx, du, qp_status, report):
    """One instance's line-search outcome against the reference at the same step; returns the reference's result.  An instance
    whose deciding comparison is a tie (smallest margin below 1e-9 relative) may take the other branch: it is reported."""
    P = c["P"]
    nx = P.nx
    r = line_search(P, c["t0"][b], c["x0"][b, :nx], c["xs0"][b, :, :nx], c["us0"][b], dx, du, way_p=c["way"][b],
                    body_params=None if c["bp"] is None else c["bp"][b], way_q=None if c["way_q"] is None else c["way_q"][b],
                    dyn=None if c["dyn"] is None else c["dyn"][b], qp_status=qp_status)
    if alpha != r["alpha"] and r["margin"] < 1e-9:
        report.append((b, alpha, r["alpha"], r["margin"]))
        return r
    assert alpha == r["alpha"], (b, alpha, r["alpha"], r["margin"], r["branch"])
    assert abs(cost - r["cost"]) <= 1e-10 * abs(r["cost"]) + 1e-13, (b, cost, r["cost"])
    assert abs(viol - r["viol"]) <= 1e-10 * abs(r["viol"]) + 1e-13, (b, viol, r["viol"])
    assert abs(dxn - r["dxn"]) <= 1e-12 * max(1.0, r["dxn"]) and abs(dun - r["dun"]) <= 1e-12 * max(1.0, r["dun"]), (b, dxn, r["dxn"], dun, r["dun"])
    if r["alpha"] > 0:
        assert np.abs(xs1 - r["xs"]).max() <= 1e-14 * max(1.0, np.abs(r["xs"]).max())
        assert np.abs(us1 - r["us"]).max() <= 1e-14 * max(1.0, np.abs(r["us"]).max())
    else:
        assert np.array_equal(xs1, c["xs0"][b, :, :nx]) and np.array_equal(us1, c["us0"][b])
    assert bool(done) == r["done"], (b, done, r["branch"])
    return r


@pytest.mark.parametrize("name", CPU_CASES)
def test_line_search_reference_against_emulation(arrangements, name):
    c = ls_case(arrangements, name)
    P = c["P"]
    B = c["x0"].shape[0]
    e = Emu(P, B)
    if c["bp"] is not None:
        e.bp = np.ascontiguousarray(c["bp"])
        e.E.emu_make_Df(C.byref(e.cp), B, p(e.bp), p(e.Df))
    flags = np.ones(B)
    e.E.emu_set_dynamic(p(c["dyn"]) if c["dyn"] is not None else None, p(flags) if c["dyn"] is not None else None)
    e.E.emu_set_way_q(p(c["way_q"]) if c["way_q"] is not None else None)
    try:
        way = np.ascontiguousarray(c["way"]); t0 = np.ascontiguousarray(c["t0"])
        lin = e.linearize(way, t0, c["xs0"], c["us0"])
        dx, du, stats, ws = e.qp(3, c["xs0"], c["us0"], c["x0"], lin)
        xs1, us1, done = e.linesearch(c["xs0"], c["us0"], c["x0"], t0, way, lin, ws, stats)
    finally:
        e.E.emu_set_dynamic(None, None)
        e.E.emu_set_way_q(None)
    report, branches = [], []
    for b in range(B):
        r = check_against_reference(c, b, stats[b, 3], stats[b, 4], stats[b, 5], stats[b, 10], stats[b, 11], xs1[b], us1[b], done[b],
                                    dx[b], du[b], stats[b, 2], report)
        branches.append(r["branch"])
    print(name, branches, "ties:", report)
    assert len(report) <= 1, report
