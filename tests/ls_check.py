"""Independent restatement of the SQP line search (upr_linesearch.h upr_ls_instance; the rule of the oracle's orc_solve: ocs2_sqp's
filter line search with alpha_decay 0.5, alpha_min 1e-4, gamma_c 1e-6, g_max 1e6, g_min 1e-6, Armijo factor 1e-4, and its three
convergence tests) in numpy on top of the oracle's merit (Oracle.performance), at a GIVEN step: the device's or the emulation's own QP
step, so that the comparison tests the line search alone.

The oracle has no end-effector box: its rows (tests/test_ee_box.box_rows) are added to the inequality part of the merit at knots
1 .. N-1 with the weight dt, as the kernel does.  The result carries the smallest relative margin of every comparison that decided
it, so that a test can tell a tie (rounding decides) from a defect."""
import copy

import numpy as np

from oracle.oracle import Oracle

ALPHA_DECAY, ALPHA_MIN, GAMMA_C, G_MAX, G_MIN, ARMIJO = 0.5, 1e-4, 1e-6, 1e6, 1e-6, 1e-4


def _margin(a, b):
    """relative distance of the two sides of a comparison a < b"""
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def line_search(P, t0, x0, xs, us, dx, du, way_p=None, body_params=None, way_q=None, dyn=None, pflag=1.0, qp_status=0.0):
    """One SQP iteration's line search for one instance.  xs [N+1][nx], us [N][nu], dx, du: the step (states sliced to nx).
    Returns dict(alpha (0: rejected), cost, viol, dxn, dun, xs, us (the iterate afterwards), done, margin, branch)."""
    from test_ee_box import box_rows

    Pb = copy.copy(P)
    if way_p is not None:
        Pb.way_p = np.asarray(way_p)
    if body_params is not None:
        Pb.body_params = np.asarray(body_params)
    if way_q is not None:
        Pb.way_q = np.asarray(way_q)
    O = Oracle(Pb)
    if dyn is not None:
        O.set_dynamic_obstacle(np.asarray(dyn), pflag)
    N, dt = P.N, P.dt
    box = bool(getattr(P, "ee_box", False))
    wp = np.asarray(Pb.way_p)

    def merit(X, U):
        perf = O.performance(t0, x0, X, U).copy()
        if box:
            for k in range(1, N):
                v = np.minimum(0.0, box_rows(P, P.way_t, wp, t0 + k * dt, X[k, :P.nq]))
                perf[3] += dt * float(v @ v)
        return perf

    xs, us, dx, du = (np.asarray(a, dtype=np.float64) for a in (xs, us, dx, du))
    base = merit(xs, us)
    base_viol = np.sqrt(base[1] + base[2] + base[3])
    descent = 0.0
    for k in range(N):
        _, gx, gu, _, _ = O.stage_cost(t0 + k * dt, xs[k], us[k])
        descent += dt * (gx @ dx[k] + gu @ du[k])
    dxn, dun = np.linalg.norm(dx), np.linalg.norm(du)
    margins = []
    alpha, accepted, perf, armijo = 1.0, False, base, False
    if qp_status != 2.0:
        while alpha >= ALPHA_MIN:
            Xt, Ut = xs + alpha * dx, us + alpha * du
            perf = merit(Xt, Ut)
            viol = np.sqrt(perf[1] + perf[2] + perf[3])
            margins += [_margin(viol, G_MAX), _margin(viol, G_MIN)]
            if viol > G_MAX:
                accepted = False
            elif viol < G_MIN:
                armijo = descent < 0.0
                if armijo:
                    rhs = base[0] + ARMIJO * alpha * descent
                    accepted = perf[0] < rhs
                    margins.append(_margin(perf[0], rhs))
                else:
                    accepted = True
            else:
                a, b = perf[0] < base[0] - GAMMA_C * base_viol, viol < (1.0 - GAMMA_C) * base_viol
                accepted = a or b
                margins += [_margin(perf[0], base[0] - GAMMA_C * base_viol), _margin(viol, (1.0 - GAMMA_C) * base_viol)]
            if accepted:
                break
            alpha *= ALPHA_DECAY
    if accepted:
        cost, viol = perf[0], np.sqrt(perf[1] + perf[2] + perf[3])
        xs_out, us_out = xs + alpha * dx, us + alpha * du
    else:
        cost, viol, xs_out, us_out = base[0], base_viol, xs, us
    metrics = accepted and abs(base[0] - cost) < P.cost_tol and viol < G_MIN
    primal = accepted and alpha * dxn < P.delta_tol and alpha * dun < P.delta_tol
    if accepted:
        margins += [_margin(abs(base[0] - cost), P.cost_tol), _margin(alpha * dxn, P.delta_tol), _margin(alpha * dun, P.delta_tol)]
    branch = ("rejected" if not accepted else "full" if alpha == 1.0 else "backtracked",
              "armijo" if accepted and viol < G_MIN else "filter",
              "metrics" if metrics else "primal" if primal else "stepsize" if not accepted else "continue")
    return dict(alpha=alpha if accepted else 0.0, cost=cost, viol=viol, dxn=dxn, dun=dun, xs=xs_out, us=us_out,
                done=(not accepted) or metrics or primal, margin=min(margins) if margins else np.inf, branch=branch)
