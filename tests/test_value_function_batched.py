"""CPU tests of the batched value function: the host recursion with the slack pairs of softened rows against a dense
condensation that keeps every slack as a variable, the slack pairs the QP kernels export against their own optimality
conditions, and the SOURCE of the cost-to-go and query kernels (upright_amd/csrc/upr_value.h) through the test-only host
emulation tests/emu/upr_vf_emu.cpp (one thread per workgroup) against the host module upright_amd/value_function.py, which is
their specification.  The execution on the GPU is checked by tests/test_gpu_value_function.py."""
import ctypes as C
import os
import types
from pathlib import Path

import numpy as np
import pytest

import fb_check
from kkt_check import friction_rows
from test_emu import Emu, _case, _obstacle_case
from upright_amd import _capi
from upright_amd.problem import THING_HOME, thing_problem
from upright_amd.sampling import stationary_guess, waypoints_for
from upright_amd.value_function import (_dynamics, qp_objective, qp_slack_penalties, record_layout, riccati_value_function, slot_active,
                                        slot_layout)

VF_EMU = Path(os.environ.get("UPR_VF_EMU_LIB", str(Path(__file__).resolve().parent / "emu" / "libupr_vf_emu.so")))
p = _capi.ptr
ip = _capi.iptr

# the slack dictionary of tests/test_emu.py::test_soft_rows_kernel_source
SOFT = dict(state_box=True, input_box=True, poly_ineq=True, equality=False, lower_L2_penalty=100.0, upper_L2_penalty=50.0,
            lower_L1_penalty=0.0, upper_L1_penalty=0.5)


def _vf():
    V = C.CDLL(str(VF_EMU))
    V.emu_vf_qp3.restype = C.c_long
    V.emu_vf_kkt_doubles.restype = C.c_long
    return V


# ---- 1. host recursion with pairs against a dense condensation ------------------------------------------------------------------------
def dense_condensation(P, lin, sol, E, Df, pairs=None):
    """Hessian of min over (u_0 .. u_{N-1}, every slack sigma) of the QP's barrier-augmented quadratic as a function of x_0: the whole
    horizon condensed into one dense system in z = [x_0; u; sigma] (dynamics eliminated).  A softened row c = G z >= 0 with slack sigma
    contributes w0 (G z + sigma)^2 / 2 (the row's barrier, w0 = lam / t) + (Z + w_s) sigma^2 / 2 (penalty and the barrier of sigma >= 0,
    w_s = gam / tau); a hard row w0 (G z)^2 / 2.  Nothing here uses the eliminated weight w0 (Z + w_s) / (Z + w0 + w_s).  A softened
    equality is the penalty Z |R z|^2 / 2; a hard one keeps its multipliers as variables with the recursion's -rho I on their block."""
    nq, nx, nu, N, h = P.nq, P.nx, P.nu, P.N, P.dt
    ne, nfc = Df.shape
    o = record_layout(P)
    npoly = E.shape[0]
    _, _, _, no, upper, softened = slot_layout(P, npoly)
    act = slot_active(P, npoly)
    sl = P.slacks or {}
    soft_eq = bool(sl.get("equality", sl.get("poly_ineq")))
    Zs = np.where(upper, float(sl.get("upper_L2_penalty", 100.0)), float(sl.get("lower_L2_penalty", 100.0)))
    A, Bq = _dynamics(nq, h)
    Bf = np.hstack([Bq, np.zeros((nx, nfc))])
    w0 = sol["lam"] / sol["slack"]
    on = act & softened if pairs is not None else np.zeros_like(act)
    w_s = pairs[2] / pairs[1] if pairs is not None else np.zeros_like(w0)
    nsig = int(on.sum())
    nz = nx + N * nu + nsig
    T = [np.hstack([np.eye(nx), np.zeros((nx, nz - nx))])]
    Sel = []
    for k in range(N):
        S = np.zeros((nu, nz)); S[:, nx + k * nu:nx + (k + 1) * nu] = np.eye(nu)
        Sel.append(S); T.append(A @ T[k] + Bf @ S)
    iu = np.triu_indices(nq)
    D = np.hstack([np.zeros((ne, nq)), Df])
    Hz = np.zeros((nz, nz))
    Rall = []
    sig_at = nx + N * nu
    for k in range(N + 1):
        rec = lin[k]
        rows = []   # (slot, row of the constraint in z)
        Ix = T[k]
        for i in range(nx):
            rows.append((i, Ix[i])); rows.append((nx + i, -Ix[i]))
        if k < N:
            for i in range(nu):
                rows.append((2 * nx + i, Sel[k][i])); rows.append((2 * nx + nu + i, -Sel[k][i]))
            for r in range(npoly):
                rows.append((2 * nx + 2 * nu + r, E[r] @ Sel[k][nq:]))
            if no:
                Jo = rec[o["obs"] + no:o["obs"] + no + no * nq].reshape(no, nq)
                for r in range(no):
                    rows.append((2 * nx + 2 * nu + npoly + r, Jo[r] @ T[k][:nq]))
        Gk, wk = [], []
        for j, g in rows:
            if not act[k, j]:
                continue
            g = g.copy()
            if on[k, j]:
                g[sig_at] = 1.0
                Hz[sig_at, sig_at] += Zs[j] + w_s[k, j]
                sig_at += 1
            Gk.append(g); wk.append(w0[k, j])
        Gk = np.array(Gk)
        Hz += Gk.T @ (np.array(wk)[:, None] * Gk)
        if k < N:
            Hk = np.zeros((nq, nq)); Hk[iu] = rec[o["hess"]:o["hess"] + o["nh"]]; Hk = Hk + np.triu(Hk, 1).T
            Hxx = h * np.diag(P.Qdiag).astype(float); Hxx[:nq, :nq] += h * Hk
            Hz += T[k].T @ Hxx @ T[k] + Sel[k].T @ (h * np.diag(P.Rdiag)) @ Sel[k]
            Ck = rec[o["gx"]:o["gx"] + ne * nx].reshape(ne, nx)
            R = Ck @ T[k] + D @ Sel[k]
            if soft_eq:
                Hz += float(sl.get("lower_L2_penalty", 100.0)) * R.T @ R
            else:
                Rall.append(R)
        elif P.terminal_constraint:
            Jp = rec[o["hess"]:o["hess"] + 3 * nq].reshape(3, nq)
            CN = np.zeros((3 + 2 * nq, nx)); CN[:3, :nq] = -Jp; CN[3:, nq:] = np.eye(2 * nq)
            Hz += T[N].T @ (CN.T @ CN / 1e-6) @ T[N]
    assert sig_at == nz
    if Rall:   # hard rows: [[H, R'], [R, -rho I]] (value_function.py: rho 1e-6 where the forces cannot span the rows, else 1e-12)
        Rm = np.vstack(Rall)
        Hz = np.block([[Hz, Rm.T], [Rm, -(1e-6 if nfc < ne else 1e-12) * np.eye(Rm.shape[0])]])
    return Hz[:nx, :nx] - Hz[:nx, nx:] @ np.linalg.solve(Hz[nx:, nx:], Hz[nx:, :nx])


def _synthetic(seed=3, soft_eq=True):
    rng = np.random.default_rng(seed)
    nq, nb, nc, nf, N, h = 2, 1, 1, 3, 4, 0.1
    nx, nfc, ne = 3 * nq, nf * nc, 6 * nb
    nu = nq + nfc
    P = types.SimpleNamespace(nq=nq, nx=nx, nu=nu, N=N, dt=h, nb=nb, nf=nf, nc=nc, pair_a=[], proj_sph=[], terminal_constraint=True,
                              slacks=dict(SOFT, equality=soft_eq), Qdiag=rng.uniform(0.1, 1.0, nx), Rdiag=rng.uniform(0.1, 1.0, nu), xd=rng.normal(size=nx))
    o = record_layout(P)
    stride = o["hess"] + max(o["nh"], 3 * nq)
    lin = np.zeros((N + 1, stride))
    iu = np.triu_indices(nq)
    for k in range(N):
        J = rng.normal(size=(3, nq)); lin[k, o["hess"]:o["hess"] + o["nh"]] = (J.T @ J)[iu]
        lin[k, o["gx"]:o["gx"] + ne * nx] = rng.normal(size=ne * nx)
    lin[N, o["hess"]:o["hess"] + 3 * nq] = rng.normal(size=3 * nq)
    E = rng.normal(size=(5 * nc, nfc)); Df = rng.normal(size=(ne, nfc))
    ni = 2 * nx + 2 * nu + 5 * nc
    lam = rng.uniform(0.0, 2.0, (N + 1, ni)); t = rng.uniform(0.05, 2.0, (N + 1, ni))
    act = slot_active(P, 5 * nc)
    lam = np.where(act, lam, 0.0); t = np.where(act, t, 1.0)
    sol = dict(dx=np.zeros((N + 1, nx)), du=np.zeros((N, nu)), pi=rng.normal(size=(N + 1, nx)), nu=rng.normal(size=(N, ne)), lam=lam, slack=t)
    pairs = (rng.uniform(0.0, 1.0, (N + 1, ni)), rng.uniform(0.05, 2.0, (N + 1, ni)), rng.uniform(0.0, 2.0, (N + 1, ni)))
    xs, us = rng.normal(size=(N + 1, nx)), rng.normal(size=(N, nu))
    return P, xs, us, lin, sol, E, Df, pairs


def test_host_recursion_with_slack_pairs_against_a_dense_condensation():
    """riccati_value_function(..., pairs=...) on a synthetic problem like the one of
    tests/test_host.py::test_value_function_recursion_against_a_dense_solve, with softened boxes and friction rows and random
    (t, lam, sigma, tau, gam), against the condensation above that keeps every sigma as a variable: independent of the formula of the
    eliminated weight.  Bound: 1e-7 relative on P_0, the bound of that test.  With a softened equality and with a hard one."""
    for soft_eq in (True, False):
        P, xs, us, lin, sol, E, Df, pairs = _synthetic(3, soft_eq)
        Pk, pk, X, U = riccati_value_function(P, xs, us, lin, sol, E, Df, pairs=pairs)
        V = dense_condensation(P, lin, sol, E, Df, pairs)
        err = np.abs(Pk[0] - V).max() / np.abs(V).max()
        print("host recursion with pairs vs dense condensation (soft_eq %d): %.2e relative" % (soft_eq, err))
        assert err < 1e-7, err
        # the pairs matter: with lam / t on the softened rows the recursion is another matrix (by more than 100x the bound)
        P0 = riccati_value_function(P, xs, us, lin, sol, E, Df)[0][0]
        assert np.abs(P0 - V).max() / np.abs(V).max() > 100 * 1e-7
        # pairs = None keeps the arithmetic of the hard recursion: the (0, 1, 0) pairs of hard rows change nothing either
        Ph = types.SimpleNamespace(**{**P.__dict__, "slacks": dict(equality=soft_eq, lower_L2_penalty=100.0)})
        a = riccati_value_function(Ph, xs, us, lin, sol, E, Df)[0]
        b = riccati_value_function(Ph, xs, us, lin, sol, E, Df, pairs=pairs)[0]
        assert np.array_equal(a, b)


# ---- the QP kernels with their export, through the emulation ------------------------------------------------------------------------------
def _export(e, kernel, xs, us, x0, lin):
    """One QP per instance on the emulated kernel source (1: generic, 3: production with upr_qp_args::kkt) and its primal-dual point in
    the layout of BatchMPC.qp_kkt() / qp_slack_pairs(): (sol[b] dicts, pairs[b] tuples, stats, raw) with raw = (ws, mult, offsets) as the
    cost-to-go kernel takes them."""
    P, B = e.P, e.B
    V = _vf()
    offs = (C.c_int * 8)()
    V.emu_vf_offsets(C.byref(e.cp), kernel, offs)
    offs = np.array(list(offs), dtype=np.int32)
    ni = int(offs[7])
    n1, N, nx, ne = P.N + 1, P.N, e.nx, e.ne
    if kernel == 1:
        dx, du, stats, ws = e.qp(1, xs, us, x0, lin)
        mult = ws
    else:
        stats = np.zeros((B, 12))
        need = V.emu_vf_qp3(C.byref(e.cp), B, None, None, None, None, None, None, C.c_long(0), None, None, C.c_long(0))
        assert need > 0
        ws = np.zeros((B, need))
        kd = V.emu_vf_kkt_doubles(C.byref(e.cp))
        mult = np.full((B, kd), np.nan)   # (device memory is not zero: every slot of the export must be written)
        assert V.emu_vf_qp3(C.byref(e.cp), B, p(xs), p(us), p(x0), p(lin), p(e.Df), p(ws), C.c_long(need), p(stats), p(mult), C.c_long(kd)) == 0
        dx = ws[:, :n1 * nx].reshape(B, n1, nx); du = ws[:, n1 * nx:n1 * nx + N * e.nu].reshape(B, N, e.nu)
    act = slot_active(P)
    _, _, _, _, _, softened = slot_layout(P)
    sols, pairs = [], []
    for b in range(B):
        m = mult[b]
        blk = lambda o: m[o:o + n1 * ni].reshape(n1, ni)
        lam = np.where(act, blk(offs[2]), 0.0); t = np.where(act, blk(offs[3]), 1.0)
        if kernel == 3:   # the export itself carries the defaults
            assert np.array_equal(lam, blk(offs[2])) and np.array_equal(t, blk(offs[3]))
        sols.append(dict(dx=dx[b], du=du[b], pi=m[offs[0]:offs[0] + n1 * nx].reshape(n1, nx), nu=m[offs[1]:offs[1] + N * ne].reshape(N, ne), lam=lam, slack=t))
        if offs[4] >= 0:
            on = act & softened
            sg, ta, ga = np.where(on, blk(offs[4]), 0.0), np.where(on, blk(offs[5]), 1.0), np.where(on, blk(offs[6]), 0.0)
            if kernel == 3:
                assert np.array_equal(sg, blk(offs[4])) and np.array_equal(ta, blk(offs[5])) and np.array_equal(ga, blk(offs[6]))
            pairs.append((sg, ta, ga))
        else:
            pairs.append(None)
    return sols, pairs, stats, (ws, mult, offs)


def _soft_case(arrangements):
    """The inputs of tests/test_emu.py::test_soft_rows_kernel_source at the tolerance that test converges to: instance 1 starts with a
    base acceleration beyond what the friction cone balances."""
    B = 2
    P, x0, way, xs, us = _case(arrangements, B, 11, qp_tol=1e-7, qp_iter_max=40)
    x0[1, 18] = 5.0
    xs[1, :, 18] = 5.0
    P.slacks = dict(SOFT)
    return P, x0, way, xs, us


def test_exported_slack_pairs_satisfy_their_own_conditions(arrangements):
    """The slack pairs (sigma, tau, gam) of the softened rows as the generic kernel leaves them in its workspace and as the production
    kernel's SOFT instantiation exports them (out of its parked copies), against the conditions of the pair at the QP's exit, each bounded
    by the residual of the kernel that folds it in (upr_qp.h: upr_qp_ineq_sweep what == 3; upr_qp3.h: sweep_row_soft):
        |sigma - tau|                 <= stats[8]  r_ineq: the max over the rows of |c + sigma - t| and |sigma - tau|
        |Z sigma + z - lam - gam|     <= stats[6]  r_stat: takes the max of the slack stationarity in
        gam tau                       <= ntot stats[9]  r_comp is the MEAN of lam t and gam tau over all ntot pairs, every product positive
    (+ 1e-12: the kernels evaluate the same expressions in another order).  tau, gam > 0 (interior point)."""
    P, x0, way, xs, us = _soft_case(arrangements)
    e = Emu(P, 2)
    lin = e.linearize(way, np.zeros(2), xs, us)
    act = slot_active(P)
    _, _, _, _, upper, softened = slot_layout(P)
    on = act & softened
    assert softened.all()   # every class is softened here: each row brings its pair
    ntot = 2 * int(act.sum())
    Z = np.where(upper, 50.0, 100.0); z = np.where(upper, 0.5, 0.0)
    big = {}
    for kernel in (1, 3):
        sols, pairs, stats, _ = _export(e, kernel, xs, us, x0, lin)
        for b in range(2):
            assert stats[b, 2] == 0
            sg, ta, ga = pairs[b]
            lam = sols[b]["lam"]
            assert np.all(ta[on] > 0) and np.all(ga[on] > 0) and np.all(sg[~on] == 0) and np.all(ta[~on] == 1) and np.all(ga[~on] == 0)
            r_pair = np.abs(sg - ta)[on].max()
            r_stat = np.abs(Z * sg + z - lam - ga)[on].max()
            r_comp = (ga * ta)[on].max()
            print("kernel %d instance %d: |sigma - tau| %.2e (r_ineq %.2e)  |Z sigma + z - lam - gam| %.2e (r_stat %.2e)  gam tau %.2e (ntot r_comp %.2e)  max sigma %.2e"
                  % (kernel, b, r_pair, stats[b, 8], r_stat, stats[b, 6], r_comp, ntot * stats[b, 9], sg.max()))
            assert r_pair <= stats[b, 8] + 1e-12 and r_stat <= stats[b, 6] + 1e-12 and r_comp <= ntot * stats[b, 9] + 1e-12
        big[kernel] = pairs[1][0].max()
    # the violated instance carries active slacks
    assert big[1] > 1e-3 and big[3] > 1e-3, big


# ---- 3. emulated cost-to-go kernel against the host module ----------------------------------------------------------------------------------
def _emu_cost_to_go(e, xs, us, lin, raw):
    ws, mult, offs = raw
    P, B = e.P, e.B
    n1, nx = P.N + 1, e.nx
    out = dict(Pk=np.full((B, n1, nx, nx), np.nan), pk=np.full((B, n1, nx), np.nan), J=np.full((B, n1), np.nan), X=np.full((B, n1, nx), np.nan))
    _vf().emu_vf_cost_to_go(C.byref(e.cp), B, p(xs), p(us), p(lin), p(e.Df), p(ws), C.c_long(ws.shape[1]), p(mult), C.c_long(mult.shape[1]),
                            ip(offs), p(out["Pk"]), p(out["pk"]), p(out["J"]), p(out["X"]))
    return out


def host_cost_to_go(P, xs, us, lin, sol, Df, pairs):
    E = friction_rows(P) if P.nf == 3 else np.zeros((0, P.nf * P.nc))
    Pk, pk, X, U = riccati_value_function(P, xs, us, lin, sol, E, Df, pairs=pairs)
    stage = qp_objective(P, xs, lin, X, U) + qp_slack_penalties(P, lin, sol, Df, pairs)
    J = np.array([stage[k:].sum() for k in range(P.N + 1)])
    return dict(Pk=Pk, pk=pk, J=J, X=X)


def rel_err(a, b):
    """max |a - b| relative to the largest entry of b, per knot (the cost-to-go matrices span decades along the horizon); J, one number
    per knot that ends at 0: relative to J_0."""
    if np.ndim(a) == 1:
        return float(np.abs(a - b).max() / np.abs(b).max())
    a = np.asarray(a).reshape(a.shape[0], -1); b = np.asarray(b).reshape(b.shape[0], -1)
    return float((np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-300)).max())


def _ctg_cases(arrangements, name):
    if name == "headline":
        P, x0, way, xs, us = _case(arrangements, 2, 5, qp_tol=1e-9, qp_iter_max=40)
        return P, x0, way, xs, us, 3
    if name in ("soft", "soft_generic"):   # (the production kernel's export, and the generic kernel's workspace)
        return _soft_case(arrangements) + (3 if name == "soft" else 1,)
    if name == "robust":   # the settings of tests/test_emu.py::test_kkt_conditions_checked_in_numpy (BASELINE config 4)
        P = thing_problem(arrangements["robust_8corner"], nf=1, force_weight=0.0, qp_tol=1e-9, qp_iter_max=40)
        P.slacks = dict(state_box=True, input_box=False, poly_ineq=True)
        x0 = np.tile(np.concatenate([THING_HOME, np.zeros(18)]), (1, 1))
        way = waypoints_for(P, x0, offset=(-2.0, 1.0, 0.0))
        xs, us = stationary_guess(x0, P.N, P.nu)
        return P, x0, way, np.ascontiguousarray(xs), np.ascontiguousarray(us), 3
    # (the seed of tests/test_emu.py's "collision_rows" case: both instances start outside the obstacles' margins -- seed 4's first one
    #  does not, its hard rows are infeasible and the QP diverges; the headline instantiation with state-polytopic rows)
    P, x0, way, xs, us = _obstacle_case(arrangements, 2, 5, qp_tol=1e-8, qp_iter_max=40)
    return P, x0, way, xs, us, 3


# Pk: measured disagreement of the emulated kernel with the host recursion (relative to the largest entry of the knot's matrix, worst
# knot and instance) | the floor: the host recursion against the dense condensation of the same inputs on P_0.  The bound is 3x the
# first number.  (The headline's worst knot is knot 2 of instance 0, barrier weights to 9e8 next to h R = 1e-3 on the forces: S = Df Hff^-1
# Df' + 1e-12 I spans twelve decades there, and the host's indefinite stage system and the kernel's Cholesky factor of S round it
# differently; on P_0 the two differ by 3.2e-6 and 9.6e-8, the kernel from the dense condensation by 3.2e-6 and 4.6e-7.)
MEASURED_PK = {
    "headline": (9.55e-05, 4.63e-07),
    "soft": (7.64e-09, 2.29e-06),
    "soft_generic": (7.64e-09, 4.38e-06),
    "robust": (1.74e-10, 2.48e-08),
    "collision_rows": (1.68e-08, 1.84e-07),
}
# pk (p_0: a sum of some 300 products; the other knots are copies of the costates) and J (some 2000 products per instance): the rounding
# of double-precision sums of that length, n eps = 2000 x 1.1e-16, with a margin -- measured 1.0e-16 .. 5.5e-16.  X = xs + dx: one
# addition, the same on both sides.
TOL_SUMS = 1e-12


@pytest.mark.parametrize("name", ["headline", "soft", "soft_generic", "robust", "collision_rows"])
def test_cost_to_go_kernel_source_against_the_host_module(arrangements, name):
    """upr_vf_instance (the body of upr_value_kernel) at one thread per workgroup against value_function.riccati_value_function /
    qp_objective / qp_slack_penalties on the primal-dual point of the same emulated QP: Pk, pk, J and X at every knot, for the
    headline (hard), both instances of the soft case, upright_robust's eight bodies (frictionless, softened equality and state
    boxes) and the bottle with collision rows.  Bound on Pk: 3x the measured disagreement (MEASURED_PK above, with the floor: the host
    recursion against the dense condensation on the same inputs, itself held under eps cond(M) N); on pk and J: rounding of their sums;
    X: exact.  The binding check of Pk is tests/test_vf_reference.py: every shape against a reference that is neither."""
    P, x0, way, xs, us, kernel = _ctg_cases(arrangements, name)
    B = x0.shape[0]
    e = Emu(P, B)
    lin = e.linearize(way, np.zeros(B), xs, us)
    sols, pairs, stats, raw = _export(e, kernel, xs, us, x0, lin)
    assert np.all(stats[:, 2] == 0), stats[:, 2]
    dev = _emu_cost_to_go(e, xs, us, lin, raw)
    assert all(np.all(np.isfinite(v)) for v in dev.values())
    worst = dict(Pk=0.0, pk=0.0, J=0.0, X=0.0, floor=0.0)
    for b in range(B):
        host = host_cost_to_go(P, xs[b], us[b], lin[b], sols[b], e.Df[b], pairs[b])
        for key in ("Pk", "pk", "J", "X"):
            worst[key] = max(worst[key], rel_err(dev[key][b], host[key]))
        E = friction_rows(P) if P.nf == 3 else np.zeros((0, P.nf * P.nc))
        V = dense_condensation(P, lin[b], sols[b], E, e.Df[b], pairs[b])
        floor = np.abs(host["Pk"][0] - V).max() / np.abs(V).max()
        worst["floor"] = max(worst["floor"], floor)
        # the floor is held too: two float64 routes to the same P_0 (a recursion of N stage solves, one condensed solve), each solve good
        # to eps cond relative, with the stage systems' condition number as the dense reference computes it (fb_check: cond(M) per knot)
        cond = fb_check.feedback_reference(P, lin[b], sols[b], E, e.Df[b], pairs=pairs[b])[2].max()
        worst["floor_bound"] = max(worst.get("floor_bound", 0.0), np.finfo(float).eps * cond * P.N)
        assert floor <= np.finfo(float).eps * cond * P.N, (b, floor, cond)
        assert np.abs(dev["Pk"][b] - np.swapaxes(dev["Pk"][b], 1, 2)).max() == 0.0
    print("cost-to-go kernel source vs host, %s: " % name + "  ".join("%s %.2e" % kv for kv in worst.items()))
    tol_pk = 3.0 * MEASURED_PK[name][0]
    assert worst["Pk"] <= tol_pk, (worst["Pk"], tol_pk)
    assert worst["pk"] <= TOL_SUMS and worst["J"] <= TOL_SUMS and worst["X"] == 0.0, worst
    if name in ("soft", "soft_generic"):
        # discrimination: on the instance with active slacks, lam / t in place of the effective weight moves P_0 by more than 100x the
        # tolerance -- otherwise the comparison would say nothing about softened rows
        host = host_cost_to_go(P, xs[1], us[1], lin[1], sols[1], e.Df[1], pairs[1])
        E = friction_rows(P)
        wrong = riccati_value_function(P, xs[1], us[1], lin[1], sols[1], E, e.Df[1])[0]
        moved = np.abs(wrong[0] - host["Pk"][0]).max() / np.abs(host["Pk"][0]).max()
        print("lam / t in place of the effective weight moves P_0 by %.2e" % moved)
        assert moved > 100.0 * tol_pk, (moved, tol_pk)


# ---- 4. emulated query kernel ------------------------------------------------------------------------------------------------------------------
def numpy_query(P, ctg, t0, inst, t, x):
    """ValueFunction._seg / value / gradient on downloaded Pk, pk, J, X."""
    V, G = np.zeros(len(t)), np.zeros((len(t), P.nx))
    for i in range(len(t)):
        b = inst[i]
        s = min(max((float(t[i]) - t0[b]) / P.dt, 0.0), float(P.N))
        j = min(int(s), P.N - 1); a = s - j
        v, g = [], []
        for k in (j, j + 1):
            d = x[i] - ctg["X"][b, k]
            v.append(ctg["J"][b, k] + ctg["pk"][b, k] @ d + 0.5 * d @ ctg["Pk"][b, k] @ d)
            g.append(ctg["pk"][b, k] + ctg["Pk"][b, k] @ d)
        V[i] = (1 - a) * v[0] + a * v[1]; G[i] = (1 - a) * g[0] + a * g[1]
    return V, G


def query_points(P, ctg, t0, n, seed):
    """n points spread over instances and times: at knot times, between them, before the first knot and behind the last; states near
    the plan's."""
    rng = np.random.default_rng(seed)
    B = ctg["X"].shape[0]
    inst = rng.integers(0, B, n).astype(np.int32)
    t = t0[inst] + rng.uniform(-0.3, P.N * P.dt + 0.3, n)
    t[::4] = t0[inst[::4]] + P.dt * rng.integers(0, P.N + 1, len(t[::4]))   # knot times
    k = np.clip(((t - t0[inst]) / P.dt).astype(int), 0, P.N)
    x = ctg["X"][inst, k] + rng.normal(size=(n, P.nx)) * 1e-2
    return inst, np.ascontiguousarray(t), np.ascontiguousarray(x)


def test_query_kernel_source_against_numpy(arrangements):
    """upr_vf_query_point (the body of upr_value_query_kernel) against numpy on the same Pk, pk, J, X: a few hundred fused operations
    per output, 1e-12 relative (V: to |V|; dV/dx: to the largest component of the point's gradient)."""
    P, x0, way, xs, us, kernel = _ctg_cases(arrangements, "headline")
    e = Emu(P, 2)
    lin = e.linearize(way, np.zeros(2), xs, us)
    sols, pairs, stats, raw = _export(e, kernel, xs, us, x0, lin)
    ctg = _emu_cost_to_go(e, xs, us, lin, raw)
    t0 = np.array([0.25, -1.0])
    inst, t, x = query_points(P, ctg, t0, 64, 0)
    V, G = np.full(64, np.nan), np.full((64, P.nx), np.nan)
    _vf().emu_vf_query(C.byref(e.cp), 64, ip(inst), p(t), p(x), p(t0), p(ctg["Pk"]), p(ctg["pk"]), p(ctg["J"]), p(ctg["X"]), p(V), p(G))
    Vn, Gn = numpy_query(P, ctg, t0, inst, t, x)
    assert (t < t0[inst]).any() and (t > t0[inst] + P.N * P.dt).any() and np.abs(Vn).min() > 0
    assert (np.abs(V - Vn) / np.abs(Vn)).max() < 1e-12
    assert (np.abs(G - Gn).max(axis=1) / np.abs(Gn).max(axis=1)).max() < 1e-12
