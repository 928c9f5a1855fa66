"""Fixed-iteration race / indexing screen of the two QP structures behind the production kernel: the generic kernel (upr_qp.h,
upr_qp_kernel<NT> at 64, 128, 256, 512 or 1024 lanes) and the second structure (upr_qp2.h, the five UPR_QP2_SHAPES at 64, 128 or 256
lanes).  upr_qp_plan (upr_qp_select.h) hands them every problem the production structure does not take -- a horizon above 64 on
anything but a frictionless star of several bodies without rows, more than UPR_QP3_NOMAX state rows per knot, a run-time
instantiation that is switched off -- and the knobs UPR_QP_KERNEL = 1 | 2 and UPR_QP_GENERIC put every A/B run on them.

The procedure is tests/test_gpu_qp_screen.py's: the device solves ITERS interior-point iterations (qp_tol = 0) on its own
linearisation records, the same source compiled for the host (tests/emu: emu_qp, emu_qp2, one thread per workgroup, where UPR_SYNC is
nothing) is fed those records with the instance's own inertial parameters and a workspace poisoned with NaN.  After a fixed number of
iterations a race, a missed barrier or a wrong lane split shows at 1e-3 and above (that file's docstring says why a converged
comparison cannot see one); 1e-8 relative to max |dx| leaves room for FMA contraction and the device's reciprocal / rsqrt rounding.

CASES names the structure and the kernel that has to run, worked out on the host from the selection rules (the lane count of the
generic kernel: upr_qp_generic_nt, 512 lanes from max(ne nx, nx nx) = 1024 on, 256 from 512 on, else 64) -- never copied from the
device; tests/test_qp_fallback_reference.py (the CPU twin) resolves every case through emu_qp_select and guards the table's coverage.

The independent leg (emulation and device share their source): one CONVERGED QP per distinct (structure, shape) at the problem's own
tolerances, its primal-dual point -- read where upr_qp_fill_generic / upr_qp2_fill say the kernel left pi, nu, y_N, lam -- through
tests/kkt_check.py, and its step against the production kernel's wherever that kernel takes the problem too."""
import copy
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

from upright_amd import _capi
from upright_amd.engine import BatchMPC
from upright_amd.sampling import stationary_guess

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import test_gpu_qp_screen as S  # noqa: E402
from test_gpu_qp_screen import _box_arch, _golden, _headline, _obstacles, _robust, _soft_boxes  # noqa: E402

GENERIC, SECOND, PRODUCTION = 1, 2, 3
ITERS = 6
QP2_SHAPES = [(9, 1, 4, 3), (9, 1, 4, 1), (6, 1, 4, 1), (6, 1, 4, 3), (9, 2, 8, 3)]   # UPR_QP2_SHAPES (the twin holds the header against it)
QP2_LANES = [64, 128, 256]
GENERIC_LANES = [64, 128, 256, 512, 1024]


def gen(nt):
    return "upr_qp_kernel<%d>" % nt


def qp2(shape, nt):
    return "upr_qp2_kernel<upr_qp2_dims<%d, %d, %d, %d>, %d>" % (tuple(shape) + (nt,))


# ---- builders beyond the production screen's: each returns dict(P, x0, way[, bp]) ---------------------------------------------------------
def _without_slacks(**kw):
    """A golden config whose slacks are cleared: "plain" for upr_qp_plan, so that the second structure takes it."""
    c = _golden(**kw)
    c["P"].slacks = None
    return c


def _box_arch_ee_box(**kw):
    """box_arch's 20 collision pairs and an end-effector box around the target: 26 state rows per knot, more than UPR_QP3_NOMAX.  The
    box holds start and target (0.3 m apart in x and y) and leaves 3 cm of height either way."""
    c = _box_arch(**kw)
    P = c["P"]
    P.ee_box, P.ee_box_lower, P.ee_box_upper = True, np.array([-0.4, -0.4, -0.03]), np.array([0.4, 0.4, 0.03])
    assert P.n_state_rows == 26
    return c


UR10_N10 = S.CASES[(6, 1, 4, 1, 10, False, True, False)][1]
DICE = {"name": "full_dice_point1", "arr": "foam_die2"}
CUPS = {"name": "full_cups_point1", "arr": "blue_cups"}
K1 = {"UPR_QP_KERNEL": "1"}

# name -> (builder, kwargs, environment at create, structure, kernel name); B is the builders' 3 to 6
CASES = {
    # -- the generic kernel at the lane count upr_qp_generic_nt picks (nx = 3 nq, ne = 6 nb; big = max(ne nx, nx nx))
    "generic_headline": (_headline, {}, K1, GENERIC, gen(256)),                               # big 729: baseline
    "generic_rows": (_obstacles, {}, K1, GENERIC, gen(256)),                                  # hard collision rows: ob, hob
    "generic_rows_soft": (_obstacles, {"soft": True}, K1, GENERIC, gen(256)),                 # rows and slacks together
    "generic_soft_boxes": (_soft_boxes, {}, K1, GENERIC, gen(256)),                           # slacks on the boxes: sgk, tak, gak
    "generic_thing_demo": (_golden, {"name": "thing_demo"}, K1, GENERIC, gen(256)),           # nf 1, nfc 4 < ne 6, softened
    "generic_ur10_N10": (_golden, UR10_N10, K1, GENERIC, gen(64)),                            # nq 6 (big 324), the smallest horizon
    "generic_dice": (_golden, DICE, K1, GENERIC, gen(256)),                                   # two bodies, shared contacts: ne 12
    "generic_box_arch": (_box_arch, {}, K1, GENERIC, gen(256)),                               # three bodies and rows: ne 18, big 729
    "generic_cups": (_golden, CUPS, K1, GENERIC, gen(512)),                                   # ne 42: big 1134
    "generic_robust": (_robust, {"N": 20}, K1, GENERIC, gen(512)),                            # ne 48 (big 1296), frictionless, own inertial parameters
    # -- the fallbacks of an empty environment
    "fallback_N65": (_headline, {"N": 65}, {}, SECOND, qp2((9, 1, 4, 3), 128)),               # the smallest horizon the production structure refuses here
    "fallback_N65_soft": (_soft_boxes, {"N": 65}, {}, GENERIC, gen(256)),                     # ... with slacks: not plain
    "fallback_26_rows": (_box_arch_ee_box, {}, {}, GENERIC, gen(256)),                        # d.no 26 > UPR_QP3_NOMAX
    "fallback_no_jit_N12": (_headline, {"B": 4, "N": 12}, {"UPR_QP3_JIT": "0"}, SECOND, qp2((9, 1, 4, 3), 128)),
    # -- 512 lanes asked of the second structure: an alias of its 128-lane form
    "qp2_9x1x4x3_nt512": (_headline, {}, {"UPR_QP_KERNEL": "2", "UPR_QP_NT": "512"}, SECOND, qp2((9, 1, 4, 3), 128)),
}
# -- every lane count of the generic kernel on two shapes that together use every block of its LDS layout
for _nt in GENERIC_LANES:
    CASES["generic_rows_soft_nt%d" % _nt] = (_obstacles, {"soft": True}, {"UPR_QP_KERNEL": "1", "UPR_QP_GENERIC_NT": str(_nt)}, GENERIC, gen(_nt))
    CASES["generic_dice_nt%d" % _nt] = (_golden, DICE, {"UPR_QP_KERNEL": "1", "UPR_QP_GENERIC_NT": str(_nt)}, GENERIC, gen(_nt))
# -- the second structure: its five shapes at its three lane counts
QP2_BUILDERS = {
    (9, 1, 4, 3): (_headline, {}),
    (9, 1, 4, 1): (_without_slacks, {"name": "thing_demo", "level": True}),
    (6, 1, 4, 1): (_without_slacks, {"name": "ur10_demo", "level": True}),
    (6, 1, 4, 3): (_golden, {"name": "full_bottle_arm_only"}),
    (9, 2, 8, 3): (_golden, DICE),
}
for _shape, (_b, _kw) in QP2_BUILDERS.items():
    for _nt in QP2_LANES:
        CASES["qp2_%s_nt%d" % ("x".join(map(str, _shape)), _nt)] = (_b, _kw, {"UPR_QP_KERNEL": "2", "UPR_QP_NT": str(_nt)}, SECOND, qp2(_shape, _nt))

# lane counts the launchers refuse: (environment, builder, kwargs, message)
REFUSED = {
    "generic_nt96": ({"UPR_QP_KERNEL": "1", "UPR_QP_GENERIC_NT": "96"}, _headline, {}, "UPR_QP_GENERIC_NT must be 64, 128, 256, 512 or 1024"),
    "qp2_nt96": ({"UPR_QP_KERNEL": "2", "UPR_QP_NT": "96"}, _headline, {}, "UPR_QP_NT must be 64, 128 or 256"),
}

# screens that need more than 1e-8 (relative to max(1, max |dx|, |du|)): 3 x the value measured against the emulation, and its cause
# (none: the largest of the table is 6.95e-9, du of fallback_no_jit_N12 -- the target 2.2 m away at a horizon of 1.2 s, max |dx| 9.9)
TOL = {
}
# the reported residuals against the emulation's, relative to themselves + 1e-9: measured at most 3.1e-7 (fallback_N65_soft); where more,
# 3 x the measured value and the cause.  One cause for all of them, and it is not a race: one body on four frictionless contacts.  After
# six iterations its stationarity residual sits at 1e-12 ... 3e-11 -- terms of order one that cancel; the other three residuals agree to
# 1e-6 and better, the steps to 2e-11 -- so the rounding of the last sums, 2e-12 ... 2e-11 absolute, is 1e-3 ... 2e-2 of the 1e-9 floor.
# The host emulation built with and without FMA contraction parts from itself by as much on the same records (thing_demo 8.4e-3,
# ur10 N 10 1.8e-3, 9,1,4,1 3.4e-3, 6,1,4,1 1.5e-2), and the 64-, 128- and 256-lane forms give the same figure to three digits.
RES_TOL = {
    "generic_thing_demo": 3.7e-2,      # measured 1.23e-2
    "generic_ur10_N10": 3.2e-3,        # measured 1.06e-3
    "qp2_9x1x4x1_nt64": 4.9e-2, "qp2_9x1x4x1_nt128": 4.9e-2, "qp2_9x1x4x1_nt256": 4.9e-2,      # measured 1.62e-2 at all three
    "qp2_6x1x4x1_nt64": 3.1e-2, "qp2_6x1x4x1_nt128": 3.1e-2, "qp2_6x1x4x1_nt256": 3.1e-2,      # measured 1.02e-2 at all three
}

def _at_rest(c):
    """Every instance at the config's own start state, joint rates zero.  A hard object-dynamics equality on frictionless contacts
    (nfc 4 < ne 6, no soft_eq) holds no tangential load: with the builders' perturbed joint rates the FIXED first knot violates it by
    3e-3 to 6e-2 whatever the step, every kernel (the production one too) ends at its iteration cap and there is no point to check."""
    nq = c["P"].nq
    c["x0"] = np.ascontiguousarray(c["x0"]); c["x0"][:, nq:2 * nq] = 0.0
    c["xs0"], c["us0"] = (np.ascontiguousarray(a) for a in stationary_guess(c["x0"], c["P"].N, c["P"].nu))
    return c


def _near_target(c):
    """The target 0.4 m from the start: the headline's 2.2 m cannot be reached in a horizon of 1.2 s (N = 12), the terminal
    equality of that QP has no solution and every kernel ends at its cap."""
    from upright_amd.sampling import waypoints_for
    c["way"] = waypoints_for(c["P"], c["x0"], offset=(-0.3, 0.3, 0.0))
    return c


# the converged leg: one case per distinct (structure, shape) -> (does tests/kkt_check.py take the problem class?, what the converged
# run changes in the case's inputs so that its QP has a solution).  kkt_check has no end-effector box rows: fallback_26_rows is compared
# with nothing there (the rows themselves are tests/test_gpu_ee_box.py's).
CONVERGED = {
    "generic_headline": (True, None), "generic_rows": (True, None), "generic_rows_soft": (True, None), "generic_soft_boxes": (True, None),
    "generic_thing_demo": (True, None), "generic_ur10_N10": (True, _at_rest), "generic_dice": (True, None), "generic_box_arch": (True, None),
    "generic_cups": (True, None), "generic_robust": (True, None),
    "fallback_N65": (True, None), "fallback_N65_soft": (True, None), "fallback_26_rows": (False, None), "fallback_no_jit_N12": (True, _near_target),
    "qp2_9x1x4x3_nt128": (True, None), "qp2_9x1x4x1_nt128": (True, _at_rest), "qp2_6x1x4x1_nt128": (True, _at_rest), "qp2_6x1x4x3_nt128": (True, None),
    "qp2_9x2x8x3_nt128": (True, None),
}
# ... and the cases among them that the production kernel takes too under default knobs (the twin holds emu_qp_select against it)
ALSO_PRODUCTION = [n for n in CONVERGED if not n.startswith("fallback_")]


def converged_case(name):
    c = build_case(name)
    adjust = CONVERGED[name][1]
    return adjust(c) if adjust else c


def build_case(name, **kw):
    """dict(P, x0, way, bp, xs0, us0, B) of a case; kw: qp_tol / qp_iter_max where the screen fixes them"""
    builder, bkw, _, _, _ = CASES[name]
    c = builder(**{k: v for k, v in bkw.items() if k != "iters"}, **kw)
    P, x0 = c["P"], c["x0"]
    B = x0.shape[0]
    bp = c.get("bp")
    if bp is None:
        bp = np.broadcast_to(P.body_params, (B,) + np.shape(P.body_params))
    xs0, us0 = stationary_guess(x0, P.N, P.nu)
    return dict(P=P, x0=x0, way=c["way"], bp=np.ascontiguousarray(bp, dtype=np.float64), xs0=np.ascontiguousarray(xs0), us0=np.ascontiguousarray(us0), B=B)


def emulate(structure, P, B, xs, us, x0, lin, bp):
    """The generic kernel's (emu_qp) or the second structure's (emu_qp2) body on the host, NaN in every double of the instance
    workspace before the solve: dx [B][N+1][nx], du [B][N][nu], stats [B][NSTATS], the workspace [B][stride]."""
    from test_emu import Emu
    e = Emu(P, B, bp=bp)
    p = _capi.ptr
    xs = np.ascontiguousarray(xs[:, :, :e.nx]); us = np.ascontiguousarray(us); x0 = np.ascontiguousarray(x0[:, :e.nx]); lin = np.ascontiguousarray(lin)
    stats = np.zeros((B, _capi.NSTATS))
    if structure == GENERIC:
        ws = np.full((B, e.ws_stride), np.nan)
        e.E.emu_qp(C.byref(e.cp), B, p(xs), p(us), p(x0), p(lin), p(e.Df), p(ws), p(stats))
    else:
        assert structure == SECOND, structure
        need = e.E.emu_qp2(C.byref(e.cp), B, None, None, None, None, None, None, C.c_long(0), None)
        assert need > 0, need
        ws = np.full((B, need), np.nan)
        assert e.E.emu_qp2(C.byref(e.cp), B, p(xs), p(us), p(x0), p(lin), p(e.Df), p(ws), C.c_long(need), p(stats)) == 0
    n1, N = P.N + 1, P.N
    return ws[:, e.ws_dx:e.ws_dx + n1 * e.nx].reshape(B, n1, e.nx), ws[:, e.ws_du:e.ws_du + N * e.nu].reshape(B, N, e.nu), stats, ws


def compare(dxs, dus, res, iters, status, dxe, due, se):
    """The screen's figures of one case: (dx, du relative to max(1, max |.|), residuals relative to themselves + 1e-9); iteration counts
    and status asserted equal"""
    assert np.all(np.isfinite(dxe)) and np.all(np.isfinite(due))
    assert np.array_equal(iters, se[:, 1]) and np.array_equal(status, se[:, 2]), (iters, status, se[:, 1], se[:, 2])
    ex = np.abs(dxs - dxe).max() / max(1.0, np.abs(dxe).max())
    eu = np.abs(dus - due).max() / max(1.0, np.abs(due).max())
    er = (np.abs(res - se[:, 6:10]) / (np.abs(se[:, 6:10]) + 1e-9)).max()
    return float(ex), float(eu), float(er)


def _set_env(monkeypatch, env):
    for k in ("UPR_QP_KERNEL", "UPR_QP_GENERIC", "UPR_QP_NT", "UPR_QP_GENERIC_NT", "UPR_QP3_JIT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _kernel_name(mpc):
    return mpc.kernel_times()["qp_kernel"].replace("  ", " ")


@pytest.mark.parametrize("name", list(CASES))
def test_fallback_kernel_fixed_iterations_vs_host_emulation(name, monkeypatch):
    _, _, env, structure, kernel = CASES[name]
    _set_env(monkeypatch, env)
    c = build_case(name, qp_tol=0.0, qp_iter_max=ITERS)
    P, B = c["P"], c["B"]
    mpc = BatchMPC(P, B, body_params=c["bp"], way_p=c["way"])
    try:
        assert _kernel_name(mpc) == kernel, (_kernel_name(mpc), kernel)      # (without this a case could run the production kernel)
        mpc.set_observation(0.0, c["x0"])
        mpc.set_guess(c["xs0"], c["us0"])
        dxs, dus = mpc.qp_step()
        st = mpc.stats()
        lin = mpc.lin_records()
    finally:
        mpc.close()
    dxe, due, se, _ = emulate(structure, P, B, c["xs0"], c["us0"], c["x0"], lin, c["bp"])
    assert np.all(se[:, 1] == ITERS) or np.any(se[:, 2] == 2)
    res = np.stack([st[k] for k in ("qp_res_stat", "qp_res_eq", "qp_res_ineq", "qp_res_comp")], axis=1)
    ex, eu, er = compare(dxs[:, :, :P.nx], dus, res, st["qp_iters_last"], st["qp_status_last"], dxe, due, se)
    tol, res_tol = TOL.get(name, 1e-8), RES_TOL.get(name, 1e-4)
    print("fallback screen %s [%s]: dx %.2e du %.2e res %.2e (tolerances %.0e, %.1e)" % (name, kernel, ex, eu, er, tol, res_tol))
    assert tol <= 1e-6
    # (a race shows up at 1e-3 and above)
    assert ex < tol and eu < tol, (ex, eu)
    assert er < res_tol, er


@pytest.mark.parametrize("name", list(REFUSED))
def test_lane_counts_the_launchers_refuse(name, monkeypatch):
    """A lane count outside a launcher's list ends the QP launch with the launcher's message; nothing is launched."""
    env, builder, kw, message = REFUSED[name]
    _set_env(monkeypatch, env)
    c = builder(**kw)
    mpc = BatchMPC(c["P"], c["x0"].shape[0], way_p=c["way"])
    try:
        mpc.set_observation(0.0, c["x0"])
        with pytest.raises(RuntimeError, match=message):
            mpc.qp_step()
    finally:
        mpc.close()


def converged_point(c, env, monkeypatch, kernel=None):
    """One QP at the problem's own tolerances on a fresh handle: (qp_kkt() dict, lin records, stats, kernel name)"""
    _set_env(monkeypatch, env)
    mpc = BatchMPC(c["P"], c["B"], body_params=c["bp"], way_p=c["way"])
    try:
        ran = _kernel_name(mpc)
        assert kernel is None or ran == kernel, (ran, kernel)
        mpc.set_observation(0.0, c["x0"])
        mpc.set_guess(c["xs0"], c["us0"])
        sol = mpc.qp_kkt()
        lin = mpc.lin_records()
        st = mpc.stats()
    finally:
        mpc.close()
    return sol, lin, st, ran


def kkt_of(c, sol, lin, which):
    """tests/kkt_check.py on the instances `which` (each with its own inertial parameters): the worst of the four residuals, [4]"""
    from kkt_check import kkt_residuals
    P, nx = c["P"], c["P"].nx
    worst = np.zeros(4)
    for b in which:
        Pb = copy.copy(P); Pb.body_params = c["bp"][b]
        s = {k: v[b] for k, v in sol.items()}
        s["dx"] = s["dx"][:, :nx]
        worst = np.maximum(worst, kkt_residuals(Pb, c["bp"][b], c["x0"][b][:nx], c["xs0"][b][:, :nx], c["us0"][b], lin[b], s))
    return worst


def step_difference(P, sol, ref, which):
    """dx and du of the instances `which` against another kernel's, relative to max(1, max |.|) of the other's"""
    dx, du, rx, ru = sol["dx"][which][:, :, :P.nx], sol["du"][which], ref["dx"][which][:, :, :P.nx], ref["du"][which]
    return float(np.abs(dx - rx).max() / max(1.0, np.abs(rx).max())), float(np.abs(du - ru).max() / max(1.0, np.abs(ru).max()))


@pytest.mark.parametrize("name", list(CONVERGED))
def test_fallback_kernel_converged_point_is_a_kkt_point(name, monkeypatch):
    """The only check on where these kernels leave pi, nu, y_N, lam in the instance workspace (o_* of upr_qp_fill_generic and
    upr_qp2_fill; the value function and the gain gather read them): the converged point at the problem's own tolerances is a KKT
    point of the sub-problem assembled in numpy (kkt_check's 1e-7), and the step is the production kernel's (2e-5, the figure of the
    production-against-generic comparison of tests/test_gpu_parity.py) wherever that kernel takes the problem."""
    _, _, env, structure, kernel = CASES[name]
    c = converged_case(name)
    P = c["P"]
    sol, lin, st, _ = converged_point(c, env, monkeypatch, kernel)
    # (generic_rows: the obstacle stands inside the reach of the hard linearised rows of instances 0 and 2 -- that QP has no solution
    # and every kernel ends at its cap on them; the other two instances are the case.  Everywhere else every instance converges.)
    which = np.flatnonzero(st["qp_status_last"] == 0)
    assert len(which) == (2 if name == "generic_rows" else c["B"]), (st["qp_status_last"], st["qp_iters_last"])
    if CONVERGED[name][0]:
        res = kkt_of(c, sol, lin, which)
        print("fallback converged %s [%s]: KKT stat %.2e eq %.2e ineq %.2e comp %.2e" % ((name, kernel) + tuple(res)))
        assert res.max() < 1e-7, res
    if name in ALSO_PRODUCTION:
        ref, _, st3, ran = converged_point(c, {}, monkeypatch)
        assert ran.startswith("upr_qp3_"), ran
        assert np.array_equal(np.flatnonzero(st3["qp_status_last"] == 0), which), (st3["qp_status_last"], which)
        ex, eu = step_difference(P, sol, ref, which)
        print("fallback converged %s against %s: dx %.2e du %.2e" % (name, ran, ex, eu))
        assert ex < 2e-5 and eu < 2e-5, (ex, eu)
