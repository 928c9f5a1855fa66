"""Helpers of the cost-to-go screen (tests/test_vf_reference.py on the host, tests/test_gpu_vf_screen.py on the device): the body of
upr_value_kernel (upright_amd/csrc/upr_value.h) against the dense reference of tests/fb_check.py, which returns the cost-to-go
matrices P_k of the same recursion out of a dense quasi-definite solve per knot -- no Cholesky factor of Hff, no Schur complement on
the forces, none of the kernel's code and none of the host module's (upright_amd/value_function.py).

pack_point lays a primal-dual point out for the kernel with offsets of its own: blocks in another order than the production kernel's
export or the workspaces of the other QP kernels, NaN between and around them, the step in a workspace row that holds nothing else.
The emulated kernel (emu_vf_cost_to_go takes every offset as an argument) therefore runs at any shape from a point in the layout
of BatchMPC.qp_kkt() / qp_slack_pairs(), and an offset taken from the wrong place reads NaN."""
import ctypes as C
import os
from pathlib import Path

import numpy as np

import fb_check
from kkt_check import force_jacobian
from upright_amd import _capi
from upright_amd.value_function import slot_layout

HERE = Path(__file__).resolve().parent
GAP = 5      # NaN doubles between the blocks of a packed point


def emu_dims(P):
    """dict(nx, nu, ne, nfc, ws_dx, ws_du) of upr_make_dims for P (tests/emu/upr_emu.cpp: emu_dims)."""
    E = C.CDLL(os.environ.get("UPR_EMU_LIB", str(HERE / "emu" / "libupr_emu.so")))
    d = (C.c_int * 16)()
    cp = _capi.problem_to_c(P)
    E.emu_dims(C.byref(cp), d)
    return dict(nx=d[0], nu=d[1], ne=d[2], ws_dx=d[6], ws_du=d[7], nfc=d[13])


def contracted_library():
    """tests/emu/upr_vf_emu.cpp built with the host compiler's FMA contraction on (libupr_vf_emu_fma.so: the build makes it where the
    host has the instruction), or None.  The plain emulation rounds every product; hipcc contracts a * b + c on the device, and over a
    21-knot recursion with cond(M) 1e6 .. 4e7 the two orders of rounding part by 3e-10 .. 1.2e-8 of a knot's largest entry.  This
    build parts from the plain one by those same figures, case by case, so the device is held against it at 1e-10."""
    lib = HERE / "emu" / "libupr_vf_emu_fma.so"
    try:
        has_fma = " fma " in Path("/proc/cpuinfo").read_text().replace("\n", " ")
    except OSError:
        has_fma = False
    return C.CDLL(str(lib)) if has_fma and lib.exists() else None


def run_cost_to_go(V, e, xs, us, lin, raw):
    """emu_vf_cost_to_go of the library V (test_value_function_batched._emu_cost_to_go, which runs the plain build) for the instances
    of the Emu e: dict(Pk, pk, J, X), pre-filled with NaN."""
    ws, mult, offs = raw
    P, B = e.P, e.B
    n1, nx = P.N + 1, e.nx
    p, ip = _capi.ptr, _capi.iptr
    out = dict(Pk=np.full((B, n1, nx, nx), np.nan), pk=np.full((B, n1, nx), np.nan), J=np.full((B, n1), np.nan), X=np.full((B, n1, nx), np.nan))
    V.emu_vf_cost_to_go(C.byref(e.cp), B, p(xs), p(us), p(lin), p(e.Df), p(ws), C.c_long(ws.shape[1]), p(mult), C.c_long(mult.shape[1]),
                        ip(offs), p(out["Pk"]), p(out["pk"]), p(out["J"]), p(out["X"]))
    return out


def pack_point(P, sols, pairs, dx, du):
    """The kernel's inputs for B instances: (ws [B][stride], mult [B][mstride], offs int32[8]) with offs = o_pi, o_nu, o_lam, o_t,
    o_sig, o_tau, o_gam (-1: no softened inequality rows), ni as emu_vf_cost_to_go takes them.
    sols[b]: dict(pi [N+1][nx], nu [N][ne], lam, slack [N+1][ni]) -- BatchMPC.qp_kkt() sliced to the instance, or the `sol` of
    fb_check.emu_qp3_cfg_fb; pairs[b]: (sigma, tau, gam) [N+1][ni] each or None; dx [B][N+1][>= nx], du [B][N][nu]."""
    d = emu_dims(P)
    nx, nu, ne, N = d["nx"], d["nu"], d["ne"], P.N
    B = len(sols)
    ni = np.asarray(sols[0]["lam"]).shape[1]
    soft = pairs[0] is not None
    assert all((q is not None) == soft for q in pairs)
    # blocks in an order of their own: t, gam, nu, lam, sigma, pi, tau
    sizes = dict(t=(N + 1) * ni, gam=(N + 1) * ni if soft else 0, nu=N * ne, lam=(N + 1) * ni, sig=(N + 1) * ni if soft else 0,
                 pi=(N + 1) * nx, tau=(N + 1) * ni if soft else 0)
    off, o = {}, GAP
    for name, n in sizes.items():
        off[name] = o if n else -1
        o += n + (GAP if n else 0)
    mult = np.full((B, o), np.nan)
    stride = max(d["ws_dx"] + (N + 1) * nx, d["ws_du"] + N * nu) + GAP
    ws = np.full((B, stride), np.nan)
    for b in range(B):
        s = sols[b]
        blocks = dict(t=s["slack"], nu=s["nu"], lam=s["lam"], pi=s["pi"])
        if soft:
            blocks.update(sig=pairs[b][0], tau=pairs[b][1], gam=pairs[b][2])
        for name, v in blocks.items():
            v = np.asarray(v, dtype=np.float64).reshape(-1)
            assert v.size == sizes[name], (name, v.size, sizes[name])
            mult[b, off[name]:off[name] + v.size] = v
        ws[b, d["ws_dx"]:d["ws_dx"] + (N + 1) * nx] = np.asarray(dx[b])[:, :nx].reshape(-1)
        ws[b, d["ws_du"]:d["ws_du"] + N * nu] = np.asarray(du[b]).reshape(-1)
    offs = np.array([off["pi"], off["nu"], off["lam"], off["t"], off["sig"], off["tau"], off["gam"], ni], dtype=np.int32)
    return ws, mult, offs


def cost_to_go_reference(P, lin, sol, pairs, bp, extended=False, first=0):
    """P_k [N + 1 - first][nx][nx], knots first .. N, of the QP whose interior-point iteration factors the point (sol, pairs) of one
    instance: fb_check.feedback_reference's second output (float64, or 50 digits with extended=True)."""
    return fb_check.feedback_reference(P, lin, sol, fb_check.friction_rows_of(P), force_jacobian(P, bp), pairs=pairs, first=first,
                                       extended=extended)[1]


def pk_errors(Pk, P_ref):
    """err[knots]: max |P - P_ref| of every knot relative to that knot's max |P_ref| (test_value_function_batched.rel_err's
    convention, one figure per knot; works on float64 and on extended-precision object arrays)."""
    P_ref = np.asarray(P_ref)
    Pk = np.asarray(Pk)
    assert Pk.shape == P_ref.shape, (Pk.shape, P_ref.shape)
    out = np.zeros(P_ref.shape[0])
    for k in range(P_ref.shape[0]):
        scale = max(abs(v) for v in P_ref[k].reshape(-1))
        assert scale > 0, "knot %d: the reference matrix is identically zero" % k
        out[k] = float(max(abs(v) for v in (Pk[k] - P_ref[k]).reshape(-1)) / scale)
    return out


# ---- the kernel's own algebra in numpy ------------------------------------------------------------------------------------------------------
def schur_cholesky_statement(P, lin, sol, pairs, bp):
    """P_k [N+1][nx][nx] by the factorisation upr_vf_instance uses, in float64 numpy and in none of its code: the forces eliminated
    through the Cholesky factor of Hff, S = Df Hff^-1 Df' + rho I formed explicitly and factored by a second Cholesky, the jerks
    through the Cholesky factor of Rq + Bq' P+ Bq:  P_k = Hxx + A' P+ A - W'W + Y'Y,  W = Lq^-1 Bq' P+ A,  Y = Ls^-1 C.
    Where this lands next to the kernel against the 50-digit twin, the kernel's distance is the conditioning of that route (S is
    formed from the INVERSE of barrier weights that span many decades) and not a defect of its code."""
    from upright_amd.value_function import _dynamics, record_layout, slot_active
    nq, nx, nu, N, h = P.nq, P.nx, P.nu, P.N, float(P.dt)
    Df = force_jacobian(P, bp)
    E = fb_check.friction_rows_of(P)
    ne, nfc = Df.shape
    npoly, no = E.shape[0], fb_check.n_state_rows(P)
    o = record_layout(P)
    sl = P.slacks or {}
    _, _, _, _, upper, softened = slot_layout(P, npoly)
    w = np.asarray(sol["lam"], dtype=np.float64) / np.asarray(sol["slack"], dtype=np.float64)
    if pairs is not None:
        Zs = np.where(upper, float(sl.get("upper_L2_penalty", 100.0)), float(sl.get("lower_L2_penalty", 100.0)))
        w_s = np.asarray(pairs[2]) / np.asarray(pairs[1])
        w = np.where(slot_active(P, npoly) & softened, w * (Zs + w_s) / (Zs + w + w_s), w)
    if bool(sl.get("equality", sl.get("poly_ineq"))):
        rho = 1.0 / float(sl.get("lower_L2_penalty", 100.0))
    else:
        rho = fb_check.RHO_PROX if nfc < ne else fb_check.RHO_FULL
    A, Bq = _dynamics(nq, h)
    iu = np.triu_indices(nq)
    o_u, o_p, o_o = 2 * nx, 2 * nx + 2 * nu, 2 * nx + 2 * nu + npoly
    Pn = np.diag(w[N][:nx] + w[N][nx:2 * nx])
    if P.terminal_constraint:
        CN = np.zeros((3 + 2 * nq, nx)); CN[:3, :nq] = -lin[N][o["hess"]:o["hess"] + 3 * nq].reshape(3, nq); CN[3:, nq:] = np.eye(2 * nq)
        Pn = Pn + CN.T @ CN / fb_check.RHO_N
    out = [Pn]
    for k in range(N - 1, -1, -1):
        rec, wk = lin[k], w[k]
        Hee = np.zeros((nq, nq)); Hee[iu] = rec[o["hess"]:o["hess"] + o["nh"]]; Hee = Hee + np.triu(Hee, 1).T
        Hxx = h * np.diag(np.asarray(P.Qdiag, dtype=float)); Hxx[:nq, :nq] += h * Hee
        if k >= 1:
            Hxx += np.diag(wk[:nx] + wk[nx:2 * nx])
            if no:
                Jo = rec[o["obs"] + no:o["obs"] + no + no * nq].reshape(no, nq)
                Hxx[:nq, :nq] += Jo.T @ (wk[o_o:o_o + no, None] * Jo)
        Huu = np.diag(h * np.asarray(P.Rdiag, dtype=float) + wk[o_u:o_u + nu] + wk[o_u + nu:o_u + 2 * nu])
        Hff = Huu[nq:, nq:].copy()
        if npoly:
            Hff += E.T @ (wk[o_p:o_p + npoly, None] * E)
        C = rec[o["gx"]:o["gx"] + ne * nx].reshape(ne, nx)
        YF = np.linalg.solve(np.linalg.cholesky(Hff), Df.T)
        S = YF.T @ YF + rho * np.eye(ne)
        Y = np.linalg.solve(np.linalg.cholesky(S), C)
        BP = Bq.T @ Pn
        W = np.linalg.solve(np.linalg.cholesky(Huu[:nq, :nq] + BP @ Bq), BP @ A)
        Pk = Hxx + A.T @ Pn @ A - W.T @ W + Y.T @ Y
        Pn = 0.5 * (Pk + Pk.T)
        out.append(Pn)
    return np.array(out[::-1])


# ---- input controls: what the comparison must be able to see, computed on the reference alone -------------------------------------------
def state_row_slots(P, ni):
    """Slots of the state rows (collision pairs, projectile, end-effector box) in a knot's inequality block."""
    no = fb_check.n_state_rows(P)
    return slice(ni - no, ni) if no else slice(0, 0)


def control_wrong_iterate(P, lin, sol, pairs, sol_next, pairs_next, bp, P_ref=None):
    """How far the reference moves when it is fed the point of one more interior-point iteration: max over the knots."""
    P_ref = cost_to_go_reference(P, lin, sol, pairs, bp) if P_ref is None else P_ref
    return float(pk_errors(cost_to_go_reference(P, lin, sol_next, pairs_next, bp), P_ref).max())


def control_zeroed_state_rows(P, lin, sol, pairs, bp, P_ref=None):
    """... when the barrier weights of the state-row slots are set to zero (lam = 0 there)."""
    P_ref = cost_to_go_reference(P, lin, sol, pairs, bp) if P_ref is None else P_ref
    lam = np.array(sol["lam"], dtype=np.float64)
    rows = state_row_slots(P, lam.shape[1])
    assert rows.stop > rows.start, "the problem has no state rows"
    lam[:, rows] = 0.0
    return float(pk_errors(cost_to_go_reference(P, lin, dict(sol, lam=lam), pairs, bp), P_ref).max())


def control_without_pairs(P, lin, sol, pairs, bp, P_ref=None):
    """... when the softened rows enter with lam / t in place of the effective weight w0 (Z + w_s) / (Z + w0 + w_s)."""
    assert pairs is not None and slot_layout(P)[5].any()
    P_ref = cost_to_go_reference(P, lin, sol, pairs, bp) if P_ref is None else P_ref
    return float(pk_errors(cost_to_go_reference(P, lin, sol, None, bp), P_ref).max())
