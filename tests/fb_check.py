"""Dense reference for the linear feedback gains of one QP instance (sqp.use_feedback_policy: u = u* + K (x - x*)), in numpy.

Inputs: the linearisation records of the instance, a primal-dual point of its QP in the layout of BatchMPC.qp_kkt() (with
qp_slack_pairs() where inequality rows are softened), the friction rows E and d(object dynamics)/d(forces) Df.  From the barrier
weights of that point it builds, knot by knot and backward from N, the stage system an interior-point iteration AT that point factors,

    M [K_u; K_nu] = G,    M = [[Huu + B' P+ B, D'], [D, -rho I]],    G = [B' P+ A; C],    P = Hxx + A' P+ A - G' M^-1 G

and returns K_k = -K_u (ocs2 sign): jerk rows [:nq] and contact-force rows [nq:] out of the SAME solve.  Nothing here uses the
oracle's interior-point code or a factor of the kernels (no Cholesky of Hff, no Schur complement S, no 6 x 6 blocks): M is assembled
dense and handed to numpy.linalg.solve.  Taken from upright_amd/value_function.py and the header comments of upr_qp.h / upr_qp3.h:
the weights w = lam / t, the soft-row rule w0 (Z + w_s) / (Z + w0 + w_s), rho = 1 / Z for a softened equality (the penalty
Z/2 |C dx + Df df|^2 written with its multiplier), 1e-6 where the forces cannot span the rows, 1e-12 otherwise, and rho_N = 1e-6 of
the terminal equality.

`extended=True` runs the same statements in mpmath (50 digits) on object arrays: the rounding error of the float64 reference is
measured against it.  Its linear solve is Gaussian elimination in the given order (primal block first) that skips zeros -- M is
quasi-definite, every order has its pivots, and at 50 digits the growth of an unpivoted elimination is of no account -- so that a
21-knot recursion of the largest shape (135-square M, 27 right-hand sides) stays at seconds."""
import numpy as np

from upright_amd.value_function import record_layout, slot_active, slot_layout

RHO_N = 1e-6
RHO_PROX = 1e-6
RHO_FULL = 1e-12
MP_DIGITS = 50


def _to_mp(a):
    import mpmath
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for i, v in enumerate(a.reshape(-1)):
        flat[i] = mpmath.mpf(float(v))        # (exact: every double is a 53-bit binary fraction)
    return out


def _mm(X, Y):
    """X @ Y; on object arrays over the non-zeros of both factors (the dynamics, selector and friction matrices are mostly zero)."""
    if X.dtype != object:
        return X @ Y
    out = np.zeros((X.shape[0], Y.shape[1]), dtype=object)
    nz = [np.array([c for c in range(Y.shape[1]) if Y[k, c] != 0], dtype=int) for k in range(Y.shape[0])]
    for i in range(X.shape[0]):
        row = X[i]
        for k in range(X.shape[1]):
            if len(nz[k]) and row[k] != 0:
                out[i, nz[k]] = out[i, nz[k]] + Y[k, nz[k]] * row[k]
    return out      # (array * scalar throughout: an mpf on the left of an array first tries to convert the array)


def _solve(M, G):
    if M.dtype != object:
        return np.linalg.solve(M, G)
    n = M.shape[0]
    W = np.hstack([M, G]).copy()
    nc = W.shape[1]
    for j in range(n):
        piv = W[j, j]
        cols = [c for c in range(j + 1, nc) if W[j, c] != 0]
        for i in range(j + 1, n):
            if W[i, j] != 0:
                f = W[i, j] / piv
                W[i, cols] = W[i, cols] - W[j, cols] * f
                W[i, j] = 0
    X = np.zeros((n, G.shape[1]), dtype=object)
    for j in range(n - 1, -1, -1):
        r = W[j, n:].copy()
        for c in range(j + 1, n):
            if W[j, c] != 0:
                r = r - X[c] * W[j, c]
        X[j] = r / W[j, j]
    return X


def n_state_rows(P):
    return len(P.pair_a) + len(P.proj_sph) + (6 if getattr(P, "ee_box", False) else 0)


def feedback_reference(P, lin, sol, E, Df, pairs=None, first=0, extended=False):
    """Gains of the QP whose interior-point iteration factors the point `sol` (dict with lam, slack [N+1][ni]; pairs = (sigma, tau,
    gam)[N+1][ni] or None), knots first .. N-1 (the recursion runs backward from N: a tail is exact without the rest).
    Returns (K[N-first][nu][nx], Pk[N+1-first][nx][nx], cond[N-first]): index 0 is knot `first`; cond: the 2-norm condition number of
    M per knot (float64 run; None with extended=True)."""
    nq, nx, nu, N, h = P.nq, P.nx, P.nu, P.N, float(P.dt)
    ne, nfc = Df.shape
    npoly = E.shape[0]
    no = n_state_rows(P)
    o = record_layout(P)
    cv = _to_mp if extended else (lambda a: np.asarray(a, dtype=np.float64))
    if extended:
        import mpmath
        mpmath.mp.dps = MP_DIGITS
    one = cv(1.0)[()]
    sl = P.slacks or {}
    _, _, _, _, upper, softened = slot_layout(P, npoly)
    # ---- barrier weights of the point
    lam, t = cv(sol["lam"]), cv(sol["slack"])
    w = lam / t
    if pairs is not None:
        ZU, ZL = float(sl.get("upper_L2_penalty", 100.0)), float(sl.get("lower_L2_penalty", 100.0))
        on = slot_active(P, npoly) & softened
        tau, gam = cv(pairs[1]), cv(pairs[2])
        for k, j in zip(*np.nonzero(on)):
            Z = cv(ZU if upper[j] else ZL)[()]
            w_s = gam[k, j] / tau[k, j]
            w[k, j] = w[k, j] * (Z + w_s) / (Z + w[k, j] + w_s)
    soft_eq = bool(sl.get("equality", sl.get("poly_ineq")))
    if soft_eq:
        rho = one / cv(float(sl.get("lower_L2_penalty", 100.0)))[()]
    else:
        rho = cv(RHO_PROX if nfc < ne else RHO_FULL)[()]
    # ---- constants: triple-integrator dynamics, forces outside them; D = [0 Df]
    hh = cv(h)[()]
    A = np.zeros((nx, nx), dtype=object if extended else float); B = np.zeros((nx, nu), dtype=A.dtype)
    for i in range(nq):
        A[i, i] = A[nq + i, nq + i] = A[2 * nq + i, 2 * nq + i] = one
        A[i, nq + i] = A[nq + i, 2 * nq + i] = hh
        A[i, 2 * nq + i] = hh * hh / 2
        B[i, i] = hh * hh * hh / 6; B[nq + i, i] = hh * hh / 2; B[2 * nq + i, i] = hh
    D = np.zeros((ne, nu), dtype=A.dtype); D[:, nq:] = cv(Df)
    Em = cv(E)
    Q, R = cv(np.asarray(P.Qdiag, dtype=float)), cv(np.asarray(P.Rdiag, dtype=float))
    iu = np.triu_indices(nq)
    o_x, o_u, o_p, o_o = 0, 2 * nx, 2 * nx + 2 * nu, 2 * nx + 2 * nu + npoly
    # ---- terminal knot
    Pn = np.zeros((nx, nx), dtype=A.dtype)
    for i in range(nx):
        Pn[i, i] = w[N][o_x + i] + w[N][o_x + nx + i]
    if P.terminal_constraint:
        CN = np.zeros((3 + 2 * nq, nx), dtype=A.dtype)
        CN[:3, :nq] = -cv(lin[N][o["hess"]:o["hess"] + 3 * nq].reshape(3, nq))
        for i in range(2 * nq):
            CN[3 + i, nq + i] = one
        Pn = Pn + _mm(CN.T.copy(), CN) / cv(RHO_N)[()]
    Ks, Ps, conds = [], [Pn], []
    for k in range(N - 1, first - 1, -1):
        rec, wk = lin[k], w[k]
        Hxx = np.zeros((nx, nx), dtype=A.dtype)
        Hee = np.zeros((nq, nq), dtype=A.dtype); Hee[iu] = cv(rec[o["hess"]:o["hess"] + o["nh"]])
        Hee = Hee + np.triu(Hee, 1).T
        Hxx[:nq, :nq] = Hee * hh
        for i in range(nx):
            Hxx[i, i] = Hxx[i, i] + hh * Q[i]
        if k >= 1:     # (x_0 is fixed: knot 0 carries no state rows)
            for i in range(nx):
                Hxx[i, i] = Hxx[i, i] + wk[o_x + i] + wk[o_x + nx + i]
            if no:
                Jo = cv(rec[o["obs"] + no:o["obs"] + no + no * nq].reshape(no, nq))
                Hxx[:nq, :nq] = Hxx[:nq, :nq] + _mm(Jo.T.copy(), wk[o_o:o_o + no, None] * Jo)
        Huu = np.zeros((nu, nu), dtype=A.dtype)
        for i in range(nu):
            Huu[i, i] = hh * R[i] + wk[o_u + i] + wk[o_u + nu + i]
        if npoly:
            Huu[nq:, nq:] = Huu[nq:, nq:] + _mm(Em.T.copy(), wk[o_p:o_p + npoly, None] * Em)
        C = cv(rec[o["gx"]:o["gx"] + ne * nx].reshape(ne, nx))
        BtP = _mm(B.T.copy(), Pn)
        M = np.zeros((nu + ne, nu + ne), dtype=A.dtype)
        M[:nu, :nu] = Huu + _mm(BtP, B)
        M[:nu, nu:] = D.T; M[nu:, :nu] = D
        for i in range(ne):
            M[nu + i, nu + i] = -rho
        G = np.vstack([_mm(A.T.copy(), BtP.T.copy()).T, C])
        X = _solve(M, G)
        AtP = _mm(A.T.copy(), Pn)                                  # (the sparse factor on the left both times: P+ is symmetric)
        Pk = Hxx + _mm(A.T.copy(), AtP.T.copy()).T - _mm(G.T.copy(), X)
        Pk = (Pk + Pk.T) / 2
        Ks.append(-X[:nu]); Ps.append(Pk)
        if not extended:
            conds.append(np.linalg.cond(M))
        Pn = Pk
    return np.array(Ks[::-1]), np.array(Ps[::-1]), (None if extended else np.array(conds[::-1]))


def block_errors(K, K_ref, nq):
    """err[N][2]: max |K - K_ref| over the jerk rows [:nq] and over the force rows [nq:] of every knot, relative to that block's
    max |K_ref|.  A block whose reference is identically zero is an error of the case's inputs."""
    K_ref = np.asarray(K_ref)
    out = np.zeros((K_ref.shape[0], 2))
    for k in range(K_ref.shape[0]):
        for j, rows in enumerate((slice(0, nq), slice(nq, None))):
            ref = K_ref[k, rows]
            scale = max(abs(v) for v in ref.reshape(-1))
            assert scale > 0, "knot %d block %d: the reference gains are identically zero" % (k, j)
            d = np.asarray(K)[k, rows] - ref
            out[k, j] = float(max(abs(v) for v in d.reshape(-1)) / scale)
    return out


# ---- the emulated production kernel with both exits (tests/emu/upr_emu.cpp: emu_qp3_cfg_fb) ------------------------------------------------
def export_layout(E, cp):
    import ctypes as C
    out = (C.c_int * 10)()
    E.emu_qp3_export_layout(C.byref(cp), out)
    return dict(zip(("stride", "o_pi", "o_nu", "o_yN", "o_lam", "o_t", "o_sig", "o_tau", "o_gam", "ni"), list(out)))


def split_point(P, lay, nx, ne, mult):
    """One instance's export buffer as (sol, pairs): the dictionaries of BatchMPC.qp_kkt() / qp_slack_pairs() sliced to it."""
    n1, N, ni = P.N + 1, P.N, lay["ni"]
    blk = lambda off: mult[off:off + n1 * ni].reshape(n1, ni)
    sol = dict(pi=mult[lay["o_pi"]:lay["o_pi"] + n1 * nx].reshape(n1, nx), nu=mult[lay["o_nu"]:lay["o_nu"] + N * ne].reshape(N, ne),
               lam=blk(lay["o_lam"]), slack=blk(lay["o_t"]))
    pairs = (blk(lay["o_sig"]), blk(lay["o_tau"]), blk(lay["o_gam"])) if lay["o_sig"] >= 0 else None
    return sol, pairs


def emu_qp3_cfg_fb(cfg, P, B, xs, us, x0, lin, bp, iters):
    """The production kernel's body at exactly instantiation cfg on the host for `iters` interior-point iterations (P.qp_tol = 0):
    dict(dx, du, stats, K [B][N][nu][nx], sol [B], pairs [B], Df [B][ne][nfc]).  The gains and the export are pre-filled with NaN: every
    entry must be written."""
    import copy
    import ctypes as C
    import os
    from pathlib import Path

    from upright_amd import _capi
    E = C.CDLL(os.environ.get("UPR_EMU_LIB", str(Path(__file__).resolve().parent / "emu" / "libupr_emu.so")))   # (as tests/test_emu.py)
    E.emu_qp3_cfg.restype = C.c_long
    E.emu_qp3_cfg_fb.restype = C.c_long
    P = copy.copy(P)
    P.qp_iter_max = int(iters)
    assert P.qp_tol == 0.0
    c = (C.c_int * 8)(*[int(v) for v in cfg])
    cp = _capi.problem_to_c(P)
    need = E.emu_qp3_cfg(c, None, B, None, None, None, None, None, None, C.c_long(0), None)
    assert need > 0, (cfg, need)
    dims = (C.c_int * 16)()
    E.emu_dims(C.byref(cp), dims)
    nx, nu, ne, ws_dx, ws_du, nfc = dims[0], dims[1], dims[2], dims[6], dims[7], dims[13]
    lay = export_layout(E, cp)
    N, n1 = P.N, P.N + 1
    ws = np.full((B, need), np.nan)
    stats = np.zeros((B, _capi.NSTATS))
    fb = np.full((B, N, nu, nx), np.nan)
    mult = np.full((B, lay["stride"]), np.nan)
    bp = np.ascontiguousarray(bp)
    Df = np.zeros((B, ne, nfc))
    E.emu_make_Df(C.byref(cp), B, _capi.ptr(bp), _capi.ptr(Df))
    xs = np.ascontiguousarray(xs[:, :, :nx]); us = np.ascontiguousarray(us); x0 = np.ascontiguousarray(x0[:, :nx])
    lin = np.ascontiguousarray(lin)
    rc = E.emu_qp3_cfg_fb(c, C.byref(cp), B, _capi.ptr(xs), _capi.ptr(us), _capi.ptr(x0), _capi.ptr(lin), _capi.ptr(Df),
                          _capi.ptr(ws), C.c_long(need), _capi.ptr(stats), _capi.ptr(fb), _capi.ptr(mult), C.c_long(lay["stride"]))
    assert rc == 0, (cfg, rc)
    assert np.all(np.isfinite(fb)), "gains: %d entries not written" % int((~np.isfinite(fb)).sum())
    # (the export too, but for the slot of pi_0: x_0 is fixed, the QP has no such multiplier, and the emulation's costate sums read
    #  state-row scratch of knot 0 that nothing writes -- value_function.py rebuilds the gradient at x_0 itself)
    written = np.isfinite(mult); written[:, lay["o_pi"]:lay["o_pi"] + nx] = True
    assert np.all(written), "export: %d entries not written" % int((~written).sum())
    pts = [split_point(P, lay, nx, ne, mult[b]) for b in range(B)]
    return dict(dx=ws[:, ws_dx:ws_dx + n1 * nx].reshape(B, n1, nx), du=ws[:, ws_du:ws_du + N * nu].reshape(B, N, nu), stats=stats, K=fb,
                sol=[s for s, _ in pts], pairs=[q for _, q in pts], Df=Df)


def friction_rows_of(P):
    from kkt_check import friction_rows
    return friction_rows(P) if P.nf == 3 else np.zeros((0, P.nf * P.nc))
