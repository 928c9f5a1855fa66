"""The expected linearisation record of every knot of a batch, stated in numpy on the oracle's terms, and its comparison with what
a linearisation kernel wrote (the device in trajectory or points mode, or the kernel source through the host emulation).

A case is dict(P, bp [B][nb][10], way [B][n_way][3], way_q [B][n_way][4] | None, t0 [B], xs [B][N+1][nx], us [B][N][nu],
dyn [B][9 n_dyn] | None, pflag [B] | None).  Instance b gets an Oracle of its own that carries bp[b], way[b] and way_q[b]; knot k
of instance b lies at the time t0[b] + k dt, the dynamic obstacles are predicted tau = k dt ahead of dyn[b].  The terms:
Oracle.eq_constraint (g, dg/dx), Oracle.stage_cost less the joint-space quadratic (cost, gradient and Gauss-Newton Hessian of the
end-effector term in q), Oracle.terminal_constraint, Oracle.obstacle_rows and, for the end-effector box (which the oracle does
not have), [p_d(t) + upper - p; p - (p_d(t) + lower)] with p and dp/dq out of Oracle.ee_kinematics.

Record layout (restated here, not read from the library):
    [g ne][gx ne nx][cost][grad nq][hess, packed upper triangle nq (nq + 1) / 2][d no][dd/dq no nq],   ne = 6 nb, nx = 3 nq,
    state rows in the slot order [pairs][projectile][box upper 3][box lower 3];
    terminal record (knot N): grad[0:3] = the target-position residual, hess[0 : 3 nq] = -C_N[:3, :nq] row-major.

Compared slots -- the ones a consumer reads (upr_qp*.h, upr_linesearch.h, upr_value.h):
  * knots 0 .. N-1: g, gx, cost, grad, hess (the QP kernels read all of them at every stage; the line search sums cost, g and the
    directional derivative grad' dx over knots 0 .. N-1; the value kernel reads grad and hess of knot 0 for its gradient in x_0);
  * knots 1 .. N-1: the state rows and their gradients.  Knot 0's rows are written but never read: x_0 is fixed, the QP kernels
    stage the rows for 1 <= k < N only, the line search sums them from k = 1 and the value kernel adds them for k >= 1;
  * knot N: grad[0:3] (QP right-hand side, the line search's terminal violation) and hess[0 : 3 nq] (the QP's terminal Jacobian).
    Nothing else of the terminal record is read (its g, gx, rows are not written; its cost slot is not summed).
compare() returns, per slot class, the largest error in units of the class's own scale with the instance and the knot where it
occurred; TOL holds the project's bounds in the same units.

The projectile-path row is the one slot whose fp64 value is not determined to rounding level by its inputs.  Its closest time is
what the reference's iteration leaves (projectile_path_constraint.h:12-45: Newton on the cubic from t = 0, at most 10 steps,
stopping test 1e-4), and in motion that iteration often ends at its step limit while still jumping about: every rounding error
of a step is then multiplied by the derivative f f'' / f'^2 of the Newton map of every later step, and the row is evaluated at a
time where the distance is not stationary.  Found by this screen on the thrown-ball case, instance 0, knot 4 (last update -1.76,
final time 1.591 s against the stationary point 0.654 s): the fp64 oracle is 2.06e-12 away from the same iteration in 50-digit
arithmetic and the device 5.1e-11 away from the oracle.  Neither side is wrong -- both run the reference's iteration -- so the
bound of such a slot is widened by projectile_allowance(): the forward rounding-error bound of the iteration in fp64 (4.97e-10
at that slot, below 1e-18 wherever the iteration converges, 0 where the time is clamped to 0), evaluated in 50-digit arithmetic
from the oracle's inputs alone.  compare(..., allowance=) subtracts it from the absolute error before the table's bound applies."""
import copy

import numpy as np

from oracle.oracle import Oracle

SLOTS = ("g", "gx", "cost", "grad", "hess", "rows", "row_grad", "term_c", "term_C")
# g, gx, cost: relative to max(1, |reference|_inf of the knot's slot); the others absolute
TOL = dict(g=1e-11, gx=1e-10, cost=1e-11, grad=1e-11, hess=1e-11, term_c=1e-11, term_C=1e-11, rows=1e-13, row_grad=1e-12)
RELATIVE = ("g", "gx", "cost")


def dims(P):
    nq, nb = P.nq, P.nb
    ne, nx = 6 * nb, 3 * nq
    o_gx = ne
    o_cost = o_gx + ne * nx
    o_grad = o_cost + 1
    o_hess = o_grad + nq
    o_rows = o_hess + nq * (nq + 1) // 2
    nsr = len(P.pair_a) + len(P.proj_sph)
    no = nsr + (6 if P.ee_box else 0)
    return dict(nq=nq, ne=ne, nx=nx, gx=o_gx, cost=o_cost, grad=o_grad, hess=o_hess, rows=o_rows, nsr=nsr, no=no,
                row_grad=o_rows + no, stride=o_rows + no * (1 + nq))


def target_position(way_t, way_p, t):
    """the waypoints interpolated linearly in time and held outside their interval"""
    way_p = np.asarray(way_p).reshape(-1, 3)
    if len(way_t) == 1:
        return way_p[0].copy()
    return np.array([np.interp(t, way_t, way_p[:, i]) for i in range(3)])


def instance_oracle(c, b):
    Pb = copy.copy(c["P"])
    Pb.body_params = np.asarray(c["bp"][b]).reshape(Pb.nb, 10)
    Pb.way_p = np.asarray(c["way"][b]).reshape(-1, 3)
    if c.get("way_q") is not None:
        Pb.way_q = np.asarray(c["way_q"][b]).reshape(-1, 4)
    O = Oracle(Pb)
    if c.get("dyn") is not None:
        O.set_dynamic_obstacle(np.asarray(c["dyn"][b]), 1.0 if c.get("pflag") is None else float(c["pflag"][b]))
    return O


def expected_records(c, time_shift=0.0):
    """dict slot class -> array: g [B][N][ne], gx [B][N][ne][nx], cost [B][N], grad [B][N][nq], hess [B][N][nq][nq],
    rows [B][N-1][no], row_grad [B][N-1][no][nq] (knots 1 .. N-1), term_c [B][3], term_C [B][3][nq].  time_shift: added to every
    knot time (the teeth test's wrong clock)."""
    P = c["P"]
    D = dims(P)
    B, N, nq, nx, ne, no, nsr = c["xs"].shape[0], P.N, D["nq"], D["nx"], D["ne"], D["no"], D["nsr"]
    xs, us = c["xs"][:, :, :nx], c["us"]
    E = dict(g=np.zeros((B, N, ne)), gx=np.zeros((B, N, ne, nx)), cost=np.zeros((B, N)), grad=np.zeros((B, N, nq)),
             hess=np.zeros((B, N, nq, nq)), rows=np.zeros((B, max(N - 1, 0), no)), row_grad=np.zeros((B, max(N - 1, 0), no, nq)),
             term_c=np.zeros((B, 3)), term_C=np.zeros((B, 3, nq)))
    Q, R, xd = np.asarray(P.Qdiag), np.asarray(P.Rdiag), np.asarray(P.xd)
    for b in range(B):
        O = instance_oracle(c, b)
        for k in range(N):
            x, u, t = xs[b, k], us[b, k], c["t0"][b] + k * P.dt + time_shift
            E["g"][b, k], E["gx"][b, k], _ = O.eq_constraint(x, u)
            cost, cgx, _, H, _ = O.stage_cost(t, x, u)
            E["cost"][b, k] = cost - 0.5 * np.sum(Q * (x - xd) ** 2) - 0.5 * np.sum(R * u ** 2)
            E["grad"][b, k] = (cgx - Q * (x - xd))[:nq]
            E["hess"][b, k] = (H - np.diag(Q))[:nq, :nq]
            if k >= 1 and no > 0:
                if nsr:
                    E["rows"][b, k - 1, :nsr], E["row_grad"][b, k - 1, :nsr] = O.obstacle_rows(x, tau=k * P.dt + time_shift)
                if P.ee_box:
                    ee, dee = O.ee_kinematics(x, jac=True)
                    p, Jp = ee[:3], dee[:3, :nq]
                    pd = target_position(P.way_t, c["way"][b], t)
                    E["rows"][b, k - 1, nsr:] = np.concatenate([pd + P.ee_box_upper - p, p - (pd + P.ee_box_lower)])
                    E["row_grad"][b, k - 1, nsr:] = np.concatenate([-Jp, Jp])
        if P.terminal_constraint:
            cN, CN = O.terminal_constraint(c["t0"][b] + N * P.dt + time_shift, xs[b, N])
            E["term_c"][b], E["term_C"][b] = cN[:3], -CN[:3, :nq]
    return E


def projectile_allowance(c, lever=2.0):
    """{"rows": [B][N-1][no], "row_grad": [B][N-1][no][nq]}: forward bound of the fp64 rounding error of the projectile rows and of
    their gradients, zero everywhere else; None for a problem without projectile rows.  Per step of the iteration t <- t - f / f'
    (f the cubic, Horner form): |d upd| <= |df| / |f'| + |upd| |df'| / |f'| + 2 u |upd| with |df| <= 7 u (|a t^3| + |b t^2| + |c t| +
    |d|) + the rounding of the coefficients (dot products of rounded differences), likewise |df'|; the error carried into the next
    step is multiplied by |f f'' / f'^2|.  The row moves by w |e . r'(t)| / |e| per unit of time, its unit direction by |r'(t)| / |e|
    (gradient: times the largest |d centre / d q_j|, bounded by `lever` = 2 m for the arms of this project: UR10 reach 1.3 m on its
    base)."""
    import mpmath as mp
    P = c["P"]
    if len(P.proj_sph) == 0 or c.get("dyn") is None:
        return None
    D = dims(P)
    B, N, nq, nx, npair = c["xs"].shape[0], P.N, D["nq"], D["nx"], len(P.pair_a)
    out = dict(rows=np.zeros((B, N - 1, D["no"])), row_grad=np.zeros((B, N - 1, D["no"], nq)))
    F, u = mp.mpf, mp.mpf(2) ** -53
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]                        # noqa: E731
    adot = lambda a, b: abs(a[0] * b[0]) + abs(a[1] * b[1]) + abs(a[2] * b[2])        # noqa: E731
    with mp.workdps(50):
        for b in range(B):
            if c.get("pflag") is not None and c["pflag"][b] <= 0.5:
                continue      # flag off: the time is 0 and the row's weight is 0
            O = instance_oracle(c, b)
            d0 = np.asarray(c["dyn"][b]).reshape(-1, 9)[-1]
            for k in range(1, N):
                tau = k * P.dt
                centres = O.sphere_centers(c["xs"][b, k, :nx])
                g = [F(float(v)) for v in d0[6:9]]
                v = [F(float(d0[3 + i])) + tau * g[i] for i in range(3)]
                r = [F(float(d0[i])) + tau * F(float(d0[3 + i])) + F(0.5) * tau * tau * g[i] for i in range(3)]
                for i, s_ in enumerate(P.proj_sph):
                    cc = [F(float(x)) for x in centres[s_]]
                    dr = [cc[j] - r[j] for j in range(3)]
                    a3, a2, a1, a0 = dot(g, g), 3 * dot(v, g), 2 * (dot(v, v) - dot(dr, g)), -2 * dot(dr, v)
                    e3, e2, e1, e0 = 4 * u * adot(g, g), 12 * u * adot(v, g), 10 * u * (adot(v, v) + adot(dr, g)), 10 * u * adot(dr, v)
                    t, err = F(0), F(0)
                    for _ in range(10):
                        f, df, ddf = ((a3 * t + a2) * t + a1) * t + a0, (3 * a3 * t + 2 * a2) * t + a1, 6 * a3 * t + 2 * a2
                        ef = 7 * u * (abs(a3 * t ** 3) + abs(a2 * t * t) + abs(a1 * t) + abs(a0)) + abs(t ** 3) * e3 + t * t * e2 + abs(t) * e1 + e0
                        edf = 7 * u * (abs(3 * a3 * t * t) + abs(2 * a2 * t) + abs(a1)) + 3 * t * t * e3 + 2 * abs(t) * e2 + e1
                        upd = f / df
                        err = abs(f * ddf / df ** 2) * err + ef / abs(df) + abs(upd) * edf / abs(df) + 2 * u * abs(upd) + u * abs(t - upd)
                        t = t - upd
                        if abs(upd) < 1e-4:
                            break
                    if t <= 0:      # clamped to 0: exact unless the rounding can carry it across
                        err = err if -t < err else F(0)
                        t = F(0)
                    rd = [v[j] + t * g[j] for j in range(3)]
                    e = [cc[j] - (r[j] + t * v[j] + t * t * g[j] / 2) for j in range(3)]
                    dist = mp.sqrt(dot(e, e))
                    w = P.proj_scale / P.proj_dist[i] * (1.0 if c.get("pflag") is None else float(c["pflag"][b]))
                    out["rows"][b, k - 1, npair + i] = float(w * abs(dot(e, rd)) / dist * err)
                    out["row_grad"][b, k - 1, npair + i, :] = float(w * mp.sqrt(dot(rd, rd)) / dist * err * lever)
    return out


def split_records(P, lin):
    """The compared slots of records lin [B][N+1][stride] (trajectory mode), in the shape of expected_records()."""
    D = dims(P)
    B, n1, stride = lin.shape
    N, nq, nx, ne, no = n1 - 1, D["nq"], D["nx"], D["ne"], D["no"]
    assert N == P.N and stride == D["stride"], (lin.shape, D["stride"])
    s = lin[:, :N]
    iu = np.triu_indices(nq)
    H = np.zeros((B, N, nq, nq))
    H[:, :, iu[0], iu[1]] = s[:, :, D["hess"]:D["rows"]]
    H[:, :, iu[1], iu[0]] = s[:, :, D["hess"]:D["rows"]]
    r = lin[:, 1:N]
    out = dict(g=s[:, :, :ne], gx=s[:, :, D["gx"]:D["cost"]].reshape(B, N, ne, nx), cost=s[:, :, D["cost"]], grad=s[:, :, D["grad"]:D["hess"]],
               hess=H, rows=r[:, :, D["rows"]:D["row_grad"]], row_grad=r[:, :, D["row_grad"]:].reshape(B, max(N - 1, 0), no, nq))
    if P.terminal_constraint:
        out["term_c"] = lin[:, N, D["grad"]:D["grad"] + 3]
        out["term_C"] = lin[:, N, D["hess"]:D["hess"] + 3 * nq].reshape(B, 3, nq)
    return out


def split_points(P, B, out, rows=None):
    """Points-mode output (BatchMPC.linearize_points at the B N stage knots, instance-major; BatchMPC.state_rows at the
    B (N - 1) knots 1 .. N-1) in the shape of expected_records(): no terminal slots."""
    N, nq = P.N, P.nq
    got = {k: np.asarray(out[k]).reshape((B, N) + np.asarray(out[k]).shape[1:]) for k in ("g", "gx", "cost", "grad", "hess")}
    if rows is not None:
        d, dq = rows
        got["rows"] = d.reshape(B, N - 1, -1)
        got["row_grad"] = dq.reshape(B, N - 1, -1, nq)
    return got


def compare(expected, got, slots=None, allowance=None):
    """{slot class: (error, instance, knot)}: the largest error of the class in the units TOL is stated in, and where it occurred
    (knot: the record's knot index; None for the terminal slots).  A non-finite entry counts as an infinite error.  allowance:
    projectile_allowance()'s arrays, subtracted from the absolute error of their slots first."""
    res = {}
    for name in slots or SLOTS:
        if name not in got or name not in expected or expected[name].size == 0:
            continue
        e, g = expected[name], np.asarray(got[name])
        assert e.shape == g.shape, (name, e.shape, g.shape)
        err = np.abs(g - e)
        err[~np.isfinite(err)] = np.inf
        if allowance is not None and name in allowance:
            err = np.maximum(0.0, err - allowance[name])
        lead = 1 if name.startswith("term") else 2
        err = err.reshape(err.shape[:lead] + (-1,)).max(axis=-1)
        if name in RELATIVE:
            err = err / np.maximum(1.0, np.abs(e).reshape(e.shape[:lead] + (-1,)).max(axis=-1))
        i = np.unravel_index(np.argmax(err), err.shape)
        knot = int(i[1]) + (1 if name in ("rows", "row_grad") else 0) if lead == 2 else None
        res[name] = (float(err[i]), int(i[0]), knot)
    return res


def failures(res, tol=None):
    tol = tol or TOL
    return {k: v for k, v in res.items() if not v[0] < tol[k]}


def fmt(res):
    return " ".join("%s %.1e" % (k, v[0]) for k, v in res.items())
