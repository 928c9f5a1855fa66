"""Batched MPC engine: thin Python owner of a `upr_batch` handle (include/upright_mi.h).

One `BatchMPC` = B independent instances of one problem family on the current HIP device.  It is what
`bindings.ControllerInterface` wraps with B = 1, and what the benchmark / multi-GPU driver shard over
ranks.  All numerics run in libupright_mi.so; this file only moves arrays across the C-ABI.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, cont, iptr, ptr

F8, I4 = np.float64, np.int32


def uptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint))


def _level_of(speeds, s, what):
    """the lattice level of the speed s (None: -1, free)"""
    if s is None:
        return -1
    hit = np.flatnonzero(speeds == float(s))
    if hit.size != 1:
        raise ValueError("retime_plan: %s must equal a lattice speed" % what)
    return int(hit[0])


class BatchMPC:
    def __init__(self, problem, B=1, body_params=None, way_p=None, way_q=None, device=None):
        self.problem = problem.validate()
        self.B = int(B)
        self.nx, self.nu, self.N = problem.nx, problem.nu, problem.N
        self.nxf = problem.nx_full   # interface state: robot state + 9 per dynamic obstacle
        self.ne = 6 * problem.nb
        if body_params is None:
            body_params = np.broadcast_to(problem.body_params, (self.B,) + problem.body_params.shape)
        if way_p is None:
            way_p = np.broadcast_to(problem.way_p, (self.B,) + problem.way_p.shape)
        self.body_params = cont(body_params).reshape(self.B, problem.nb, 10)
        self.way_p = cont(way_p).reshape(self.B, len(problem.way_t), 3)
        self._c = _capi.problem_to_c(problem)
        self._lib = _capi.lib()
        if device is not None:     # one process per GPU: the launcher's LOCAL_RANK (None: the thread's current device)
            check(self._lib.upr_set_device(int(device)))
        self._h = self._lib.upr_batch_create(C.byref(self._c), self.B, ptr(self.body_params), ptr(self.way_p))
        if not self._h:
            raise RuntimeError(self._lib.upr_last_error().decode())
        if way_q is None and getattr(problem, "way_q", None) is not None:
            way_q = np.broadcast_to(np.asarray(problem.way_q, dtype=np.float64), (self.B, len(problem.way_t), 4))
        if way_q is not None:
            self.set_target_orientations(way_q)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.upr_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ControllerInterface surface, batched ------------------------------------------------------
    def reset(self, way_p=None):
        if way_p is not None:
            self.way_p = cont(way_p).reshape(self.B, len(self.problem.way_t), 3)
        check(self._lib.upr_batch_reset(self._h, ptr(self.way_p) if way_p is not None else None))

    def set_target_orientations(self, way_q):
        """Target orientations per instance and waypoint, (B, n_way, 4) quaternions xyzw."""
        self.way_q = cont(way_q).reshape(self.B, len(self.problem.way_t), 4)
        check(self._lib.upr_batch_set_target_orientations(self._h, ptr(self.way_q)))

    def set_observation(self, t, x):
        x = cont(x).reshape(self.B, self.nxf)
        t = cont(np.broadcast_to(np.asarray(t, dtype=np.float64), (self.B,)))
        check(self._lib.upr_batch_set_observation(self._h, ptr(t), 1, ptr(x)))

    def set_guess(self, xs, us):
        xs = cont(xs).reshape(self.B, self.N + 1, self.nxf)
        us = cont(us).reshape(self.B, self.N, self.nu)
        check(self._lib.upr_batch_set_guess(self._h, ptr(xs), ptr(us)))

    def set_sqp_iterations(self, n):
        """SQP iterations of the next advance only (sqp.init_sqp_iteration of a solve without a previous solution)."""
        check(self._lib.upr_batch_set_sqp_iterations(self._h, int(n)))

    def advance(self):
        check(self._lib.upr_batch_advance(self._h))

    def advance_async(self):
        check(self._lib.upr_batch_advance_async(self._h))

    def sync(self):
        check(self._lib.upr_batch_sync(self._h))

    def solution(self):
        ts = np.zeros((self.B, self.N + 1))
        xs = np.zeros((self.B, self.N + 1, self.nxf))
        us = np.zeros((self.B, self.N, self.nu))
        check(self._lib.upr_batch_get_solution(self._h, ptr(ts), ptr(xs), ptr(us)))
        return ts, xs, us

    def tick(self, t, x, want_stats=False):
        """One control period: set_observation(t, x), advance(), evaluate(t, x_obs=x) in one call and one synchronisation
        (upr_batch_tick).  Returns (x_opt, u_opt) or (x_opt, u_opt, stats)."""
        t = cont(np.broadcast_to(np.asarray(t, dtype=np.float64), (self.B,)))
        xo = cont(x).reshape(self.B, self.nxf)
        xr = np.zeros((self.B, self.nxf)); u = np.zeros((self.B, self.nu))
        s = np.zeros((self.B, _capi.NSTATS)) if want_stats else None
        check(self._lib.upr_batch_tick(self._h, ptr(t), 1, ptr(xo), ptr(xr), ptr(u), ptr(s) if want_stats else None))
        if want_stats:
            return xr, u, {name: s[:, i] for i, name in enumerate(_capi.STAT_NAMES)}
        return xr, u

    def tick_graph_replays(self):
        """Control periods upr_batch_tick served by replaying its captured HIP graph."""
        return int(self._lib.upr_batch_tick_graph_replays(self._h))

    def evaluate(self, t, x_obs=None):
        """Plan state and input at time t.  With x_obs (B, nx) and use_feedback_policy the input is the linear
        policy u*(t) + K(t) (x_obs - x*(t)) of the last solve (ocs2::LinearController), else the feed-forward input."""
        t = cont(np.broadcast_to(np.asarray(t, dtype=np.float64), (self.B,)))
        x = np.zeros((self.B, self.nxf))
        u = np.zeros((self.B, self.nu))
        if x_obs is not None and self.problem.use_feedback_policy:
            xo = cont(x_obs).reshape(self.B, self.nxf)
            check(self._lib.upr_batch_evaluate_policy(self._h, ptr(t), 1, ptr(xo), ptr(x), ptr(u)))
        else:
            check(self._lib.upr_batch_evaluate(self._h, ptr(t), 1, ptr(x), ptr(u)))
        return x, u

    def feedback_gains(self):
        """K[B][N][nu][nx] at the knots of the last solve (u = bias + K x, ocs2 sign)."""
        K = np.zeros((self.B, self.N, self.nu, self.nxf))
        check(self._lib.upr_batch_get_feedback(self._h, ptr(K)))
        return K

    def last_solve_ms(self):
        return float(self._lib.upr_batch_last_solve_ms(self._h))

    def stats(self):
        s = np.zeros((self.B, _capi.NSTATS))
        check(self._lib.upr_batch_get_stats(self._h, ptr(s)))
        return {name: s[:, i] for i, name in enumerate(_capi.STAT_NAMES)}

    def preserved_stats(self):
        """Context manager: statistics and QP dispatch keys of the last advance are put back on exit (upr_batch_hold_stats) --
        around a query that solves one more QP on the handle."""
        import contextlib

        @contextlib.contextmanager
        def hold():
            check(self._lib.upr_batch_hold_stats(self._h, 0))
            try:
                yield
            finally:
                check(self._lib.upr_batch_hold_stats(self._h, 1))

        return hold()

    # -- term-level access ----------------------------------------------------------------------------
    def linearize_points(self, x, u, t=None, inst=None):
        x = cont(x).reshape(-1, self.nxf)
        n = x.shape[0]
        u = cont(u).reshape(n, self.nu)
        t = cont(np.zeros(n) if t is None else np.broadcast_to(np.asarray(t, dtype=np.float64), (n,)))
        inst = cont(np.zeros(n) if inst is None else inst, dtype=np.int32)
        nq = self.problem.nq
        out = dict(
            g=np.zeros((n, self.ne)), gx=np.zeros((n, self.ne, self.nx)), cost=np.zeros(n),
            grad=np.zeros((n, nq)), hess=np.zeros((n, nq, nq)), ee=np.zeros((n, 3)),
        )
        check(self._lib.upr_batch_linearize_points(
            self._h, n, iptr(inst), ptr(t), ptr(x), ptr(u), ptr(out["g"]), ptr(out["gx"]), ptr(out["cost"]),
            ptr(out["grad"]), ptr(out["hess"]), ptr(out["ee"])))
        return out

    def obstacle_rows(self, x, jac=True):
        """Collision rows d (n, n_pairs) and d d / d q (n, n_pairs, nq) at n states (`obstacle_avoidance`)."""
        x = cont(x).reshape(-1, self.nxf)
        n, npair, nq = x.shape[0], len(self.problem.pair_a) + len(self.problem.proj_sph), self.problem.nq
        d = np.zeros((n, npair)); dq = np.zeros((n, npair, nq))
        check(self._lib.upr_batch_obstacle_rows(self._h, n, ptr(x), ptr(d), ptr(dq) if jac else None))
        return (d, dq) if jac else d

    def state_rows(self, x, t=None, inst=None, jac=True):
        """Every state row at n points: d (n, no) and d d / d q (n, no, nq), no = n_pairs + n_proj (+ 6 with the end-effector box),
        slot order [pairs][projectile][box upper 3][box lower 3].  The box rows depend on the time and on the instance's targets."""
        x = cont(x).reshape(-1, self.nxf)
        n, no, nq = x.shape[0], self.problem.n_state_rows, self.problem.nq
        t = cont(np.zeros(n) if t is None else np.broadcast_to(np.asarray(t, dtype=np.float64), (n,)))
        inst = cont(np.zeros(n) if inst is None else np.broadcast_to(np.asarray(inst), (n,)), dtype=np.int32)
        d = np.zeros((n, no)); dq = np.zeros((n, no, nq))
        check(self._lib.upr_batch_state_rows(self._h, n, iptr(inst), ptr(t), ptr(x), ptr(d), ptr(dq) if jac else None))
        return (d, dq) if jac else d

    def set_projectile_flag(self, s):
        """Activation flag of the projectile rows per instance (8th entry of the target state)."""
        s = cont(np.broadcast_to(np.asarray(s, dtype=np.float64), (self.B,)))
        check(self._lib.upr_batch_set_projectile_flag(self._h, ptr(s)))

    def eq_input_jacobian(self, inst=0):
        gu = np.zeros((self.ne, self.nu))
        check(self._lib.upr_batch_eq_input_jacobian(self._h, int(inst), ptr(gu)))
        return gu

    def qp_step(self):
        dxs = np.zeros((self.B, self.N + 1, self.nxf))
        dus = np.zeros((self.B, self.N, self.nu))
        check(self._lib.upr_batch_qp_step(self._h, ptr(dxs), ptr(dus)))
        return dxs, dus

    def qp_kkt(self):
        """One QP at the current trajectory: step and the multipliers the kernel ended with (see upr_batch_qp_kkt)."""
        P = self.problem
        ni = C.c_int(0)
        nin = 2 * self.nx + 2 * self.nu + (5 * P.nc if P.nf == 3 else 0) + P.n_state_rows
        out = dict(dx=np.zeros((self.B, self.N + 1, self.nxf)), du=np.zeros((self.B, self.N, self.nu)),   # (dx: interface width, zero obstacle block)
                   pi=np.zeros((self.B, self.N + 1, self.nx)), nu=np.zeros((self.B, self.N, self.ne)),
                   yN=np.zeros((self.B, 3 + 2 * P.nq if P.terminal_constraint else 0)), lam=np.zeros((self.B, self.N + 1, nin)))
        check(self._lib.upr_batch_qp_kkt(self._h, ptr(out["dx"]), ptr(out["du"]), ptr(out["pi"]), ptr(out["nu"]),
                                         ptr(out["yN"]) if out["yN"].size else None, ptr(out["lam"]), C.byref(ni)))
        assert ni.value == nin, (ni.value, nin)
        out["slack"] = np.ones((self.B, self.N + 1, nin))   # the rows' slacks at the exit (lam / slack = barrier weights of the last iterate)
        check(self._lib.upr_batch_qp_slacks(self._h, ptr(out["slack"])))
        return out

    def qp_slack_pairs(self):
        """Slack pairs (sigma, tau, gam) of the softened rows of the QP the last qp_kkt() solved, each (B, N + 1, ni) in the slot
        order of lam: 0 / 1 / 0 where a slot is not a softened row of the knot (upr_batch_qp_slack_pairs)."""
        shape = (self.B, self.N + 1, 2 * self.nx + 2 * self.nu + (5 * self.problem.nc if self.problem.nf == 3 else 0) + self.problem.n_state_rows)
        sig, tau, gam = np.zeros(shape), np.ones(shape), np.zeros(shape)
        check(self._lib.upr_batch_qp_slack_pairs(self._h, ptr(sig), ptr(tau), ptr(gam)))
        return sig, tau, gam

    # -- value function of the last QP, batched on the device --------------------------------------------
    def value_function_update(self, interface_states=False):
        """Linearise at the current plan, solve one QP there and run the cost-to-go kernel for every instance; statistics and
        dispatch keys of the last advance are left as they were (upr_batch_value_function_update).  A handle with a dynamic obstacle
        is refused unless interface_states is set: the caller then takes value_function's interface-state convention
        (upr_batch_value_function_update_interface)."""
        if interface_states:
            check(self._lib.upr_batch_value_function_update_interface(self._h))
        else:
            check(self._lib.upr_batch_value_function_update(self._h))

    def track_value_function(self, on=True):
        """Tracked mode: every advance() / tick() hands its own last QP to the cost-to-go kernel in-stream, so that value_function,
        cost_to_go and equality_lagrangian answer for the QP the solve ran last (ocs2's expansion point) without an update; the result
        stays valid across set_observation until the next advance (upr_batch_track_value_function)."""
        check(self._lib.upr_batch_track_value_function(self._h, 1 if on else 0))

    def value_function(self, t, x, inst=None):
        """V (n,) and dV/dx (n, nxf) at n points: interface states x (n, nxf), times t (scalar or (n,)), instance of each point
        (default: point i belongs to instance i when n == B, else instance 0).  The obstacle block of dV/dx is zero."""
        x = cont(x).reshape(-1, self.nxf)
        n = x.shape[0]
        t = cont(np.broadcast_to(np.asarray(t, dtype=np.float64), (n,)))
        if inst is None:
            inst = np.arange(n) if n == self.B else np.zeros(n)
        inst = cont(np.broadcast_to(np.asarray(inst), (n,)), dtype=np.int32)
        V, g = np.zeros(n), np.zeros((n, self.nxf))
        check(self._lib.upr_batch_value_function(self._h, n, iptr(inst), ptr(t), ptr(x), ptr(V), ptr(g)))
        return V, g

    def equality_lagrangian(self, t, inst=None):
        """nu(t) (n, ne): multipliers of the object-dynamics rows of the QP the cost-to-go belongs to at times t (scalar: one per
        instance, or (n,)), piecewise linear between the knots (upr_batch_equality_lagrangian)."""
        t = np.asarray(t, dtype=np.float64)
        n = self.B if t.ndim == 0 else t.shape[0]
        t = cont(np.broadcast_to(t, (n,)))
        if inst is None:
            inst = np.arange(n) if n == self.B else np.zeros(n)
        inst = cont(np.broadcast_to(np.asarray(inst), (n,)), dtype=np.int32)
        nu = np.zeros((n, self.ne))
        check(self._lib.upr_batch_equality_lagrangian(self._h, n, iptr(inst), ptr(t), ptr(nu)))
        return nu

    def cost_to_go(self):
        """dict(Pk (B, N + 1, nx, nx), pk (B, N + 1, nx), J (B, N + 1), X (B, N + 1, nx)) of the last value_function_update() or, in tracked mode,
        of the last advance() / tick(): robot-block shapes also with dynamic obstacles."""
        out = dict(Pk=np.zeros((self.B, self.N + 1, self.nx, self.nx)), pk=np.zeros((self.B, self.N + 1, self.nx)),
                   J=np.zeros((self.B, self.N + 1)), X=np.zeros((self.B, self.N + 1, self.nx)))
        check(self._lib.upr_batch_get_cost_to_go(self._h, ptr(out["Pk"]), ptr(out["pk"]), ptr(out["J"]), ptr(out["X"])))
        return out

    def value_function_ms(self):
        """Device time (ms) of the last cost-to-go launch."""
        return float(self._lib.upr_batch_value_function_ms(self._h))

    # -- balance check under inertial-parameter scenarios ---------------------------------------------------
    @property
    def balance_columns(self):
        """Cone generators of the arrangement: four per contact (n + mu s0, n + mu s1, n - mu s0, n - mu s1) with friction, the
        normal alone without."""
        return self.problem.nc * (4 if self.problem.nf == 3 else 1)

    def balance_check(self, x, params, want_z=False, want_iters=False, mu_scale=None):
        """rho (n, n_scen): the distance of the wrench the bodies need at the robot states x (n, 3 nq) to the contact wrench cone of
        the arrangement, under the inertial parameters params (n_scen, nb, 10) shared by all points or (n, n_scen, nb, 10) per
        point -- 0 if and only if balancing forces exist (upr_batch_balance_points; the force bounds are not part of it).  With
        want_z / want_iters the tuple (rho, z (n, n_scen, ncol), iters (n, n_scen)) restricted to what was asked for; z are the
        multipliers of the cone generators (balance_forces turns them into contact forces).  mu_scale (a number or one per scenario,
        finite and >= 0): every contact's friction coefficient is scaled by it in that scenario (the --mu of process_sim_runs.py as
        a scenario axis, upr_batch_balance_points_mu); None and 1 give the same bits.  mu_scale of shape (n_scen, nc): a scale per
        scenario and contact (upr_batch_balance_points_cmu; every pair of objects its own friction, compute_minimum_mu.py:12-30).

        The study's sweep (upright_robust/scripts/planning_sim_loop.py:548-559,613-616: the centre of mass at the centre, the face
        centres and the vertices of its box, times three inertia scales = 45 scenarios) for a one-body arrangement:

            th = mpc.problem.body_params                      # (1, 10): [m, m c, vech(I)]
            h = np.array([0.02, 0.02, 0.03])                  # half extents of the CoM box
            offs = [np.zeros(3)] + [s * h[a] * np.eye(3)[a] for a in range(3) for s in (1, -1)] + [(2 * np.array(v) - 1) * h for v in np.ndindex(2, 2, 2)]
            params = []
            for d in offs:
                for k in (1.0, 0.5, 0.1):
                    p = th.copy(); p[:, 1:4] += p[:, :1] * d; p[:, 4:] *= k
                    params.append(p)
            rho = mpc.balance_check_plan(np.stack(params))    # (B, N + 1, 45)
            unsafe = (rho > 1e-6).any(axis=(1, 2))            # instances whose plan loses balance in some scenario
        """
        x, n, params, n_scen, per_point = self._points_args(x, params)
        rho, z, iters = self._outputs((n, n_scen), (True, (), F8), (want_z, (self.balance_columns,), F8), (want_iters, (), I4))
        if self._per_contact(mu_scale, n_scen):
            entry, mu = self._lib.upr_batch_balance_points_cmu, cont(mu_scale)
        else:
            entry, mu = self._lib.upr_batch_balance_points_mu, self._mu_scale(mu_scale, n_scen)
        check(entry(self._h, n, ptr(x), n_scen, ptr(params), per_point, ptr(mu), ptr(rho), ptr(z), iptr(iters)))
        return self._asked_for(rho, z, iters)

    # -- what the balance family's methods share: the arguments of the points forms (the plan forms: _plan_params), the optional
    # outputs and what is returned of them
    def _points_args(self, x, params):
        """x (n, 3 nq), n, params (n_scen, nb, 10) or per point (n, n_scen, nb, 10), n_scen, per_point 0 | 1"""
        P = self.problem
        x = cont(x).reshape(-1, self.nx)
        n = x.shape[0]
        params = cont(params)
        per_point = 1 if params.ndim == 4 else 0
        params = params.reshape((n, -1, P.nb, 10) if per_point else (-1, P.nb, 10))
        return x, n, params, (params.shape[1] if per_point else params.shape[0]), per_point

    @staticmethod
    def _outputs(shape, *specs):
        """For every (wanted, trailing shape, dtype): zeros of shape + trailing shape, or None where it is not wanted."""
        return [np.zeros(shape + tail, dtype=dtype) if wanted else None for wanted, tail, dtype in specs]

    @staticmethod
    def _asked_for(*arrays):
        """The arrays that exist: the first alone, or the tuple of them."""
        out = tuple(a for a in arrays if a is not None)
        return out[0] if len(out) == 1 else out

    @staticmethod
    def _mu_scale(mu_scale, n_scen):
        if mu_scale is None:
            return None
        return np.ascontiguousarray(np.broadcast_to(np.asarray(mu_scale, dtype=np.float64), (n_scen,)))

    def _per_contact(self, mu_scale, n_scen):
        """mu_scale of shape (n_scen, nc): a scale per scenario and contact (the _cmu entries); every other shape takes the entry it
        always took."""
        return mu_scale is not None and np.ndim(mu_scale) == 2 and np.shape(mu_scale) == (n_scen, self.problem.nc)

    def contact_groups(self):
        """Labels (nc,) of the contacts by their pair of objects (contact_body1, contact_body2), numbered in the order of first
        occurrence: compute_contact_idx of upright_cmd/scripts/tools/compute_minimum_mu.py:12-30, the `groups` of friction_margin."""
        P = self.problem
        seen, labels = {}, np.zeros(P.nc, dtype=np.int64)
        for i in range(P.nc):
            labels[i] = seen.setdefault((int(P.contact_body1[i]), int(P.contact_body2[i])), len(seen))
        return labels

    def _group_masks(self, groups):
        """groups: labels (nc,) (-1: in no group; groups numbered 0 .. max) or a list of index lists -> masks (n_grp,) uint32."""
        nc = self.problem.nc
        if len(groups) and np.ndim(groups[0]) == 0:
            labels = np.asarray(groups)
            if labels.shape != (nc,):
                raise ValueError("groups: a label array needs one label per contact")
            sets = [np.flatnonzero(labels == g) for g in range(int(labels.max()) + 1)] if labels.max() >= 0 else []
        else:
            sets = [np.asarray(g, dtype=np.int64).ravel() for g in groups]
        masks = np.zeros(len(sets), dtype=np.uint32)
        for g, idx in enumerate(sets):
            if idx.size and (idx.min() < 0 or idx.max() >= 32):
                raise ValueError("groups: contact indices must lie in 0 .. 31")
            for i in idx:
                masks[g] |= np.uint32(1) << np.uint32(i)
        return masks

    def _mu_base(self, mu_base, n_scen):
        if mu_base is None:
            return None
        return np.ascontiguousarray(np.broadcast_to(np.asarray(mu_base, dtype=np.float64), (n_scen, self.problem.nc)))

    def balance_check_plan(self, params=None, want_iters=False, mu_scale=None):
        """rho (B, N + 1, n_scen) at the knots of the current plan, evaluated where they lie on the device (upr_batch_balance_plan).
        params None: every instance against its own body parameters (n_scen = 1, the nominal check); (n_scen, nb, 10): the same
        scenarios for every instance; (B, n_scen, nb, 10): per instance.  mu_scale as in balance_check."""
        n_scen, per_instance, params = self._plan_params(params)
        rho, iters = self._outputs((self.B, self.N + 1, n_scen), (True, (), F8), (want_iters, (), I4))
        if self._per_contact(mu_scale, n_scen):
            entry, mu = self._lib.upr_batch_balance_plan_cmu, cont(mu_scale)
        else:
            entry, mu = self._lib.upr_batch_balance_plan_mu, self._mu_scale(mu_scale, n_scen)
        check(entry(self._h, n_scen, ptr(params), per_instance, ptr(mu), ptr(rho), iptr(iters)))
        return self._asked_for(rho, iters)

    def _plan_params(self, params):
        if params is None:
            return 1, 0, None
        P = self.problem
        params = cont(params)
        per_instance = 1 if params.ndim == 4 else 0
        params = params.reshape((self.B, -1, P.nb, 10) if per_instance else (-1, P.nb, 10))
        return (params.shape[1] if per_instance else params.shape[0]), per_instance, params

    def friction_margin(self, x, params, kappa_max=8.0, want_lo=False, want_z=False, want_y=False, want_iters=False, groups=None, mu_base=None):
        """kappa* (n, n_scen): the friction margin of the robot states x (n, 3 nq) under the inertial parameters params (layouts of
        balance_check) -- the smallest common scale on the arrangement's friction coefficients at which balancing forces exist
        (upr_batch_friction_margin_points).  kappa* < 1: the state is balanced and 1 - kappa* of the friction could be lost;
        kappa* > 1: this much more friction would have been needed; kappa* = 0: normal forces alone balance the state; inf: no
        friction up to kappa_max times the arrangement's helps (tipping, lift-off).  The smallest friction coefficient of contact i
        that keeps the state balanced is kappa* mu_i (mu_i = problem.contact_mu, the margin already subtracted).  The force bounds
        u_lb / u_ub are not part of it.  kappa* carries the rule of the search: a state counts as balanced at a scale when the
        distance rho there is <= 1e-8 max(|b|, 1), the precision the controller enforces the constraint to, so kappa* lies below
        the exact boundary by what that ball allows (about 1e-8 at the arrangements of the study), and it is the upper end of a
        bracket of width kappa_max 2^-32.

        Returns kappa* alone or the tuple (kappa*, kappa_lo, z, y, iters) restricted to what was asked for: kappa_lo (n, n_scen) the
        last infeasible scale; z (n, n_scen, ncol) >= 0 the generator multipliers at kappa* with |b + A(kappa*) z| inside the ball;
        y (n, n_scen, 6 nb) the residual at kappa_lo, a separating direction (y' a_j(kappa_lo) >= 0 for every generator, y' b > 0);
        iters (n, n_scen) the least-squares solves over all evaluations.

        groups (labels (nc,), -1: in no group -- contact_groups() gives them by pair of objects -- or a list of index lists; groups
        may overlap): the margin of every contact group by itself (upr_batch_friction_margin_groups_points), which interface binds
        the state.  kappa scales the friction of the group's contacts only; the others keep mu_base (a number, (nc,) or (n_scen,
        nc); None: 1) times their coefficient.  Every result gains a trailing group axis: kappa* (n, n_scen, n_grp), z (n, n_scen,
        n_grp, ncol), ...  kappa*_g = 0: the group's friction is not needed; inf: more friction on this group alone does not help.
        groups=None is the common margin above."""
        x, n, params, n_scen, per_point = self._points_args(x, params)
        masks = None if groups is None else self._group_masks(groups)
        hi, lo, z, y, iters = self._outputs((n, n_scen) if masks is None else (n, n_scen, len(masks)), (True, (), F8), (want_lo, (), F8),
                                            (want_z, (self.balance_columns,), F8), (want_y, (self.ne,), F8), (want_iters, (), I4))
        if masks is None:
            if mu_base is not None:
                raise ValueError("mu_base needs groups")
            check(self._lib.upr_batch_friction_margin_points(self._h, n, ptr(x), n_scen, ptr(params), per_point, float(kappa_max),
                                                             ptr(hi), ptr(lo), ptr(z), ptr(y), iptr(iters)))
        else:
            base = self._mu_base(mu_base, n_scen)
            check(self._lib.upr_batch_friction_margin_groups_points(self._h, n, ptr(x), n_scen, ptr(params), per_point, len(masks), uptr(masks), ptr(base),
                                                                    float(kappa_max), ptr(hi), ptr(lo), ptr(z), ptr(y), iptr(iters)))
        return self._asked_for(hi, lo, z, y, iters)

    def friction_margin_plan(self, params=None, kappa_max=8.0, want_lo=False, want_iters=False, groups=None, mu_base=None, worst=False):
        """kappa* (B, N + 1, n_scen) at the knots of the current plan, evaluated where they lie on the device
        (upr_batch_friction_margin_plan); params as in balance_check_plan, the quantity as in friction_margin.  With want_lo /
        want_iters the tuple (kappa*, kappa_lo, iters) restricted to what was asked for.

        groups, mu_base as in friction_margin (upr_batch_friction_margin_groups_plan): kappa* (B, N + 1, n_scen, n_grp).  worst=True
        (with groups): instead of kappa* per knot the pair (worst (B, n_scen, n_grp), knot (B, n_scen, n_grp)) -- the largest kappa*
        over the knots of every instance (inf counts as largest) and the first knot that attains it, reduced on the device; only
        these are downloaded.  want_lo / want_iters are not available with it."""
        n_scen, per_instance, params = self._plan_params(params)
        if groups is None:
            if mu_base is not None or worst:
                raise ValueError("mu_base and worst need groups")
            hi, lo, iters = self._outputs((self.B, self.N + 1, n_scen), (True, (), F8), (want_lo, (), F8), (want_iters, (), I4))
            check(self._lib.upr_batch_friction_margin_plan(self._h, n_scen, ptr(params), per_instance, float(kappa_max), ptr(hi), ptr(lo), iptr(iters)))
            return self._asked_for(hi, lo, iters)
        masks = self._group_masks(groups)
        base = self._mu_base(mu_base, n_scen)
        if worst and (want_lo or want_iters):
            raise ValueError("worst=True returns the reduction alone")
        hi, lo, iters = self._outputs((self.B, self.N + 1, n_scen, len(masks)), (not worst, (), F8), (want_lo, (), F8), (want_iters, (), I4))
        w, knot = self._outputs((self.B, n_scen, len(masks)), (worst, (), F8), (worst, (), I4))
        check(self._lib.upr_batch_friction_margin_groups_plan(self._h, n_scen, ptr(params), per_instance, len(masks), uptr(masks), ptr(base),
                                                              float(kappa_max), ptr(hi), ptr(lo), iptr(iters), ptr(w), iptr(knot)))
        return self._asked_for(hi, lo, iters, w, knot)

    def speed_margin(self, x, params, s_max=4.0, want_out=False, want_z=False, want_y=False, want_iters=False):
        """s (n, n_scen, 2) = (s_lo, s_hi): the interval of uniform replay speeds at which the robot states x (n, 3 nq) are balanced
        under the inertial parameters params (layouts of balance_check; upr_batch_speed_margin_points).  Replaying a trajectory s
        times faster turns a knot (q, v, a) into (q, s v, s^2 a); a speed counts as balanced when the distance rho there is <= 1e-8
        max(|b|, 1), the rule of friction_margin.  s_lo = 0: balanced at rest; s_hi = s_max: balanced up to s_max; s_hi < 1: the
        plan must be slowed down to s_hi of its speed; s_hi > 1: it could be s_hi times faster; s_lo > 0: the state NEEDS motion
        (a tilted tray); (inf, -inf): no speed in [0, s_max] balances it.  Both ends are the accepted, conservative side of a
        bracket of width s_max 2^-32.  s_max must be finite and > 1.

        Returns s alone or the tuple (s, out, z, y, iters) restricted to what was asked for: out (n, n_scen, 2) = (s_lo_out,
        s_hi_out) the rejected neighbours of the two ends (0 below an s_lo of 0, inf above an s_hi of s_max; (0, s_max) where no
        speed is accepted); z (n, n_scen, 2, ncol) >= 0 the generator multipliers at s_lo and at s_hi; y (n, n_scen, 2, 6 nb) the
        residuals at s_lo_out and s_hi_out, separating directions; iters (n, n_scen) the least-squares solves over all
        evaluations (at most 3 + 3 * 32 of them)."""
        x, n, params, n_scen, per_point = self._points_args(x, params)
        speed, z, y, iters = self._outputs((n, n_scen), (True, (4,), F8), (want_z, (2, self.balance_columns), F8), (want_y, (2, self.ne), F8),
                                           (want_iters, (), I4))
        check(self._lib.upr_batch_speed_margin_points(self._h, n, ptr(x), n_scen, ptr(params), per_point, float(s_max), ptr(speed), ptr(z), ptr(y),
                                                      iptr(iters)))
        return self._asked_for(speed[..., 0::2].copy(), speed[..., 1::2].copy() if want_out else None, z, y, iters)

    def speed_margin_plan(self, params=None, s_max=4.0, want_out=False, want_iters=False, window=False):
        """s (B, N + 1, n_scen, 2) = (s_lo, s_hi) at the knots of the current plan, evaluated where they lie on the device
        (upr_batch_speed_margin_plan); params as in balance_check_plan, the quantity as in speed_margin.  With want_out /
        want_iters the tuple (s, out, iters) restricted to what was asked for.

        window=True: instead of s per knot the triple (window (B, n_scen, 2), knot (B, n_scen, 2), limit (B,)) -- the largest s_lo
        and the smallest s_hi over the knots of every instance (the speeds at which the WHOLE plan stays balanced in a scenario:
        window[..., 0] <= s <= window[..., 1]), the first knot that attains each, and the largest speed at which s v, s^2 a and
        s^3 u of every knot stay inside the velocity, acceleration and jerk bounds of the problem (inf for a plan at rest);
        reduced on the device, only these are downloaded.  want_out / want_iters are not available with it."""
        n_scen, per_instance, params = self._plan_params(params)
        if window and (want_out or want_iters):
            raise ValueError("window=True returns the reductions alone")
        speed, iters = self._outputs((self.B, self.N + 1, n_scen), (not window, (4,), F8), (want_iters, (), I4))
        w, knot = self._outputs((self.B, n_scen, 2), (window, (), F8), (window, (), I4))
        limit = np.zeros(self.B) if window else None
        check(self._lib.upr_batch_speed_margin_plan(self._h, n_scen, ptr(params), per_instance, float(s_max), ptr(speed), iptr(iters), ptr(w), iptr(knot),
                                                    ptr(limit)))
        if window:
            return w, knot, limit
        return self._asked_for(speed[..., 0::2].copy(), speed[..., 1::2].copy() if want_out else None, iters)

    def path_accel_margin(self, x, params, d_max=8.0, speed=1.0, want_out=False, want_z=False, want_y=False, want_iters=False):
        """d (n, n_scen, 2) = (d_lo, d_hi): the interval of path accelerations sddot (1 / s) at which the robot states x (n, 3 nq) are
        balanced under the inertial parameters params (layouts of balance_check; upr_batch_path_accel_margin_points).  Replaying a
        trajectory with the time scaling s(t), sdot = speed and sddot = d, turns a knot (q, v, a) into (q, speed v, speed^2 a + d v);
        d counts as balanced when the distance rho there is <= 1e-8 max(|b|, 1), the rule of friction_margin.  d < 0 is braking
        along the path (the geometric path is kept): d_lo is the hardest balanced braking (-d_max: balanced down to -d_max; the
        default 8 stops a replay at speed 1 within 125 ms), d_hi the hardest balanced acceleration; d_lo <= 0 <= d_hi iff the state
        itself is balanced at this speed; d_hi < 0: it is balanced only while braking at least that hard; (inf, -inf): no d in
        [-d_max, d_max] balances it.  Both ends are the accepted, conservative side of a bracket of width d_max 2^-31.  d_max must
        be finite and > 0, speed finite and >= 0.

        Returns d alone or the tuple (d, out, z, y, iters) restricted to what was asked for: out (n, n_scen, 2) = (d_lo_out,
        d_hi_out) the rejected neighbours of the two ends (-inf below a d_lo of -d_max, inf above a d_hi of d_max; (-d_max, d_max)
        where no d is accepted); z (n, n_scen, 2, ncol) >= 0 the generator multipliers at d_lo and at d_hi; y (n, n_scen, 2, 6 nb)
        the residuals at d_lo_out and d_hi_out, separating directions; iters (n, n_scen) the least-squares solves over all
        evaluations (at most 3 + 3 * 32 of them)."""
        x, n, params, n_scen, per_point = self._points_args(x, params)
        acc, z, y, iters = self._outputs((n, n_scen), (True, (4,), F8), (want_z, (2, self.balance_columns), F8), (want_y, (2, self.ne), F8),
                                         (want_iters, (), I4))
        check(self._lib.upr_batch_path_accel_margin_points(self._h, n, ptr(x), n_scen, ptr(params), per_point, float(d_max), float(speed), ptr(acc),
                                                           ptr(z), ptr(y), iptr(iters)))
        return self._asked_for(acc[..., 0::2].copy(), acc[..., 1::2].copy() if want_out else None, z, y, iters)

    def path_accel_margin_plan(self, params=None, d_max=8.0, speed=1.0, want_out=False, want_iters=False, window=False):
        """d (B, N + 1, n_scen, 2) = (d_lo, d_hi) at the knots of the current plan, evaluated where they lie on the device
        (upr_batch_path_accel_margin_plan); params as in balance_check_plan, the quantity as in path_accel_margin.  With want_out /
        want_iters the tuple (d, out, iters) restricted to what was asked for.

        window=True: instead of d per knot the triple (window (B, n_scen, 2), knot (B, n_scen, 2), limit (B, 2)) -- the largest d_lo
        and the smallest d_hi over the knots of every instance (the sddot at which the WHOLE plan stays balanced in a scenario if all
        knots brake alike), the first knot that attains each, and the interval (lo, hi) of d for which speed^2 a + d v of every knot
        stays inside the acceleration bounds of the problem ((-inf, inf) for a plan at rest, lo > hi if speed^2 a is outside them
        already; jerk is not part of it: a step in sddot is an impulse of jerk); reduced on the device, only these are downloaded.
        want_out / want_iters are not available with it."""
        n_scen, per_instance, params = self._plan_params(params)
        if window and (want_out or want_iters):
            raise ValueError("window=True returns the reductions alone")
        acc, iters = self._outputs((self.B, self.N + 1, n_scen), (not window, (4,), F8), (want_iters, (), I4))
        w, knot = self._outputs((self.B, n_scen, 2), (window, (), F8), (window, (), I4))
        limit = np.zeros((self.B, 2)) if window else None
        check(self._lib.upr_batch_path_accel_margin_plan(self._h, n_scen, ptr(params), per_instance, float(d_max), float(speed), ptr(acc), iptr(iters),
                                                         ptr(w), iptr(knot), ptr(limit)))
        if window:
            return w, knot, limit
        return self._asked_for(acc[..., 0::2].copy(), acc[..., 1::2].copy() if want_out else None, iters)

    @staticmethod
    def _dirs(dirs, frame):
        """dirs (n_dir, 6) contiguous, n_dir, frame 0 | 1"""
        dirs = cont(dirs).reshape(-1, 6)
        if frame not in ("world", "tray", 0, 1):
            raise ValueError("frame must be 'world' or 'tray'")
        return dirs, dirs.shape[0], (1 if frame in ("tray", 1) else 0)

    def disturbance_margin(self, x, params, dirs, r_max=8.0, frame="tray", want_out=False, want_z=False, want_y=False, want_iters=False):
        """r (n_dir, n, n_scen, 2) = (r_lo, r_hi): the interval of unplanned tray acceleration along each direction of dirs that the
        robot states x (n, 3 nq) absorb with the objects balanced under the inertial parameters params (layouts of balance_check;
        upr_batch_disturbance_margin_points).  dirs (n_dir, 6): rows u = (u_alpha, u_a), the angular (rad/s^2) and linear (m/s^2)
        acceleration of the tray per unit r, 1 <= n_dir <= 32, finite, no row all zero; frame "tray": in the tray's own frame (rotated
        by every state's C_we), "world": in the world frame.  The state displaced by r along u has the end-effector accelerations
        (alpha + r u_alpha, a_ee + r u_a); r counts as balanced when the distance rho there is <= 1e-8 max(|b|, 1), the rule of
        friction_margin.  -r_lo is what the state absorbs along -u, r_hi what it absorbs along +u (r_max: balanced up to r_max);
        r_lo <= 0 <= r_hi iff the state itself is balanced; (inf, -inf): no r in [-r_max, r_max] balances it.  Both ends are the
        accepted, conservative side of a bracket of width r_max 2^-31.  path_accel_margin at speed 1 is the direction (omega, v_ee) in
        the world frame.  r_max must be finite and > 0.

        Returns r alone or the tuple (r, out, z, y, iters) restricted to what was asked for, every array with the leading direction
        axis: out (n_dir, n, n_scen, 2) = (r_lo_out, r_hi_out) the rejected neighbours of the two ends (-inf below an r_lo of -r_max,
        inf above an r_hi of r_max; (-r_max, r_max) where no r is accepted); z (n_dir, n, n_scen, 2, ncol) >= 0 the generator
        multipliers at r_lo and at r_hi; y (n_dir, n, n_scen, 2, 6 nb) the residuals at r_lo_out and r_hi_out, separating directions;
        iters (n_dir, n, n_scen) the least-squares solves over all evaluations (at most 3 + 3 * 32 of them)."""
        x, n, params, n_scen, per_point = self._points_args(x, params)
        dirs, n_dir, frame = self._dirs(dirs, frame)
        reach, z, y, iters = self._outputs((n_dir, n, n_scen), (True, (4,), F8), (want_z, (2, self.balance_columns), F8), (want_y, (2, self.ne), F8),
                                           (want_iters, (), I4))
        check(self._lib.upr_batch_disturbance_margin_points(self._h, n, ptr(x), n_scen, ptr(params), per_point, n_dir, ptr(dirs), frame, float(r_max),
                                                            ptr(reach), ptr(z), ptr(y), iptr(iters)))
        return self._asked_for(reach[..., 0::2].copy(), reach[..., 1::2].copy() if want_out else None, z, y, iters)

    def disturbance_margin_plan(self, dirs, params=None, r_max=8.0, frame="tray", want_out=False, want_iters=False, window=False, radius=False):
        """r (n_dir, B, N + 1, n_scen, 2) = (r_lo, r_hi) at the knots of the current plan, evaluated where they lie on the device
        (upr_batch_disturbance_margin_plan); params as in balance_check_plan, the quantity as in disturbance_margin.  With want_out /
        want_iters the tuple (r, out, iters) restricted to what was asked for.

        window=True: instead of r per knot the pair (window (n_dir, B, n_scen, 2), knot (n_dir, B, n_scen, 2)) -- per direction the
        largest r_lo and the smallest r_hi over the knots of every instance and the first knot that attains each.  radius=True: the
        pair (radius (B, n_scen), binding (B, n_scen, 3)) -- radius = min over directions of min(-window_lo, window_hi), the largest
        r that every knot of the plan absorbs along every +-u given (negative when some knot is not balanced, -inf when some knot and
        direction accept nothing), binding = (direction, sign -1 | +1, knot) of the end that attains it (directions in ascending
        order, the lower end before the upper, the first end wins ties).  With both: (window, knot, radius, binding).  Reduced on the
        device, only these are downloaded; want_out / want_iters are not available with them."""
        n_scen, per_instance, params = self._plan_params(params)
        dirs, n_dir, frame = self._dirs(dirs, frame)
        reduced = window or radius
        if reduced and (want_out or want_iters):
            raise ValueError("window=True / radius=True return the reductions alone")
        reach, iters = self._outputs((n_dir, self.B, self.N + 1, n_scen), (not reduced, (4,), F8), (want_iters, (), I4))
        w, knot = self._outputs((n_dir, self.B, n_scen, 2), (window, (), F8), (window, (), I4))
        rad, bind = self._outputs((self.B, n_scen), (radius, (), F8), (radius, (3,), I4))
        check(self._lib.upr_batch_disturbance_margin_plan(self._h, n_scen, ptr(params), per_instance, n_dir, ptr(dirs), frame, float(r_max), ptr(reach),
                                                          iptr(iters), ptr(w), iptr(knot), ptr(rad), iptr(bind)))
        if reduced:
            return self._asked_for(w, knot, rad, bind)
        return self._asked_for(reach[..., 0::2].copy(), reach[..., 1::2].copy() if want_out else None, iters)

    def retime_plan(self, speeds, params=None, start=None, end=None, common=False, boxes=True, want_reach=False, want_edges=False, want_iters=False,
                    reserve=None, dirs=None, frame="tray", substeps=1):
        """(duration, level): the fastest time law on the lattice `speeds` that replays the geometric path of the current plan with the
        objects balanced at every knot (upr_batch_retime_plan), where speed_margin_plan could only offer one uniform factor.  speeds
        (M,): replay speeds s_0 < s_1 < .., finite, >= 0, 1 <= M <= 32.  The law gives knot i the speed speeds[level[i]] and keeps
        sddot constant on every segment: d_i = (s_{i+1}^2 - s_i^2) / (2 dt), the segment lasts 2 dt / (s_i + s_{i+1}); two speeds that sum
        to 0 are no edge.  An edge is admissible in a scenario iff its departing state x_i(s_i, d_i) and its arriving state
        x_{i+1}(s_{i+1}, d_i), x(s, d) = (q, s v, s^2 a + d v), are both balanced by the rule of path_accel_margin (rho <= 1e-8
        max(|b|, 1)) and, with boxes, s v and s^2 a + d v of every joint stay inside the velocity and acceleration bounds of the problem
        at both ends.  Positions do not move.  Jerk is NOT enforced: a step of sddot at a knot is an impulse of jerk.  The optimum
        over the lattice is exact (a dynamic programme, ties to the smallest level).  start / end: the speed of the first / last
        knot, which must equal a lattice value, or None: free.  params as in balance_check_plan.

        duration (B, n_scen) in seconds, inf where no time law exists on the lattice; level (B, n_scen, N + 1) int32, -1 throughout
        where duration is inf.  common=True: ONE time law per instance that holds under every scenario -- duration (B,), level (B,
        N + 1).  With want_reach / want_edges / want_iters the tuple (duration, level, reach, edges, iters) restricted to what was
        asked for: reach (.., 2) = (f, g), f the last knot with a level reachable forward from the start, g the first knot that has
        a level from which the end can be reached -- (N, 0) for a feasible plan, where an infeasible one blocks from each side;
        edges (B, n_scen, N, M) uint32, bit m' of row (i, m): the edge m -> m' of segment i is admissible in that scenario (per
        scenario with common=True too: the law runs on their AND); iters, same shape, the least-squares solves of a mask row.
        retimed_states(level, speeds) gives the times and states of the law.

        The study's sweep (balance_check) as one braking law that holds under all 45 scenarios and ends at rest:

            th = mpc.problem.body_params                      # (1, 10): [m, m c, vech(I)]
            h = np.array([0.02, 0.02, 0.03])                  # half extents of the CoM box
            offs = [np.zeros(3)] + [s * h[a] * np.eye(3)[a] for a in range(3) for s in (1, -1)] + [(2 * np.array(v) - 1) * h for v in np.ndindex(2, 2, 2)]
            params = []
            for d in offs:
                for k in (1.0, 0.5, 0.1):
                    p = th.copy(); p[:, 1:4] += p[:, :1] * d; p[:, 4:] *= k
                    params.append(p)
            speeds = np.linspace(0.0, 1.5, 13)
            duration, level = mpc.retime_plan(speeds, np.stack(params), common=True, end=0.0)   # (B,), (B, N + 1)
            t, dep, arr = mpc.retimed_states(level, speeds)   # knot times and the states on both sides of every segment

        reserve=r (a number >= 0; upr_batch_retime_plan_reserve): a time-optimal law rides the constraint, its end states absorb about
        nothing.  With a reserve an end state is accepted only if it is balanced itself and, when r > 0, still balanced when the tray is
        pushed by +r u and by -r u along every row u = (u_alpha, u_a) of dirs (n_dir, 6) -- the displacement, the frame ("tray" |
        "world") and the unit of r are disturbance_margin's.  The answer is the fastest law on the lattice that keeps that reserve at
        every knot; outputs and options as above, iters at most 2 M (1 + 2 n_dir) projections per row.  Between +r u and -r u the
        whole segment is certified (the cone is convex); nothing is claimed for combinations of directions.  reserve=0 gives the plain
        law bit for bit; reserve=None (the default) is the plain call and ignores dirs and frame.

            zx = np.array([[0, 0, 0, 0, 0, 1.0], [0, 0, 0, 1.0, 0, 0]])       # the tray's own z and x axes
            duration, level = mpc.retime_plan(speeds, reserve=0.5, dirs=zx)   # every knot absorbs 0.5 m/s^2 along +-z and +-x

        substeps=R (an integer 1 .. 16; upr_batch_retime_plan_substeps): everything above holds at the knots only.  With R > 1 an edge is
        admissible only if the objects are also balanced at the R - 1 interior path points tau_r = r dt / R of its segment: the point
        (Q, Q', Q'') of replay_plan's quintic Hermite path there, at the speed s_r = sqrt(((R - r) s_i^2 + r s_{i+1}^2) / R) the edge's
        constant sddot gives it, the state (Q, s_r Q', s_r^2 Q'' + d_i Q'); with boxes the interior states stay inside the bounds too.  The
        law is still one level per knot: replay_plan and retimed_states take it as it is, retimed_substates(level, speeds, R) gives the
        states that were judged.  iters at most M (R + 1) projections per row.  Nothing is claimed between the substep points:
        replay_plan on the returned law is the check.  substeps=1 (the default) is the plain call; substeps > 1 together with reserve is
        a ValueError.  The slide of replay_plan's example, which the plain call accepts at 1.1185 and a 10 ms clock rejects on six
        samples:

            mpc.retime_plan([1.1185], boxes=False, substeps=2)[0]                          # 1.788109: the midpoints miss the peak
            mpc.retime_plan([1.1185], boxes=False, substeps=4)[0]                          # inf: the points 1/4 of segment 4, 3/4 of segment 15
            duration, level = mpc.retime_plan([1.11, 1.1185], boxes=False, substeps=4)     # 1.789473, level 0 at knots 5 and 15 only
            mpc.replay_plan(level[:, 0], [1.11, 1.1185], 0.01, boxes=False, reductions=True)[3][..., 2]   # 0 samples rejected
        """
        speeds = cont(speeds).reshape(-1)
        if int(substeps) != substeps:
            raise ValueError("substeps must be an integer")
        if substeps != 1 and reserve is not None:
            raise ValueError("substeps > 1 together with reserve is not available")
        n_scen, per_instance, params = self._plan_params(params)
        lead = (self.B,) if common else (self.B, n_scen)
        dur, level, reach = self._outputs(lead, (True, (), F8), (True, (self.N + 1,), I4), (want_reach, (2,), I4))
        edges, iters = self._outputs((self.B, n_scen, self.N, speeds.size), (want_edges, (), np.uint32), (want_iters, (), I4))
        head = (self._h, n_scen, ptr(params), per_instance, int(speeds.size), ptr(speeds), _level_of(speeds, start, "start"), _level_of(speeds, end, "end"),
                int(bool(common)), int(bool(boxes)))
        outs = (ptr(dur), iptr(level), iptr(reach), uptr(edges) if want_edges else None, iptr(iters))
        if substeps != 1:
            check(self._lib.upr_batch_retime_plan_substeps(*head, int(substeps), *outs))
        elif reserve is None:
            check(self._lib.upr_batch_retime_plan(*head, *outs))
        else:
            if frame not in ("world", "tray", 0, 1):
                raise ValueError("frame must be 'world' or 'tray'")
            dirs = None if dirs is None else cont(dirs).reshape(-1, 6)
            check(self._lib.upr_batch_retime_plan_reserve(*head, 0 if dirs is None else dirs.shape[0], ptr(dirs), 1 if frame in ("tray", 1) else 0,
                                                          float(reserve), *outs))
        return self._asked_for(dur, level, reach, edges, iters)

    def retimed_states(self, level, speeds):
        """(t, dep, arr) of the time laws `level` (.., N + 1) of retime_plan on the current plan (solution()), leading axes (B,) or (B,
        n_scen): t (.., N + 1) the knot times, the cumulative 2 dt / (s_i + s_{i+1}); dep (.., N, 3 nq) the state in which knot i
        departs on segment i, (q_i, s_i v_i, s_i^2 a_i + d_i v_i); arr (.., N, 3 nq) the state in which knot i + 1 arrives from it,
        (q_{i+1}, s_{i+1} v_{i+1}, s_{i+1}^2 a_{i+1} + d_i v_{i+1}).  NaN where the plan has no time law (level -1).  Plain numpy."""
        speeds = np.asarray(speeds, dtype=np.float64).reshape(-1)
        level = np.asarray(level)
        _, xs, _ = self.solution()
        nq, dt = self.problem.nq, float(self.problem.dt)
        x = xs[..., :3 * nq]
        if level.ndim == 3:
            x = np.broadcast_to(x[:, None], level.shape[:2] + x.shape[1:])
        ok = (level >= 0).all(axis=-1)
        s = np.where(level >= 0, speeds[np.maximum(level, 0)], np.nan)
        s0, s1 = s[..., :-1], s[..., 1:]
        d = (s1 - s0) * (s1 + s0) / (2.0 * dt)
        t = np.zeros(level.shape)
        t[..., 1:] = np.cumsum(2.0 * dt / (s0 + s1), axis=-1)
        t[~ok] = np.nan

        def side(xk, sk):
            q, v, a = xk[..., :nq], xk[..., nq:2 * nq], xk[..., 2 * nq:]
            return np.concatenate([q + 0.0 * sk[..., None], sk[..., None] * v, (sk * sk)[..., None] * a + d[..., None] * v], axis=-1)
        return t, side(x[..., :-1, :], s0), side(x[..., 1:, :], s1)

    def retimed_substates(self, level, speeds, substeps):
        """(t, x) of the time laws `level` (.., N + 1) of retime_plan on the current plan at the substep points of every segment, leading
        axes as retimed_states': t (.., N, R + 1) = T_i + 2 tau_r / (s_i + s_r), tau_r = r dt / R; x (.., N, R + 1, 3 nq) the states
        retime_plan(.., substeps=R) judges, (Q, s_r Q', s_r^2 Q'' + d_i Q') on the quintic Hermite path of replay_plan with s_r =
        sqrt(((R - r) s_i^2 + r s_{i+1}^2) / R).  r = 0 is retimed_states' dep and r = R its arr, as doubles (the knot records are not
        interpolated).  NaN where the plan has no time law (level -1).  Plain numpy."""
        R = int(substeps)
        if R < 1:
            raise ValueError("substeps must be >= 1")
        T, dep, arr = self.retimed_states(level, speeds)
        speeds = np.asarray(speeds, dtype=np.float64).reshape(-1)
        level = np.asarray(level)
        _, xs, _ = self.solution()
        nq, dt = self.problem.nq, float(self.problem.dt)
        xk = xs[..., :3 * nq]
        if level.ndim == 3:
            xk = np.broadcast_to(xk[:, None], level.shape[:2] + xk.shape[1:])
        s = np.where(level >= 0, speeds[np.maximum(level, 0)], np.nan)
        s0, s1 = s[..., :-1], s[..., 1:]
        d = (s1 - s0) * (s1 + s0) / (2.0 * dt)
        x0, x1 = xk[..., :-1, :], xk[..., 1:, :]
        c = [x0[..., :nq], dt * x0[..., nq:2 * nq], dt * dt * x0[..., 2 * nq:], x1[..., :nq], dt * x1[..., nq:2 * nq], dt * dt * x1[..., 2 * nq:]]
        t = np.empty(s0.shape + (R + 1,))
        x = np.empty(s0.shape + (R + 1, 3 * nq))
        t[..., 0], x[..., 0, :] = T[..., :-1], dep
        with np.errstate(divide="ignore", invalid="ignore"):
            t[..., R] = T[..., :-1] + 2.0 * dt / (s0 + s1)
            x[..., R, :] = arr
            for r in range(1, R):
                tau, g = float(r) * dt / float(R), (float(r) * dt / float(R)) / dt
                sr = np.sqrt((float(R - r) * (s0 * s0) + float(r) * (s1 * s1)) / float(R))
                H = [1 - 10 * g**3 + 15 * g**4 - 6 * g**5, g - 6 * g**3 + 8 * g**4 - 3 * g**5, .5 * g**2 - 1.5 * g**3 + 1.5 * g**4 - .5 * g**5,
                     10 * g**3 - 15 * g**4 + 6 * g**5, -4 * g**3 + 7 * g**4 - 3 * g**5, .5 * g**3 - g**4 + .5 * g**5]
                D = [-30 * g**2 + 60 * g**3 - 30 * g**4, 1 - 18 * g**2 + 32 * g**3 - 15 * g**4, g - 4.5 * g**2 + 6 * g**3 - 2.5 * g**4,
                     30 * g**2 - 60 * g**3 + 30 * g**4, -12 * g**2 + 28 * g**3 - 15 * g**4, 1.5 * g**2 - 4 * g**3 + 2.5 * g**4]
                E = [-60 * g + 180 * g**2 - 120 * g**3, -36 * g + 96 * g**2 - 60 * g**3, 1 - 9 * g + 18 * g**2 - 10 * g**3,
                     60 * g - 180 * g**2 + 120 * g**3, -24 * g + 84 * g**2 - 60 * g**3, 3 * g - 12 * g**2 + 10 * g**3]
                Q0 = sum(w * v for w, v in zip(H, c))
                Q1 = sum(w * v for w, v in zip(D, c)) / dt
                Q2 = sum(w * v for w, v in zip(E, c)) / (dt * dt)
                t[..., r] = T[..., :-1] + 2.0 * tau / (s0 + sr)
                x[..., r, :] = np.concatenate([Q0 + 0.0 * sr[..., None], sr[..., None] * Q1, (sr * sr)[..., None] * Q2 + d[..., None] * Q1], axis=-1)
        return t, x

    def replay_plan(self, level, speeds, tick, params=None, t0=0.0, n_samples=None, boxes=True, want_rho=False, want_iters=False, reductions=False):
        """(t, x, excess): the time law `level` of retime_plan replayed on a clock (upr_batch_replay_plan) -- the states a tracking
        controller needs at t_k = t0 + k tick and the balance of the objects at every one of them, BETWEEN the knots too, where
        retime_plan claims nothing.  level (B, N + 1) int: ONE law per instance, indices into speeds, or -1 throughout (no law); a (B,
        n_scen, N + 1) array is refused: call once per scenario with level[:, sc].  speeds as in retime_plan; tick > 0, t0 >= 0;
        n_samples None: floor((the largest finite duration - t0) / tick) + 1 (at least 1), the durations being retimed_states' t[.., N].
        On segment i the law keeps sddot = d_i, so a sample t' after knot i has the speed s = s_i + d_i t' and lies at the path time tau
        = t' (s_i + d_i t' / 2); the path between two knots is, per joint, the quintic Hermite interpolant Q of their records (q, v, a)
        -- C2 across the knots, the plan's own cubic wherever the plan satisfies its dynamics, retimed_states' dep at t' = 0 and arr at
        the end of the segment; a sample on a knot takes the departing side.  params as in balance_check_plan.

        t (K,); x (B, K, 3 nq) = (Q, s Q', s^2 Q'' + d Q'); excess (B, K, n_scen) = rho / max(|b|, 1) of the balance check at x: the sample
        is accepted iff excess <= 1e-8, the rule of retime_plan.  Sample k exists iff t_k <= the duration of its plan; x and excess are
        NaN past the end and for a plan without a law.  With want_rho / want_iters the tuple (t, x, excess, rho, iters) restricted to
        what was asked for.  reductions=True: (duration (B,), count (B,), worst (B, n_scen), verdict (B, n_scen, 3), box_first (B,))
        alone, reduced on the device, nothing else is downloaded -- count the existing samples, worst the largest excess over them (NaN
        without any), verdict = (first sample attaining worst, first rejected sample or -1, number rejected), box_first (boxes=True) the
        first existing sample at which some joint's velocity or acceleration leaves its bounds, else -1.  Jerk is not judged.

        One level at speed 1 asks whether the plan as it stands is balanced between its knots.  A law accepted at every knot can leave
        the cone inside a segment: a translation whose path acceleration peaks at 0.8 mu g BETWEEN two knots (tests/retime_ref.py,
        slide_case), replayed uniformly at 1.1185 -- 1.1185^2 * 0.8 = 1.0008 > 1 while every knot keeps a margin of 1.5e-3 mu g:

            duration, level = mpc.retime_plan([1.1185], boxes=False)                      # finite: every knot is balanced
            t, x, excess = mpc.replay_plan(level[:, 0], [1.1185], 0.01, boxes=False)       # 179 samples at 100 Hz
            np.flatnonzero(excess[0, :, 0] > 1e-8)                                         # 37 38 39 140 141 142: between knots 4-5 and 15-16
        """
        speeds = cont(speeds).reshape(-1)
        level = np.asarray(level)
        if level.ndim == 3:
            raise ValueError("replay_plan takes one law per instance, level (B, N + 1): call once per scenario with level[:, sc]")
        if level.shape != (self.B, self.N + 1):
            raise ValueError("level must have the shape (B, N + 1)")
        level = cont(level, dtype=np.int32)
        n_scen, per_instance, params = self._plan_params(params)
        if n_samples is None:
            ok = (level >= 0).all(axis=-1) & (level < speeds.size).all(axis=-1)
            s = speeds[np.clip(level, 0, speeds.size - 1)]
            with np.errstate(divide="ignore"):
                dur = np.cumsum(2.0 * float(self.problem.dt) / (s[:, :-1] + s[:, 1:]), axis=-1)[:, -1]
            dur = dur[ok & np.isfinite(dur)]
            n_samples = max(1, int(np.floor((dur.max() - t0) / tick)) + 1) if dur.size and tick > 0 and dur.max() >= t0 else 1
        K = int(n_samples)
        if K < 1:
            raise ValueError("n_samples must be >= 1")   # (the sizes of the outputs; every other refusal is the library's)
        head = (self._h, n_scen, ptr(params), per_instance, int(speeds.size), ptr(speeds), iptr(level), float(tick), float(t0), K, int(bool(boxes)))
        if reductions:
            if want_rho or want_iters:
                raise ValueError("reductions=True returns the reductions alone")
            dur, count, bfirst = self._outputs((self.B,), (True, (), F8), (True, (), I4), (True, (), I4))
            worst, verdict = self._outputs((self.B, n_scen), (True, (), F8), (True, (3,), I4))
            check(self._lib.upr_batch_replay_plan(*head, ptr(dur), iptr(count), None, None, None, None, ptr(worst), iptr(verdict), iptr(bfirst)))
            return dur, count, worst, verdict, bfirst
        count, = self._outputs((self.B,), (True, (), I4))
        x, = self._outputs((self.B, K), (True, (3 * self.problem.nq,), F8))
        excess, rho, iters = self._outputs((self.B, K, n_scen), (True, (), F8), (want_rho, (), F8), (want_iters, (), I4))
        check(self._lib.upr_batch_replay_plan(*head, None, iptr(count), ptr(x), ptr(rho), ptr(excess), iptr(iters), None, None, None))
        gone = np.arange(K)[None, :] >= count[:, None]
        x[gone] = np.nan
        excess[gone] = np.nan
        t = float(t0) + np.arange(K, dtype=np.float64) * float(tick)
        return self._asked_for(t, x, excess, rho, iters)

    def balance_ms(self):
        """Device time (ms) of the kernel launches of the last balance check, friction margin, speed margin, path-acceleration margin, retiming,
        replay or disturbance margin (HIP events around them)."""
        return float(self._lib.upr_batch_balance_ms(self._h))

    def balance_forces(self, z):
        """Contact forces f (..., nf nc), in the layout of the force block of u, from generator multipliers z (..., ncol): f = S z."""
        return balance_forces(self.problem, z)

    def device_ptrs(self):
        xs, us = C.c_void_p(), C.c_void_p()
        check(self._lib.upr_batch_device_ptrs(self._h, C.byref(xs), C.byref(us)))
        return xs.value, us.value

    def copy_solution_device(self, xs_ptr, us_ptr):
        check(self._lib.upr_batch_copy_solution_device(self._h, C.c_void_p(xs_ptr), C.c_void_p(us_ptr)))

    def copy_policy_device(self, u_ptr):
        """u_0 of every instance as the last tick() evaluated it, device -> device on the engine's stream (asynchronous)."""
        check(self._lib.upr_batch_copy_policy_device(self._h, C.c_void_p(u_ptr)))

    def device_index(self):
        return int(self._lib.upr_batch_device(self._h))

    def stream_ptr(self):
        """The engine's HIP stream (hipStream_t) as an integer, e.g. for torch.cuda.ExternalStream."""
        return int(self._lib.upr_batch_stream(self._h) or 0)

    def reset_async(self):
        check(self._lib.upr_batch_reset_async(self._h))

    def qp_profile(self):
        """Debug: arm (first call) / read-and-clear the per-phase cycle counters of the QP kernel, [B][wave 0..3][16]."""
        out = np.zeros((self.B, 4, 16))
        check(self._lib.upr_batch_qp_profile(self._h, ptr(out)))
        return out

    def lin_records(self):
        stride = C.c_int(0)
        check(self._lib.upr_batch_get_lin(self._h, None, C.byref(stride)))
        lin = np.zeros((self.B, self.N + 1, stride.value))
        check(self._lib.upr_batch_get_lin(self._h, ptr(lin), C.byref(stride)))
        return lin

    def enable_timing(self, on=True):
        """on: False / 0 no events; True / 1 around every kernel of an advance; 2 around the QP kernel only; 3 around every
        fourth QP launch."""
        check(self._lib.upr_batch_enable_timing(self._h, int(on)))

    def kernel_times(self):
        ms = np.zeros(3)
        n = np.zeros(3, dtype=np.int32)
        check(self._lib.upr_batch_kernel_times(self._h, ptr(ms), iptr(n)))
        return dict(linearize_ms=ms[0], qp_ms=ms[1], linesearch_ms=ms[2], launches=n.tolist(),
                    qp_kernel=self._lib.upr_batch_qp_kernel_name(self._h).decode(), ls_kernel=self._lib.upr_batch_ls_kernel_name(self._h).decode(),
                    lin_kernel=self._lib.upr_batch_lin_kernel_name(self._h).decode(),
                    ws_doubles=int(self._lib.upr_batch_ws_doubles(self._h)))


def core_object_dynamics(problem, body_params, forces, Cm, w, al, a):
    """upright_core.bindings.compute_object_dynamics_constraints, batched over the leading axis."""
    c = _capi.problem_to_c(problem)
    forces = cont(forces).reshape(-1, problem.nf * problem.nc)
    n = forces.shape[0]
    out = np.zeros((n, 6 * problem.nb))
    check(_capi.lib().upr_core_object_dynamics(
        C.byref(c), ptr(cont(body_params).reshape(problem.nb, 10)), n, ptr(forces), ptr(cont(Cm).reshape(n, 9)),
        ptr(cont(w).reshape(n, 3)), ptr(cont(al).reshape(n, 3)), ptr(cont(a).reshape(n, 3)), ptr(out)))
    return out


def core_friction_rows(problem, forces):
    c = _capi.problem_to_c(problem)
    forces = cont(forces).reshape(-1, 3 * problem.nc)
    n = forces.shape[0]
    out = np.zeros((n, 5 * problem.nc))
    check(_capi.lib().upr_core_friction_rows(C.byref(c), n, ptr(forces), ptr(out)))
    return out


def balance_forces(problem, z):
    """f = S z: the contact forces (..., nf nc) the multipliers z (..., ncol) of the balance check stand for.  With friction the
    generators of contact i are n_i + mu_i s_i0, n_i + mu_i s_i1, n_i - mu_i s_i0, n_i - mu_i s_i1 (upright_robust/modelling.py:39-43);
    without, z is the normal force itself."""
    z = np.asarray(z, dtype=np.float64)
    if problem.nf == 1:
        return z.copy()
    n, s, mu = np.asarray(problem.contact_normal), np.asarray(problem.contact_span).reshape(-1, 2, 3), np.asarray(problem.contact_mu)[:, None]
    S = np.stack([n + mu * s[:, 0], n + mu * s[:, 1], n - mu * s[:, 0], n - mu * s[:, 1]], axis=2)     # (nc, 3, 4)
    f = np.einsum("cdg,...cg->...cd", S, z.reshape(z.shape[:-1] + (problem.nc, 4)))
    return f.reshape(z.shape[:-1] + (3 * problem.nc,))
