"""Drop-in for the pybind11 module `upright_control.bindings` (upright_control/src/pybindings.cpp:43-428).

Same class and attribute names; `ControllerInterface` drives one instance (B = 1) of the batched HIP
engine through the C-ABI of libupright_mi.so.  Covered: the balancing OCP (object-dynamics equality, friction
rows), obstacle avoidance over sphere pairs, up to four dynamic obstacles, the projectile-path constraint on the last, the
end-effector box constraint, HPIPM slack settings, the linear feedback policy.  What the engine does not cover raises
RuntimeError -- at construction for OCP terms (inertial alignment, operating points), at the call for the
solver-internal getters (value function, Lagrangian, visualisation) -- the way the reference throws
std::runtime_error; never a silent fallback.
"""
import enum
import warnings

import numpy as np

from . import robots
from .core_bindings import ContactPoint, RigidBody  # noqa: F401  (BalancingSettings carries them)
from .engine import BatchMPC
from .problem import Problem


class scalar_array(list):
    def push_back(self, v):
        self.append(float(v))


class vector_array(list):
    def push_back(self, v):
        self.append(np.array(v, dtype=np.float64))


class matrix_array(list):
    def push_back(self, v):
        self.append(np.array(v, dtype=np.float64))


class StringPairVector(list):
    def push_back(self, v):
        self.append(tuple(v))


class DynamicObstacleVector(list):
    push_back = list.append


class DynamicObstacleModeVector(list):
    push_back = list.append


class MapStringScalar(dict):
    pass


class RobotBaseType(enum.Enum):
    Fixed = 0
    Nonholonomic = 1
    Omnidirectional = 2
    Floating = 3


def robot_base_type_from_string(s):
    try:
        return {"fixed": RobotBaseType.Fixed, "nonholonomic": RobotBaseType.Nonholonomic,
                "omnidirectional": RobotBaseType.Omnidirectional, "floating": RobotBaseType.Floating}[s]
    except KeyError:
        raise RuntimeError("Cannot parse RobotBaseType from string.")  # base_type.h:24


def robot_base_type_to_string(t):
    return t.name.lower()


class RobotDimensions:
    def __init__(self):
        self.q = self.v = self.x = self.u = 0


class OptimizationDimensions:
    """dimensions.h:18-46."""

    def __init__(self):
        self.robot = RobotDimensions()
        self.o = 0
        self.c = 0
        self.nf = 3

    def q(self): return self.robot.q + 3 * self.o
    def v(self): return self.robot.v + 3 * self.o
    def x(self): return self.robot.x + 9 * self.o
    def f(self): return self.nf * self.c
    def u(self): return self.robot.u + self.f()


class BalancingSettings:
    def __init__(self):
        self.enabled = False
        self.arrangement_name = ""
        self.bodies = {}
        self.contacts = []
        self.force_weight = 0.01


class DynamicObstacleMode:
    def __init__(self):
        self.time = 0.0
        self.position = np.zeros(3); self.velocity = np.zeros(3); self.acceleration = np.zeros(3)


class DynamicObstacle:
    def __init__(self):
        self.name = ""; self.radius = 0.0; self.modes = DynamicObstacleModeVector()


class ObstacleSettings:
    def __init__(self):
        self.enabled = False
        self.collision_link_pairs = StringPairVector()
        self.minimum_distance = 0.0
        self.obstacle_urdf_path = ""
        self.dynamic_obstacles = DynamicObstacleVector()


class InertialAlignmentSettings:
    def __init__(self):
        self.cost_enabled = False; self.constraint_enabled = False
        self.use_angular_acceleration = False; self.align_with_fixed_vector = False
        self.cost_weight = 1.0; self.alpha = 0.0
        self.contact_plane_normal = np.array([0.0, 0, 1]); self.contact_plane_span = np.zeros((2, 3)); self.com = np.zeros(3)


class MPCSettings:
    def __init__(self):
        self.time_horizon = 1.0; self.debug_print = False; self.cold_start = False


class RolloutSettings:
    def __init__(self):
        self.abs_tol_ode = 1e-9; self.rel_tol_ode = 1e-6; self.max_num_steps_per_second = 10000
        self.timestep = 1e-2; self.check_numerical_stability = True


class SlackSettings:
    def __init__(self):
        self.enabled = False; self.input_box = True; self.state_box = True; self.poly_ineq = True
        self.upper_L2_penalty = 100.0; self.lower_L2_penalty = 100.0; self.upper_L1_penalty = 0.0; self.lower_L1_penalty = 0.0
        self.upper_low_bound = 0.0; self.lower_low_bound = 0.0


class HPIPMSettings:
    def __init__(self):
        self.iter_max = 30; self.warm_start = 0; self.slacks = SlackSettings()


class SQPSettings:
    def __init__(self):
        self.sqp_iteration = 1; self.init_sqp_iteration = 1; self.delta_tol = 1e-6; self.cost_tol = 1e-4
        self.use_feedback_policy = True; self.dt = 0.01; self.project_state_input_equality_constraints = True
        self.print_solver_status = True; self.print_solver_statistics = True; self.print_line_search = False
        self.hpipm = HPIPMSettings()


class TrackingSettings:
    def __init__(self):
        self.rate = 125; self.min_policy_update_time = 0.01; self.kp = 0; self.kv = 0; self.ka = 0
        self.enforce_state_limits = True; self.enforce_input_limits = False; self.enforce_ee_position_limits = False
        self.use_projectile = False; self.state_violation_margin = 0.1; self.input_violation_margin = 1.0
        self.ee_position_violation_margin = 0.1


class EstimationSettings:
    def __init__(self):
        self.robot_init_variance = 0; self.robot_process_variance = 1.0; self.robot_measurement_variance = 1.0


class ControllerSettings:
    """controller_settings.h:47-119 (pybindings.cpp:246-303)."""

    def __init__(self):
        self.initial_state = np.zeros(0)
        self.gravity = np.array([0.0, 0, -9.81])
        self.recompile_libraries = True
        self.debug = False
        self.mpc = MPCSettings(); self.sqp = SQPSettings(); self.rollout = RolloutSettings()
        self.tracking = TrackingSettings(); self.estimation = EstimationSettings()
        self.input_weight = np.zeros((0, 0)); self.state_weight = np.zeros((0, 0)); self.end_effector_weight = np.zeros((6, 6))
        self.input_limit_lower = np.zeros(0); self.input_limit_upper = np.zeros(0)
        self.state_limit_lower = np.zeros(0); self.state_limit_upper = np.zeros(0)
        self.end_effector_box_constraint_enabled = False
        self.xyz_lower = np.zeros(3); self.xyz_upper = np.zeros(3)
        self.projectile_path_constraint_enabled = False
        self.projectile_path_distances = np.zeros(0); self.projectile_path_scale = 1.0; self.projectile_path_collision_links = []
        self.robot_urdf_path = ""; self.lib_folder = "/tmp/ocs2"
        self.robot_base_type = RobotBaseType.Fixed
        self.locked_joints = MapStringScalar(); self.base_pose = np.zeros(3)
        self.dims = OptimizationDimensions()
        self.end_effector_link_name = ""
        self.use_operating_points = False
        self.operating_times = scalar_array(); self.operating_states = vector_array(); self.operating_inputs = vector_array()
        self.balancing_settings = BalancingSettings()
        self.inertial_alignment_settings = InertialAlignmentSettings()
        self.obstacle_settings = ObstacleSettings()
        self.xd = np.zeros(0)


class TargetTrajectories:
    """ocs2::TargetTrajectories (pybindings.cpp:348-357): state = [r_d(3), Q_d(4, xyzw), s]."""

    def __init__(self, ts, xs, us):
        self.ts = scalar_array(float(t) for t in ts)
        self.xs = vector_array(np.array(x, dtype=np.float64) for x in xs)
        self.us = vector_array(np.array(u, dtype=np.float64) for u in us)

    @staticmethod
    def _interp(ts, vals, t):
        if len(vals) == 1 or t <= ts[0]:
            return np.array(vals[0])
        if t >= ts[-1]:
            return np.array(vals[-1])
        i = int(np.searchsorted(ts, t, side="right")) - 1
        a = (ts[i + 1] - t) / (ts[i + 1] - ts[i])
        return a * np.asarray(vals[i]) + (1 - a) * np.asarray(vals[i + 1])

    def get_desired_state(self, t):
        return self._interp(list(self.ts), list(self.xs), t)

    def get_desired_input(self, t):
        return self._interp(list(self.ts), list(self.us), t)


class VectorFunctionLinearApproximation:
    def __init__(self):
        self.f = np.zeros(0); self.dfdx = np.zeros((0, 0)); self.dfdu = np.zeros((0, 0))


class VectorFunctionQuadraticApproximation(VectorFunctionLinearApproximation):
    def __init__(self):
        super().__init__()
        self.dfdxx = matrix_array(); self.dfdux = matrix_array(); self.dfduu = matrix_array()


class ScalarFunctionQuadraticApproximation:
    """pybindings.cpp:326-338."""

    def __init__(self):
        self.f = 0.0
        self.dfdx = np.zeros(0); self.dfdu = np.zeros(0)
        self.dfdxx = np.zeros((0, 0)); self.dfdux = np.zeros((0, 0)); self.dfduu = np.zeros((0, 0))


class LinearController:
    """ocs2::LinearController as getLinearController returns it: u(t, x) = bias(t) + gain(t) x."""

    def __init__(self):
        self.timeStamp = scalar_array(); self.biasArray = vector_array(); self.gainArray = matrix_array()


class SystemPinocchioMapping:
    """pybindings.cpp:57-65; dynamics/system_pinocchio_mapping.h:81-142: state / input -> the generalised position,
    velocity and acceleration of the Pinocchio model, in which the dynamic obstacles' coordinates come FIRST."""

    def __init__(self, dims):
        self.dims = dims

    def _split(self, state):
        x = np.asarray(state, dtype=np.float64)
        d = self.dims
        if x.shape != (d.x(),):
            raise ValueError(f"state has shape {x.shape}, expected ({d.x()},)")
        return x[: d.robot.x], [x[d.robot.x + 9 * i: d.robot.x + 9 * (i + 1)] for i in range(d.o)]

    def get_pinocchio_joint_position(self, state):
        xr, obs = self._split(state)
        return np.concatenate([o[0:3] for o in obs] + [xr[: self.dims.robot.q]])

    def get_pinocchio_joint_velocity(self, state, input):
        xr, obs = self._split(state)
        d = self.dims.robot
        return np.concatenate([o[3:6] for o in obs] + [xr[d.q: d.q + d.v]])

    def get_pinocchio_joint_acceleration(self, state, input):
        xr, obs = self._split(state)
        d = self.dims.robot
        return np.concatenate([o[6:9] for o in obs] + [xr[d.q + d.v: d.q + 2 * d.v]])


MAX_DYNAMIC_OBSTACLES = 4   # UPR_MAX_DYN (include/upright_mi.h)


def problem_from_settings(s):
    """ControllerSettings -> Problem (what ControllerInterface's constructor assembles,
    controller_interface.cpp:103-393).  Raises RuntimeError for OCP terms outside the accelerated path."""
    if len(s.obstacle_settings.dynamic_obstacles) > MAX_DYNAMIC_OBSTACLES:
        raise RuntimeError("the MI355X engine supports %d dynamic obstacles" % MAX_DYNAMIC_OBSTACLES)
    if s.inertial_alignment_settings.cost_enabled or s.inertial_alignment_settings.constraint_enabled:
        raise RuntimeError("inertial alignment is outside the accelerated path (SURVEY.md section 2, row 12)")
    if s.use_operating_points:
        raise RuntimeError("operating points are not supported by the MI355X engine yet")
    if not s.balancing_settings.enabled:
        raise RuntimeError("Balancing constraints disabled: the MI355X engine accelerates the balancing OCP only")
    sl = s.sqp.hpipm.slacks
    if sl.enabled and (sl.upper_low_bound != 0 or sl.lower_low_bound != 0):
        raise RuntimeError("slack lower bounds other than 0 are not supported by the MI355X engine")
    d = s.dims
    if d.o != len(s.obstacle_settings.dynamic_obstacles):
        raise RuntimeError("dims.o must equal the number of dynamic obstacles")
    base = robot_base_type_to_string(s.robot_base_type)
    chain = robots.from_config({"base_type": base, "dims": {"q": d.robot.q}, "base_pose": list(s.base_pose)})
    from .core_bindings import contact_tables
    from .problem import contacts_from_fixture

    bodies, contacts = s.balancing_settings.bodies, s.balancing_settings.contacts
    if len(contacts) != d.c:
        raise RuntimeError("dims.c does not match the number of contact points")
    arr = {
        "bodies": [{"name": n, "params": bodies[n].get_parameters().tolist()} for n in bodies],
        "contacts": [dict(object1_name=c.object1_name, object2_name=c.object2_name, mu=c.mu, normal=np.asarray(c.normal).tolist(),
                          span=np.asarray(c.span).tolist(), r_co_o1=np.asarray(c.r_co_o1).tolist(), r_co_o2=np.asarray(c.r_co_o2).tolist())
                     for c in contacts],
    }
    tables = contacts_from_fixture(arr)
    for name, W in (("input_weight", s.input_weight), ("state_weight", s.state_weight), ("end_effector_weight", s.end_effector_weight)):
        W = np.asarray(W)
        if np.abs(W - np.diag(np.diag(W))).max() > 0:
            raise RuntimeError(f"{name} must be diagonal")
    nf, nc = d.nf, d.c
    T, dt = float(s.mpc.time_horizon), float(s.sqp.dt)
    N = int(round(T / dt))
    if abs(N * dt - T) > 1e-9:
        raise RuntimeError("time_horizon must be a multiple of sqp.dt")
    frictionless = nf == 1
    # controller_interface.cpp:330-357
    f_lb = np.full(nf * nc, 0.0 if frictionless else -1e2)
    f_ub = np.full(nf * nc, 1e2)
    xd = np.asarray(s.xd, dtype=np.float64)[: d.robot.x]   # the cost acts on the robot block (controller_interface.cpp:400-420)
    if xd.size == 0:
        xd = np.zeros(d.robot.x)
    P = Problem(
        chain=chain, nf=nf, N=N, dt=dt, gravity=np.asarray(s.gravity, dtype=np.float64),
        Qdiag=np.diag(np.asarray(s.state_weight)).copy(),
        Rdiag=np.concatenate([np.diag(np.asarray(s.input_weight)), s.balancing_settings.force_weight * np.ones(nf * nc)]),
        xd=xd, Wee=np.diag(np.asarray(s.end_effector_weight)).copy(),
        x_lb=np.asarray(s.state_limit_lower, dtype=np.float64), x_ub=np.asarray(s.state_limit_upper, dtype=np.float64),
        u_lb=np.concatenate([np.asarray(s.input_limit_lower, dtype=np.float64), f_lb]),
        u_ub=np.concatenate([np.asarray(s.input_limit_upper, dtype=np.float64), f_ub]),
        sqp_iters=int(s.sqp.sqp_iteration), qp_iter_max=int(s.sqp.hpipm.iter_max), use_feedback_policy=bool(s.sqp.use_feedback_policy),
        delta_tol=float(s.sqp.delta_tol), cost_tol=float(s.sqp.cost_tol), **tables,
    )
    P.n_dyn = d.o
    if sl.enabled:
        # hpipm_interface SlackSettings (pybindings.cpp:160-181): which row classes get a slack and its penalties
        P.slacks = dict(state_box=bool(sl.state_box), input_box=bool(sl.input_box), poly_ineq=bool(sl.poly_ineq),
                        lower_L2_penalty=float(sl.lower_L2_penalty), upper_L2_penalty=float(sl.upper_L2_penalty),
                        lower_L1_penalty=float(sl.lower_L1_penalty), upper_L1_penalty=float(sl.upper_L1_penalty))
    try:
        if s.obstacle_settings.enabled:
            # controller_interface.cpp:172-228,450-481: sphere pairs by name, hard state inequality "obstacle_avoidance"
            dyn = {o.name: o.radius for o in s.obstacle_settings.dynamic_obstacles}
            cm = robots.collision_model(chain, [tuple(p) for p in s.obstacle_settings.collision_link_pairs], dynamic=dyn)
            for k, v in cm.items():
                setattr(P, k, v)
            P.obs_min_dist = float(s.obstacle_settings.minimum_distance)
        if s.projectile_path_constraint_enabled:
            # controller_interface.cpp:272-294; the constraint reads the LAST 9 entries of the state: the last dynamic obstacle
            if d.o < 1:
                raise RuntimeError("projectile_path_constraint needs a dynamic obstacle")
            robots.add_projectile_rows(P, s.projectile_path_collision_links, s.projectile_path_distances, s.projectile_path_scale)
        if s.end_effector_box_constraint_enabled:
            # controller_interface.cpp:257-270: six state rows around the interpolated target position (wrappers.py:239-250)
            P.ee_box = True
            P.ee_box_lower = np.asarray(s.xyz_lower, dtype=np.float64).reshape(-1).copy()
            P.ee_box_upper = np.asarray(s.xyz_upper, dtype=np.float64).reshape(-1).copy()
            P.validate()
    except ValueError as e:
        raise RuntimeError(str(e))
    return P.validate()


class ControllerInterface:
    """ControllerPythonInterface (controller_python_interface.h:13-93; pybindings.cpp:364-427)."""

    def __init__(self, settings):
        self.settings = settings
        self.problem = problem_from_settings(settings)
        self._mpc = None
        self._target = None
        self._t = 0.0
        self._x = np.array(settings.initial_state, dtype=np.float64)
        self._first = True
        self._solves, self._vf, self._vf_key = 0, None, None
        self.last_qp_status = 0   # hpipm status of the last solve's final QP: 0 solved, 1 iteration limit, 2 numerical failure

    def _set_target(self, target):
        self._target = target
        ts = np.array(list(target.ts), dtype=np.float64)
        ps = np.array([np.asarray(x)[:3] for x in target.xs], dtype=np.float64).reshape(len(ts), 3)
        qs = np.array([np.asarray(x)[3:7] if np.asarray(x).size >= 7 else [0.0, 0.0, 0.0, 1.0] for x in target.xs], dtype=np.float64).reshape(len(ts), 4)
        self.problem.way_t, self.problem.way_p, self.problem.way_q = ts, ps, qs
        if self._mpc is not None and len(self._mpc.problem.way_t) == len(ts) and np.array_equal(self._mpc.problem.way_t, ts):
            self._mpc.reset(ps.reshape(1, len(ts), 3))
            self._mpc.set_target_orientations(qs.reshape(1, len(ts), 4))
        else:
            if self._mpc is not None:
                self._mpc.close()
            self._mpc = BatchMPC(self.problem, 1)
        if self.problem.n_dyn:
            # 8th entry of the target state: activation of the projectile constraint (projectile_path_constraint.h:88-90)
            x0t = np.asarray(target.xs[0], dtype=np.float64)
            self._mpc.set_projectile_flag(float(x0t[7]) if x0t.size > 7 else 0.0)
        self._first = True
        self._solves, self._vf, self._vf_key = 0, None, None   # solver-level queries describe a solve on THIS target / handle

    def reset(self, targetTrajectories):
        self._set_target(targetTrajectories)

    def setTargetTrajectories(self, targetTrajectories):
        self._set_target(targetTrajectories)

    def setObservation(self, t, x, u):
        x = np.asarray(x)
        if x.dtype != np.float64 or x.shape != (self.problem.nx_full,):
            raise TypeError("setObservation(): incompatible function arguments (x must be float64 of length nx)")
        self._t, self._x = float(t), x.copy()

    def advanceMpc(self):
        if self._mpc is None:
            raise RuntimeError("advanceMpc called before reset(targetTrajectories)")
        # ocs2's SQP solver runs sqp.init_sqp_iteration iterations from the initializer's guess while it holds no
        # previous solution (first solve after construction / reset), sqp.sqp_iteration warm-started ones afterwards;
        # mpc.cold_start resets the solver before every solve (pybindings.cpp:148,194-195; controller.yaml:15,56-57)
        cold = bool(self.settings.mpc.cold_start)
        if cold and not self._first:
            self._mpc.reset()
        if self._first or cold:
            self._mpc.set_sqp_iterations(int(self.settings.sqp.init_sqp_iteration))
        self._mpc.set_observation(self._t, self._x)
        self._mpc.advance()
        self._first = False
        self._solves += 1   # (what the value function of the last QP is cached against)
        self.last_qp_status = int(self._mpc.stats()["qp_status_last"][0])
        if self.last_qp_status != 0 and self.settings.sqp.print_solver_status:
            # what ocs2 prints from hpipm's return code when print_solver_status is set
            warnings.warn("QP of the last SQP iteration ended with status %d (%s)" % (
                self.last_qp_status, "iteration limit" if self.last_qp_status == 1 else "numerical failure: step rejected"), RuntimeWarning)

    def evaluateMpcSolution(self, current_time, current_state, opt_state, opt_input):
        # controller_python_interface.h:46-55: the policy is evaluated at the CURRENT state (a LinearController when
        # sqp.use_feedback_policy is set, the feed-forward input otherwise)
        xo = np.asarray(current_state, dtype=np.float64).reshape(1, -1) if self.problem.use_feedback_policy else None
        x, u = self._mpc.evaluate(float(current_time), xo)
        opt_state[:] = x[0]
        opt_input[:] = u[0]

    def getMpcSolution(self, t, x, u):
        ts, xs, us = self._mpc.solution()
        del t[:], x[:], u[:]
        for k in range(self.problem.N + 1):
            t.push_back(ts[0, k]); x.push_back(xs[0, k])
            u.push_back(us[0, min(k, self.problem.N - 1)])  # ocs2 repeats the last input at the final node

    def getLastSolveTime(self):
        return self._mpc.last_solve_ms()

    def getStateDim(self):
        return self.problem.nx_full

    def getInputDim(self):
        return self.problem.nu

    # -- term-level access (pybindings.cpp:414-424) ---------------------------------------------------------
    def _lin(self, t, x, u):
        if self._mpc is None:
            self._mpc = BatchMPC(self.problem, 1)
        return self._mpc.linearize_points(np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64), t)

    def getStateInputEqualityConstraintValue(self, name, t, x, u):
        if name != "object_dynamics":
            raise RuntimeError(f"no equality constraint named '{name}'")
        return self._lin(t, x, u)["g"][0]

    def getStateInputInequalityConstraintValue(self, name, t, x, u):
        if name == "end_effector_box_constraint" and self.problem.ee_box:
            # end_effector_box_constraint.h:47-76: [p_d(t) + upper - p; p - (p_d(t) + lower)], the last six state rows
            if self._mpc is None:
                self._mpc = BatchMPC(self.problem, 1)
            return self._mpc.state_rows(np.asarray(x, dtype=np.float64), t=float(t), jac=False)[0][-6:]
        if name in ("obstacle_avoidance", "projectile_constraint") and len(self.problem.pair_a) + len(self.problem.proj_sph) > 0:
            if self._mpc is None:
                self._mpc = BatchMPC(self.problem, 1)
            rows = self._mpc.obstacle_rows(np.asarray(x, dtype=np.float64), jac=False)[0]
            npair = len(self.problem.pair_a)
            return rows[:npair] if name == "obstacle_avoidance" else rows[npair:]
        if name != "contact_forces" or self.problem.nf != 3:
            raise RuntimeError(f"no inequality constraint named '{name}'")
        from .engine import core_friction_rows

        return core_friction_rows(self.problem, np.asarray(u, dtype=np.float64)[self.problem.nq:])[0]

    def getCostValue(self, name, t, x, u):
        x = np.asarray(x, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
        if name == "end_effector_cost":
            return float(self._lin(t, x, u)["cost"][0])
        if name == "state_input_cost":
            P = self.problem
            xr = x[: P.nx]   # (the robot's part of the state: dynamic obstacles carry no cost, controller_interface.cpp:400-420)
            return float(0.5 * np.sum(P.Qdiag * (xr - P.xd) ** 2) + 0.5 * np.sum(P.Rdiag * u ** 2))
        raise RuntimeError(f"no cost named '{name}'")

    def stateInputEqualityConstraint(self, t, x, u):
        return self.getStateInputEqualityConstraintValue("object_dynamics", t, x, u)

    def stateInputEqualityConstraintLinearApproximation(self, t, x, u):
        """pybindings.cpp:405-408: {f, dfdx, dfdu} of the object-dynamics equality at (t, x, u)."""
        out = self._lin(t, x, u)
        P = self.problem
        approx = VectorFunctionLinearApproximation()
        approx.f = out["g"][0]
        approx.dfdx = np.hstack([out["gx"][0], np.zeros((approx.f.size, P.nx_full - P.nx))])
        approx.dfdu = self._mpc.eq_input_jacobian(0)
        return approx

    def flowMap(self, t, x, u):
        """pybindings.cpp:388-389; system_dynamics.h:15-22,33-38: [v, a, jerk] for the robot, [v, a, 0] per obstacle."""
        P = self.problem
        x = np.asarray(x, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
        nq = P.nq
        parts = [x[nq:3 * nq], u[:nq]]
        for i in range(P.n_dyn):
            o = x[3 * nq + 9 * i: 3 * nq + 9 * (i + 1)]
            parts += [o[3:9], np.zeros(3)]
        return np.concatenate(parts)

    def flowMapLinearApproximation(self, t, x, u):
        """pybindings.cpp:390-392: the dynamics are linear time-invariant, so dfdx / dfdu are constant."""
        P = self.problem
        nq, nx, nu = P.nq, P.nx_full, P.nu
        approx = VectorFunctionLinearApproximation()
        approx.f = self.flowMap(t, x, u)
        A = np.zeros((nx, nx)); B = np.zeros((nx, nu))
        A[:2 * nq, nq:3 * nq] = np.eye(2 * nq)
        B[2 * nq:3 * nq, :nq] = np.eye(nq)
        for i in range(P.n_dyn):
            o = 3 * nq + 9 * i
            A[o:o + 6, o + 3:o + 9] = np.eye(6)
        approx.dfdx, approx.dfdu = A, B
        return approx

    def cost(self, t, x, u):
        """pybindings.cpp:393-394: intermediate cost = state_input_cost + end_effector_cost at (t, x, u)."""
        return self.getCostValue("state_input_cost", t, x, u) + self.getCostValue("end_effector_cost", t, x, u)

    def costQuadraticApproximation(self, t, x, u):
        """pybindings.cpp:395-397: value, gradients and (Gauss-Newton) Hessians of the intermediate cost."""
        P = self.problem
        x = np.asarray(x, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
        out = self._lin(t, x, u)
        nq, nx, nxf = P.nq, P.nx, P.nx_full
        q = ScalarFunctionQuadraticApproximation()
        q.f = self.cost(t, x, u)
        q.dfdx = np.zeros(nxf); q.dfdx[:nx] = P.Qdiag * (x[:nx] - P.xd); q.dfdx[:nq] += out["grad"][0]
        q.dfdu = P.Rdiag * u
        q.dfdxx = np.zeros((nxf, nxf)); q.dfdxx[:nx, :nx] = np.diag(P.Qdiag); q.dfdxx[:nq, :nq] += out["hess"][0]
        q.dfduu = np.diag(P.Rdiag)
        q.dfdux = np.zeros((P.nu, nxf))
        return q

    def getBias(self, t):
        """pybindings.cpp:385: bias of the linear policy u = bias(t) + K(t) x (ocs2::LinearController), interpolated
        between the knots like the gain."""
        c = self.getLinearController()
        ts = np.array(list(c.timeStamp))
        return TargetTrajectories._interp(list(ts), list(c.biasArray), float(t))

    def getLinearController(self):
        """pybindings.cpp:386-387: the ocs2::LinearController of the last solve (knot times, biases, gains)."""
        if not self.problem.use_feedback_policy:
            raise RuntimeError("sqp.use_feedback_policy is false: the solution carries a feed-forward controller")
        K = self._mpc.feedback_gains()[0]
        ts, xs, us = self._mpc.solution()
        c = LinearController()
        for k in range(self.problem.N):
            c.timeStamp.push_back(ts[0, k]); c.gainArray.push_back(K[k]); c.biasArray.push_back(us[0, k] - K[k] @ xs[0, k])
        return c

    # -- solver-level queries (pybindings.cpp:398-403,409-412): answered from the last QP of the last solve ---------------------------
    def _outside(self, name):
        raise RuntimeError(f"ControllerInterface.{name} is outside the accelerated path of the MI355X engine")

    def _on_device(self):
        """Which path answers the solver-level queries.  Hard inequality rows and no dynamic obstacle: the host module
        (upright_amd/value_function.py, one instance in numpy).  HPIPM slacks on inequality rows (their barrier pairs enter the weights
        the kernels factor) or a dynamic obstacle (interface states): the batched cost-to-go on the device, upr_value.h behind
        BatchMPC.value_function_update() / value_function() / equality_lagrangian().  Same expansion point -- the QP at the plan the
        last advanceMpc ended with -- and the same once-per-solve caching on both."""
        sl = self.problem.slacks or {}
        return bool(self.problem.n_dyn) or bool(sl.get("state_box") or sl.get("input_box") or sl.get("poly_ineq"))

    def _need_solve(self):
        if self._mpc is None or self._solves == 0:
            raise RuntimeError("no MPC solve yet on the current target: call advanceMpc first"
                               + (" (a problem with HPIPM slacks or dynamic obstacles is answered from the device's cost-to-go of that solve)" if self._on_device() else ""))

    def _value_function(self, riccati=True):
        """upright_amd/value_function.py: the Riccati cost-to-go of the QP at the plan the last advanceMpc ended with, rebuilt on the
        host from the primal-dual point the kernel exports (costates, multipliers and slacks); cached per solve."""
        from .value_function import ValueFunction

        self._need_solve()
        if self._vf_key != self._solves or (riccati and self._vf.Pk is None):
            self._vf, self._vf_key = ValueFunction(self._mpc, 0, riccati=riccati), self._solves
        return self._vf

    def _device_query(self, query):
        """query(handle) on the device path: the cost-to-go is rebuilt at the first query after a solve, and again whenever the handle
        reports it stale (something touched the plan or the observation since)."""
        self._need_solve()
        if self._vf_key != self._solves:
            self._mpc.value_function_update(interface_states=True)
            self._vf, self._vf_key = None, self._solves
        try:
            return query(self._mpc)
        except RuntimeError as e:
            if "stale" not in str(e):
                raise
            self._mpc.value_function_update(interface_states=True)
            return query(self._mpc)

    def valueFunction(self, t, x):
        """pybindings.cpp:398-399 (ocs2 getValueFunction(t, x).f): cost-to-go of the plan from t, expanded to second order in x."""
        if self._on_device():
            return float(self._device_query(lambda m: m.value_function(float(t), np.asarray(x, dtype=np.float64), 0))[0][0])
        return float(self._value_function().value(t, x))

    def valueFunctionStateDerivative(self, t, x):
        """pybindings.cpp:400-402 (ocs2 getValueFunction(t, x).dfdx): costate of the plan at t plus P(t) (x - x*(t)); zero in the block
        of a dynamic obstacle (data of the QP the engine solves)."""
        if self._on_device():
            return self._device_query(lambda m: m.value_function(float(t), np.asarray(x, dtype=np.float64), 0))[1][0].copy()
        g = np.zeros(self.problem.nx_full)
        g[:self.problem.nx] = self._value_function().gradient(t, x)
        return g

    def stateInputEqualityConstraintLagrangian(self, t, x, u):
        """pybindings.cpp:409-412: multipliers of the state-input equality (the object-dynamics rows) of the last QP at time t."""
        if self._on_device():
            return self._device_query(lambda m: m.equality_lagrangian(np.array([float(t)]), 0))[0].copy()
        return self._value_function(riccati=False).equality_multiplier(t).copy()   # (the multipliers alone)

    def getStateInequalityConstraintValue(self, name, t, x):
        # the reference looks `name` up among the STATE-ONLY constraints, of which the OCP has none
        # (controller_python_interface.h:67-72; every inequality is registered as a state-input one)
        raise RuntimeError(f"no state-only constraint named '{name}'")

    def visualizeTrajectory(self, t, x, u, speed):
        self._outside("visualizeTrajectory (ROS visualisation)")

    def getLinearFeedbackGain(self, t):
        """pybindings.cpp:382-384: gain of the linear policy at time t (linear interpolation between knots)."""
        if not self.problem.use_feedback_policy:
            raise RuntimeError("sqp.use_feedback_policy is false: the solution carries a feed-forward controller")
        K = self._mpc.feedback_gains()[0]
        ts = self._mpc.solution()[0][0]
        P = self.problem
        s = min(max((float(t) - ts[0]) / P.dt, 0.0), P.N - 1)
        j = min(int(s), P.N - 1)
        a = s - j
        return (1 - a) * K[j] + a * K[min(j + 1, P.N - 1)]


class BalancingConstraintWrapper:
    """balancing_constraint_wrapper.h:16-66: f = [contact rows (5c), object dynamics (6 nb)], dfdx likewise."""

    def __init__(self, settings):
        if not settings.balancing_settings.enabled:
            raise RuntimeError("Balancing settings not enabled.")
        self.problem = problem_from_settings(settings)
        self._mpc = BatchMPC(self.problem, 1)

    def getLinearApproximation(self, t, x, u):
        from .engine import core_friction_rows

        P = self.problem
        out = self._mpc.linearize_points(np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64), t)
        a = core_friction_rows(P, np.asarray(u, dtype=np.float64)[P.nq:])[0] if P.nf == 3 else np.zeros(0)
        approx = VectorFunctionLinearApproximation()
        approx.f = np.concatenate([a, out["g"][0]])
        approx.dfdx = np.vstack([np.zeros((a.size, P.nx)), out["gx"][0]])
        approx.dfdu = np.zeros((approx.f.size, 0))
        return approx
