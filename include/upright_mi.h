/* upright_mi.h -- C-ABI of libupright_mi.so, the MI355X-native batched MPC engine.
 *
 * Drop-in boundary for the reference's hot path.  Every entry point names the
 * reference interface it replaces (paths relative to the reference repository root).  Plain C types
 * only: pointers, sizes, doubles.  All functions return 0 on success, non-zero on failure, and
 * upr_last_error() returns the message (the Python shim raises it as RuntimeError, mirroring how
 * the reference's std::runtime_error surfaces through pybind11).
 *
 * Device policy: every compute entry point runs hand-written HIP kernels on the current HIP device.
 * There is NO CPU fallback: without a GPU the calls fail with an error.
 */
#ifndef UPRIGHT_MI_H
#define UPRIGHT_MI_H

#ifdef __cplusplus
extern "C" {
#endif

#define UPR_MAX_JOINTS 12
#define UPR_MAX_CONTACTS 32
#define UPR_MAX_BODIES 8
#define UPR_MAX_WAYPOINTS 8
#define UPR_MAX_NX 36  /* 3 * UPR_MAX_JOINTS */
#define UPR_MAX_NU 108 /* UPR_MAX_JOINTS + 3 * UPR_MAX_CONTACTS */
#define UPR_MAX_SPHERES 16
#define UPR_MAX_PAIRS 32
#define UPR_MAX_DYN 4     /* dynamic obstacles (dimensions.h:32-45: the state carries 9 entries per obstacle) */

/* Problem family shared by all instances of a batch: what ControllerInterface's constructor reads
 * from ControllerSettings (upright_control/src/controller_interface.cpp:103-393;
 * upright_control/include/upright_control/controller_settings.h:47-119). */
typedef struct upr_problem {
    /* dims: upright_control/include/upright_control/dimensions.h:18-46 */
    int nq; /* robot joints (nq == nv); x = [q, v, a] */
    int nb; /* balanced bodies */
    int nc; /* contact points */
    int nf; /* 3 = frictional contact forces, 1 = frictionless (normal force only) */
    int N;  /* shooting intervals: time_horizon / dt (controller.yaml:13,55) */
    double dt;

    /* serial chain (replaces the Pinocchio model of upright_control/include/upright_control/util.h:15-65):
     * joint frame i = parent * (R_i, p_i) * motion(axis_i, q_i); type 0 prismatic, 1 revolute */
    int joint_type[UPR_MAX_JOINTS];
    double joint_axis[UPR_MAX_JOINTS][3];
    double joint_R[UPR_MAX_JOINTS][9];
    double joint_p[UPR_MAX_JOINTS][3];
    double tool_R[9];
    double tool_p[3];

    double gravity[3]; /* controller.yaml:6 */

    /* contacts: upright_core/include/upright_core/contact.h:10-46; body index -1 = EE / fixture */
    int contact_body1[UPR_MAX_CONTACTS];
    int contact_body2[UPR_MAX_CONTACTS];
    double contact_mu[UPR_MAX_CONTACTS];
    double contact_normal[UPR_MAX_CONTACTS][3];
    double contact_span[UPR_MAX_CONTACTS][6];
    double contact_r1[UPR_MAX_CONTACTS][3];
    double contact_r2[UPR_MAX_CONTACTS][3];

    /* costs: controller_interface.cpp:400-420, cost/end_effector_cost.h:33-84 */
    double Qdiag[UPR_MAX_NX];
    double Rdiag[UPR_MAX_NU];
    double xd[UPR_MAX_NX];
    double Wee[6]; /* diagonal of the end-effector pose weight: position (3), orientation error (3) */

    /* bounds: controller_interface.cpp:157-169,330-357 */
    double x_lb[UPR_MAX_NX], x_ub[UPR_MAX_NX];
    double u_lb[UPR_MAX_NU], u_ub[UPR_MAX_NU];

    /* target waypoint times (positions are per instance): reference_trajectory.h:18-47 */
    int n_way;
    double way_t[UPR_MAX_WAYPOINTS];

    /* solver settings: upright_control/src/pybindings.cpp:183-213, controller.yaml:54-72 */
    int sqp_iters;
    int qp_iter_max;
    double qp_tol;
    double delta_tol;
    double cost_tol;
    int terminal_constraint; /* stationary_desired_position_constraint at knot N */
    int use_feedback_policy; /* sqp.use_feedback_policy (controller.yaml:60; pybindings.cpp:199): keep the Riccati gains of
                                the last QP and apply them in upr_batch_evaluate_policy */

    /* collision avoidance (controller_interface.cpp:172-228,450-481; obstacles/simple.yaml:11-41): spheres rigidly
     * attached to chain frames (sph_frame: -1 world, i < nq the link carried by joint i, nq the tool frame) and the
     * pairs whose distance |c_a - c_b| - r_a - r_b - obs_min_dist stays >= 0 at knots 1..N-1 (hard state
     * inequality "obstacle_avoidance"; replaces ocs2::SelfCollisionConstraintCppAd over hpp-fcl sphere pairs) */
    int n_sph;
    int sph_frame[UPR_MAX_SPHERES];
    double sph_off[UPR_MAX_SPHERES][3];
    double sph_r[UPR_MAX_SPHERES];
    int n_pairs;
    int pair_a[UPR_MAX_PAIRS], pair_b[UPR_MAX_PAIRS];
    double obs_min_dist; /* controller.yaml:108 */
    /* pair_b == -1: the ground half-space z >= 0 (controller_interface.cpp:93-101).
     * n_dyn (0 .. UPR_MAX_DYN) dynamic obstacles (system_dynamics.h:29-39, dimensions.h:32-45; obstacles/dynamic.yaml): the
     * state handed to set_observation / returned by get_solution / evaluate is [robot x (3 nq), then r, v, a (9) of every
     * obstacle in turn]; an obstacle is uncontrolled, so inside the solve it is the ballistic function of time of its
     * observed state.  Spheres with sph_frame == -2 - i ride on obstacle i (-2: the first).  The projectile-path rows below
     * follow the LAST obstacle (projectile_path_constraint.h:82,114 read state.tail(9)). */
    int n_dyn;
    /* projectile_path_constraint.h:12-167 ("projectile_constraint"): rows w s (|c_i - r_closest| - dist_i),
     * w = proj_scale / dist_i, c_i the centre of sphere proj_sph[i], r_closest the closest future point of the
     * obstacle's path, s the per-instance activation flag (upr_batch_set_projectile_flag) */
    int n_proj;
    int proj_sph[8];
    double proj_dist[8];
    double proj_scale;
    /* soft constraints: ocs2 hpipm_interface SlackSettings (upright_control/src/pybindings.cpp:160-181; values
     * upright_control/src/upright_control/wrappers.py:121-143).  A softened row c(z) >= 0 becomes c(z) + sigma >= 0,
     * sigma >= 0, with cost 1/2 Z sigma^2 + z sigma (Z: L2, z: L1 penalty; "lower" for lower bounds and polytopic
     * rows, "upper" for upper bounds). */
    int soft_state_box, soft_input_box, soft_poly;
    double soft_L2_lower, soft_L2_upper, soft_L1_lower, soft_L1_upper;
    /* soft_eq: the object-dynamics equality is softened as well.  ocs2's HPIPM interface hands state-input equalities to
     * HPIPM as general (polytopic) constraints with lg = ug, so `slacks.poly_ineq` puts a slack pair on every such row:
     * lg - sl <= C dx + D du + e <= ug + su.  With equal L2 penalties Z and no L1 penalty (the reference's defaults,
     * wrappers.py:121-143) eliminating the pair leaves the quadratic penalty Z/2 |C dx + D du + e|^2, i.e. the
     * regularised equality C dx + D du + e = nu / Z -- the Schur complement S = Df Hff^-1 Df' + I / Z.  This is what
     * makes the frictionless multi-body problems of upright_robust (config/demos/_base.yaml:62-75) solvable at all:
     * with hard rows they admit no motion ("config 4").  Requires soft_L2_lower == soft_L2_upper > 0 and zero
     * L1 penalties. */
    int soft_eq;
    /* tolerance of the stationarity residual of the QP (HPIPM's tol_stat / res_g_max; ocs2's hpipm_interface::Settings
     * keeps it at 1e-6 next to 1e-8 for the equality, inequality and complementarity residuals, which `qp_tol` carries:
     * below ~1e-7 the stationarity residual of these problems is roundoff of the factorisation once the barrier
     * parameter is small).  <= 0: use qp_tol. */
    double qp_tol_stat;
    /* end-effector box (end_effector_box_constraint.h:47-76, "end_effector_box_constraint"; controller.yaml:91-94): with
     * ee_box != 0 the end-effector position p(q) stays inside p_d(t) + [ee_box_lower, ee_box_upper] at knots 1..N-1, p_d the
     * interpolated target position of the end-effector cost.  Six state rows per knot, upper rows first:
     * [p_d + ee_box_upper - p (3); p - (p_d + ee_box_lower) (3)], Jacobian [-J_p; J_p] in the q columns.  They are appended
     * to the state-row block, whose slot order is [collision pairs n_pairs][projectile n_proj][box upper 3][box lower 3];
     * softened by soft_poly like the other state-polytopic rows. */
    int ee_box;
    double ee_box_lower[3], ee_box_upper[3];
} upr_problem;

const char* upr_last_error(void);
/* 1 if a HIP device is usable, else 0 (never initialises anything else) */
int upr_device_available(void);
/* One process per GPU (torch.distributed launchers hand every rank its LOCAL_RANK): select the HIP device the NEXT
 * upr_batch_create of this thread uses.  A handle remembers its device (upr_batch_device) and every call on it makes that device
 * current first.  The reference has no counterpart (one CPU solver per process). */
int upr_set_device(int device);

/* ------------------------------------------------------------------------------------------------
 * upright_core.bindings twins (upright_core/src/pybindings.cpp:53-56).  Batched: n states at once.
 * contact/body tables come from `P` (nq, chain and cost fields are ignored).
 *   upr_core_object_dynamics  <-> compute_object_dynamics_constraints (contact_constraints.h:162-194)
 *       forces[n][nf*nc], C[n][9] row-major world<-EE, w/al/a[n][3]  ->  out[n][6*nb] (UNnormalised)
 *   upr_core_friction_rows    <-> compute_contact_force_constraints_linearized (contact_constraints.h:50-77)
 *       forces[n][3*nc] -> out[n][5*nc]
 * body_params[nb][10] = [m, m*c, vech(I)] (rigid_body.h:47-51). Host pointers. */
int upr_core_object_dynamics(const upr_problem* P, const double* body_params, int n, const double* forces,
                             const double* C, const double* w, const double* al, const double* a, double* out);
int upr_core_friction_rows(const upr_problem* P, int n, const double* forces, double* out);

/* ------------------------------------------------------------------------------------------------
 * Batched MPC: B independent instances of the same problem family.  One instance with B = 1 is what
 * `bindings.ControllerInterface` (upright_control/src/pybindings.cpp:364-427) wraps.
 * Per-instance data: body_params[B][nb][10] (the upright_robust parameter axis,
 * balancing_constraints.cpp:92-102), way_p[B][n_way][3] (targets, wrappers.py:31-43). */
typedef struct upr_batch upr_batch;

upr_batch* upr_batch_create(const upr_problem* P, int B, const double* body_params, const double* way_p);
void upr_batch_destroy(upr_batch* h);

/* ControllerInterface.reset / setTargetTrajectories (pybindings.cpp:371-374): new targets, forget
 * the previous solution (next advance starts from the DefaultInitializer guess,
 * controller_interface.cpp:385-386). way_p may be NULL to keep targets. */
int upr_batch_reset(upr_batch* h, const double* way_p);

/* Target orientations (the quaternion part of ocs2::TargetTrajectories states, wrappers.py:31-43: Q_d = Q_EE(x0) (x) Q_offset):
 * way_q[B][n_way][4], xyzw; between waypoints the target is their SLERP (reference_trajectory.h:18-47).  They enter the
 * end-effector cost through its orientation error (cost/end_effector_cost.h:33-84) when Wee[3..5] != 0.  Default: identity. */
int upr_batch_set_target_orientations(upr_batch* h, const double* way_q);

/* ControllerInterface.setObservation (pybindings.cpp:369-370): t[B] (or t[1] broadcast if
 * t_stride == 0), x[B][nx_full], nx_full = 3 nq + 9 n_dyn. Host pointers.  Every x / xs argument of this interface has
 * nx_full entries per state; the feedback gains have nx_full columns (zero for the obstacle part). */
int upr_batch_set_observation(upr_batch* h, const double* t, int t_stride, const double* x);

/* Overwrite the initial guess (operating points, controller_interface.cpp:376-383): xs[B][N+1][nx],
 * us[B][N][nu]. */
int upr_batch_set_guess(upr_batch* h, const double* xs, const double* us);

/* ControllerInterface.advanceMpc (pybindings.cpp:375): one MPC solve = `sqp_iters` SQP iterations
 * (linearise -> QP -> filter line search) for every instance, all on the GPU. */
int upr_batch_advance(upr_batch* h);

/* SQP iterations of the NEXT advance only (afterwards `sqp_iters` of the problem again): ocs2's solver runs
 * sqp.init_sqp_iteration iterations while it has no previous solution -- the first solve after construction or reset, and
 * every solve with mpc.cold_start (upright_control/src/pybindings.cpp:148,194-195; controller.yaml:15,56-57;
 * upright_robust/config/demos/_base.yaml:64-65 sets 3).  n = 0 cancels. */
int upr_batch_set_sqp_iterations(upr_batch* h, int n);

/* Same, but inputs stay in HBM and no host synchronisation is done (used by bench.py so that the
 * timed region contains only device work); upr_batch_sync waits for completion. */
int upr_batch_advance_async(upr_batch* h);
int upr_batch_sync(upr_batch* h);

/* ControllerInterface.getMpcSolution (pybindings.cpp:376-377): ts[B][N+1], xs[B][N+1][nx], us[B][N][nu] */
int upr_batch_get_solution(upr_batch* h, double* ts, double* xs, double* us);

/* ControllerInterface.evaluateMpcSolution (pybindings.cpp:378-381): interpolate the stored solution
 * at time t[B] -> x_out[B][nx], u_out[B][nu] (feed-forward policy). */
int upr_batch_evaluate(upr_batch* h, const double* t, int t_stride, double* x_out, double* u_out);

/* Linear feedback policy of the last solve (sqp.use_feedback_policy = true: the primal solution carries an
 * ocs2::LinearController, evaluated by ControllerPythonInterface::evaluateMpcSolution with the CURRENT state,
 * controller_python_interface.h:46-55):
 *     u(t, x) = (1 - a) [u_j + K_j (x - x_j)] + a [u_j+1 + K_j+1 (x - x_j+1)],   t = t_j + a dt
 * K_j are the Riccati gains of the last QP (sign convention of ocs2: u = bias + K x).  x_obs[B][nx], outputs as
 * upr_batch_evaluate.  Needs use_feedback_policy != 0 at creation.
 * The gains are formed on demand: an advance leaves them in the factors of its last QP, and this call forms the one or two knots
 * it interpolates between from there, per instance, in the evaluating kernel -- no array of all gains is written for it. */
int upr_batch_evaluate_policy(upr_batch* h, const double* t, int t_stride, const double* x_obs, double* x_out, double* u_out);
/* One control period of the reference's loop in ONE call and one synchronisation: what ControllerManager.step does with three
 * (manager.py:156-176: setObservation(t, x) -> advanceMpc() -> evaluateMpcSolution(t, x, x_opt, u_opt)), for callers that replan
 * every period.  The observation is uploaded once (the policy is evaluated at the state that was just observed, at its own time),
 * transfers go through the engine's pinned staging buffer, and the statistics of the solve come back with the result.
 * x[B][nx_full] observed states, x_out[B][nx_full], u_out[B][nu] as upr_batch_evaluate[_policy]; stats_out[B][UPR_NSTATS] or NULL.
 * Results are bit-identical to the three calls.  The policy reads knot 0 of the plan just solved straight from the QP's factors
 * (upr_batch_evaluate_policy): a period forms the gains of that one knot and writes no gain array.
 * From the third period in a row that enqueues the same operations (warm start, same SQP iteration count, no event timing ...)
 * the period's stream operations -- copies in, prepare, linearise, QP, line search, policy, copies out -- are replayed as ONE HIP
 * graph launch (UPR_TICK_GRAPH=0: never); upr_batch_tick_graph_replays counts the periods served that way. */
int upr_batch_tick(upr_batch* h, const double* t, int t_stride, const double* x, double* x_out, double* u_out, double* stats_out);
long long upr_batch_tick_graph_replays(upr_batch* h);

/* ControllerInterface.getLinearFeedbackGain (pybindings.cpp:382-384) at the knots: K[B][N][nu][nx]; jerk rows from the
 * Riccati recursion, contact-force rows from the elimination of the object-dynamics equality
 * (f = f* - Hff^-1 Df' S^-1 C dx).
 * The whole array is formed at the first call after an advance (one gather kernel over the QP's factors; the device array,
 * B N nu nx doubles, is allocated at the first call on the handle); further calls until the next advance only copy.  Calls that
 * solve another QP on the handle (upr_batch_qp_kkt, upr_batch_qp_step, upr_batch_value_function_update) gather it first, so the
 * gains stay those of the last advance.  UPR_FB_FUSED=1 | 0 at creation: the array with every advance instead, written by the QP
 * kernel's exit | by the gather kernel behind it. */
int upr_batch_get_feedback(upr_batch* h, double* K);

/* activation flag of the projectile constraint per instance: the 8th entry of the target state
 * (reference_trajectory.h; set by the target-flag protocol of mrt_node.cpp:243-265).  s[B]; default 0. */
int upr_batch_set_projectile_flag(upr_batch* h, const double* s);

/* ControllerInterface.getLastSolveTime (pybindings.cpp:366), milliseconds of the last advance */
double upr_batch_last_solve_ms(const upr_batch* h);

/* per-instance statistics of the last advance: stats[B][UPR_NSTATS] =
 * [sqp_iters_done, qp_iters_last, qp_status_last, step_alpha_last, cost, constraint_violation,
 *  qp_res_stat, qp_res_eq, qp_res_ineq, qp_res_comp, dx_norm, du_norm] */
#define UPR_NSTATS 12
int upr_batch_get_stats(upr_batch* h, double* stats);
/* restore == 0: keep a copy of the statistics and of the QP dispatch keys of the last advance; restore != 0: put it back.  Brackets
 * a solver-level query that solves one more QP on the handle (upr_batch_qp_kkt behind ControllerInterface.valueFunction,
 * pybindings.cpp:398-403): afterwards the statistics describe the solve again (ocs2's getValueFunction does not disturb its solver). */
int upr_batch_hold_stats(upr_batch* h, int restore);

/* ------------------------------------------------------------------------------------------------
 * Term-level access (ControllerInterface.getStateInputEqualityConstraintValue("object_dynamics"),
 * getStateInputInequalityConstraintValue("contact_forces"), getCostValue, pybindings.cpp:414-424;
 * BalancingConstraintWrapper.getLinearApproximation, balancing_constraint_wrapper.h:45-60).
 * Evaluates the per-knot linearisation kernel on arbitrary (x, u) pairs of instance family `h`:
 *   n points, inst[n] instance index of each point (body parameters / target), t[n], x[n][nx], u[n][nu]
 *   g[n][ne], gx[n][ne][nx]             object_dynamics equality and d/dx   (ne = 6 nb)
 *   cost[n], grad[n][nq], hess[n][nq][nq]  end-effector cost, gradient and Gauss-Newton Hessian
 *   ee[n][3]                            end-effector position
 * Any output pointer may be NULL. */
int upr_batch_linearize_points(upr_batch* h, int n, const int* inst, const double* t, const double* x,
                               const double* u, double* g, double* gx, double* cost, double* grad,
                               double* hess, double* ee);
/* ControllerInterface.getStateInputInequalityConstraintValue("obstacle_avoidance", t, x, u) (pybindings.cpp:417-419;
 * mpc_sim.py:191-219) at n states: d[n][n_pairs + n_proj] and (may be NULL) dq[n][n_pairs + n_proj][nq] = d d / d q.  The
 * end-effector box rows are not among them (upr_batch_state_rows); fails when the problem has no pairs / projectile rows. */
int upr_batch_obstacle_rows(upr_batch* h, int n, const double* x, double* d, double* dq);
/* Every state row at n points (instance inst[n], time t[n], interface state x[n][nx_full]): d[n][no] and (may be NULL)
 * dq[n][no][nq], no = n_pairs + n_proj + (ee_box ? 6 : 0), in the slot order of the record's row block
 * [pairs][projectile][box upper 3][box lower 3].  The box rows depend on t and on the instance's targets
 * (getStateInputInequalityConstraintValue("end_effector_box_constraint", t, x, u)). */
int upr_batch_state_rows(upr_batch* h, int n, const int* inst, const double* t, const double* x, double* d, double* dq);
/* constant d(object_dynamics)/du of instance `inst`: gu[ne][nu] */
int upr_batch_eq_input_jacobian(upr_batch* h, int inst, double* gu);

/* One QP (the SQP sub-problem at the current trajectory of every instance) without the line
 * search: dxs[B][N+1][nx], dus[B][N][nu].  For QP-level parity tests. */
int upr_batch_qp_step(upr_batch* h, double* dxs, double* dus);

/* The same QP with the multipliers it ended with, for an independent check of the optimality conditions
 * (tests/kkt_check.py assembles the QP in numpy from upr_batch_get_lin and the problem constants): pi[B][N+1][nx]
 * costates of the dynamics (pi_0 unused), nu[B][N][ne] multipliers of the object-dynamics rows, yN[B][3 + 2 nq] of the
 * terminal equality, lam[B][N+1][ni] of the inequality rows with ni = 2 nx + 2 nu + np + no in the slot order
 * [x lower][x upper][u lower][u upper][friction rows][state rows: collision pairs, projectile rows, end-effector box upper 3,
 * lower 3]; *ni_out = ni.  Pointers may be NULL.
 * With dynamic obstacles (n_dyn > 0) dxs has the interface width, dxs[B][N+1][nx + 9 n_dyn], with a zero obstacle block as
 * upr_batch_qp_step returns it (the obstacle is data of the QP); pi keeps the robot block, pi[B][N+1][nx]. */
int upr_batch_qp_kkt(upr_batch* h, double* dxs, double* dus, double* pi, double* nu, double* yN, double* lam, int* ni_out);
/* Slacks t[B][N+1][ni] of the inequality rows at the exit of the QP the last upr_batch_qp_kkt call solved (slot order of lam; 1 in
 * slots that are not rows of the knot).  lam / t are the barrier weights of the last interior-point iterate: with the costates they
 * are what the reference's solver-level queries -- valueFunction, valueFunctionStateDerivative,
 * stateInputEqualityConstraintLagrangian, upright_control/src/pybindings.cpp:398-412 (ocs2 getValueFunction = the Riccati
 * cost-to-go of the last QP, HPIPM's barrier-augmented P_k) -- are served from (upright_amd/value_function.py). */
int upr_batch_qp_slacks(upr_batch* h, double* t);
/* Slack pairs of the softened rows of that QP (HPIPM slacks, `soft_*` above): sigma[B][N+1][ni] the slack variable of the row (cost
 * 1/2 Z sigma^2 + z sigma), tau and gam the slack and the multiplier of sigma >= 0, slot order of lam; sigma = 0, tau = 1, gam = 0 in slots
 * that are not softened rows of the knot.  The kernels factor such a row with the weight w0 (Z + gam / tau) / (Z + w0 + gam / tau),
 * w0 = lam / t.  Same lifetime as upr_batch_qp_slacks; any pointer may be NULL. */
int upr_batch_qp_slack_pairs(upr_batch* h, double* sigma, double* tau, double* gam);

/* ------------------------------------------------------------------------------------------------
 * Value function of the last QP for the whole batch (ControllerInterface.valueFunction / valueFunctionStateDerivative,
 * upright_control/src/pybindings.cpp:398-402 -> ocs2 getValueFunction: the Riccati cost-to-go of the solver's last QP), on the device.
 *   upr_batch_value_function_update  linearises at the current plan, solves one QP there with the multiplier export and runs the
 *       cost-to-go kernel (upright_amd/csrc/upr_value.h): P_k, p_k, J_k and the expansion points X_k of every instance and knot stay
 *       in device memory.  Softened inequality rows enter with the weight above, a softened equality with S = Df Hff^-1 Df' + I / Z.
 *       Statistics and QP dispatch keys of the last advance are put back afterwards (as upr_batch_hold_stats does).  Every query
 *       behind it has robot-state shapes: a handle with dynamic obstacles is refused, as before.
 *   upr_batch_value_function_update_interface  the same update for any handle, dynamic obstacles included: the caller accepts the
 *       interface-state convention of upr_batch_value_function below.  Without a dynamic obstacle the two entries are one.
 *   upr_batch_track_value_function(h, on)  tracked mode: every advance and tick with at least one SQP iteration hands ITS OWN last QP
 *       to the cost-to-go kernel, in-stream between that QP launch and its line search: no second linearisation, no extra QP, no
 *       synchronisation.  The expansion point X_k = xs_lin + dx is that QP's solution -- ocs2's getValueFunction semantics: with a
 *       line-search step alpha < 1 the plan the advance stores differs from X.  (upr_batch_value_function_update describes the QP at
 *       the finished plan instead: one SQP iteration past it.)  Switching on allocates the buffers; never call it inside an advance
 *       (between upr_batch_advance_async and upr_batch_sync).  A tracked cost-to-go belongs to the solve: it stays valid across
 *       upr_batch_set_observation until the next advance or tick replaces it; upr_batch_reset, upr_batch_reset_async,
 *       upr_batch_set_guess and switching tracking off make it stale.  A tick's captured graph carries the kernel and the copy of
 *       the plan's time as two more nodes of its one chain.
 *   upr_batch_value_function  V[n] and dVdx[n][nx] at n points (inst[n], t[n], x[n][nx]):
 *       V(t, x) = J + p'(x - X) + 1/2 (x - X)'P (x - X),  dV/dx = p + P (x - X), of the two knots around t, interpolated linearly in t
 *       (t is clamped to the plan's horizon).  Fails before the first update, and with "stale" once the plan or the observation
 *       changed since the update (advance, tick, reset, set_guess, set_observation).  With dynamic obstacles (n_dyn > 0) the points
 *       are interface states, x[n][nx + 9 n_dyn], and dVdx[n][nx + 9 n_dyn] comes back with a ZERO obstacle block: the obstacle is
 *       data of the QP the engine solves, not a state of its Riccati recursion.
 *   upr_batch_equality_lagrangian  nu_out[n][ne] at n points (inst[n], t[n]): the multipliers of the object-dynamics rows of the
 *       same QP (stateInputEqualityConstraintLagrangian, pybindings.cpp:409-412), piecewise linear between the knots; the last knot
 *       carries none, so the last interval holds nu[N-1].  Same validity as upr_batch_value_function.
 *   upr_batch_get_cost_to_go  Pk[B][N+1][nx][nx], pk[B][N+1][nx], J[B][N+1], X[B][N+1][nx]; any pointer may be NULL.  Robot-block shapes
 *       with and without dynamic obstacles.
 *   upr_batch_value_function_ms  device time (ms) of the last cost-to-go launch, HIP events around that launch only (a tracked launch
 *       is timed only on a handle with upr_batch_enable_timing on; reading it waits for that launch). */
int upr_batch_value_function_update(upr_batch* h);
int upr_batch_value_function_update_interface(upr_batch* h);
int upr_batch_track_value_function(upr_batch* h, int on);
int upr_batch_equality_lagrangian(upr_batch* h, int n, const int* inst, const double* t, double* nu_out);
int upr_batch_value_function(upr_batch* h, int n, const int* inst, const double* t, const double* x, double* V, double* dVdx);
int upr_batch_get_cost_to_go(upr_batch* h, double* Pk, double* pk, double* J, double* X);
double upr_batch_value_function_ms(upr_batch* h);

/* ------------------------------------------------------------------------------------------------
 * Balance check under inertial-parameter scenarios: does a state stay balanced when the true parameters are not the ones it was
 * planned with?  Replaces the off-line test of upright_robust/scripts/process_sim_runs.py:87-270 (is the wrench an object needs
 * inside the contact wrench cone of upright_robust/src/upright_robust/modelling.py:106-132), batched on the device
 * (upright_amd/csrc/upr_balance.h: a state kernel and a Lawson-Hanson projection in fp64 -- a lane per job with the passive system
 * in registers for one-body arrangements, a wave per job with the passive system in LDS for every other shape).
 *   For a robot state x = [q, v, a], parameters theta[nb][10] (the layout of body_params) and the handle's arrangement:
 *       rho(x; theta) = min over z >= 0 of | b + A z |_2,   b = g(x, f = 0; theta),   A = dg/df(theta) S,
 *   g the object-dynamics residual exactly as the linearisation records it (per body divided by its mass, the whole vector by
 *   sqrt(6 nb)), S the generators of the friction pyramids, contact by contact in the order n + mu s0, n + mu s1, n - mu s0,
 *   n - mu s1 (nf = 3: ncol = 4 nc) or the normal alone (nf = 1: ncol = nc); contact forces are f = S z.  rho is the distance, in the
 *   units of the constraint the controller enforces, from the needed wrench to the contact wrench cone: rho = 0 if and only if
 *   balancing forces exist.  The force bounds u_lb / u_ub are NOT part of it.  Levers and 1 / m in A follow theta, not the
 *   handle's own parameters.  rho is unique, z is not.
 *   Stopping rule (UPR_BAL_TOL of upr_balance.h, 1e-14): a column enters only while -a_j' r > tol |a_j| max(|b|, 1); iteration cap
 *   3 ncol least-squares solves -- a job that reaches it reports exactly that count in iters.
 *   upr_batch_balance_points  n states x[n][3 nq] (robot states, also with dynamic obstacles) times n_scen scenarios:
 *       params[n_scen][nb][10] shared by all points (per_point == 0) or params[n][n_scen][nb][10] (per_point == 1);
 *       rho[n][n_scen], z[n][n_scen][ncol] or NULL, iters[n][n_scen] or NULL.  Host pointers.
 *   upr_batch_balance_plan  the knots of the handle's current plan where they lie on the device (no host copy of xs), enqueued on
 *       the handle's stream behind whatever is in flight, one synchronisation at the end: rho[B][N+1][n_scen], iters likewise or
 *       NULL.  params == NULL with n_scen == 1: each instance against its own body_params (the nominal check); else
 *       params[n_scen][nb][10], or params[B][n_scen][nb][10] with per_instance != 0.
 *   Both leave the plan, statistics, dispatch keys, warm start, value-function validity and tick graph exactly as they were. */
int upr_batch_balance_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point,
                             double* rho, double* z, int* iters);
int upr_batch_balance_plan(upr_batch* h, int n_scen, const double* params, int per_instance, double* rho, int* iters);
/* The same two calls with friction as a scenario axis (the --mu of process_sim_runs.py): mu_scale[n_scen], finite and >= 0, scales
 * every contact's friction coefficient in the generators of scenario s (mu_i -> mu_scale[s] mu_i; nf = 1 generators carry no mu);
 * NULL means ones, and a scale of exactly 1 gives the answer of the call without it bit for bit.  The two calls above are these
 * with NULL. */
int upr_batch_balance_points_mu(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point,
                                const double* mu_scale, double* rho, double* z, int* iters);
int upr_batch_balance_plan_mu(upr_batch* h, int n_scen, const double* params, int per_instance, const double* mu_scale, double* rho,
                              int* iters);

/* ------------------------------------------------------------------------------------------------
 * Friction margin (upright_amd/csrc/upr_margin.h): the smallest common scale kappa* on the arrangement's friction coefficients at
 * which balancing forces exist -- one launch instead of a --mu sweep, and the signed quantity rho is not.  With rho(x; theta, kappa)
 * the distance above on the generators of kappa mu_i,
 *       kappa*(x; theta) = inf { kappa in [0, kappa_max] : rho(x; theta, kappa) <= 1e-8 max(|b|, 1) },   +inf if kappa_max fails
 *   (1e-8, UPR_BAL_FEAS: the tolerance the controller's QP enforces the equality to).  kappa* < 1: balanced, 1 - kappa* of the
 *   friction could be lost; > 1: this much more friction would have been needed; 0: normal forces alone balance the state; +inf: no
 *   friction helps (tipping, lift-off).  The smallest friction coefficient of contact i is kappa* mu_i.  The force bounds are NOT
 *   part of it, and kappa* carries the 1e-8 rule: it lies below the exact boundary by what that ball allows.
 *   rho at 0, then at kappa_max, then 32 halvings (UPR_BAL_BISECT), every one a cold projection of the rho calls:
 *       kappa_hi  the answer: the last feasible point (0: the first evaluation passed; +inf: kappa_max failed);
 *       kappa_lo  the last infeasible point (0 with kappa_hi = 0; kappa_max with kappa_hi = +inf); kappa_hi - kappa_lo <= kappa_max 2^-32;
 *       z         multipliers at kappa_hi: z >= 0 and |b + A(kappa_hi) z| <= 1e-8 max(|b|, 1) (zeros with kappa_hi = +inf);
 *       y         b + A(kappa_lo) z of the projection at kappa_lo: y' a_j(kappa_lo) >= 0 for every generator and y' b > 0, so no
 *                 forces balance the state at kappa_lo (zeros with kappa_hi = 0);
 *       iters     least-squares solves over all evaluations, at most 34 * 3 ncol.
 *   upr_batch_friction_margin_points  layouts of upr_batch_balance_points: kappa_hi[n][n_scen], kappa_lo likewise or NULL,
 *       z[n][n_scen][ncol] or NULL, y[n][n_scen][6 nb] or NULL, iters[n][n_scen] or NULL.  Host pointers.
 *   upr_batch_friction_margin_plan  the knots of the current plan on the device, as upr_batch_balance_plan (params == NULL: n_scen
 *       == 1, every instance's own body_params): kappa_hi[B][N+1][n_scen], kappa_lo and iters likewise or NULL.
 *   kappa_max must be finite and > 0.  Both share the scratch of the balance check, report their device time through
 *   upr_batch_balance_ms and leave the handle as the balance check does. */
int upr_batch_friction_margin_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point,
                                     double kappa_max, double* kappa_hi, double* kappa_lo, double* z, double* y, int* iters);
int upr_batch_friction_margin_plan(upr_batch* h, int n_scen, const double* params, int per_instance, double kappa_max,
                                   double* kappa_hi, double* kappa_lo, int* iters);
/* The balance check with a friction scale per scenario AND contact: mu_scale_c[n_scen][nc], finite and >= 0, mu_i -> mu_scale_c[s][i]
 * mu_i.  upright_cmd/scripts/tools/compute_minimum_mu.py:12-30 gives every pair of objects its own friction coefficient; this is rho
 * for such a vector.  Rows that are uniform over the contacts give the bits of the _mu calls, all ones those of the plain calls. */
int upr_batch_balance_points_cmu(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point,
                                 const double* mu_scale_c, double* rho, double* z, int* iters);
int upr_batch_balance_plan_cmu(upr_batch* h, int n_scen, const double* params, int per_instance, const double* mu_scale_c, double* rho,
                               int* iters);
/* Friction margin per contact group: which interface binds a state (compute_minimum_mu.py:12-30, compute_contact_idx: one friction
 * coefficient per pair of objects).  group_mask[n_grp]: bit i of word g set -- contact i belongs to group g (groups may overlap;
 * every mask non-empty, no bit >= nc).  mu_base[n_scen][nc], finite and >= 0, or NULL (ones): the scale of the contacts outside the
 * group.  With A_g(kappa) built on kappa mu_i inside group g and mu_base[s][i] mu_i outside,
 *       kappa*_g = inf { kappa in [0, kappa_max] : rho_g(kappa) <= 1e-8 max(|b|, 1) },   +inf if kappa_max fails
 *   by the algorithm and with the outputs of the friction margin above, every one with a trailing group axis:
 *   kappa_hi[n][n_scen][n_grp], kappa_lo, iters likewise, z[n][n_scen][n_grp][ncol], y[n][n_scen][n_grp][6 nb].  kappa*_g = 0: the
 *   friction of group g is not needed; +inf: more friction on group g alone does not help.  One group of all contacts without
 *   mu_base gives the bits of upr_batch_friction_margin_points.  The force bounds u_lb / u_ub are NOT part of it.
 *   upr_batch_friction_margin_groups_plan  the knots of the current plan: kappa_hi[B][N+1][n_scen][n_grp] or NULL; worst[B][n_scen]
 *       [n_grp] or NULL: the largest kappa_hi over the knots (+inf counts as largest), reduced on the device, worst_knot (or NULL)
 *       the first knot that attains it -- with kappa_hi NULL only these are downloaded.  kappa_hi and worst must not both be NULL.
 *   Scratch, timing and the state of the handle as the friction margin above. */
int upr_batch_friction_margin_groups_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point,
                                            int n_grp, const unsigned* group_mask, const double* mu_base, double kappa_max,
                                            double* kappa_hi, double* kappa_lo, double* z, double* y, int* iters);
int upr_batch_friction_margin_groups_plan(upr_batch* h, int n_scen, const double* params, int per_instance, int n_grp,
                                          const unsigned* group_mask, const double* mu_base, double kappa_max, double* kappa_hi,
                                          double* kappa_lo, int* iters, double* worst, int* worst_knot);
/* ------------------------------------------------------------------------------------------------
 * Speed margin (upright_amd/csrc/upr_speed.h): the interval of uniform replay speeds at which a state is balanced.  A trajectory
 * replayed s times faster, q(t) -> q(s t), turns x = (q, v, a) into x_s = (q, s v, s^2 a); b(s) = b0 + s^2 (b1 - b0) and A does not
 * depend on s, so rho is convex in s^2 and the balanced speeds form one interval.  A speed is accepted iff rho(x_s; theta) <= 1e-8
 * max(|b(s)|, 1) (UPR_BAL_FEAS) on the cold projection of the rho calls, b(s) rebuilt from the scaled state at every evaluation.
 *   Evaluations lie on the grid s_max k 2^-32; the nominal speed is the grid point floor(2^32 / s_max), s = 1 itself for a power of
 *   two.  Rest and s_max first; both accepted: done.  Rest accepted: 32 halvings for the upper end.  Else a seed: the nominal speed,
 *   else s_max, else a descent search on the slope r' (b1 - b0) (32 halvings without an accepted point: no speed is accepted); then
 *   halvings of [0, seed] and, unless s_max is accepted, of [seed, s_max]: at most 3 + 3 * 32 evaluations.
 *       speed[4]  s_lo: the smallest accepted speed found (0 if rest is accepted); s_lo_out: the largest rejected speed below it (0
 *                 if none); s_hi: the largest accepted speed found (s_max if s_max is accepted); s_hi_out: the smallest rejected
 *                 speed above it (+inf if s_max is accepted).  No speed accepted: +inf, 0, -inf, s_max.  A bisected end has
 *                 |in - out| = s_max 2^-32; the reported ends are the accepted side.
 *       z[2]      multipliers at s_lo and at s_hi: z >= 0 and |b(s) + A z| <= 1e-8 max(|b(s)|, 1) (zeros without an accepted end);
 *       y[2]      the residual of the projection at s_lo_out and at s_hi_out: y' a_j >= 0 for every generator and y' b(s) > 0 (zeros
 *                 without a rejected end);
 *       iters     least-squares solves over all evaluations.
 *   upr_batch_speed_margin_points  layouts of upr_batch_balance_points: speed[n][n_scen][4], z[n][n_scen][2][ncol] or NULL,
 *       y[n][n_scen][2][6 nb] or NULL, iters[n][n_scen] or NULL.  Host pointers.
 *   upr_batch_speed_margin_plan  the knots of the current plan on the device, as upr_batch_balance_plan: speed[B][N+1][n_scen][4] or
 *       NULL, iters[B][N+1][n_scen] or NULL; window[B][n_scen][2] or NULL: the largest s_lo and the smallest s_hi over the knots,
 *       reduced on the device, knot[B][n_scen][2] (or NULL) the first knot attaining each -- with speed NULL only the reductions are
 *       downloaded; limit[B] or NULL: the largest s at which s v, s^2 a and s^3 u of every knot stay inside the velocity,
 *       acceleration and jerk boxes of the problem (+inf for a plan at rest).  speed and window must not both be NULL.
 *   s_max must be finite and > 1.  Scratch, timing and the state of the handle as the friction margin above. */
int upr_batch_speed_margin_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point, double s_max,
                                  double* speed, double* z, double* y, int* iters);
int upr_batch_speed_margin_plan(upr_batch* h, int n_scen, const double* params, int per_instance, double s_max, double* speed,
                                int* iters, double* window, int* knot, double* limit);
/* ------------------------------------------------------------------------------------------------
 * Path-acceleration margin (upright_amd/csrc/upr_pathacc.h): how hard a state can brake along its own path, or accelerate along it,
 * with the objects still balanced.  A trajectory replayed with the time scaling s(t) turns a knot x = (q, v, a) into x(s0, d) = (q,
 * s0 v, s0^2 a + d v), s0 = sdot (`speed`), d = sddot in 1 / s; d < 0 is braking (from sdot = 1, sddot = -beta stops the replay in
 * 1 / beta seconds if held).  b(d) = b(0) + d b2 and A does not depend on d, so rho^2 is convex in d and the balanced d form one
 * interval.  d is accepted iff rho(x(s0, d); theta) <= 1e-8 max(|b(d)|, 1) (UPR_BAL_FEAS) on the cold projection of the rho calls,
 * b(d) rebuilt from the transformed state at every evaluation.
 *   Evaluations lie on the grid d(k) = d_max (k - 2^31) 2^-31, k = 0 .. 2^32: -d_max, 0 and d_max are grid points.  The algorithm is
 *   the speed margin's with d = 0 as the nominal point: -d_max and d_max first; both accepted: done.  -d_max accepted: 32 halvings
 *   for the upper end.  Else a seed: d = 0, else d_max, else a descent search on the slope r' b2 (32 halvings without an accepted
 *   point: no d is accepted; its first midpoint is d = 0 again); then halvings on both sides of the seed.
 *       accel[4]  d_lo: the smallest accepted d found (-d_max if -d_max is accepted); d_lo_out: the largest rejected d below it (-inf
 *                 if none); d_hi: the largest accepted d found (d_max if d_max is accepted); d_hi_out: the smallest rejected d above
 *                 it (+inf if none).  No d accepted: +inf, -d_max, -inf, d_max.  A bisected end has |in - out| = d_max 2^-31; the
 *                 reported ends are the accepted side.  0 in [d_lo, d_hi] iff the state is balanced at speed s0; d_hi < 0: it is
 *                 balanced only while braking at least that hard; d_lo: the hardest balanced braking.
 *       z[2], y[2], iters   as the speed margin's, at d_lo / d_hi and at d_lo_out / d_hi_out.
 *   upr_batch_path_accel_margin_points  layouts of upr_batch_speed_margin_points: accel[n][n_scen][4], z[n][n_scen][2][ncol] or NULL,
 *       y[n][n_scen][2][6 nb] or NULL, iters[n][n_scen] or NULL.  Host pointers.
 *   upr_batch_path_accel_margin_plan  the knots of the current plan on the device, as upr_batch_speed_margin_plan: accel[B][N+1]
 *       [n_scen][4] or NULL, iters or NULL; window[B][n_scen][2] or NULL: the largest d_lo and the smallest d_hi over the knots,
 *       knot[B][n_scen][2] (or NULL) the first knot attaining each; limit[B][2] or NULL: the interval (lo, hi) of d for which
 *       s0^2 a_i + d v_i stays inside the acceleration box of every joint at every knot ((-inf, +inf) for a plan at rest; lo > hi
 *       when s0^2 a is outside the box already).  Jerk is not part of it: a step in sddot is an impulse of jerk.  accel and window
 *       must not both be NULL.
 *   d_max must be finite and > 0, speed finite and >= 0.  Scratch, timing and the state of the handle as the friction margin above. */
int upr_batch_path_accel_margin_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point,
                                       double d_max, double speed, double* accel, double* z, double* y, int* iters);
int upr_batch_path_accel_margin_plan(upr_batch* h, int n_scen, const double* params, int per_instance, double d_max, double speed,
                                     double* accel, int* iters, double* window, int* knot, double* limit);
/* ------------------------------------------------------------------------------------------------
 * Retiming on a speed lattice (upright_amd/csrc/upr_retime.h): the fastest time law s(t) that replays the geometric path of the current
 * plan with the objects balanced at every knot.  speeds[n_lvl]: the lattice s_0 < s_1 < .., finite, >= 0, 1 <= n_lvl <= 32.  A time
 * law gives every knot i = 0 .. N a level m_i; sddot is constant on every segment: d_i = (s_{m_{i+1}}^2 - s_{m_i}^2) / (2 dt), the
 * segment lasts 2 dt / (s_{m_i} + s_{m_{i+1}}), and an edge whose two speeds sum to 0 does not exist.  Edge (i, m -> m') is admissible
 * in a scenario iff the departing state x_i(s_m, d) and the arriving state x_{i+1}(s_m', d), x(s, d) = (q, s v, s^2 a + d v), are both
 * accepted by the rule of the margins above (rho <= 1e-8 max(|b|, 1) on the cold projection) and, with boxes != 0, s v and s^2 a + d v
 * of every joint lie inside the velocity and acceleration boxes of the problem at both ends (positions do not move; jerk is not
 * enforced: a step of sddot at a knot is an impulse of jerk).  The optimum is exact on the lattice: T[N][m] = 0 (only for end_level
 * when it is >= 0), T[i][m] = min over admissible m' of the segment's time + T[i + 1][m'], ties to the smallest m'; the law starts at
 * start_level, or (-1) at the level with the smallest T[0][.], ties to the smallest.
 *       duration  T at the start; +inf when no time law exists on the lattice
 *       level     [N + 1] the levels of the optimal law; all -1 when duration is infinite
 *       reach     (f, g): f the last knot with a non-empty set of levels reachable forward from the start, g the first knot that
 *                 has a level with finite T; (N, 0) for a feasible plan
 *       edges     the masks, bit m' of row (segment i, level m): the edge m -> m' is admissible;  iters: the least-squares solves of
 *                 a mask row (at most 2 n_lvl projections)
 *   params as upr_batch_speed_margin_plan.  common == 0: duration[B][n_scen], level[B][n_scen][N+1], reach[B][n_scen][2]; common != 0:
 *   one time law per instance that holds under every scenario (an edge must be admissible in all of them): duration[B], level[B][N+1],
 *   reach[B][2].  edges[B][n_scen][N][n_lvl] and iters[B][n_scen][N][n_lvl] are per scenario in both cases.  NULL outputs are not
 *   copied; duration and level must not both be NULL.  Scratch, timing and the state of the handle as the friction margin above. */
int upr_batch_retime_plan(upr_batch* h, int n_scen, const double* params, int per_instance, int n_lvl, const double* speeds, int start_level,
                          int end_level, int common, int boxes, double* duration, int* level, int* reach, unsigned* edges, int* iters);
/* Retiming with a reserve (upright_amd/csrc/upr_retime_rsv.h): the fastest time law on the lattice whose every end state still absorbs
 * the unplanned tray acceleration `reserve` along every +-u of dirs.  Lattice, edges, boxes, common, start / end, the programme, the
 * outputs, their layouts and the required-pointer refusal are upr_batch_retime_plan's; dirs[n_dir][6], frame and the unit of reserve
 * are the disturbance margin's below (1 <= n_dir <= 32, finite, no row all zero; frame 0: world, 1: tray, rotated by the end state's own
 * C_we); reserve r must be finite and >= 0.  An end state is accepted iff its record R is accepted and, when r > 0, R displaced by +r u_k
 * and by -r u_k is accepted for every k (the same rule, unchanged).  Evaluated in a fixed order -- R, then k ascending, +r before -r, an
 * end state stops at its first rejection, the departing state before the arriving one -- so iters (at most 2 n_lvl (1 + 2 n_dir)
 * projections per mask row) is reproducible.  With r == 0 no displaced record is evaluated and every output equals
 * upr_batch_retime_plan's bit for bit.
 *   Claimed: b is affine in (alpha, a_ee) and the cone is convex, so up to the ball of the rule acceptance at +-r u_k certifies the whole
 *   segment between them.  NOT claimed: anything about combinations of directions (as the disturbance margin's radius).
 *   upr_batch_disturbance_margin_* on the retimed states reports the radius a law achieves. */
int upr_batch_retime_plan_reserve(upr_batch* h, int n_scen, const double* params, int per_instance, int n_lvl, const double* speeds,
                                  int start_level, int end_level, int common, int boxes, int n_dir, const double* dirs, int frame,
                                  double reserve, double* duration, int* level, int* reach, unsigned* edges, int* iters);
/* Retiming with substeps (upright_amd/csrc/upr_retime_sub.h): the fastest time law on the lattice whose every segment is balanced at
 * substeps - 1 interior points of the path as well as at its two knots.  Lattice, edges, d, boxes, common, start / end, the programme,
 * the outputs, their layouts and the required-pointer refusal are upr_batch_retime_plan's; substeps = R must be 1 .. 16.  Segment i gets
 * the path points tau_r = r dt / R, r = 0 .. R: r = 0 and r = R are the knots i and i + 1, their records the plan's own; for 0 < r < R
 * the record is (Q, Q', Q'') of the quintic Hermite interpolant of upr_batch_replay_plan below at tau_r.  On the edge m -> m' the speed at
 * point r is s_r = sqrt(((R - r) s_m^2 + r s_m'^2) / R) (constant sddot makes s^2 linear in tau; s_0 = s_m, s_R = s_m' exactly), d is the
 * edge's, the state (Q, s_r Q', s_r^2 Q'' + d Q').  The edge is admissible iff it exists, with boxes s_r Q' and s_r^2 Q'' + d Q' of every
 * joint lie inside their boxes at every r, and all R + 1 states are accepted by the rule, unchanged.  Evaluated in a fixed order -- the
 * boxes at r = 0, R, then 1 .. R - 1; the projections departing, arriving, then r = 1 .. R - 1, stopping at the first rejection -- so
 * iters (at most n_lvl (R + 1) projections per mask row) is reproducible.  With substeps == 1 every output equals upr_batch_retime_plan's
 * bit for bit.
 *   Claimed: the law is balanced at the knots and at the R - 1 interior path points of every segment.  NOT claimed: anything between
 *   those points -- upr_batch_replay_plan on the returned law is the caller's check -- and jerk. */
int upr_batch_retime_plan_substeps(upr_batch* h, int n_scen, const double* params, int per_instance, int n_lvl, const double* speeds,
                                   int start_level, int end_level, int common, int boxes, int substeps, double* duration, int* level,
                                   int* reach, unsigned* edges, int* iters);
/* Replay of a time law on a clock (upright_amd/csrc/upr_replay.h): the states (q, qdot, qddot) of a retimed plan at t_k = t0 + k tick,
 * k = 0 .. n_samp - 1, and the balance of the objects at every one of them -- between the knots, where the retiming above claims
 * nothing.  speeds[n_lvl] as upr_batch_retime_plan's; level[B][N+1] ONE law per instance: lattice indices, or -1 throughout (no law);
 * a law must not hold speed 0 over a segment.  Knot times T_0 = 0, T_{i+1} = T_i + 2 dt / (s_i + s_{i+1}), summed in this order; the
 * duration is T_N.  A sample lies on the segment i with T_i <= t_k < T_{i+1} (on a knot: the departing side), at the path time tau of the
 * law's constant sddot; the path between two knots is, per joint, the quintic Hermite interpolant of their records (q, v, a), C2 across
 * the knots and equal to the plan's own cubic wherever the plan satisfies its dynamics; the state is (Q, s Q', s^2 Q'' + d Q').  Sample
 * k EXISTS iff t_k <= T_N.
 *       duration[B]              T_N, +inf without a law;
 *       count[B]                 the existing samples (the first count ones), 0 without a law;
 *       x[B][n_samp][3 nq]       the sample states; past the end the state at T_N, without a law (q_0, 0, 0);
 *       rho, excess[B][n_samp][n_scen]  the distance of the cold projection and excess = rho / max(|b|, 1): accepted iff excess <= 1e-8,
 *                                the rule of the friction margin; NaN for a sample that does not exist;
 *       iters[B][n_samp][n_scen] least-squares solves, 0 for a sample that does not exist;
 *       worst[B][n_scen]         the largest excess over the existing samples, NaN without any;
 *       verdict[B][n_scen][3]    (first sample attaining worst or -1, first rejected sample or -1, number rejected);
 *       box_first[B]             with boxes != 0 the first existing sample whose s Q' or s^2 Q'' + d Q' leaves the velocity or acceleration
 *                                box of some joint, else -1.  Positions do not move, jerk is not judged.
 *   params as upr_batch_speed_margin_plan (per_instance: a set per instance for all its samples).  tick must be finite and > 0, t0 finite
 *   and >= 0, 1 <= n_samp <= 65536.  Every output may be NULL and is then not copied; x, rho, excess and worst must not all be NULL; with
 *   x alone nothing is projected.  One level at speed 1 asks whether the plan as it stands is balanced between its knots.  Scratch,
 *   timing and the state of the handle as the friction margin above. */
int upr_batch_replay_plan(upr_batch* h, int n_scen, const double* params, int per_instance, int n_lvl, const double* speeds, const int* level,
                          double tick, double t0, int n_samp, int boxes, double* duration, int* count, double* x, double* rho, double* excess,
                          int* iters, double* worst, int* verdict, int* box_first);
/* ------------------------------------------------------------------------------------------------
 * Disturbance margin (upright_amd/csrc/upr_disturb.h): how much tray acceleration the plan did not choose a state absorbs along given
 * directions with the objects still balanced.  dirs[n_dir][6] holds rows u = (u_alpha, u_a), rad/s^2 and m/s^2 per unit r, 1 <= n_dir
 * <= 32, every entry finite, no row all zero; frame 0: world, the frame the state's omega, alpha and a_ee are in; frame 1: the tray
 * frame, u_world = C_we u_tray for both halves with the state's own C_we.  The state displaced by r along u has (alpha + r u_alpha,
 * a_ee + r u_a); b(r) = b(0) + r b_u and A does not depend on r, so the accepted r form one interval.  The rule, the grid r(k) =
 * r_max (k - 2^31) 2^-31 and the algorithm are the path-acceleration margin's (its special case u = (omega, v_ee), speed 1).
 *       reach[4]  r_lo, r_lo_out, r_hi, r_hi_out with the conventions of accel[4] above (open ends -inf / +inf; no r accepted: +inf,
 *                 -r_max, -inf, r_max; a bisected end has |in - out| = r_max 2^-31).  -r_lo is what the state absorbs along -u, r_hi
 *                 what it absorbs along +u; 0 in [r_lo, r_hi] iff the state is balanced.
 *       z[2], y[2], iters   as the path-acceleration margin's.
 *   The layouts are direction-major.  upr_batch_disturbance_margin_points: reach[n_dir][n][n_scen][4], z[n_dir][n][n_scen][2][ncol] or
 *       NULL, y[n_dir][n][n_scen][2][6 nb] or NULL, iters[n_dir][n][n_scen] or NULL.  Host pointers.
 *   upr_batch_disturbance_margin_plan  the knots of the current plan on the device: reach[n_dir][B][N+1][n_scen][4] or NULL, iters or
 *       NULL; window[n_dir][B][n_scen][2] or NULL: per direction the largest r_lo and the smallest r_hi over the knots, knot[n_dir][B]
 *       [n_scen][2] (or NULL) the first knot attaining each; radius[B][n_scen] or NULL: min over directions of min(-window_lo,
 *       window_hi), the largest r every knot absorbs along every +-u given -- negative when some knot is not balanced, -inf when some
 *       job accepts nothing; binding[B][n_scen][3] or NULL: (direction, sign -1 | +1, knot) of the end that attains radius, directions
 *       in ascending order, the lower end before the upper, the first end wins ties.  reach, window and radius must not all be NULL.
 *   r_max must be finite and > 0.  Scratch, timing and the state of the handle as the friction margin above. */
int upr_batch_disturbance_margin_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point,
                                        int n_dir, const double* dirs, int frame, double r_max,
                                        double* reach, double* z, double* y, int* iters);
int upr_batch_disturbance_margin_plan(upr_batch* h, int n_scen, const double* params, int per_instance,
                                      int n_dir, const double* dirs, int frame, double r_max,
                                      double* reach, int* iters, double* window, int* knot, double* radius, int* binding);
/* device time (ms) of the kernel launches of the last balance check, friction margin, speed margin, path-acceleration margin, retiming
 * (with or without a reserve), replay or disturbance margin on the handle, HIP events around them (copies excluded) */
double upr_batch_balance_ms(upr_batch* h);

/* raw device pointers for zero-copy consumers (torch / RCCL all-gather of solved trajectories):
 * xs (B*(N+1)*nx doubles) and us (B*N*nu doubles) */
int upr_batch_device_ptrs(upr_batch* h, void** xs, void** us);

/* average device time (ms) of each kernel over the last advance, measured with HIP events on the
 * engine's stream: out[0] = linearise, out[1] = QP, out[2] = line search; launches[3] = #launches */
int upr_batch_kernel_times(upr_batch* h, double* ms, int* launches);
/* on: 0 no events; 1 events around every kernel; 2 around the QP kernel only; 3 around every fourth QP launch (the first, the
 * fifth, ...).  A recorded event holds the stream for 3 - 4 us (tools/exp_timing_modes.py; 6 us under rocprofv3, whose
 * kernel trace shows no gap between two kernels without one): a throughput run that wants the dominant kernel's average duration and
 * nothing else asks for 3 */
int upr_batch_enable_timing(upr_batch* h, int on);
/* name of the QP kernel instantiation this handle launches (as rocprofv3 prints it): bench.py's roofline.kernel */
const char* upr_batch_qp_kernel_name(const upr_batch* h);
/* name of the line-search kernel instantiation the handle's last line-search launch ran (upr_linesearch_kernel<NQ, NT, NFM, NBM,
 * EXACT, OBS, STAGE>, as rocprofv3 prints it); "" before the first advance */
const char* upr_batch_ls_kernel_name(upr_batch* h);
/* name of the linearisation kernel instantiation the handle's last linearisation launch ran, in trajectory or points mode:
 * upr_linearize_kernel<NQ, USE_MFMA, OCC, ORI, NPASS> with every argument written out, or upr_linearize2_kernel<NQ> followed by
 * " kpw=<knots per workgroup> blocks=<workgroups>" of that launch; "" before the first launch */
const char* upr_batch_lin_kernel_name(upr_batch* h);
int upr_batch_device(const upr_batch* h);   /* the HIP device the handle lives on; -1 for a null handle */
/* doubles of device workspace per instance (QP result, multipliers, the QP kernel's far arrays): what an instance writes once and
 * re-streams every interior-point iteration -- bench.py's model of the compulsory DRAM traffic of a launch */
long long upr_batch_ws_doubles(const upr_batch* h);

/* copy the current solution into caller-owned DEVICE buffers (torch tensors handed to the RCCL
 * all-gather of solved trajectories): xs_dst[B][N+1][nx], us_dst[B][N][nu]; asynchronous on the
 * engine's stream, follow with upr_batch_sync. */
int upr_batch_copy_solution_device(upr_batch* h, void* xs_dst, void* us_dst);
/* copy the inputs the last upr_batch_tick evaluated, u[B][nu] (the u_0 of every instance: what the closed loop's exchange
 * step gathers), from the engine's device buffer into a caller-owned DEVICE buffer; asynchronous on the engine's
 * stream.  Fails before the first tick. */
int upr_batch_copy_policy_device(upr_batch* h, void* u_dst);
/* the engine's HIP stream (a hipStream_t): for callers that order their own streams against it with events instead of
 * upr_batch_sync -- the RCCL exchange step of bench.py makes the collective's stream wait for the copy-out, no host sync */
void* upr_batch_stream(upr_batch* h);

/* debug / test accessors: per-phase cycle counters of the production QP kernel (first call arms it,
 * later calls read and clear prof[B][4][16]: 16 phases as seen by lane 0 of each of the first four waves); per-knot linearisation records lin[B][N+1][*stride] */
int upr_batch_qp_profile(upr_batch* h, double* out);
int upr_batch_get_lin(upr_batch* h, double* lin, int* stride);

/* upr_batch_reset without target change and without host synchronisation */
int upr_batch_reset_async(upr_batch* h);

#ifdef __cplusplus
}
#endif
#endif
