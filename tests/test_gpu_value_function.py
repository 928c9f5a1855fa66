"""The batched value function on the MI355X (upright_amd/csrc/upr_value.h behind BatchMPC.value_function_update / cost_to_go /
value_function): the device's cost-to-go against the host module on the headline batch, on thing_demo (HPIPM slacks, from the
reference's YAML) and on the upright_robust shape; against finite differences of the QP's optimal value, slack penalties included;
the query kernel against numpy; the bookkeeping of the handle; and the launch time against the QP's.  The kernel SOURCE is checked
without a GPU by tests/test_value_function_batched.py."""
import numpy as np
import pytest

from test_gpu_configs import _cfg
from test_value_function_batched import SOFT, host_cost_to_go, numpy_query, query_points, rel_err
from upright_amd import control
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, stationary_guess, waypoints_for
from upright_amd.value_function import qp_objective, qp_slack_penalties

pytestmark = pytest.mark.gpu

# pk (p_0: a sum of some 300 products; the other knots are copies of the costates) and J (some 2000 products per instance): rounding of
# double-precision sums of that length (tests/test_value_function_batched.py, TOL_SUMS); X = xs + dx is one addition
TOL_SUMS = 1e-12


def _host(mpc, insts):
    """The host module's cost-to-go of the QP at the handle's current plan for the given instances (one more QP on the handle: the
    kernels are deterministic, it ends at the primal-dual point the update's QP ended at)."""
    P = mpc.problem
    with mpc.preserved_stats():
        sol = mpc.qp_kkt()
    pairs = mpc.qp_slack_pairs() if P.slacks else None
    lin = mpc.lin_records()
    _, xs, us = mpc.solution()
    out = {}
    for b in insts:
        Df = mpc.eq_input_jacobian(b)[:, P.nq:]
        out[b] = host_cost_to_go(P, xs[b][:, :P.nx], us[b], lin[b], {k: v[b] for k, v in sol.items()}, Df,
                                 tuple(a[b] for a in pairs) if pairs is not None else None)
    return out


def _compare(mpc, insts, name, measured_pk):
    mpc.value_function_update()
    dev = mpc.cost_to_go()
    host = _host(mpc, insts)
    worst = dict(Pk=0.0, pk=0.0, J=0.0, X=0.0)
    for b in insts:
        for key in worst:
            worst[key] = max(worst[key], rel_err(dev[key][b], host[b][key]))
    print("device cost-to-go vs host module, %s: " % name + "  ".join("%s %.2e" % kv for kv in worst.items()) + "  (%.3f ms)" % mpc.value_function_ms())
    assert all(np.all(np.isfinite(v)) for v in dev.values())
    assert np.abs(dev["Pk"] - np.swapaxes(dev["Pk"], 2, 3)).max() == 0.0
    assert worst["Pk"] <= 3.0 * measured_pk, (worst["Pk"], measured_pk)
    assert worst["pk"] <= TOL_SUMS and worst["J"] <= TOL_SUMS and worst["X"] == 0.0, worst
    return dev


# Measured on the device (Pk against the host module, relative to the largest entry of the knot's matrix, worst knot and instance; the
# reductions of the kernel run over 256 lanes, the host's in numpy): bound = 3x
MEASURED_PK = {"headline": 1.13e-05, "thing_demo": 4.87e-09, "robust": 5.33e-10}


def test_headline_batch_against_the_host_module(arrangements):
    """value_function_update() + cost_to_go() on the headline at B = 1024 after one advance: 16 seeded instances against the host
    module, all 1024 finite with symmetric Pk."""
    B = 1024
    P = thing_problem(arrangements["pink_bottle"])
    x0 = level_tray_states(B, seed=3)
    mpc = BatchMPC(P, B, way_p=waypoints_for(P, x0))
    mpc.set_observation(0.0, x0)
    mpc.advance()
    insts = sorted(np.random.default_rng(0).choice(B, 16, replace=False).tolist())
    dev = _compare(mpc, insts, "headline", MEASURED_PK["headline"])
    assert np.all(dev["J"][:, 0] > dev["J"][:, -1]) and np.all(dev["J"][:, -1] == 0.0)
    mpc.close()


def test_thing_demo_against_the_host_module():
    """thing_demo.yaml as the reference merges it (tests/golden/configs.json): frictionless bottle with HPIPM slacks -- the problem
    the host path behind ControllerInterface refuses."""
    m = control.ControllerManager.from_config(_cfg("thing_demo"))
    m.warmstart()
    mpc = m.mpc._mpc
    P = mpc.problem
    assert P.slacks and (P.slacks.get("state_box") or P.slacks.get("input_box") or P.slacks.get("poly_ineq"))
    _compare(mpc, [0], "thing_demo", MEASURED_PK["thing_demo"])
    mpc.close()


def test_robust_shape_against_the_host_module():
    """upright_robust's eight-corner arrangement at N = 20 (softened state boxes and equality, per-instance inertial parameters)."""
    rng = np.random.default_rng(7)
    B = 4
    bp = np.zeros((B, 8, 10))
    for b in range(B):
        sc = (1.0, 0.5, 0.1)[b % 3]
        for i in range(8):
            com = rng.uniform([-0.06, -0.06, -0.15], [0.06, 0.06, 0.15])
            bp[b, i] = [1.0, *com, sc * 0.009375, 0, 0, sc * 0.009375, 0, sc * 0.00375]
    cfg = _cfg("robust_sim", **{"mpc.time_horizon": 2.0})
    x0 = np.tile(np.array(control.ControllerSettings(cfg).initial_state), (B, 1))
    x0[:, :2] += rng.uniform(-0.2, 0.2, (B, 2))
    bm = control.BatchControllerManager.from_config(cfg, x0, body_params=bp)
    bm.warmstart()
    assert "upr_qp3_cfg<9, 8, 32, 1, 20, 256" in bm.mpc.kernel_times()["qp_kernel"]
    _compare(bm.mpc, list(range(B)), "robust", MEASURED_PK["robust"])
    bm.mpc.close()


# ---- finite differences of the QP's optimal value, penalties included ---------------------------------------------------------------
def _fd_disagreement(arrangements, accel, insts, halve=False, **settings):
    """Worst relative disagreement (gradient, curvature) of the device's p_0, P_0 with central finite differences of the QP's optimal
    value (stage costs + slack penalties, evaluated by the host functions on the exported point) over the observed state, for the
    instances `insts` of the soft case of tests/test_emu.py::test_soft_rows_kernel_source with the base acceleration `accel` on instance
    1: the six directions and steps of tests/test_gpu_parity.py::test_value_function_against_finite_differences.  halve: the stencil of
    a direction is halved until the finite differences agree with those of half the stencil (gradient to 1.25e-4, curvature to 0.5 %: a
    quarter of the bounds they are held against) -- a property of the reference alone; the scales used come back too.  Also returns
    the largest slack of each instance."""
    B = 2
    P = thing_problem(arrangements["pink_bottle"], **settings)
    P.slacks = dict(SOFT)
    x0 = level_tray_states(B, seed=11)
    way = waypoints_for(P, x0)
    xs0, us0 = stationary_guess(x0, P.N, P.nu)
    x0[1, 18] = accel
    xs0[1, :, 18] = accel
    mpc = BatchMPC(P, B, way_p=way)
    Df = [mpc.eq_input_jacobian(b)[:, P.nq:] for b in range(B)]

    def solve(x):
        mpc.set_observation(0.0, x)
        mpc.set_guess(xs0, us0)
        sol = mpc.qp_kkt()
        assert np.all(mpc.stats()["qp_status_last"][insts] == 0)
        pairs = mpc.qp_slack_pairs()
        lin = mpc.lin_records()
        V = np.zeros(B)
        for b in insts:
            s = {k: v[b] for k, v in sol.items()}
            X = xs0[b] + s["dx"]; U = us0[b] + s["du"]
            assert np.abs(X[0] - x[b]).max() < 1e-12
            V[b] = (qp_objective(P, xs0[b], lin[b], X, U) + qp_slack_penalties(P, lin[b], s, Df[b], tuple(a[b] for a in pairs))).sum()
        return V, pairs

    V0, pairs = solve(x0)
    sig_max = pairs[0].reshape(B, -1).max(axis=1)
    mpc.set_observation(0.0, x0)
    mpc.set_guess(xs0, us0)
    mpc.value_function_update()
    ctg = mpc.cost_to_go()
    assert np.abs(ctg["J"][insts, 0] - V0[insts]).max() < 1e-10 * np.abs(V0[insts]).max()      # the device's J_0 is that value

    def fd(d, s):   # directional derivative and curvature along d from the stencil s d, per instance
        Vp, _ = solve(x0 + s * d[None])
        Vm, _ = solve(x0 - s * d[None])
        return (Vp - Vm) / (2.0 * s), (Vp + Vm - 2.0 * V0) / (s * s)

    rng = np.random.default_rng(0)
    worst = np.zeros((B, 2))
    scales = []
    for trial in range(6):
        d = np.zeros(P.nx)
        d[:P.nq] = rng.uniform(-1, 1, P.nq) * 2e-4               # joint positions
        d[P.nq:2 * P.nq] = rng.uniform(-1, 1, P.nq) * 1e-3       # joint velocities (as test_value_function_against_finite_differences)
        s = 1.0
        g_fd, h_fd = fd(d, s)
        while halve:
            g2, h2 = fd(d, 0.5 * s)
            if all(abs(g_fd[b] - g2[b]) <= 1.25e-4 * abs(g2[b]) and abs(h_fd[b] - h2[b]) <= 5e-3 * abs(h2[b]) for b in insts):
                break
            s, g_fd, h_fd = 0.5 * s, g2, h2
            assert s >= 1.0 / 64, "the finite differences do not settle"
        scales.append(s)
        for b in insts:
            g_vf, h_vf = float(ctg["pk"][b, 0] @ d), float(d @ ctg["Pk"][b, 0] @ d)
            worst[b, 0] = max(worst[b, 0], abs(g_fd[b] - g_vf) / max(abs(g_fd[b]), 1e-12))
            worst[b, 1] = max(worst[b, 1], abs(h_fd[b] - h_vf) / max(abs(h_fd[b]), 1e-12))
    mpc.close()
    return worst, sig_max, scales


# Instance 1 (active slacks), measured on the device: (gradient, curvature) relative disagreement; bound = 3x.  The base acceleration
# of instance 1: 5.0 (tests/test_emu.py) does not converge at the solver's default tolerances (1e-8; the 1e-7 that test converges
# to leaves 2e-2 of noise on instance 0's gradient: three separately converged QPs); 3.0 is the first violation on the way down whose
# curvature disagreement is below the 10 % cap (3.0: 4.0e-2, max sigma 1.59; 2.5: 2.5e-2; 2.0: 9.2e-3, max sigma 0.44).
FD_ACCEL = 3.0
MEASURED_FD_ACTIVE = (4.32e-06, 3.98e-02)


def test_cost_to_go_against_finite_differences_with_softened_rows(arrangements):
    """The method of tests/test_gpu_parity.py::test_value_function_against_finite_differences on the soft case: instance 0 keeps that
    test's bounds (5e-4 on the gradient, 2 % on the curvature); instance 1, whose slacks are active (sigma > 1e-3), 3x the measured
    disagreement, which must stay below 10 % on the curvature to be evidence at all.

    What the finite differences need on instance 0 to be a reference at those bounds.  With that test's stencil and the solver's default
    tolerance they are not: 4.4e-3 and 1.7e-1 against the cost-to-go -- and 5.2e-3 and 1.7e-1 for the same instance with HARD rows, the
    path that test checks on another seed.  Two errors of the reference itself, both measured without the cost-to-go: (a) three
    separately converged QPs at 1e-8 leave the value uncertain by some 1e-9, which is 1 % of a second difference of 1e-6 and grows
    fourfold with every halving of the stencil: instance 0 is converged to 1e-11 here (15 iterations; instance 1 of the same batch
    does not get there and is not read in that pass); (b) in three of the six directions the full stencil reaches across a change of
    the active set, where the value is only piecewise quadratic -- halving it moves the second difference by 0.9 %, 7 % and 11 %: a
    direction's stencil is halved until the differences agree with those of half the stencil to a quarter of the bounds (it ends at
    1, 1, 1/2, 1/2, 1/4, 1).  Then, measured on the device: gradient 5.8e-6, curvature 1.4e-3 at worst.
    Instance 1 keeps the full stencil and the default tolerance (it converges no further, and its noise forbids a smaller stencil)."""
    w0, sig0, scales = _fd_disagreement(arrangements, FD_ACCEL, [0], halve=True, qp_tol=1e-11, qp_iter_max=40)
    w1, sig1, _ = _fd_disagreement(arrangements, FD_ACCEL, [1], qp_iter_max=40)
    print("cost-to-go vs finite differences: instance 0 gradient %.1e curvature %.1e (stencil scales %s); instance 1 gradient %.1e curvature %.1e (max sigma %.2e, %.2e)"
          % (w0[0, 0], w0[0, 1], scales, w1[1, 0], w1[1, 1], sig0[0], sig1[1]))
    assert sig1[1] > 1e-3
    assert w0[0, 0] < 5e-4 and w0[0, 1] < 0.02, w0[0]
    assert w1[1, 1] < 0.10, w1[1]
    assert w1[1, 0] <= 3.0 * MEASURED_FD_ACTIVE[0] and w1[1, 1] <= 3.0 * MEASURED_FD_ACTIVE[1], w1[1]


# ---- query kernel, bookkeeping, timing --------------------------------------------------------------------------------------------------
def _headline(arrangements, B, seed=3):
    P = thing_problem(arrangements["pink_bottle"])
    x0 = level_tray_states(B, seed=seed)
    mpc = BatchMPC(P, B, way_p=waypoints_for(P, x0))
    t0 = np.linspace(0.0, 1.0, B)
    mpc.set_observation(t0, x0)
    mpc.advance()
    return P, mpc, t0, x0


def test_query_kernel_against_numpy(arrangements):
    """value_function(t, x, inst) at 256 points spread over instances and times (knot times, between them, before the first knot and
    behind the last) against numpy on the downloaded Pk, pk, J, X: 1e-12 relative (V: to |V|; dV/dx: to the largest component)."""
    P, mpc, t0, _ = _headline(arrangements, 32)
    mpc.value_function_update()
    ctg = mpc.cost_to_go()
    inst, t, x = query_points(P, ctg, t0, 256, 1)
    V, G = mpc.value_function(t, x, inst)
    Vn, Gn = numpy_query(P, ctg, t0, inst, t, x)
    assert (t < t0[inst]).any() and (t > t0[inst] + P.N * P.dt).any() and len(set(inst.tolist())) > 16
    assert (np.abs(V - Vn) / np.abs(Vn)).max() < 1e-12
    assert (np.abs(G - Gn).max(axis=1) / np.abs(Gn).max(axis=1)).max() < 1e-12
    # at the plan's own first expansion point: the cost-to-go of the plan and the gradient p_0
    V, G = mpc.value_function(t0, ctg["X"][:, 0])
    assert np.array_equal(V, ctg["J"][:, 0]) and np.array_equal(G, ctg["pk"][:, 0])
    mpc.close()


def test_bookkeeping_of_the_handle(arrangements):
    """An update leaves statistics and dispatch keys as the advance left them (the next advance is bit-identical to one without the
    update in between); two updates on the same plan give bit-identical Pk; queries fail before the first update and, with "stale",
    once the plan or the observation changed; a problem with dynamic obstacles is refused."""
    P, mpc, t0, x0 = _headline(arrangements, 64)
    with pytest.raises(RuntimeError, match="no upr_batch_value_function_update"):
        mpc.value_function(0.0, x0)
    before = {k: v.copy() for k, v in mpc.stats().items()}
    mpc.value_function_update()
    a = mpc.cost_to_go()
    after = mpc.stats()
    assert all(np.array_equal(before[k], after[k]) for k in before), [k for k in before if not np.array_equal(before[k], after[k])]
    mpc.value_function_update()
    b = mpc.cost_to_go()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # dispatch keys: the advance that follows equals the one of a twin handle that never ran an update
    twin = BatchMPC(P, 64, way_p=mpc.way_p)
    twin.set_observation(t0, x0); twin.advance()
    for h in (mpc, twin):
        h.set_observation(t0 + 0.1, x0); h.advance()
    assert all(np.array_equal(u, v) for u, v in zip(mpc.solution(), twin.solution()))
    assert all(np.array_equal(u, v) for u, v in zip(mpc.stats().values(), twin.stats().values()))
    twin.close()
    # stale after the advance (and after set_observation / set_guess / reset)
    for call in (lambda: mpc.value_function(0.0, x0), mpc.cost_to_go):
        with pytest.raises(RuntimeError, match="stale"):
            call()
    mpc.value_function_update()
    mpc.value_function(0.0, x0)
    for i, change in enumerate((lambda: mpc.set_observation(t0, x0), lambda: mpc.set_guess(*mpc.solution()[1:]), mpc.reset)):
        change()
        with pytest.raises(RuntimeError, match="stale"):
            mpc.value_function(0.0, x0)
        if i < 2:
            mpc.value_function_update()
    mpc.close()
    # dynamic obstacles: refused with upr_batch_qp_kkt's message
    m = control.ControllerManager.from_config(_cfg("projectile_head_on"))
    m.warmstart()
    with pytest.raises(RuntimeError, match="not available with a dynamic obstacle"):
        m.mpc._mpc.value_function_update()
    m.mpc._mpc.close()


def test_cost_to_go_launch_is_shorter_than_the_qp_launch(arrangements):
    """Timing sanity on the headline at B = 1024: one backward sweep with nq-square pivots is less work than one interior-point
    iteration, of which a QP launch runs about ten -- value_function_ms() (HIP events around the cost-to-go launch) below the QP
    launch time of the same handle (kernel_times() after an advance with enable_timing(1)).  Measured: 0.595 ms (median of five
    launches, the first 0.611) against 2.37 ms per QP launch of the advance after a changed observation (1.89 ms in a steady loop:
    DESIGN.md section 3.6)."""
    P, mpc, _, x0 = _headline(arrangements, 1024)
    mpc.enable_timing(1)
    mpc.set_observation(0.1, x0)
    mpc.advance()
    qp_ms = float(mpc.kernel_times()["qp_ms"])
    mpc.enable_timing(0)
    ms = []
    for _ in range(5):
        mpc.value_function_update()
        ms.append(mpc.value_function_ms())
    print("cost-to-go launch %.3f ms (median of 5, first %.3f) against %.3f ms per QP launch" % (float(np.median(ms)), ms[0], qp_ms))
    assert 0.0 < float(np.median(ms)) < qp_ms
    mpc.close()
