"""Tracked value function on the MI355X (upr_batch_track_value_function: the advance hands its own last QP to upr_value_kernel
in-stream), the equality multipliers on the device (BatchMPC.equality_lagrangian), the value function with dynamic obstacles, and
ControllerInterface's three solver-level queries on all eleven golden configs.  The kernel SOURCE of the multiplier paths is checked
without a GPU by tests/test_value_function_tracked.py."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from test_gpu_configs import GOLD, _cfg, _level_tool
from test_value_function_batched import host_cost_to_go, numpy_query, rel_err
from upright_amd import control
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, stationary_guess, waypoints_for

pytestmark = pytest.mark.gpu

TOL_SUMS = 1e-12   # tests/test_gpu_value_function.py: rounding of the sums behind pk and J


# ---- shapes: (handle, observation time, observation, guess) twice over, identical ------------------------------------------------------
def _headline(arrangements, B=3, **settings):
    P = thing_problem(arrangements["pink_bottle"], **settings)
    x0 = level_tray_states(B, seed=3)
    return BatchMPC(P, B, way_p=waypoints_for(P, x0)), np.linspace(0.0, 0.5, B), x0


def _thing_demo(arrangements):
    m = control.ControllerManager.from_config(_cfg("thing_demo"))
    assert m.mpc.problem.slacks and m.mpc.problem.nf == 1
    return m.mpc._mpc, np.zeros(1), np.array(m.settings.initial_state)[None]


def _robust(arrangements=None):
    rng = np.random.default_rng(7)
    B = 2
    bp = np.zeros((B, 8, 10))
    for b in range(B):
        for i in range(8):
            com = rng.uniform([-0.06, -0.06, -0.15], [0.06, 0.06, 0.15])
            bp[b, i] = [1.0, *com, 0.009375, 0, 0, 0.009375, 0, 0.00375]
    cfg = _cfg("robust_sim", **{"mpc.time_horizon": 2.0})
    x0 = np.tile(np.array(control.ControllerSettings(cfg).initial_state), (B, 1))
    x0[:, :2] += rng.uniform(-0.2, 0.2, (B, 2))
    bm = control.BatchControllerManager.from_config(cfg, x0, body_params=bp)
    assert (bm.problem.nb, bm.problem.N) == (8, 20)
    return bm.mpc, np.zeros(B), x0


def _sudden(arrangements=None):
    """sudden_t1.0 as tests/test_gpu_configs.py sets it up (level tray: the frictionless hard rows are feasible at the first knot)."""
    cfg = _cfg("sudden_t1.0")
    x0 = np.array(control.ControllerSettings(cfg).initial_state)
    m = control.ControllerManager.from_config(cfg, x0=x0)
    _level_tool(m.mpc.problem.chain, x0[:9])
    m.mpc._mpc.close(); m.mpc._mpc = None
    m.mpc.reset(m.ref)
    assert m.mpc.problem.n_dyn == 1 and len(m.mpc.problem.pair_a) == 21
    return m.mpc._mpc, np.zeros(1), x0[None]


def _projectile():
    """The ball thrown across the tray's path of tests/test_gpu_configs.py::test_config5_projectile_from_reference_yaml, path row on."""
    cfg = _cfg("projectile_head_on")
    cfg["waypoints"][0]["position"] = [0.0, -1.2, 0.0]
    m = control.ControllerManager.from_config(cfg)
    P = m.mpc.problem
    x0 = np.array(m.settings.initial_state)
    _level_tool(P.chain, x0[:9])
    p0, _ = P.chain.forward(x0[:9])
    T = 1.0
    v0 = np.array([2.5, 0.0, 0.5 * 9.81 * T]); a0 = np.array([0.0, 0.0, -9.81])
    cross = p0 + np.array([0.0, -0.6, 0.45])
    x0[27:] = np.concatenate([cross - v0 * T - 0.5 * a0 * T * T, v0, a0])
    ref = control.TargetTrajectories([0.0], [np.concatenate([p0 + [0.0, -1.2, 0.0], [0, 0, 0, 1], [1.0]])], [np.zeros(P.nu)])
    m.mpc._mpc.close(); m.mpc._mpc = None
    m.update(ref)
    assert P.n_dyn == 1 and len(P.proj_sph) == 1
    return m.mpc._mpc, np.zeros(1), x0[None]


def _assert_nu_is_the_qps(mpc, t0, nu_qp):
    """nu(t) of the device at the knot times of instance 0 against the multipliers qp_kkt() exported for the same QP, nu_qp[N][ne]: an
    independent source (downloaded by another path), so a wrong stride of the kernel's copy or a wrong plan time cannot pass.  Knot 0
    is exact (s = 0).  At knot k the segment coordinate (t0 + k dt - t0) / dt is k to within 2 eps k, so the interpolation mixes in
    at most 2 eps N |nu_k - nu_k+-1| <= 1e-14 max|nu| of a neighbour: bound 1e-13 max|nu|."""
    P = mpc.problem
    got = mpc.equality_lagrangian(t0[0] + P.dt * np.arange(P.N), 0)
    assert got.shape == nu_qp.shape and np.abs(nu_qp).max() > 0
    assert np.array_equal(got[0], nu_qp[0])
    assert np.abs(got - nu_qp).max() <= 1e-13 * np.abs(nu_qp).max(), np.abs(got - nu_qp).max()


def _everything(mpc, t0):
    """Pk, pk, J, X of the handle's cost-to-go and nu(t) at knot times, between them, before the plan and past the horizon."""
    out = mpc.cost_to_go()
    P = mpc.problem
    rel = np.concatenate([P.dt * np.arange(P.N + 1), [-0.2, 0.033, 0.95 * P.dt * P.N, P.dt * P.N + 0.4]])
    inst = np.repeat(np.arange(mpc.B), len(rel))
    out["nu"] = mpc.equality_lagrangian(np.asarray(t0)[inst] + np.tile(rel, mpc.B), inst)
    return out


# ---- tracked equals the explicit update, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,iters", [("headline", 1), ("headline", 2), ("thing_demo", 1), ("robust", 1), ("sudden", 1)])
def test_tracked_equals_the_explicit_update_bitwise(arrangements, shape, iters):
    """Twin handles, same observation, same set_guess(stationary_guess).  R: (iters - 1 SQP iterations, then) value_function_update(...);
    T: track_value_function() and ONE advance of `iters` SQP iterations.  The QP T's advance ran last is the QP R's update solves --
    same linearisation point, same records -- so Pk, pk, J, X and nu are equal with ==: the kernels are deterministic and the
    dispatch order only permutes workgroups.  Shapes: headline (B = 3), thing_demo from the golden config (SOFT, nf = 1), the
    robust shape at N = 20 (93.9 KiB of LDS: the attribute path of the value kernel), sudden_t1.0 (state rows, a dynamic obstacle)."""
    make = dict(headline=_headline, thing_demo=_thing_demo, robust=_robust, sudden=_sudden)[shape]
    (R, t0, x0), (T, _, _) = make(arrangements), make(arrangements)
    xs0, us0 = stationary_guess(x0, R.N, R.nu)
    for h in (R, T):
        h.set_observation(t0, x0)
        h.set_guess(xs0, us0)
    # (T first: where the working set is above 64 KiB, the tracked launch must not lean on an attribute the update set)
    T.track_value_function()
    T.set_sqp_iterations(iters)
    T.advance()
    if iters > 1:
        R.set_sqp_iterations(iters - 1)
        R.advance()
    R.value_function_update(interface_states=True)
    r, t = _everything(R, t0), _everything(T, t0)
    for key in ("Pk", "pk", "J", "X", "nu"):
        assert np.all(np.isfinite(r[key])), key
        assert np.array_equal(r[key], t[key]), (key, float(np.abs(r[key] - t[key]).max()))
    assert np.abs(r["nu"]).max() > 0
    # with a line-search step below one the plan T stores differs from the expansion point X (ocs2's semantics); with a full step it is X
    alpha = T.stats()["step_alpha_last"]
    Xplan = T.solution()[1][:, :, :R.nx]
    for b in range(T.B):
        assert (alpha[b] < 1.0) or np.abs(Xplan[b] - t["X"][b]).max() < 1e-12
    R.close(); T.close()


def test_tracking_changes_nothing_else(arrangements):
    """Twin handles on the headline shape, tracking on and off: after a cold advance and a warm one, solution(), stats() and
    feedback_gains() are bitwise equal."""
    (A, t0, x0), (Bh, _, _) = _headline(arrangements, use_feedback_policy=True), _headline(arrangements, use_feedback_policy=True)
    A.track_value_function()
    for dt in (0.0, 0.1):
        for h in (A, Bh):
            h.set_observation(t0 + dt, x0)
            h.advance()
        assert all(np.array_equal(u, v) for u, v in zip(A.solution(), Bh.solution()))
        sa, sb = A.stats(), Bh.stats()
        assert all(np.array_equal(sa[k], sb[k]) for k in sa)
        assert np.array_equal(A.feedback_gains(), Bh.feedback_gains())
    with pytest.raises(RuntimeError, match="no upr_batch_value_function_update"):
        Bh.cost_to_go()
    assert np.all(np.isfinite(A.cost_to_go()["Pk"]))
    A.close(); Bh.close()


def _closed_loop(T, S, t0, x0):
    """Seven tick()s on the tracking handle T against set_observation + advance on its tracking twin S: cost_to_go() and
    equality_lagrangian() bitwise equal after every period, the later periods replayed from T's captured graph."""
    T.track_value_function(); S.track_value_function()
    x = x0.copy()
    for k in range(7):
        t = t0 + 0.01 * k
        xo, uo = T.tick(t, x)
        S.set_observation(t, x)
        S.advance()
        a, b = _everything(T, t), _everything(S, t)
        for key in a:
            assert np.all(np.isfinite(a[key])) and np.array_equal(a[key], b[key]), (k, key)
        x = xo
    assert T.tick_graph_replays() >= 1
    return x, a


def test_closed_loop_ticks_track_like_advances(arrangements):
    """Seven tick()s on a tracking handle (headline, B = 3, feedback policy on) against set_observation + advance on a tracking twin:
    after every period cost_to_go() and equality_lagrangian() are bitwise equal, the later periods come out of the captured graph
    (one more kernel node, one more copy node); and the validity rule of a tracked cost-to-go."""
    (T, t0, x0), (S, _, _) = _headline(arrangements, use_feedback_policy=True), _headline(arrangements, use_feedback_policy=True)
    assert T.problem.use_feedback_policy
    x, a = _closed_loop(T, S, t0, x0)
    # a tracked cost-to-go belongs to the solve: still there after the next observation ...
    T.set_observation(t0 + 0.07, x)
    V, g = T.value_function(t0 + 0.07, x)
    assert np.all(np.isfinite(V)) and g.shape == (3, T.nx)
    assert np.array_equal(T.cost_to_go()["Pk"], a["Pk"])
    # ... stale after a reset, and after tracking is switched off
    T.reset()
    with pytest.raises(RuntimeError, match="stale"):
        T.cost_to_go()
    S.track_value_function(False)
    for call in (S.cost_to_go, lambda: S.equality_lagrangian(0.0)):
        with pytest.raises(RuntimeError, match="stale"):
            call()
    S.set_observation(t0 + 0.07, x)
    S.advance()                       # an untracked advance brings nothing back
    with pytest.raises(RuntimeError, match="stale"):
        S.cost_to_go()
    T.close(); S.close()


def _robust_in_a_fresh_process():
    """Run by the test below in a process of its own.  The dynamic-LDS limit of upr_value_kernel is an attribute of the function for
    the whole process, and in the suite's process an earlier update has long raised it: here the FIRST launch above 64 KiB (the robust
    shape, 93.9 KiB) is the tracked one, inside an advance; then the explicit update on the twin (bitwise equal), then ticks replayed
    from a captured graph against advances on fresh twins."""
    (R, t0, x0), (T, _, _) = _robust(), _robust()
    xs0, us0 = stationary_guess(x0, R.N, R.nu)
    for h in (R, T):
        h.set_observation(t0, x0)
        h.set_guess(xs0, us0)
    T.track_value_function()
    T.set_sqp_iterations(1)
    T.advance()
    R.value_function_update()
    r, t = _everything(R, t0), _everything(T, t0)
    for key in r:
        assert np.all(np.isfinite(t[key])) and np.array_equal(r[key], t[key]), key
    R.close(); T.close()
    (T, t0, x0), (S, _, _) = _robust(), _robust()
    _closed_loop(T, S, t0, x0)
    T.close(); S.close()
    print("robust tracked first: ok")


def test_tracked_launch_above_64k_first_in_its_process():
    """The attribute path of tracked mode on the robust shape (_robust_in_a_fresh_process above), where no earlier update can have set
    the limit: one child process, which is what this test is about."""
    here = Path(__file__).resolve().parent
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(here), str(here.parent)] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])))
    out = subprocess.run([sys.executable, "-c", "import test_gpu_value_function_tracked as m; m._robust_in_a_fresh_process()"],
                         cwd=str(here), env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "robust tracked first: ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])


# ---- tracking off: the headline computes what the parent commit computed ---------------------------------------------------------------
def test_headline_dump_outputs_equal_the_parents():
    """bench.py --dump-outputs of the headline (tracking off, as bench.py runs it) against the sha256 of every array the PARENT commit
    dumped with the same arguments on the MI355X (tests/golden/value_function_tracked_parent.json): with tracking off every enqueue
    sequence is the parent's, so every output is bit-identical.  (The twin test above compares tracking on against off; a change that
    hit both alike is seen here.)  A later change that alters the headline's outputs on purpose records new hashes in that file."""
    gold = json.load(open(Path(__file__).resolve().parent / "golden" / "value_function_tracked_parent.json"))["dump_outputs"]
    root = Path(__file__).resolve().parents[1]
    with tempfile.TemporaryDirectory() as td:
        out = subprocess.run([sys.executable, str(root / "bench.py"), *gold["args"], "--dump-outputs", td], cwd=str(root), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
        got = {f.name: hashlib.sha256(f.read_bytes()).hexdigest() for f in sorted(Path(td).glob("*.npy"))}
    assert sorted(got) == sorted(gold["sha256"]), (sorted(got), sorted(gold["sha256"]))
    diff = [k for k in got if got[k] != gold["sha256"][k]]
    assert not diff, diff


# ---- dynamic obstacles against the host module ----------------------------------------------------------------------------------------
# Measured on the device (Pk against the host module, relative to the largest entry of the knot's matrix, worst knot; the kernel's
# reductions run over 256 lanes, the host's in numpy): bound = 3x, the rule of tests/test_gpu_value_function.py::MEASURED_PK
# (sudden_t1.0 from the golden start: the base - chair1 row is in the way of the plan, its QP stops at the iteration cap as in
# tests/test_gpu_configs.py; projectile_head_on with the ball of that file's test thrown across the tray's path, QP status 0.  Zero
# weights on the obstacle's rows move Pk by 6.8e-1 and 1.0: the golden obstacle states have teeth as they are.)
MEASURED_PK_DYN = {"sudden_t1.0": 1.88e-13, "projectile_head_on": 9.54e-11}


def _dyn_rows(P):
    """Slots (within a knot's inequality rows) of the rows that involve the dynamic obstacle: its collision pairs and the projectile rows."""
    dyn_sph = set(np.nonzero(np.asarray(P.sph_frame) <= -2)[0].tolist())
    rows = [r for r in range(len(P.pair_a)) if int(P.pair_a[r]) in dyn_sph or int(P.pair_b[r]) in dyn_sph]
    rows += [len(P.pair_a) + i for i in range(len(P.proj_sph))]
    base = 2 * P.nx + 2 * P.nu + (5 * P.nc if P.nf == 3 else 0)
    return [base + r for r in rows]


@pytest.mark.parametrize("name", ["sudden_t1.0", "projectile_head_on"])
def test_dynamic_obstacle_cost_to_go_against_the_host_module(name):
    """value_function_update(interface_states=True) + cost_to_go() with a dynamic obstacle against the host module on the same primal-dual point (one more
    qp_kkt on the handle, as tests/test_gpu_value_function.py::_compare): pk, J to the rounding of their sums, X exact, Pk to 3x the
    measured disagreement.  Teeth: on the host module alone, zero weights on the obstacle's rows move Pk at some knot by more than
    100x that bound -- the rows of the obstacle are in the cost-to-go, read out of the records the linearisation writes.  Interface
    convention: dV/dx has the interface width, a zero obstacle block, and its robot block is numpy's on the downloaded arrays."""
    mpc, t0, x0 = _sudden() if name == "sudden_t1.0" else _projectile()
    P = mpc.problem
    mpc.set_observation(t0, x0)
    mpc.set_sqp_iterations(3)
    mpc.advance()
    with pytest.raises(RuntimeError, match="not available with a dynamic obstacle"):
        mpc.value_function_update()                      # (the robot-state entry keeps refusing such a handle)
    mpc.value_function_update(interface_states=True)
    dev = mpc.cost_to_go()
    assert dev["Pk"].shape == (1, P.N + 1, P.nx, P.nx) and dev["X"].shape == (1, P.N + 1, P.nx)   # robot-block shapes
    with mpc.preserved_stats():
        sol = {k: v[0] for k, v in mpc.qp_kkt().items()}
    assert sol["dx"].shape == (P.N + 1, P.nx_full) and not sol["dx"][:, P.nx:].any() and sol["pi"].shape == (P.N + 1, P.nx)
    sol["dx"] = sol["dx"][:, :P.nx]
    _assert_nu_is_the_qps(mpc, t0, sol["nu"])
    lin = mpc.lin_records()[0]
    _, xs, us = mpc.solution()
    Df = mpc.eq_input_jacobian(0)[:, P.nq:]
    host = host_cost_to_go(P, xs[0][:, :P.nx], us[0], lin, sol, Df, None)
    worst = {key: rel_err(dev[key][0], host[key]) for key in ("Pk", "pk", "J", "X")}
    zeroed = dict(sol, lam=sol["lam"].copy())
    zeroed["lam"][:, _dyn_rows(P)] = 0.0
    moved = rel_err(host_cost_to_go(P, xs[0][:, :P.nx], us[0], lin, zeroed, Df, None)["Pk"], host["Pk"])
    print("device cost-to-go vs host module, %s: " % name + "  ".join("%s %.2e" % kv for kv in worst.items())
          + "  | zero weights on the obstacle's rows move Pk by %.2e  (QP status %d)" % (moved, int(mpc.stats()["qp_status_last"][0])))
    assert all(np.all(np.isfinite(v)) for v in dev.values())
    tol_pk = 3.0 * MEASURED_PK_DYN[name]
    assert MEASURED_PK_DYN[name] <= 1e-4   # (the emulation's worst case on any shape is 9.6e-5: more would be a defect, not a bound)
    assert worst["Pk"] <= tol_pk, (worst["Pk"], tol_pk)
    assert worst["pk"] <= TOL_SUMS and worst["J"] <= TOL_SUMS and worst["X"] == 0.0, worst
    assert moved > 100.0 * tol_pk, (moved, tol_pk)
    # the interface convention of the query
    rng = np.random.default_rng(5)
    n = 12
    t = t0[0] + rng.uniform(-0.1, P.N * P.dt + 0.1, n)
    k = np.clip(((t - t0[0]) / P.dt).astype(int), 0, P.N)
    x = np.zeros((n, P.nx_full))
    x[:, :P.nx] = dev["X"][0, k] + rng.normal(size=(n, P.nx)) * 1e-2
    x[:, P.nx:] = rng.normal(size=(n, P.nx_full - P.nx))
    V, g = mpc.value_function(t, x, np.zeros(n, dtype=np.int32))
    Vn, Gn = numpy_query(P, dev, t0, np.zeros(n, dtype=int), t, x[:, :P.nx])
    assert g.shape == (n, P.nx_full) and not g[:, P.nx:].any()
    assert (np.abs(V - Vn) / np.abs(Vn)).max() < 1e-12
    assert (np.abs(g[:, :P.nx] - Gn).max(axis=1) / np.abs(Gn).max(axis=1)).max() < 1e-12
    mpc.close()


# ---- ControllerInterface on every golden config ------------------------------------------------------------------------------------------
DEVICE_PATH = ("thing_demo", "robust_sim", "projectile_head_on", "sudden_t1.0")   # the four the host path refused
MEASURED_PK_THING_DEMO = 4.87e-09   # tests/test_gpu_value_function.py::MEASURED_PK["thing_demo"]


@pytest.mark.parametrize("name", list(GOLD))
def test_controller_interface_queries_on_every_golden_config(name):
    """reset + setObservation + advanceMpc (ControllerManager.from_config / warmstart), then valueFunction,
    valueFunctionStateDerivative and stateInputEqualityConstraintLagrangian: finite, of the right shapes.  On the four configs that go
    to the device path (HPIPM slacks on inequality rows, or a dynamic obstacle) they are the handle's own value_function /
    equality_lagrangian at the same (t, x); on thing_demo the gradient also agrees with the host module's, with the slack pairs, to
    what the Pk bound of that shape allows: |dPk| |x - X|_1 with |dPk| <= 3 x 4.87e-9 max|Pk| at the two knots, plus the rounding of pk."""
    assert len(GOLD) == 11
    m = control.ControllerManager.from_config(_cfg(name))
    m.warmstart()
    ci = m.mpc
    P = ci.problem
    x = np.array(m.settings.initial_state)
    x[:P.nq] += np.random.default_rng(1).uniform(-1e-2, 1e-2, P.nq)
    u = np.zeros(P.nu)
    for t in (0.0, 0.13):
        V = ci.valueFunction(t, x)
        g = ci.valueFunctionStateDerivative(t, x)
        nu = ci.stateInputEqualityConstraintLagrangian(t, x, u)
        assert isinstance(V, float) and np.isfinite(V)
        assert g.shape == (P.nx_full,) and np.all(np.isfinite(g)) and nu.shape == (6 * P.nb,) and np.all(np.isfinite(nu))
        assert ci._on_device() == (name in DEVICE_PATH)
        if name in DEVICE_PATH:
            Vh, gh = ci._mpc.value_function(t, x, 0)
            assert V == Vh[0] and np.array_equal(g, gh[0]) and np.array_equal(nu, ci._mpc.equality_lagrangian(np.array([t]), 0)[0])
            assert not g[P.nx:].any()
    if name == "thing_demo":
        mpc = ci._mpc
        dev = mpc.cost_to_go()
        with mpc.preserved_stats():
            sol = {k: v[0] for k, v in mpc.qp_kkt().items()}
        pairs = tuple(a[0] for a in mpc.qp_slack_pairs())
        _assert_nu_is_the_qps(mpc, np.zeros(1), sol["nu"])
        _, xs, us = mpc.solution()
        host = host_cost_to_go(P, xs[0], us[0], mpc.lin_records()[0], sol, mpc.eq_input_jacobian(0)[:, P.nq:], pairs)
        hb = {k: v[None] for k, v in host.items()}
        _, Gn = numpy_query(P, hb, np.zeros(1), [0], [0.13], x[None, :P.nx])
        j = 1
        bound = sum(3.0 * MEASURED_PK_THING_DEMO * np.abs(host["Pk"][k]).max() * np.abs(x[:P.nx] - host["X"][k]).sum() for k in (j, j + 1)) \
            + TOL_SUMS * np.abs(Gn).max()
        err = np.abs(g[:P.nx] - Gn[0]).max()
        print("thing_demo: gradient through ControllerInterface vs host module with slack pairs: %.2e (bound %.2e, largest component %.2e)" % (err, bound, np.abs(Gn).max()))
        assert err <= bound, (err, bound)
        assert np.array_equal(dev["X"][0], host["X"])
    ci._mpc.close()
