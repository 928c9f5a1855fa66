"""The replay of a time law on a clock (upright_amd/csrc/upr_replay.h) through its host emulation (tests/emu/upr_replay_emu.cpp): the
sampler's body per plan, the state point, the jobs in both forms and the reduction, in the plain and the -mfma -ffp-contract=fast build,
against numpy's knot times, segment search and quintic Hermite, the closed form of a sliding translation and the CPU reference at the
joint-space sample states (tests/replay_ref.py); the assertions tests/test_gpu_replay.py repeats on the device's answers.

Observed on the emulation (x86-64): slide at 1.1185, tick 0.01, K = 179: knot margins >= 1.5e-3 mu0 g0, sample margins 1.15e-5 from the
bound, rejected 37 38 39 140 141 142 (segments 4 and 15), the retiming's duration finite; slide laws at tick 0.037 (min |margin|,
rejected): ramp 1.2e-3, 21; zigzag 3.2e-2, 17; uniform 1.25 2.5e-3, 19; generic plans, tick 0.05: own laws (scenario 0's) K = 37, counts 31 37 31,
0 of 198 jobs undecided, 0 rejected under scenario 0 (39 under the other); all levels 4: 0 of 162 undecided, 76 rejected; zigzag: 0 of 258
undecided, 107 rejected; states against numpy at the scale max(1, |x|_inf): q 2.8e-16, qdot 3.5e-15, qddot 2.4e-13 (plain), the FMA twin
against the plain build 8.5e-16, 6.1e-15, 3.2e-13; the device function against dep / arr 1.2e-16, 1.1e-15, 2.2e-14, the Hermite against
the cubic of a rolled-out plan 1.6e-16, 3.5e-15, 9.3e-14; foam_die2: 0 of 172 undecided, 31 rejected."""
import time

import numpy as np
import pytest

import balance_ref as R
import replay_ref as V
import retime_ref as Q

_SLOWEST = [0.0, ""]


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.time()
    yield
    dt = time.time() - t0
    if dt > _SLOWEST[0]:
        _SLOWEST[:] = [dt, request.node.name]
    print("replay (emulation): %s took %.1f s; the slowest so far: %s, %.1f s" % (request.node.name, dt, _SLOWEST[1], _SLOWEST[0]))


def run(P, xs, params, speeds, level, tick, **kw):
    return V.run_emu(P, xs, params, speeds, level, tick, **kw)


def _retime(P, xs, params, speeds):
    return Q.run_emu(P, xs, params, speeds, boxes=False)["duration"]


def test_between_the_knots(arrangements):
    """1. the slide replayed uniformly at 1.1185: every knot keeps 1e-6 mu0 g0 on the closed form (the retiming returns a finite
    duration), every sample of the 10 ms clock lies 1e-6 mu0 g0 from the bound, the closed form rejects some of them -- and the call's
    rejected set is the closed form's, between knots 4-5 and 15-16; verdict and worst are consistent with it.  Both forms."""
    assert V.body_between_knots(run, arrangements, retime=_retime) == [37, 38, 39, 140, 141, 142]
    V.body_between_knots(lambda *a, **k: run(*a, **dict(k, form=0)), arrangements)


def test_slide_laws_with_path_acceleration(arrangements):
    """2. the ramp 1 2 3 4 5 .. 5 4 3 2 1, the zigzag 1 .. 5 .. 1 .. 5 and uniform 1.25 on SLIDE_SPEEDS at tick 0.037: the decisions are
    the closed form's, whose margins keep 1e-6 mu0 g0."""
    V.body_slide_laws(run, arrangements)
    V.body_slide_laws(lambda *a, **k: run(*a, **dict(k, form=0)), arrangements)


def test_device_function_meets_the_retimed_states(arrangements):
    """3. upr_rpl_state at t' = 0 and t' = dt_i of every segment equals retimed_states' dep and arr (1e-12, 1e-10, 1e-9 at the scale
    max(1, |x|_inf)); upr_rpl_locate puts a knot time on the departing side."""
    G, laws = V.generic_laws(arrangements)
    P, h, sp = G["P"], float(G["P"].dt), G["speeds"]
    worst = np.zeros(3)
    for name, level in laws[1:]:
        T = V.knot_times(level, sp, h)
        _, dep, arr = Q.retimed_states(G["xs"], level[:, None], sp, h, P.nq)
        for b in range(G["xs"].shape[0]):
            s = sp[level[b]]
            for i in range(P.N):
                x0, _ = V.emu_state(P, G["xs"][b, i], G["xs"][b, i + 1], s[i], s[i + 1], 0.0)
                x1, _ = V.emu_state(P, G["xs"][b, i], G["xs"][b, i + 1], s[i], s[i + 1], T[b, i + 1] - T[b, i])
                worst = np.maximum(worst, V.assert_states(np.stack([x0, x1]), np.stack([dep[b, 0, i], arr[b, 0, i]]), (name, b, i)))
                assert V.emu_locate(T[b], T[b, i]) == (i, 0.0)
            assert V.emu_locate(T[b], T[b, P.N])[0] == P.N - 1 and V.emu_locate(T[b], 0.5 * (T[b, 3] + T[b, 4]))[0] == 3
    print("replay: the device function against dep / arr: %s" % worst)


def test_hermite_is_the_cubic_of_a_rolled_out_plan(arrangements):
    """3. a plan rolled out through the triple integrator from random jerks: between the knots the interpolant equals q_i + tau v_i +
    tau^2 a_i / 2 + tau^3 j_i / 6 and its derivatives, to the same tolerances."""
    P = R.table_problem(arrangements, "pink_bottle")
    nq, N, h = P.nq, P.N, float(P.dt)
    rng = np.random.default_rng(4)
    x = np.zeros((N + 1, 3 * nq))
    x[0] = rng.uniform(-1, 1, 3 * nq)
    jerk = rng.uniform(-20, 20, (N, nq))
    for i in range(N):
        q, v, a, j = x[i, :nq], x[i, nq:2 * nq], x[i, 2 * nq:], jerk[i]
        x[i + 1] = np.concatenate([q + h * v + h * h / 2 * a + h**3 / 6 * j, v + h * a + h * h / 2 * j, a + h * j])
    worst = np.zeros(3)
    for i in range(N):
        for tau in (0.0, 0.013, 0.05, 0.0871, h):
            got, _ = V.emu_state(P, x[i], x[i + 1], 1.0, 1.0, tau)
            q, v, a, j = x[i, :nq], x[i, nq:2 * nq], x[i, 2 * nq:], jerk[i]
            want = np.concatenate([q + tau * v + tau * tau / 2 * a + tau**3 / 6 * j, v + tau * a + tau * tau / 2 * j, a + tau * j])
            worst = np.maximum(worst, V.assert_states(got[None], want[None], (i, tau)))
    print("replay: Hermite against the cubic: %s" % worst)


def test_generic_plans(arrangements):
    """4. retime_ref's generic case (B = 3, two scenarios, M = 5, boxes on), tick 0.05, under each plan's own optimal law (counts differ:
    NaN tails), all levels 4 and the zigzag 0 2 4 2 0 ..: T_N, the knot times and count equal numpy's as doubles, the states within the
    tolerances, at most 10 % undecided samples on the reference alone, numpy's box decisions 1e-9 from their bounds, then the decisions
    on decided samples, box_first, worst and verdict."""
    res = V.body_generic(run, arrangements)
    assert res["top"][2] == 162 and res["zigzag"][2] == 258
    V.body_generic(run, arrangements, form=0)


def test_shapes_and_edges(arrangements):
    """5. K = 1, t0 > 0, t0 at and past T_N, a sample on a knot time, a plan without a law among others, speed 0 at the first knot,
    params None / shared / per instance; foam_die2 with B = 2; the wave form on the one-body shape."""
    V.body_edges(run, arrangements)
    V.body_edges(lambda *a, **k: run(*a, **dict(k, form=0)), arrangements)
    V.body_multi_body(run, arrangements)


def test_fma_twin(arrangements):
    """6. the -mfma -ffp-contract=fast build (how hipcc contracts for the device): count, duration and box_first equal, states within
    the tolerances of check 3, decisions equal on decided samples; the slide's rejected set is the closed form's."""
    if not V.have_fma_twin():
        pytest.skip("the host has no FMA instruction (/proc/cpuinfo): the twin is not built")
    G, laws = V.generic_laws(arrangements)
    for form in (-1, 0):
        for name, level in laws:
            a = run(G["P"], G["xs"], G["params"], G["speeds"], level, 0.05, form=form, fma=True)
            b = run(G["P"], G["xs"], G["params"], G["speeds"], level, 0.05, form=form)
            assert np.array_equal(a["times"], b["times"])
            assert V.agree(a, b, G["P"], G["xs"], G["params"], G["speeds"], level, 0.05) >= 60
            print("replay, FMA twin against the plain build, %s: state errors %s" % (name, V.state_errors(a["x"], b["x"])))
    twin = lambda *a, **k: run(*a, **dict(k, fma=True))   # noqa: E731
    V.body_between_knots(twin, arrangements)
    V.body_slide_laws(twin, arrangements)
    M = V.multi_body_case(arrangements)
    a, b = (run(M["P"], M["xs"], M["params"], M["speeds"], M["level"], 0.05, fma=f) for f in (True, False))
    V.agree(a, b, M["P"], M["xs"], M["params"], M["speeds"], M["level"], 0.05)
