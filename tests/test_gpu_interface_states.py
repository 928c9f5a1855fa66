"""Interface states [robot x (nx) | r v a of every dynamic obstacle (9 n_dyn)] through every entry of the C-ABI that takes or returns
them, at B = 2 with one obstacle (nxf = 36) and with two (nxf = 45): where a hard-coded 9, a wrong row stride or the wrong one of the
two stored observations shows.  R = [:nx] is the robot block of a state, O = [nx:] its obstacle block.  What an entry does with O:
  solution                    the ballistic continuation of the LAST observation by k dt
  evaluate (with x_obs too)   ... of the observation the stored solution belongs to by max(t - t0, 0)
  tick                        as observed
  set_guess, evaluate's x_obs, value_function's x: ignored
  qp_step, qp_kkt dx, feedback_gains, value_function's gradient: exactly zero
  linearize_points, state_rows: the obstacle of every point as given
and the refusals of these entries, word for word.  One handle per case; every check brings the handle into the state it needs and
returns the arrays it obtained."""
import ctypes as C

import numpy as np
import pytest

from test_interface_states import assert_ballistic
from upright_amd import _capi
from upright_amd._capi import check, iptr, ptr
from upright_amd.engine import BatchMPC

pytestmark = pytest.mark.gpu

B = 2
T0, T1 = 0.25, 0.375
RANGE = "instance index out of range"


def _c(a):
    return np.ascontiguousarray(a)


class Rig:
    def __init__(self, arrangements, case):
        from test_emu import _projectile_case, _two_obstacle_case

        if case == "ball":
            P, x0r, way, _, _, dyn = _projectile_case(arrangements, B, use_feedback_policy=True)
        else:
            P, x0r, way, _, _, chair, ball = _two_obstacle_case(arrangements, B, use_feedback_policy=True)
            chair = chair + np.arange(B)[:, None] * np.array([0.05, -0.1, 0.0, 0.01, 0.02, 0.0, 0.0, 0.03, 0.0])   # the instances differ
            dyn = np.concatenate([chair, ball], axis=1)
        self.P, self.nx, self.N = P, P.nx, P.N
        self.R, self.O = slice(0, P.nx), slice(P.nx, P.nx_full)
        self.x = _c(np.concatenate([x0r, dyn], axis=1))
        assert self.x.shape == (B, {"ball": 36, "chair_ball": 45}[case]) and not np.array_equal(self.x[0, self.O], self.x[1, self.O])
        self.rng = np.random.default_rng(17)
        self.x1 = self.other_obstacles(self.x)          # a second observation: the obstacles somewhere else, moving differently
        self.mpc = BatchMPC(P, B, way_p=way)
        self.mpc.set_projectile_flag(1.0)
        self.fresh = {k: self.message(f) for k, f in FRESH.items()}   # what a handle without a plan refuses

    def other_obstacles(self, x):
        y = x.copy()
        y[:, self.O] += self.rng.uniform(0.05, 0.15, y[:, self.O].shape)
        return y

    def solve(self, t=T0, x=None):
        """a cold solve from the observation (t, x)"""
        self.mpc.reset()
        self.mpc.set_observation(t, self.x if x is None else x)
        self.mpc.advance()

    def updated(self):
        self.solve()
        self.mpc.value_function_update(interface_states=True)

    def stale(self):
        self.updated()
        self.mpc.set_observation(T1, self.x)

    def message(self, f):
        with pytest.raises(RuntimeError) as e:
            f(self)
        return str(e.value)

    def continued(self, got, x, tau):
        """got[..., O] continues the obstacle blocks of the observation x[B][nxf] by tau (per leading index of got)"""
        dyn = np.broadcast_to(x[:, self.O].reshape((B,) + (1,) * (got.ndim - 2) + (-1,)), got[..., self.O].shape)
        assert_ballistic(_c(got[..., self.O]), _c(dyn), tau)


@pytest.fixture(scope="module", params=["ball", "chair_ball"])
def rig(request, arrangements):
    r = Rig(arrangements, request.param)
    yield r
    r.mpc.close()


def knot_tau(r):
    return np.broadcast_to(np.arange(r.N + 1) * r.P.dt, (B, r.N + 1))


def check_solution(r):
    r.solve()
    ts, xs, us = r.mpc.solution()
    assert np.all(np.isfinite(xs)) and np.array_equal(ts, T0 + knot_tau(r))
    r.continued(xs, r.x, knot_tau(r))     # (the accelerations bitwise, and knot 0 the observation itself)
    return dict(xs=xs, us=us)


def check_set_guess(r):
    r.mpc.reset()
    r.mpc.set_observation(T0, r.x)
    xs = np.tile(r.x[:, None, :], (1, r.N + 1, 1))
    xs[..., r.R] += r.rng.uniform(-0.05, 0.05, xs[..., r.R].shape)
    xs[..., r.O] = np.nan                 # the obstacle block of a guess is ignored
    us = r.rng.uniform(-0.1, 0.1, (B, r.N, r.P.nu))
    r.mpc.set_guess(xs, us)
    _, got, gu = r.mpc.solution()
    assert np.array_equal(got[..., r.R].view(np.uint64), xs[..., r.R].view(np.uint64)) and np.array_equal(gu, us)
    r.continued(got, r.x, knot_tau(r))
    return dict(xs=got)


def check_qp_step_and_kkt(r):
    r.mpc.reset()
    r.mpc.set_observation(T0, r.x)
    xs = np.tile(r.x[:, None, :], (1, r.N + 1, 1))
    xs[..., r.O] = np.nan
    r.mpc.set_guess(xs, np.zeros((B, r.N, r.P.nu)))
    dxs, dus = r.mpc.qp_step()
    kkt = r.mpc.qp_kkt()
    for dx in (dxs, kkt["dx"]):
        assert dx.shape == (B, r.N + 1, r.P.nx_full)
        assert np.all(dx[..., r.O] == 0.0) and np.all(np.isfinite(dx[..., r.R])) and np.any(dx[..., r.R] != 0.0)
    assert kkt["pi"].shape == (B, r.N + 1, r.nx) and np.all(np.isfinite(kkt["pi"])) and np.any(kkt["pi"] != 0.0)
    return dict(dxs=dxs, dus=dus, **{"kkt_" + k: v for k, v in kkt.items()})


def check_feedback_gains(r):
    r.solve()
    K = r.mpc.feedback_gains()
    assert K.shape == (B, r.N, r.P.nu, r.P.nx_full)
    assert np.all(K[..., r.O] == 0.0) and np.all(np.isfinite(K)) and np.any(K[..., r.R] != 0.0)
    return dict(K=K)


def check_value_function(r):
    r.updated()
    ctg = r.mpc.cost_to_go()
    k = 3
    x = r.x.copy()
    x[:, r.R] = ctg["X"][:, k] + r.rng.uniform(-0.02, 0.02, (B, r.nx))
    V, g = r.mpc.value_function(T0 + k * r.P.dt, x)
    assert g.shape == (B, r.P.nx_full) and np.all(g[:, r.O] == 0.0)
    V2, g2 = r.mpc.value_function(T0 + k * r.P.dt, r.other_obstacles(x))
    assert np.array_equal(V.view(np.uint64), V2.view(np.uint64)) and np.array_equal(g.view(np.uint64), g2.view(np.uint64))
    for b in range(B):
        want = ctg["pk"][b, k] + ctg["Pk"][b, k] @ (x[b, r.R] - ctg["X"][b, k])
        assert np.abs(g[b, r.R] - want).max() < 1e-9 * max(1.0, np.abs(g[b]).max())
    return dict(V=V, g=g, **ctg)


def check_evaluate_early(r):
    r.solve()
    xe, ue = r.mpc.evaluate(T0 + 0.03)
    r.continued(xe, r.x, (T0 + 0.03) - T0)
    xc, uc = r.mpc.evaluate(T0 - 1.0)      # before the plan: the clamp, the obstacles as observed
    assert np.array_equal(xc[:, r.O].view(np.uint64), r.x[:, r.O].view(np.uint64))
    return dict(xe=xe, ue=ue, xc=xc, uc=uc)


def check_evaluate_after_second_observation(r):
    r.solve()
    r.mpc.set_observation(T1, r.x1)        # no advance: the stored solution still belongs to (T0, x)
    xe, ue = r.mpc.evaluate(T0 + 0.03)
    r.continued(xe, r.x, (T0 + 0.03) - T0)
    xp, up = r.mpc.evaluate(T0 + 0.03, x_obs=r.x1)
    r.continued(xp, r.x, (T0 + 0.03) - T0)
    xs = r.mpc.solution()[1]
    r.continued(xs, r.x1, knot_tau(r))     # ... and the trajectory on the device is for the last observation
    assert not np.array_equal(xs[:, 0, r.O], r.x[:, r.O])
    return dict(xe=xe, ue=ue, xp=xp, up=up, xs=xs)


def check_evaluate_policy_ignores_obstacles(r):
    r.solve()
    xo = r.x.copy()
    xo[:, r.R] += r.rng.uniform(-0.01, 0.01, (B, r.nx))
    xa, ua = r.mpc.evaluate(T0 + 0.02, x_obs=xo)
    xb, ub = r.mpc.evaluate(T0 + 0.02, x_obs=r.other_obstacles(xo))
    assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64)) and np.array_equal(ua.view(np.uint64), ub.view(np.uint64))
    assert np.any(ua != r.mpc.evaluate(T0 + 0.02)[1])      # (the policy saw the robot block)
    return dict(xa=xa, ua=ua)


def check_points(r):
    r.solve()
    n, inst, t = 3, np.array([1, 0, 1], dtype=np.int32), np.array([0.0, 0.4, 1.1])
    X = np.tile(r.x[0], (n, 1))
    X[:, :9] += r.rng.uniform(-0.3, 0.3, (n, 9))
    X[:, 9:r.nx] += r.rng.uniform(-0.05, 0.05, (n, r.nx - 9))
    X = r.other_obstacles(r.other_obstacles(X))       # distinct obstacle blocks per point
    assert len({X[i, r.O].tobytes() for i in range(n)}) == n
    U = r.rng.uniform(-0.2, 0.2, (n, r.P.nu))

    def both(X, sel):
        lin = r.mpc.linearize_points(X[sel], U[sel], t=t[sel], inst=inst[sel])
        d, dq = r.mpc.state_rows(X[sel], t=t[sel], inst=inst[sel])
        return dict(lin, d=d, dq=dq)

    whole = both(X, slice(0, n))
    assert all(np.all(np.isfinite(v)) for v in whole.values())
    for i in range(n):
        one = both(X, slice(i, i + 1))
        for k, v in whole.items():
            assert np.array_equal(v[i:i + 1].view(np.uint64), one[k].view(np.uint64)), (i, k)
    X2 = X.copy()
    X2[1] = r.other_obstacles(X[1:2])[0]
    moved = both(X2, slice(0, n))
    for k, v in whole.items():
        assert np.array_equal(v[[0, 2]].view(np.uint64), moved[k][[0, 2]].view(np.uint64)), k
    assert not np.array_equal(whole["d"][1], moved["d"][1])    # (the rows of point 1 saw its obstacles)
    return whole


def check_tick(r):
    r.mpc.reset()
    xt, ut = r.mpc.tick(T0, r.x)
    assert np.array_equal(xt[:, r.O].view(np.uint64), r.x[:, r.O].view(np.uint64)) and np.all(np.isfinite(xt)) and np.all(np.isfinite(ut))
    xs = r.mpc.solution()[1]
    r.continued(xs, r.x, knot_tau(r))      # (the tick observed the obstacles for the plan too)
    return dict(xt=xt, ut=ut, xs=xs)


CHECKS = [check_solution, check_set_guess, check_qp_step_and_kkt, check_feedback_gains, check_value_function, check_evaluate_early,
          check_evaluate_after_second_observation, check_evaluate_policy_ignores_obstacles, check_points, check_tick]


@pytest.mark.parametrize("chk", CHECKS, ids=lambda f: f.__name__[6:])
def test_interface_states(rig, chk):
    chk(rig)


# ---- the refusals of these entries: (state of the handle, call, message) -------------------------------------------------------------
def _raw(name, *args):
    def f(r):
        check(getattr(_capi.lib(), name)(r.mpc._h, *[a(r) if callable(a) else a for a in args]))
    return f


def _two(r):
    return r.x, np.array([T0, T0 + 0.1]), np.array([0, B], dtype=np.int32)     # two points, the second of an instance that is not there


_D = lambda n: (lambda r: ptr(np.zeros(n)))            # noqa: E731  (an output nobody reads)
_I = lambda r: iptr(np.zeros(2, dtype=np.int32))      # noqa: E731
QUERIES = {
    "value_function": lambda r: r.mpc.value_function(T0, r.x),
    "equality_lagrangian": lambda r: r.mpc.equality_lagrangian(T0),
    "get_cost_to_go": lambda r: r.mpc.cost_to_go(),
}
# what a handle refuses before its first plan (Rig.__init__ collects the messages)
FRESH = dict({k + "_before_update": f for k, f in QUERIES.items()},
             update_without_plan=lambda r: r.mpc.value_function_update(interface_states=True),
             hold_stats_nothing_held=_raw("upr_batch_hold_stats", 1))
NONE_YET = ": no upr_batch_value_function_update on this handle yet"
STALE = ": the cost-to-go is stale (the plan or the observation changed since upr_batch_value_function_update)"
REFUSALS = {
    "value_function_range": (Rig.updated, lambda r: r.mpc.value_function(_two(r)[1], _two(r)[0], inst=_two(r)[2]), RANGE),
    "equality_lagrangian_range": (Rig.updated, lambda r: r.mpc.equality_lagrangian(_two(r)[1], inst=_two(r)[2]), RANGE),
    "state_rows_range": (None, lambda r: r.mpc.state_rows(_two(r)[0], t=_two(r)[1], inst=_two(r)[2]), RANGE),
    "state_rows_range_negative": (None, lambda r: r.mpc.state_rows(_two(r)[0], t=_two(r)[1], inst=np.array([-1, 0])), RANGE),
    "linearize_points_range": (None, lambda r: r.mpc.linearize_points(_two(r)[0], np.zeros((2, r.P.nu)), t=_two(r)[1], inst=_two(r)[2]), RANGE),
    "value_function_null_inst": (Rig.updated, _raw("upr_batch_value_function", 2, None, _D(2), _D(90), _D(2), _D(90)), "upr_batch_value_function: null argument"),
    "value_function_null_t": (Rig.updated, _raw("upr_batch_value_function", 2, _I, None, _D(90), _D(2), _D(90)), "upr_batch_value_function: null argument"),
    "value_function_null_x": (Rig.updated, _raw("upr_batch_value_function", 2, _I, _D(2), None, _D(2), _D(90)), "upr_batch_value_function: null argument"),
    "equality_lagrangian_null_inst": (Rig.updated, _raw("upr_batch_equality_lagrangian", 2, None, _D(2), _D(90)), "upr_batch_equality_lagrangian: null argument"),
    "equality_lagrangian_null_out": (Rig.updated, _raw("upr_batch_equality_lagrangian", 2, _I, _D(2), None), "upr_batch_equality_lagrangian: null argument"),
    "tick_null_x": (None, _raw("upr_batch_tick", _D(2), 1, None, _D(90), _D(90), None), "upr_batch_tick: null argument"),
    "tick_null_out": (None, _raw("upr_batch_tick", _D(2), 1, _D(90), None, _D(90), None), "upr_batch_tick: null argument"),
    # readiness comes first: a stale handle says so whatever else is wrong with the call
    "value_function_stale_before_range": (Rig.stale, lambda r: r.mpc.value_function(_two(r)[1], _two(r)[0], inst=_two(r)[2]), "upr_batch_value_function" + STALE),
    "value_function_stale_before_null": (Rig.stale, _raw("upr_batch_value_function", 2, None, None, None, None, None), "upr_batch_value_function" + STALE),
    # ... then the empty call, which succeeds whatever its pointers are
    "update_without_plan": ("fresh", None, "upr_batch_value_function_update: no plan on this handle yet (advance or set a guess first)"),
    "hold_stats_nothing_held": ("fresh", None, "upr_batch_hold_stats: nothing held on this handle"),
}
for _k, _f in QUERIES.items():
    REFUSALS[_k + "_before_update"] = ("fresh", None, "upr_batch_" + _k + NONE_YET)
    REFUSALS[_k + "_stale"] = (Rig.stale, _f, "upr_batch_" + _k + STALE)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(rig, name):
    state, call, msg = REFUSALS[name]
    if state == "fresh":
        assert rig.fresh[name] == msg
        return
    if state:
        state(rig)
    assert rig.message(call) == msg


def test_empty_query_and_held_statistics(rig):
    """n <= 0 comes before the null and range checks (and after readiness); a snapshot held across an update is the caller's own"""
    L = _capi.lib()
    rig.updated()
    assert L.upr_batch_value_function(rig.mpc._h, 0, None, None, None, None, None) == 0
    assert L.upr_batch_equality_lagrangian(rig.mpc._h, 0, None, None, None) == 0
    rig.solve()
    before = rig.mpc.stats()
    with rig.mpc.preserved_stats():
        rig.mpc.value_function_update(interface_states=True)     # (takes and puts back a snapshot of its own inside the caller's)
        rig.mpc.qp_kkt()
    after = rig.mpc.stats()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert rig.message(_raw("upr_batch_hold_stats", 1)) == "upr_batch_hold_stats: nothing held on this handle"
