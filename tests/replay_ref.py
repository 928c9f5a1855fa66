"""CPU reference of the replay of a time law on a clock (upright_amd/csrc/upr_replay.h), its cases and the assertions its CPU and GPU
tests share.  The plans, the lattices and the closed form of the slide are retime_ref's, the residual is balance_ref's; neither module is
changed.

The reference is numpy throughout: the knot times are np.cumsum of 2 h / (s_i + s_{i+1}), the segment of a sample np.searchsorted on
them (side="right": a sample on a knot takes the departing side), the path between two knots the quintic Hermite interpolant written
out below, the state (Q, s Q', s^2 Q'' + d Q'); rho_ref of a sample is balance_ref.reference at that JOINT-SPACE state.  A sample is
rejected when rho_ref > EPS max(|b|, 1) and DECIDED when |rho_ref - EPS max(|b|, 1)| > RHO_TOL max(|b|, 1), the family's rule for "away
from the boundary".  On the slide (retime_ref.slide_plans: a translation on a minimum-jerk profile) the closed form of a sample's margin
is mu0 g0 - |s^2 c(tau) + d w(tau)|, c and w the analytic second and first derivative of the profile at u = (i h + tau) / (N h).

run(P, xs, params, speeds, level, tick, t0=0.0, K=None, boxes=True, form=-1) -> dict(duration, count, x, rho, excess, iters, worst,
verdict, box_first[, times]) with the RAW arrays of the entry (nothing set to NaN in Python) is what a test file hands to the bodies
below; params None: every instance's own body parameters."""
import ctypes as C
import os
from pathlib import Path

import numpy as np

import balance_ref as R
import retime_ref as Q

EPS, RHO_TOL = Q.EPS, Q.RHO_TOL
TOL_Q, TOL_V, TOL_A = 1e-12, 1e-10, 1e-9      # states, at the scale max(1, |x|_inf) of the sample
RAMP = [1, 2, 3, 4] + [5] * 13 + [4, 3, 2, 1]
ZIGZAG = [1, 2, 3, 4, 5, 4, 3, 2, 1, 2, 3, 4, 5, 4, 3, 2, 1, 2, 3, 4, 5]
GENERIC_ZIGZAG = [0, 2, 4, 2] * 5 + [0]


# ---- numpy's replay -------------------------------------------------------------------------------------------------------------------
def knot_times(level, speeds, h):
    """T (.., N + 1): 0 and the cumulative 2 h / (s_i + s_{i+1}); NaN throughout where level is -1"""
    level = np.asarray(level)
    s = np.asarray(speeds, dtype=np.float64)[np.maximum(level, 0)]
    T = np.zeros(level.shape)
    with np.errstate(divide="ignore"):
        T[..., 1:] = np.cumsum(2.0 * h / (s[..., :-1] + s[..., 1:]), axis=-1)
    T[(level < 0).any(axis=-1)] = np.nan
    return T


def hermite(x0, x1, h, g, nq):
    """(Q, Q', Q'') of the quintic Hermite interpolant of the records x0, x1 = (q, v, a) at sigma = g"""
    c = [x0[:nq], h * x0[nq:2 * nq], h * h * x0[2 * nq:3 * nq], x1[:nq], h * x1[nq:2 * nq], h * h * x1[2 * nq:3 * nq]]
    H = [1 - 10 * g**3 + 15 * g**4 - 6 * g**5, g - 6 * g**3 + 8 * g**4 - 3 * g**5, .5 * g**2 - 1.5 * g**3 + 1.5 * g**4 - .5 * g**5,
         10 * g**3 - 15 * g**4 + 6 * g**5, -4 * g**3 + 7 * g**4 - 3 * g**5, .5 * g**3 - g**4 + .5 * g**5]
    D = [-30 * g**2 + 60 * g**3 - 30 * g**4, 1 - 18 * g**2 + 32 * g**3 - 15 * g**4, g - 4.5 * g**2 + 6 * g**3 - 2.5 * g**4,
         30 * g**2 - 60 * g**3 + 30 * g**4, -12 * g**2 + 28 * g**3 - 15 * g**4, 1.5 * g**2 - 4 * g**3 + 2.5 * g**4]
    E = [-60 * g + 180 * g**2 - 120 * g**3, -36 * g + 96 * g**2 - 60 * g**3, 1 - 9 * g + 18 * g**2 - 10 * g**3,
         60 * g - 180 * g**2 + 120 * g**3, -24 * g + 84 * g**2 - 60 * g**3, 3 * g - 12 * g**2 + 10 * g**3]
    return sum(a * b for a, b in zip(H, c)), sum(a * b for a, b in zip(D, c)) / h, sum(a * b for a, b in zip(E, c)) / (h * h)


def sample_state(x0, x1, s0, s1, h, tp, nq):
    """(state (3 nq), tau, s, d) of a sample tp after the departing knot"""
    d = Q.accel(s0, s1, h)
    s = s0 + d * tp
    tau = min(max(tp * (s0 + 0.5 * d * tp), 0.0), h)
    q, q1, q2 = hermite(x0, x1, h, tau / h, nq)
    return np.concatenate([q, s * q1, s * s * q2 + d * q1]), tau, s, d


def replay(P, xs, level, speeds, tick, t0, K):
    """numpy's samples of ONE plan xs (N + 1, 3 nq) under the law level (N + 1,): dict(T, duration, count, t (K,), x (K, 3 nq), seg, tau,
    s, d (K,), box (K,): the smallest distance of s Q' and s^2 Q'' + d Q' to their bounds, >= 0 inside).  Past the end: the state at T_N;
    without a law (q_0, 0, 0)."""
    nq, N, h = P.nq, P.N, float(P.dt)
    speeds = np.asarray(speeds, dtype=np.float64)
    t = t0 + np.arange(K, dtype=np.float64) * tick
    out = dict(t=t, x=np.zeros((K, 3 * nq)), seg=np.zeros(K, dtype=int), tau=np.zeros(K), s=np.zeros(K), d=np.zeros(K), box=np.full(K, np.inf))
    if level[0] < 0:
        out["x"][:, :nq] = xs[0, :nq]
        return dict(out, T=np.full(N + 1, np.nan), duration=np.inf, count=0)
    T = knot_times(level, speeds, h)
    sp = speeds[level]
    lb, ub = np.asarray(P.x_lb)[nq:3 * nq], np.asarray(P.x_ub)[nq:3 * nq]
    count = int(np.count_nonzero(t <= T[N]))
    for k in range(K):
        tc = min(t[k], T[N])
        i = min(int(np.searchsorted(T, tc, side="right")) - 1, N - 1)
        x, tau, s, d = sample_state(xs[i], xs[i + 1], sp[i], sp[i + 1], h, tc - T[i], nq)
        out["x"][k], out["seg"][k], out["tau"][k], out["s"][k], out["d"][k] = x, i, tau, s, d
        out["box"][k] = min((x[nq:] - lb).min(), (ub - x[nq:]).min())
    return dict(out, T=T, duration=float(T[N]), count=count)


def judged(P, x, theta):
    """(rejected, decided, excess_ref) of the states x (n, 3 nq) under theta (nb, 10) by balance_ref.reference"""
    o = R.reference(P, x, np.asarray(theta)[None], False)
    rho, scale = o["rho"][:, 0], np.maximum(o["bnorm"][:, 0], 1.0)
    return rho > EPS * scale, np.abs(rho - EPS * scale) > RHO_TOL * scale, rho / scale


def reduce_np(excess, count):
    """numpy's (worst (B, ns), verdict (B, ns, 3)) of excess (B, K, ns) over the first count (B,) samples"""
    B, K, ns = excess.shape
    worst, verdict = np.full((B, ns), np.nan), np.zeros((B, ns, 3), dtype=np.int32)
    for b in range(B):
        for sc in range(ns):
            e = excess[b, :count[b], sc]
            rej = ~(e <= EPS)
            if e.size:
                worst[b, sc] = e.max()
            verdict[b, sc] = (int(np.argmax(e)) if e.size else -1, int(np.flatnonzero(rej)[0]) if rej.any() else -1, int(rej.sum()))
    return worst, verdict


def slide_margins(S, rp, b=0):
    """the closed-form margins (K,) of numpy's samples rp of plan b of retime_ref.slide_case, in units of mu0 g0"""
    P = S["P"]
    Tt = P.N * float(P.dt)
    length = S["xs"][b, -1, 0] - S["xs"][b, 0, 0]
    _, d1, d2 = Q.min_jerk((rp["seg"] * float(P.dt) + rp["tau"]) / Tt)
    return (S["bound"] - np.abs(rp["s"] ** 2 * length * d2 / (Tt * Tt) + rp["d"] * length * d1 / Tt)) / S["bound"]


def knot_margins(S, level, speeds):
    """the closed-form margins of both end states of every segment, in units of mu0 g0"""
    h, N = float(S["P"].dt), S["P"].N
    s = np.asarray(speeds, dtype=np.float64)[np.asarray(level)]
    out = []
    for i in range(N):
        d = Q.accel(s[i], s[i + 1], h)
        out += [S["bound"] - abs(s[k] ** 2 * S["c"][k] + d * S["w"][k]) for k in (i, i + 1)]
    return np.array(out) / S["bound"]


# ---- the kernel source through the host emulation -----------------------------------------------------------------------------------
def emu_lib(fma=False):
    name = "libupr_replay_emu_fma.so" if fma else "libupr_replay_emu.so"
    return C.CDLL(os.environ.get("UPR_REPLAY_EMU_FMA_LIB" if fma else "UPR_REPLAY_EMU_LIB", str(Path(__file__).resolve().parent / "emu" / name)))


def have_fma_twin():
    try:
        has_fma = " fma " in Path("/proc/cpuinfo").read_text().replace("\n", " ")
    except OSError:
        has_fma = False
    if has_fma:
        assert (Path(__file__).resolve().parent / "emu" / "libupr_replay_emu_fma.so").exists(), "the host has FMA but libupr_replay_emu_fma.so was not built"
    return has_fma


def blank(P, B, K, ns):
    """the outputs of a call, poisoned"""
    return dict(duration=np.full(B, -7.0), count=np.full(B, -7, dtype=np.int32), x=np.full((B, K, 3 * P.nq), -7.0), rho=np.full((B, K, ns), -7.0),
                excess=np.full((B, K, ns), -7.0), iters=np.full((B, K, ns), -7, dtype=np.int32), worst=np.full((B, ns), -7.0),
                verdict=np.full((B, ns, 3), -7, dtype=np.int32), box_first=np.full(B, -7, dtype=np.int32))


def default_K(level, speeds, h, tick, t0):
    T = knot_times(level, speeds, h)[..., -1]
    T = T[np.isfinite(T)]
    return max(1, int(np.floor((T.max() - t0) / tick)) + 1) if T.size and T.max() >= t0 else 1


def _scenarios(P, B, params):
    if params is None:
        return np.ascontiguousarray(np.repeat(np.asarray(P.body_params, dtype=np.float64)[None, None], B, axis=0)), True
    params = np.ascontiguousarray(params, dtype=np.float64)
    return params, params.ndim == 4


def run_emu(P, xs, params, speeds, level, tick, t0=0.0, K=None, boxes=True, form=-1, fma=False):
    from upright_amd import _capi

    xs = np.ascontiguousarray(xs, dtype=np.float64)
    B, nk = xs.shape[:2]
    params, per = _scenarios(P, B, params)
    ns = params.shape[1] if per else params.reshape(-1, P.nb, 10).shape[0]
    speeds = np.ascontiguousarray(speeds, dtype=np.float64)
    level = np.ascontiguousarray(level, dtype=np.int32)
    K = default_K(level, speeds, float(P.dt), tick, t0) if K is None else K
    out = blank(P, B, K, ns)
    out["times"] = np.full((B, nk), -7.0)
    cp = _capi.problem_to_c(P)
    rc = emu_lib(fma).emu_rpl_plan(C.byref(cp), B, nk, _capi.ptr(xs), ns, _capi.ptr(params), 1 if per else 0, speeds.size, _capi.ptr(speeds), _capi.iptr(level),
                                   C.c_double(tick), C.c_double(t0), K, int(boxes), _capi.ptr(out["duration"]), _capi.iptr(out["count"]), _capi.ptr(out["x"]),
                                   _capi.ptr(out["rho"]), _capi.ptr(out["excess"]), _capi.iptr(out["iters"]), _capi.ptr(out["worst"]),
                                   _capi.iptr(out["verdict"]), _capi.iptr(out["box_first"]), _capi.ptr(out["times"]), int(form))
    assert rc == 0
    return out


def emu_state(P, x0, x1, s0, s1, tp, fma=False):
    """upr_rpl_state through the emulation: (state (3 nq), box flag)"""
    from upright_amd import _capi

    x0, x1 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(x1, dtype=np.float64)
    out = np.zeros(3 * P.nq)
    cp = _capi.problem_to_c(P)
    f = emu_lib(fma).emu_rpl_state
    f.restype = C.c_int
    flag = f(C.byref(cp), _capi.ptr(x0), _capi.ptr(x1), C.c_double(s0), C.c_double(s1), C.c_double(float(P.dt)), C.c_double(tp), _capi.ptr(out))
    return out, bool(flag)


def emu_locate(T, t):
    from upright_amd import _capi

    T = np.ascontiguousarray(T, dtype=np.float64)
    i, tp = C.c_int(-1), C.c_double(np.nan)
    emu_lib().emu_rpl_locate(_capi.ptr(T), T.size - 1, C.c_double(t), C.byref(i), C.byref(tp))
    return i.value, tp.value


def run_device(mpc, xs, params, speeds, level, tick, t0=0.0, K=None, boxes=True):
    """upr_batch_replay_plan through ctypes on the plan xs installed with set_guess: every output of ONE call, raw"""
    from upright_amd import _capi

    P = mpc.problem
    mpc.set_guess(xs, np.zeros((mpc.B, mpc.N, mpc.nu)))
    B = mpc.B
    speeds = np.ascontiguousarray(speeds, dtype=np.float64)
    level = np.ascontiguousarray(level, dtype=np.int32)
    if params is None:
        ns, per, par = 1, 0, None
    else:
        par, per = _scenarios(P, B, params)
        ns = par.shape[1] if per else par.reshape(-1, P.nb, 10).shape[0]
    K = default_K(level, speeds, float(P.dt), tick, t0) if K is None else K
    out = blank(P, B, K, ns)
    rc = mpc._lib.upr_batch_replay_plan(mpc._h, ns, _capi.ptr(par), int(per), speeds.size, _capi.ptr(speeds), _capi.iptr(level), float(tick), float(t0), K,
                                        int(boxes), _capi.ptr(out["duration"]), _capi.iptr(out["count"]), _capi.ptr(out["x"]), _capi.ptr(out["rho"]),
                                        _capi.ptr(out["excess"]), _capi.iptr(out["iters"]), _capi.ptr(out["worst"]), _capi.iptr(out["verdict"]),
                                        _capi.iptr(out["box_first"]))
    assert rc == 0, mpc._lib.upr_last_error()
    return out


# ---- what every answer must satisfy -----------------------------------------------------------------------------------------------------
def state_errors(x, ref):
    """the largest |x - ref| of the q, qdot and qddot blocks over the samples, each at the scale max(1, |ref|_inf) of its sample"""
    nq = x.shape[-1] // 3
    scale = np.maximum(1.0, np.abs(ref).max(axis=-1, keepdims=True))
    e = np.abs(x - ref) / scale
    return float(e[..., :nq].max()), float(e[..., nq:2 * nq].max()), float(e[..., 2 * nq:].max())


def assert_states(x, ref, what=""):
    eq, ev, ea = state_errors(x, ref)
    assert eq <= TOL_Q and ev <= TOL_V and ea <= TOL_A, (what, eq, ev, ea)
    return eq, ev, ea


def check_call(P, xs, params, speeds, level, tick, t0, out, boxes=True, decided_min=0.9):
    """One answer against numpy's replay and the reference: T_N and count equal as doubles / ints, the states within the tolerances,
    NaN and 0 past the end, the decisions equal on decided samples, box_first where numpy's box decisions lie >= 1e-9 from their bounds,
    worst and verdict numpy's reduction of the answer's own excess.  Returns dict(errors, decided, total, rejected (B, ns) lists)."""
    B, K = out["x"].shape[:2]
    params_b, per = _scenarios(P, B, params)
    ns = out["excess"].shape[2]
    errs, n_dec, n_tot, rejected = np.zeros(3), 0, 0, {}
    for b in range(B):
        rp = replay(P, xs[b], level[b], speeds, tick, t0, K)
        assert out["duration"][b] == rp["duration"], (b, out["duration"][b], rp["duration"])
        assert out["count"][b] == rp["count"], (b, out["count"][b], rp["count"])
        if "times" in out and level[b][0] >= 0:
            assert np.array_equal(out["times"][b], rp["T"]), b
        errs = np.maximum(errs, assert_states(out["x"][b], rp["x"], b))
        n = rp["count"]
        assert np.all(np.isnan(out["excess"][b, n:])) and np.all(np.isnan(out["rho"][b, n:])) and np.all(out["iters"][b, n:] == 0)
        assert np.all(np.isfinite(out["excess"][b, :n])) and np.all(out["iters"][b, :n] >= 0)
        if boxes:
            assert np.abs(rp["box"][:n]).min(initial=np.inf) >= 1e-9, (b, np.abs(rp["box"][:n]).min())   # (on numpy alone)
            outside = np.flatnonzero(rp["box"][:n] < 0)
            assert out["box_first"][b] == (outside[0] if outside.size else -1), (b, out["box_first"][b], outside)
        else:
            assert out["box_first"][b] == -1
        for sc in range(ns):
            theta = params_b[b, sc] if per else params_b.reshape(-1, P.nb, 10)[sc]
            rej, dec, _ = judged(P, rp["x"][:n], theta)
            got = ~(out["excess"][b, :n, sc] <= EPS)
            assert np.array_equal(got[dec], rej[dec]), (b, sc, np.flatnonzero(got != rej))
            scale = out["rho"][b, :n, sc] / np.where(out["excess"][b, :n, sc] > 0, out["excess"][b, :n, sc], 1.0)
            assert np.all((out["excess"][b, :n, sc] == 0) | (scale >= 1.0 - 1e-12))
            n_dec += int(dec.sum()); n_tot += n
            rejected[b, sc] = np.flatnonzero(rej).tolist()
    assert n_tot == 0 or n_dec >= decided_min * n_tot, (n_dec, n_tot)       # (on the reference alone)
    worst, verdict = reduce_np(out["excess"], out["count"])
    assert np.array_equal(out["worst"], worst, equal_nan=True) and np.array_equal(out["verdict"], verdict), (out["worst"], worst, out["verdict"], verdict)
    return dict(errors=errs, decided=n_dec, total=n_tot, rejected=rejected)


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------------------------
def generic_laws(arrangements):
    """retime_ref.generic_case (B = 3, `shifted`, M = 5) with its laws: (name, level (B, N + 1)) -- each plan's own optimal law under
    scenario 0 from numpy's programme on the reference masks, all levels 4, the zigzag 0 2 4 2 0 .."""
    G = Q.generic_case(arrangements)
    if "replay_laws" not in G:
        P, h = G["P"], float(G["P"].dt)
        own = np.stack([Q.programme(G["ref"]["masks"][b, 0], G["speeds"], h)["level"] for b in range(G["xs"].shape[0])])
        B = G["xs"].shape[0]
        G["replay_laws"] = [("own", own), ("top", np.full((B, P.N + 1), 4, dtype=np.int32)), ("zigzag", np.tile(np.array(GENERIC_ZIGZAG, dtype=np.int32), (B, 1)))]
    return G, G["replay_laws"]


# ---- the assertions both test files make ----------------------------------------------------------------------------------------------
def body_between_knots(run, arrangements, retime=None):
    """1.  Returns the rejected samples of plan 0."""
    S = Q.slide_case(arrangements)
    P, sp, N = S["P"], np.array([1.1185]), S["P"].N
    level = np.zeros((2, N + 1), dtype=np.int32)
    tick, K = 0.01, 179
    km = knot_margins(S, level[0], sp)
    rp = replay(P, S["xs"][0], level[0], sp, tick, 0.0, K)
    m = slide_margins(S, rp)
    want = np.flatnonzero(m < 0)
    print("replay, slide at 1.1185: knot margins >= %.2e, sample margins %.2e from the bound, rejected by the closed form: %s (segments %s)"
          % (km.min(), np.abs(m).min(), want.tolist(), sorted(set(rp["seg"][want].tolist()))))
    assert km.min() >= 1e-6 and np.abs(m).min() >= 1e-6 and want.size >= 1 and rp["count"] == K     # (on the closed form alone)
    out = run(P, S["xs"], S["params"], sp, level, tick, K=K, boxes=False)
    for b in range(2):
        mb = slide_margins(S, replay(P, S["xs"][b], level[b], sp, tick, 0.0, K), b)
        got = np.flatnonzero(~(out["excess"][b, :, 0] <= EPS))
        assert np.array_equal(got, np.flatnonzero(mb < 0)), (b, got, np.flatnonzero(mb < 0))
        assert out["count"][b] == K and tuple(out["verdict"][b, 0, 1:]) == (got[0], got.size) and out["worst"][b, 0] > EPS
        assert out["verdict"][b, 0, 0] in got and out["worst"][b, 0] == out["excess"][b, :, 0].max()
    assert set(rp["seg"][want].tolist()) == {4, 15}
    if retime is not None:
        dur = retime(P, S["xs"], S["params"], sp)       # the retiming accepts every knot: the case the replay exists for
        assert np.all(np.isfinite(dur)) and np.allclose(dur, N * float(P.dt) / 1.1185, rtol=1e-12)
    return want.tolist()


def body_slide_laws(run, arrangements):
    """2."""
    S = Q.slide_case(arrangements)
    P, N = S["P"], S["P"].N
    sp = S["speeds"]
    res = {}
    for name, law, K in (("ramp", RAMP, 46), ("zigzag", ZIGZAG, 59), ("uniform 1.25", [4] * (N + 1), 44)):
        level = np.tile(np.array(law, dtype=np.int32), (2, 1))
        rp = replay(P, S["xs"][0], level[0], sp, 0.037, 0.0, K)
        m = slide_margins(S, rp)
        assert rp["count"] == K and np.abs(m).min() >= 1e-6, (name, rp["count"], np.abs(m).min())     # (on the closed form alone)
        out = run(P, S["xs"], S["params"], sp, level, 0.037, K=K, boxes=False)
        got = np.flatnonzero(~(out["excess"][0, :, 0] <= EPS))
        assert np.array_equal(got, np.flatnonzero(m < 0)), (name, got, np.flatnonzero(m < 0))
        assert out["count"][0] == K and out["verdict"][0, 0, 2] == got.size
        res[name] = (float(np.abs(m).min()), got.size)
    print("replay, slide laws: (min |margin| / mu0 g0, rejected) %s" % res)
    assert all(n >= 1 for _, n in res.values())
    return res


def body_generic(run, arrangements, form=-1):
    """4.  Returns {law: (state errors, decided, total, rejected samples)}."""
    G, laws = generic_laws(arrangements)
    P = G["P"]
    res = {}
    for name, level in laws:
        out = run(P, G["xs"], G["params"], G["speeds"], level, 0.05, form=form)
        r = check_call(P, G["xs"], G["params"], G["speeds"], level, 0.05, 0.0, out)
        res[name] = (r["errors"].tolist(), r["decided"], r["total"], sum(len(v) for v in r["rejected"].values()), out["count"].tolist(), out["box_first"].tolist(),
                     sum(len(v) for (_, sc), v in r["rejected"].items() if sc == 0))
    print("replay, generic: law -> (state errors q, qdot, qddot; decided; jobs; rejected; count; box_first; rejected under scenario 0) %s" % res)
    # (the own laws are scenario 0's: the reference rejects none of their samples under it; under scenario 1 they are another plan's law)
    assert res["own"][6] == 0 and res["top"][3] >= 1 and res["zigzag"][3] >= 1
    assert len(set(res["own"][4])) > 1                         # (count differs across the plans: NaN tails)
    return res


def body_edges(run, arrangements):
    """5. (the shapes that need no second form)"""
    S, (G, laws) = Q.slide_case(arrangements), generic_laws(arrangements)
    P, sp, h, N = S["P"], S["speeds"], float(S["P"].dt), S["P"].N
    ramp = np.tile(np.array(RAMP, dtype=np.int32), (2, 1))
    T = knot_times(ramp[0], sp, h)
    kw = dict(boxes=False)
    # K = 1; t0 > 0; t0 past the end
    for t0, K in ((0.0, 1), (0.3, 7), (T[N] + 0.01, 3), (T[N], 2)):
        out = run(P, S["xs"], S["params"], sp, ramp, 0.1, t0=t0, K=K, **kw)
        check_call(P, S["xs"], S["params"], sp, ramp, 0.1, t0, out, boxes=False, decided_min=0.0)
    assert np.all(out["count"] == 1)                           # (the sample at T_N exists, the next does not)
    out = run(P, S["xs"], S["params"], sp, ramp, 0.1, t0=T[N] + 0.01, K=3, **kw)
    assert np.all(out["count"] == 0) and np.all(np.isnan(out["worst"])) and np.all(out["verdict"] == np.array([-1, -1, 0]))
    assert_states(out["x"][0, 0], np.concatenate([S["xs"][0, N, :P.nq], 0.5 * S["xs"][0, N, P.nq:2 * P.nq], 0.25 * S["xs"][0, N, 2 * P.nq:]]))
    # a sample exactly on a knot takes the departing side (the ramp: d changes at knots 1 .. 4, and the two sides differ in qddot)
    _, dep, arr = Q.retimed_states(S["xs"][:1], ramp[:1, None], sp, h, P.nq)
    n_sides = 0
    for i in (1, 2, 3, 4, 17, 18):
        out = run(P, S["xs"][:1], S["params"], sp, ramp[:1], 0.1, t0=float(T[i]), K=1, **kw)
        assert out["count"][0] == 1
        assert_states(out["x"][0, 0], dep[0, 0, i], i)
        gap = np.abs(dep[0, 0, i] - arr[0, 0, i - 1]).max()
        n_sides += int(gap > 1e-3 and np.abs(out["x"][0, 0] - arr[0, 0, i - 1]).max() > 0.5 * gap)
    assert n_sides >= 3
    # a plan with no law in a batch with others
    mixed = ramp.copy()
    mixed[1] = -1
    out = run(P, S["xs"], S["params"], sp, mixed, 0.037, K=46, **kw)
    check_call(P, S["xs"], S["params"], sp, mixed, 0.037, 0.0, out, boxes=False)
    assert out["count"][1] == 0 and out["duration"][1] == np.inf and out["count"][0] == 46 and np.isnan(out["worst"][1, 0])
    want = np.zeros(3 * P.nq)
    want[:P.nq] = S["xs"][1, 0, :P.nq]
    assert np.array_equal(out["x"][1], np.tile(want, (46, 1)))
    # speed 0 at the first knot, s_1 > 0
    rest = np.tile(np.array([0, 1, 2, 3] + [3] * 13 + [3, 2, 1, 1], dtype=np.int32), (2, 1))
    out = run(P, S["xs"], S["params"], sp, rest, 0.05, **kw)
    check_call(P, S["xs"], S["params"], sp, rest, 0.05, 0.0, out, boxes=False)
    assert np.all(out["x"][:, 0, P.nq:2 * P.nq] == 0.0) and out["count"][0] >= out["x"].shape[1] - 1
    # params: None (n_scen = 1), shared, per instance
    own = laws[0][1]
    Pg = G["P"]
    th0 = np.asarray(Pg.body_params, dtype=np.float64)[None]
    none = run(Pg, G["xs"], None, G["speeds"], own, 0.05)
    shared = run(Pg, G["xs"], th0, G["speeds"], own, 0.05)
    assert all(np.array_equal(none[k], shared[k], equal_nan=True) for k in none if k != "times")
    per = np.stack([G["params"], G["params"][::-1], G["params"]])
    out = run(Pg, G["xs"], per, G["speeds"], own, 0.05)
    check_call(Pg, G["xs"], per, G["speeds"], own, 0.05, 0.0, out)
    two = run(Pg, G["xs"], G["params"], G["speeds"], own, 0.05)
    assert np.array_equal(out["excess"][0], two["excess"][0], equal_nan=True) and np.array_equal(out["excess"][1, :, 0], two["excess"][1, :, 1], equal_nan=True)


def multi_body_case(arrangements):
    if "replay_die2" not in Q._CASES:
        P = R.table_problem(arrangements, "foam_die2")
        Q._CASES["replay_die2"] = dict(P=P, xs=Q.quintic_plans(P, 2, 11, 1.6), params=Q.shifted(P), speeds=np.array([0.5, 1.0, 1.5]),
                                       level=np.tile(np.array([1, 2, 1, 0] * 5 + [1], dtype=np.int32), (2, 1)))
    return Q._CASES["replay_die2"]


def body_multi_body(run, arrangements):
    """5. foam_die2 (two bodies, eight contacts), B = 2"""
    M = multi_body_case(arrangements)
    out = run(M["P"], M["xs"], M["params"], M["speeds"], M["level"], 0.05)
    r = check_call(M["P"], M["xs"], M["params"], M["speeds"], M["level"], 0.05, 0.0, out)
    print("replay, foam_die2: decided %d of %d jobs, rejected %d, state errors %s" % (r["decided"], r["total"], sum(len(v) for v in r["rejected"].values()), r["errors"]))
    return out


def agree(a, b, P, xs, params, speeds, level, tick, exact=False):
    """6. two builds of the same source: count equal, states within the tolerances, decisions equal on decided samples; exact (device
    against the emulation of what it runs): iters on decided samples and verdict on plans whose samples are all decided too"""
    B, K = a["x"].shape[:2]
    params_b, per = _scenarios(P, B, params)
    assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["duration"], b["duration"]) and np.array_equal(a["box_first"], b["box_first"])
    assert_states(a["x"], b["x"])
    n_dec = 0
    for bb in range(B):
        n = int(a["count"][bb])
        rp = replay(P, xs[bb], level[bb], speeds, tick, 0.0, K)
        all_dec = True
        for sc in range(a["excess"].shape[2]):
            theta = params_b[bb, sc] if per else params_b.reshape(-1, P.nb, 10)[sc]
            _, dec, _ = judged(P, rp["x"][:n], theta)
            assert np.array_equal((a["excess"][bb, :n, sc] <= EPS)[dec], (b["excess"][bb, :n, sc] <= EPS)[dec])
            if exact:
                assert np.array_equal(a["iters"][bb, :n, sc][dec], b["iters"][bb, :n, sc][dec]), (bb, sc)
            all_dec = all_dec and bool(dec.all())
            n_dec += int(dec.sum())
        if exact and all_dec:
            assert np.array_equal(a["verdict"][bb, :, 1:], b["verdict"][bb, :, 1:]), (bb, a["verdict"][bb], b["verdict"][bb])
    return n_dec
