"""CPU reference of the batched speed margin (upright_amd/csrc/upr_speed.h), its case table and the assertions its CPU and GPU tests
share.

rho_ref(s) of a job is balance_ref.reference at x_s = (q, s v, s^2 a): the oracle's b and A at the scaled state, the smallest of the
three CPU residuals; nothing of b(s) = b0 + s^2 (b1 - b0) is in it.  A speed is accepted when rho_ref <= EPS max(|b|, 1).  The class of
a job comes from evaluations on the reference alone at 0, 1 - 1e-3, 1 + 1e-3 and s_max, plus a 65-point grid of [0, s_max] for the
emptiness decision:
    all        rest and s_max both accepted;
    upper_lt1  rest accepted, s_max not, 1 - 1e-3 not: the plan must be slowed down;
    upper_one  rest and 1 - 1e-3 accepted, 1 + 1e-3 not: the upper end is the nominal speed;
    upper_gt1  rest and 1 + 1e-3 accepted, s_max not: the plan could be sped up;
    window     rest rejected, some speed accepted;
    none       no speed accepted (the grid and the four points).
Jobs.replay is the algorithm of upr_speed.h (upr_spd_ctl, transcribed) on rho_ref.

The table (build_case): per arrangement the launches 64 x 4 = 256 jobs (shared scenarios), 7 x 37 = 259 (per point), 37 x 1 in both
layouts and 1 x 1 in both layouts.  The states (make_states; q from tilted_q, a Newton iteration on the tray's third row so that
`level` means level to rounding):
    rest       v = a = 0 on a level tray;
    facet c    a level tray at v = 0 whose load feels g0 (e_z + c mu0 s) in the tray frame, s a pyramid axis of contact 0,
               c in {1/4, 1, 4}: s+ = 1 / sqrt(c) where sliding on that facet binds;
    liftoff    a level tray at v = 0 with a_ee = (k - g0) e_z, k in [5, 8]: s+ = sqrt(g0 / (g0 - k));
    comp       the tray pitched by phi, tan phi = 2 max mu, about a pyramid axis, horizontal acceleration g0 tan phi uphill: at s = 1
               the load is purely normal; where sliding binds, s-^2 = (t - mu) / (t (1 + mu t)), s+^2 = (t + mu) / (t (1 - mu t)),
               t = tan phi;
    comp sigma the same with the acceleration divided by sigma^2: the load is purely normal at s = sigma and the window is sigma times
               the one above.  sigma = 0.25: the window lies below the nominal speed and excludes rest, so only the descent search
               of upr_speed.h finds a seed, after rejected midpoints at 2, 1 and 0.5 whose slope must send it down (with the sign
               of the slope inverted the search walks up and the job ends as none: Jobs.replay(flip=True)); sigma = 3: where the
               friction is small enough for the window to fit between 2 and s_max, a descent that must go up; sigma = 4: rejected
               at rest and at the nominal speed, accepted at s_max -- the seed is s_max and the upper end is open;
    aggr       the same tilt with the acceleration downhill: nothing balances it;
    inside / outside   the generic kinds of balance_ref.points (arrangements with friction only: without it the slightly tilted tray
               of those kinds is unbalanced at every speed and each such job would cost the 65-point grid).
The fixture-box `down` family next to an unbounded-force threshold is not part of it."""
import numpy as np

import balance_ref as R
from oracle.oracle import Oracle

EPS = 1e-8           # UPR_BAL_FEAS
BISECT = 32          # UPR_BAL_BISECT
K = 1 << BISECT
S_MAX = 4.0
RHO_TOL = 1e-9       # the project's bound on |rho - rho_ref| / max(|b|, 1) (tests/test_balance_check.py)
GRID = 65
NAMES = [r[0] for r in R.TABLE + R.EXTRA]
ONE_BODY = [r[0] for r in R.TABLE + R.EXTRA if r[4][0] == 1]
CLASSES = ("all", "upper_lt1", "upper_one", "upper_gt1", "window", "none")
FACET_C = (0.25, 1.0, 4.0)


def scaled_state(x, s, nq):
    """x_s = (q, s v, s^2 a)"""
    x = np.array(x, dtype=np.float64)
    x[..., nq:2 * nq] *= s
    x[..., 2 * nq:3 * nq] *= s * s
    return x


def at(k, s_max=S_MAX):
    return s_max * (float(k) * 2.0 ** -BISECT)


# ---- states ---------------------------------------------------------------------------------------------------------------------------
def tilted_q(P, O, rng, row2=(0.0, 0.0)):
    """A configuration whose tray has C_we[2, 0:2] = row2 (the third row of C_we is the world's vertical in the tray frame; (0, 0): a
    level tray), from balance_ref.level_q by Newton steps on the oracle's kinematic Jacobian."""
    nq = P.nq
    q = R.level_q(P, rng)
    for _ in range(30):
        x = np.concatenate([q, np.zeros(2 * nq)])
        ee, dee = O.ee_kinematics(x, jac=True)
        err = np.array([ee[3 + 6] - row2[0], ee[3 + 7] - row2[1]])
        if np.abs(err).max() < 1e-15:
            break
        J = dee[[3 + 6, 3 + 7], :nq]
        q = q - np.linalg.lstsq(J, err, rcond=None)[0]
    assert np.abs(err).max() < 1e-13 and ee[3 + 8] > 0.0, err
    return q


def make_states(P, kinds, seed):
    """One state per entry of kinds; returns (x [n][3 nq], info): info[i] the known answer of state i where there is one --
    ("hi", s+) or ("window", s-, s+) -- else None."""
    rng = np.random.default_rng(seed)
    O = Oracle(P)
    nq = P.nq
    mu0 = float(P.contact_mu[0])
    mumax = float(np.max(P.contact_mu))
    ez = np.array([0.0, 0.0, 1.0])
    xs, info = [], []
    generic = {}
    for kind in kinds:
        if kind in ("inside", "outside"):
            generic.setdefault(kind, []).append(len(xs))
            xs.append(None); info.append(None)
            continue
        zero = np.zeros(nq)
        if kind == "rest":
            q = tilted_q(P, O, rng)
            xs.append(np.concatenate([q, zero, zero])); info.append(None)
            continue
        ax = np.asarray(P.contact_span)[0][int(rng.integers(2))] * (1.0 if rng.integers(2) else -1.0)
        if kind.startswith("facet"):
            c = float(kind[5:])
            q = tilted_q(P, O, rng)
            Cm = O.ee_kinematics(np.concatenate([q, zero, zero]))[3:12].reshape(3, 3)
            xs.append(R.state_for(O, q, zero, Cm @ (R.G0 * c * mu0 * ax), np.zeros(3)))
            info.append(("hi", 1.0 / np.sqrt(c)))
        elif kind == "liftoff":
            k = rng.uniform(5.0, 8.0)
            q = tilted_q(P, O, rng)
            xs.append(R.state_for(O, q, zero, (k - R.G0) * ez, np.zeros(3)))
            info.append(("hi", np.sqrt(R.G0 / (R.G0 - k))))
        elif kind.startswith("comp") or kind == "aggr":
            sigma = float(kind[4:]) if len(kind) > 4 else 1.0      # the speed at which the load is purely normal
            t = 2.0 * mumax if P.nf == 3 else 0.4
            phi = np.arctan(t)
            row = np.cos(phi) * ez - np.sin(phi) * ax          # the world's vertical in the tray frame
            q = tilted_q(P, O, rng, row[:2])
            Cm = O.ee_kinematics(np.concatenate([q, zero, zero]))[3:12].reshape(3, 3)
            h = (Cm @ ax + np.sin(phi) * ez) / np.cos(phi)     # uphill, horizontal
            assert abs(h[2]) < 1e-12 and abs(np.linalg.norm(h) - 1.0) < 1e-12
            sign = -1.0 if kind == "aggr" else 1.0
            xs.append(R.state_for(O, q, zero, sign * R.G0 * t * h / (sigma * sigma), np.zeros(3)))
            if kind != "aggr" and P.nf == 3 and t * mu0 < 1.0:
                info.append(("window", sigma * np.sqrt((t - mu0) / (t * (1.0 + mu0 * t))),
                             min(S_MAX, sigma * np.sqrt((t + mu0) / (t * (1.0 - mu0 * t))))))
            else:
                info.append(None)
        else:
            raise ValueError(kind)
    for kind, rows in generic.items():
        xg = R.points(P, [kind] * len(rows), seed=seed + (1 if kind == "inside" else 2))
        for r, x in zip(rows, xg):
            xs[r] = x
    return np.stack(xs), info


def kinds_main(P):
    k = ["rest"] * 6 + ["facet0.25"] * 3 + ["facet1.0"] * 3 + ["facet4.0"] * 3 + ["liftoff"] * 10 + ["comp"] * 6 + ["aggr"] * 2
    k += ["comp0.25"] * 3 + ["comp3.0"] * 2 + ["comp4.0"] * 3
    fill = ["inside", "outside"] if P.nf == 3 else ["rest", "liftoff"]
    return k + [fill[i % 2] for i in range(64 - len(k))]


def scenario_set(P):
    """balance_ref.scenarios with the centre of mass moved by 0.4 of the box vertex: at the vertex itself the reference rejects the
    bottle at rest on a level tray, every job of that scenario would be of the class none and each of them costs the 65-point
    grid."""
    scen = R.scenarios(P)
    scen[1] = R.com_shift(np.asarray(P.body_params, dtype=np.float64), [0.008, -0.008, 0.012])
    return scen


def keep_out_vanishing_loads(P, x, kinds, info, thetas):
    """A lift-off state under a scenario that rejects it at rest has b(s) -> 0 at the lift-off speed: the rule rho <= EPS max(|b|, 1)
    accepts a window about 1e-7 wide around it, which the kernel's descent search finds and the 65-point grid of the classifier cannot.
    Such states are replaced by their rest state (DESIGN 3.10 records the finding).  thetas(i): the parameter sets state i meets."""
    nq = P.nq
    for i, kind in enumerate(kinds):
        if kind != "liftoff":
            continue
        x0 = scaled_state(x[i:i + 1], 0.0, nq)
        out = R.reference(P, x0, np.stack(thetas(i)), False)
        if np.any(out["rho"][0] > EPS * np.maximum(out["bnorm"][0], 1.0)):
            x[i], kinds[i], info[i] = x0[0], "rest", None


def build_case(arrangements, name):
    P = R.table_problem(arrangements, name)
    seed = 23 + sum(map(ord, name))
    kinds = kinds_main(P)
    x, info = make_states(P, kinds, seed)
    scen = scenario_set(P)
    keep_out_vanishing_loads(P, x, kinds, info, lambda i: scen)
    launches = [dict(P=P, x=x, params=scen, per_point=False, kinds=kinds, info=info)]                                               # 64 x 4 = 256
    # (no aggr and no comp0.25 state among the first seven, which meet 37 scenarios each: a job of the class none costs the reference
    #  the 65-point grid, and so does nearly a window far from the middle of the range)
    k2 = (["rest", "liftoff", "facet4.0", "comp", "liftoff", "comp4.0", "facet1.0", "comp0.25", "aggr"] * 5)[:37]
    x2, info2 = make_states(P, k2, seed + 5)
    keep_out_vanishing_loads(P, x2, k2, info2, lambda i: scen)
    per = np.stack([scen[(np.arange(37) + i) % 4] for i in range(7)])
    launches.append(dict(P=P, x=x2[:7], params=per, per_point=True, kinds=k2[:7], info=info2[:7]))                                   # 7 x 37 = 259
    launches.append(dict(P=P, x=x2, params=scen[1:2], per_point=False, kinds=k2, info=info2))                                        # 37 x 1
    launches.append(dict(P=P, x=x2, params=np.stack([scen[i % 4:i % 4 + 1] for i in range(37)]), per_point=True, kinds=k2, info=info2))   # 37 x 1
    launches.append(dict(P=P, x=x[16:17], params=scen[:1], per_point=False, kinds=kinds[16:17], info=info[16:17]))                   # 1 x 1
    launches.append(dict(P=P, x=x[26:27], params=scen[None, 1:2], per_point=True, kinds=kinds[26:27], info=info[26:27]))             # 1 x 1
    return launches


# ---- the reference -------------------------------------------------------------------------------------------------------------------
class Jobs:
    """The jobs of one launch with a memo of reference evaluations: ref(i, sc, s) -> dict(rho, bnorm, b, A, z)."""

    def __init__(self, L, s_max=S_MAX):
        self.L, self.P, self.s_max = L, L["P"], s_max
        self.x = np.asarray(L["x"]).reshape(-1, 3 * self.P.nq)
        self.params = np.asarray(L["params"], dtype=np.float64)
        self.per_point = L["per_point"]
        self.n = self.x.shape[0]
        self.ns = self.params.shape[1] if self.per_point else self.params.shape[0]
        self._memo = {}

    def theta(self, i, sc):
        return self.params[i, sc] if self.per_point else self.params[sc]

    def ref(self, i, sc, s):
        key = (i, sc, float(s))
        if key not in self._memo:
            out = R.reference(self.P, scaled_state(self.x[i:i + 1], float(s), self.P.nq), self.theta(i, sc)[None], False)
            self._memo[key] = dict(rho=float(out["rho"][0, 0]), bnorm=float(out["bnorm"][0, 0]), b=out["b"][0, 0], A=out["A"][0, 0], z=out["z"][0, 0])
        return self._memo[key]

    def accepted(self, i, sc, s):
        e = self.ref(i, sc, s)
        return e["rho"] <= EPS * max(e["bnorm"], 1.0)

    def near(self, i, sc, s):
        """|rho_ref - EPS s| / s at one evaluation: how far the decision is from the boundary"""
        e = self.ref(i, sc, s)
        sc_ = max(e["bnorm"], 1.0)
        return abs(e["rho"] - EPS * sc_) / sc_

    def classify(self, i, sc):
        e0, eM = self.accepted(i, sc, 0.0), self.accepted(i, sc, self.s_max)
        if e0:
            if eM:
                return "all"
            if not self.accepted(i, sc, 1.0 - 1e-3):
                return "upper_lt1"
            return "upper_gt1" if self.accepted(i, sc, 1.0 + 1e-3) else "upper_one"
        if eM or self.accepted(i, sc, 1.0 - 1e-3) or self.accepted(i, sc, 1.0 + 1e-3):
            return "window"
        # (the grid from its middle outwards: the same 65 points, the wide windows found early)
        grid = np.linspace(0.0, self.s_max, GRID)
        return "window" if any(self.accepted(i, sc, s) for s in grid[np.argsort(np.abs(grid - 0.5 * self.s_max), kind="stable")]) else "none"

    def classes(self):
        if "sclass" not in self.L:
            self.L["sclass"] = np.array([[self.classify(i, sc) for sc in range(self.ns)] for i in range(self.n)])
        return self.L["sclass"]

    def slope(self, i, sc, s):
        """g = r' (b1 - b0) with r = b + A z of the reference at s, b0 and b1 the oracle's b at rest and at s = 1"""
        e = self.ref(i, sc, s)
        return float((e["b"] + e["A"] @ e["z"]) @ (self.ref(i, sc, 1.0)["b"] - self.ref(i, sc, 0.0)["b"]))

    def slope_cos(self, i, sc, s):
        """the slope as a cosine, g / (|r| |b1 - b0|): how far its sign is from undecided"""
        e = self.ref(i, sc, s)
        d = self.ref(i, sc, 1.0)["b"] - self.ref(i, sc, 0.0)["b"]
        return self.slope(i, sc, s) / max(np.linalg.norm(e["b"] + e["A"] @ e["z"]) * np.linalg.norm(d), 1e-300)

    def replay(self, i, sc, flip=False, trace=None):
        """upr_spd_ctl of upr_speed.h on rho_ref: (speed[4], evaluations).  flip: the descent search with the sign of the slope
        inverted (what a wrong sign in the kernel would compute); trace: a list that receives (s, |cosine of the slope|, distance of
        the decision from the boundary) of every rejected midpoint of the descent search."""
        s_max = self.s_max
        F = lambda k: self.accepted(i, sc, at(k, s_max))   # noqa: E731
        n_ev = 2
        e0, eM = F(0), F(K)
        lo_in, lo_out, hi_in, hi_out = 0, 0, (K if eM else 0), K
        if not e0:
            k1 = int(float(K) / s_max)
            seed = None
            if k1 > 0:
                n_ev += 1
                if F(k1):
                    seed = k1
            if seed is None and eM:
                seed = K
            if seed is None:
                dl, dh = 0, K
                for _ in range(BISECT):
                    mid = (dl + dh) >> 1
                    n_ev += 1
                    if F(mid):
                        seed = mid
                        break
                    if trace is not None:
                        trace.append((at(mid, s_max), abs(self.slope_cos(i, sc, at(mid, s_max))), self.near(i, sc, at(mid, s_max))))
                    if (self.slope(i, sc, at(mid, s_max)) < 0.0) != flip:
                        dl = mid
                    else:
                        dh = mid
                    if dh - dl <= 1:
                        break
            if seed is None:
                return np.array([np.inf, 0.0, -np.inf, s_max]), n_ev
            lo_in = seed
            if not eM:
                hi_in = seed
            while lo_in - lo_out > 1:
                mid = (lo_in + lo_out) >> 1
                n_ev += 1
                if F(mid):
                    lo_in = mid
                else:
                    lo_out = mid
        while not eM and hi_out - hi_in > 1:
            mid = (hi_in + hi_out) >> 1
            n_ev += 1
            if F(mid):
                hi_in = mid
            else:
                hi_out = mid
        return np.array([at(lo_in, s_max), 0.0 if e0 else at(lo_out, s_max), at(hi_in, s_max), np.inf if eM else at(hi_out, s_max)]), n_ev


def device_class(speed, s_max=S_MAX):
    """The class a returned speed[..., 4] stands for (the windows of the upper classes are the classifier's)."""
    lo, lo_out, hi, hi_out = (speed[..., k] for k in range(4))
    out = np.full(lo.shape, "window", dtype="<U9")
    rest = (lo == 0.0) & (lo_out == 0.0)
    out[rest] = "upper_one"
    out[rest & (hi_out <= 1.0 - 1e-3)] = "upper_lt1"
    out[rest & (hi >= 1.0 + 1e-3)] = "upper_gt1"
    out[rest & (hi == s_max) & np.isinf(hi_out)] = "all"
    out[np.isinf(lo)] = "none"
    return out


# ---- the kernel source through the host emulation -----------------------------------------------------------------------------------
def emu_lib(fma=False):
    import ctypes as C
    import os
    from pathlib import Path

    name = "libupr_speed_emu_fma.so" if fma else "libupr_speed_emu.so"
    return C.CDLL(os.environ.get("UPR_SPEED_EMU_FMA_LIB" if fma else "UPR_SPEED_EMU_LIB", str(Path(__file__).resolve().parent / "emu" / name)))


def have_fma_twin():
    """Whether the host has the FMA instruction (/proc/cpuinfo, as the build decides): the twin library must then exist."""
    from pathlib import Path

    try:
        has_fma = " fma " in Path("/proc/cpuinfo").read_text().replace("\n", " ")
    except OSError:
        has_fma = False
    if has_fma:
        assert (Path(__file__).resolve().parent / "emu" / "libupr_speed_emu_fma.so").exists(), "the host has FMA but libupr_speed_emu_fma.so was not built"
    return has_fma


def run_emu(P, x, params, per_point, s_max=S_MAX, form=-1, fma=False):
    """dict(speed (n, ns, 4), z (n, ns, 2, ncol), y (n, ns, 2, 6 nb), iters (n, ns)) of the speed-margin job compiled for the host;
    form as balance_ref.run_emu; fma: the twin built with -mfma -ffp-contract=fast."""
    import ctypes as C

    from upright_amd import _capi

    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3 * P.nq)
    params = np.ascontiguousarray(params, dtype=np.float64)
    n, ns = x.shape[0], (params.shape[1] if per_point else params.shape[0])
    out = dict(speed=np.full((n, ns, 4), np.nan), z=np.full((n, ns, 2, R.ncol(P)), np.nan), y=np.full((n, ns, 2, 6 * P.nb), np.nan),
               iters=np.full((n, ns), -1, dtype=np.int32))
    cp = _capi.problem_to_c(P)
    rc = emu_lib(fma).emu_spd_points(C.byref(cp), n, _capi.ptr(x), ns, _capi.ptr(params), 1 if per_point else 0, C.c_double(s_max),
                                     _capi.ptr(out["speed"]), _capi.ptr(out["z"]), _capi.ptr(out["y"]), _capi.iptr(out["iters"]), int(form))
    assert rc == 0
    return out


def emu_rhs(P, x, theta, s):
    """b [n][6 nb] as a job builds it: the state point, the record scaled by s, the rhs routine"""
    import ctypes as C

    from upright_amd import _capi

    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3 * P.nq)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    b = np.full((x.shape[0], 6 * P.nb), np.nan)
    cp = _capi.problem_to_c(P)
    assert emu_lib().emu_spd_rhs(C.byref(cp), x.shape[0], _capi.ptr(x), _capi.ptr(theta), C.c_double(s), _capi.ptr(b)) == 0
    return b


def emu_plan(P, speed, xs, us):
    """(window, knot, limit) of the plan reductions compiled for the host: speed (B, nk, ns, 4), xs (B, nk, nx), us (B, nk - 1, nu)"""
    import ctypes as C

    from upright_amd import _capi

    speed, xs, us = (np.ascontiguousarray(a, dtype=np.float64) for a in (speed, xs, us))
    B, nk, ns = speed.shape[:3]
    w, kn, lim = np.full((B, ns, 2), np.nan), np.full((B, ns, 2), -1, dtype=np.int32), np.full(B, np.nan)
    cp = _capi.problem_to_c(P)
    assert emu_lib().emu_spd_plan(C.byref(cp), B, nk, ns, _capi.ptr(speed), xs.shape[2], us.shape[2], _capi.ptr(xs), _capi.ptr(us), _capi.ptr(w),
                                  _capi.iptr(kn), _capi.ptr(lim)) == 0
    return w, kn, lim


def numpy_plan(P, speed, xs, us):
    """The same reductions in numpy: max / min / first argmax over the knots; the limit speed from the boxes of the problem."""
    w = np.stack([speed[..., 0].max(axis=1), speed[..., 2].min(axis=1)], axis=-1)
    kn = np.stack([speed[..., 0].argmax(axis=1), speed[..., 2].argmin(axis=1)], axis=-1).astype(np.int32)
    nq = P.nq
    x_lb, x_ub, u_lb, u_ub = (np.asarray(a, dtype=np.float64) for a in (P.x_lb, P.x_ub, P.u_lb, P.u_ub))

    def lim(v, lb, ub, p):
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(v > 0, ub / v, lb / v)
        q = np.where(v == 0, np.inf, np.maximum(q, 0.0))
        return (q ** (1.0 / p)).reshape(v.shape[0], -1).min(axis=1)

    limit = np.minimum(np.minimum(lim(xs[..., nq:2 * nq], x_lb[nq:2 * nq], x_ub[nq:2 * nq], 1), lim(xs[..., 2 * nq:3 * nq], x_lb[2 * nq:3 * nq], x_ub[2 * nq:3 * nq], 2)),
                       lim(us[..., :nq], u_lb[:nq], u_ub[:nq], 3))
    return w, kn, limit


_CASES = {}


def cases(arrangements, name):
    """build_case(name), each launch with its Jobs (key "jobs"), its classes on the reference (key "sclass") and the emulation's
    answer (key "emu"); computed once per session, shared by the tests, modified by none."""
    if name not in _CASES:
        launches = build_case(arrangements, name)
        for L in launches:
            L["jobs"] = Jobs(L)
            L["jobs"].classes()
            L["emu"] = run_emu(L["P"], L["x"], L["params"], L["per_point"])
        _CASES[name] = launches
    return _CASES[name]


def class_counts(launches):
    allc = np.concatenate([L["sclass"].ravel() for L in launches])
    return {c: int((allc == c).sum()) for c in CLASSES}


# the arrangements on which sliding on the facet of contact 0 binds before anything else, confirmed on the reference (the facet states
# have s+ = 1 / sqrt(c) and the compensated tilt its closed-form window there, in the scenarios FACET_SCENARIOS).  Not among them:
# foam_die2 -- the stack of two dice tips at 0.693 mu0 g, before it slides (facet states with c = 1 have s+ = 0.8325 on the reference);
# fixture_box -- a push towards a wall of the fixture is held by the wall; the shapes without friction.
SLIDING_BINDS = ("pink_bottle", "pink_bottle_arm", "bottle_20_contacts", "box_arch", "blue_cups")


def expected_classes(P, name=""):
    """The classes an arrangement of the table holds at least five jobs of.  upper_one needs a state whose upper end is the nominal
    speed: the facet states with c = 1 where sliding binds.  Without friction (nf = 1) a load is balanced only where it is purely
    normal: the facet states are rejected as soon as they move (upper_lt1), so upper_one does not occur; on foam_die2 the stack tips
    before it slides and the c = 1 states end at 0.8325 (upper_lt1)."""
    return ("all", "upper_lt1", "upper_gt1", "window", "none") + (("upper_one",) if P.nf == 3 and name != "foam_die2" else ())


SLOPE_MIN = 1e-6     # a descent step counts as decided when |g| >= SLOPE_MIN |r| |b1 - b0| on the reference


def steady(L):
    """Jobs that bisect no end and whose decisions are decided on the reference: evaluation and iteration counts are compared on
    them.  The class all: two evaluations, both 1e-9 max(|b|, 1) away from the boundary.  The class none: rest, s_max, the nominal
    point and every midpoint of the descent search 1e-9 max(|b|, 1) away from the boundary, and the slope of every midpoint at least
    SLOPE_MIN |r| |b1 - b0| away from zero -- a search that closes in on an interior minimiser of rho ends on slopes that vanish,
    where the last bit decides which neighbour is evaluated next; the aggravated tilt, whose rho grows with the speed all the way,
    stays decided."""
    if "steady" not in L:
        J = L["jobs"]
        m = np.isin(L["sclass"], ("all", "none"))
        for i, sc in np.argwhere(m):
            i, sc = int(i), int(sc)
            ok = J.near(i, sc, 0.0) > RHO_TOL and J.near(i, sc, J.s_max) > RHO_TOL
            if ok and L["sclass"][i, sc] == "none":
                tr = []
                J.replay(i, sc, trace=tr)
                ok = J.near(i, sc, at(int(float(K) / J.s_max), J.s_max)) > RHO_TOL and all(c >= SLOPE_MIN and n > RHO_TOL for _, c, n in tr)
            m[i, sc] = ok
        L["steady"] = m
    return L["steady"]


# ---- the assertions both test files make on an answer (emulation or device) ---------------------------------------------------------
def check_answer(L, out, s_max=S_MAX):
    """The conventions, the bracket, both certificates at both ends on the oracle's b and A (no solver), rho_ref at every in and out,
    the class.  out: dict(speed, z, y, iters).  Returns the list of violations (check, i, sc, class, figure in units of max(|b|, 1))."""
    J = L["jobs"]
    P = J.P
    sp, z, y, it = out["speed"], out["z"], out["y"], out["iters"]
    assert sp.shape == (J.n, J.ns, 4) and not np.any(np.isnan(sp))
    cls = L["sclass"]
    got = device_class(sp, s_max)
    assert np.array_equal(got, cls), [(i, sc, sp[i, sc], cls[i, sc]) for i, sc in np.argwhere(got != cls)[:5]]
    assert it.min() >= 0 and it.max() <= (3 + 3 * BISECT) * 3 * R.ncol(P)
    tol_col = R.emu_lib().emu_bal_tol()
    step = s_max * 2.0 ** -BISECT
    bad = []
    for i in range(J.n):
        for sc in range(J.ns):
            c = cls[i, sc]
            lo, lo_out, hi, hi_out = sp[i, sc]
            if c == "none":
                assert lo == np.inf and lo_out == 0.0 and hi == -np.inf and hi_out == s_max
                assert not z[i, sc].any()
            else:
                assert 0.0 <= lo <= hi <= s_max
            if c == "all":
                assert (lo, lo_out, hi, hi_out) == (0.0, 0.0, s_max, np.inf) and not y[i, sc].any()
            if c.startswith("upper"):
                assert lo == 0.0 and lo_out == 0.0 and not y[i, sc, 0].any()
                assert hi_out - hi == step, (i, sc, hi, hi_out)                                                  # the bracket, exact
            if c == "window":
                assert lo - lo_out == step, (i, sc, lo, lo_out)
                assert (hi == s_max and hi_out == np.inf) or hi_out - hi == step, (i, sc, hi, hi_out)
            for e, s_in, s_out in ((0, lo, lo_out), (1, hi, hi_out)):
                if np.isfinite(s_in):                                                                           # accepted end
                    r = J.ref(i, sc, s_in)
                    s1 = max(r["bnorm"], 1.0)
                    res = np.linalg.norm(r["b"] + r["A"] @ z[i, sc, e])
                    if not z[i, sc, e].min() >= 0.0: bad.append(("z >= 0", i, sc, c, e, z[i, sc, e].min()))
                    if not res <= (EPS + RHO_TOL) * s1: bad.append(("|b + A z|", i, sc, c, e, res / s1))
                    if not r["rho"] <= (EPS + RHO_TOL) * s1: bad.append(("rho_ref(in)", i, sc, c, e, r["rho"] / s1))
                rejected = (c in ("window", "none") and e == 0) or (np.isfinite(s_out) and e == 1)
                if rejected:                                                                                    # rejected end
                    r = J.ref(i, sc, s_out)
                    s1 = max(r["bnorm"], 1.0)
                    yy = y[i, sc, e]
                    w = (r["A"].T @ yy) / (np.linalg.norm(r["A"], axis=0) * s1)
                    if not np.all(w >= -10.0 * tol_col): bad.append(("a_j' y", i, sc, c, e, w.min()))
                    sep = yy @ r["b"] / np.linalg.norm(yy)
                    if not sep >= (EPS - RHO_TOL) * s1: bad.append(("y' b / |y|", i, sc, c, e, sep / s1))
                    if not r["rho"] >= (EPS - RHO_TOL) * s1: bad.append(("rho_ref(out)", i, sc, c, e, r["rho"] / s1))
    return bad


def known_answers(L, speed, scenarios=R.FACET_SCENARIOS):
    """Largest |s - s_known| over the states of a launch with shared scenarios that carry a known answer, per kind: dict(facet,
    liftoff, window).  Facets and windows in the scenarios that keep sliding the binding mode (a moved centre of mass tips the
    bottle first), lift-off in every scenario."""
    worst = dict(facet=0.0, liftoff=0.0, window=0.0)
    for i, (kind, inf) in enumerate(zip(L["kinds"], L["info"])):
        if inf is None:
            continue
        if kind == "liftoff":
            worst["liftoff"] = max(worst["liftoff"], float(np.abs(speed[i, :, 2] - inf[1]).max()))
        elif kind.startswith("facet"):
            worst["facet"] = max(worst["facet"], float(np.abs(speed[i, list(scenarios), 2] - inf[1]).max()))
        elif kind.startswith("comp"):
            d = np.abs(speed[i, list(scenarios)][:, [0, 2]] - np.array(inf[1:]))
            worst["window"] = max(worst["window"], float(d.max()))
    return worst
