"""CPU reference of the batched path-acceleration margin (upright_amd/csrc/upr_pathacc.h), its case table and the assertions its CPU
and GPU tests share.

rho_ref(d) of a job is balance_ref.reference at the JOINT-SPACE state x(s0, d) = (q, s0 v, s0^2 a + d v): the oracle's b and A there,
the smallest of the three CPU residuals.  Nothing of the kernel's record transform (C_we, s0 omega, s0^2 alpha + d omega, s0^2 a_ee +
d v_ee) or of b(d) = b(0) + d b2 is in it.  d is accepted when rho_ref <= EPS max(|b|, 1).  The class of a job comes from the reference
alone: its values at -d_max, 0 and +d_max, plus a 65-point grid of [-d_max, d_max] for the emptiness decision:
    all       -d_max and +d_max both accepted;
    hi        -d_max accepted, +d_max not: an upper end (hi_in: 0 accepted, hi_out: 0 rejected -- balanced only while braking);
    lo        the mirror (lo_in, lo_out);
    both      both ends rejected, 0 accepted;
    window    both ends and 0 rejected, something accepted;
    none      nothing accepted (the grid and the three points).
Jobs.replay is the algorithm of upr_speed.h (upr_spd_ctl, transcribed, nominal point 2^31) on rho_ref.

The states (make_states).  All on a tray levelled or pitched to rounding by speed_ref.tilted_q; the joint velocity is the least-norm
solution of [J_v; J_omega] v = [v_ee; 0] on the oracle's Jacobian, the joint acceleration comes from balance_ref.state_for:
    rest          v = 0: x(s0, d) does not depend on d -- all under the scenarios that hold it, none otherwise, two evaluations;
    slide w       level tray, a_ee = alpha = 0, v_ee = w (C_we pyramid axis of contact 0): d_hi = -d_lo = mu0 g0 / w where sliding binds;
    lift          level tray, a_ee = alpha = 0, v_ee = w e_z, w in [1.5, 3]: d_lo = -g0 / w on every shape, d_hi open (lo_in);
    sink          the same with v_ee = -w e_z: d_hi = g0 / w, d_lo open (hi_in; the mirror the class table needs);
    falling       v_ee = -w e_z, a_ee = -(g0 + k) e_z, k in [1, 3]: rejected at 0, accepted below d = -k / w (hi_out);
    rising        v_ee = +w e_z, a_ee = -(g0 + k) e_z: accepted above d = k / w (lo_out);
    comp sigma    the tray pitched by phi, tan phi = t = 2 mu_max, about a pyramid axis; a = 0; v_ee = w h, h uphill-horizontal, w = 2
                  sigma: where sliding binds the window d w / g0 in [(t - mu0) / (1 + mu0 t), (t + mu0) / (1 - mu0 t)], which excludes 0
                  and both ends -- only the descent search seeds it, sigma = 1 after one decided slope step, sigma = 4 after three;
                  "compd": the same downhill, the mirrored window;
    aggr          the pitched tray with v_ee across the slope: nothing balances it (rho is even in d: the slope of the descent search
                  vanishes at d = 0 and its sign there is rounding, so the solve counts of these jobs are not compared);
    steep         the pitched tray pushed downhill by a_ee = -g0 t h, moving uphill at w = 0.5: purely normal only at d = 4 g0 t, the
                  window lies above d_max = 8 -- none, with every slope of the descent search decided (it walks up to d_max): the none
                  jobs whose solve counts are compared;
    inside        the generic kind of balance_ref.points (a random joint velocity of norm <= 0.45), friction shapes only; its `outside`
                  kind is understood by make_states but not in the table: nearly every such job is a none job in motion.
With s0 != 1 the states keep their construction and the known answers follow from a_ee(s0, d) = s0^2 a_ee + d v_ee (known() below).
Without friction (nf = 1) the compensated tilt is balanced at one d alone, where the rule's ball accepts a sliver about 1e-7 wide that the
kernel's descent search finds and the 65-point grid cannot (the finding of DESIGN 3.10 again): the table of those shapes holds none.  A lift / sink / falling / rising state under a scenario that rejects it at rest has b(d) -> 0 at free fall, where the
rule's ball accepts a sliver the grid cannot see: such states are replaced by their rest state."""
import numpy as np

import balance_ref as R
import speed_ref as S
from oracle.oracle import Oracle
from speed_ref import SLIDING_BINDS, scenario_set, tilted_q  # noqa: F401
from balance_ref import state_for, table_problem  # noqa: F401

EPS = S.EPS
BISECT = S.BISECT
K = S.K
HALF = K >> 1
D_MAX = 8.0
RHO_TOL = S.RHO_TOL
GRID = 65
NAMES = S.NAMES
ONE_BODY = S.ONE_BODY
CLASSES = ("all", "hi_in", "hi_out", "lo_in", "lo_out", "both", "window", "none")
VERTICAL = ("lift", "sink", "falling", "rising")


def path_state(x, s0, d, nq):
    """x(s0, d) = (q, s0 v, s0^2 a + d v)"""
    x = np.array(x, dtype=np.float64)
    v = x[..., nq:2 * nq].copy()
    x[..., nq:2 * nq] = s0 * v
    x[..., 2 * nq:3 * nq] = s0 * s0 * x[..., 2 * nq:3 * nq] + d * v
    return x


def at(k, d_max=D_MAX):
    return d_max * (float(int(k) - HALF) * 2.0 ** -(BISECT - 1))


# ---- states ---------------------------------------------------------------------------------------------------------------------------
def velocity_for(O, q, v_ee):
    """the least-norm joint velocity with the end effector's linear velocity v_ee and no angular velocity"""
    nq = q.size
    _, dee = O.ee_kinematics(np.concatenate([q, np.zeros(2 * nq)]), jac=True)
    J = np.concatenate([dee[12:15, nq:2 * nq], dee[15:18, nq:2 * nq]])
    return np.linalg.lstsq(J, np.concatenate([np.asarray(v_ee, dtype=np.float64), np.zeros(3)]), rcond=None)[0]


def make_states(P, kinds, seed):
    """One state per entry of kinds; returns (x [n][3 nq], info): info[i] describes the known answer of state i at speed 1 as (what,
    value ...) for known(), or None."""
    rng = np.random.default_rng(seed)
    O = Oracle(P)
    nq = P.nq
    mu0 = float(P.contact_mu[0])
    mumax = float(np.max(P.contact_mu))
    ez = np.array([0.0, 0.0, 1.0])
    zero = np.zeros(nq)
    xs, info = [], []
    generic = {}
    for kind in kinds:
        if kind in ("inside", "outside"):
            generic.setdefault(kind, []).append(len(xs))
            xs.append(None); info.append(None)
            continue
        if kind == "rest":
            xs.append(np.concatenate([tilted_q(P, O, rng), zero, zero])); info.append(None)
            continue
        ax = np.asarray(P.contact_span)[0][int(rng.integers(2))] * (1.0 if rng.integers(2) else -1.0)
        if kind.startswith("slide"):
            w = float(kind[5:])
            q = tilted_q(P, O, rng)
            Cm = O.ee_kinematics(np.concatenate([q, zero, zero]))[3:12].reshape(3, 3)
            xs.append(state_for(O, q, velocity_for(O, q, w * (Cm @ ax)), np.zeros(3), np.zeros(3)))
            info.append(("slide", w))
        elif kind in VERTICAL:
            w = rng.uniform(1.5, 3.0)
            k = rng.uniform(1.0, 3.0)
            q = tilted_q(P, O, rng)
            sv = 1.0 if kind in ("lift", "rising") else -1.0
            a = np.zeros(3) if kind in ("lift", "sink") else -(R.G0 + k) * ez
            xs.append(state_for(O, q, velocity_for(O, q, sv * w * ez), a, np.zeros(3)))
            info.append((kind, w, k))
        elif kind.startswith("comp") or kind in ("aggr", "steep"):
            down = kind.startswith("compd")
            sigma = 1.0 if kind == "aggr" else 0.25 if kind == "steep" else float(kind[5:] if down else kind[4:])
            w = 2.0 * sigma
            t = 2.0 * mumax if P.nf == 3 else 0.4
            phi = np.arctan(t)
            row = np.cos(phi) * ez - np.sin(phi) * ax          # the world's vertical in the tray frame
            q = tilted_q(P, O, rng, row[:2])
            Cm = O.ee_kinematics(np.concatenate([q, zero, zero]))[3:12].reshape(3, 3)
            h = (Cm @ ax + np.sin(phi) * ez) / np.cos(phi)     # uphill, horizontal
            assert abs(h[2]) < 1e-12 and abs(np.linalg.norm(h) - 1.0) < 1e-12
            a_ee = np.zeros(3)
            if kind == "aggr":
                vdir = np.cross(ez, h)                         # across the slope
                info.append(None)
            elif kind == "steep":
                vdir, a_ee = h, -R.G0 * t * h
                info.append(None)
            else:
                vdir = -h if down else h
                info.append(("comp", w, t, -1.0 if down else 1.0) if (P.nf == 3 and t * mu0 < 1.0) else None)
            xs.append(state_for(O, q, velocity_for(O, q, w * vdir), a_ee, np.zeros(3)))
        else:
            raise ValueError(kind)
    for kind, rows in generic.items():
        xg = R.points(P, [kind] * len(rows), seed=seed + (1 if kind == "inside" else 2))
        for r, x in zip(rows, xg):
            xs[r] = x
    return np.stack(xs), info


def known(P, inf, s0=1.0, d_max=D_MAX):
    """(d_lo, d_hi) of a state with a known answer at speed s0; None where an end is not given in closed form (open ends are +-d_max)."""
    mu0 = float(P.contact_mu[0])
    what = inf[0]
    clip = lambda v: float(np.clip(v, -d_max, d_max))   # noqa: E731
    w = inf[1]                                           # a_ee(s0, d) = s0^2 a_ee + d v_ee: d multiplies the plan's own velocity
    if what == "slide":
        e = mu0 * R.G0 / w
        return clip(-e), clip(e)
    if what == "lift":
        return clip(-R.G0 / w), d_max
    if what == "sink":
        return -d_max, clip(R.G0 / w)
    edge = (s0 * s0 * (R.G0 + inf[2]) - R.G0) / w if what in ("falling", "rising") else 0.0   # -s0^2 (g0 + k) -+ d w >= -g0
    if what == "falling":
        return -d_max, clip(-edge)
    if what == "rising":
        return clip(edge), d_max
    if what == "comp":
        t, sgn = inf[2], inf[3]
        lo, hi = R.G0 * (t - mu0) / (1.0 + mu0 * t) / w, R.G0 * (t + mu0) / (1.0 - mu0 * t) / w
        return (clip(lo), clip(hi)) if sgn > 0 else (clip(-hi), clip(-lo))
    raise ValueError(what)


def kinds_main(P):
    if P.nf == 3:
        k = ["rest"] * 4 + ["slide0.5"] * 4 + ["slide1.0"] * 4 + ["lift"] * 6 + ["sink"] * 6 + ["falling"] * 6 + ["rising"] * 6
        k += ["comp1.0"] * 4 + ["comp4.0"] * 4 + ["compd1.0"] * 3 + ["compd4.0"] * 3 + ["steep"] * 2
        return k + ["inside"] * (64 - len(k))
    # without friction a load is balanced only where it is purely normal: no compensated tilt (the module's docstring), and the generic
    # kinds are balanced nowhere
    k = ["rest"] * 6 + ["slide0.5"] * 6 + ["slide1.0"] * 6 + ["lift"] * 11 + ["sink"] * 11 + ["falling"] * 11 + ["rising"] * 11 + ["steep", "steep"]
    return k


K2 = {3: ["rest", "lift", "falling", "comp1.0", "sink", "slide0.5", "rising", "comp4.0", "compd1.0", "slide1.0", "compd4.0", "aggr"],
      1: ["rest", "lift", "falling", "slide1.0", "sink", "slide0.5", "rising", "lift", "sink", "falling", "rising", "aggr"]}


def kinds_second(P):
    base = K2[P.nf]
    k = (base * 4)[:37]
    # (one aggr state: a none job costs the reference its grid)
    return [((base[3] if P.nf == 3 else "rest") if (kind == "aggr" and i > 11) else kind) for i, kind in enumerate(k)]


def keep_out_vanishing_loads(P, x, kinds, info, thetas):
    """speed_ref.keep_out_vanishing_loads for the vertical kinds of this table."""
    nq = P.nq
    for i, kind in enumerate(kinds):
        if kind not in VERTICAL:
            continue
        x0 = np.concatenate([x[i, :nq], np.zeros(2 * nq)])
        out = R.reference(P, x0[None], np.stack(thetas(i)), False)
        if np.any(out["rho"][0] > EPS * np.maximum(out["bnorm"][0], 1.0)):
            x[i], kinds[i], info[i] = x0, "rest", None


def build_case(arrangements, name):
    P = table_problem(arrangements, name)
    seed = 41 + sum(map(ord, name))
    kinds = kinds_main(P)
    x, info = make_states(P, kinds, seed)
    scen = scenario_set(P)
    keep_out_vanishing_loads(P, x, kinds, info, lambda i: scen)
    L = lambda **kw: dict(P=P, d_max=D_MAX, speed=1.0, **kw)   # noqa: E731
    launches = [L(x=x, params=scen, per_point=False, kinds=kinds, info=info)]                                                       # 64 x 4 = 256
    k2 = kinds_second(P)
    x2, info2 = make_states(P, k2, seed + 5)
    keep_out_vanishing_loads(P, x2, k2, info2, lambda i: scen)
    per = np.stack([scen[(np.arange(37) + i) % 4] for i in range(7)])
    launches.append(L(x=x2[:7], params=per, per_point=True, kinds=k2[:7], info=info2[:7]))                                           # 7 x 37 = 259
    launches.append(L(x=x2, params=scen[0:1], per_point=False, kinds=k2, info=info2))                                                # 37 x 1
    launches.append(L(x=x2, params=np.stack([scen[i % 4:i % 4 + 1] for i in range(37)]), per_point=True, kinds=k2, info=info2))       # 37 x 1
    launches.append(L(x=x[5:6], params=scen[:1], per_point=False, kinds=kinds[5:6], info=info[5:6]))                                 # 1 x 1
    launches.append(L(x=x[13:14], params=scen[None, 3:4], per_point=True, kinds=kinds[13:14], info=info[13:14]))                     # 1 x 1
    slow = dict(launches[2])                                                                                                         # 37 x 1
    slow.update(d_max=3.0, speed=0.5)
    launches.append(slow)
    return launches


# ---- the reference -------------------------------------------------------------------------------------------------------------------
class Jobs:
    """The jobs of one launch with a memo of reference evaluations: ref(i, sc, d) -> dict(rho, bnorm, b, A, z)."""

    def __init__(self, L):
        self.L, self.P, self.d_max, self.s0 = L, L["P"], float(L["d_max"]), float(L["speed"])
        self.x = np.asarray(L["x"]).reshape(-1, 3 * self.P.nq)
        self.params = np.asarray(L["params"], dtype=np.float64)
        self.per_point = L["per_point"]
        self.n = self.x.shape[0]
        self.ns = self.params.shape[1] if self.per_point else self.params.shape[0]
        nq = self.P.nq
        self.moving = np.any(self.x[:, nq:2 * nq] != 0.0, axis=1)   # (v = 0: x(s0, d) is one state whatever d)
        self._memo = {}

    def theta(self, i, sc):
        return self.params[i, sc] if self.per_point else self.params[sc]

    def ref(self, i, sc, d):
        key = (i, sc, float(d) if self.moving[i] else 0.0)
        if key not in self._memo:
            out = R.reference(self.P, path_state(self.x[i:i + 1], self.s0, key[2], self.P.nq), self.theta(i, sc)[None], False)
            self._memo[key] = dict(rho=float(out["rho"][0, 0]), bnorm=float(out["bnorm"][0, 0]), b=out["b"][0, 0], A=out["A"][0, 0], z=out["z"][0, 0])
        return self._memo[key]

    def accepted(self, i, sc, d):
        e = self.ref(i, sc, d)
        return e["rho"] <= EPS * max(e["bnorm"], 1.0)

    def near(self, i, sc, d):
        e = self.ref(i, sc, d)
        s1 = max(e["bnorm"], 1.0)
        return abs(e["rho"] - EPS * s1) / s1

    def grid(self):
        g = np.linspace(-self.d_max, self.d_max, GRID)
        return g[np.argsort(np.abs(g), kind="stable")]   # (from the middle outwards)

    def classify(self, i, sc):
        lo, mid, hi = self.accepted(i, sc, -self.d_max), self.accepted(i, sc, 0.0), self.accepted(i, sc, self.d_max)
        if lo and hi:
            return "all"
        if lo:
            return "hi_in" if mid else "hi_out"
        if hi:
            return "lo_in" if mid else "lo_out"
        if mid:
            return "both"
        return "window" if any(self.accepted(i, sc, d) for d in self.grid()) else "none"

    def classes(self):
        if "pclass" not in self.L:
            self.L["pclass"] = np.array([[self.classify(i, sc) for sc in range(self.ns)] for i in range(self.n)])
        return self.L["pclass"]

    def b2(self, i, sc):
        return self.ref(i, sc, 1.0)["b"] - self.ref(i, sc, 0.0)["b"]

    def slope(self, i, sc, d):
        """g = r' b2 with r = b + A z of the reference at d, b2 the oracle's b at d = 1 minus the one at d = 0"""
        e = self.ref(i, sc, d)
        return float((e["b"] + e["A"] @ e["z"]) @ self.b2(i, sc))

    def slope_cos(self, i, sc, d):
        e = self.ref(i, sc, d)
        return self.slope(i, sc, d) / max(np.linalg.norm(e["b"] + e["A"] @ e["z"]) * np.linalg.norm(self.b2(i, sc)), 1e-300)

    def replay(self, i, sc, flip=False, trace=None):
        """upr_spd_ctl of upr_speed.h with the nominal point 2^31 on rho_ref: (accel[4], evaluations).  flip: the descent search with
        the sign of the slope inverted; trace: receives (d, |cosine of the slope|, distance of the decision from the boundary) of every
        rejected midpoint of the descent search."""
        dm = self.d_max
        F = lambda k: self.accepted(i, sc, at(k, dm))   # noqa: E731
        n_ev = 2
        e0, eM = F(0), F(K)
        lo_in, lo_out, hi_in, hi_out = 0, 0, (K if eM else 0), K
        if not e0:
            seed = None
            n_ev += 1
            if F(HALF):
                seed = HALF
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
                        trace.append((at(mid, dm), abs(self.slope_cos(i, sc, at(mid, dm))), self.near(i, sc, at(mid, dm))))
                    if (self.slope(i, sc, at(mid, dm)) < 0.0) != flip:
                        dl = mid
                    else:
                        dh = mid
                    if dh - dl <= 1:
                        break
            if seed is None:
                return np.array([np.inf, -dm, -np.inf, dm]), n_ev
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
        return np.array([at(lo_in, dm), -np.inf if e0 else at(lo_out, dm), at(hi_in, dm), np.inf if eM else at(hi_out, dm)]), n_ev


def device_class(acc, d_max=D_MAX):
    """The class a returned accel[..., 4] stands for."""
    lo, lo_out, hi, hi_out = (acc[..., k] for k in range(4))
    open_lo, open_hi = (lo == -d_max) & np.isneginf(lo_out), (hi == d_max) & np.isposinf(hi_out)
    zero_in = (lo <= 0.0) & (0.0 <= hi)
    out = np.where(zero_in, "both", "window").astype("<U6")
    out[open_lo & ~open_hi] = np.where(zero_in, "hi_in", "hi_out")[open_lo & ~open_hi]
    out[open_hi & ~open_lo] = np.where(zero_in, "lo_in", "lo_out")[open_hi & ~open_lo]
    out[open_lo & open_hi] = "all"
    out[np.isinf(lo) & (lo > 0)] = "none"
    return out


# ---- the kernel source through the host emulation -----------------------------------------------------------------------------------
def emu_lib(fma=False):
    import ctypes as C
    import os
    from pathlib import Path

    name = "libupr_pathacc_emu_fma.so" if fma else "libupr_pathacc_emu.so"
    return C.CDLL(os.environ.get("UPR_PATHACC_EMU_FMA_LIB" if fma else "UPR_PATHACC_EMU_LIB", str(Path(__file__).resolve().parent / "emu" / name)))


def have_fma_twin():
    from pathlib import Path

    try:
        has_fma = " fma " in Path("/proc/cpuinfo").read_text().replace("\n", " ")
    except OSError:
        has_fma = False
    if has_fma:
        assert (Path(__file__).resolve().parent / "emu" / "libupr_pathacc_emu_fma.so").exists(), "the host has FMA but libupr_pathacc_emu_fma.so was not built"
    return has_fma


def run_emu(P, x, params, per_point, d_max=D_MAX, speed=1.0, form=-1, fma=False):
    """dict(accel (n, ns, 4), z (n, ns, 2, ncol), y (n, ns, 2, 6 nb), iters (n, ns)) of the job compiled for the host"""
    import ctypes as C

    from upright_amd import _capi

    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3 * P.nq)
    params = np.ascontiguousarray(params, dtype=np.float64)
    n, ns = x.shape[0], (params.shape[1] if per_point else params.shape[0])
    out = dict(accel=np.full((n, ns, 4), np.nan), z=np.full((n, ns, 2, R.ncol(P)), np.nan), y=np.full((n, ns, 2, 6 * P.nb), np.nan),
               iters=np.full((n, ns), -1, dtype=np.int32))
    cp = _capi.problem_to_c(P)
    rc = emu_lib(fma).emu_pac_points(C.byref(cp), n, _capi.ptr(x), ns, _capi.ptr(params), 1 if per_point else 0, C.c_double(d_max), C.c_double(speed),
                                     _capi.ptr(out["accel"]), _capi.ptr(out["z"]), _capi.ptr(out["y"]), _capi.iptr(out["iters"]), int(form))
    assert rc == 0
    return out


def run_launch(L, **kw):
    return run_emu(L["P"], L["x"], L["params"], L["per_point"], L["d_max"], L["speed"], **kw)


def emu_rhs(P, x, theta, speed, d):
    """b [n][6 nb] as a job builds it: the state point with v_ee, the transformed record, the rhs routine"""
    import ctypes as C

    from upright_amd import _capi

    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3 * P.nq)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    b = np.full((x.shape[0], 6 * P.nb), np.nan)
    cp = _capi.problem_to_c(P)
    assert emu_lib().emu_pac_rhs(C.byref(cp), x.shape[0], _capi.ptr(x), _capi.ptr(theta), C.c_double(speed), C.c_double(d), _capi.ptr(b)) == 0
    return b


def emu_plan(P, accel, xs, speed):
    """(window, knot, limit) of the plan reductions compiled for the host: accel (B, nk, ns, 4), xs (B, nk, nx)"""
    import ctypes as C

    from upright_amd import _capi

    accel, xs = (np.ascontiguousarray(a, dtype=np.float64) for a in (accel, xs))
    B, nk, ns = accel.shape[:3]
    w, kn, lim = np.full((B, ns, 2), np.nan), np.full((B, ns, 2), -1, dtype=np.int32), np.full((B, 2), np.nan)
    cp = _capi.problem_to_c(P)
    assert emu_lib().emu_pac_plan(C.byref(cp), B, nk, ns, _capi.ptr(accel), xs.shape[2], C.c_double(speed), _capi.ptr(xs), _capi.ptr(w), _capi.iptr(kn),
                                  _capi.ptr(lim)) == 0
    return w, kn, lim


def numpy_plan(P, accel, xs, speed):
    """The same reductions in numpy: max / min / first argmax over the knots; the interval of d from the acceleration box."""
    w = np.stack([accel[..., 0].max(axis=1), accel[..., 2].min(axis=1)], axis=-1)
    kn = np.stack([accel[..., 0].argmax(axis=1), accel[..., 2].argmin(axis=1)], axis=-1).astype(np.int32)
    nq = P.nq
    lb, ub = (np.asarray(a, dtype=np.float64)[2 * nq:3 * nq] for a in (P.x_lb, P.x_ub))
    v, a = xs[..., nq:2 * nq], speed * speed * xs[..., 2 * nq:3 * nq]
    with np.errstate(divide="ignore", invalid="ignore"):
        dl, du = (lb - a) / v, (ub - a) / v
    lo = np.where(v == 0, -np.inf, np.where(v > 0, dl, du)).reshape(xs.shape[0], -1).max(axis=1)
    hi = np.where(v == 0, np.inf, np.where(v > 0, du, dl)).reshape(xs.shape[0], -1).min(axis=1)
    return w, kn, np.stack([lo, hi], axis=-1)


_CASES = {}


def cases(arrangements, name):
    """build_case(name), each launch with its Jobs (key "jobs"), its classes on the reference (key "pclass") and the emulation's
    answer (key "emu"); computed once per session, shared by the tests, modified by none."""
    if name not in _CASES:
        launches = build_case(arrangements, name)
        for L in launches:
            L["jobs"] = Jobs(L)
            L["jobs"].classes()
            L["emu"] = run_launch(L)
        _CASES[name] = launches
    return _CASES[name]


def class_counts(launches):
    allc = np.concatenate([L["pclass"].ravel() for L in launches])
    return {c: int((allc == c).sum()) for c in CLASSES}


def expected_classes(P):
    """The classes an arrangement of the table holds at least five jobs of: all of them with friction; without it (nf = 1) the
    compensated tilt is balanced at one d alone, so there is no window."""
    return CLASSES if P.nf == 3 else tuple(c for c in CLASSES if c != "window")


SLOPE_MIN = S.SLOPE_MIN


def steady(L):
    """speed_ref.steady for this quantity: the jobs of the classes all and none whose every decision is 1e-9 max(|b|, 1) away from the
    boundary on the reference (and, for none, every slope of the descent search decided)."""
    if "steady" not in L:
        J = L["jobs"]
        m = np.isin(L["pclass"], ("all", "none"))
        for i, sc in np.argwhere(m):
            i, sc = int(i), int(sc)
            ok = J.near(i, sc, -J.d_max) > RHO_TOL and J.near(i, sc, J.d_max) > RHO_TOL
            if ok and L["pclass"][i, sc] == "none":
                tr = []
                J.replay(i, sc, trace=tr)
                ok = J.near(i, sc, 0.0) > RHO_TOL and all(c >= SLOPE_MIN and n > RHO_TOL for _, c, n in tr)
            m[i, sc] = ok
        L["steady"] = m
    return L["steady"]


# ---- the assertions both test files make on an answer (emulation or device) ---------------------------------------------------------
def check_answer(L, out):
    """The conventions, the bracket, both certificates at both ends on the oracle's b and A (bounds of DESIGN 3.7 / 3.8, as
    speed_ref.check_answer), rho_ref on its own side at every in and out, the class.  out: dict(accel, z, y, iters).  Returns the list
    of violations."""
    J = L["jobs"]
    P, dm = J.P, J.d_max
    ac, z, y, it = out["accel"], out["z"], out["y"], out["iters"]
    assert ac.shape == (J.n, J.ns, 4) and not np.any(np.isnan(ac))
    cls = L["pclass"]
    got = device_class(ac, dm)
    assert np.array_equal(got, cls), [(i, sc, ac[i, sc], cls[i, sc]) for i, sc in np.argwhere(got != cls)[:5]]
    assert it.min() >= 0 and it.max() <= (3 + 3 * BISECT) * 3 * R.ncol(P)
    tol_col = R.emu_lib().emu_bal_tol()
    step = dm * 2.0 ** -(BISECT - 1)
    bad = []
    for i in range(J.n):
        for sc in range(J.ns):
            c = cls[i, sc]
            lo, lo_out, hi, hi_out = ac[i, sc]
            if c == "none":
                assert lo == np.inf and lo_out == -dm and hi == -np.inf and hi_out == dm
                assert not z[i, sc].any()
            else:
                assert -dm <= lo <= hi <= dm
            if c == "all":
                assert (lo, lo_out, hi, hi_out) == (-dm, -np.inf, dm, np.inf) and not y[i, sc].any()
            if c.startswith("hi"):
                assert lo == -dm and lo_out == -np.inf and not y[i, sc, 0].any()
                assert hi_out - hi == step, (i, sc, hi, hi_out)                                                  # the bracket, exact
            if c.startswith("lo"):
                assert hi == dm and hi_out == np.inf and not y[i, sc, 1].any()
                assert lo - lo_out == step, (i, sc, lo, lo_out)
            if c in ("both", "window"):
                assert lo - lo_out == step and hi_out - hi == step, (i, sc, ac[i, sc])
            for e, d_in, d_out in ((0, lo, lo_out), (1, hi, hi_out)):
                if np.isfinite(d_in):                                                                           # accepted end
                    r = J.ref(i, sc, d_in)
                    s1 = max(r["bnorm"], 1.0)
                    res = np.linalg.norm(r["b"] + r["A"] @ z[i, sc, e])
                    if not z[i, sc, e].min() >= 0.0: bad.append(("z >= 0", i, sc, c, e, z[i, sc, e].min()))
                    if not res <= (EPS + RHO_TOL) * s1: bad.append(("|b + A z|", i, sc, c, e, res / s1))
                    if not r["rho"] <= (EPS + RHO_TOL) * s1: bad.append(("rho_ref(in)", i, sc, c, e, r["rho"] / s1))
                if np.isfinite(d_out):                                                                          # rejected end
                    r = J.ref(i, sc, d_out)
                    s1 = max(r["bnorm"], 1.0)
                    yy = y[i, sc, e]
                    w = (r["A"].T @ yy) / (np.linalg.norm(r["A"], axis=0) * s1)
                    if not np.all(w >= -10.0 * tol_col): bad.append(("a_j' y", i, sc, c, e, w.min()))
                    sep = yy @ r["b"] / np.linalg.norm(yy)
                    if not sep >= (EPS - RHO_TOL) * s1: bad.append(("y' b / |y|", i, sc, c, e, sep / s1))
                    if not r["rho"] >= (EPS - RHO_TOL) * s1: bad.append(("rho_ref(out)", i, sc, c, e, r["rho"] / s1))
    return bad


def known_answers(L, accel, name, scenarios=R.FACET_SCENARIOS):
    """Largest relative |d - d_known| / |d_known| over the states of a launch with shared scenarios that carry a known answer, per
    family: dict(vertical, slide, comp) and the count of ends compared.  Slide and comp where sliding binds (SLIDING_BINDS, in the
    scenarios that keep it so), the vertical kinds on every arrangement in every scenario.  Ends clipped to +-d_max are skipped."""
    P, dm, s0 = L["P"], L["d_max"], L["speed"]
    worst = dict(vertical=0.0, slide=0.0, comp=0.0, n=0)
    ns = accel.shape[1]
    for i, inf in enumerate(L["info"]):
        if inf is None:
            continue
        fam = "vertical" if inf[0] in VERTICAL else inf[0]
        if fam != "vertical" and name not in SLIDING_BINDS:
            continue
        rows = range(ns) if fam == "vertical" else [s for s in scenarios if s < ns]
        kn = known(P, inf, s0, dm)
        for col, v in ((0, kn[0]), (2, kn[1])):
            if abs(v) >= dm:
                continue
            for sc in rows:
                worst[fam] = max(worst[fam], abs(accel[i, sc, col] - v) / abs(v))
                worst["n"] += 1
    return worst
