"""CPU reference of the batched disturbance margin (upright_amd/csrc/upr_disturb.h), its case table and the assertions its CPU and GPU
tests share.

rho_ref(r) of a job (point, scenario, direction u) is balance_ref.reference at the JOINT-SPACE state balance_ref.state_for(O, q, v,
a_ee(x) + r u_a, alpha(x) + r u_alpha): a_ee(x), alpha(x) and C_we come from the oracle's ee_kinematics of x, a tray-frame u is rotated
by that C_we in numpy.  Nothing of the kernel's record transform is in it.  Jobs subclasses pathacc_ref.Jobs for ONE direction block of
a launch (ref overridden, no `moving` short-cut), so classify, replay, slope, steady, device_class and check_answer of pathacc_ref serve
unchanged, block by block: a block is a dict with the keys check_answer reads (d_max = r_max, speed = 1).

The table.  States are kinds of pathacc_ref.make_states, cut to about 500 jobs per arrangement (a job costs the reference as much as
one of pathacc's).  Directions (tray frame, u_alpha = 0): span_0, span_1 of contact 0 and e_z; on friction shapes also cos(phi) span_j
+ sin(phi) e_z, tan(phi) = 2 mu_max.  Every constructed state has omega = 0 and v_ee = +-w u^ for some unit u^; where u^ is a direction
of the set the chord is pathacc's interval times +-w and pathacc_ref.known gives the closed form (known()).  The record does not hold
v_ee, so rest, slide, lift and sink are one state to this quantity: both along the span directions, all along e_z at r_max = 8 and
lo_in at r_max = 12 (r_lo = -g0, free fall).  falling / rising: lo_out along e_z (r_lo = k), none along the others.  The compensated
tilt along the tray's own span direction: a window that excludes 0.  Every direction of the set has a non-negative e_z part and nothing
bounds an upward push, so hi_in / hi_out cannot occur on the set itself: one more launch runs span_0 and e_z NEGATED, where
they are the mirrors of lo_in / lo_out (r_hi = g0, r_hi = -k).
Launches: shared scenarios; per-point scenarios; two 1 x 1; r_max = 12 (so that -g0 is inside the range); the negated directions."""
import numpy as np

import balance_ref as R
import pathacc_ref as A
from oracle.oracle import Oracle

EPS, RHO_TOL, BISECT = A.EPS, A.RHO_TOL, A.BISECT
R_MAX = 8.0
NAMES, ONE_BODY, CLASSES = A.NAMES, A.ONE_BODY, A.CLASSES
MULTI_BODY = "foam_die2"          # the multi-body shape the device is held against the emulation on
FRAMES = {"world": 0, "tray": 1}


def step(r_max):
    return r_max * 2.0 ** -(BISECT - 1)


def tray_dirs(P):
    """(n_dir, 6): (0, span_0), (0, span_1), (0, e_z) and, with friction, (0, cos(phi) span_j + sin(phi) e_z), tan(phi) = 2 mu_max"""
    span = np.asarray(P.contact_span, dtype=np.float64)[0]
    ez = np.array([0.0, 0.0, 1.0])
    u = [span[0], span[1], ez]
    if P.nf == 3:
        phi = np.arctan(2.0 * float(np.max(P.contact_mu)))
        u += [np.cos(phi) * span[j] + np.sin(phi) * ez for j in range(2)]
    return np.concatenate([np.zeros((len(u), 3)), np.stack(u)], axis=1)


def ee_of(O, x):
    """C_we (3, 3), v_ee, omega, a_ee, alpha of the oracle at x"""
    ee = O.ee_kinematics(np.asarray(x, dtype=np.float64))
    return ee[3:12].reshape(3, 3), ee[12:15], ee[15:18], ee[18:21], ee[21:24]


def world_dirs(P, x, dirs):
    """(n, n_dir, 6): tray-frame dirs rotated by the oracle's C_we of every state, in numpy"""
    O = Oracle(P)
    out = []
    for xi in np.asarray(x).reshape(-1, 3 * P.nq):
        Cm = ee_of(O, xi)[0]
        out.append(np.concatenate([dirs[:, :3] @ Cm.T, dirs[:, 3:] @ Cm.T], axis=1))
    return np.stack(out)


def displaced(P, x, u_world, r):
    """the joint-space state whose end effector has (a_ee(x) + r u_a, alpha(x) + r u_alpha): x (3 nq,), u_world (6,)"""
    O = Oracle(P)
    nq = P.nq
    _, _, _, a, al = ee_of(O, x)
    return R.state_for(O, x[:nq], x[nq:2 * nq], a + r * u_world[3:], al + r * u_world[:3])


class Jobs(A.Jobs):
    """The jobs of one direction block: block = dict(launch, d=direction index, d_max=r_max, speed=1)."""

    def __init__(self, block):
        super().__init__(block)
        self.moving = np.ones(self.n, dtype=bool)        # (no short-cut: every r is another state)
        self.O = Oracle(self.P)
        u = np.asarray(block["dirs"], dtype=np.float64)[block["d"]]
        self.base = []
        nq = self.P.nq
        for x in self.x:
            Cm, _, _, a, al = ee_of(self.O, x)
            ua, ul = (Cm @ u[:3], Cm @ u[3:]) if block["frame"] == "tray" else (u[:3], u[3:])
            self.base.append((x[:nq], x[nq:2 * nq], a, al, ul, ua))

    def ref(self, i, sc, r):
        key = (i, sc, float(r))
        if key not in self._memo:
            q, v, a, al, ul, ua = self.base[i]
            x = R.state_for(self.O, q, v, a + key[2] * ul, al + key[2] * ua)
            out = R.reference(self.P, x[None], self.theta(i, sc)[None], False)
            self._memo[key] = dict(rho=float(out["rho"][0, 0]), bnorm=float(out["bnorm"][0, 0]), b=out["b"][0, 0], A=out["A"][0, 0], z=out["z"][0, 0])
        return self._memo[key]


def blocks_of(L):
    """The direction blocks of a launch, each with its Jobs (key "jobs") and the classes on the reference (key "pclass"); once."""
    if "blocks" not in L:
        L["blocks"] = []
        for d in range(len(L["dirs"])):
            b = dict(L, d=d, d_max=L["r_max"], speed=1.0)
            b["jobs"] = Jobs(b)
            b["jobs"].classes()
            L["blocks"].append(b)
    return L["blocks"]


def block_out(out, d):
    """the answer of direction d in the keys pathacc_ref.check_answer reads"""
    return dict(accel=out["reach"][d], z=out["z"][d], y=out["y"][d], iters=out["iters"][d])


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def kinds_main(P):
    if P.nf == 3:
        return ["rest", "slide1.0", "lift", "falling", "comp1.0", "compd1.0", "inside", "inside"]
    return ["rest", "rest", "slide1.0", "slide0.5", "lift", "lift", "sink", "sink", "falling", "rising", "rest", "lift"]


ROWS_PER_POINT = {3: [0, 2, 4, 6, 7], 1: [0, 3, 5, 8, 10]}
KINDS_FAR = ["rest", "lift", "sink", "slide0.5", "rising", "falling"]


def build_case(arrangements, name):
    P = R.table_problem(arrangements, name)
    seed = 43 + sum(map(ord, name))
    scen = A.scenario_set(P)
    dirs = tray_dirs(P)
    L = lambda **kw: dict(dict(P=P, r_max=R_MAX, frame="tray", dirs=dirs), **kw)   # noqa: E731
    k0 = kinds_main(P)
    x0, i0 = A.make_states(P, k0, seed)
    A.keep_out_vanishing_loads(P, x0, k0, i0, lambda i: scen)
    launches = [L(x=x0, params=scen, per_point=False, kinds=k0, info=i0)]                                                 # 8 | 12 x 4 x n_dir
    rows = ROWS_PER_POINT[P.nf]
    per = np.stack([scen[(np.arange(3) + i) % 4] for i in range(len(rows))])
    launches.append(L(x=x0[rows], params=per, per_point=True, kinds=[k0[r] for r in rows], info=[i0[r] for r in rows]))   # 5 x 3 x n_dir
    launches.append(L(x=x0[4:5], params=scen[:1], per_point=False, kinds=k0[4:5], info=i0[4:5]))                          # 1 x 1 x n_dir
    launches.append(L(x=x0[1:2], params=scen[None, 3:4], per_point=True, kinds=k0[1:2], info=i0[1:2]))                    # 1 x 1 x n_dir
    # r_max = 12: -g0 is inside the range (lo_in along e_z), and so is the window of the compensated tilt along the tray's own span
    # direction, g0 (sin(phi) -+ mu cos(phi)), which passes 8 where mu_max is large (the stacked arrangements)
    k1 = list(KINDS_FAR)
    far = scen[[0, 3, 2]]
    x1, i1 = A.make_states(P, k1, seed + 5)
    A.keep_out_vanishing_loads(P, x1, k1, i1, lambda i: far)
    tilt = [4, 5] if P.nf == 3 else []
    launches.append(L(x=np.concatenate([x1[:4], x0[tilt]]), params=far, per_point=False, kinds=k1[:4] + [k0[r] for r in tilt],
                      info=i1[:4] + [i0[r] for r in tilt], r_max=12.0))                                                   # 6 | 4 x 3 x n_dir
    launches.append(L(x=x1, params=far, per_point=False, kinds=k1, info=i1, r_max=12.0, dirs=-dirs[[0, 2]]))              # 6 x 3 x 2, negated
    return launches


def known(L, i, d):
    """(r_lo, r_hi) of state i of a launch along direction d in closed form, or None: where omega = 0 and v_ee = sigma w u^ with u^
    the (world-frame) direction, the chord is pathacc's interval of d times sigma w.  Open and clipped ends come out as +-r_max."""
    inf = L["info"][i]
    if inf is None:
        return None
    P = L["P"]
    Cm, v, om, _, _ = ee_of(Oracle(P), L["x"][i])
    u = np.asarray(L["dirs"])[d]
    if np.any(u[:3] != 0.0) or np.abs(om).max() > 1e-12:
        return None
    uw = Cm @ u[3:] if L["frame"] == "tray" else u[3:]
    w = float(np.linalg.norm(v))
    if abs(np.linalg.norm(uw) - 1.0) > 1e-12 or abs(abs(float(uw @ v)) - w) > 1e-9 * w:
        return None
    lo, hi = A.known(P, inf, 1.0, L["r_max"] / w)
    return (w * lo, w * hi) if uw @ v > 0 else (-w * hi, -w * lo)


def known_answers(L, reach, name, scenarios=R.FACET_SCENARIOS):
    """pathacc_ref.known_answers for this quantity: the largest relative |r - r_known| / |r_known| per family over the (state,
    direction) pairs of a launch with shared scenarios that carry a known answer, and the count of ends compared."""
    worst = dict(vertical=0.0, slide=0.0, comp=0.0, n=0)
    rm = L["r_max"]
    ns = reach.shape[2]
    for i, inf in enumerate(L["info"]):
        if inf is None:
            continue
        fam = "vertical" if inf[0] in A.VERTICAL else inf[0]
        if fam != "vertical" and name not in A.SLIDING_BINDS:
            continue
        rows = range(ns) if fam == "vertical" else [s for s in scenarios if s < ns]
        for d in range(reach.shape[0]):
            kn = known(L, i, d)
            if kn is None:
                continue
            for col, v in ((0, kn[0]), (2, kn[1])):
                if abs(v) >= rm:
                    continue
                for sc in rows:
                    worst[fam] = max(worst[fam], abs(reach[d, i, sc, col] - v) / abs(v))
                    worst["n"] += 1
    return worst


def class_counts(launches):
    allc = np.concatenate([b["pclass"].ravel() for L in launches for b in blocks_of(L)])
    return {c: int((allc == c).sum()) for c in CLASSES}


expected_classes = A.expected_classes


# ---- the kernel source through the host emulation -----------------------------------------------------------------------------------
def emu_lib(fma=False):
    import ctypes as C
    import os
    from pathlib import Path

    name = "libupr_disturb_emu_fma.so" if fma else "libupr_disturb_emu.so"
    return C.CDLL(os.environ.get("UPR_DISTURB_EMU_FMA_LIB" if fma else "UPR_DISTURB_EMU_LIB", str(Path(__file__).resolve().parent / "emu" / name)))


def have_fma_twin():
    from pathlib import Path

    try:
        has_fma = " fma " in Path("/proc/cpuinfo").read_text().replace("\n", " ")
    except OSError:
        has_fma = False
    if has_fma:
        assert (Path(__file__).resolve().parent / "emu" / "libupr_disturb_emu_fma.so").exists(), "the host has FMA but libupr_disturb_emu_fma.so was not built"
    return has_fma


def run_emu(P, x, params, per_point, dirs, r_max=R_MAX, frame="tray", form=-1, fma=False):
    """dict(reach (n_dir, n, ns, 4), z (n_dir, n, ns, 2, ncol), y (n_dir, n, ns, 2, 6 nb), iters (n_dir, n, ns)) of the job compiled for
    the host"""
    import ctypes as C

    from upright_amd import _capi

    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3 * P.nq)
    params = np.ascontiguousarray(params, dtype=np.float64)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 6)
    n, ns, nd = x.shape[0], (params.shape[1] if per_point else params.shape[0]), dirs.shape[0]
    out = dict(reach=np.full((nd, n, ns, 4), np.nan), z=np.full((nd, n, ns, 2, R.ncol(P)), np.nan), y=np.full((nd, n, ns, 2, 6 * P.nb), np.nan),
               iters=np.full((nd, n, ns), -1, dtype=np.int32))
    cp = _capi.problem_to_c(P)
    rc = emu_lib(fma).emu_dst_points(C.byref(cp), n, _capi.ptr(x), ns, _capi.ptr(params), 1 if per_point else 0, nd, _capi.ptr(dirs), FRAMES[frame],
                                     C.c_double(r_max), _capi.ptr(out["reach"]), _capi.ptr(out["z"]), _capi.ptr(out["y"]), _capi.iptr(out["iters"]),
                                     int(form))
    assert rc == 0
    return out


def run_launch(L, **kw):
    return run_emu(L["P"], L["x"], L["params"], L["per_point"], L["dirs"], L["r_max"], L["frame"], **kw)


def emu_rhs(P, x, theta, u, frame, r):
    """b [n][6 nb] as a job builds it: the state point, the displaced record, the rhs routine"""
    import ctypes as C

    from upright_amd import _capi

    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3 * P.nq)
    theta, u = (np.ascontiguousarray(a, dtype=np.float64) for a in (theta, u))
    b = np.full((x.shape[0], 6 * P.nb), np.nan)
    cp = _capi.problem_to_c(P)
    assert emu_lib().emu_dst_rhs(C.byref(cp), x.shape[0], _capi.ptr(x), _capi.ptr(theta), _capi.ptr(u), FRAMES[frame], C.c_double(r), _capi.ptr(b)) == 0
    return b


def emu_plan(reach):
    """(window, knot, radius, binding) of the plan reductions compiled for the host: reach (n_dir, B, nk, ns, 4)"""
    from upright_amd import _capi

    reach = np.ascontiguousarray(reach, dtype=np.float64)
    nd, B, nk, ns = reach.shape[:4]
    w, kn = np.full((nd, B, ns, 2), np.nan), np.full((nd, B, ns, 2), -1, dtype=np.int32)
    rad, bind = np.full((B, ns), np.nan), np.full((B, ns, 3), -9, dtype=np.int32)
    assert emu_lib().emu_dst_plan(B, nk, ns, nd, _capi.ptr(reach), _capi.ptr(w), _capi.iptr(kn), _capi.ptr(rad), _capi.iptr(bind)) == 0
    return w, kn, rad, bind


def numpy_plan(reach):
    """The same reductions in numpy: per direction max / min / first argmax over the knots; over the ends in the order (direction,
    lower before upper) the smallest of (-window_lo, window_hi) and the first end that attains it."""
    w = np.stack([reach[..., 0].max(axis=2), reach[..., 2].min(axis=2)], axis=-1)                          # (nd, B, ns, 2)
    kn = np.stack([reach[..., 0].argmax(axis=2), reach[..., 2].argmin(axis=2)], axis=-1).astype(np.int32)
    nd, B, ns = w.shape[:3]
    cand = np.moveaxis(w * np.array([-1.0, 1.0]), 0, 2).reshape(B, ns, 2 * nd)                              # end e of direction d at 2 d + e
    first = cand.argmin(axis=2)
    rad = np.take_along_axis(cand, first[..., None], axis=2)[..., 0]
    d, e = first // 2, first % 2
    bi, si = np.meshgrid(np.arange(B), np.arange(ns), indexing="ij")
    return w, kn, rad, np.stack([d, 2 * e - 1, kn[d, bi, si, e]], axis=-1).astype(np.int32)


_CASES = {}


def cases(arrangements, name):
    """build_case(name), each launch with its direction blocks (blocks_of: Jobs and classes on the reference) and the emulation's
    answer (key "emu"); computed once per session, shared by the tests, modified by none."""
    if name not in _CASES:
        launches = build_case(arrangements, name)
        for L in launches:
            blocks_of(L)
            L["emu"] = run_launch(L)
        _CASES[name] = launches
    return _CASES[name]


def check_launch(L, out):
    """pathacc_ref.check_answer on every direction block of a launch: the list of violations, each with its direction first"""
    bad = []
    for d, b in enumerate(blocks_of(L)):
        bad += [(d,) + v for v in A.check_answer(b, block_out(out, d))]
    return bad


def steady(L):
    """pathacc_ref.steady per direction block: (n_dir, n, ns) bool"""
    return np.stack([A.steady(b) for b in blocks_of(L)])


def classes_of(out, r_max):
    return np.stack([A.device_class(out["reach"][d], r_max) for d in range(out["reach"].shape[0])])
