"""CPU reference of the friction margin per contact group (upright_amd/csrc/upr_margin.h, upr_grp_args), its case table and the
assertions its CPU and GPU tests share.

rho_ref of a job at a scale vector v (nc,) is balance_ref.reference on a copy of the problem whose contact_mu is v * mu, elementwise.
The scale vector of group g at kappa is kappa on the contacts of the group and the base scale beta[s] (ones without a table)
elsewhere.  GroupJobs is margin_ref.Jobs with that evaluation: feasible, classify (four evaluations: 0, 1 - 1e-3, 1 + 1e-3,
kappa_max) and bisect are the inherited ones, so a group of a launch is a launch of margin_ref ("view") and margin_ref.check_answer,
reference_bisections and near_masks apply to it as they stand.

The table (build_case): per arrangement one launch of 200 - 260 (point, scenario) jobs with shared scenarios, 37 x 1 in both
parameter layouts and 1 x 1 in both layouts.  As in margin_ref the states are mostly `lift` (normal forces alone balance them: zero
for every group) and `down` (inf for every group); the `inside` states are the ones that need friction, and which group's friction
they need is the question.  The finite (job, group) pairs cost a full bisection on the reference each and end on the boundary (their
iteration counts are not compared between device and emulation), so they are kept to a few dozen per arrangement."""
import copy
import ctypes as C
import os
from pathlib import Path

import numpy as np

import balance_ref as R
import margin_ref as M

EPS, BISECT, KAPPA_MAX, RHO_TOL = M.EPS, M.BISECT, M.KAPPA_MAX, M.RHO_TOL
FRICTION = ["foam_die2", "box_arch", "blue_cups", "fixture_box", "bottle_20_contacts"]
NF1 = ["pink_bottle_nf1", "robust_8corner"]
NAMES = FRICTION + NF1
ONE_BODY = ["fixture_box", "bottle_20_contacts"]
FINITE = ("below", "one", "above")


def scaled_c(P, v):
    Pk = copy.copy(P)
    Pk.contact_mu = np.asarray(v, dtype=np.float64) * np.asarray(P.contact_mu, dtype=np.float64)
    return Pk


def pair_labels(P):
    """compute_contact_idx of the reference's friction tool: a label per contact by its pair of objects, first occurrence first."""
    seen, out = {}, []
    for i in range(P.nc):
        out.append(seen.setdefault((int(P.contact_body1[i]), int(P.contact_body2[i])), len(seen)))
    return np.array(out)


def by_pair(P):
    lab = pair_labels(P)
    return [np.flatnonzero(lab == g) for g in range(lab.max() + 1)]


def masks_of(groups):
    return np.array([sum(1 << int(i) for i in g) for g in groups], dtype=np.uint32)


class GroupJobs(M.Jobs):
    """The jobs of one launch for one of its groups: ref(i, s, kappa) evaluates the reference at the group's scale vector."""

    def __init__(self, L, g):
        super().__init__(L)
        self.g, self.idx = g, np.asarray(L["groups"][g])
        self.base = None if L.get("mu_base") is None else np.asarray(L["mu_base"], dtype=np.float64)

    def scale(self, s, kappa):
        v = np.ones(self.P.nc) if self.base is None else self.base[s].copy()
        v[self.idx] = kappa
        return v

    def ref(self, i, s, kappa):
        key = (i, s, float(kappa))
        if key not in self._memo:
            out = R.reference(scaled_c(self.P, self.scale(s, kappa)), self.x[i:i + 1], self.theta(i, s)[None], False)
            self._memo[key] = dict(rho=float(out["rho"][0, 0]), bnorm=float(out["bnorm"][0, 0]), b=out["b"][0, 0], A=out["A"][0, 0])
        return self._memo[key]


def views(L):
    """One launch of margin_ref per group of L: dict(jobs, mclass), classes on the reference alone; computed once."""
    if "views" not in L:
        vs = []
        for g in range(len(L["groups"])):
            J = GroupJobs(L, g)
            V = dict(jobs=J, g=g)
            V["mclass"] = np.array([[J.classify(i, s) for s in range(J.ns)] for i in range(J.n)])
            vs.append(V)
        L["views"] = vs
    return L["views"]


def group_out(out, g):
    """The answer of group g of an answer with a trailing group axis, in the layout margin_ref.check_answer reads."""
    return dict(kappa_hi=out["kappa_hi"][:, :, g], kappa_lo=out["kappa_lo"][:, :, g], z=out["z"][:, :, g], y=out["y"][:, :, g], iters=out["iters"][:, :, g])


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def groups_of(P, name):
    if name == "fixture_box":
        return [np.arange(0, 4), np.arange(4, 8)]                       # bottom / walls
    if name == "bottle_20_contacts":
        return [np.arange(0, 10), np.arange(10, 20), np.arange(5, 15)]  # both words of the column masks, one overlapping group
    if name == "pink_bottle_nf1":
        return [np.arange(0, 2), np.arange(2, 4)]
    if name == "robust_8corner":
        return [np.arange(0, 16), np.arange(16, 32)]
    return by_pair(P)


def build_case(arrangements, name):
    P = R.table_problem(arrangements, name)
    seed = 5 + sum(map(ord, name))
    groups = groups_of(P, name)
    scen = R.scenarios(P)
    calm = "inside" if P.nf == 3 else "lift"
    down = "lift" if name == "fixture_box" else "down"   # (margin_ref.N_DOWN: rho is not accurate to 1e-9 next to kappa mu = 1)
    if name == "blue_cups":
        # 7 bodies, 112 columns: 37 points x 1 scenario only -- the nominal one (seven cups side by side, a pair of objects each:
        # with the centres of mass moved to the CoM-box vertex no state of the table is balanced at any friction)
        k2 = (["lift", down] * 19)[:34] + [calm] * 3
        x2 = R.points(P, k2, seed=seed)
        return [dict(P=P, x=x2, params=scen[0:1], per_point=False, kinds=k2, groups=groups, mu_base=None)]
    kinds = ["lift"] * 34 + [down] * 24 + [calm] * 6
    if P.nb == 1 and P.nf == 3:
        kinds = ["lift"] * 32 + [down] * 24 + [calm] * 6 + ["facet"] * 2
    x = R.points(P, kinds, seed=seed)
    base = dict(P=P, groups=groups, mu_base=None)
    launches = [dict(base, x=x, params=scen, per_point=False, kinds=kinds)]                                              # 64 x 4 = 256
    k2 = (["lift", down] * 19)[:34] + [calm] * 3
    x2 = R.points(P, k2, seed=seed + 1)
    launches.append(dict(base, x=x2, params=scen[1:2], per_point=False, kinds=k2))                                       # 37 x 1
    launches.append(dict(base, x=x2, params=np.stack([scen[i % 4:i % 4 + 1] for i in range(37)]), per_point=True, kinds=k2))   # 37 x 1
    launches.append(dict(base, x=x[63:64], params=scen[1:2], per_point=False, kinds=kinds[63:64]))                       # 1 x 1
    launches.append(dict(base, x=x[1:2], params=scen[None, 1:2], per_point=True, kinds=kinds[1:2]))                      # 1 x 1
    if name == "box_arch":
        # a non-default base scale: half the friction on one pair of objects, in the CoM-shift scenario and the nominal one
        beta = np.ones((2, P.nc))
        beta[:, groups[0]] = 0.5
        launches.append(dict(P=P, groups=groups, mu_base=beta, x=x2, params=scen[:2], per_point=False, kinds=k2))        # 37 x 2
    return launches


# ---- the kernel source through the host emulation -------------------------------------------------------------------------------------
def emu_lib():
    return C.CDLL(os.environ.get("UPR_GROUP_MARGIN_EMU_LIB", str(Path(__file__).resolve().parent / "emu" / "libupr_group_margin_emu.so")))


def run_emu(P, x, params, per_point, groups, mu_base=None, kappa_max=KAPPA_MAX, form=-1):
    """dict(kappa_hi, kappa_lo, z, y, iters), each with a trailing group axis, of the group job compiled for the host."""
    from upright_amd import _capi

    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3 * P.nq)
    params = np.ascontiguousarray(params, dtype=np.float64)
    n, ns, ng = x.shape[0], (params.shape[1] if per_point else params.shape[0]), len(groups)
    out = dict(kappa_hi=np.full((n, ns, ng), np.nan), kappa_lo=np.full((n, ns, ng), np.nan), z=np.full((n, ns, ng, R.ncol(P)), np.nan),
               y=np.full((n, ns, ng, 6 * P.nb), np.nan), iters=np.full((n, ns, ng), -1, dtype=np.int32))
    masks = masks_of(groups)
    base = None if mu_base is None else np.ascontiguousarray(mu_base, dtype=np.float64)
    cp = _capi.problem_to_c(P)
    rc = emu_lib().emu_grp_points(C.byref(cp), n, _capi.ptr(x), ns, _capi.ptr(params), 1 if per_point else 0, ng, masks.ctypes.data_as(C.POINTER(C.c_uint)),
                                  _capi.ptr(base), C.c_double(kappa_max), _capi.ptr(out["kappa_hi"]), _capi.ptr(out["kappa_lo"]), _capi.ptr(out["z"]),
                                  _capi.ptr(out["y"]), _capi.iptr(out["iters"]), int(form))
    assert rc == 0
    return out


def run_emu_rho(P, x, params, per_point, mu_scale_c, form=-1):
    """(rho, iters) of the balance check with a scale per scenario and contact, mu_scale_c (n_scen, nc), through the emulation."""
    from upright_amd import _capi

    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3 * P.nq)
    params = np.ascontiguousarray(params, dtype=np.float64)
    n, ns = x.shape[0], (params.shape[1] if per_point else params.shape[0])
    mu = np.ascontiguousarray(mu_scale_c, dtype=np.float64)
    assert mu.shape == (ns, P.nc)
    rho, iters = np.full((n, ns), np.nan), np.full((n, ns), -1, dtype=np.int32)
    cp = _capi.problem_to_c(P)
    rc = emu_lib().emu_grp_rho_points(C.byref(cp), n, _capi.ptr(x), ns, _capi.ptr(params), 1 if per_point else 0, _capi.ptr(mu), _capi.ptr(rho), None,
                                      _capi.iptr(iters), int(form))
    assert rc == 0
    return rho, iters


def emu_worst(kappa_hi):
    """(worst, knot) of kappa_hi (B, nk, ...) by the reduction of the plan call, through the emulation."""
    k = np.ascontiguousarray(kappa_hi, dtype=np.float64)
    B, nk = k.shape[:2]
    inner = int(np.prod(k.shape[2:]))
    w, kn = np.full((B,) + k.shape[2:], np.nan), np.full((B,) + k.shape[2:], -1, dtype=np.int32)
    assert emu_lib().emu_grp_worst(k.ctypes.data_as(C.POINTER(C.c_double)), B, nk, C.c_longlong(inner), w.ctypes.data_as(C.POINTER(C.c_double)),
                                   kn.ctypes.data_as(C.POINTER(C.c_int))) == 0
    return w, kn


_CASES = {}


def cases(arrangements, name):
    """build_case(name), each launch with its views (reference classes per group) and the emulation's answer (key "emu"); computed
    once per session, shared by the tests, modified by none."""
    if name not in _CASES:
        launches = build_case(arrangements, name)
        for L in launches:
            views(L)
            L["emu"] = run_emu(L["P"], L["x"], L["params"], L["per_point"], L["groups"], L["mu_base"])
        _CASES[name] = launches
    return _CASES[name]


def group_views(launches, g):
    """The views of group g over the launches that share the groups of the first one: a list margin_ref's helpers take."""
    return [views(L)[g] for L in launches]


def class_counts(launches):
    """Per group: {zero, finite, inf} counts over the launches, on the reference alone."""
    out = []
    for g in range(len(launches[0]["groups"])):
        allc = np.concatenate([views(L)[g]["mclass"].ravel() for L in launches])
        out.append(dict(zero=int((allc == "zero").sum()), finite=int(np.isin(allc, FINITE).sum()), inf=int((allc == "inf").sum()),
                        below=int((allc == "below").sum())))
    return out


# ---- assertions both test files make on an answer (emulation or device) ------------------------------------------------------------------
def check_group_answer(L, out, kappa_max=KAPPA_MAX):
    """Assertions 3 and 4 on one launch, group by group: margin_ref.check_answer (the certificates on the oracle's b and A at the
    group's scale vector, rho_ref at both ends, the class) and the bracket width, exactly kappa_max 2^-32 on finite jobs."""
    bad = []
    for g, V in enumerate(views(L)):
        og = group_out(out, g)
        bad += [(g,) + b for b in M.check_answer(V, og, kappa_max)]
        fin = np.isin(V["mclass"], FINITE)
        assert np.all(og["kappa_hi"][fin] - og["kappa_lo"][fin] == kappa_max * 2.0 ** -BISECT), (g, "bracket width")
    if L["P"].nf == 1:
        hi = out["kappa_hi"]
        assert np.all(hi == hi[:, :, :1]) and np.all((hi == 0.0) | np.isposinf(hi))                  # one evaluation, equal across groups
        assert np.all(out["iters"] == out["iters"][:, :, :1])
    return bad


def scale_vectors(L, kappa):
    """(n, n_scen, n_grp, nc): the scale vector of every (job, group) at kappa (n, n_scen, n_grp)."""
    P = L["P"]
    n, ns, ng = kappa.shape
    beta = np.ones((ns, P.nc)) if L["mu_base"] is None else np.asarray(L["mu_base"], dtype=np.float64)
    v = np.broadcast_to(beta[None, :, None, :], (n, ns, ng, P.nc)).copy()
    for g, idx in enumerate(L["groups"]):
        v[:, :, g, idx] = kappa[:, :, g, None]
    return v


def check_order(common_hi, group_hi, tol=1e-6):
    """Assertion 6 (beta = 1): where the common margin is <= 1 no group needs more than it; where it is > 1 or inf every group alone
    needs at least as much (or cannot help at all)."""
    c = common_hi[..., None]
    ok = np.where(c <= 1.0, group_hi <= c + tol, (group_hi >= c - tol) | np.isposinf(group_hi))
    return np.argwhere(~ok)


def check_rho_per_contact(L, rho_c, rho_mu, rho_plain, who, name):
    """Assertion 2 on one launch.  rho_c(x, params, per_point, scale (n_scen, nc)), rho_mu(..., mu (n_scen,)), rho_plain(x, params,
    per_point) -> (rho, iters): rows uniform over the contacts give the bits of the per-scenario call, all ones those of the call
    without a scale, and random scales from {0.5, 1, 2} per contact keep |rho - rho_ref| <= 1e-9 max(1, |b|)."""
    P, x, prm, pp = L["P"], L["x"], L["params"], L["per_point"]
    ns = prm.shape[1] if pp else prm.shape[0]
    mu = np.array([0.5, 1.0, 2.0, 0.0])[np.arange(ns) % 4]
    a, b = rho_c(x, prm, pp, np.repeat(mu[:, None], P.nc, axis=1)), rho_mu(x, prm, pp, mu)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, "uniform rows")
    a, b = rho_c(x, prm, pp, np.ones((ns, P.nc))), rho_plain(x, prm, pp)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, "all ones")
    rng = np.random.default_rng(17 + sum(map(ord, name)))
    v = rng.choice([0.5, 1.0, 2.0], size=(ns, P.nc))
    rho = rho_c(x, prm, pp, v)[0]
    J = M.Jobs(L)
    worst = 0.0
    for i in range(J.n):
        for s in range(J.ns):
            e = R.reference(scaled_c(P, v[s]), J.x[i:i + 1], J.theta(i, s)[None], False)
            worst = max(worst, abs(rho[i, s] - e["rho"][0, 0]) / max(e["bnorm"][0, 0], 1.0))
    print("balance check with a scale per contact, %s vs nnls, %s: %.2e" % (who, name, worst))
    assert worst <= RHO_TOL, (name, worst)


def check_closure(L, out, rho_c):
    """Assertion 5 on one launch: the rho call with the scale vector "kappa_hi on the group, beta elsewhere" returns rho <= EPS
    max(|b|, 1) and with kappa_lo rho above it, exactly (the products mu_i s_i are the same bits in both kernels).  One call per
    point: its (scenario, group) pairs as the scenarios of the call."""
    J = M.Jobs(L)
    P = J.P
    hi, lo = out["kappa_hi"], out["kappa_lo"]
    n, ns, ng = hi.shape
    vh, vl = scale_vectors(L, np.where(np.isfinite(hi), hi, 0.0)), scale_vectors(L, lo)
    for i in range(n):
        prm = np.stack([J.theta(i, s) for s in range(ns) for _ in range(ng)])
        b = np.array([J.ref(i, s, 1.0)["bnorm"] for s in range(ns) for _ in range(ng)])   # (|b| does not depend on the friction)
        lim = EPS * np.maximum(b, 1.0)
        rh = rho_c(J.x[i:i + 1], prm, False, vh[i].reshape(ns * ng, P.nc))[0][0]
        rl = rho_c(J.x[i:i + 1], prm, False, vl[i].reshape(ns * ng, P.nc))[0][0]
        fin, zero = np.isfinite(hi[i]).ravel(), (hi[i] == 0.0).ravel()
        # (the kernels form the limit from their own |b|; the oracle's |b| used here agrees with it to rounding -- a rho within
        #  1e-15 of the limit, relative, could show as a failure here without being one; none of the table is)
        assert np.all(rh[fin] <= lim[fin]), (i, "feasible at kappa_hi", rh[fin] / lim[fin])
        assert np.all(rl[~zero] > lim[~zero]), (i, "infeasible at kappa_lo", rl[~zero] / lim[~zero])
