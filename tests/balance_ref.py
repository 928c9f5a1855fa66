"""CPU reference of the batched balance check (upright_amd/csrc/upr_balance.h) and the case table its tests share.

For a point x = [q, v, a] and a scenario (body parameters theta [nb][10]) one Oracle carries theta; b = g(x, f = 0) and column
j = g(x, f = S e_j) - b come out of its equality-constraint call (g is affine in f), S the generators of every contact's friction
pyramid in the order of upright_robust/modelling.py:39-43 (n + mu s0, n + mu s1, n - mu s0, n - mu s1; nf = 1: the normal force
coordinate itself).  rho = min_{z >= 0} |b + A z| by scipy.optimize.nnls; the reference's own floor is its difference to a second CPU
solution, scipy.optimize.lsq_linear with bounds (0, inf) at tight tolerance (solve(): the smallest feasible residual of the three).

Cases (build_case): per arrangement of the table, points are states in motion placed by the end-effector acceleration they produce
(state_for: the joint accelerations are the least-norm solution for a wanted linear and angular acceleration of the tray, out of the
oracle's kinematic Jacobian), in the kinds
    inside    small horizontal accelerations: balancing forces exist;
    outside   horizontal accelerations well beyond mu g: outside the cone with columns in the passive set;
    down      the tray accelerates downward faster than gravity;
    facet     a tray at rest whose load feels exactly g (e_z + mu s) in the tray's frame, s a pyramid axis: the level tray accelerating
              horizontally by exactly mu g (one body, nf = 3);
    lift      a tray at rest whose load feels a purely normal force: inside the cone also without friction;
and the scenarios nominal, a centre-of-mass-box vertex (lever and residual both change), another mass, inertia scaled by 0.1.  The
free-fall class (b = 0 exactly) is the same arrangement in a problem without gravity, at rest: no floating-point walk reproduces
a = g to the last bit, a zero does.  classify() sorts jobs into the classes of the tests from the reference's solution alone."""
import copy

import numpy as np
from scipy.optimize import lsq_linear, nnls

from oracle.oracle import Oracle
from upright_amd import robots
from upright_amd.problem import THING_HOME, Problem, contacts_from_fixture, thing_problem

G0 = 9.81


def generators(P):
    """S [nc][3][gpc]: generator j of contact i as a force on object 1 (nf = 1: the normal)."""
    n, s, mu = np.asarray(P.contact_normal), np.asarray(P.contact_span), np.asarray(P.contact_mu)
    if P.nf == 1:
        return n[:, :, None]
    return np.stack([n + mu[:, None] * s[:, 0], n + mu[:, None] * s[:, 1], n - mu[:, None] * s[:, 0], n - mu[:, None] * s[:, 1]], axis=2)


def ncol(P):
    return P.nc * (4 if P.nf == 3 else 1)


def with_params(P, theta):
    Pb = copy.copy(P)
    Pb.body_params = np.ascontiguousarray(theta, dtype=np.float64).reshape(P.nb, 10)
    return Pb


def system(P, theta, x):
    """b [6 nb], A [6 nb][ncol] of one job, through Oracle.eq_constraint."""
    O = Oracle(with_params(P, theta))
    nq = P.nq
    u = np.zeros(P.nu)
    b = O.eq_constraint(x, u, jac=False).copy()
    S = generators(P)
    gpc = S.shape[2]
    A = np.zeros((b.size, P.nc * gpc))
    for i in range(P.nc):
        for g in range(gpc):
            u[:] = 0.0
            if P.nf == 3:
                u[nq + 3 * i:nq + 3 * i + 3] = S[i, :, g]
            else:
                u[nq + i] = 1.0
            A[:, i * gpc + g] = O.eq_constraint(x, u, jac=False) - b
    return b, A


def solve(b, A):
    """(rho, z, floor).  Every z >= 0 a CPU solver returns is feasible, so its residual bounds rho from above and the reference is
    the smallest of three: scipy's nnls on the raw columns, nnls on columns scaled to unit length (the cone does not depend on the
    length of a generator) and lsq_linear with bounds (0, inf) at tight tolerance.  floor = |better nnls answer - lsq_linear|, the
    reference's own uncertainty: scipy 1.15's nnls stops short of the minimum on a few jobs (box_arch 1.7185 on the raw columns
    against 1.71835 of lsq_linear and of the kernel; a pink_bottle job 0.02224 on unit-length columns against 0.02167; about one
    job in a few thousand of a headline plan under the study's sweep), never on both scalings on the jobs of the table."""
    nrm = np.linalg.norm(A, axis=0)
    As = A / nrm
    z1, _ = nnls(A, -b, maxiter=30 * A.shape[1])
    z2, _ = nnls(As, -b, maxiter=30 * A.shape[1])
    z2 = z2 / nrm
    ls = lsq_linear(As, -b, bounds=(0.0, np.inf), method="bvls", tol=1e-15, max_iter=100 * A.shape[1])
    z3 = np.maximum(ls.x, 0.0) / nrm
    r1, r2, r3 = (float(np.linalg.norm(b + A @ z)) for z in (z1, z2, z3))
    rho, z = min(((r1, z1), (r2, z2), (r3, z3)), key=lambda t: t[0])
    return rho, z, abs(min(r1, r2) - r3)


def reference(P, x, params, per_point):
    """x [n][3 nq]; params [n_scen][nb][10] or [n][n_scen][nb][10].  dict(rho [n][ns], z [n][ns][ncol], floor [n][ns], bnorm [n][ns],
    b [n][ns][m], A [n][ns][m][ncol])."""
    x = np.asarray(x).reshape(-1, 3 * P.nq)
    params = np.asarray(params, dtype=np.float64)
    n = x.shape[0]
    ns = params.shape[1] if per_point else params.shape[0]
    m, nc_ = 6 * P.nb, ncol(P)
    out = dict(rho=np.zeros((n, ns)), z=np.zeros((n, ns, nc_)), floor=np.zeros((n, ns)), bnorm=np.zeros((n, ns)),
               b=np.zeros((n, ns, m)), A=np.zeros((n, ns, m, nc_)))
    for i in range(n):
        for s in range(ns):
            th = params[i, s] if per_point else params[s]
            b, A = system(P, th, x[i])
            rho, z, fl = solve(b, A)
            out["rho"][i, s], out["z"][i, s], out["floor"][i, s], out["bnorm"][i, s] = rho, z, fl, np.linalg.norm(b)
            out["b"][i, s], out["A"][i, s] = b, A
    return out


# ---- scenarios ----------------------------------------------------------------------------------------------------------------
def com_shift(theta, delta):
    th = np.array(theta, dtype=np.float64).reshape(-1, 10)
    th[:, 1:4] += th[:, :1] * np.asarray(delta)
    return th


def scale_mass(theta, k):
    """other masses (k: one factor, or one per body) with the same centres of mass and the same inertias about them"""
    th = np.array(theta, dtype=np.float64).reshape(-1, 10)
    th[:, 0:4] *= np.reshape(np.asarray(k, dtype=np.float64), (-1, 1))
    return th


def mass_factors(P):
    """the "different mass" scenario: 1.5 times the mass, 3 times for a body that carries another one (object 1 of a contact
    between two bodies).  With equal factors a carried body as heavy as its carrier keeps a column of their contact attractive
    however the tray moves (-a_j' b has the sign of 1 / m1 - 1 / m2 under a downward pull), so the class "outside with z = 0" would
    be empty in the stacked arrangements."""
    k = np.full(P.nb, 1.5)
    for b1 in np.asarray(P.contact_body1):
        if b1 >= 0:
            k[b1] = 3.0
    return k


def scale_inertia(theta, k):
    th = np.array(theta, dtype=np.float64).reshape(-1, 10)
    th[:, 4:] *= k
    return th


def scenarios(P, rng=None, n=4):
    """nominal, a CoM-box vertex, a different mass, inertia x 0.1; further ones (n > 4) are random mixtures of the three."""
    th0 = np.asarray(P.body_params, dtype=np.float64)
    out = [th0.copy(), com_shift(th0, [0.02, -0.02, 0.03]), scale_mass(th0, mass_factors(P)), scale_inertia(th0, 0.1)]
    while len(out) < n:
        out.append(scale_inertia(scale_mass(com_shift(th0, rng.uniform(-0.03, 0.03, 3)), rng.uniform(0.5, 2.0)), rng.uniform(0.1, 2.0)))
    return np.stack(out[:n])


def study_sweep(theta, half_extents, inertia_scales=(1.0, 0.5, 0.1)):
    """The study's 45 scenarios (planning_sim_loop.py:548-559,613-616): the centre of mass at the centre, the 6 face centres and the
    8 vertices of its box (15), times three inertia scales.  [45][nb][10]."""
    h = np.asarray(half_extents, dtype=np.float64)
    offs = [np.zeros(3)]
    for a in range(3):
        for sgn in (1.0, -1.0):
            e = np.zeros(3); e[a] = sgn * h[a]; offs.append(e)
    offs += [(2.0 * np.array(v) - 1.0) * h for v in np.ndindex(2, 2, 2)]
    return np.stack([scale_inertia(com_shift(theta, d), k) for d in offs for k in inertia_scales])


# ---- points ---------------------------------------------------------------------------------------------------------------------
def state_for(O, q, v, a_ee, al_ee):
    """[q, v, qdd] whose end effector has the linear acceleration a_ee and the angular acceleration al_ee (world frame): both are
    affine in qdd, the least-norm solution of the 6 x nq system out of the oracle's kinematic Jacobian."""
    nq = q.size
    x = np.concatenate([q, v, np.zeros(nq)])
    ee, dee = O.ee_kinematics(x, jac=True)
    # ee: [p 3, C 9, v 3, w 3, a 3, al 3]
    J = np.concatenate([dee[18:21, 2 * nq:], dee[21:24, 2 * nq:]])
    rhs = np.concatenate([np.asarray(a_ee) - ee[18:21], np.asarray(al_ee) - ee[21:24]])
    x[2 * nq:] = np.linalg.lstsq(J, rhs, rcond=None)[0]
    return x


def level_q(P, rng, spread=0.25):
    """a configuration with a level tray (upright_amd/sampling.py: vertical axes free, the pitch chain sums to zero)"""
    if P.nq == 9:
        d = np.zeros(9)
        d[0:4] = rng.uniform(-spread, spread, 4); d[4:6] = rng.uniform(-spread, spread, 2); d[6] = -(d[4] + d[5])
        return THING_HOME + d
    d = np.zeros(6)
    d[0] = rng.uniform(-spread, spread); d[1:3] = rng.uniform(-spread, spread, 2); d[3] = -(d[1] + d[2])
    return THING_HOME[3:] + d


def points(P, kinds, seed, beyond=False):
    """One state per entry of `kinds` ("inside" | "outside" | "down" | "facet" | "lift"); beyond: the facet states are pushed 5 %
    further (the states just outside the facet)."""
    rng = np.random.default_rng(seed)
    O = Oracle(P)
    nq = P.nq
    mu = float(np.min(P.contact_mu))
    xs = []
    for kind in kinds:
        q = level_q(P, rng)
        if kind in ("facet", "lift"):
            # tray at rest; the specific force a - g the bodies feel, in the tray's frame: g0 (e_z + mu s) for a facet state (s a
            # pyramid axis of contact 0: what a level tray accelerating horizontally by exactly mu g produces -- the home pose is
            # level to 1 degree only, which alone would put the state 0.08 outside), k e_z for a lift state (a purely normal load:
            # inside the cone also without friction, nf = 1)
            x0 = np.concatenate([q, np.zeros(2 * nq)])
            Cm = O.ee_kinematics(x0)[3:12].reshape(3, 3)
            ez = np.array([0.0, 0.0, 1.0])
            if kind == "facet":
                s = np.asarray(P.contact_span)[0][int(rng.integers(2))] * (1.0 if rng.integers(2) else -1.0)
                f = G0 * (ez + (1.05 if beyond else 1.0) * float(P.contact_mu[0]) * s)
            else:
                f = rng.uniform(5.0, 14.0) * ez
            xs.append(state_for(O, q, np.zeros(nq), np.asarray(P.gravity) + Cm @ f, np.zeros(3)))
            continue
        q = q + rng.uniform(-0.03, 0.03, nq)          # a slightly tilted tray
        v = rng.uniform(-0.15, 0.15, nq)
        th = rng.uniform(0, 2 * np.pi)
        hdir = np.array([np.cos(th), np.sin(th), 0.0])
        if kind == "inside":
            a, al = rng.uniform(0.0, 0.3) * mu * G0 * hdir + np.array([0, 0, rng.uniform(-1, 1)]), rng.uniform(-0.3, 0.3, 3)
        elif kind == "outside":
            a, al = rng.uniform(2.0, 4.0) * max(mu, 0.2) * G0 * hdir + np.array([0, 0, rng.uniform(-2, 2)]), rng.uniform(-2, 2, 3)
        elif kind == "down":
            a, al = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), -G0 * rng.uniform(1.5, 2.5)]), rng.uniform(-0.2, 0.2, 3)
        else:
            raise ValueError(kind)
        xs.append(state_for(O, q, v, a, al))
    return np.stack(xs)


# ---- arrangements of the case table ------------------------------------------------------------------------------------------------
def arm_only_problem(arrangement, nf=3):
    """pink_bottle on the fixed-base UR10 (nq = 6): the chain is all the balance check reads besides the contact tables"""
    c = contacts_from_fixture(arrangement)
    nq, nu = 6, 6 + nf * len(c["contact_mu"])
    big = np.full(18, 10.0)
    return Problem(chain=robots.ur10(), nf=nf, Qdiag=np.zeros(18), Rdiag=np.ones(nu) * 1e-3, xd=np.zeros(18), x_lb=-big, x_ub=big,
                   u_lb=np.full(nu, -100.0), u_ub=np.full(nu, 100.0), **c).validate()


TABLE = (  # name, arrangement, kind of chain, nf, (nb, nc, ncol)
    ("pink_bottle", "pink_bottle", "thing", 3, (1, 4, 16)),
    ("pink_bottle_arm", "pink_bottle", "arm", 3, (1, 4, 16)),
    ("pink_bottle_nf1", "pink_bottle", "thing", 1, (1, 4, 4)),
    ("foam_die2", "foam_die2", "thing", 3, (2, 8, 32)),
    ("box_arch", "box_arch", "thing", 3, (3, 16, 64)),
    ("blue_cups", "blue_cups", "thing", 3, (7, 28, 112)),
    ("robust_8corner", "robust_8corner", "thing", 1, (8, 32, 32)),
)


# beyond the table: one-body shapes with more columns than the study's 16 -- the lane-per-job form keeps its column sets in two
# 64-bit masks: a fixture box (8 contacts, 32 columns: one word) and the bottle on twenty contact points (80 columns: both words)
EXTRA = (
    ("fixture_box", "simulation_box_with_fixture", "thing", 3, (1, 8, 32)),
    ("bottle_20_contacts", "pink_bottle_x5", "thing", 3, (1, 20, 80)),
)


def _bottle_x5(arr):
    """pink_bottle with every contact point repeated at 1, 0.9 .. 0.6 of its distance from the centre of the support"""
    import copy as _copy

    out = _copy.deepcopy(arr)
    cs = out["contacts"]
    mid2 = np.mean([c["r_co_o2"] for c in cs], axis=0)
    mid1 = np.mean([c["r_co_o1"] for c in cs], axis=0)
    new = []
    for k in (1.0, 0.9, 0.8, 0.7, 0.6):
        for c in cs:
            d = _copy.deepcopy(c)
            d["r_co_o2"] = (mid2 + k * (np.asarray(c["r_co_o2"]) - mid2)).tolist()
            d["r_co_o1"] = (mid1 + k * (np.asarray(c["r_co_o1"]) - mid1)).tolist()
            new.append(d)
    out["contacts"] = new
    return out


def table_problem(arrangements, name):
    row = [r for r in TABLE + EXTRA if r[0] == name][0]
    arr = _bottle_x5(arrangements["pink_bottle"]) if row[1] == "pink_bottle_x5" else arrangements[row[1]]
    P = arm_only_problem(arr, nf=row[3]) if row[2] == "arm" else thing_problem(arr, nf=row[3])
    assert (P.nb, P.nc, ncol(P)) == row[4], (name, P.nb, P.nc, ncol(P))
    return P


def build_case(arrangements, name):
    """The jobs of one arrangement: a list of launches dict(P, x [n][3 nq], params, per_point), with job counts n * n_scen in
    {256, 259, 37, 1} and both parameter layouts, and the zero-gravity launch of the free-fall class."""
    P = table_problem(arrangements, name)
    rng = np.random.default_rng(7 + sum(map(ord, name)))
    one_body = P.nb == 1
    calm = "inside" if P.nf == 3 else "lift"      # (without friction only a purely normal load is inside the cone)
    kinds = [calm] * 20 + ["outside"] * 24 + ["down"] * 12 + (["facet"] * 8 if one_body and P.nf == 3 else [calm] * 4 + ["outside"] * 4)
    seed = sum(map(ord, name))
    x = points(P, kinds, seed=seed)
    launches = [dict(P=P, x=x, params=scenarios(P), per_point=False, kinds=kinds)]                                  # 64 x 4 = 256
    if "facet" in kinds:    # the same states pushed 5 % further: the oracle must find them outside (the facet is a facet)
        launches[0]["x_beyond"] = points(P, kinds, seed=seed, beyond=True)
    k2 = ([calm, "outside", "down"] * 13)[:37]
    x2 = points(P, k2, seed=1 + sum(map(ord, name)))
    if name in [r[0] for r in TABLE]:
        per = np.stack([scenarios(P, rng, 37) for _ in range(7)])
    else:
        # (the shapes beyond the table: the four named scenarios in turn, rotated from point to point -- on random mixtures scipy
        #  1.15's nnls ends above lsq_linear and the kernel on five fixture_box jobs, by up to 3.7e-3, whatever the order or the
        #  scaling of the columns: the floor assertion of the CPU tests does not pass there, so those inputs are not used)
        per = np.stack([scenarios(P)[(np.arange(37) + i) % 4] for i in range(7)])
    launches.append(dict(P=P, x=x2[:7], params=per, per_point=True, kinds=k2[:7]))   # 7 x 37 = 259
    launches.append(dict(P=P, x=x2, params=scenarios(P)[1:2], per_point=False, kinds=k2))                            # 37 x 1
    launches.append(dict(P=P, x=x2[:37], params=np.stack([scenarios(P)[i % 4:i % 4 + 1] for i in range(37)]), per_point=True, kinds=k2))   # 37 x 1, per point
    launches.append(dict(P=P, x=x[21:22], params=scenarios(P)[:1], per_point=False, kinds=kinds[21:22]))              # 1 x 1
    launches.append(dict(P=P, x=x[21:22], params=scenarios(P)[None, 1:2], per_point=True, kinds=kinds[21:22]))        # 1 x 1, per point
    # free fall: no gravity, at rest -- b = 0 exactly
    P0 = copy.copy(P); P0.gravity = np.zeros(3)
    xf = np.stack([np.concatenate([level_q(P, rng) + rng.uniform(-0.2, 0.2, P.nq), np.zeros(2 * P.nq)]) for _ in range(2)])
    launches.append(dict(P=P0, x=xf, params=scenarios(P), per_point=False, kinds=["free_fall"] * 2))
    return launches


# scenarios of the main launch in which a facet state stays on the facet: nominal, other mass, other inertia (a moved centre of
# mass tips the bottle first: mu = 0.234 against a support half-width over height of 0.03 / 0.1275 = 0.2353)
FACET_SCENARIOS = (0, 2, 3)


def classify(ref, P, kinds=None):
    """Boolean masks over the jobs of one launch, from the reference's solution alone (and, for the facet class, the kind the point
    was built as)."""
    rho, z, bn = ref["rho"], ref["z"], ref["bnorm"]
    npass = (z > 0).sum(axis=-1)
    facet = np.zeros_like(rho, dtype=bool)
    if kinds is not None and rho.shape[1] == 4:
        rows = [i for i, k in enumerate(kinds) if k == "facet"]
        for s in FACET_SCENARIOS:
            facet[rows, s] = rho[rows, s] <= 1e-9
    return dict(inside=rho <= 1e-9, outside_passive=(rho >= 1e-2) & (npass > 0), outside_zero=(rho >= 1e-2) & (npass == 0) & (rho == bn),
                free_fall=bn == 0.0, full_rank=(npass == 6) & (P.nb == 1), facet=facet)


def expected_classes(P):
    """The classes an arrangement of the table can hold: a facet of the friction pyramid and six passive columns on one body need
    one body with friction (nf = 1 has four columns in all)."""
    c = ["inside", "outside_passive", "outside_zero", "free_fall"]
    if P.nb == 1 and P.nf == 3:
        c += ["facet", "full_rank"]
    return c


# ---- the kernel source through the host emulation, and the shared, cached table -----------------------------------------------------
def emu_lib():
    import ctypes as C
    import os
    from pathlib import Path

    E = C.CDLL(os.environ.get("UPR_BALANCE_EMU_LIB", str(Path(__file__).resolve().parent / "emu" / "libupr_balance_emu.so")))
    E.emu_bal_tol.restype = C.c_double
    return E


def run_emu(P, x, params, per_point, form=-1):
    """dict(rho, z, iters) of the projection job compiled for the host (tests/emu/upr_balance_emu.cpp), shapes of reference().
    form: -1 the form the library launches for P (one body: a lane per job, upr_bal_job1; else a wave per job, upr_bal_job),
    0 / 1 that form."""
    import ctypes as C

    from upright_amd import _capi

    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3 * P.nq)
    params = np.ascontiguousarray(params, dtype=np.float64)
    n, ns = x.shape[0], (params.shape[1] if per_point else params.shape[0])
    out = dict(rho=np.full((n, ns), np.nan), z=np.full((n, ns, ncol(P)), np.nan), iters=np.full((n, ns), -1, dtype=np.int32))
    cp = _capi.problem_to_c(P)
    rc = emu_lib().emu_bal_points(C.byref(cp), n, _capi.ptr(x), ns, _capi.ptr(params), 1 if per_point else 0, _capi.ptr(out["rho"]),
                                  _capi.ptr(out["z"]), _capi.iptr(out["iters"]), int(form))
    assert rc == 0
    return out


_CASES = {}


def cases(arrangements, name):
    """build_case(name) with the reference (key "ref") and the emulation's answer (key "emu") of every launch: computed once per
    session and shared by the tests; nothing modifies it."""
    if name not in _CASES:
        launches = build_case(arrangements, name)
        for L in launches:
            L["ref"] = reference(L["P"], L["x"], L["params"], L["per_point"])
            L["emu"] = run_emu(L["P"], L["x"], L["params"], L["per_point"])
            L["classes"] = classify(L["ref"], L["P"], L["kinds"])
        _CASES[name] = launches
    return _CASES[name]


def certificate(ref, z, tol):
    """Largest violation, in units of its bound, of the three optimality conditions of min_{z >= 0} |b + A z| over the jobs of a
    launch (no solver involved: b, A of the oracle and the z under test): z >= 0; a_j' r >= -10 tol |a_j| max(|b|, 1) for every
    column; |z_j a_j' r| <= the same bound times |z|_inf.  Returns (most negative z, worst dual ratio, worst complementarity
    ratio); the ratios must stay <= 1."""
    b, A = ref["b"], ref["A"]
    r = b + np.einsum("...mc,...c->...m", A, z)
    w = np.einsum("...mc,...m->...c", A, r)
    bound = 10.0 * tol * np.linalg.norm(A, axis=-2) * np.maximum(ref["bnorm"], 1.0)[..., None]
    zinf = np.abs(z).max(axis=-1)[..., None]
    dual = (-w / bound).max()
    comp = (np.abs(z * w) / np.maximum(bound * zinf, 1e-300)).max() if np.any(zinf > 0) else 0.0
    return float(z.min()), float(dual), float(comp)
