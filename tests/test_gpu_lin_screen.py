"""Screen of every launch form of the linearisation (upr_launch_select.h, upr_lin_plan): whole records, in trajectory mode (what
advance, qp_step and tick launch: knot, instance and time come from the point index, the terminal record is its own, dynamic
obstacles are predicted from the observation) and in points mode, against the numpy statement of tests/lin_check.py on the
oracle's terms, at the project's own tolerances (lin_check.TOL).  kernel_times()["lin_kernel"] names the instantiation the launch
ran; the last test asserts that the table reached every instantiation the plan can pick, at both chain lengths.

CASES maps a case to (builder, builder kwargs, environment at upr_batch_create, form the launch must pick).  A form is
("lin2", NQ) or ("lin", NQ, USE_MFMA, OCC, ORI, NPASS).  The builders give every instance its own inertial
parameters, targets and non-zero time, a trajectory in motion and (where there is one) its own obstacle and projectile flag, so
that every piece of addressing can fail visibly.  tests/test_lin_reference.py runs the same table through the host emulation;
tests/test_emu.py (test_every_linearisation_form_has_a_screen_case) fails the CPU suite when the list of instantiations gains
one without a case here, and test_lin_and_ls_selection_record holds the plan to the forms of this table on the host."""
import json
import os
import re
import sys
import time
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import lin_check  # noqa: E402
from upright_amd.sampling import stationary_guess  # noqa: E402

ORI_W = np.array([1.0, 1.0, 1.0, 0.3, 0.5, 0.2])
WAY_T2 = np.array([0.4, 1.6])     # two waypoints: the switch lies inside the 2 s horizon of every instance below


# ---- the case builders: each returns the case dict of lin_check ---------------------------------------------------------------
def _arr():
    return json.load(open(HERE / "golden" / "arrangements.json"))


def _finish(P, x0, way, seed, bp=None, way_q=None, dyn=None, pflag=None):
    """The case of (P, x0 [B][nx], way): per-instance inertial parameters (unless given), non-zero times, a trajectory in motion
    (stationary guess + uniform +-0.3 on q, v, a; joint inputs in +-1, forces in +-3)."""
    rng = np.random.default_rng(seed)
    B, nx = x0.shape[0], P.nx
    if bp is None:     # mass, first moments and inertia of every body scaled by up to 5 %, differently per instance
        bp = np.asarray(P.body_params)[None] * (1.0 + 0.05 * rng.uniform(-1, 1, (B,) + np.shape(P.body_params)))
    xs, us = stationary_guess(x0[:, :nx], P.N, P.nu)
    xs = xs + rng.uniform(-0.3, 0.3, xs.shape)
    us = np.concatenate([rng.uniform(-1, 1, (B, P.N, P.nq)), rng.uniform(-3, 3, (B, P.N, P.nu - P.nq))], axis=2)
    t0 = 0.05 + 0.13 * (np.arange(B) % 17)
    way = np.asarray(way, dtype=np.float64).reshape(B, -1, 3) + (np.arange(B) % 11)[:, None, None] * np.array([0.05, -0.03, 0.02])   # every instance its own targets
    c = dict(P=P, bp=np.ascontiguousarray(bp), way=np.ascontiguousarray(np.asarray(way, dtype=np.float64).reshape(B, -1, 3)),
             way_q=None if way_q is None else np.ascontiguousarray(way_q), t0=np.ascontiguousarray(t0),
             xs=np.ascontiguousarray(xs), us=np.ascontiguousarray(us), dyn=None if dyn is None else np.ascontiguousarray(dyn),
             pflag=None if pflag is None else np.ascontiguousarray(pflag, dtype=np.float64))
    assert c["way"].shape[1] == len(P.way_t)
    return c


def _two_waypoints(P, way):
    P.way_t = WAY_T2.copy()
    way = np.asarray(way).reshape(len(way), -1, 3)[:, 0]
    return np.stack([way, way + np.array([0.3, -0.2, 0.1])], axis=1)


def _targets_near(P, x0, seed):
    """target orientations (xyzw) a moderate rotation (|axis-angle| about 0.3) away from the orientation at x0, per waypoint"""
    from upright_amd.control import quat_multiply_xyzw, rot_to_quat_xyzw
    rng = np.random.default_rng(seed)
    B, nw = x0.shape[0], len(P.way_t)
    q = np.zeros((B, nw, 4))
    for b in range(B):
        qe = rot_to_quat_xyzw(P.chain.forward(x0[b, :P.nq])[1])
        for w in range(nw):
            dq = np.concatenate([0.15 * rng.normal(size=3), [1.0]])
            q[b, w] = quat_multiply_xyzw(qe, dq / np.linalg.norm(dq))
    return q


def _with_box(P):
    P.ee_box, P.ee_box_lower, P.ee_box_upper = True, np.array([-0.5, -1.5, -0.1]), np.array([2.5, 0.5, 0.1])


def _thing(arr="pink_bottle", B=3, seed=13, box=False, ori=False, rows=None, two=False):
    """Thing with an arrangement of tests/golden/arrangements.json; rows: None, "simple" (obstacles/simple.yaml's 20 pairs) or
    "small" (test_emu._obstacle_case: a world sphere, two self-collision pairs, a far pair)."""
    from upright_amd import robots
    from upright_amd.problem import thing_problem
    from upright_amd.sampling import level_tray_states, waypoints_for
    P = thing_problem(_arr()[arr])
    x0 = level_tray_states(B, seed=seed)
    way = waypoints_for(P, x0, offset=(-0.5, 0.5, 0.0))
    if rows == "simple":
        for k, v in robots.collision_model(P.chain, robots.SIMPLE_COLLISION_PAIRS).items():
            setattr(P, k, v)
    elif rows == "small":
        from test_emu import _obstacle_case
        P, _, _, _, _ = _obstacle_case(_arr(), B, 4)
    if two or ori:
        way = _two_waypoints(P, way)
    way_q = None
    if ori:
        P.Wee = ORI_W.copy()
        way_q = _targets_near(P, x0, seed + 1)
    if box:
        _with_box(P)
    return _finish(P, x0, way, seed + 2, way_q=way_q)


def _robust(N=20):
    from test_gpu_parity import _robust_problem
    P, bp, x0, way = _robust_problem(_arr(), 4, N=N)
    return _finish(P, x0, way, 31, bp=bp)


def _golden(name, arr="pink_bottle", ori=False, rows=False, seed=41):
    """A golden merged config through the controller manager (the fixed-base UR10 shapes: nq = 6); rows: a small collision
    model on the arm (a self-collision pair, wrist against the ground, the tray's link against a world sphere)."""
    from test_gpu_qp_screen import _golden as qp_golden
    from upright_amd import robots
    g = qp_golden(name, arr=arr, level=(name == "ur10_demo"))
    P, x0 = g["P"], g["x0"]
    way = g["way"]
    if rows:
        p0 = P.chain.forward(x0[0, :P.nq])[0]
        pairs = [("wrist1_collision_link", "shoulder_collision_link"), ("wrist3_collision_link", "ground"), ("balanced_object_collision_link", "obs_a")]
        for k, v in robots.collision_model(P.chain, pairs, spheres={"obs_a": ("world", tuple(p0 + np.array([0.6, 0.5, 0.3])), 0.15)}).items():
            setattr(P, k, v)
    way_q = None
    if ori:
        P.Wee = ORI_W.copy()
        way = _two_waypoints(P, way)
        way_q = _targets_near(P, x0, seed + 1)
    return _finish(P, x0, way, seed, way_q=way_q)


def _thrown_ball():
    """test_emu._projectile_case: a ball as dynamic obstacle, collision rows and a projectile-path row; the flag on for instances
    0 and 2, off for instance 1; every instance its own ball"""
    from test_emu import _projectile_case
    P, x0, way, _, _, dyn = _projectile_case(_arr(), 3)
    return _finish(P, x0, way, 51, dyn=dyn, pflag=[1.0, 0.0, 1.0])


def _two_obstacles():
    """tests/test_gpu_parity.py test_two_dynamic_obstacles: a drifting chair (obstacle 0) and the thrown ball (obstacle 1, the one
    the projectile row follows)"""
    from test_emu import _projectile_case
    from upright_amd import robots
    B = 3
    P, x0, way, _, _, ball = _projectile_case(_arr(), B)
    pairs = [("wrist1_collision_link_0", "shoulder_collision_link_0"), ("wrist3_collision_link_0", "ground"),
             ("base_collision_link_0", "chair1"), ("forearm_collision_sphere_link2_0", "projectile1"), ("balanced_object_collision_link_0", "chair1")]
    for k, v in robots.collision_model(P.chain, pairs, dynamic={"chair1": 0.25, "projectile1": 0.2}).items():
        setattr(P, k, v)
    P.n_dyn = 2
    P.proj_sph = np.zeros(0, dtype=np.int32); P.proj_dist = np.zeros(0)
    robots.add_projectile_rows(P, ["balanced_object_collision_link"], [0.35], 0.2)
    p0, _ = P.chain.forward(x0[0, :9])
    chair = np.tile(np.concatenate([p0 * [1, 1, 0] + [0.9, -0.5, 0.25], [0.0, 0.15, 0.0], [0.02, 0.0, 0.0]]), (B, 1))
    chair[:, :2] += [[0.0, 0.0], [0.1, -0.1], [-0.1, 0.15]]
    return _finish(P, x0, way, 53, dyn=np.concatenate([chair, ball], axis=1), pflag=[0.0, 1.0, 1.0])


LIN2_OFF, NO_MFMA = {"UPR_LIN2": "0"}, {"UPR_LIN_MFMA": "0"}
OCC3, OCC4 = {"UPR_LIN_OCC": "3"}, {"UPR_LIN_OCC": "4"}
PASSES1, PASSES3 = dict(LIN2_OFF, UPR_LIN_ROW_PASSES="1"), dict(LIN2_OFF, UPR_LIN_ROW_PASSES="3")
ARM, UR10 = {"name": "full_bottle_arm_only"}, {"name": "ur10_demo"}
# case -> (builder, kwargs, environment at upr_batch_create, form)
CASES = {
    "headline_B37": (_thing, {"B": 37}, {}, ("lin2", 9)),          # 777 knots: 27 workgroups of 28 and one of 21
    "headline_B1024": (_thing, {"B": 1024}, {}, ("lin2", 9)),      # 768 workgroups, the launch the bench times
    "ur10_demo": (_golden, UR10, {}, ("lin2", 6)),                 # nq 6, nf 1
    "arm_only": (_golden, ARM, {}, ("lin2", 6)),                   # nq 6, nf 3
    "robust_N20": (_robust, {}, {}, ("lin2", 9)),
    "robust_N100": (_robust, {"N": 100}, {}, ("lin2", 9)),
    "cups": (_thing, {"arr": "blue_cups"}, {}, ("lin2", 9)),
    "dice": (_thing, {"arr": "foam_die2"}, {}, ("lin2", 9)),
    "box_arch_rows": (_thing, {"arr": "box_arch", "rows": "simple", "B": 4}, {}, ("lin2", 9)),
    "collision_rows": (_thing, {"rows": "small", "B": 4}, {}, ("lin2", 9)),
    "ur10_collision_rows": (_golden, dict(UR10, rows=True), {}, ("lin2", 6)),
    "thrown_ball": (_thrown_ball, {}, {}, ("lin2", 9)),
    "two_obstacles": (_two_obstacles, {}, {}, ("lin2", 9)),
    "box_only": (_thing, {"box": True, "two": True}, {}, ("lin2", 9)),
    "box_collision_rows": (_thing, {"rows": "small", "box": True, "B": 4}, {}, ("lin2", 9)),
    "orientation": (_thing, {"ori": True}, {}, ("lin", 9, True, 2, True, 1)),
    "orientation_ur10": (_golden, dict(UR10, ori=True), {}, ("lin", 6, True, 2, True, 1)),
    "orientation_box": (_thing, {"ori": True, "box": True}, {}, ("lin", 9, True, 2, True, 1)),
    # forms chosen per handle
    "headline_lin2_off": (_thing, {"B": 37}, LIN2_OFF, ("lin", 9, True, 2, False, 3)),
    "collision_rows_lin2_off": (_thing, {"rows": "small", "B": 4}, LIN2_OFF, ("lin", 9, True, 2, False, 2)),
    "arm_only_lin2_off": (_golden, ARM, LIN2_OFF, ("lin", 6, True, 2, False, 3)),
    "ur10_collision_rows_lin2_off": (_golden, dict(UR10, rows=True), LIN2_OFF, ("lin", 6, True, 2, False, 2)),
    "headline_no_mfma": (_thing, {"B": 5}, NO_MFMA, ("lin", 9, False, 2, False, 1)),
    "arm_only_no_mfma": (_golden, ARM, NO_MFMA, ("lin", 6, False, 2, False, 1)),
    "orientation_no_mfma": (_thing, {"ori": True}, NO_MFMA, ("lin", 9, False, 2, True, 1)),
    "orientation_ur10_no_mfma": (_golden, dict(UR10, ori=True), NO_MFMA, ("lin", 6, False, 2, True, 1)),
    # forms behind the A/B knobs UPR_LIN_OCC and UPR_LIN_ROW_PASSES: two small cases per value
    "headline_occ3": (_thing, {"B": 5}, OCC3, ("lin", 9, True, 3, False, 1)),
    "arm_only_occ3": (_golden, ARM, OCC3, ("lin", 6, True, 3, False, 1)),
    "headline_occ4": (_thing, {"B": 5}, OCC4, ("lin", 9, True, 4, False, 1)),
    "arm_only_occ4": (_golden, ARM, OCC4, ("lin", 6, True, 4, False, 1)),
    "collision_rows_passes1": (_thing, {"rows": "small", "B": 4}, PASSES1, ("lin", 9, True, 2, False, 1)),
    "ur10_collision_rows_passes1": (_golden, dict(UR10, rows=True), PASSES1, ("lin", 6, True, 2, False, 1)),
    "collision_rows_passes3": (_thing, {"rows": "small", "B": 4}, PASSES3, ("lin", 9, True, 2, False, 3)),
    "ur10_collision_rows_passes3": (_golden, dict(UR10, rows=True), PASSES3, ("lin", 6, True, 2, False, 3)),
}
KNOBS = sorted({(k, v[2][k]) for v in CASES.values() for k in ("UPR_LIN_OCC", "UPR_LIN_ROW_PASSES") if k in v[2]})
# knots per workgroup of upr_linearize2_kernel: 28 for the headline shape (768 workgroups at B = 1024), 256 / NQ at most
KPW = {"headline_B37": (28, 28), "headline_B1024": (28, 768)}     # case -> (kpw, workgroups) in trajectory mode
RAGGED = ("headline_B37", "ur10_demo", "arm_only")                # the last workgroup of the trajectory-mode launch is not full
LIN2_NAME = re.compile(r"upr_linearize2_kernel<(\d+)> kpw=(\d+) blocks=(\d+)")
LIN_NAME = re.compile(r"upr_linearize_kernel<(\d+), (true|false), (\d+), (true|false), (\d+)>")


def build_case(name):
    builder, kw = CASES[name][:2]
    return builder(**kw)


def parse_lin_kernel(name):
    """kernel_times()["lin_kernel"] -> (form, kpw, workgroups) (the latter two None for upr_linearize_kernel)"""
    m = LIN2_NAME.fullmatch(name)
    if m:
        return ("lin2", int(m.group(1))), int(m.group(2)), int(m.group(3))
    m = LIN_NAME.fullmatch(name)
    assert m, name
    g = m.groups()
    return ("lin", int(g[0]), g[1] == "true", int(g[2]), g[3] == "true", int(g[4])), None, None


def obstacle_at(dyn, tau):
    """[r, v, a] blocks of dyn (.., 9 n) propagated ballistically by tau"""
    d = np.asarray(dyn, dtype=np.float64).reshape(-1, 9)
    out = np.concatenate([d[:, :3] + tau * d[:, 3:6] + 0.5 * tau * tau * d[:, 6:], d[:, 3:6] + tau * d[:, 6:], d[:, 6:]], axis=1)
    return out.reshape(np.shape(dyn))


def run_on_device(c, env):
    """(records of the trajectory-mode launch, its kernel name, points-mode output in lin_check's shape, its kernel name)"""
    from upright_amd.engine import BatchMPC
    P = c["P"]
    B, N, nx = c["xs"].shape[0], P.N, P.nx
    xs = c["xs"]
    if c["dyn"] is not None:    # interface states carry the observed obstacle; trajectory mode predicts it from the observation
        xs = np.concatenate([xs, np.repeat(c["dyn"][:, None, :], N + 1, axis=1)], axis=2)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        mpc = BatchMPC(P, B, body_params=c["bp"], way_p=c["way"], way_q=c["way_q"])
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        assert mpc.kernel_times()["lin_kernel"] == ""
        if c["pflag"] is not None:
            mpc.set_projectile_flag(c["pflag"])
        mpc.set_observation(c["t0"], xs[:, 0])
        mpc.set_guess(xs, c["us"])
        mpc.qp_step()
        lin = mpc.lin_records()
        name_t = mpc.kernel_times()["lin_kernel"]
        # the same knots in points mode: instance, time and (predicted) obstacle of every point explicit
        X = xs[:, :N].copy()
        if c["dyn"] is not None:
            for k in range(N):
                X[:, k, nx:] = obstacle_at(c["dyn"], k * P.dt)
        inst = np.repeat(np.arange(B), N).reshape(B, N)
        t = c["t0"][:, None] + np.arange(N)[None, :] * P.dt
        out = mpc.linearize_points(X.reshape(B * N, -1), c["us"].reshape(B * N, -1), t.ravel(), inst.ravel())
        rows = None
        if P.n_state_rows:
            rows = mpc.state_rows(X[:, 1:].reshape(B * (N - 1), -1), t[:, 1:].ravel(), inst[:, 1:].ravel())
        name_p = mpc.kernel_times()["lin_kernel"]
    finally:
        mpc.close()
    return lin, name_t, lin_check.split_points(P, B, out, rows), name_p


def screen_case(name):
    """One case on the device: dict(name_t, name_p, traj, points: {slot class: (error, instance, knot)}, seconds)"""
    tic = time.time()
    c = build_case(name)
    expected = lin_check.expected_records(c)
    lin, name_t, pts, name_p = run_on_device(c, CASES[name][2])
    allow = lin_check.projectile_allowance(c)
    got = lin_check.split_records(c["P"], lin)
    traj = lin_check.compare(expected, got, allowance=allow)
    points = lin_check.compare(expected, pts, allowance=allow)
    r = dict(name_t=name_t, name_p=name_p, traj=traj, points=points, npoints=lin.shape[0] * lin.shape[1])
    if allow is not None:     # for the record: the projectile rows' error before their rounding allowance, and the allowance there
        raw = lin_check.compare(expected, got, slots=("rows", "row_grad"))
        r["raw"] = {k: v + (float(allow[k][v[1], v[2] - 1].max()),) for k, v in raw.items()}
    r["seconds"] = time.time() - tic
    return r


def check_result(name, r, reached):
    form = CASES[name][3]
    print("%s: %s | points mode: %s (%.1f s)" % (name, r["name_t"], r["name_p"], r["seconds"]))
    print("   trajectory mode: %s" % lin_check.fmt(r["traj"]))
    print("   points mode:     %s" % lin_check.fmt(r["points"]))
    if r.get("raw"):
        print("   before the projectile rows' rounding allowance (error, instance, knot, allowance there): %s" % r["raw"])
    ran, kpw, blocks = parse_lin_kernel(r["name_t"])
    reached[name] = r["name_t"]
    assert ran == tuple(form), (name, r["name_t"], form)
    assert parse_lin_kernel(r["name_p"])[0] == tuple(form), (name, r["name_p"], form)
    if ran[0] == "lin2":
        assert 1 <= kpw <= 256 // ran[1] and blocks == -(-r["npoints"] // kpw), (r["name_t"], r["npoints"])
        if name in KPW:
            assert (kpw, blocks) == KPW[name], r["name_t"]
        if name in RAGGED:
            assert r["npoints"] % kpw != 0, (r["name_t"], r["npoints"])
    slots = set(lin_check.SLOTS) - (set() if has_rows(name) else {"rows", "row_grad"})     # every slot class was compared
    assert slots == set(r["traj"]) and slots - {"term_c", "term_C"} == set(r["points"]), (sorted(r["traj"]), sorted(r["points"]))
    bad = {"trajectory": lin_check.failures(r["traj"]), "points": lin_check.failures(r["points"])}
    assert not bad["trajectory"] and not bad["points"], (name, bad)


def has_rows(name):
    kw = CASES[name][1]
    return bool(kw.get("rows") or kw.get("box")) or CASES[name][0] in (_thrown_ball, _two_obstacles)


@pytest.fixture(scope="module")
def reached():
    seen = {}
    yield seen
    print("linearisation kernels reached:")
    for n in sorted(set(seen.values())):
        print("   ", n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_linearisation_records_against_the_oracle(name, reached):
    check_result(name, screen_case(name), reached)


@pytest.mark.gpu
def test_the_table_reaches_every_linearisation_instantiation(reached):
    """Both chain lengths and every instantiation the plan can pick were launched by the cases above."""
    assert set(reached) == set(CASES), "run the whole module: %s" % sorted(set(CASES) - set(reached))
    forms = {parse_lin_kernel(n)[0] for n in reached.values()}
    want = {("lin2", nq) for nq in (6, 9)} | {("lin", nq) + f for nq in (6, 9) for f in (
        (True, 2, True, 1), (False, 2, True, 1), (False, 2, False, 1), (True, 3, False, 1), (True, 4, False, 1), (True, 2, False, 3),
        (True, 2, False, 2), (True, 2, False, 1))}
    assert forms == want, (sorted(want - forms), sorted(forms - want))

