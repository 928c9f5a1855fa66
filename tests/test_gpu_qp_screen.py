"""Fixed-iteration race / indexing screen of EVERY instantiation of the production QP kernel (upr_qp3_list.h) and of the run-time
instantiation (hiprtc).  The device solves k interior-point iterations (qp_tol = 0) on its own linearisation records; the same
source, compiled for the host at the instantiation the device ran (tests/emu, emu_qp3_cfg: one thread per workgroup), is fed
those records.  An interior-point method given a wrong Newton direction still converges -- only in more iterations -- so the
converged comparisons with the oracle cannot see an LDS race, a reduction whose host twin does something else or a wave-role
split that misses a row; after a fixed number of iterations such a defect shows up at 1e-3 and above.  1e-8 relative to
max |dx| leaves room for FMA contraction and the device's reciprocal / rsqrt rounding.

CASES maps every (nq, nb, nc, nf, N, ROWS, SOFT, DENSE) of the library's list to a builder; tests/test_emu.py
(test_every_qp_instantiation_has_a_screen_case) fails the CPU suite when an instantiation is added without one."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from upright_amd import _capi
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, stationary_guess, waypoints_for

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
EMU = HERE / "emu" / "libupr_emu.so"
KNAME = re.compile(r"upr_qp3_(kernel|jit)<upr_qp3_cfg<(\d+), (\d+), (\d+), (\d+), (\d+), 256, (true|false), (true|false), (true|false)>>")


def parse_qp_kernel(name):
    """(nq, nb, nc, nf, N, ROWS, SOFT, DENSE) of kernel_times()["qp_kernel"], and whether it is a run-time instantiation."""
    m = KNAME.fullmatch(name)
    assert m, name
    g = m.groups()
    return tuple(int(v) for v in g[1:6]) + tuple(v == "true" for v in g[6:]), g[0] == "jit"


def emu_qp3_cfg(cfg, P, B, xs, us, x0, lin, bp):
    """The production kernel's body at exactly instantiation cfg on the host: dx [B][N+1][nx], du [B][N][nu], stats [B][12]."""
    E = C.CDLL(str(EMU))
    E.emu_qp3_cfg.restype = C.c_long
    c = (C.c_int * 8)(*[int(v) for v in cfg])
    cp = _capi.problem_to_c(P)
    need = E.emu_qp3_cfg(c, None, B, None, None, None, None, None, None, C.c_long(0), None)
    assert need > 0, (cfg, need)
    dims = (C.c_int * 16)()
    E.emu_dims(C.byref(cp), dims)
    nx, nu, ne, ws_dx, ws_du, nfc = dims[0], dims[1], dims[2], dims[6], dims[7], dims[13]
    ws = np.full((B, need), np.nan)
    stats = np.zeros((B, _capi.NSTATS))
    bp = np.ascontiguousarray(bp)
    Df = np.zeros((B, ne, nfc))
    E.emu_make_Df(C.byref(cp), B, _capi.ptr(bp), _capi.ptr(Df))
    xs = np.ascontiguousarray(xs[:, :, :nx]); us = np.ascontiguousarray(us); x0 = np.ascontiguousarray(x0[:, :nx])
    lin = np.ascontiguousarray(lin)
    rc = E.emu_qp3_cfg(c, C.byref(cp), B, _capi.ptr(xs), _capi.ptr(us), _capi.ptr(x0), _capi.ptr(lin), _capi.ptr(Df),
                       _capi.ptr(ws), C.c_long(need), _capi.ptr(stats))
    assert rc == 0, (cfg, rc)
    n1, N = P.N + 1, P.N
    return ws[:, ws_dx:ws_dx + n1 * nx].reshape(B, n1, nx), ws[:, ws_du:ws_du + N * nu].reshape(B, N, nu), stats


# ---- the case builders: each returns dict(P, x0, way[, bp]) ----------------------------------------------------------------
def _arr():
    import json
    return json.load(open(HERE / "golden" / "arrangements.json"))


def _headline(B=6, seed=13, **kw):
    P = thing_problem(_arr()["pink_bottle"], **kw)
    x0 = level_tray_states(B, seed=seed)
    return dict(P=P, x0=x0, way=waypoints_for(P, x0))


def _obstacles(soft=False, **kw):
    from test_emu import _obstacle_case
    P, x0, way, _, _ = _obstacle_case(_arr(), 4, 4, **kw)
    if soft:
        P.slacks = dict(state_box=False, input_box=False, poly_ineq=True, equality=False, lower_L2_penalty=100.0, upper_L2_penalty=100.0)
    return dict(P=P, x0=x0, way=way)


def _soft_boxes(**kw):
    c = _headline(B=4, seed=61, **kw)
    c["P"].slacks = dict(state_box=True, input_box=True, poly_ineq=False, lower_L2_penalty=100.0, upper_L2_penalty=50.0, upper_L1_penalty=0.5)
    return c


def _robust(N=20, **kw):
    from test_gpu_parity import _robust_problem
    P, bp, x0, way = _robust_problem(_arr(), 4, N=N, **kw)
    return dict(P=P, x0=x0, way=way, bp=bp)


def _box_arch(**kw):
    from upright_amd import robots
    from upright_amd.problem import THING_HOME
    P = thing_problem(_arr()["box_arch"], **kw)
    for k, v in robots.collision_model(P.chain, robots.SIMPLE_COLLISION_PAIRS).items():
        setattr(P, k, v)
    x0 = np.tile(np.concatenate([THING_HOME, np.zeros(18)]), (4, 1))
    x0[:, 1] += [0.0, -0.05, 0.02, -0.02]
    return dict(P=P, x0=x0, way=waypoints_for(P, x0, offset=(-0.3, 0.3, 0.0)))


def _golden(name, arr="pink_bottle", level=False, override=None, **kw):
    """A golden merged config through the reference's manager, its Problem at three start states (joint rates perturbed)."""
    from test_gpu_parity import _level_tool, _manager_from_golden
    m = _manager_from_golden(name, _arr(), arr=arr, **(override or {}))
    P = m.mpc.problem
    if m.mpc._mpc is not None:
        m.mpc._mpc.close(); m.mpc._mpc = None
    x = np.array(m.settings.initial_state)
    if level:
        _level_tool(P.chain, x[:P.nq])
    for k, v in kw.items():
        setattr(P, k, v)
    B = 3
    x0 = np.tile(x, (B, 1))
    x0[:, P.nq:2 * P.nq] += np.random.default_rng(4).uniform(-0.05, 0.05, (B, P.nq))
    return dict(P=P, x0=x0, way=np.tile(np.asarray(P.way_p), (B, 1, 1)))


# (nq, nb, nc, nf, N, ROWS, SOFT, DENSE) -> (builder, kwargs, run-time instantiation); the first 13 are upr_qp3_list.h's own
CASES = {
    (9, 1, 4, 3, 20, False, False, False): (_headline, {"iters": 8}, None),                         # headline (test_qp_kernel_vs_host_emulation's case)
    (9, 1, 4, 3, 20, True, False, False): (_obstacles, {}, None),                                  # collision rows
    (9, 1, 4, 3, 20, False, True, False): (_soft_boxes, {}, None),                                 # slacks on the boxes
    (9, 1, 4, 3, 20, True, True, False): (_obstacles, {"soft": True}, None),                       # collision rows with slacks
    (9, 1, 4, 1, 20, False, True, False): (_golden, {"name": "thing_demo"}, None),                # thing_demo: nf 1, slacks
    (9, 8, 32, 1, 20, False, True, False): (_robust, {}, None),                                     # upright_robust 8-corner (config 4)
    (9, 3, 16, 3, 20, True, False, True): (_box_arch, {}, None),                                    # box_arch + collision rows (config 3)
    (6, 1, 4, 1, 20, False, True, False): (_golden, {"name": "ur10_demo", "level": True}, None),  # ur10_demo (config 1)
    (6, 1, 4, 1, 10, False, True, False): (_golden, {"name": "ur10_demo", "level": True, "override": {
        "mpc.time_horizon": 1.0, "waypoints": [{"time": 0, "position": [0.15, 0.1, 0.05], "orientation": [0, 0, 0, 1]}]}}, None),
    (6, 1, 4, 3, 20, False, False, False): (_golden, {"name": "full_bottle_arm_only"}, None),     # arm only, with friction
    (9, 2, 8, 3, 20, False, False, True): (_golden, {"name": "full_dice_point1", "arr": "foam_die2"}, None),   # stacked dice
    (9, 7, 28, 3, 20, False, False, False): (_golden, {"name": "full_cups_point1", "arr": "blue_cups"}, None),  # seven cups: BIGF
    (9, 8, 32, 1, 100, False, True, False): (_robust, {"N": 100}, None),                            # the reference's horizon: KFAR
    # run-time instantiations (hiprtc): a horizon outside the list, and the headline shape compiled at run time
    (9, 1, 4, 3, 12, False, False, False): (_headline, {"B": 4, "N": 12}, "1"),
}
RUN_TIME_HEADLINE = (9, 1, 4, 3, 20, False, False, False)
ITERS = 6   # (8 for the headline)
# screens that need more than 1e-8 (relative to max |dx|, |du|): measured value and reason
TOL = {
    # measured 1.6e-8 (dx) / 2.0e-8 (du): the largest step of the table (max |dx| 9.9: the target 2.2 m away at a horizon of 1.2 s)
    (9, 1, 4, 3, 12, False, False, False): 5e-8,
}
# the reported residuals against the emulation's, relative to themselves + 1e-9: measured at most 6.4e-6; where more, measured value and
# reason.  (Frictionless contacts: the equality residual of the proximal / softened rows sits a few decades above rounding after
# six iterations, where the device's reciprocal / rsqrt rounding shows in it.)
RES_TOL = {
    (6, 1, 4, 1, 20, False, True, False): 1e-2,    # measured 1.05e-3
    (6, 1, 4, 1, 10, False, True, False): 1e-2,    # measured 3.0e-4
    (9, 8, 32, 1, 100, False, True, False): 1e-2,  # measured 1.25e-3
}


def _ids(c):
    return "x".join(str(int(v)) for v in c)


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("jit"))


def _screen(cfg, builder, kw, jit, jit_cache, monkeypatch, tol, res_tol=1e-4):
    if jit is not None:
        monkeypatch.setenv("UPR_QP3_JIT", jit)
        monkeypatch.setenv("UPR_JIT_CACHE", jit_cache)
    kw = dict(kw)
    iters = kw.pop("iters", ITERS)
    c = builder(**kw, qp_tol=0.0, qp_iter_max=iters)
    P, x0, way = c["P"], c["x0"], c["way"]
    B = x0.shape[0]
    bp = c.get("bp")
    if bp is None:
        bp = np.ascontiguousarray(np.broadcast_to(P.body_params, (B,) + np.shape(P.body_params)))
    mpc = BatchMPC(P, B, body_params=bp, way_p=way)
    try:
        ran, is_jit = parse_qp_kernel(mpc.kernel_times()["qp_kernel"].replace("  ", " "))
        assert ran == cfg and is_jit == (jit is not None), (ran, cfg, mpc.kernel_times()["qp_kernel"])
        mpc.set_observation(0.0, x0)
        xs0, us0 = stationary_guess(x0, P.N, P.nu)
        mpc.set_guess(xs0, us0)
        dxs, dus = mpc.qp_step()
        st = mpc.stats()
        lin = mpc.lin_records()
    finally:
        mpc.close()
    dxe, due, se = emu_qp3_cfg(cfg, P, B, xs0, us0, x0, lin, bp)
    dxs = dxs[:, :, :P.nx]
    assert np.all(np.isfinite(dxe)) and np.all(np.isfinite(due))
    assert np.array_equal(st["qp_iters_last"], se[:, 1]) and np.array_equal(st["qp_status_last"], se[:, 2]), (st["qp_iters_last"], se[:, 1], se[:, 2])
    assert np.all(se[:, 1] == iters) or np.any(se[:, 2] == 2)
    ex = np.abs(dxs - dxe).max() / max(1.0, np.abs(dxe).max())
    eu = np.abs(dus - due).max() / max(1.0, np.abs(due).max())
    res = np.stack([st[k] for k in ("qp_res_stat", "qp_res_eq", "qp_res_ineq", "qp_res_comp")], axis=1)
    er = (np.abs(res - se[:, 6:10]) / (np.abs(se[:, 6:10]) + 1e-9)).max()
    print("screen %s: dx %.2e du %.2e res %.2e (tolerances %.0e, %.0e)" % (_ids(cfg), ex, eu, er, tol, res_tol))
    # (a race shows up at 1e-3 and above)
    assert ex < tol and eu < tol, (ex, eu)
    # the residuals the kernel reports: relative to themselves + 1e-9 (below that they sit at rounding level and differ freely)
    assert er < res_tol, er


@pytest.mark.parametrize("cfg", list(CASES), ids=_ids)
def test_qp_instantiation_fixed_iterations_vs_host_emulation(cfg, jit_cache, monkeypatch):
    builder, kw, jit = CASES[cfg]
    _screen(cfg, builder, kw, jit, jit_cache, monkeypatch, TOL.get(cfg, 1e-8), RES_TOL.get(cfg, 1e-4))


def test_run_time_instantiation_of_the_headline_shape_vs_host_emulation(jit_cache, monkeypatch):
    """UPR_QP3_JIT=2: the headline shape compiled by hiprtc at handle creation instead of the library's own code object -- the
    run-time compile path against the same emulation."""
    _screen(RUN_TIME_HEADLINE, _headline, {}, "2", jit_cache, monkeypatch, 1e-8)
