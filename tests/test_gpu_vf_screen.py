"""Device screen of the cost-to-go kernel (upr_value_kernel of upright_amd/csrc/upr_value.h: one body, every dimension at run time,
256 lanes) at every shape the QP screen reaches: the 13 listed instantiations of tests/test_gpu_qp_screen.py, the headline with an
end-effector box that binds (the six box rows among the state rows) and the headline under UPR_QP_KERNEL = 1 and 2, whose
multipliers the kernel reads out of the instance workspace.  tests/test_vf_reference.py is the CPU twin: it holds the inputs of the
cases, the threshold table VF_TOL and the controls that keep the comparison from being empty.

Per case, one handle at qp_iter_max = K_IT, qp_tol = 0, on the device's own linearisation records and primal-dual point:
  (i)   Pk of every knot and instance against the dense reference of tests/fb_check.py (no code shared with the kernel), VF_TOL;
  (ii)  Pk against the SAME source on the host (one thread per workgroup, the point packed with offsets of its own: vf_check.pack_point)
        to 1e-10 of the knot's largest entry -- the race and indexing check -- for the build of the emulation that contracts
        a * b + c into an FMA as hipcc does (vf_check.contracted_library; a host without the instruction has no such build), and to
        test_vf_reference.EMU_TOL for the plain build, whose rounding of every product the recursion carries to 3e-10 .. 1.2e-8;
        pk and J at the rounding of their sums, X equal;
  (iii) Pk exactly symmetric, everything finite.
The run-time instantiated shape stays with the CPU twin: its export layout is the listed kernels', and compiling it takes longer
than a screen case should."""
import copy
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import vf_check
from test_gpu_fb_screen import KIND_NAME, _check_kernel, _time_at
from test_gpu_qp_screen import CASES, _ids
from test_value_function_batched import TOL_SUMS, numpy_query, rel_err
from test_value_function_tracked import _host_vf
from test_vf_reference import CAP, EE_BOX, EMU_TOL, K_IT, KIND1, KIND2, VF_TOL, _softened, emulated_cost_to_go, vf_case, vf_ids
from upright_amd.engine import BatchMPC

pytestmark = pytest.mark.gpu

DEVICE_CASES = [k for k in CASES if CASES[k][2] is None] + [EE_BOX, KIND1, KIND2]
UR10, ROBUST = (6, 1, 4, 1, 20, False, True, False), (9, 8, 32, 1, 20, False, True, False)


def _open(key, monkeypatch):
    """The case and its handle at K_IT iterations, the kernel name checked: (c, mpc)."""
    if key in (KIND1, KIND2):
        monkeypatch.setenv("UPR_QP_KERNEL", "1" if key == KIND1 else "2")
    c = vf_case(key)
    P = copy.copy(c["P"]); P.qp_iter_max = K_IT
    assert P.qp_tol == 0.0
    mpc = BatchMPC(P, c["B"], body_params=c["bp"], way_p=c["way"])
    try:
        _check_kernel(mpc, KIND_NAME["1" if key == KIND1 else "2"] if key in (KIND1, KIND2) else c["cfg"], None)
    except BaseException:
        mpc.close()
        raise
    return c, mpc


def _point(c, mpc):
    """One more QP on the handle (deterministic: it ends where the update's QP ended): (sols [B], pairs [B], kkt, lin), the iteration
    count and status required."""
    P, B = c["P"], c["B"]
    kkt = mpc.qp_kkt()
    pairs = mpc.qp_slack_pairs() if _softened(P) else None
    lin = mpc.lin_records()
    st = mpc.stats()
    assert np.all(st["qp_iters_last"] == K_IT), st["qp_iters_last"]
    assert not np.any(st["qp_status_last"] == 2), st["qp_status_last"]
    sols = [{k: kkt[k][b] for k in ("pi", "nu", "lam", "slack")} for b in range(B)]
    return sols, [None if pairs is None else tuple(q[b] for q in pairs) for b in range(B)], kkt, lin


@pytest.mark.parametrize("key", DEVICE_CASES, ids=vf_ids)
def test_cost_to_go_kernel_at_every_qp_shape(key, monkeypatch):
    c, mpc = _open(key, monkeypatch)
    P, B = c["P"], c["B"]
    try:
        mpc.set_observation(0.0, c["x0"])
        mpc.set_guess(c["xs0"], c["us0"])
        mpc.value_function_update()
        dev = mpc.cost_to_go()
        sols, pairs, kkt, lin = _point(c, mpc)
    finally:
        mpc.close()
    # (iii)
    assert all(np.all(np.isfinite(v)) for v in dev.values()), {k: int((~np.isfinite(v)).sum()) for k, v in dev.items()}
    assert np.array_equal(dev["Pk"], np.swapaxes(dev["Pk"], 2, 3))
    # (i) the dense reference on the device's records and point
    e_ref = max(vf_check.pk_errors(dev["Pk"][b], vf_check.cost_to_go_reference(P, lin[b], sols[b], pairs[b], c["bp"][b])).max() for b in range(B))
    # (ii) the same source on the host
    nx = P.nx
    pt = dict(sol=sols, pairs=pairs, dx=kkt["dx"][:, :, :nx], du=kkt["du"])
    emu, _ = emulated_cost_to_go(c, lin, pt)
    e_emu = max(vf_check.pk_errors(dev["Pk"][b], emu["Pk"][b]).max() for b in range(B))
    fma, e_con = vf_check.contracted_library(), 0.0
    if fma is not None:      # ... and built with FMA contraction, as the device code is: 1e-10 without exception
        con, _ = emulated_cost_to_go(c, lin, pt, lib=fma)
        e_con = max(vf_check.pk_errors(dev["Pk"][b], con["Pk"][b]).max() for b in range(B))
        print("vf screen %s: device vs the contracted build of the emulation %.2e (tolerance 1e-10)" % (vf_ids(key), e_con))
    e_pk = max(rel_err(dev["pk"][b], emu["pk"][b]) for b in range(B))
    e_J = max(rel_err(dev["J"][b], emu["J"][b]) for b in range(B))
    tol, tol_emu = VF_TOL[key][0], EMU_TOL.get(key, 1e-10)
    print("vf screen %s: device vs reference %.2e (threshold %.1e)  device vs emulated Pk %.2e (tolerance %.0e)  pk %.2e  J %.2e"
          % (vf_ids(key), e_ref, tol, e_emu, tol_emu, e_pk, e_J))
    assert tol <= CAP
    assert e_ref < tol, (e_ref, tol)
    assert e_emu <= tol_emu, (e_emu, tol_emu)
    assert e_con <= 1e-10, e_con
    assert e_pk <= TOL_SUMS and e_J <= TOL_SUMS, (e_pk, e_J)
    assert np.array_equal(dev["X"], emu["X"])


@pytest.mark.parametrize("key", [UR10, ROBUST], ids=_ids)
def test_queries_at_the_edges_of_the_plan(key, monkeypatch):
    """upr_value_query_kernel on nx = 18 (ur10_demo) and on ne = 48 (upright_robust: more rows than the 64 lanes of a point serve in one
    pass of nu(t)): value_function and equality_lagrangian at seven points, one time each, the instances taking turns -- before
    t0, exactly at t0, exactly on an inner knot, between knots, inside the last interval, exactly at t0 + N dt, past the horizon;
    states off the plan.  Against numpy on the downloaded cost-to-go (test_value_function_batched.numpy_query) and the host module's
    ValueFunction.equality_multiplier on the QP's own nu: 1e-12 relative (V: to |V|; dV/dx and nu: to the point's largest component)."""
    c, mpc = _open(key, monkeypatch)
    P, B, N, dt = c["P"], c["B"], c["P"].N, c["P"].dt
    t0 = -0.125      # (a plan that does not start at zero; the knot times below then have an exact quotient (t - t0) / dt)
    try:
        mpc.set_observation(t0, c["x0"])
        mpc.set_guess(c["xs0"], c["us0"])
        mpc.value_function_update()
        ctg = mpc.cost_to_go()
        s = np.array([-1.5, 0.0, 8.0, 11.3, N - 0.4, float(N), N + 0.7])
        t = np.array([t0 + v * dt if v != int(v) else _time_at(v, dt, t0) for v in s])
        inst = (np.arange(len(s)) % B).astype(np.int32)
        k = np.clip(np.round(s).astype(int), 0, N)
        x = ctg["X"][inst, k] + 1e-2 * np.random.default_rng(5).standard_normal((len(s), P.nx))
        xf = np.zeros((len(s), mpc.nxf)); xf[:, :P.nx] = x
        V, G = mpc.value_function(t, xf, inst)
        nu_t = mpc.equality_lagrangian(t, inst)
        _, _, kkt, _ = _point(c, mpc)
    finally:
        mpc.close()
    assert P.nx == 3 * key[0] and nu_t.shape[1] == 6 * key[1]
    assert all((t[i] - t0) / dt == s[i] for i in (1, 2, 5))
    Vn, Gn = numpy_query(P, ctg, np.full(B, t0), inst, t, x)
    assert np.abs(Vn).min() > 0
    e_V = (np.abs(V - Vn) / np.abs(Vn)).max()
    e_G = (np.abs(G[:, :P.nx] - Gn).max(axis=1) / np.abs(Gn).max(axis=1)).max()
    e_nu = 0.0
    for i in range(len(s)):
        want = _host_vf(P, t0, kkt["nu"][inst[i]]).equality_multiplier(t[i])
        assert np.abs(want).max() > 0
        e_nu = max(e_nu, np.abs(nu_t[i] - want).max() / np.abs(want).max())
    print("vf queries %s: V %.2e  dV/dx %.2e  nu(t) %.2e" % (_ids(key), e_V, e_G, e_nu))
    assert e_V < 1e-12 and e_G < 1e-12 and e_nu < 1e-12, (e_V, e_G, e_nu)
