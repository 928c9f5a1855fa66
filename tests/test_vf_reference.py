"""CPU twin of tests/test_gpu_vf_screen.py: the cost-to-go matrices the SOURCE of upr_value_kernel writes (upr_vf_instance of
upright_amd/csrc/upr_value.h through the host emulation, one thread per workgroup) against the dense reference of tests/fb_check.py
(tests/vf_check.py: cost_to_go_reference), for every key of test_gpu_qp_screen.CASES and four more cases: the headline with an
end-effector box that binds (ee_box), the headline's point as the generic and the second-structure QP kernels leave it in their
workspaces (kind1, kind2: UPR_QP_KERNEL = 1 / 2 on the device) and the converged headline point of
test_value_function_batched._ctg_cases (converged).

The point: the one the QP exports after K_IT = 5 interior-point iterations at qp_tol = 0 (the inputs of tests/test_fb_reference.py,
FB_WAY_OFFSET included).  The cost-to-go kernel takes its weights from the exported point itself, so point and matrices come from
one run.  At that point the barrier weights are moderate and the recursion is well conditioned: every knot of every instance is held
to VF_TOL, relative to the knot's max |P_ref|.

VF_TOL holds per case 10 x max(a, h), two digits up, never above CAP = 1e-3: a the float64 dense reference against its 50-digit twin,
h value_function.riccati_value_function against that twin, both on instance 0 (N = 100: its last TAIL knots).  Both are float64
statements of the same matrices by two different factorisations and neither is the kernel; the factor 10 leaves room for a third
order of operations (FMA contraction, 256-lane sums, the Cholesky factor of S).  `python tests/test_vf_reference.py [case ...]`
measures a and h with the twin; the test itself runs float64 only.

Controls, on the reference alone: the point of one more iteration, zeroed weights of the state rows, lam / t in place of the
effective weight of softened rows each move P_k by at least ten thresholds -- the comparison would see such a defect."""
import copy
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import fb_check
import vf_check
from test_emu import Emu, _case, _knobs, _select
from test_fb_reference import CAP, K_IT, TAIL, fb_case
from test_gpu_qp_screen import CASES, RUN_TIME_HEADLINE, _arr, _ids
from test_value_function_batched import TOL_SUMS, _ctg_cases, _emu_cost_to_go, _export, _vf, host_cost_to_go, rel_err
from upright_amd.value_function import riccati_value_function, slot_active

EE_BOX, KIND1, KIND2, CONVERGED = "ee_box", "kind1", "kind2", "converged"
HEADLINE = RUN_TIME_HEADLINE
HEADLINE_ROWS = (9, 1, 4, 3, 20, True, False, False)
VF_CASES = list(CASES) + [EE_BOX, KIND1, KIND2, CONVERGED]

# case -> (threshold, a: float64 reference vs 50-digit twin, h: host module vs twin); threshold = 10 max(a, h), two digits up.
# Behind each: the emulated kernel against the float64 reference (worst knot and instance) | the device against the reference |
# the device against the emulation (tests/test_gpu_vf_screen.py)
VF_TOL = {
    (9, 1, 4, 3, 20, False, False, False): (7.3e-08, 7.22e-09, 7.21e-09),           # emulated 1.32e-08 | device 1.00e-08 | device vs emulated 8.47e-09
    (9, 1, 4, 3, 20, True, False, False): (2.9e-08, 1.83e-09, 2.81e-09),            # 6.92e-09 | 7.51e-09 | 2.32e-09
    (9, 1, 4, 3, 20, False, True, False): (1.7e-08, 1.64e-09, 1.62e-09),            # 7.58e-09 | 5.69e-09 | 9.59e-09
    (9, 1, 4, 3, 20, True, True, False): (3.3e-08, 3.27e-09, 3.28e-09),             # 6.65e-09 | 5.81e-09 | 5.78e-09
    (9, 1, 4, 1, 20, False, True, False): (7.5e-08, 7.41e-09, 5.85e-09),            # 1.10e-08 | 9.26e-09 | 5.23e-09
    (9, 8, 32, 1, 20, False, True, False): (1.0e-08, 9.91e-10, 8.09e-10),           # 1.64e-09 | 1.34e-09 | 3.27e-10
    (9, 3, 16, 3, 20, True, False, True): (5.4e-08, 4.83e-09, 5.32e-09),            # 1.05e-08 | 1.25e-08 | 1.24e-08
    (6, 1, 4, 1, 20, False, True, False): (2.3e-10, 1.64e-11, 2.26e-11),            # 3.56e-11 | 2.48e-11 | 9.36e-12
    (6, 1, 4, 1, 10, False, True, False): (6.8e-11, 2.46e-12, 6.77e-12),            # 7.28e-12 | 7.55e-12 | 3.11e-12
    (6, 1, 4, 3, 20, False, False, False): (2.0e-08, 1.75e-09, 1.92e-09),           # 5.80e-09 | 3.61e-09 | 5.54e-09
    (9, 2, 8, 3, 20, False, False, True): (4.2e-08, 4.15e-09, 4.13e-09),            # 9.02e-09 | 8.57e-09 | 1.14e-09
    (9, 7, 28, 3, 20, False, False, False): (4.4e-08, 4.36e-09, 4.37e-09),          # 9.06e-09 | 6.13e-09 | 7.22e-09
    (9, 8, 32, 1, 100, False, True, False): (5.7e-09, 5.66e-10, 5.66e-10),          # 1.00e-09 | 7.79e-10 | 6.22e-10 (target moved: VF_WAY_OFFSET)
    (9, 1, 4, 3, 12, False, False, False): (1.3e-08, 1.25e-09, 6.94e-10),           # 1.45e-09 | not run on the device
    EE_BOX: (3.8e-08, 3.78e-09, 3.78e-09),                                          # 7.41e-09 | 8.03e-09 | 1.42e-09
    KIND1: (7.2e-08, 7.15e-09, 7.13e-09),                                           # 1.32e-08 | 9.98e-09 | 8.49e-09
    KIND2: (7.2e-08, 7.11e-09, 7.11e-09),                                           # 1.32e-08 | 1.19e-08 | 8.50e-09
    # converged: a third term s = 8.88e-05, vf_check.schur_cholesky_statement (the kernel's route in float64 numpy) against the twin.
    # The kernel sits 9.55e-05 from the twin, the host module 6.08e-08: barrier weights to 9e8 beside h R = 1e-3 on the forces, and
    # S = Df Hff^-1 Df' + 1e-12 I formed explicitly loses what the indefinite stage system keeps.  The numpy statement of that route
    # lands at the same knot (2) at the same size on both instances (8.88e-05 / 5.64e-05 against the kernel's 9.55e-05 / 5.35e-05):
    # conditioning of the route, not a defect of the kernel's code ("The cost-to-go screen")
    CONVERGED: (8.9e-04, 6.40e-08, 6.08e-08),                                       # 9.55e-05 | host only
}
S_CONVERGED = 8.88e-05
# Pk of the device against the plain emulation's on the same records and point: cases that measure more than 1e-10 of the knot's
# largest entry get 3 x the measured value.  The reason is one for all of them: the plain emulation rounds every product, the device
# contracts a * b + c into one FMA, and the recursion carries the difference with cond(M) 1e6 .. 4e7.  Shown on the host: the
# emulation built with contraction on (vf_check.contracted_library) parts from the plain build by the figure in brackets, the
# device's own to two digits -- and the device is held against THAT build at 1e-10 (tests/test_gpu_vf_screen.py: measured 0, bit for
# bit, on the five frictionless cases, 9e-15 .. 4.2e-11 on the others).
EMU_TOL = {
    (9, 1, 4, 3, 20, False, False, False): 2.6e-08,     # measured 8.47e-09 (host builds: 8.53e-09)
    (9, 1, 4, 3, 20, True, False, False): 7.0e-09,      # 2.32e-09 (2.28e-09)
    (9, 1, 4, 3, 20, False, True, False): 2.9e-08,      # 9.59e-09 (9.55e-09)
    (9, 1, 4, 3, 20, True, True, False): 1.8e-08,       # 5.78e-09 (5.69e-09)
    (9, 1, 4, 1, 20, False, True, False): 1.6e-08,      # 5.23e-09 (5.23e-09)
    (9, 8, 32, 1, 20, False, True, False): 9.9e-10,     # 3.27e-10 (3.28e-10)
    (9, 3, 16, 3, 20, True, False, True): 3.8e-08,      # 1.24e-08 (1.24e-08)
    (6, 1, 4, 3, 20, False, False, False): 1.7e-08,     # 5.54e-09 (5.57e-09)
    (9, 2, 8, 3, 20, False, False, True): 3.5e-09,      # 1.14e-09 (1.14e-09)
    (9, 7, 28, 3, 20, False, False, False): 2.2e-08,    # 7.22e-09 (7.19e-09)
    (9, 8, 32, 1, 100, False, True, False): 1.9e-09,    # 6.22e-10 (6.22e-10)
    (9, 1, 4, 3, 12, False, False, False): 1.1e-09,     # not run on the device (host builds: 3.40e-10)
    EE_BOX: 4.3e-09,                                    # 1.42e-09 (1.44e-09)
    KIND1: 2.6e-08,                                     # 8.49e-09 (8.53e-09)
    KIND2: 2.6e-08,                                     # 8.50e-09 (8.50e-09)
}
# a case whose inputs fail a control gets its target moved by this offset (m), as tests/test_fb_reference.py's FB_WAY_OFFSET does
VF_WAY_OFFSET = {
    # the reference's horizon: with the QP screen's target no softened state box comes near its bound within five iterations --
    # without pairs 2.8e-9, wrong iterate 1.2e-7 before; 7.4e-3 and 5.1e-2 (worst instance each) with it
    (9, 8, 32, 1, 100, False, True, False): (-2.0, 1.0, 0.5),
}


def vf_ids(key):
    return key if isinstance(key, str) else _ids(key)


def vf_case(key, monkeypatch=None):
    """dict(P, x0, way, bp, xs0, us0, B, cfg): the inputs of a case at qp_tol = 0, qp_iter_max = K_IT (converged: at its own
    tolerance); cfg: the instantiation of the production kernel that solves it."""
    if key in CASES:
        c = dict(fb_case(key, monkeypatch), cfg=key)
        if key in VF_WAY_OFFSET:
            c["way"] = np.asarray(c["way"], dtype=float) + np.asarray(VF_WAY_OFFSET[key], dtype=float)
        return c
    if key in (KIND1, KIND2):
        return dict(fb_case(HEADLINE, monkeypatch), cfg=HEADLINE)
    if key == EE_BOX:      # the active box of tests/test_ee_box.py::test_one_sqp_iteration_with_an_active_box
        from test_ee_box import _with_box
        P, x0, way, xs, us = _case(_arr(), 2, 5, qp_tol=0.0, qp_iter_max=K_IT)
        _with_box(P)
        P.use_feedback_policy = True      # (as fb_case: the emulated entry also writes the gains)
        cfg = HEADLINE_ROWS
    else:
        assert key == CONVERGED, key
        P, x0, way, xs, us, _ = _ctg_cases(_arr(), "headline")
        cfg = HEADLINE
    B = x0.shape[0]
    bp = np.ascontiguousarray(np.broadcast_to(P.body_params, (B,) + np.shape(P.body_params)))
    return dict(P=P, x0=x0, way=way, bp=bp, xs0=np.ascontiguousarray(xs), us0=np.ascontiguousarray(us), B=B, cfg=cfg)


def _workspace_point(kind, c, lin, iters):
    """The generic (1) or second-structure (2) QP kernel's source for `iters` iterations and the point it leaves in its workspace:
    (sols, pairs, dx, du, raw) with raw = (ws, mult = ws, offsets) as upr_batch_value_function_update hands them to the kernel."""
    P = copy.copy(c["P"]); P.qp_iter_max = int(iters)
    B, N, n1 = c["B"], P.N, P.N + 1
    e = Emu(P, B, bp=c["bp"])
    nx, ne = e.nx, e.ne
    xs = np.ascontiguousarray(c["xs0"][:, :, :nx]); x0 = np.ascontiguousarray(c["x0"][:, :nx])
    dx, du, stats, ws = e.qp(kind, xs, c["us0"], x0, lin)
    assert np.all(stats[:, 1] == iters) and not np.any(stats[:, 2] == 2), stats[:, 1:3]
    offs = (C.c_int * 8)()
    if kind == 1:
        _vf().emu_vf_offsets(C.byref(e.cp), 1, offs)
        offs = np.array(list(offs), dtype=np.int32)
    else:
        r = _select(e.E, P, _knobs(qp_kernel=2))
        assert r["name"].startswith("upr_qp2_kernel"), r["name"]
        ni = 2 * nx + 2 * e.nu + (5 * P.nc if P.nf == 3 else 0) + fb_check.n_state_rows(P)
        offs = np.array([r["o_pi"], r["o_nu"], r["o_lam"], r["o_t"], r["o_sig"], r["o_tau"], r["o_gam"], ni], dtype=np.int32)
    assert offs[4] < 0      # (the headline has no softened rows)
    ni = int(offs[7])
    act = slot_active(P)
    sols = []
    for b in range(B):
        m = ws[b]
        blk = lambda o: m[o:o + n1 * ni].reshape(n1, ni)
        sols.append(dict(pi=m[offs[0]:offs[0] + n1 * nx].reshape(n1, nx).copy(), nu=m[offs[1]:offs[1] + N * ne].reshape(N, ne).copy(),
                         lam=np.where(act, blk(offs[2]), 0.0), slack=np.where(act, blk(offs[3]), 1.0)))
    return sols, [None] * B, dx.copy(), du.copy(), (ws, ws, offs)


def emulated_point(key, c, lin, iters=K_IT):
    """The primal-dual point of the case's QP on the emulated kernel source: dict(sol [B], pairs [B], dx, du, raw); raw: the kernel's
    inputs in the layout its QP kernel leaves them, where the case is about that layout (None: the packed point alone)."""
    P, B = c["P"], c["B"]
    if key in (KIND1, KIND2):
        sols, pairs, dx, du, raw = _workspace_point(1 if key == KIND1 else 2, c, lin, iters)
        return dict(sol=sols, pairs=pairs, dx=dx, du=du, raw=raw)
    if key == CONVERGED:
        e = Emu(P, B, bp=c["bp"])
        sols, pairs, stats, raw = _export(e, 3, c["xs0"], c["us0"], c["x0"], lin)
        assert np.all(stats[:, 2] == 0), stats[:, 2]
        return dict(sol=sols, pairs=pairs, dx=np.stack([s["dx"] for s in sols]), du=np.stack([s["du"] for s in sols]), raw=raw)
    r = fb_check.emu_qp3_cfg_fb(c["cfg"], P, B, c["xs0"], c["us0"], c["x0"], lin, c["bp"], iters)
    assert np.all(r["stats"][:, 1] == iters) and not np.any(r["stats"][:, 2] == 2), r["stats"][:, 1:3]
    return dict(sol=r["sol"], pairs=r["pairs"], dx=r["dx"], du=r["du"], raw=None)


def emulated_cost_to_go(c, lin, pt, raw=None, lib=None):
    """upr_vf_instance on the host for every instance of the case, on the packed point (or on `raw`): dict(Pk, pk, J, X).  lib: another
    build of the emulation (vf_check.contracted_library)."""
    P, B = c["P"], c["B"]
    e = Emu(P, B, bp=c["bp"])
    xs = np.ascontiguousarray(c["xs0"][:, :, :e.nx])
    if raw is None:
        raw = vf_check.pack_point(P, pt["sol"], pt["pairs"], pt["dx"], pt["du"])
    us, lin = np.ascontiguousarray(c["us0"]), np.ascontiguousarray(lin)
    return (_emu_cost_to_go(e, xs, us, lin, raw) if lib is None else vf_check.run_cost_to_go(lib, e, xs, us, lin, raw)), e


def vf_lds_bytes(nq, nb, nc, nf, N, no=0):
    """Dynamic LDS of upr_value_kernel for a shape: upr_vf_lds_layout restated (every block rounded up to an even count of doubles)."""
    nx, ne, nfc = 3 * nq, 6 * nb, nf * nc
    nu = nq + nfc
    ni = 2 * nx + 2 * nu + (5 * nc if nf == 3 else 0) + no
    blocks = [nx * nx] * 3 + [nq * nx] * 3 + [nq * nq] * 2 + [ne * nx] * 2 + [ne * ne] * 2 + [nfc * ne, 9 * nc if nf == 3 else nc, ni, N + 1, 2]
    return 8 * sum((n + 1) & ~1 for n in blocks)


def linearised(c):
    e = Emu(c["P"], c["B"], bp=c["bp"])
    return e.linearize(c["way"], np.zeros(c["B"]), c["xs0"], c["us0"])


def _softened(P):
    return any(bool((P.slacks or {}).get(k)) for k in ("state_box", "input_box", "poly_ineq"))


@pytest.mark.parametrize("key", VF_CASES, ids=vf_ids)
def test_emulated_cost_to_go_against_the_dense_reference(key, monkeypatch):
    """Linearise with the emulation, take the point of the emulated QP kernel after K_IT iterations, run the emulated cost-to-go kernel
    on the packed point.  Pk of every knot and instance under VF_TOL against the float64 dense reference and exactly symmetric; X
    exact; pk and J within TOL_SUMS of the host module's; no NaN.  Where the case is about a multiplier layout (kind1, kind2,
    converged) the kernel on the layout as its QP kernel leaves it returns the same bits as on the packed point.  The controls, on
    the reference alone, each at ten thresholds or more."""
    c = vf_case(key, monkeypatch)
    P, B, N = c["P"], c["B"], c["P"].N
    lin = linearised(c)
    pt = emulated_point(key, c, lin)
    dev, e = emulated_cost_to_go(c, lin, pt)
    assert vf_lds_bytes(P.nq, P.nb, P.nc, P.nf, N, fb_check.n_state_rows(P)) == 8 * _vf().emu_vf_lds_doubles(C.byref(e.cp))
    assert all(np.all(np.isfinite(v)) for v in dev.values()), {k: int((~np.isfinite(v)).sum()) for k, v in dev.items()}
    if pt["raw"] is not None:
        as_left, _ = emulated_cost_to_go(c, lin, pt, raw=pt["raw"])
        assert all(np.array_equal(as_left[k], dev[k]) for k in dev), [k for k in dev if not np.array_equal(as_left[k], dev[k])]
    tol = VF_TOL[key][0]
    assert tol <= CAP
    # the build with FMA contraction (where the host has one): under the same threshold, and no further from the plain build than the
    # device is allowed to be (the converged point is outside this: ill-conditioned, no device case)
    fma = vf_check.contracted_library() if key != CONVERGED else None
    if fma is not None:
        con, _ = emulated_cost_to_go(c, lin, pt, lib=fma)
        e_con = max(vf_check.pk_errors(con["Pk"][b], dev["Pk"][b]).max() for b in range(B))
        e_con_ref = max(vf_check.pk_errors(con["Pk"][b], vf_check.cost_to_go_reference(P, lin[b], pt["sol"][b], pt["pairs"][b], c["bp"][b])).max() for b in range(B))
        print("vf reference %s: contracted build vs plain build %.2e (tolerance %.1e)  vs reference %.2e" % (vf_ids(key), e_con, EMU_TOL.get(key, 1e-10), e_con_ref))
        assert e_con <= EMU_TOL.get(key, 1e-10), (e_con, EMU_TOL.get(key, 1e-10))
        assert e_con_ref < tol, (e_con_ref, tol)
    soft, rows = _softened(P), fb_check.n_state_rows(P) > 0
    nxt = emulated_point(key, c, lin, K_IT + 1) if key != CONVERGED else None
    worst = dict(Pk=0.0, pk=0.0, J=0.0, host=0.0)
    ctl = dict(iterate=np.inf, rows=np.inf, pairs=0.0)
    xs = c["xs0"][:, :, :e.nx]
    for b in range(B):
        sol, pairs, bp = pt["sol"][b], pt["pairs"][b], c["bp"][b]
        ref = vf_check.cost_to_go_reference(P, lin[b], sol, pairs, bp)
        worst["Pk"] = max(worst["Pk"], vf_check.pk_errors(dev["Pk"][b], ref).max())
        assert np.array_equal(dev["Pk"][b], np.swapaxes(dev["Pk"][b], 1, 2))
        assert np.array_equal(dev["X"][b], xs[b] + pt["dx"][b][:, :e.nx])
        host = host_cost_to_go(P, xs[b], c["us0"][b], lin[b], dict(sol, dx=pt["dx"][b][:, :e.nx], du=pt["du"][b]), e.Df[b], pairs)
        worst["pk"] = max(worst["pk"], rel_err(dev["pk"][b], host["pk"]))
        worst["J"] = max(worst["J"], rel_err(dev["J"][b], host["J"]))
        worst["host"] = max(worst["host"], vf_check.pk_errors(host["Pk"], ref).max())
        if key == CONVERGED:
            # the evidence behind this case's third term stays live: the numpy statement of the kernel's route misses the reference
            # where the kernel does (same order: within a factor 3 either way), the host module does not
            e_k = vf_check.pk_errors(dev["Pk"][b], ref)
            e_s = vf_check.pk_errors(vf_check.schur_cholesky_statement(P, lin[b], sol, pairs, bp), ref)
            print("converged, instance %d: kernel %.2e (knot %d)  numpy statement of its route %.2e (knot %d)" % (b, e_k.max(), e_k.argmax(), e_s.max(), e_s.argmax()))
            assert e_k.max() / 3.0 <= e_s.max() <= 3.0 * e_k.max() and e_k.argmax() == e_s.argmax(), (e_k.max(), e_s.max())
            assert vf_check.pk_errors(host["Pk"], ref).max() < 1e-2 * e_k.max()
        if nxt is not None:
            ctl["iterate"] = min(ctl["iterate"], vf_check.control_wrong_iterate(P, lin[b], sol, pairs, nxt["sol"][b], nxt["pairs"][b], bp, ref))
        if rows:
            ctl["rows"] = min(ctl["rows"], vf_check.control_zeroed_state_rows(P, lin[b], sol, pairs, bp, ref))
        if soft:
            ctl["pairs"] = max(ctl["pairs"], vf_check.control_without_pairs(P, lin[b], sol, pairs, bp, ref))
    print("vf reference %s: emulated vs reference %.2e (threshold %.1e)  host module vs reference %.2e  pk %.2e  J %.2e  controls: wrong iterate %.2e"
          "  zeroed state rows %.2e  without pairs %.2e" % (vf_ids(key), worst["Pk"], tol, worst["host"], worst["pk"], worst["J"], ctl["iterate"], ctl["rows"], ctl["pairs"]))
    assert worst["Pk"] < tol, (worst["Pk"], tol)
    assert worst["pk"] <= TOL_SUMS and worst["J"] <= TOL_SUMS, worst
    if nxt is not None:
        assert ctl["iterate"] >= 10.0 * tol, (ctl["iterate"], tol)
    if rows:
        assert ctl["rows"] >= 10.0 * tol, (ctl["rows"], tol)
    if soft:
        assert ctl["pairs"] >= 10.0 * tol, (ctl["pairs"], tol)


def test_table_reaches_every_form_of_the_cost_to_go_kernel():
    """Every case of the QP screen has a threshold here, and the table keeps the forms the kernel's run-time dimensions open up:
    nq = 6, 3 x 3 contact blocks on several bodies, a working set above the 64 KiB that need the raised LDS limit, state rows, softened
    inequality rows, a softened equality, horizons other than 20."""
    assert set(VF_TOL) == set(VF_CASES), set(VF_CASES) ^ set(VF_TOL)
    assert all(t[0] <= CAP and t[0] >= 10.0 * max(t[1], t[2]) for t in VF_TOL.values())
    assert VF_TOL[CONVERGED][0] >= 10.0 * S_CONVERGED
    keys = [k for k in VF_TOL if not isinstance(k, str)]
    assert any(k[0] == 6 for k in keys)
    assert any(k[3] == 3 and k[1] > 1 for k in keys)
    assert any(vf_lds_bytes(*k[:5]) > 64 * 1024 for k in keys) and any(vf_lds_bytes(*k[:5]) <= 64 * 1024 for k in keys)
    assert any(k[5] for k in keys) and EE_BOX in VF_TOL
    assert any(k[6] for k in keys)
    assert any(k[4] < 20 for k in keys) and any(k[4] > 20 for k in keys)
    soft_eq = []
    for k in keys:
        if k[6] and k[1] > 1:      # (the multi-body frictionless shapes: their builder softens the equality)
            sl = CASES[k][0](**{n: v for n, v in CASES[k][1].items() if n != "iters"})["P"].slacks or {}
            soft_eq.append(bool(sl.get("equality", sl.get("poly_ineq"))))
    assert any(soft_eq)


# ---- measuring a and h ----------------------------------------------------------------------------------------------------------------------
def measure_thresholds(key):
    """(a, h, threshold) of a case on instance 0 (N > 20: its last TAIL knots): the float64 dense reference and the host module
    against the 50-digit twin of the reference."""
    c = vf_case(key)
    P, N = c["P"], c["P"].N
    lin = linearised(c)
    pt = emulated_point(key, c, lin)
    sol, pairs, bp = pt["sol"][0], pt["pairs"][0], c["bp"][0]
    first = N - TAIL if N > 20 else 0
    twin = vf_check.cost_to_go_reference(P, lin[0], sol, pairs, bp, extended=True, first=first)
    ref = vf_check.cost_to_go_reference(P, lin[0], sol, pairs, bp)
    nx = ref.shape[1]
    host = riccati_value_function(P, c["xs0"][0][:, :nx], c["us0"][0], lin[0], dict(sol, dx=pt["dx"][0][:, :nx], du=pt["du"][0]),
                                  fb_check.friction_rows_of(P), vf_check.force_jacobian(P, bp), pairs=pairs)[0]
    dev, _ = emulated_cost_to_go(c, lin, pt)
    a, h = vf_check.pk_errors(ref[first:], twin).max(), vf_check.pk_errors(host[first:], twin).max()
    k = vf_check.pk_errors(dev["Pk"][0][first:], twin).max()
    t = 10.0 * max(a, h)
    if key == CONVERGED:      # the third term: the kernel's route in float64 numpy
        s = vf_check.pk_errors(vf_check.schur_cholesky_statement(P, lin[0], sol, pairs, bp), twin).max()
        print("converged: s (Schur complement and two Cholesky factors in numpy vs twin) %.2e" % s)
        t = 10.0 * max(a, h, s)
    unit = 10.0 ** (np.floor(np.log10(t)) - 1)
    return a, h, min(float("%.1e" % (np.ceil(t / unit) * unit)), CAP), k


if __name__ == "__main__":
    from test_emu import _NoDevice
    from upright_amd import control_bindings
    control_bindings.BatchMPC = _NoDevice      # (as fb_case does under pytest: no handle while a manager builds its Problem)
    for key in [k for k in VF_CASES if not sys.argv[1:] or vf_ids(k) in sys.argv[1:]]:
        a, h, t, k = measure_thresholds(key)
        print("%s: a %.2e  h %.2e  threshold %.1e  emulated vs twin %.2e" % (vf_ids(key), a, h, t, k), flush=True)
