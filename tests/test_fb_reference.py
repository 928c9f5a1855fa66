"""CPU twin of tests/test_gpu_fb_screen.py: the feedback gains the production QP kernel's SOURCE writes (write_feedback of upr_qp3.h,
through the exact-instantiation entry emu_qp3_cfg_fb of the host emulation) against the dense reference of tests/fb_check.py, for
every key of test_gpu_qp_screen.CASES.

Which iterate: the kernel writes K from the factorisation of the LAST EXECUTED interior-point iteration, that is of the iterate before
the last step, while the exported point is the iterate after it.  In the fixed-iteration regime (qp_tol = 0) the point exported with
qp_iter_max = k is the point the run with qp_iter_max = k + 1 factors: the reference takes the point of the first run, the gains come
from the second (K_IT = 5: the gains run is the six iterations of the QP screen).  The negative control feeds the reference the point
of the k + 1 run instead: it must miss by at least ten times the case's threshold.

Compared per knot and per block (jerk rows [:nq], force rows [nq:]) relative to the block's max |K_ref|; every (knot, block) of every
instance takes part.  FB_TOL holds per case 10 x max(a, b), a: the float64 reference against its extended-precision twin (mpmath, 50
digits), b: the emulated gains against that twin, both on instance 0 (N = 100: its last ten knots); never above CAP = 1e-3."""
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import fb_check
from kkt_check import force_jacobian
from test_emu import Emu, _NoDevice
from test_gpu_qp_screen import CASES, _ids
from upright_amd.sampling import stationary_guess
from upright_amd.value_function import riccati_value_function

K_IT = 5          # the exported point: after five iterations; the gains: of the sixth factorisation (ITERS of the QP screen)
CAP = 1e-3        # no threshold above this fraction of the block scale: every indexing defect shows at order one
TAIL = 10         # N = 100: the extended-precision twin runs the last ten knots of instance 0

# case -> (threshold, measured a: float64 reference vs twin, measured b: emulated gains vs twin); threshold = 10 max(a, b), two digits up
FB_TOL = {
    (9, 1, 4, 3, 20, False, False, False): (3.4e-08, 3.40e-09, 1.62e-09),         # worst instance 4.99e-09, wrong iterate 2.53e-01
    (9, 1, 4, 3, 20, True, False, False): (5.6e-08, 3.29e-09, 5.56e-09),          # worst instance 6.62e-09, wrong iterate 4.39e-01
    (9, 1, 4, 3, 20, False, True, False): (4.0e-08, 2.76e-09, 3.96e-09),          # worst instance 4.93e-09, wrong iterate 2.40e-01
    (9, 1, 4, 3, 20, True, True, False): (5.1e-08, 2.60e-09, 5.02e-09),           # worst instance 4.89e-09, wrong iterate 5.22e-01
    (9, 1, 4, 1, 20, False, True, False): (5.4e-08, 5.40e-09, 2.83e-09),          # worst instance 3.84e-09, wrong iterate 1.26e-01
    (9, 8, 32, 1, 20, False, True, False): (3.0e-08, 1.96e-09, 2.94e-09),         # worst instance 4.72e-09, wrong iterate 4.72e-01
    (9, 3, 16, 3, 20, True, False, True): (4.8e-08, 2.18e-09, 4.78e-09),          # worst instance 5.13e-09, wrong iterate 3.06e-01
    (6, 1, 4, 1, 20, False, True, False): (2.7e-08, 2.63e-09, 1.38e-09),          # worst instance 2.17e-09, wrong iterate 8.67e-01
    (6, 1, 4, 1, 10, False, True, False): (2.7e-09, 2.08e-10, 2.66e-10),          # worst instance 4.16e-10, wrong iterate 1.82e+00
    (6, 1, 4, 3, 20, False, False, False): (2.8e-08, 2.76e-09, 2.33e-09),         # worst instance 3.40e-09, wrong iterate 8.46e-01
    (9, 2, 8, 3, 20, False, False, True): (4.7e-08, 3.04e-09, 4.65e-09),          # worst instance 4.00e-09, wrong iterate 4.15e-01
    (9, 7, 28, 3, 20, False, False, False): (5.0e-08, 2.15e-09, 4.92e-09),        # worst instance 4.25e-09, wrong iterate 2.25e-01
    (9, 8, 32, 1, 100, False, True, False): (7.0e-08, 2.23e-09, 6.94e-09),        # worst instance 6.77e-09, wrong iterate 9.65e-04
    (9, 1, 4, 3, 12, False, False, False): (3.5e-08, 3.43e-09, 2.97e-09),         # worst instance 2.74e-09, wrong iterate 4.88e-01
}
# cases whose QP-screen inputs leave every row far from its bound -- the barrier weights of iterates five and six then sit orders below
# h Q and h R, the gains of the two iterates agree to 3e-9 .. 3e-7 and the negative control cannot tell them apart: their targets are
# moved away by this offset (m), which drives jerks and rates to their bounds inside the horizon
FB_WAY_OFFSET = {
    (9, 1, 4, 1, 20, False, True, False): (-2.0, 1.0, 0.5),     # thing_demo: wrong iterate 2.95e-7 before, 1.3e-1 with it
    (6, 1, 4, 1, 20, False, True, False): (-2.0, 1.0, 0.5),     # ur10_demo: 3.5e-9 before, 8.7e-1 with it
    (6, 1, 4, 1, 10, False, True, False): (-2.0, 1.0, 0.5),     # ur10_demo at N 10: 5.9e-9 before, 1.8 with it
}


def fb_case(cfg, monkeypatch=None):
    """The QP screen's case for cfg at qp_tol = 0: dict(P, x0, way, bp, xs0, us0, B)."""
    builder, kw, _ = CASES[cfg]
    if monkeypatch is not None:     # (the golden builders keep their manager's Problem: no handle on a machine without a device)
        from upright_amd import control_bindings
        monkeypatch.setattr(control_bindings, "BatchMPC", _NoDevice)
    kw = {k: v for k, v in kw.items() if k != "iters"}
    c = builder(**kw, qp_tol=0.0, qp_iter_max=K_IT)
    P, x0 = c["P"], c["x0"]
    P.use_feedback_policy = True      # (the reference's default; without it the kernel does not keep the first knot's gain)
    B = x0.shape[0]
    bp = c.get("bp")
    if bp is None:
        bp = np.ascontiguousarray(np.broadcast_to(P.body_params, (B,) + np.shape(P.body_params)))
    xs0, us0 = stationary_guess(x0, P.N, P.nu)
    if cfg in FB_WAY_OFFSET:
        c["way"] = np.asarray(c["way"], dtype=float) + np.asarray(FB_WAY_OFFSET[cfg], dtype=float)
    return dict(P=P, x0=x0, way=c["way"], bp=np.ascontiguousarray(bp), xs0=np.ascontiguousarray(xs0), us0=np.ascontiguousarray(us0), B=B)


def reference_gains(P, lin, sol, pairs, bp, **kw):
    return fb_check.feedback_reference(P, lin, sol, fb_check.friction_rows_of(P), force_jacobian(P, bp), pairs=pairs, **kw)


def two_runs(cfg, c, lin):
    """The emulated instantiation for K_IT and K_IT + 1 iterations on the same records: (run k, run k + 1)."""
    P, B = c["P"], c["B"]
    runs = [fb_check.emu_qp3_cfg_fb(cfg, P, B, c["xs0"], c["us0"], c["x0"], lin, c["bp"], it) for it in (K_IT, K_IT + 1)]
    for r, it in zip(runs, (K_IT, K_IT + 1)):
        assert np.all(r["stats"][:, 1] == it), (r["stats"][:, 1], it)
        assert not np.any(r["stats"][:, 2] == 2), r["stats"][:, 2]
    return runs


def measure(cfg, c, lin, runs):
    """(a, b, worst emulated-vs-float64 error over all instances, negative control, worst cond(M), Pk agreement with the host module)."""
    P, B, N, nx = c["P"], c["B"], c["P"].N, c["P"].nx
    pt, gains = runs
    first = N - TAIL if N > 20 else 0
    Kx, _, _ = reference_gains(P, lin[0], pt["sol"][0], pt["pairs"][0], c["bp"][0], first=first, extended=True)
    worst, control, cond, pk_err = 0.0, np.inf, 0.0, 0.0
    a = b = 0.0
    for i in range(B):
        Kr, Pk, cd = reference_gains(P, lin[i], pt["sol"][i], pt["pairs"][i], c["bp"][i])
        Kd = gains["K"][i][:, :, :nx]
        worst = max(worst, fb_check.block_errors(Kd, Kr, P.nq).max())
        Kw, _, _ = reference_gains(P, lin[i], gains["sol"][i], gains["pairs"][i], c["bp"][i])
        control = min(control, fb_check.block_errors(Kd, Kw, P.nq).max())
        cond = max(cond, cd.max())
        # the reference's cost-to-go against the host module's on the same inputs
        sol = dict(pt["sol"][i], dx=pt["dx"][i], du=pt["du"][i])
        Ph = riccati_value_function(P, c["xs0"][i][:, :nx], c["us0"][i], lin[i], sol, fb_check.friction_rows_of(P), force_jacobian(P, c["bp"][i]),
                                    pairs=pt["pairs"][i])[0]
        pk_err = max(pk_err, max(np.abs(Pk[k] - Ph[k]).max() / np.abs(Ph[k]).max() for k in range(N + 1)))
        if i == 0:
            a = fb_check.block_errors(Kr[first:], Kx, P.nq).max()
            b = fb_check.block_errors(Kd[first:], Kx, P.nq).max()
    return a, b, worst, control, cond, pk_err


@pytest.mark.parametrize("cfg", list(CASES), ids=_ids)
def test_emulated_feedback_gains_against_the_dense_reference(cfg, monkeypatch):
    """Linearise with the emulation, solve with the emulated instantiation for K_IT and K_IT + 1 iterations, compare the gains of the
    second run with K_ref at the point of the first: every (knot, block) of every instance under FB_TOL; the wrong iterate misses by
    ten thresholds at least; the reference's P_k agree with value_function.riccati_value_function's.  Prints a, b and the control."""
    c = fb_case(cfg, monkeypatch)
    P, B = c["P"], c["B"]
    lin = Emu(P, B, bp=c["bp"]).linearize(c["way"], np.zeros(B), c["xs0"], c["us0"])
    runs = two_runs(cfg, c, lin)
    a, b, worst, control, cond, pk_err = measure(cfg, c, lin, runs)
    tol = FB_TOL[cfg][0]
    print("fb reference %s: a (float64 vs extended) %.2e  b (emulated vs extended) %.2e  worst instance %.2e  threshold %.1e  wrong iterate %.2e"
          "  cond(M) %.2e  P_k vs host module %.2e" % (_ids(cfg), a, b, worst, tol, control, cond, pk_err))
    assert tol <= CAP
    assert worst < tol, (worst, tol)
    assert control >= 10.0 * tol, (control, tol)
    # P_k of the reference against riccati_value_function's: two orderings of the same float64 statements, each solve good to
    # eps cond(M) relative, accumulated over the N knots of the recursion
    assert pk_err <= np.finfo(float).eps * cond * P.N, (pk_err, cond)
