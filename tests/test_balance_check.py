"""CPU tests of the batched balance check (upright_amd/csrc/upr_balance.h) through the test-only host emulation
tests/emu/upr_balance_emu.cpp: the generator matrix against the reference's grasp matrices and cone generators
(tests/golden/grasp.json), the projection against tests/balance_ref.py (scipy's nnls on the oracle's b and A) over the case table,
an optimality certificate that involves no solver, and the iteration counts.  The execution on the GPU is checked by
tests/test_gpu_balance_check.py on the same table.

Bound of the comparison: |rho - rho_ref| <= 1e-9 max(1, |b|).  The project asserts g to 1e-11 relative at term level
(tests/lin_check.py), the distance to a convex cone is 1-Lipschitz in b, and the factor 100 covers the conditioning of the passive
systems and the stopping rule.  Largest errors observed per arrangement: DESIGN.md section 3.7."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

import balance_ref as R
from kkt_check import force_jacobian_from_grasp
from oracle.oracle import Oracle
from upright_amd import _capi
from upright_amd.engine import balance_forces
from upright_amd.problem import THING_HOME, thing_problem

ROOT = Path(__file__).resolve().parents[1]
NAMES = [r[0] for r in R.TABLE + R.EXTRA]
ONE_BODY = [r[0] for r in R.TABLE + R.EXTRA if r[4][0] == 1]
JOB_COUNTS = {1, 37, 256, 259}


def test_header_names_the_stopping_rule_and_the_cap():
    """The stopping rule is a named constant of the header, tol <= 1e-10; the cap is 3 ncol; the header says that the force bounds are
    not part of rho."""
    E = R.emu_lib()
    src = (ROOT / "upright_amd" / "csrc" / "upr_balance.h").read_text()
    m = re.search(r"#define\s+UPR_BAL_TOL\s+(\S+)", src)
    assert m and float(m.group(1)) == E.emu_bal_tol() and 0 < E.emu_bal_tol() <= 1e-10
    assert [E.emu_bal_iter_cap(n) for n in (4, 16, 128)] == [12, 48, 384]
    assert "u_lb / u_ub" in src and "NOT part of it" in src
    assert "u_lb / u_ub are NOT part of it" in (ROOT / "include" / "upright_mi.h").read_text()


@pytest.mark.parametrize("name", ["pink_bottle", "box_arch", "robust_8corner"])
def test_generator_matrix_against_the_reference_grasp_matrix(arrangements, name):
    """A's columns (upr_bal_column) at the fixture's nominal parameters equal G blockdiag(S) of tests/golden/grasp.json -- the
    reference's compute_cwc_span_form -- up to the per-body 1 / m, the 1 / sqrt(6 nb) and the sign of dg/df, with the torque rows
    shifted to each body's centre of mass (kkt_check.force_jacobian_from_grasp); generator order from the fixture.  1e-12."""
    arr = arrangements[name]
    gr = json.load(open(ROOT / "tests" / "golden" / "grasp.json"))[name]
    assert gr["names"] == [b["name"] for b in arr["bodies"]]
    P = thing_problem(arr, nf=3)
    nc = P.nc
    S = np.zeros((3 * nc, 4 * nc))
    for i, Si in enumerate(gr["S"]):
        S[3 * i:3 * i + 3, 4 * i:4 * i + 4] = np.asarray(Si)
    D = force_jacobian_from_grasp(gr["G"], [b["mass"] for b in arr["bodies"]], [b["com"] for b in arr["bodies"]], P.nb)
    want = D @ S
    x = np.concatenate([THING_HOME, 0.1 * np.ones(18)])
    m, ncol = 6 * P.nb, 4 * nc
    b = np.full((1, 1, m), np.nan); A = np.full((1, 1, m, ncol), np.nan)
    th = np.ascontiguousarray(P.body_params)
    assert R.emu_lib().emu_bal_system(C.byref(_capi.problem_to_c(P)), 1, _capi.ptr(x), 1, _capi.ptr(th), 0, _capi.ptr(b), _capi.ptr(A)) == 0
    err = np.abs(A[0, 0] - want).max()
    print("generator matrix %s (%d x %d): %.2e" % (name, m, ncol, err))
    assert err <= 1e-12 * max(1.0, np.abs(want).max())
    # and b is the oracle's g at zero forces
    g = Oracle(P).eq_constraint(x, np.zeros(P.nu), jac=False)
    assert np.abs(b[0, 0] - g).max() <= 1e-11 * max(1.0, np.abs(g).max())


@pytest.mark.parametrize("name", NAMES)
def test_case_table_holds_every_class_on_the_oracle_alone(arrangements, name):
    """The reference alone: its floor (nnls against lsq_linear) is <= 1e-10 on every job, the job counts are the table's with both
    parameter layouts, and every class the arrangement can hold has at least five jobs."""
    launches = R.cases(arrangements, name)
    counts, layouts = set(), set()
    total = {}
    for L in launches:
        assert L["ref"]["floor"].max() <= 1e-10, (name, L["ref"]["floor"].max())
        if "free_fall" not in L["kinds"]:
            counts.add(L["ref"]["rho"].size); layouts.add((L["ref"]["rho"].size, L["per_point"]))
            xs = L["x"].reshape(-1, 3, L["P"].nq)
            for i, kind in enumerate(L["kinds"]):                    # states in motion: q, v, a all non-zero ...
                moving = np.abs(xs[i]).max(axis=1) > 0
                if kind in ("facet", "lift"):                        # ... but for the two kinds built at rest (v = 0, a != 0)
                    assert moving[0] and not moving[1] and moving[2], (name, i, kind)
                else:
                    assert np.all(moving), (name, i, kind)
        for k, v in L["classes"].items():
            total[k] = total.get(k, 0) + int(v.sum())
    assert counts == JOB_COUNTS and {(1, False), (1, True), (37, False), (37, True)} <= layouts and any(p for _, p in layouts if _ == 259)
    print(name, total)
    if name in [r[0] for r in R.TABLE]:      # (the shapes beyond the table are there for their column counts, not for the classes)
        for k in R.expected_classes(launches[0]["P"]):
            assert total[k] >= 5, (name, k, total)


@pytest.mark.parametrize("name", ["pink_bottle", "pink_bottle_arm"])
def test_facet_states_lie_on_a_facet(arrangements, name):
    """The facet class on the oracle alone: rho <= 1e-9 at the states (asserted with the class count above), and the same states
    pushed 5 % further along the pyramid axis are outside by more than 1e-3."""
    L = R.cases(arrangements, name)[0]
    rows = [i for i, k in enumerate(L["kinds"]) if k == "facet"]
    beyond = R.reference(L["P"], L["x_beyond"][rows], L["params"][list(R.FACET_SCENARIOS)], False)
    assert L["classes"]["facet"].sum() == len(rows) * len(R.FACET_SCENARIOS)
    assert beyond["rho"].min() > 1e-3, beyond["rho"].min()


@pytest.mark.parametrize("name", NAMES)
def test_kernel_source_against_the_reference(arrangements, name):
    """upr_bal_job under emulation against nnls on every job of the table: |rho - rho_ref| <= 1e-9 max(1, |b|)."""
    worst = 0.0
    for L in R.cases(arrangements, name):
        err = np.abs(L["emu"]["rho"] - L["ref"]["rho"]) / np.maximum(1.0, L["ref"]["bnorm"])
        assert np.all(np.isfinite(L["emu"]["rho"]))
        worst = max(worst, float(err.max()))
    print("balance check, kernel source vs nnls, %s: %.2e" % (name, worst))
    assert worst <= 1e-9, (name, worst)


@pytest.mark.parametrize("name", NAMES)
def test_optimality_certificate_of_the_kernel_source(arrangements, name):
    """No reference solver involved: on the oracle's b and A the emulation's z is non-negative, every column's a_j' r stays above
    -10 tol |a_j| max(|b|, 1), and |z_j a_j' r| below the same bound times |z|_inf -- the optimality conditions of the projection."""
    tol = R.emu_lib().emu_bal_tol()
    for L in R.cases(arrangements, name):
        zmin, dual, comp = R.certificate(L["ref"], L["emu"]["z"], tol)
        assert zmin >= 0.0 and dual <= 1.0 and comp <= 1.0, (name, zmin, dual, comp)
        # rho is the norm of that residual
        r = L["ref"]["b"] + np.einsum("...mc,...c->...m", L["ref"]["A"], L["emu"]["z"])
        assert np.abs(np.linalg.norm(r, axis=-1) - L["emu"]["rho"]).max() <= 1e-11 * max(1.0, L["ref"]["bnorm"].max())


@pytest.mark.parametrize("name", NAMES)
def test_iteration_counts(arrangements, name):
    """Every job ends below the cap of 3 ncol least-squares solves; the jobs outside the cone with z = 0 and the free-fall jobs take
    none and return z = 0 (rho = |b|, exactly 0 in free fall); the passive set never exceeds min(6 nb, ncol)."""
    for L in R.cases(arrangements, name):
        P = L["P"]
        cap = 3 * R.ncol(P)
        it, z = L["emu"]["iters"], L["emu"]["z"]
        assert it.min() >= 0 and it.max() < cap, (name, it.max(), cap)
        for k in ("outside_zero", "free_fall"):
            m = L["classes"][k]
            assert np.all(it[m] == 0) and np.all(z[m] == 0.0)
            assert np.array_equal(L["emu"]["rho"][m], np.linalg.norm(L["ref"]["b"][m], axis=-1)) or \
                np.abs(L["emu"]["rho"][m] - L["ref"]["bnorm"][m]).max() <= 1e-14 * max(1.0, L["ref"]["bnorm"].max())
        assert np.all(L["emu"]["rho"][L["classes"]["free_fall"]] == 0.0)
        assert (z > 0).sum(axis=-1).max() <= min(6 * P.nb, R.ncol(P))


@pytest.mark.parametrize("name", ONE_BODY)
def test_one_body_arrangements_in_both_forms(arrangements, name):
    """One-body arrangements run the lane-per-job form (upr_bal_job1, what R.cases holds); the wave-per-job form takes them as well:
    same bound against the reference, the certificate, and the two forms agree to 1e-13 max(1, |b|) with equal iteration counts."""
    tol = R.emu_lib().emu_bal_tol()
    for L in R.cases(arrangements, name):
        lane = R.run_emu(L["P"], L["x"], L["params"], L["per_point"], form=1)
        wave = R.run_emu(L["P"], L["x"], L["params"], L["per_point"], form=0)
        assert all(np.array_equal(lane[k], L["emu"][k]) for k in lane)
        scale = np.maximum(1.0, L["ref"]["bnorm"])
        assert (np.abs(wave["rho"] - L["ref"]["rho"]) / scale).max() <= 1e-9
        assert (np.abs(wave["rho"] - lane["rho"]) / scale).max() <= 1e-13 and np.array_equal(wave["iters"], lane["iters"])
        zmin, dual, comp = R.certificate(L["ref"], wave["z"], tol)
        assert zmin >= 0.0 and dual <= 1.0 and comp <= 1.0, (name, zmin, dual, comp)
    # a problem with more than one body cannot take the lane form
    Pm = R.table_problem(arrangements, "foam_die2")
    x = np.zeros((1, 27)); o = np.zeros((1, 1)); it = np.zeros((1, 1), dtype=np.int32)
    assert R.emu_lib().emu_bal_points(C.byref(_capi.problem_to_c(Pm)), 1, _capi.ptr(x), 1, _capi.ptr(np.ascontiguousarray(Pm.body_params)), 0,
                                      _capi.ptr(o), None, _capi.iptr(it), 1) == 1


def test_no_decision_hangs_on_the_last_bit(arrangements, tmp_path):
    """The emulation compiled a second time with fused multiply-adds (as the device compiler contracts them) takes the same number
    of least-squares solves on every job of the table and agrees to 1e-13 max(1, |b|): the CPU twin of the device-against-emulation
    screen.  Skipped on a host without FMA instructions."""
    import os
    import subprocess

    if "fma" not in open("/proc/cpuinfo").read():
        pytest.skip("no FMA instructions on this host")
    lib = tmp_path / "libupr_balance_emu_fma.so"
    subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=fast", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", str(lib),
                           str(ROOT / "tests" / "emu" / "upr_balance_emu.cpp")])
    old = os.environ.get("UPR_BALANCE_EMU_LIB")
    os.environ["UPR_BALANCE_EMU_LIB"] = str(lib)
    try:
        for name in NAMES:
            for L in R.cases(arrangements, name):
                f = R.run_emu(L["P"], L["x"], L["params"], L["per_point"])
                assert np.array_equal(f["iters"], L["emu"]["iters"]), (name, np.argwhere(f["iters"] != L["emu"]["iters"])[:5])
                assert (np.abs(f["rho"] - L["emu"]["rho"]) / np.maximum(1.0, L["ref"]["bnorm"])).max() <= 1e-13
    finally:
        if old is None:
            del os.environ["UPR_BALANCE_EMU_LIB"]
        else:
            os.environ["UPR_BALANCE_EMU_LIB"] = old


def test_forces_helper_reproduces_rho_through_the_oracle(arrangements):
    """balance_forces: f = S z of the emulation's z, handed to the oracle's equality constraint as the force block of u, leaves a
    residual of norm rho -- with friction (box_arch: both bodies of a contact in a column) and without (robust_8corner)."""
    for name in ("box_arch", "robust_8corner"):
        L = R.cases(arrangements, name)[0]
        P = L["P"]
        f = balance_forces(P, L["emu"]["z"])
        assert f.shape == L["emu"]["z"].shape[:2] + (P.nf * P.nc,)
        for i in (0, 25, 50):
            for s in range(4):
                u = np.concatenate([np.zeros(P.nq), f[i, s]])
                g = Oracle(R.with_params(P, L["params"][s])).eq_constraint(L["x"][i], u, jac=False)
                assert abs(np.linalg.norm(g) - L["emu"]["rho"][i, s]) <= 1e-11 * max(1.0, L["ref"]["bnorm"][i, s])
