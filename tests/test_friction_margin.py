"""The batched friction margin (upright_amd/csrc/upr_margin.h) through its host emulation (tests/emu/upr_margin_emu.cpp: the same
source, one thread per wave), against tests/margin_ref.py: the classes of the table on the reference alone, the bracket, the two
solver-free certificates, the reference at both ends of the bracket, the known answers (facet states, the pushed fixture box, the
wedge), rho with a friction scale, and the iteration counts.  tests/test_gpu_friction_margin.py makes the same assertions on the
device."""
from pathlib import Path

import numpy as np
import pytest

import balance_ref as R
import margin_ref as M
from upright_amd import _capi
from upright_amd.problem import thing_problem

ROOT = Path(__file__).resolve().parents[1]


def test_entry_points_and_documents():
    names = {n for n, _, _ in _capi.PROTOTYPES}
    assert {"upr_batch_friction_margin_points", "upr_batch_friction_margin_plan", "upr_batch_balance_points_mu", "upr_batch_balance_plan_mu"} <= names
    E = M.emu_lib()
    assert E.emu_mar_feas() == M.EPS and E.emu_mar_bisect() == M.BISECT
    header = (ROOT / "include" / "upright_mi.h").read_text()
    assert "kappa* mu_i" in header and "The force bounds are NOT" in header
    from upright_amd.engine import BatchMPC

    doc = BatchMPC.friction_margin.__doc__
    assert "kappa* mu_i" in doc and "force bounds" in doc and "1e-8" in doc
    assert "3.8" in (ROOT / "DESIGN.md").read_text() and "friction_margin" in (ROOT / "README.md").read_text()


@pytest.mark.parametrize("name", M.NAMES)
def test_classes_on_the_reference(arrangements, name):
    """Every class the issue requires of an arrangement holds at least 5 jobs of the table, on the reference alone (four evaluations
    per job: 0, 1 - 1e-3, 1 + 1e-3, kappa_max).  nf = 3: zero, below one, inf; pink_bottle also at one; fixture_box at one and above
    one, finite; nf = 1: zero and inf.  Not required, because the arrangement cannot be shown to hold it on the reference:
    fixture_box holds no inf job -- lift-off is held by friction on the fixture's side walls from kappa = 1 / 0.18 on, below
    kappa_max, and a box that low does not tip (margin_ref.N_DOWN has the figures of those states)."""
    launches = M.cases(arrangements, name)
    P = launches[0]["P"]
    got = M.class_counts(launches)
    print("friction margin, classes of %s: %s" % (name, got))
    need = ["zero", "inf"] if P.nf == 1 else ["zero", "below", "inf"]
    if name == "pink_bottle":
        need += ["one"]
    if name == "fixture_box":
        need = ["zero", "below", "one", "above"]
    for c in need:
        assert got[c] >= 5, (name, c, got)
    if P.nf == 1:
        assert got["below"] == got["one"] == got["above"] == 0
    # job counts 1, 37, 256, 259 in both parameter layouts (and the 2 x 4 pushed facet states of the one-body shapes with friction)
    assert sorted(L["mclass"].size for L in launches) in ([1, 1, 37, 37, 256, 259], [1, 1, 8, 37, 37, 256, 259])
    assert {(L["mclass"].size, L["per_point"]) for L in launches} >= {(1, False), (1, True), (37, False), (37, True), (256, False), (259, True)}


@pytest.mark.parametrize("name", M.NAMES)
def test_bracket_certificates_and_reference(arrangements, name):
    """Checks 1 - 4 on every job of the table, the form the library launches: the bracket (exact), z >= 0 and |b + A(kappa_hi) z| <=
    (1e-8 + 1e-9) max(|b|, 1) on the oracle's b and A, a_j' y >= -10 UPR_BAL_TOL |a_j| max(|b|, 1) and y' b / |y| >= (1e-8 - 1e-9)
    max(|b|, 1) on the oracle's A(kappa_lo), rho_ref at both ends, and the reference's class.  Prints the largest |kappa - kappa_ref|
    against full CPU bisections (DESIGN 3.8 records it)."""
    launches = M.cases(arrangements, name)
    for k, L in enumerate(launches):
        bad = M.check_answer(L, L["emu"])
        assert not bad, (name, k, bad[:5])
    bs = M.reference_bisections(launches)
    worst = max([abs(launches[k]["emu"]["kappa_hi"][i, s] - hi) for k, i, s, hi, _ in bs] or [0.0])
    print("friction margin, emulation vs reference bisection, %s: %d finite jobs, largest |kappa - kappa_ref| %.2e" % (name, len(bs), worst))


@pytest.mark.parametrize("name", M.ONE_BODY)
def test_one_body_arrangements_in_both_forms(arrangements, name):
    """One-body arrangements run a lane per job; form 0 sends them through the wave-per-job job (UPR_BAL_FORM=0 on the device):
    both answer the same jobs with the same checks and the same class."""
    for k, L in enumerate(M.cases(arrangements, name)):
        for form in (0, 1):
            out = M.run_emu(L["P"], L["x"], L["params"], L["per_point"], form=form)
            bad = M.check_answer(L, out)
            assert not bad, (name, k, form, bad[:5])
            if form == 1:
                assert all(np.array_equal(out[key], L["emu"][key]) for key in out)


@pytest.mark.parametrize("name", ["pink_bottle", "pink_bottle_arm", "fixture_box", "bottle_20_contacts"])
def test_known_answers(arrangements, name):
    """Facet states (the load feels exactly g (e_z + mu s)) in the scenarios that keep them on the facet: |kappa - 1| <= 1e-6; the
    fixture box pushed 5 % further: |kappa - 1.05| <= 1e-6.  The 1e-6: the 1e-8 rule moves kappa* by at most 1e-8 sqrt(6)
    sqrt(1 + mu^2) / (mu g) = 1.4e-8 at mu = 0.18, the bracket adds 1.9e-9, the facet construction is good to 1e-9
    (test_facet_states_lie_on_a_facet); 1e-6 leaves a factor 50 and separates 1 from 1.05 by four decades."""
    launches = M.cases(arrangements, name)
    L = launches[0]
    rows = [i for i, k in enumerate(L["kinds"]) if k == "facet"]
    assert len(rows) == 2
    k1 = L["emu"]["kappa_hi"][rows][:, list(R.FACET_SCENARIOS)]
    print("friction margin, facet states of %s: kappa - 1 = %s" % (name, (k1 - 1.0).ravel()))
    assert np.abs(k1 - 1.0).max() <= 1e-6
    if name == "fixture_box":
        Lb = launches[-1]
        assert Lb["kinds"] == ["beyond"] * 2
        kb = Lb["emu"]["kappa_hi"][:, list(R.FACET_SCENARIOS)]
        print("friction margin, pushed facet states of fixture_box: kappa - 1.05 = %s" % (kb - 1.05).ravel())
        assert np.abs(kb - 1.05).max() <= 1e-6


def test_wedge_minimum_friction(arrangements):
    """The one published answer of compute_minimum_mu.py: over the 41 tilt angles of test_wedge_minimum_friction_known_answer
    (states given as C_we, at rest) the smallest kappa* mu is tan 7.5 deg to the 2e-3 of that test."""
    P = thing_problem(arrangements["wedge"])
    mu = np.asarray(P.contact_mu)
    assert np.all(mu == mu[0])
    st = np.zeros((41, 18))
    for k, d in enumerate(np.linspace(-10, 10, 41)):
        th = np.deg2rad(d)
        st[k, :9] = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]).ravel()
    out = M.run_emu_states(P, st, np.asarray(P.body_params)[None], False)
    best = float(out["kappa_hi"].min() * mu[0])
    print("friction margin, wedge: min over the tilt angles of kappa* mu = %.6f (tan 7.5 deg = %.6f)" % (best, np.tan(np.deg2rad(7.5))))
    assert abs(best - np.tan(np.deg2rad(7.5))) < 2e-3
    if P.nb == 1:
        other = M.run_emu_states(P, st, np.asarray(P.body_params)[None], False, form=0)
        assert np.abs(other["kappa_hi"] - out["kappa_hi"]).max() <= 1e-6


@pytest.mark.parametrize("name", M.NAMES)
def test_rho_with_a_friction_scale(arrangements, name):
    """balance check with mu_scale, first launch of the arrangement: rho at kappa in {0.5, 1, 2} does not increase (to 1e-9 max(|b|,
    1)), at kappa = 1 it is the call without a scale bit for bit, and |rho - rho_ref| <= 1e-9 max(1, |b|) at kappa in {0.5, 2}."""
    L = M.cases(arrangements, name)[0]
    J = L["jobs"]
    args = (L["P"], L["x"], L["params"], L["per_point"])
    rho = {k: M.run_emu_rho(*args, mu_scale=k)[0] for k in (0.5, 1.0, 2.0)}
    plain, it_plain = M.run_emu_rho(*args)
    old = R.run_emu(*args)
    assert np.array_equal(rho[1.0], plain) and np.array_equal(plain, old["rho"]) and np.array_equal(it_plain, old["iters"])
    M.check_rho_scaled(J, rho, name, "emulation")
    # one scale per scenario in one call
    mixed = M.run_emu_rho(*args, mu_scale=np.array([0.5, 1.0, 2.0, 1.0]))[0]
    assert all(np.array_equal(mixed[:, s], rho[k][:, s]) for s, k in enumerate((0.5, 1.0, 2.0, 1.0)))


@pytest.mark.parametrize("name", M.NAMES)
def test_iterations(arrangements, name):
    """iters <= (2 + 32) 3 ncol on every job (check_answer); a zero-class job takes exactly one evaluation -- its count is that of
    the rho call at kappa = 0; the share of jobs with a decision within 1e-9 max(|b|, 1) of the boundary, on the reference (those
    the device test does not compare iteration counts on), is at most 5 % of the arrangement's jobs."""
    launches = M.cases(arrangements, name)
    for L in launches:
        zero = L["mclass"] == "zero"
        it0 = M.run_emu_rho(L["P"], L["x"], L["params"], L["per_point"], mu_scale=0.0)[1]
        assert np.array_equal(L["emu"]["iters"][zero], it0[zero])
        assert np.all(L["emu"]["iters"][zero] <= 3 * R.ncol(L["P"]))
    share = M.near_decision_share(launches)
    print("friction margin, %s: %.2f %% of the jobs have a decision within 1e-9 max(|b|, 1) of the boundary" % (name, 100.0 * share))
    assert share <= 0.05, (name, share)
