"""The batched speed margin (upright_amd/csrc/upr_speed.h) through its host emulation (tests/emu/upr_speed_emu.cpp), against the CPU
reference and on the case table of tests/speed_ref.py: the claim b(s) = b0 + s^2 (b1 - b0) the kernel rests on, the classes the table
holds, and the assertions tests/test_gpu_speed_margin.py repeats on the device's answers."""
import numpy as np
import pytest

import balance_ref as R
import speed_ref as S


@pytest.mark.parametrize("name", S.NAMES)
def test_rhs_is_affine_in_the_squared_speed(arrangements, name):
    """|b_ref(s) - b0 - s^2 (b1 - b0)| <= 1e-12 max(|b|, 1) on random states in motion (the generic kinds: v, a, omega and alpha all
    non-zero), s in {0.3, 1, 2.5}, on the oracle's b at x_s; and the b a job builds from the scaled record equals the oracle's to the
    same bound."""
    P = R.table_problem(arrangements, name)
    x = R.points(P, ["inside", "outside", "down"] * 4, seed=5 + sum(map(ord, name)))
    scen = R.scenarios(P)
    worst, worst_emu = 0.0, 0.0
    for sc in (0, 1, 3):
        b = {s: np.stack([R.system(P, scen[sc], S.scaled_state(xi, s, P.nq))[0] for xi in x]) for s in (0.0, 0.3, 1.0, 2.5)}
        for s in (0.3, 1.0, 2.5):
            scale = np.maximum(np.linalg.norm(b[s], axis=1), 1.0)
            worst = max(worst, float((np.linalg.norm(b[s] - b[0.0] - s * s * (b[1.0] - b[0.0]), axis=1) / scale).max()))
            worst_emu = max(worst_emu, float((np.linalg.norm(S.emu_rhs(P, x, scen[sc], s) - b[s], axis=1) / scale).max()))
    print("speed margin, %s: |b(s) - b0 - s^2 (b1 - b0)| %.2e, scaled record vs oracle %.2e (units of max(|b|, 1))" % (name, worst, worst_emu))
    assert worst <= 1e-12 and worst_emu <= 1e-12


@pytest.mark.parametrize("name", S.NAMES)
def test_table_holds_every_class(arrangements, name):
    """At least five jobs of every class the arrangement can hold, on the reference alone; a none job has rho_ref above the limit on the
    whole grid."""
    launches = S.cases(arrangements, name)
    counts = S.class_counts(launches)
    n_none = sum(int((L["sclass"] == "none").sum()) for L in launches)
    n_cmp = sum(int((S.steady(L) & (L["sclass"] == "none")).sum()) for L in launches)
    print("speed margin, %s: classes %s; none jobs whose counts are compared %d of %d" % (name, counts, n_cmp, n_none))
    assert n_cmp >= 5
    for c in S.expected_classes(launches[0]["P"], name):
        assert counts[c] >= 5, (name, c, counts)
    assert sorted(L["sclass"].size for L in launches) == [1, 1, 37, 37, 256, 259]
    for L in launches:
        J = L["jobs"]
        for i, sc in np.argwhere(L["sclass"] == "none"):
            assert not any(J.accepted(int(i), int(sc), s) for s in np.linspace(0.0, J.s_max, S.GRID))


@pytest.mark.parametrize("name", S.NAMES)
def test_bracket_certificates_and_reference(arrangements, name):
    """S.check_answer on the emulation's answer to every launch; the largest difference to CPU replays of the algorithm on rho_ref
    (the first bisecting jobs of the arrangement) is printed for DESIGN 3.10."""
    launches = S.cases(arrangements, name)
    for k, L in enumerate(launches):
        bad = S.check_answer(L, L["emu"])
        assert not bad, (name, k, bad[:5])
    L = launches[2]
    J = L["jobs"]
    rows = [(int(i), int(sc)) for i, sc in np.argwhere(np.isin(L["sclass"], ("upper_lt1", "upper_gt1", "window")))][:4]
    w = 0.0
    for i, sc in rows:
        sp, n_ev = J.replay(i, sc)
        assert n_ev <= 3 + 3 * S.BISECT
        fin = np.isfinite(sp)
        w = max(w, float(np.abs(sp[fin] - L["emu"]["speed"][i, sc][fin]).max()))
    print("speed margin, %s: emulation vs CPU replay on %d bisecting jobs, largest difference of an end %.2e" % (name, len(rows), w))


@pytest.mark.parametrize("name", S.ONE_BODY)
def test_wave_form_on_one_body_shapes(arrangements, name):
    """The wave-per-job job on the one-body shapes: the same checks, and the same answer as the lane form on the jobs that bisect
    no end."""
    for k, L in enumerate(S.cases(arrangements, name)):
        out = S.run_emu(L["P"], L["x"], L["params"], L["per_point"], form=0)
        bad = S.check_answer(L, out)
        assert not bad, (name, k, bad[:5])
        m = S.steady(L)
        assert np.array_equal(out["speed"][m], L["emu"]["speed"][m])


@pytest.mark.parametrize("name", S.NAMES)
def test_known_answers(arrangements, name):
    """|s - s_known| <= 1e-6 (the shift of the EPS rule): the lift-off states have s+ = sqrt(g0 / (g0 - k)) in every scenario, without
    friction too; on the arrangements where sliding binds first (S.SLIDING_BINDS) the scaled facet states have s+ = 1 / sqrt(c) = 2, 1,
    0.5 and the window states their closed form, in the scenarios that keep it so."""
    L = S.cases(arrangements, name)[0]
    w = S.known_answers(L, L["emu"]["speed"])
    print("speed margin, %s: largest |s - s_known| facet %.2e, lift-off %.2e, window %.2e" % (name, w["facet"], w["liftoff"], w["window"]))
    assert w["liftoff"] <= 1e-6
    if name in S.SLIDING_BINDS:
        assert w["facet"] <= 1e-6 and w["window"] <= 1e-6


@pytest.mark.parametrize("name", S.NAMES)
def test_fma_twin_takes_the_same_evaluations(arrangements, name):
    """The -mfma -ffp-contract=fast build of the emulation (how hipcc contracts for the device): the same answer and the same
    iteration counts on the jobs that bisect no end, the same class everywhere."""
    if not S.have_fma_twin():
        pytest.skip("the host has no FMA instruction (/proc/cpuinfo): the twin is not built")
    for L in S.cases(arrangements, name):
        out = S.run_emu(L["P"], L["x"], L["params"], L["per_point"], fma=True)
        assert np.array_equal(S.device_class(out["speed"]), L["sclass"])
        m = S.steady(L)
        assert np.array_equal(out["iters"][m], L["emu"]["iters"][m]) and np.array_equal(out["speed"][m], L["emu"]["speed"][m])


@pytest.mark.parametrize("name", S.NAMES)
def test_monotone_sanity_on_upper_jobs(arrangements, name):
    """On every upper job of the first launch with s_hi >= 1e-3, the balance check of the emulation at x_s: balanced at 0.99 s_hi, not
    balanced at 1.01 s_hi_out.  (s_hi < 1e-3: without friction a facet state's upper end is a few grid steps above rest, 1 % of
    which moves rho by less than the rule's ball.)"""
    L = S.cases(arrangements, name)[0]
    P = L["P"]
    sp = L["emu"]["speed"]
    rows = np.argwhere(np.char.startswith(L["sclass"], "upper") & (sp[..., 2] >= 1e-3))
    assert len(rows) >= 5
    for factor, col, inside in ((0.99, 2, True), (1.01, 3, False)):
        x = np.stack([S.scaled_state(L["x"][i], factor * sp[i, sc, col], P.nq) for i, sc in rows])
        rho = R.run_emu(P, x, np.stack([L["params"][sc:sc + 1] for _, sc in rows]), True)["rho"][:, 0]
        assert np.all((rho <= 1e-8) == inside), (name, factor, rows[(rho <= 1e-8) != inside][:5])


@pytest.mark.parametrize("name", S.NAMES)
def test_table_sees_the_descent_search_and_the_open_upper_end(arrangements, name):
    """The paths of the algorithm beyond the nominal seed, on the reference alone: the sigma = 0.25 and sigma = 3 states are windows
    that exclude rest, the nominal speed, s_max and the first midpoint 2 (the descent search seeds them after at least one decision
    on the slope; with its sign inverted the replay ends without a seed, so a kernel with the wrong sign fails the class check on
    these jobs); the sigma = 4 states are rejected at rest and at the
    nominal speed and accepted at s_max (seeded by s_max, open upper end).  At least five jobs of each; the emulation of both
    forms agrees with the replay on them."""
    launches = S.cases(arrangements, name)
    n_descent = n_top = 0
    for L in launches[:4]:
        J = L["jobs"]
        P = L["P"]
        wave = S.run_emu(P, L["x"], L["params"], L["per_point"], form=0) if P.nb == 1 else L["emu"]
        for i, kind in enumerate(L["kinds"]):
            if kind not in ("comp0.25", "comp3.0", "comp4.0"):
                continue
            for sc in range(J.ns):
                if L["sclass"][i, sc] != "window":
                    continue
                top = J.accepted(i, sc, J.s_max)
                if kind != "comp4.0" and not top and not J.accepted(i, sc, 1.0) and not J.accepted(i, sc, 2.0) and n_descent < 6:
                    sp, n_ev = J.replay(i, sc)
                    assert np.isfinite(sp).all() and 0.0 < sp[0] <= sp[2] < J.s_max and n_ev > 3 + 2
                    assert np.isinf(J.replay(i, sc, flip=True)[0][0])
                    for out in (L["emu"], wave):
                        assert np.abs(out["speed"][i, sc] - sp).max() <= 1e-6, (name, i, sc, out["speed"][i, sc], sp)
                    n_descent += 1
                if kind == "comp4.0" and top and not J.accepted(i, sc, 1.0) and n_top < 6:
                    for out in (L["emu"], wave):
                        assert out["speed"][i, sc, 2] == J.s_max and np.isinf(out["speed"][i, sc, 3]) and out["speed"][i, sc, 0] > 1.0
                    n_top += 1
    print("speed margin, %s: windows seeded by the descent search %d, by s_max %d (checked; the table holds more)" % (name, n_descent, n_top))
    assert n_descent >= 5 and n_top >= 5


def test_plan_reductions_on_the_host():
    """upr_bal_speed_window / upr_bal_speed_limit compiled for the host against numpy on random values with ties, infinities and a plan
    at rest: window and knot exactly, limit to 1e-12 relative."""
    from upright_amd.problem import thing_problem
    import json
    from pathlib import Path

    P = thing_problem(json.load(open(Path(__file__).resolve().parent / "golden" / "arrangements.json"))["pink_bottle"])
    rng = np.random.default_rng(9)
    B, nk, ns = 5, 21, 3
    speed = np.round(rng.uniform(0.0, 4.0, (B, nk, ns, 4)), 1)          # (one decimal: ties between knots)
    speed[1, 3, 0] = [np.inf, 0.0, -np.inf, 4.0]
    speed[2, :, 1, 0] = 0.0; speed[2, :, 1, 2] = 4.0
    xs = rng.uniform(-1.0, 1.0, (B, nk, 3 * P.nq)); us = rng.uniform(-5.0, 5.0, (B, nk - 1, P.nu))
    xs[4, :, P.nq:] = 0.0; us[4] = 0.0
    w, kn, lim = S.emu_plan(P, speed, xs, us)
    w0, kn0, lim0 = S.numpy_plan(P, speed, xs, us)
    assert np.array_equal(w, w0) and np.array_equal(kn, kn0)
    assert lim[4] == np.inf and lim0[4] == np.inf
    rel = np.abs(lim[:4] - lim0[:4]) / lim0[:4]
    print("speed margin: limit speed, host build of the kernel body vs numpy, largest relative difference %.2e" % rel.max())
    assert rel.max() <= 1e-12
