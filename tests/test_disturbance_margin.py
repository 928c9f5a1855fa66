"""The batched disturbance margin (upright_amd/csrc/upr_disturb.h) through its host emulation (tests/emu/upr_disturb_emu.cpp), against
the CPU reference and on the case table of tests/disturb_ref.py: the displaced record the kernel rests on, the classes the table holds,
and the assertions tests/test_gpu_disturbance_margin.py repeats on the device's answers.

Observed on the emulation (x86-64, nine arrangements): displaced record vs the oracle's b at the displaced joint-space state at most
4.2e-15 max(|b|, 1); closed forms at most 2.3e-8 relative (vertical), 4.5e-8 (slide), 5.0e-8 (compensated tilt); against
path_accel_margin's emulation with dirs = (omega, v_ee) of the oracle: equal."""
import numpy as np
import pytest

import balance_ref as R
import disturb_ref as D
import pathacc_ref as A
from oracle.oracle import Oracle


@pytest.mark.parametrize("name", D.NAMES)
def test_table_holds_every_class(arrangements, name):
    """At least five jobs of every class the arrangement can hold (all of pathacc_ref.CLASSES, without window where nf = 1), on the
    reference alone; the launches of the table: both parameter layouts, 1 x 1, r_max = 12, the negated directions."""
    launches = D.cases(arrangements, name)
    counts = D.class_counts(launches)
    print("disturbance margin, %s: classes %s, %d jobs" % (name, counts, sum(counts.values())))
    for c in D.expected_classes(launches[0]["P"]):
        assert counts[c] >= 5, (name, c, counts)
    nd = 5 if launches[0]["P"].nf == 3 else 3
    assert [len(L["dirs"]) for L in launches] == [nd] * 5 + [2]
    assert [L["per_point"] for L in launches] == [False, True, False, True, False, False]
    assert [L["r_max"] for L in launches] == [8.0] * 4 + [12.0] * 2
    assert [np.asarray(L["x"]).shape[0] for L in launches][2:4] == [1, 1] and sum(counts.values()) <= 520


@pytest.mark.parametrize("name", D.NAMES)
def test_rhs_of_the_displaced_record(arrangements, name):
    """|b_emu - b_ref| <= 1e-12 max(|b|, 1): the b a job builds from the displaced record (C_we, omega, alpha + r u_alpha, a_ee + r u_a),
    u in the tray frame and rotated in numpy for the world frame, against the oracle's b at the displaced joint-space state, on random
    states in motion and directions with an angular part."""
    P = R.table_problem(arrangements, name)
    x = R.points(P, ["inside", "outside", "down"] * 3, seed=9 + sum(map(ord, name)))
    scen = R.scenarios(P)
    rng = np.random.default_rng(5)
    worst = 0.0
    for sc in (0, 1, 3):
        u = rng.uniform(-1.0, 1.0, 6)
        uw = D.world_dirs(P, x, u[None])[:, 0]
        for r in (0.0, 1.7, -3.0):
            b = np.stack([R.system(P, scen[sc], D.displaced(P, xi, ui, r))[0] for xi, ui in zip(x, uw)])
            scale = np.maximum(np.linalg.norm(b, axis=1), 1.0)
            worst = max(worst, float((np.linalg.norm(D.emu_rhs(P, x, scen[sc], u, "tray", r) - b, axis=1) / scale).max()))
            bw = np.stack([D.emu_rhs(P, xi, scen[sc], ui, "world", r)[0] for xi, ui in zip(x, uw)])
            worst = max(worst, float((np.linalg.norm(bw - b, axis=1) / scale).max()))
    print("disturbance margin, %s: displaced record vs oracle %.2e (units of max(|b|, 1))" % (name, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("name", D.NAMES)
def test_bracket_certificates_and_reference(arrangements, name):
    """pathacc_ref.check_answer on the emulation's answer to every launch and every direction block: the class of every job equal to
    the reference's, in - out = r_max 2^-31 where an end was bisected, both certificates on the oracle's b and A within EPS +- RHO_TOL."""
    for k, L in enumerate(D.cases(arrangements, name)):
        bad = D.check_launch(L, L["emu"])
        assert not bad, (name, k, bad[:5])


@pytest.mark.parametrize("name", D.ONE_BODY)
def test_wave_form_on_one_body_shapes(arrangements, name):
    """The wave-per-job job on the one-body shapes: the same checks, and the same answer as the lane form on the steady jobs."""
    for k, L in enumerate(D.cases(arrangements, name)):
        out = D.run_launch(L, form=0)
        bad = D.check_launch(L, out)
        assert not bad, (name, k, bad[:5])
        m = D.steady(L)
        assert np.array_equal(out["reach"][m], L["emu"]["reach"][m])


@pytest.mark.parametrize("name", D.NAMES)
def test_known_answers(arrangements, name):
    """|r - r_known| <= 1e-6 |r_known| (pathacc's bound) where the state moves along +-u: r_lo = k (falling / rising along e_z), -g0
    (free fall, r_max = 12), g0 and -k on the negated directions, +-mu0 g0 and the compensated-tilt window where sliding binds; at
    least five ends per arrangement."""
    launches = D.cases(arrangements, name)
    n = 0
    for k in (0, 4, 5):
        L = launches[k]
        w = D.known_answers(L, L["emu"]["reach"], name)
        print("disturbance margin, %s, launch %d: largest relative |r - r_known| vertical %.2e, slide %.2e, comp %.2e (%d ends)"
              % (name, k, w["vertical"], w["slide"], w["comp"], w["n"]))
        assert w["vertical"] <= 1e-6 and w["slide"] <= 1e-6 and w["comp"] <= 1e-6
        n += w["n"]
    assert n >= 5


@pytest.mark.parametrize("name", D.NAMES)
def test_fma_twin_takes_the_same_evaluations(arrangements, name):
    """The -mfma -ffp-contract=fast build of the emulation: the same class everywhere, the same answer and solve counts on the steady
    jobs."""
    if not D.have_fma_twin():
        pytest.skip("the host has no FMA instruction (/proc/cpuinfo): the twin is not built")
    for L in D.cases(arrangements, name):
        out = D.run_launch(L, fma=True)
        assert np.array_equal(D.classes_of(out, L["r_max"]), np.stack([b["pclass"] for b in D.blocks_of(L)]))
        m = D.steady(L)
        assert np.array_equal(out["iters"][m], L["emu"]["iters"][m]) and np.array_equal(out["reach"][m], L["emu"]["reach"][m])


def path_states(arrangements, name):
    """(P, launch, rows): >= 8 states of pathacc's table (its first launch) that span its classes, two of each where it has them"""
    L = A.cases(arrangements, name)[0]
    rows = []
    for c in A.CLASSES:
        rows += [(int(i), int(sc)) for i, sc in np.argwhere((L["pclass"] == c) & L["jobs"].moving[:, None])[:2]]
    return L["P"], L, rows


@pytest.mark.parametrize("name", ["pink_bottle", "foam_die2"])
def test_equals_the_path_acceleration_margin(arrangements, name):
    """n = 1, frame = world, dirs = [(omega, v_ee)] of the oracle, r_max = d_max: the emulation's reach equals the emulation's
    path_accel_margin at speed 1, on states of pathacc's table of every class."""
    P, L, rows = path_states(arrangements, name)
    assert len(rows) >= 8 and len({L["pclass"][i, sc] for i, sc in rows}) >= 6
    O = Oracle(P)
    for i, sc in rows:
        _, v, om, _, _ = D.ee_of(O, L["x"][i])
        out = D.run_emu(P, L["x"][i:i + 1], L["params"][sc:sc + 1], False, np.concatenate([om, v])[None], L["d_max"], "world")
        want = L["emu"]["accel"][i, sc]
        assert np.array_equal(out["reach"][0, 0, 0], want), (name, i, sc, out["reach"][0, 0, 0], want)


@pytest.mark.parametrize("name", ["pink_bottle", "blue_cups"])
def test_tray_against_world_and_symmetry(arrangements, name):
    """Tray-frame dirs against the same directions rotated in numpy and passed as world, point by point: equal class, ends within two
    grid steps.  dirs (u, -u) in one call: r_lo(-u) = -r_hi(u) and r_hi(-u) = -r_lo(u), == on steady jobs and within two grid steps
    elsewhere; swapping the direction order permutes the blocks bit for bit."""
    L = D.cases(arrangements, name)[0]
    P, dirs, rm = L["P"], L["dirs"], L["r_max"]
    tol = 2.0 * D.step(rm)
    uw = D.world_dirs(P, L["x"], dirs)
    for i in range(0, len(L["x"]), 2):
        out = D.run_emu(P, L["x"][i:i + 1], L["params"], False, uw[i], rm, "world")
        a, b = out["reach"][:, 0], L["emu"]["reach"][:, i]
        assert np.array_equal(D.classes_of(out, rm)[:, 0], D.classes_of(L["emu"], rm)[:, i])
        fin = np.isfinite(a)
        assert np.array_equal(fin, np.isfinite(b)) and np.array_equal(a[~fin], b[~fin]) and np.abs(a[fin] - b[fin]).max() <= tol
    both = D.run_emu(P, L["x"], L["params"], False, np.concatenate([dirs, -dirs]), rm, "tray")
    nd = len(dirs)
    assert all(np.array_equal(both[k][:nd], L["emu"][k]) for k in both)
    mirror = -both["reach"][nd:][..., [2, 3, 0, 1]]
    m = D.steady(L)
    assert np.array_equal(mirror[m], both["reach"][:nd][m])
    fin = np.isfinite(mirror)
    assert np.array_equal(fin, np.isfinite(both["reach"][:nd])) and np.array_equal(mirror[~fin], both["reach"][:nd][~fin])
    assert np.abs(mirror[fin] - both["reach"][:nd][fin]).max() <= tol
    perm = np.arange(nd)[::-1]
    swapped = D.run_emu(P, L["x"], L["params"], False, dirs[perm], rm, "tray")
    assert all(np.array_equal(swapped[k], L["emu"][k][perm]) for k in swapped)


def test_plan_reductions_on_the_host():
    """upr_bal_disturb_reduce compiled for the host against numpy, on random values with ties between knots and between ends, an
    unbalanced knot (radius < 0), a scenario that accepts nothing (-inf), a repeated direction and n_dir = 1 and 32: window, knot,
    radius and binding exactly; no NaN."""
    rng = np.random.default_rng(13)
    for nd in (1, 4, 32):
        B, nk, ns = 3, 21, 4
        lo = -np.round(rng.uniform(0.5, 8.0, (nd, B, nk, ns)), 1)          # (one decimal: ties between knots and between ends)
        hi = np.round(rng.uniform(0.5, 8.0, (nd, B, nk, ns)), 1)
        reach = np.stack([lo, lo - 0.25, hi, hi + 0.25], axis=-1)
        reach[0, 1, 7, 2] = [1.5, 1.25, 3.0, 3.25]                           # an unbalanced knot: 0 < r_lo
        reach[nd - 1, 2, 3, 1] = [np.inf, -8.0, -np.inf, 8.0]                # a job that accepts nothing
        reach[:, 0, :, 3, 0], reach[:, 0, :, 3, 2] = -8.0, 8.0               # open everywhere: radius = r_max, the first end binds
        if nd > 2:
            reach[2] = reach[1]                                              # a repeated direction: the first one binds
        w, kn, rad, bind = D.emu_plan(reach)
        w0, kn0, rad0, bind0 = D.numpy_plan(reach)
        assert np.array_equal(w, w0) and np.array_equal(kn, kn0) and np.array_equal(rad, rad0) and np.array_equal(bind, bind0)
        assert not np.any(np.isnan(w)) and not np.any(np.isnan(rad))
        assert rad[2, 1] == -np.inf and tuple(bind[2, 1]) == (nd - 1, -1, 3) and rad[0, 3] == 8.0 and tuple(bind[0, 3]) == (0, -1, 0)
        assert rad[1, 2] <= -1.5 < 0.0 and (nd <= 2 or not np.any(bind[..., 0] == 2))
