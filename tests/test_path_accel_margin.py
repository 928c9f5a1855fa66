"""The batched path-acceleration margin (upright_amd/csrc/upr_pathacc.h) through its host emulation (tests/emu/upr_pathacc_emu.cpp),
against the CPU reference and on the case table of tests/pathacc_ref.py: the record transform the kernel rests on, the classes the table
holds, and the assertions tests/test_gpu_path_accel_margin.py repeats on the device's answers.

Observed on the emulation (x86-64, nine arrangements): transformed record vs the oracle's b at x(s0, d) at most 4.4e-15 max(|b|, 1), the
oracle's b affine in d to 1.0e-14; closed forms at most 2.2e-8 relative (lift-off, sink, falling, rising), 4.5e-8 (slide), 5.0e-8
(compensated tilt)."""
import numpy as np
import pytest

import balance_ref as R
import pathacc_ref as A


@pytest.mark.parametrize("name", A.NAMES)
def test_rhs_of_the_transformed_record(arrangements, name):
    """|b_emu - b_ref| <= 1e-12 max(|b|, 1): the b a job builds from the transformed record (C_we, s0 omega, s0^2 alpha + d omega,
    s0^2 a_ee + d v_ee) against the oracle's b at the joint-space state (q, s0 v, s0^2 a + d v), on random states in motion; and the
    oracle's b is affine in d to the same bound."""
    P = R.table_problem(arrangements, name)
    x = R.points(P, ["inside", "outside", "down"] * 4, seed=7 + sum(map(ord, name)))
    scen = R.scenarios(P)
    worst, worst_aff = 0.0, 0.0
    for sc in (0, 1, 3):
        for s0 in (1.0, 0.8, 0.5):
            b = {d: np.stack([R.system(P, scen[sc], A.path_state(xi, s0, d, P.nq))[0] for xi in x]) for d in (0.0, 1.0, 1.7, -3.0)}
            for d in (0.0, 1.7, -3.0):
                scale = np.maximum(np.linalg.norm(b[d], axis=1), 1.0)
                worst = max(worst, float((np.linalg.norm(A.emu_rhs(P, x, scen[sc], s0, d) - b[d], axis=1) / scale).max()))
                worst_aff = max(worst_aff, float((np.linalg.norm(b[d] - b[0.0] - d * (b[1.0] - b[0.0]), axis=1) / scale).max()))
    print("path-acceleration margin, %s: transformed record vs oracle %.2e, |b(d) - b(0) - d b2| %.2e (units of max(|b|, 1))" % (name, worst, worst_aff))
    assert worst <= 1e-12 and worst_aff <= 1e-12


@pytest.mark.parametrize("name", A.NAMES)
def test_table_holds_every_class(arrangements, name):
    """At least five jobs of every class the arrangement can hold, on the reference alone; the launches of the table; few none jobs in
    motion (each costs the reference its grid), and a none job has rho_ref above the limit on the whole grid."""
    launches = A.cases(arrangements, name)
    counts = A.class_counts(launches)
    n_none = sum(int(((L["pclass"] == "none") & L["jobs"].moving[:, None]).sum()) for L in launches)
    n_cmp = sum(int((A.steady(L) & (L["pclass"] == "none")).sum()) for L in launches)
    print("path-acceleration margin, %s: classes %s; none jobs in motion %d, none jobs whose counts are compared %d" % (name, counts, n_none, n_cmp))
    for c in A.expected_classes(launches[0]["P"]):
        assert counts[c] >= 5, (name, c, counts)
    assert n_none <= 20 and n_cmp >= 5
    assert sorted(L["pclass"].size for L in launches) == [1, 1, 37, 37, 37, 256, 259]
    assert [(L["d_max"], L["speed"]) for L in launches] == [(8.0, 1.0)] * 6 + [(3.0, 0.5)]
    for L in launches:
        J = L["jobs"]
        for i, sc in np.argwhere(L["pclass"] == "none"):
            assert not any(J.accepted(int(i), int(sc), d) for d in J.grid())


@pytest.mark.parametrize("name", A.NAMES)
def test_bracket_certificates_and_reference(arrangements, name):
    """A.check_answer on the emulation's answer to every launch: in - out = d_max 2^-31 where an end was bisected, the certificates at
    all four ends, rho_ref on its own side at every in and out, the class of every job."""
    for k, L in enumerate(A.cases(arrangements, name)):
        bad = A.check_answer(L, L["emu"])
        assert not bad, (name, k, bad[:5])


@pytest.mark.parametrize("name", A.ONE_BODY)
def test_wave_form_on_one_body_shapes(arrangements, name):
    """The wave-per-job job on the one-body shapes: the same checks, and the same answer as the lane form on the jobs that bisect
    no end."""
    for k, L in enumerate(A.cases(arrangements, name)):
        out = A.run_launch(L, form=0)
        bad = A.check_answer(L, out)
        assert not bad, (name, k, bad[:5])
        m = A.steady(L)
        assert np.array_equal(out["accel"][m], L["emu"]["accel"][m])


@pytest.mark.parametrize("name", A.NAMES)
def test_known_answers(arrangements, name):
    """|d - d_known| <= 1e-6 |d_known| (the family's bound for the closed forms of DESIGN 3.10): lift-off, sink, falling and rising on
    every arrangement in every scenario; slide and the compensated tilt where sliding binds.  Launches 0 (speed 1) and 6 (speed 0.5,
    d_max 3)."""
    launches = A.cases(arrangements, name)
    for k in (0, 6):
        L = launches[k]
        w = A.known_answers(L, L["emu"]["accel"], name)
        print("path-acceleration margin, %s, launch %d: largest relative |d - d_known| vertical %.2e, slide %.2e, comp %.2e (%d ends)"
              % (name, k, w["vertical"], w["slide"], w["comp"], w["n"]))
        assert w["n"] >= 5 or k == 6          # (d_max = 3 clips most of the closed-form ends of the slow launch)
        assert w["vertical"] <= 1e-6 and w["slide"] <= 1e-6 and w["comp"] <= 1e-6


@pytest.mark.parametrize("name", A.NAMES)
def test_descent_seeded_windows(arrangements, name):
    """The compensated tilt: windows that exclude 0 and both ends, seeded by the descent search alone (sigma = 1: one decided slope
    step, sigma = 4: three).  The emulation in both forms agrees with the replay on rho_ref; with the sign of the slope inverted the
    replay ends them as none -- on at least five jobs of every arrangement with friction (the table of a shape without friction holds no
    compensated tilt: pathacc_ref)."""
    launches = A.cases(arrangements, name)
    P = launches[0]["P"]
    n_seeded = n_flip = 0
    steps, per_kind = set(), {}
    for L in launches[:4]:
        J = L["jobs"]
        wave = A.run_launch(L, form=0) if P.nb == 1 else L["emu"]
        for i, kind in enumerate(L["kinds"]):
            if not kind.startswith("comp"):
                continue
            for sc in range(J.ns):
                if L["pclass"][i, sc] != "window" or per_kind.get(kind, 0) >= 3:
                    continue
                per_kind[kind] = per_kind.get(kind, 0) + 1
                tr = []
                ac, n_ev = J.replay(i, sc, trace=tr)
                assert np.isfinite(ac).all() and -J.d_max < ac[1] < ac[0] <= ac[2] < ac[3] < J.d_max and n_ev > 3 + 2
                assert len(tr) >= 1 and tr[0][0] == 0.0   # (the nominal point again: the first slope step is taken there)
                steps.add(len(tr))
                for out in (L["emu"], wave):
                    assert np.abs(out["accel"][i, sc] - ac).max() <= 1e-6 * np.abs(ac).max(), (name, i, sc, out["accel"][i, sc], ac)
                n_seeded += 1
                if np.isinf(J.replay(i, sc, flip=True)[0][0]):
                    n_flip += 1
    print("path-acceleration margin, %s: windows seeded by the descent search %d (slope steps %s), none with the sign flipped %d"
          % (name, n_seeded, sorted(steps), n_flip))
    if P.nf == 3:
        assert n_seeded >= 5 and n_flip >= 5
    else:
        assert not per_kind               # (no compensated tilt in the table of a shape without friction)
    if name in A.SLIDING_BINDS:
        # (sigma = 1: the window reaches up to about d = 4, the second midpoint, so one or two steps; sigma = 4: it ends below 1, three
        #  or four)
        assert min(steps) >= 1 and max(steps) >= 3, steps


@pytest.mark.parametrize("name", A.NAMES)
def test_fma_twin_takes_the_same_evaluations(arrangements, name):
    """The -mfma -ffp-contract=fast build of the emulation (how hipcc contracts for the device): the same class everywhere, the same
    answer and the same solve counts on the all and none jobs that are decided on the reference."""
    if not A.have_fma_twin():
        pytest.skip("the host has no FMA instruction (/proc/cpuinfo): the twin is not built")
    for L in A.cases(arrangements, name):
        out = A.run_launch(L, fma=True)
        assert np.array_equal(A.device_class(out["accel"], L["d_max"]), L["pclass"])
        m = A.steady(L)
        assert np.array_equal(out["iters"][m], L["emu"]["iters"][m]) and np.array_equal(out["accel"][m], L["emu"]["accel"][m])


def test_plan_reductions_on_the_host():
    """upr_bal_speed_window on the accel layout and upr_bal_pathacc_limit compiled for the host against numpy, on random values with
    ties, infinities, a plan at rest and a plan whose acceleration is outside its box: window and knot exactly, limit to 1e-12."""
    from upright_amd.problem import thing_problem
    import json
    from pathlib import Path

    P = thing_problem(json.load(open(Path(__file__).resolve().parent / "golden" / "arrangements.json"))["pink_bottle"])
    rng = np.random.default_rng(11)
    B, nk, ns = 5, 21, 3
    accel = np.round(rng.uniform(-8.0, 8.0, (B, nk, ns, 4)), 1)          # (one decimal: ties between knots)
    accel[1, 3, 0] = [np.inf, -8.0, -np.inf, 8.0]
    accel[2, :, 1, 0] = -8.0; accel[2, :, 1, 2] = 8.0
    nq = P.nq
    xs = rng.uniform(-1.0, 1.0, (B, nk, 3 * nq))
    xs[4, :, nq:] = 0.0
    # (joint 0 outside its box at two knots, at speed 0.5 too, moving forwards at one and backwards at the other: d <= -2 and d >= 2)
    xs[3, 7:9, 2 * nq] = 4.0 * (float(P.x_ub[2 * nq]) + 1.0)
    xs[3, 7, nq], xs[3, 8, nq] = 0.5, -0.5
    for speed in (1.0, 0.5):
        w, kn, lim = A.emu_plan(P, accel, xs, speed)
        w0, kn0, lim0 = A.numpy_plan(P, accel, xs, speed)
        assert np.array_equal(w, w0) and np.array_equal(kn, kn0)
        assert lim[4, 0] == -np.inf and lim[4, 1] == np.inf and np.array_equal(lim[4], lim0[4])
        assert lim[3, 0] > lim[3, 1]
        rel = np.abs(lim[:4] - lim0[:4]) / np.abs(lim0[:4])
        print("path-acceleration margin: limit, host build of the kernel body vs numpy at speed %g, largest relative difference %.2e" % (speed, rel.max()))
        assert rel.max() <= 1e-12
