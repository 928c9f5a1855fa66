"""The retiming with substeps (upright_amd/csrc/upr_retime_sub.h) through its host emulation (tests/emu/upr_retime_sub_emu.cpp): the
refinement of the plan, the mask jobs in both forms, then the programme of upr_retime.h's path kernel, against the closed form of a
sliding translation between its knots, the CPU reference at the joint-space states of the substep points and numpy's programme
(tests/retime_sub_ref.py); the assertions tests/test_gpu_retime_substeps.py repeats on the device's answers."""
import time

import numpy as np
import pytest

import balance_ref as R
import replay_ref as Y
import retime_ref as Q
import retime_sub_ref as U

_SLOWEST = [0.0, ""]


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.time()
    yield
    dt = time.time() - t0
    if dt > _SLOWEST[0]:
        _SLOWEST[:] = [dt, request.node.name]
    print("retime with substeps (emulation): %s took %.1f s; the slowest so far: %s, %.1f s" % (request.node.name, dt, _SLOWEST[1], _SLOWEST[0]))


def run(P, xs, params, speeds, **kw):
    return U.run_emu(P, xs, params, speeds, **kw)


def plain(P, xs, params, speeds, **kw):
    return Q.run_emu(P, xs, params, speeds, **kw)


def test_closed_form_slide_between_the_knots(arrangements):
    """1. lattices [1.1185], [1.11, 1.1185] and the slide's own at R in {1, 2, 4, 8}: masks == the closed form at every substep point,
    duration and level == numpy's programme; at 1.1185 R = 1 and 2 give the uniform law (the midpoints miss the peak), R = 4 and 8
    none, blocked at (4, 16); the R = 4 law of the narrow lattice replayed on a 10 ms clock rejects no sample, the R = 1 law six."""
    def replay(P, xs, params, speeds, level, tick, K):
        return Y.run_emu(P, xs, params, speeds, level, tick, K=K, boxes=False)
    U.body_slide(run, arrangements, replay)
    U.body_slide(lambda *a, **k: run(*a, **dict(k, form=0)), arrangements)


def test_one_substep_is_the_plain_retiming(arrangements):
    """2. R = 1 through the new jobs: duration, level, reach, edges and iters of retime_ref's emulation bit for bit, in both forms."""
    assert U.body_r1_is_the_plain_retiming(run, plain, arrangements) == 8


def test_reference_on_generic_plans(arrangements):
    """3. plans 0 and 1 of retime_ref's generic case, both scenarios, M = 5, boxes on, R = 3: at most 10 % undecided edges and box
    decisions away from their bounds on the reference alone; masks on decided edges, duration and level on decided plans, the invariants
    on the answer.  Then foam_die2 (two bodies: the wave form), B = 2, M = 3, R = 2."""
    U.body_reference(run, arrangements)
    U.body_reference(run, arrangements, name="foam_die2", B=2, plans=2, speeds=(0.5, 1.0, 1.5), Rs=2)


def test_the_point_sets_nest(arrangements):
    """4. masks(R = 4) within masks(R = 2) within masks(R = 1) on decided edges, durations non-decreasing."""
    U.body_nesting(run, arrangements)


def test_fine_records_and_substates(arrangements):
    """5. the refinement against numpy's Hermite at the replay's state tolerances, the knots bit for bit; the substates of every feasible
    generic law through the balance check's emulation."""
    errs = U.body_fine_records(arrangements)
    print("retime with substeps, fine records: errors q, qdot, qddot %s" % errs.tolist())
    out = U.body_substates_are_balanced(run, arrangements, lambda P, x, th: R.run_emu(P, x, th[None], False)["rho"][:, 0])
    # r = 0 and r = R of the substates are retime_ref's departing and arriving states, as doubles
    G = U.generic_case(arrangements)
    _, x = U.substates(G["P"], G["xs"][:2], out["level"], G["speeds"], 3)
    _, dep, arr = Q.retimed_states(G["xs"][:2], out["level"], G["speeds"], float(G["P"].dt), G["P"].nq)
    ok = np.isfinite(out["duration"])
    assert ok.any() and np.array_equal(x[ok][:, :, 0], dep[ok]) and np.array_equal(x[ok][:, :, 3], arr[ok])


def test_boxes(arrangements):
    """6. the boxes cut the edges numpy cuts at every substep point, and only with boxes=True."""
    U.body_boxes(run, arrangements)


def test_common_time_law(arrangements):
    """7. common=True runs the programme on the AND of the per-scenario masks of the same call."""
    U.body_common(run, arrangements)


def test_fma_twin_and_wave_form(arrangements):
    """8. the -mfma -ffp-contract=fast build (how hipcc contracts for the device) and the wave-per-job body on the one-body shape: masks
    equal on decided edges."""
    G = U.generic_case(arrangements)
    a = run(G["P"], G["xs"], G["params"], G["speeds"], substeps=3)
    wave = U.body_reference(run, arrangements, form=0)
    assert U.agree(wave, a, G["sub"], 2) >= 100
    if not U.have_fma_twin():
        pytest.skip("the host has no FMA instruction (/proc/cpuinfo): the twin is not built")
    for form in (-1, 0):
        twin = run(G["P"], G["xs"], G["params"], G["speeds"], substeps=3, form=form, fma=True)
        U.agree(twin, a, G["sub"], 2)
    S = Q.slide_case(arrangements)
    out = run(S["P"], S["xs"], S["params"], np.array(U.NARROW), substeps=4, boxes=False, fma=True)
    assert np.array_equal(out["edges"], U.slide_ref(arrangements, U.NARROW, 4)["masks"])
    U.body_fine_records(arrangements, fma=True)


def test_layouts_of_params(arrangements):
    """9. params NULL, shared and per instance give the same result: the parameter set of a job comes from the fine layout."""
    U.body_layouts(run, arrangements)
