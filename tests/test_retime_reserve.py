"""The retiming with a reserve (upright_amd/csrc/upr_retime_rsv.h) through its host emulation (tests/emu/upr_retime_rsv_emu.cpp): the mask
jobs in both forms, then the programme of upr_retime.h's path kernel, against the closed form of a sliding translation with the reserve
taken off its bound, the CPU reference at the displaced joint-space states and numpy's programme (tests/retime_rsv_ref.py); the
assertions tests/test_gpu_retime_reserve.py repeats on the device's answers.

Observed on the emulation (x86-64): slide, r = 0.25 mu0 g0: the closest closed-form decisions 1.0e-3 (span_0, span_1) and 6.2e-3 (e_z)
mu0 g0 from their bounds, masks equal, durations 2.351804 s (span_0, span_1) and 1.856566 s (e_z, the plain law); generic plans 0 and 1,
two scenarios, M = 5, three directions, r = 0.25: undecided edges 0.000 of 2000, durations 1.5055, 2.2185, 1.8366, inf; foam_die2 (B = 1,
M = 3, two directions): undecided edges 0.000 of 360; FMA twin: masks equal."""
import time

import numpy as np
import pytest

import disturb_ref as D
import retime_ref as Q
import retime_rsv_ref as V

_SLOWEST = [0.0, ""]


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.time()
    yield
    dt = time.time() - t0
    if dt > _SLOWEST[0]:
        _SLOWEST[:] = [dt, request.node.name]
    print("retime with a reserve (emulation): %s took %.1f s; the slowest so far: %s, %.1f s" % (request.node.name, dt, _SLOWEST[1], _SLOWEST[0]))


def run(P, xs, params, speeds, **kw):
    return V.run_emu(P, xs, params, speeds, **kw)


def test_closed_form_slide(arrangements):
    """1. r = 0.25 mu0 g0 along span_0, span_1 and e_z of the tray: masks == the closed form with the reserve taken off the bound at both
    ends, duration and level == numpy's programme on them; with span_0 the law is strictly slower than the plain one."""
    V.body_closed_form(run, arrangements)
    V.body_closed_form(lambda *a, **k: run(*a, **dict(k, form=0)), arrangements)


def test_reference_on_generic_plans(arrangements):
    """2. plans 0 and 1 of retime_ref's generic case, both scenarios, M = 5, boxes on, span_0, span_1, e_z in the tray frame, r = 0.25:
    at most 10 % undecided edges and box decisions away from their bounds on the reference alone; masks on decided edges, duration and
    level on decided plans, the invariants on the answer."""
    V.body_reference(run, arrangements)


def test_zero_reserve_is_the_plain_retiming(arrangements):
    """3. r = 0 with any valid dirs: duration, level, reach, edges and iters of retime_ref's emulation bit for bit, in both forms."""
    assert V.body_zero_reserve(run, arrangements) == 6


def test_monotone_in_the_reserve_and_the_directions(arrangements):
    """4. r in {0, 0.25, 0.5, 1}: each mask a subset of the previous, durations non-decreasing; a subset of the directions gives a
    superset of the masks."""
    V.body_monotone(run, arrangements)


def test_the_law_keeps_what_it_reserved(arrangements):
    """5. the retimed states of every finite law of test 2 through the disturbance margin's emulated job: r_lo <= -0.999 r and r_hi >=
    0.999 r along every direction where the reference is decided; the plain law falls short somewhere."""
    def margin(P, x, theta, dirs):
        return D.run_emu(P, x, theta[None], False, dirs, 8.0, "tray")["reach"][:, :, 0, 0::2]
    V.body_keeps_reserve(run, arrangements, margin)


def test_frames_and_order(arrangements):
    """6. tray-frame dirs against the same directions rotated in numpy and passed as world (the slide: C_we is constant); (u, -u) against
    (u); permuted dirs."""
    V.body_frames_and_order(run, arrangements)


def test_shapes(arrangements):
    """7. common, start / end, M = 1 and M = 32, n_dir = 1 and 32."""
    V.body_shapes(run, arrangements)


def test_wave_form_and_multi_body_arrangement(arrangements):
    """8. the wave-per-job body on the one-body shape (test 2's assertions, and the lane form's answer) and foam_die2 (two bodies, eight
    contacts), B = 1, M = 3, n_dir = 2."""
    out = V.body_reference(run, arrangements, form=0)
    G = V.generic_case(arrangements)
    lane = run(G["P"], G["xs"], G["params"], G["speeds"], dirs=G["dirs"], reserve=G["r"])
    bits = Q.decided_bits(G["rsv"]["decided"])
    assert np.array_equal(out["edges"][:2] & bits, lane["edges"][:2] & bits) and np.array_equal(out["duration"][:2], lane["duration"][:2])
    V.body_reference(run, arrangements, name="foam_die2", B=1, plans=1, speeds=(0.5, 1.0, 1.5), n_dir=2)


def test_fma_twin(arrangements):
    """9. the -mfma -ffp-contract=fast build (how hipcc contracts for the device): masks equal on decided edges."""
    if not V.have_fma_twin():
        pytest.skip("the host has no FMA instruction (/proc/cpuinfo): the twin is not built")
    G = V.generic_case(arrangements)
    bits = Q.decided_bits(G["rsv"]["decided"])
    for form in (-1, 0):
        twin = run(G["P"], G["xs"], G["params"], G["speeds"], dirs=G["dirs"], reserve=G["r"], form=form, fma=True)
        plain = run(G["P"], G["xs"], G["params"], G["speeds"], dirs=G["dirs"], reserve=G["r"], form=form)
        assert np.array_equal(twin["edges"][:2] & bits, plain["edges"][:2] & bits)
    S = V.slide_case(arrangements)
    out = run(S["P"], S["xs"], S["params"], S["speeds"], dirs=S["dirs"][:1], reserve=S["r"], boxes=False, fma=True)
    assert np.array_equal(out["edges"], S["refs"][0]["masks"])
