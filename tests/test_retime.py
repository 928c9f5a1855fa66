"""The retiming of a plan on a speed lattice (upright_amd/csrc/upr_retime.h) through its host emulation (tests/emu/upr_retime_emu.cpp):
the mask jobs in both forms and the dynamic programme of the path kernel against the closed form of a sliding translation, the CPU
reference at the joint-space state and numpy's programme (tests/retime_ref.py); the assertions tests/test_gpu_retime.py repeats on the
device's answers.

Observed on the emulation (x86-64): slide, the closest closed-form decision 1.7e-3 mu0 g0 from the bound, masks equal; generic plans
(B = 3, two scenarios, M = 5: 3000 edges), undecided edges 0.000, all six plans decided; FMA twin: masks equal."""
import numpy as np
import pytest

import balance_ref as R
import pathacc_ref as A
import retime_ref as Q


def run(P, xs, params, speeds, start=-1, end=-1, common=False, boxes=True, form=-1, fma=False):
    return Q.run_emu(P, xs, params, speeds, start, end, common, boxes, form, fma)


def test_closed_form_slide(arrangements):
    """1. masks == the closed form |s^2 c + d w| <= mu0 g0 at both ends, duration and level == numpy's programme; speed 1.25 is cut
    at the peak and the law is no slower than the plan."""
    Q.body_closed_form(run, arrangements)


def test_reference_on_generic_plans(arrangements):
    """2. quintic joint-space motions, B = 3, nominal and a shifted centre of mass, M = 5: at most 10 % undecided edges on the reference
    alone; masks on decided edges, duration and level on decided plans."""
    Q.body_reference(run, arrangements)


def test_invariants_on_the_answer_alone(arrangements):
    """3. path over set edges, start / end honoured, segment times add up, numpy's programme on the returned masks, level = -1 and reach
    where no law exists."""
    Q.body_invariants(run, arrangements)


def test_retimed_states_are_balanced(arrangements):
    """4. the retimed states of every feasible plan through the balance check's emulation."""
    Q.body_independent_path(run, arrangements, lambda P, x, th: R.run_emu(P, x, th[None], False)["rho"][:, 0])


def test_one_level_against_the_speed_margin(arrangements):
    """5. against the speed margin's emulation over the knots."""
    import speed_ref as S

    def speed4(P, xs, params):
        return S.run_emu(P, xs.reshape(-1, xs.shape[-1]), params, False)["speed"].reshape(xs.shape[0], xs.shape[1], -1, 4)
    Q.body_speed_margin(run, arrangements, speed4)


def test_admissible_edges_lie_in_the_path_accel_window(arrangements):
    """6. against the path-acceleration margin's emulation at the departing knot (its job on the knots of the plan: the plan entry's
    jobs; the entry itself is called on the device)."""
    def pathacc(P, xs, params, speed, d_max):
        acc = A.run_emu(P, xs.reshape(-1, xs.shape[-1]), params, False, d_max=d_max, speed=speed)["accel"]
        return acc[..., 0::2].reshape(xs.shape[0], xs.shape[1], -1, 2)
    Q.body_path_accel(run, arrangements, pathacc)


def test_common_time_law(arrangements):
    """7. common=True runs the programme on the AND of the per-scenario masks of the same call."""
    Q.body_common(run, arrangements)


def test_boxes(arrangements):
    """8. velocity and acceleration boxes cut exactly the edges numpy cuts."""
    Q.body_boxes(run, arrangements)


def test_edge_shapes(arrangements):
    """9. M = 32 (bit 31, the full mask), M = 1, a lattice with 0 and end = 0.0, start given and free, N + 1 levels and N mask rows."""
    Q.body_edge_shapes(run, arrangements)


def test_wave_form_on_the_one_body_shape(arrangements):
    """10. the wave-per-job body on the one-body shape: test 2's assertions, and the lane form's answer."""
    out = Q.body_reference(lambda *a, **k: run(*a, **dict(k, form=0)), arrangements)
    G = Q.generic_case(arrangements)
    lane = run(G["P"], G["xs"], G["params"], G["speeds"])
    bits = Q.decided_bits(G["ref"]["decided"])
    assert np.array_equal(out["edges"] & bits, lane["edges"] & bits) and np.array_equal(out["duration"], lane["duration"])


def test_multi_body_arrangement(arrangements):
    """10. foam_die2 (two bodies, eight contacts), B = 2, M = 3."""
    Q.body_reference(run, arrangements, name="foam_die2", B=2, speeds=(0.5, 1.0, 1.5))


def test_fma_twin(arrangements):
    """11. the -mfma -ffp-contract=fast build (how hipcc contracts for the device): masks equal on decided edges."""
    if not Q.have_fma_twin():
        pytest.skip("the host has no FMA instruction (/proc/cpuinfo): the twin is not built")
    G = Q.generic_case(arrangements)
    bits = Q.decided_bits(G["ref"]["decided"])
    twin, plain = run(G["P"], G["xs"], G["params"], G["speeds"], fma=True), run(G["P"], G["xs"], G["params"], G["speeds"])
    assert np.array_equal(twin["edges"] & bits, plain["edges"] & bits)
    S = Q.slide_case(arrangements)
    assert np.array_equal(run(S["P"], S["xs"], S["params"], S["speeds"], boxes=False, fma=True)["edges"], S["ref"]["masks"])


def test_programme_of_the_path_kernel_on_random_masks():
    """The path kernel's body on random masks (ties, empty rows, M = 1 .. 32, start / end, common) against numpy's programme: ==."""
    import ctypes as C

    from upright_amd._capi import iptr, ptr

    rng = np.random.default_rng(3)
    lib = Q.emu_lib()
    for M, ns, common, start, end, dens in ((1, 1, 0, -1, -1, 0.9), (5, 2, 0, -1, -1, 0.5), (5, 3, 1, 2, 0, 0.8), (32, 2, 1, -1, 31, 0.7), (32, 1, 0, 31, -1, 0.15),
                                            (7, 2, 0, 3, 3, 0.3)):
        B, N, h = 3, 9, 0.1
        speeds = np.cumsum(rng.integers(1, 3, M)) * 0.25       # (multiples of 1 / 4: exact ties between laws)
        edges = np.zeros((B, ns, N, M), dtype=np.uint32)
        for mp in range(M):
            edges |= (rng.random(edges.shape) < dens).astype(np.uint32) << np.uint32(mp)
        nout = (B,) if common else (B, ns)
        out = dict(edges=edges, duration=np.zeros(nout), level=np.zeros(nout + (N + 1,), dtype=np.int32), reach=np.zeros(nout + (2,), dtype=np.int32))
        rc = lib.emu_ret_path(B, N + 1, ns, M, ptr(speeds), C.c_double(h), start, end, common, edges.ctypes.data_as(C.POINTER(C.c_uint)), ptr(out["duration"]),
                              iptr(out["level"]), iptr(out["reach"]))
        assert rc == 0
        Q.check_invariants(out, speeds, h, start, end, bool(common))
