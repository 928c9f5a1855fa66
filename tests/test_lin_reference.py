"""The linearisation reference (tests/lin_check.py) against the linearisation kernels' source through the host emulation
(tests/emu, emu_linearize: trajectory mode), in both source forms (upr_linearize.h's phases and upr_linearize2.h's lane jobs), over
every case of the device screen's table (tests/test_gpu_lin_screen.py).  This checks the reference and the cases' inputs before any
GPU time: the conditions under which the tolerances mean something are asserted on the oracle alone, and a numpy test shows that the
comparer flags a wrong entry of every slot class, swapped instances, swapped knots and a wrong clock."""
import ctypes as C

import numpy as np
import pytest

import lin_check
import test_gpu_lin_screen as S
from test_emu import Emu, _NoDevice
from upright_amd import _capi

p = _capi.ptr
# one body (the shapes of test_emu.test_linearize_kernel_source, its numbers): everything to 1e-13, the Jacobian to 1e-12
ONE_BODY = dict(lin_check.TOL, g=1e-13, gx=1e-12, cost=1e-13, grad=1e-13, hess=1e-13, term_c=1e-13, term_C=1e-13)
_CACHE = {}


def case_and_reference(name, monkeypatch):
    """(case, expected records), built once per case of the table and shared by the tests of this module, unchanged"""
    if name not in _CACHE:
        from upright_amd import control_bindings
        monkeypatch.setattr(control_bindings, "BatchMPC", _NoDevice)   # (the golden builders keep the manager's Problem only)
        c = S.build_case(name)
        E = lin_check.expected_records(c)
        for a in list(c.values()) + list(E.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = (c, E)
    return _CACHE[name]


def emu_records(c, form):
    P = c["P"]
    B = c["xs"].shape[0]
    e = Emu(P, B, bp=c["bp"])
    try:
        e.E.emu_set_lin_form(form)
        e.E.emu_set_dynamic(p(c["dyn"]) if c["dyn"] is not None else None, p(c["pflag"]) if c["dyn"] is not None else None)
        e.E.emu_set_way_q(p(c["way_q"]) if c["way_q"] is not None else None)
        return e.linearize(c["way"], c["t0"], c["xs"], c["us"])
    finally:
        e.E.emu_set_lin_form(1); e.E.emu_set_dynamic(None, None); e.E.emu_set_way_q(None)


# distinct inputs of the table (cases that differ only in the launch form share builder and arguments)
def _distinct():
    seen, out = set(), []
    for n, v in S.CASES.items():
        key = (v[0].__name__, tuple(sorted(v[1].items())))
        if key not in seen:
            seen.add(key); out.append(n)
    return out


DISTINCT = _distinct()


@pytest.mark.parametrize("name", DISTINCT)
def test_linearisation_reference_against_emulation(name, monkeypatch):
    c, E = case_and_reference(name, monkeypatch)
    P = c["P"]
    tol = ONE_BODY if P.nb == 1 else lin_check.TOL
    for form in (0, 1):
        res = lin_check.compare(E, lin_check.split_records(P, emu_records(c, form)), allowance=lin_check.projectile_allowance(c))
        print("%s form %d: %s" % (name, form, lin_check.fmt(res)))
        assert set(res) == set(lin_check.SLOTS) - (set() if P.n_state_rows else {"rows", "row_grad"})
        assert not lin_check.failures(res, tol), (name, form, lin_check.failures(res, tol))


def quat_to_rot_xyzw(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _angle(Ra, Rb):
    return np.arccos(np.clip(0.5 * (np.trace(Ra.T @ Rb) - 1.0), -1.0, 1.0))


@pytest.mark.parametrize("name", DISTINCT)
def test_case_inputs_make_the_tolerances_mean_something(name, monkeypatch):
    """Conditions on the inputs, from the oracle alone: every instance has its own parameters, target and non-zero time; the
    velocity-dependent part of the constraint (g at (q, v, a) less g at (q, 0, a): the omega x I omega and centripetal terms) exceeds
    1e-6, 1e5 times the tolerance; every pair's centre distance exceeds 0.05 m at the sampled states; the orientation error stays
    below 2.5 rad."""
    c, E = case_and_reference(name, monkeypatch)
    P = c["P"]
    B, nq = c["xs"].shape[0], P.nq
    assert np.all(c["t0"] > 0) and (B < 2 or len(set(c["t0"][:17])) == min(B, 17))
    if B > 1:
        assert all(np.abs(c[k][0] - c[k][1]).max() > 1e-4 for k in ("bp", "way"))
    assert np.abs(c["xs"][:, 1:] - c["xs"][:, :-1]).max() > 0.1 and np.abs(c["xs"][:, :, nq:]).max() > 0.1
    if len(P.way_t) > 1:
        t = c["t0"][:, None] + np.arange(P.N + 1)[None] * P.dt
        assert (t < P.way_t[1]).any() and (t > P.way_t[0]).any() and ((t > P.way_t[0]) & (t < P.way_t[1])).any()
    if c["pflag"] is not None:
        assert set(c["pflag"]) == {0.0, 1.0} and np.abs(c["dyn"][0] - c["dyn"][1]).max() > 1e-3
    worst_v, worst_d, worst_a = np.inf, np.inf, 0.0
    for b in range(min(B, 8)):
        O = lin_check.instance_oracle(c, b)
        for k in range(0, P.N, max(1, P.N // 10)):
            x = c["xs"][b, k]
            x_still = x.copy(); x_still[nq:2 * nq] = 0.0
            worst_v = min(worst_v, np.abs(O.eq_constraint(x, c["us"][b, k], jac=False) - O.eq_constraint(x_still, c["us"][b, k], jac=False)).max())
        for k in range(1, P.N):
            x = c["xs"][b, k]
            if len(P.pair_a):
                cen = O.sphere_centers(x).copy()
                for i, f in enumerate(P.sph_frame):
                    if f <= -2:
                        cen[i] = S.obstacle_at(c["dyn"][b], k * P.dt).reshape(-1, 9)[-2 - f, :3] + P.sph_off[i]
                for a, b2 in zip(P.pair_a, P.pair_b):
                    worst_d = min(worst_d, np.linalg.norm(cen[a] - cen[b2]) if b2 >= 0 else np.inf)
            if c["way_q"] is not None:
                R = P.chain.forward(x[:nq])[1]
                worst_a = max(worst_a, max(_angle(R, quat_to_rot_xyzw(q)) for q in c["way_q"][b]))
    print("%s: velocity part of g %.2e, smallest centre distance %.3f, largest orientation error %.2f rad" % (name, worst_v, worst_d, worst_a))
    assert worst_v > 1e-6 and worst_d > 0.05 and worst_a < 2.5


def test_the_comparer_has_teeth(monkeypatch):
    """Pure numpy, on the expected records of two cases: an entry of every slot class off by 1e-9 relative, the records of two
    instances swapped, of two knots swapped, and every knot time late by dt -- each is flagged at the project's tolerances, and
    the unperturbed records are not."""
    for name in ("box_only", "thrown_ball", "orientation"):
        c, E = case_and_reference(name, monkeypatch)
        P = c["P"]
        assert not lin_check.failures(lin_check.compare(E, {k: v.copy() for k, v in E.items()}))
        for slot in lin_check.SLOTS:
            if E[slot].size == 0:
                continue
            bad = {k: v.copy() for k, v in E.items()}
            i = np.unravel_index(np.argmax(np.abs(E[slot])), E[slot].shape)
            assert abs(E[slot][i]) > 2e-2, (name, slot)
            bad[slot][i] *= 1.0 + 1e-9
            res = lin_check.compare(E, bad)
            assert set(lin_check.failures(res)) == {slot}, (name, slot, res)
            assert res[slot][1] == i[0] and (slot.startswith("term") or res[slot][2] == i[1] + (slot in ("rows", "row_grad"))), (slot, res[slot], i)
        stage = [s for s in lin_check.SLOTS if E[s].size and not s.startswith("term")]
        swapped_inst = {k: v.copy() for k, v in E.items()}
        for k in swapped_inst:
            swapped_inst[k][[0, 1]] = swapped_inst[k][[1, 0]]
        f = lin_check.failures(lin_check.compare(E, swapped_inst))
        assert set(f) == {s for s in lin_check.SLOTS if E[s].size}, (name, sorted(f))
        swapped_knot = {k: v.copy() for k, v in E.items()}
        for k in stage:
            swapped_knot[k][:, [3, 4]] = swapped_knot[k][:, [4, 3]]
        f = lin_check.failures(lin_check.compare(E, swapped_knot))
        assert set(f) == set(stage), (name, sorted(f))
        # a clock that is late by dt: whatever depends on the time moves (two waypoints: cost and gradient, box rows, terminal
        # residual; a dynamic obstacle: its rows)
        late = lin_check.expected_records(c, time_shift=P.dt)
        f = lin_check.failures(lin_check.compare(E, late))
        timed = {"cost", "grad"} if len(P.way_t) > 1 else set()
        if (P.ee_box and len(P.way_t) > 1) or P.n_dyn:
            timed |= {"rows"}
        assert timed and timed <= set(f), (name, sorted(f))
