"""CPU twin of tests/test_gpu_qp_fallback_screen.py: the table of that screen held against the selection rules (upr_qp_select.h through
emu_qp_select, the rules upr_batch_create runs) and against the lists the two older QP structures are instantiated from, and the
emulation of every case on the emulation's own linearisation.

  * every case resolves, under its knobs, to the structure and the kernel name the table states;
  * the table cannot lose coverage: every entry of UPR_QP2_SHAPES at every lane count qp2_launcher accepts, every lane count
    qp_generic_launcher accepts, and a case (or, where no fixture can run, a host-only problem) for every reason upr_qp_plan /
    upr_qp3_jit_capable give for leaving the production structure under default knobs;
  * the emulated kernels run every case to ITERS iterations with finite output, and the converged leg's inputs converge.

The reason "hard equality on frictionless contacts of several bodies" is host-only: the only frictionless multi-body fixture
(robust_8corner) admits no motion at all with hard object-dynamics rows (tests/test_gpu_parity.py,
test_config4_robust_mpc_solve_against_oracle), so no device case could converge or be compared with anything."""
import ctypes as C
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import test_gpu_qp_fallback_screen as F  # noqa: E402
from test_emu import EMU, Emu, _knobs, _NoDevice, _select  # noqa: E402
from upright_amd.problem import thing_problem  # noqa: E402

CSRC = HERE.parent / "upright_amd" / "csrc"
GENERIC, SECOND, PRODUCTION, RUN_TIME = F.GENERIC, F.SECOND, F.PRODUCTION, 2

# the cases the screen was specified with: a case deleted from the table fails test_table_is_complete
REQUIRED = (["generic_headline", "generic_rows", "generic_rows_soft", "generic_soft_boxes", "generic_thing_demo", "generic_ur10_N10",
             "generic_dice", "generic_box_arch", "generic_cups", "generic_robust",
             "fallback_N65", "fallback_N65_soft", "fallback_26_rows", "fallback_no_jit_N12", "qp2_9x1x4x3_nt512"]
            + ["generic_%s_nt%d" % (s, nt) for nt in (64, 128, 256, 512, 1024) for s in ("rows_soft", "dice")]
            + ["qp2_%s_nt%d" % (s, nt) for s in ("9x1x4x3", "9x1x4x1", "6x1x4x1", "6x1x4x3", "9x2x8x3") for nt in (64, 128, 256)])


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    from upright_amd import control_bindings
    monkeypatch.setattr(control_bindings, "BatchMPC", _NoDevice)   # (the golden builders keep their manager's Problem: no handle)


def knobs_of(env):
    """The environment at upr_batch_create as the knobs it reads from it (upr_api.hip)"""
    kw = {}
    if "UPR_QP_KERNEL" in env:
        kw["qp_kernel"] = int(env["UPR_QP_KERNEL"])
    if "UPR_QP_GENERIC" in env:
        kw["qp_generic"] = int(env["UPR_QP_GENERIC"]) != 0
    if "UPR_QP3_JIT" in env:
        kw["qp3_jit"] = int(env["UPR_QP3_JIT"])
    if "UPR_QP_NT" in env:
        kw.update(qp_nt_set=True, qp_nt=int(env["UPR_QP_NT"]))
    if "UPR_QP_GENERIC_NT" in env:
        kw.update(generic_nt_set=True, generic_nt=int(env["UPR_QP_GENERIC_NT"]))
    assert not set(env) - {"UPR_QP_KERNEL", "UPR_QP_GENERIC", "UPR_QP3_JIT", "UPR_QP_NT", "UPR_QP_GENERIC_NT"}, env
    return _knobs(**kw)


_BUILT = {}


def _problem_key(name):
    builder, kw = F.CASES[name][:2]
    return (builder.__name__, json.dumps(kw, sort_keys=True))


def _case(name, converged=False):
    """The case's inputs, built once per distinct (builder, kwargs): the lane sweeps share theirs"""
    key = (_problem_key(name), converged, F.CONVERGED[name][1] if converged else None)
    if key not in _BUILT:
        _BUILT[key] = F.converged_case(name) if converged else F.build_case(name, qp_tol=0.0, qp_iter_max=F.ITERS)
    return _BUILT[key]


@pytest.mark.parametrize("name", list(F.CASES))
def test_case_resolves_to_the_kernel_the_table_states(name):
    _, _, env, structure, kernel = F.CASES[name]
    E = C.CDLL(str(EMU))
    P = _case(name)["P"]
    r = _select(E, P, knobs_of(env))
    assert (r["structure"], r["name"]) == (structure, kernel), (name, r)
    assert structure in (GENERIC, SECOND) and not r["exported"] and not r["fb_fused"], r
    d = _select(E, P, _knobs())
    if name.startswith("fallback_"):
        # an empty environment (the run-time instantiation switched off where the case says so) leaves the production structure
        assert "UPR_QP_KERNEL" not in env and "UPR_QP_GENERIC" not in env, env
        if "UPR_QP3_JIT" in env:
            assert (d["structure"], d["source"]) == (PRODUCTION, RUN_TIME), d    # ... which would have taken it
        else:
            assert d["structure"] == structure and d["name"] == kernel, d
    if name in F.CONVERGED:
        assert (name in F.ALSO_PRODUCTION) == (d["structure"] == PRODUCTION and d["source"] != RUN_TIME), (name, d)
    # the lane count of the generic kernel where no knob sets it: the rule's thresholds, written out
    if structure == GENERIC and "UPR_QP_GENERIC_NT" not in env:
        nx, ne = 3 * P.nq, 6 * P.nb
        big = max(ne * nx, nx * nx)
        assert r["nt"] == (512 if big >= 1024 else 256 if big >= 512 else 64) and kernel == F.gen(r["nt"]), (name, r, big)


def _listed_qp2_shapes():
    text = (CSRC / "upr_qp_select.h").read_text()
    lines = [l for l in text.splitlines() if l.startswith("#define UPR_QP2_SHAPES(X)")]
    assert len(lines) == 2 and "UPR_HEADLINE_ONLY" in text, lines      # (the first: experiment builds of the headline kernel)
    return [tuple(int(v) for v in t.split(",")) for t in re.findall(r"X\(([^)]*)\)", lines[1].split("(X)", 1)[1])]


def _launcher_lanes(launcher):
    """The lane counts of a launcher's switch in upr_api_qp_old.hip: {label: instantiated NT}"""
    text = (CSRC / "upr_api_qp_old.hip").read_text()
    body = text.split(launcher, 1)[1].split("default:", 1)[0]
    out, pending = {}, []
    for label, inst in re.findall(r"case (\d+):(?:\s*return \w+<(?:D, )?(\d+)>;)?", body):
        pending.append(int(label))
        if inst:
            out.update({l: int(inst) for l in pending}); pending = []
    assert out and not pending, (out, pending)
    return out


def test_table_is_complete():
    """Every entry of UPR_QP2_SHAPES at every lane count its launcher accepts, every lane count of the generic launcher on both sweep
    shapes, the aliases under the name of the form that runs, and the cases the screen was specified with: a shape added to the list,
    a lane count added to a launcher or a case deleted from the table fails here before any GPU time."""
    assert set(F.CASES) == set(REQUIRED) and len(REQUIRED) == len(set(REQUIRED)), (set(F.CASES) ^ set(REQUIRED))
    shapes = _listed_qp2_shapes()
    assert shapes == F.QP2_SHAPES and set(F.QP2_BUILDERS) == set(shapes), shapes
    E = C.CDLL(str(EMU))
    E.emu_qp2.restype = C.c_long
    lanes2 = _launcher_lanes("upr_qp_launcher qp2_launcher(int nt) {")
    assert lanes2 == {64: 64, 128: 128, 256: 256, 512: 128}, lanes2
    assert sorted(nt for nt, inst in lanes2.items() if nt == inst) == F.QP2_LANES
    by_kernel = {}
    for name, (_, _, env, structure, kernel) in F.CASES.items():
        by_kernel.setdefault((structure, kernel), []).append(name)
    for shape in shapes:
        for nt, inst in lanes2.items():
            if nt == inst:
                assert any(F.CASES[n][2].get("UPR_QP_NT") == str(nt) for n in by_kernel.get((SECOND, F.qp2(shape, nt)), [])), (shape, nt)
        P = _case("qp2_%s_nt128" % "x".join(map(str, shape)))["P"]
        assert (P.nq, P.nb, P.nc, P.nf) == shape and not P.n_state_rows and not P.slacks, shape
        assert E.emu_qp2(C.byref(Emu(P, 1).cp), 1, None, None, None, None, None, None, C.c_long(0), None) > 0, shape    # (the emulation's own list)
    aliases = {nt: inst for nt, inst in lanes2.items() if nt != inst}
    for nt, inst in aliases.items():      # an alias runs on one shape at least, under the name of the form it stands for
        assert any(env.get("UPR_QP_NT") == str(nt) and kernel.endswith(", %d>" % inst) for _, _, env, s, kernel in F.CASES.values() if s == SECOND), nt
    lanes1 = _launcher_lanes("upr_qp_launcher qp_generic_launcher(int nt) {")
    assert lanes1 == {nt: nt for nt in F.GENERIC_LANES}, lanes1
    for nt in lanes1:
        swept = [n for n in by_kernel.get((GENERIC, F.gen(nt)), []) if F.CASES[n][2].get("UPR_QP_GENERIC_NT") == str(nt)]
        assert sorted(n.rsplit("_nt", 1)[0] for n in swept) == ["generic_dice", "generic_rows_soft"], (nt, swept)
    # the two sweep shapes use every block of upr_qp_lds_layout between them: rows (ob, hob) with slacks (sgk, tak, gak) on one
    # body, the ne x ne blocks of two coupled bodies
    rows_soft, dice = _case("generic_rows_soft_nt64")["P"], _case("generic_dice_nt64")["P"]
    assert rows_soft.n_state_rows > 0 and rows_soft.slacks["poly_ineq"] and dice.nb == 2 and any(b >= 0 for b in dice.contact_body1)
    # the rule's three lane counts are all among the cases no knob sets the count of
    assert {F.CASES[n][4] for n in REQUIRED[:10]} == {F.gen(64), F.gen(256), F.gen(512)}
    # every refusal message is the launcher's own
    text = (CSRC / "upr_api_qp_old.hip").read_text()
    assert all('upr_fail("%s")' % m in text for _, _, _, m in F.REFUSED.values())
    # the converged leg: one case per distinct (structure, shape, horizon class) of the table
    distinct = {}
    for name, (builder, kw, env, structure, kernel) in F.CASES.items():
        distinct.setdefault((structure, _problem_key(name)), name)
    assert {(F.CASES[n][3], _problem_key(n)) for n in F.CONVERGED} == set(distinct), set(distinct) ^ {(F.CASES[n][3], _problem_key(n)) for n in F.CONVERGED}
    # exceptions to 1e-8 stay below 1e-6 and name cases of the table; the residuals' exceptions have one recorded cause, which only one
    # body on frictionless contacts has
    assert set(F.TOL) <= set(F.CASES) and set(F.RES_TOL) <= set(F.CASES) and all(v <= 1e-6 for v in F.TOL.values())
    assert all((_case(n)["P"].nb, _case(n)["P"].nf) == (1, 1) for n in F.RES_TOL)


def test_every_reason_to_leave_the_production_structure_has_a_case(arrangements):
    """upr_qp_plan / upr_qp3_jit_capable, default knobs: each reason on a problem that the production structure takes until the reason
    applies.  Four of them are device cases of the table; the others resolve on the host only (the module docstring says why for the
    hard frictionless equality; the remaining N > 64 classes differ from fallback_N65 in the branch of one condition)."""
    E = C.CDLL(str(EMU))
    sel = lambda P, **kw: _select(E, P, _knobs(**kw))

    def robust(**kw):
        P = thing_problem(arrangements["robust_8corner"], nf=1, force_weight=0.0, **kw)
        P.slacks = dict(state_box=True, input_box=False, poly_ineq=True)
        return P

    def with_rows(P):
        from upright_amd import robots
        for k, v in robots.collision_model(P.chain, robots.SIMPLE_COLLISION_PAIRS).items():
            setattr(P, k, v)
        return P

    # N > 64: one body (the device case), friction on a star of several bodies, shared contacts, rows; N > 128 for the one class N > 64 is for
    assert sel(_case("fallback_N65")["P"])["structure"] == SECOND
    assert sel(thing_problem(arrangements["pink_bottle"], N=64))["structure"] == PRODUCTION
    assert sel(thing_problem(arrangements["blue_cups"], N=64))["structure"] == PRODUCTION and sel(thing_problem(arrangements["blue_cups"], N=65))["structure"] == GENERIC
    assert sel(thing_problem(arrangements["foam_die2"], N=64))["structure"] == PRODUCTION and sel(thing_problem(arrangements["foam_die2"], N=65))["structure"] == SECOND
    assert sel(robust(N=65))["structure"] == PRODUCTION and sel(with_rows(robust(N=65)))["structure"] == GENERIC
    assert sel(robust(N=128))["structure"] == PRODUCTION and sel(robust(N=129))["structure"] == GENERIC
    # ... with slacks the one-body problem is not plain: the generic kernel (the device case fallback_N65_soft)
    assert sel(_case("fallback_N65_soft")["P"])["structure"] == GENERIC
    # more than UPR_QP3_NOMAX = 20 state rows per knot: the device case, and the same problem without its end-effector box
    P = _case("fallback_26_rows")["P"]
    assert P.n_state_rows == 26 and sel(P)["structure"] == GENERIC
    assert sel(_case("generic_box_arch")["P"])["structure"] == PRODUCTION
    # a hard equality on frictionless contacts of several bodies (nfc 32 < ne 48, no soft_eq): host-only
    P = robust(); P.slacks = None
    assert sel(robust())["structure"] == PRODUCTION and sel(P)["structure"] == GENERIC and sel(P)["name"] == F.gen(512)
    # run-time instantiation switched off (or failed: run_time_ok = false takes the same branch): the device case
    P = _case("fallback_no_jit_N12")["P"]
    assert (sel(P)["structure"], sel(P)["source"]) == (PRODUCTION, RUN_TIME) and sel(P, qp3_jit=0)["structure"] == SECOND
    P = _case("fallback_N65_soft")["P"]
    assert sel(P, qp3_jit=0)["structure"] == GENERIC


def _distinct(names):
    seen, out = set(), []
    for n in names:
        k = (F.CASES[n][3], _problem_key(n))
        if k not in seen:
            seen.add(k); out.append(n)
    return out


@pytest.mark.parametrize("name", _distinct(F.CASES))
def test_emulated_case_runs_its_fixed_iterations(name):
    """The emulated kernel of the case (the lane sweeps share a problem: the emulation has one lane) on the emulation's own records, the
    workspace poisoned: finite steps, ITERS iterations on every instance, no factorisation failure."""
    structure = F.CASES[name][3]
    c = _case(name)
    P, B = c["P"], c["B"]
    lin = Emu(P, B, bp=c["bp"]).linearize(c["way"], np.zeros(B), c["xs0"], c["us0"])
    dx, du, st, _ = F.emulate(structure, P, B, c["xs0"], c["us0"], c["x0"], lin, c["bp"])
    assert np.all(np.isfinite(dx)) and np.all(np.isfinite(du)) and np.abs(dx).max() > 1e-2
    assert np.all(st[:, 1] == F.ITERS) and np.all(st[:, 2] == 1), (st[:, 1], st[:, 2])
    assert np.all(np.isfinite(st[:, 6:10]))


def emulated_point(E, P, B, r, ws):
    """The primal-dual point the emulated kernel left in the instance workspace, read at the offsets of the selection record r, in
    the layout of BatchMPC.qp_kkt() (slots that are no rows of a knot zeroed, as upr_batch_qp_kkt hands them out)"""
    ko = (C.c_int * 8)()
    E.emu_kkt_offsets(C.byref(Emu(P, 1).cp), ko)
    ni, neN = ko[4], ko[5]
    nx, nu, ne, n1, N = P.nx, P.nu, 6 * P.nb, P.N + 1, P.N
    npoly = 5 * P.nc if P.nf == 3 else 0
    lam = ws[:, r["o_lam"]:r["o_lam"] + n1 * ni].reshape(B, n1, ni).copy()
    lam[:, 0, :2 * nx] = 0.0; lam[:, N, 2 * nx:] = 0.0; lam[:, 0, 2 * nx + 2 * nu + npoly:] = 0.0
    return dict(pi=ws[:, r["o_pi"]:r["o_pi"] + n1 * nx].reshape(B, n1, nx), nu=ws[:, r["o_nu"]:r["o_nu"] + N * ne].reshape(B, N, ne),
                yN=ws[:, r["o_yN"]:r["o_yN"] + neN], lam=lam)


@pytest.mark.parametrize("name", list(F.CONVERGED))
def test_emulated_converged_point_is_a_kkt_point(name):
    """The converged leg on the host: the inputs of every converged case converge in the emulated kernel (all instances; two of four
    for generic_rows), the point read at the selection record's offsets passes tests/kkt_check.py at 1e-7, and the step is the
    emulated production kernel's at 2e-5 wherever the device test compares the two."""
    _, _, env, structure, kernel = F.CASES[name]
    E = C.CDLL(str(EMU))
    c = _case(name, converged=True)
    P, B = c["P"], c["B"]
    e = Emu(P, B, bp=c["bp"])
    lin = e.linearize(c["way"], np.zeros(B), c["xs0"], c["us0"])
    dx, du, st, ws = F.emulate(structure, P, B, c["xs0"], c["us0"], c["x0"], lin, c["bp"])
    which = np.flatnonzero(st[:, 2] == 0)
    assert len(which) == (2 if name == "generic_rows" else B), (st[:, 1], st[:, 2])
    r = _select(E, P, knobs_of(env))
    sol = dict(dx=dx, du=du, **emulated_point(E, P, B, r, ws))
    if F.CONVERGED[name][0]:
        res = F.kkt_of(c, sol, lin, which)
        print("emulated converged %s: KKT %s" % (name, res))
        assert res.max() < 1e-7, res
    if name in F.ALSO_PRODUCTION:
        dx3, du3, st3, _ = e.qp(3, c["xs0"], c["us0"], c["x0"], lin)
        assert np.array_equal(np.flatnonzero(st3[:, 2] == 0), which)
        ex, eu = F.step_difference(P, sol, dict(dx=dx3, du=du3), which)
        assert ex < 2e-5 and eu < 2e-5, (ex, eu)
