"""The friction margin per contact group on the MI355X (upr_batch_friction_margin_groups_points / _plan, upright_amd/csrc/upr_margin.h)
and the balance check with a friction scale per contact (upr_batch_balance_points_cmu / _plan_cmu): the assertions of
tests/test_group_margin.py on the same table (tests/group_margin_ref.py) with the device's answers, the device against the host
emulation of the same source, the plan form against the points form, the knot reduction, the refusals and the absence of side
effects on the handle."""
import numpy as np
import pytest

import balance_ref as R
import group_margin_ref as G
import margin_ref as M
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, waypoints_for

pytestmark = pytest.mark.gpu

_DEVICE = {}
KEYS = ("kappa_hi", "kappa_lo", "z", "y", "iters")
ALL = dict(want_lo=True, want_z=True, want_y=True, want_iters=True)


def _margin(h, L, **kw):
    return dict(zip(KEYS, h.friction_margin(L["x"], L["params"], groups=[list(g) for g in L["groups"]], mu_base=L["mu_base"], **ALL, **kw)))


def _device(arrangements, name):
    """The launches of the table (reference classes and emulation: G.cases) run once on the device: key "dev"."""
    if name not in _DEVICE:
        launches = G.cases(arrangements, name)
        h = BatchMPC(launches[0]["P"], 1)
        for L in launches:
            L["dev"] = _margin(h, L)
        assert h.balance_ms() > 0.0
        h.close()
        _DEVICE[name] = launches
    return _DEVICE[name]


def _rho_fns(h):
    rho_c = lambda x, prm, pp, v: h.balance_check(x, prm, want_iters=True, mu_scale=v)       # noqa: E731  ((n_scen, nc): the _cmu entry)
    rho_mu = lambda x, prm, pp, mu: h.balance_check(x, prm, want_iters=True, mu_scale=mu)    # noqa: E731
    rho_plain = lambda x, prm, pp: h.balance_check(x, prm, want_iters=True)                  # noqa: E731
    return rho_c, rho_mu, rho_plain


@pytest.mark.parametrize("name,form", [(n, "") for n in G.NAMES] + [(n, "0") for n in G.ONE_BODY + ["pink_bottle_nf1"]])
def test_one_group_of_all_contacts_is_the_common_margin(arrangements, name, form, monkeypatch):
    """Assertion 1: one group of every contact, mu_base NULL -- kappa_hi, kappa_lo, z, y and iters are the bits of friction_margin on
    the same jobs (labels and index lists alike); with UPR_BAL_FORM=0 the one-body arrangements run both on the wave form."""
    launches = G.cases(arrangements, name)
    P = launches[0]["P"]
    if form:
        monkeypatch.setenv("UPR_BAL_FORM", form)
    h = BatchMPC(P, 1)
    assert np.array_equal(h.contact_groups(), G.pair_labels(P))
    for L in launches[:2]:
        com = h.friction_margin(L["x"], L["params"], **ALL)
        one = h.friction_margin(L["x"], L["params"], groups=np.zeros(P.nc, dtype=int), **ALL)
        two = h.friction_margin(L["x"], L["params"], groups=[list(range(P.nc))], **ALL)
        assert all(np.array_equal(a[:, :, 0], c) and np.array_equal(b[:, :, 0], c) for a, b, c in zip(one, two, com)), name
    h.close()


@pytest.mark.parametrize("name", G.NAMES)
def test_rho_with_a_scale_per_contact(arrangements, name):
    """Assertion 2 on the device, first launch of the arrangement: uniform rows give the bits of the per-scenario call, all ones those
    of the call without a scale, random scales from {0.5, 1, 2} per contact keep |rho - rho_ref| <= 1e-9 max(1, |b|)."""
    L = G.cases(arrangements, name)[0]
    h = BatchMPC(L["P"], 1)
    G.check_rho_per_contact(L, *_rho_fns(h), "device", name)
    h.close()


@pytest.mark.parametrize("name", G.NAMES)
def test_bracket_certificates_class_and_closure(arrangements, name):
    """Assertions 3, 4 and 5 on every (job, group) of the table on the device's kappa_hi, kappa_lo, z, y, iters: the bracket exactly,
    both certificates on the oracle's b and A at the group's scale vector, rho_ref at both ends, the reference's class; and closure:
    the device's rho call at "kappa_hi on the group, beta elsewhere" is inside the ball, at kappa_lo outside, compared exactly."""
    launches = _device(arrangements, name)
    h = BatchMPC(launches[0]["P"], 1)
    for k, L in enumerate(launches):
        bad = G.check_group_answer(L, L["dev"])
        assert not bad, (name, k, bad[:5])
        G.check_closure(L, L["dev"], _rho_fns(h)[0])
    h.close()


@pytest.mark.parametrize("name", G.ONE_BODY)
def test_one_body_arrangements_on_the_wave_form(arrangements, name, monkeypatch):
    """UPR_BAL_FORM=0 sends the one-body arrangements through the wave-per-job group kernel: the same assertions on the same jobs,
    the class and (away from the boundary) the iteration counts of the emulated wave form."""
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    launches = G.cases(arrangements, name)[:3]
    ng = len(launches[0]["groups"])
    masks = [M.near_masks(G.group_views(G.cases(arrangements, name), g)) for g in range(ng)]
    h = BatchMPC(launches[0]["P"], 1)
    for k, L in enumerate(launches):
        out = _margin(h, L)
        bad = G.check_group_answer(L, out)
        assert not bad, (name, k, bad[:5])
        emu = G.run_emu(L["P"], L["x"], L["params"], L["per_point"], L["groups"], L["mu_base"], form=0)
        assert np.array_equal(M.device_class(out["kappa_hi"]), M.device_class(emu["kappa_hi"]))
        for g in range(ng):
            far = ~masks[g][k]
            assert np.array_equal(out["iters"][:, :, g][far], emu["iters"][:, :, g][far])
    h.close()


@pytest.mark.parametrize("name", G.FRICTION)
def test_full_bisections_and_order(arrangements, name):
    """Assertions 6 and 7 on the device: |kappa - kappa_ref| <= 1e-6 against full CPU bisections on at most 64 finite (job, group)
    pairs (the largest value, and the one against the emulation, are printed for DESIGN 3.9), and the order against the device's
    common margin on every job without a base table."""
    launches = _device(arrangements, name)
    ng = len(launches[0]["groups"])
    w_ref, w_emu, count = 0.0, 0.0, 0
    for g in range(ng):
        for k, i, s, kref, _ in M.reference_bisections(G.group_views(launches, g), limit=64 // ng):
            w_ref = max(w_ref, abs(launches[k]["dev"]["kappa_hi"][i, s, g] - kref))
            count += 1
    for L in launches:
        d, e = L["dev"]["kappa_hi"], L["emu"]["kappa_hi"]
        fin = np.isfinite(d) & np.isfinite(e)
        w_emu = max(w_emu, float(np.abs(d[fin] - e[fin]).max()) if fin.any() else 0.0)
    print("group margin, %s: %d finite pairs, largest |kappa - kappa_ref| device vs reference %.2e, device vs emulation %.2e" % (name, count, w_ref, w_emu))
    assert w_ref <= 1e-6, (name, w_ref)
    h = BatchMPC(launches[0]["P"], 1)
    for L in launches:
        if L["mu_base"] is None:
            com = h.friction_margin(L["x"], L["params"])
            assert not len(G.check_order(com, L["dev"]["kappa_hi"])), name
    h.close()


@pytest.mark.parametrize("name", G.NAMES)
def test_device_against_the_emulation(arrangements, name):
    """Assertion 8.  The same source on the device and on the host: the same class on every (job, group), and the same iteration
    count on every pair whose decisions all keep 1e-9 max(|b|, 1) away from the boundary on the reference (M.near_masks per group;
    the pairs left out are at most half of a launch)."""
    launches = _device(arrangements, name)
    ng = len(launches[0]["groups"])
    masks = [M.near_masks(G.group_views(launches, g)) for g in range(ng)]
    for k, L in enumerate(launches):
        d, e = L["dev"], L["emu"]
        assert np.array_equal(M.device_class(d["kappa_hi"]), M.device_class(e["kappa_hi"]))
        near = np.stack([masks[g][k] for g in range(ng)], axis=2)
        assert near.sum() <= 0.5 * near.size or near.size <= ng, (name, k, int(near.sum()), near.size)
        assert np.array_equal(d["iters"][~near], e["iters"][~near]), (name, k, np.argwhere((d["iters"] != e["iters"]) & ~near)[:5])


def _headline(arrangements, B, seed=3, **settings):
    P = thing_problem(arrangements["pink_bottle"], **settings)
    x0 = level_tray_states(B, seed=seed)
    rng = np.random.default_rng(seed)
    bp = np.stack([R.scale_mass(P.body_params, rng.uniform(0.9, 1.1)) for _ in range(B)])   # every instance its own mass
    return BatchMPC(P, B, body_params=bp, way_p=waypoints_for(P, x0)), x0, bp


GROUPS3 = [[0, 1], [2, 3], [0, 1, 2, 3]]


@pytest.mark.parametrize("form", ["", "0"])
def test_plan_form(arrangements, form, monkeypatch):
    """Assertion 9 and the reduction of assertion 1.  Headline handle, B = 3, N = 20, one cold solve, 4 scenarios: 252 jobs times
    three groups (two halves of the contacts and all of them), on the lane form and with UPR_BAL_FORM=0 on the wave form.  The plan
    call equals the points form on the downloaded plan, == on kappa_hi, kappa_lo and iters, with shared scenarios, scenarios per
    instance, params=None and a base table; the group of all contacts is friction_margin_plan; worst is the maximum over the knots
    of the plan call with the first knot that attains it, alone or beside kappa_hi; the rho plan call with a scale per contact
    equals its points form."""
    if form:
        monkeypatch.setenv("UPR_BAL_FORM", form)
    B = 3
    mpc, x0, bp = _headline(arrangements, B)
    P = mpc.problem
    N = P.N
    assert N == 20
    mpc.set_observation(0.0, x0)
    mpc.advance()
    _, xs, _ = mpc.solution()
    pts = xs.reshape(B * (N + 1), P.nx)
    scen = R.scenarios(P)
    kw = dict(want_lo=True, want_iters=True, groups=GROUPS3)
    got = mpc.friction_margin_plan(scen, **kw)
    assert mpc.balance_ms() > 0.0
    want = mpc.friction_margin(pts, scen, **kw)
    assert got[0].shape == (B, N + 1, 4, 3) and got[0][..., 0].size == 252
    assert all(np.array_equal(g.reshape(-1, 4, 3), w) for g, w in zip(got, want))
    assert not np.any(np.isnan(got[0])) and np.any(np.isfinite(got[0]) & (got[0] > 0))
    com = mpc.friction_margin_plan(scen, want_lo=True, want_iters=True)
    assert all(np.array_equal(g[..., 2], c) for g, c in zip(got, com))
    w, kn = mpc.friction_margin_plan(scen, groups=GROUPS3, worst=True)
    assert w.shape == (B, 4, 3) and np.array_equal(w, got[0].max(axis=1)) and np.array_equal(kn, got[0].argmax(axis=1))
    assert np.array_equal(w[..., 2], com[0].max(axis=1)) and np.array_equal(kn[..., 2], com[0].argmax(axis=1))
    beta = np.array([0.5, 1.0, 2.0, 0.0])[:, None] * np.ones((4, P.nc))
    got = mpc.friction_margin_plan(scen, mu_base=beta, **kw)
    want = mpc.friction_margin(pts, scen, mu_base=beta, **kw)
    assert all(np.array_equal(g.reshape(-1, 4, 3), w) for g, w in zip(got, want))
    per = np.stack([R.scenarios(P, np.random.default_rng(b), 4) for b in range(B)])
    got = mpc.friction_margin_plan(per, **kw)
    want = mpc.friction_margin(pts, np.repeat(per[:, None], N + 1, axis=1).reshape(B * (N + 1), 4, P.nb, 10), **kw)
    assert all(np.array_equal(g.reshape(-1, 4, 3), w) for g, w in zip(got, want))
    got = mpc.friction_margin_plan(**kw)
    own = np.repeat(bp[:, None, None], N + 1, axis=1).reshape(B * (N + 1), 1, P.nb, 10)
    want = mpc.friction_margin(pts, own, **kw)
    assert got[0].shape == (B, N + 1, 1, 3) and all(np.array_equal(g.reshape(-1, 1, 3), w) for g, w in zip(got, want))
    v = np.random.default_rng(5).choice([0.5, 1.0, 2.0], size=(4, P.nc))
    assert np.array_equal(mpc.balance_check_plan(scen, mu_scale=v).reshape(-1, 4), mpc.balance_check(pts, scen, mu_scale=v))
    assert np.array_equal(mpc.balance_check_plan(scen, mu_scale=np.ones((4, P.nc))), mpc.balance_check_plan(scen))
    mpc.close()


def test_refusals(arrangements):
    """Assertion 11: every refusal of the new entries raises with its message, and leaves the handle usable."""
    P = R.table_problem(arrangements, "fixture_box")
    h = BatchMPC(P, 1)
    x = R.points(P, ["lift", "inside"], seed=1)
    scen = R.scenarios(P)
    fm = lambda **kw: h.friction_margin(x, scen, **kw)   # noqa: E731
    with pytest.raises(RuntimeError, match="n_grp"):
        fm(groups=[])
    with pytest.raises(RuntimeError, match="empty mask"):
        fm(groups=[[0, 1], []])
    with pytest.raises(RuntimeError, match="empty mask"):
        fm(groups=np.array([0, 0, 0, 0, 2, 2, 2, 2]))
    with pytest.raises(RuntimeError, match="mask bit >= nc"):
        fm(groups=[[0, 8]])
    with pytest.raises(RuntimeError, match="mu_base"):
        fm(groups=[[0, 1]], mu_base=-1.0)
    with pytest.raises(RuntimeError, match="mu_base"):
        fm(groups=[[0, 1]], mu_base=np.inf)
    with pytest.raises(RuntimeError, match="kappa_max"):
        fm(groups=[[0, 1]], kappa_max=0.0)
    with pytest.raises(RuntimeError, match="kappa_max"):
        fm(groups=[[0, 1]], kappa_max=np.inf)
    bad = np.ones((4, P.nc))
    bad[2, 3] = -0.5
    with pytest.raises(RuntimeError, match="mu_scale"):
        h.balance_check(x, scen, mu_scale=bad)
    bad[2, 3] = np.nan
    with pytest.raises(RuntimeError, match="mu_scale"):
        h.balance_check_plan(scen, mu_scale=bad)
    import ctypes as C

    from upright_amd._capi import check, ptr
    masks = np.array([3], dtype=np.uint32)
    with pytest.raises(RuntimeError, match="kappa_hi and worst must not both be NULL"):
        check(h._lib.upr_batch_friction_margin_groups_plan(h._h, 4, ptr(scen), 0, 1, masks.ctypes.data_as(C.POINTER(C.c_uint)), None, 8.0, None, None,
                                                           None, None, None))
    assert fm(groups=[[0, 1, 2, 3], [4, 5, 6, 7]]).shape == (2, 4, 2)
    h.close()


def test_calls_leave_the_handle_as_it_was(arrangements):
    """Assertion 10.  Twin handles (headline, B = 3, feedback policy and tracked value function on), the same calls on both, the group
    margin in both forms, the reduction and the rho calls with a scale per contact on one of them only, between the other calls:
    solution(), stats(), the next advance() and the ticks (the later ones replayed from the captured graph) are bitwise equal."""
    B = 3
    (A, x0, bp), (T, _, _) = _headline(arrangements, B, use_feedback_policy=True), _headline(arrangements, B, use_feedback_policy=True)
    scen = R.scenarios(A.problem)
    v = np.full((4, A.problem.nc), 0.5)
    probe = lambda: (A.friction_margin(x0, scen, groups=GROUPS3, mu_base=v, **ALL), A.friction_margin_plan(groups=GROUPS3),   # noqa: E731
                     A.friction_margin_plan(scen, groups=GROUPS3, worst=True), A.balance_check_plan(scen, mu_scale=v),
                     A.balance_check(x0, scen, mu_scale=v))
    for h in (A, T):
        h.track_value_function()
        h.set_observation(0.0, x0)
    probe()
    for h in (A, T):
        h.advance()
    probe()
    for k, (u, w) in enumerate(zip(A.solution(), T.solution())):
        assert np.array_equal(u, w), k
    sa, st = A.stats(), T.stats()
    assert all(np.array_equal(sa[k], st[k]) for k in sa)
    Va, Vt = A.value_function(0.05, x0), T.value_function(0.05, x0)
    assert np.array_equal(Va[0], Vt[0]) and np.array_equal(Va[1], Vt[1])
    for h in (A, T):
        h.set_observation(0.1, x0)
        h.advance()
    for u, w in zip(A.solution(), T.solution()):
        assert np.array_equal(u, w)
    x = x0.copy()
    for k in range(5):
        xa, ua = A.tick(0.2 + 0.01 * k, x)
        xt, ut = T.tick(0.2 + 0.01 * k, x)
        assert np.array_equal(xa, xt) and np.array_equal(ua, ut), k
        if k >= 2:
            probe()
        x = xa
    assert A.tick_graph_replays() == T.tick_graph_replays() >= 1
    A.close(); T.close()
