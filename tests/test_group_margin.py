"""The friction margin per contact group (upright_amd/csrc/upr_margin.h, upr_grp_args) through its host emulation
(tests/emu/upr_group_margin_emu.cpp: the same source, one thread per wave), against tests/group_margin_ref.py: the classes of the
table on the reference alone, one group of all contacts against the common margin bit for bit, rho with a scale per contact, the
bracket and both certificates, closure on the rho call, the order against the common margin, full CPU bisections, the knot
reduction, and the resources of the kernels.  tests/test_gpu_group_margin.py makes the same assertions on the device's answers."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import balance_ref as R
import group_margin_ref as G
import margin_ref as M

ROOT = Path(__file__).resolve().parents[1]


def test_entries_and_documents():
    """The header declares the four entries and cites the reference tool; _capi binds them; BatchMPC documents groups; DESIGN has
    section 3.9 and no longer calls separate scales out of scope."""
    from upright_amd import _capi
    from upright_amd.engine import BatchMPC

    hdr = (ROOT / "include" / "upright_mi.h").read_text()
    names = {"upr_batch_balance_points_cmu", "upr_batch_balance_plan_cmu", "upr_batch_friction_margin_groups_points", "upr_batch_friction_margin_groups_plan"}
    assert all(re.search(r"\b%s\(" % n, hdr) for n in names) and names <= {p[0] for p in _capi.PROTOTYPES}
    assert "compute_minimum_mu.py:12-30" in hdr
    assert "groups" in BatchMPC.friction_margin.__doc__ and "worst" in BatchMPC.friction_margin_plan.__doc__
    design = (ROOT / "DESIGN.md").read_text()
    assert "### 3.9" in design and "`compute_minimum_mu.py`) are out of scope" not in design
    assert "contact_groups" in (ROOT / "README.md").read_text()


def test_pair_labels_are_the_reference_tools(arrangements):
    """contact_groups(): labels by (contact_body1, contact_body2) in first-occurrence order -- foam_die2 two pairs of four contacts,
    box_arch four pairs, one-body arrangements one."""
    from upright_amd.engine import BatchMPC

    for name, want in (("foam_die2", [0] * 4 + [1] * 4), ("box_arch", [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4), ("fixture_box", [0] * 8)):
        P = R.table_problem(arrangements, name)
        assert list(G.pair_labels(P)) == want
        fake = type("H", (), {"problem": P})()
        assert list(BatchMPC.contact_groups(fake)) == want
        assert list(BatchMPC._group_masks(fake, np.array(want))) == list(G.masks_of(G.by_pair(P)))
        assert list(BatchMPC._group_masks(fake, [[0, 1], [1, 5]])) == [3, 34]


@pytest.mark.parametrize("name", G.NAMES)
def test_classes_of_the_table(arrangements, name):
    """Counted on the reference alone.  lift states need no friction (zero for every group), down states are lost whatever the
    friction (inf for every group; the fixture box holds none, margin_ref.N_DOWN), inside states need friction from some group:
    every friction arrangement holds >= 5 (job, group) pairs of each class it can hold.  On the fixture box the walls are never
    needed (all zero) and the bottom group has the finite pairs.  Without friction (nf = 1): zero or inf, equal across groups."""
    launches = G.cases(arrangements, name)
    cnt = G.class_counts(launches)
    print("group margin, classes of %s per group: %s" % (name, cnt))
    tot = {k: sum(c[k] for c in cnt) for k in ("zero", "finite", "inf", "below")}
    jobs = sum(L["views"][0]["mclass"].size for L in launches)
    sizes = {L["views"][0]["mclass"].size for L in launches}
    if name == "blue_cups":
        assert sizes == {37}
    else:
        assert {1, 37} <= sizes and any(200 <= n <= 260 for n in sizes) and {L["per_point"] for L in launches} == {True, False}
    if name in G.NF1:
        assert tot["finite"] == 0 and tot["zero"] >= 5 and tot["inf"] >= 5
        for L in launches:
            assert all(np.array_equal(V["mclass"], L["views"][0]["mclass"]) for V in L["views"])
    elif name == "fixture_box":
        assert cnt[0]["below"] >= 5 and cnt[0]["zero"] >= 5 and cnt[1] == dict(zero=jobs, finite=0, inf=0, below=0)
    elif name == "bottle_20_contacts":
        # (half of the points of one contact patch: the other half carries the friction of most states -- the finite pairs are the
        #  ones of the outer rings, contacts 0 - 9, some of them above one)
        assert tot["zero"] >= 5 and tot["finite"] >= 5 and tot["inf"] >= 5
    else:
        assert tot["zero"] >= 5 and tot["below"] >= 5 and tot["inf"] >= 5


@pytest.mark.parametrize("name", G.NAMES)
def test_one_group_of_all_contacts_is_the_common_margin(arrangements, name):
    """Assertion 1 under emulation: kappa_hi, kappa_lo, z, y, iters of one group holding every contact, without a base table, are
    the bits of the common margin's job; in both forms on the one-body arrangements."""
    for L in G.cases(arrangements, name)[:2]:
        P = L["P"]
        for form in ((-1, 0) if P.nb == 1 else (-1,)):
            one = G.run_emu(P, L["x"], L["params"], L["per_point"], [np.arange(P.nc)], form=form)
            com = M.run_emu(P, L["x"], L["params"], L["per_point"], form=form)
            assert all(np.array_equal(one[k][:, :, 0], com[k]) for k in com), (name, form)


def test_knot_reduction():
    """upr_bal_margin_worst: the largest value over the knots, inf the largest of all, and the FIRST knot that attains it."""
    rng = np.random.default_rng(3)
    k = rng.choice([0.0, 0.25, 0.5, 1.5, np.inf], size=(5, 21, 4, 3))
    k[0, :, 0, 0] = 0.0
    k[1, 7, 1, 1] = k[1, 13, 1, 1] = np.inf
    w, kn = G.emu_worst(k)
    assert np.array_equal(w, k.max(axis=1)) and np.array_equal(kn, k.argmax(axis=1))
    assert kn[0, 0, 0] == 0 and kn[1, 1, 1] <= 7 and np.isinf(w[1, 1, 1])


def _emu_rho_fns(P, form=-1):
    rho_c = lambda x, prm, pp, v: G.run_emu_rho(P, x, prm, pp, v, form=form)          # noqa: E731
    rho_mu = lambda x, prm, pp, mu: M.run_emu_rho(P, x, prm, pp, mu, form=form)       # noqa: E731
    rho_plain = lambda x, prm, pp: M.run_emu_rho(P, x, prm, pp, None, form=form)      # noqa: E731
    return rho_c, rho_mu, rho_plain


@pytest.mark.parametrize("name", G.NAMES)
def test_rho_with_a_scale_per_contact(arrangements, name):
    """Assertion 2 under emulation, first launch of the arrangement (both forms on the one-body arrangements)."""
    L = G.cases(arrangements, name)[0]
    for form in ((-1, 0) if L["P"].nb == 1 else (-1,)):
        G.check_rho_per_contact(L, *_emu_rho_fns(L["P"], form), "emulation form %d" % form, name)


@pytest.mark.parametrize("name", G.NAMES)
def test_bracket_certificates_class_and_closure(arrangements, name):
    """Assertions 3, 4 and 5 on every (job, group) of the table, on the emulation's answer."""
    for k, L in enumerate(G.cases(arrangements, name)):
        bad = G.check_group_answer(L, L["emu"])
        assert not bad, (name, k, bad[:5])
        G.check_closure(L, L["emu"], _emu_rho_fns(L["P"])[0])


@pytest.mark.parametrize("name", G.ONE_BODY)
def test_one_body_arrangements_on_the_wave_form(arrangements, name):
    """The wave-per-job form takes the one-body arrangements as well: the same assertions, and the class of the lane form."""
    for k, L in enumerate(G.cases(arrangements, name)[:3]):
        out = G.run_emu(L["P"], L["x"], L["params"], L["per_point"], L["groups"], L["mu_base"], form=0)
        bad = G.check_group_answer(L, out)
        assert not bad, (name, k, bad[:5])
        assert np.array_equal(M.device_class(out["kappa_hi"]), M.device_class(L["emu"]["kappa_hi"]))


@pytest.mark.parametrize("name", G.FRICTION)
def test_full_bisections_and_order(arrangements, name):
    """Assertions 6 and 7 under emulation.  Full CPU bisections of the algorithm on the reference on at most 64 finite (job, group)
    pairs of the arrangement: |kappa - kappa_ref| <= 1e-6 (the project's facet bound); and the order against the common margin (no
    base table): where kappa*_all <= 1 no group needs more than it, where it is > 1 or inf every group alone needs at least as
    much -- first between the reference bisections of group and common margin, then on the emulation's answers for every job."""
    launches = [L for L in G.cases(arrangements, name)]
    ng = len(launches[0]["groups"])
    worst, count = 0.0, 0
    for g in range(ng):
        vs = G.group_views(launches, g)
        for k, i, s, kref, _ in M.reference_bisections(vs, limit=64 // ng):
            worst = max(worst, abs(launches[k]["emu"]["kappa_hi"][i, s, g] - kref))
            count += 1
            if launches[k]["mu_base"] is None:
                call = M.Jobs(launches[k]).bisect(i, s)[0]
                assert not len(G.check_order(np.array([call]), np.array([[kref]]))), (name, g, k, i, s, call, kref)
    print("group margin, emulation vs reference bisection, %s: %d finite pairs, largest |kappa - kappa_ref| %.2e" % (name, count, worst))
    assert worst <= 1e-6, (name, worst)
    for L in launches:
        if L["mu_base"] is None:
            com = M.run_emu(L["P"], L["x"], L["params"], L["per_point"])
            assert not len(G.check_order(com["kappa_hi"], L["emu"]["kappa_hi"])), name


@pytest.mark.parametrize("name", G.FRICTION)
def test_share_of_decisions_next_to_the_boundary(arrangements, name):
    """Assertion 8's rule on the reference: the (job, group) pairs with a decision within 1e-9 max(|b|, 1) of the boundary -- the ones
    iteration counts are not compared on -- are at most half of every launch."""
    launches = G.cases(arrangements, name)
    ng = len(launches[0]["groups"])
    masks = [M.near_masks(G.group_views(launches, g)) for g in range(ng)]
    for k in range(len(launches)):
        near = sum(int(masks[g][k].sum()) for g in range(ng))
        size = sum(masks[g][k].size for g in range(ng))
        print("group margin, %s launch %d: %d of %d pairs next to the boundary" % (name, k, near, size))
        assert near <= 0.5 * size or size <= ng    # (a launch of one job is all or nothing)


def test_kernel_resources():
    """Assertion 12, from the compiler's resource remarks (no GPU): the new lane kernel keeps 0 B of scratch inside 256 VGPRs, the new
    wave kernel 0 B of scratch, and the six kernels that were there keep the figures they had before the per-contact scale source
    (measured on the parent commit: 121, 221, 123, 223, 126, 248 VGPRs, 0 B scratch)."""
    sys.path.insert(0, str(ROOT / "tools"))
    import kernel_resources

    use = {k: v for k, v in kernel_resources.usage("api").items() if "upr_bal_" in k}
    by = lambda stem: [v for k, v in use.items() if re.search(r"\d%s[\dA-Z]" % stem, k)][0]   # noqa: E731
    for stem, vgpr in (("upr_bal_project_kernel", 121), ("upr_bal_project1_kernel", 221), ("upr_bal_project_mu_kernel", 123),
                       ("upr_bal_project1_mu_kernel", 223), ("upr_bal_margin_kernel", 126), ("upr_bal_margin1_kernel", 248)):
        u = by(stem)
        print(stem, u)
        assert (u["vgpr"], u["scratch"], u["spill"]) == (vgpr, 0, 0), (stem, u)
    lane, wave = by("upr_bal_margin1_grp_kernel"), by("upr_bal_margin_grp_kernel")
    print("upr_bal_margin1_grp_kernel", lane, "upr_bal_margin_grp_kernel", wave)
    assert lane["scratch"] == 0 and lane["spill"] == 0 and lane["vgpr"] <= 256
    assert wave["scratch"] == 0 and wave["spill"] == 0
    for stem in ("upr_bal_project_cmu_kernel", "upr_bal_project1_cmu_kernel", "upr_bal_margin_worst_kernel"):
        assert by(stem)["scratch"] == 0
