"""Every refusal of the ten entries of the balance family (upr_batch_balance_points / _plan with their _mu and _cmu twins,
upr_batch_friction_margin_points / _plan, upr_batch_friction_margin_groups_points / _plan), through ctypes so that nothing in Python
refuses first: which message a bad argument gets, which message wins when several arguments are bad, the empty call, and that a
refused call leaves the handle as it was.  fixture_box (one body with friction: the lane form), B = 1, two points, four scenarios;
once more with UPR_BAL_FORM=0, the wave form."""
import ctypes as C
import re

import numpy as np
import pytest

import balance_ref as R
from upright_amd._capi import iptr, ptr
from upright_amd.engine import BatchMPC

pytestmark = pytest.mark.gpu

# the arguments of every entry in the order of include/upright_mi.h (after the handle); who: the name its messages carry (the _mu
# entries speak as their twins); null / need: the message about its required pointers and which they are; scale: its table of
# friction scales and the word the refusal of a bad entry uses (mu_scale_c is refused as "mu_scale")
POINTS_RHO = ("n", "x", "n_scen", "params", "per", "rho", "z", "iters")
ENTRIES = {
    "upr_batch_balance_points": dict(args=POINTS_RHO, null="x, params and rho must not be NULL", need=("x", "params", "rho")),
    "upr_batch_balance_points_mu": dict(args=POINTS_RHO[:5] + ("mu_scale",) + POINTS_RHO[5:], who="upr_batch_balance_points",
                                        null="x, params and rho must not be NULL", need=("x", "params", "rho"), scale=("mu_scale", "mu_scale")),
    "upr_batch_balance_points_cmu": dict(args=POINTS_RHO[:5] + ("mu_scale_c",) + POINTS_RHO[5:], null="x, params, mu_scale_c and rho must not be NULL",
                                         need=("x", "params", "mu_scale_c", "rho"), scale=("mu_scale_c", "mu_scale")),
    "upr_batch_balance_plan": dict(args=("n_scen", "params", "per", "rho", "iters"), null="rho must not be NULL", need=("rho",)),
    "upr_batch_balance_plan_mu": dict(args=("n_scen", "params", "per", "mu_scale", "rho", "iters"), who="upr_batch_balance_plan", null="rho must not be NULL",
                                      need=("rho",), scale=("mu_scale", "mu_scale")),
    "upr_batch_balance_plan_cmu": dict(args=("n_scen", "params", "per", "mu_scale_c", "rho", "iters"), null="mu_scale_c and rho must not be NULL",
                                       need=("mu_scale_c", "rho"), scale=("mu_scale_c", "mu_scale")),
    "upr_batch_friction_margin_points": dict(args=("n", "x", "n_scen", "params", "per", "kappa_max", "kappa_hi", "kappa_lo", "z", "y", "iters"),
                                             null="x, params and kappa_hi must not be NULL", need=("x", "params", "kappa_hi")),
    "upr_batch_friction_margin_plan": dict(args=("n_scen", "params", "per", "kappa_max", "kappa_hi", "kappa_lo", "iters"), null="kappa_hi must not be NULL",
                                           need=("kappa_hi",)),
    "upr_batch_friction_margin_groups_points": dict(
        args=("n", "x", "n_scen", "params", "per", "n_grp", "group_mask", "mu_base", "kappa_max", "kappa_hi", "kappa_lo", "z", "y", "iters"),
        null="x, params and kappa_hi must not be NULL", need=("x", "params", "kappa_hi"), scale=("mu_base", "mu_base")),
    "upr_batch_friction_margin_groups_plan": dict(
        args=("n_scen", "params", "per", "n_grp", "group_mask", "mu_base", "kappa_max", "kappa_hi", "kappa_lo", "iters", "worst", "worst_knot"),
        null="kappa_hi and worst must not both be NULL", need=("kappa_hi",), scale=("mu_base", "mu_base")),
}
NAMES = sorted(ENTRIES)
POINTS = [n for n in NAMES if "n" in ENTRIES[n]["args"]]
PLAN = [n for n in NAMES if n not in POINTS]
OUTPUTS = ("rho", "kappa_hi", "kappa_lo", "z", "y", "iters", "worst", "worst_knot")
KAPPA = "friction margin: kappa_max must be finite and > 0"
MASS = "balance check: every body of every scenario needs a positive finite mass"
POISON = -7.0


def _who(name):
    return ENTRIES[name].get("who", name)


class Rig:
    """A handle on fixture_box with valid arguments for every entry; call(name, **changes) runs an entry with some of them replaced."""

    def __init__(self, arrangements):
        P = R.table_problem(arrangements, "fixture_box")
        self.P, self.h = P, BatchMPC(P, 1)
        self.x = R.points(P, ["lift", "inside"], seed=1)
        self.scen = np.ascontiguousarray(R.scenarios(P))
        assert self.x.shape == (2, P.nx) and self.scen.shape == (4, P.nb, 10) and (P.nb, P.nc) == (1, 8)
        room = (P.N + 1) * 4 * 2 * 32   # the largest output of a valid call here: z of the plan's knots, four scenarios, two groups
        self.vals = dict(n=2, x=self.x, n_scen=4, params=self.scen, per=0, mu_scale=np.ones(4), mu_scale_c=np.ones((4, P.nc)), mu_base=np.ones((4, P.nc)),
                         kappa_max=8.0, n_grp=2, group_mask=np.array([0x0F, 0xF0], dtype=np.uint32), rho=np.zeros(room), kappa_hi=np.zeros(room),
                         kappa_lo=np.zeros(room), z=np.zeros(room), y=np.zeros(room), iters=np.zeros(room, dtype=np.int32), worst=np.zeros(room),
                         worst_knot=np.zeros(room, dtype=np.int32))

    @staticmethod
    def _c(v):
        if v is None or not isinstance(v, np.ndarray):
            return v
        if v.dtype == np.uint32:
            return v.ctypes.data_as(C.POINTER(C.c_uint))
        return iptr(v) if v.dtype == np.int32 else ptr(v)

    def call(self, name, **changes):
        """(return code, message of upr_last_error after it)"""
        vals = {**self.vals, **changes}
        keep = [np.ascontiguousarray(vals[a]) if isinstance(vals[a], np.ndarray) else vals[a] for a in ENTRIES[name]["args"]]
        rc = getattr(self.h._lib, name)(self.h._h, *[self._c(v) for v in keep])
        return rc, self.h._lib.upr_last_error().decode()

    def refused(self, name, message, **changes):
        rc, err = self.call(name, **changes)
        assert rc != 0 and re.search(re.escape(message), err), (name, changes.keys(), rc, err, message)

    def answer(self):
        return self.h.balance_check(self.x, self.scen, want_z=True, want_iters=True)


@pytest.fixture(params=["", "0"])
def rig(request, arrangements, monkeypatch):
    """The rig, with the handle's answer to balance_check before the refusals; after the test the handle must give the same bits."""
    if request.param:
        monkeypatch.setenv("UPR_BAL_FORM", request.param)
    r = Rig(arrangements)
    before = r.answer()
    yield r
    after = r.answer()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    r.h.close()


def _bad_params(scen, value):
    bad = scen.copy()
    bad[2, 0, 0] = value
    return bad


def _bad_scale(like, value):
    bad = like.copy()
    bad.flat[bad.size - 2] = value
    return bad


@pytest.mark.parametrize("name", NAMES)
def test_pointers_and_scenario_counts(rig, name):
    """Each required pointer as NULL gives the entry's own message; n_scen = 0 is refused; a plan entry without params takes one
    scenario only."""
    E = ENTRIES[name]
    null = _who(name) + ": " + E["null"]
    for a in E["need"]:
        changes = {a: None}
        if name == "upr_batch_friction_margin_groups_plan":
            changes["worst"] = None   # (kappa_hi or worst: either carries a result)
        rig.refused(name, null, **changes)
    rig.refused(name, _who(name) + ": n_scen must be >= 1", n_scen=0)
    rig.refused(name, _who(name) + ": n_scen must be >= 1", n_scen=-3)
    if name in PLAN:
        own = _who(name) + ": params == NULL needs n_scen == 1 (every instance's own body parameters)"
        rig.refused(name, own, params=None, n_scen=2)
        rig.refused(name, own, params=None, n_scen=0)


@pytest.mark.parametrize("name", NAMES)
def test_values(rig, name):
    """Masses, friction scales, kappa_max and the group masks."""
    E = ENTRIES[name]
    for m in (0.0, -1.0, np.nan):
        rig.refused(name, MASS, params=_bad_params(rig.scen, m))
    if "scale" in E:
        arg, word = E["scale"]
        for v in (-0.5, np.inf):
            rig.refused(name, "balance check: every " + word + " must be finite and >= 0", **{arg: _bad_scale(rig.vals[arg], v)})
    if "kappa_max" in E["args"]:
        for k in (0.0, -1.0, np.inf, np.nan):
            rig.refused(name, KAPPA, kappa_max=k)
    if "n_grp" in E["args"]:
        grp = "friction margin of contact groups: "
        rig.refused(name, grp + "n_grp must be in 1 .. 65535", n_grp=0)
        rig.refused(name, grp + "n_grp must be in 1 .. 65535", n_grp=65536)
        rig.refused(name, grp + "group_mask must not be NULL", group_mask=None)
        rig.refused(name, grp + "group 1 has an empty mask", group_mask=np.array([3, 0], dtype=np.uint32))
        rig.refused(name, grp + "group 1 has a mask bit >= nc = 8", group_mask=np.array([3, 0x100], dtype=np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_precedence(rig, name):
    """Every argument bad at once, then mended one by one in the order of the checks: kappa_max, the groups, the required pointers,
    n_scen, the masses, the scales, and (points entries) the bound on n, which reads nothing."""
    E = ENTRIES[name]
    out = "kappa_hi" if "kappa_hi" in E["args"] else "rho"
    faults = []   # (changes, message), first check first
    if "kappa_max" in E["args"]:
        faults.append((dict(kappa_max=np.nan), KAPPA))
    if "n_grp" in E["args"]:
        faults.append((dict(n_grp=0), "friction margin of contact groups: n_grp must be in 1 .. 65535"))
    faults.append(({out: None, "worst": None}, _who(name) + ": " + E["null"]))
    faults.append((dict(n_scen=0), _who(name) + ": n_scen must be >= 1"))
    faults.append((dict(params=_bad_params(rig.scen, -1.0)), MASS))
    if "scale" in E:
        arg, word = E["scale"]
        faults.append(({arg: _bad_scale(rig.vals[arg], -0.5)}, "balance check: every " + word + " must be finite and >= 0"))
    if name in POINTS:
        faults.append((dict(n=2**31 - 1), "balance check: too many points"))
    for first in range(len(faults)):
        changes = {}
        for c, _ in faults[first:]:
            changes.update({k: v for k, v in c.items() if k in E["args"]})
        rig.refused(name, faults[first][1], **changes)


@pytest.mark.parametrize("name", POINTS)
def test_empty_call(rig, name):
    """n = 0 (and below) returns 0 before the pointers are looked at and writes nothing."""
    outs = {a: np.full_like(rig.vals[a], POISON) for a in OUTPUTS if a in ENTRIES[name]["args"]}
    for n in (0, -1):
        assert rig.call(name, n=n, **outs)[0] == 0
        assert rig.call(name, n=n, x=None, params=None, **outs)[0] == 0
    assert all(np.all(v == v.dtype.type(POISON)) for v in outs.values())
    if "kappa_max" in ENTRIES[name]["args"]:   # (kappa_max and the groups are looked at first)
        rig.refused(name, KAPPA, n=0, kappa_max=0.0)
