"""CPU reference of the retiming with substeps (upright_amd/csrc/upr_retime_sub.h) and the assertions its CPU and GPU tests share.  The
plans, the lattices, the boxes and the programme are retime_ref's, the interpolant is replay_ref's, the residual is balance_ref's; none of
the three modules is changed.

Segment i gets the path points tau_r = r h / R, r = 0 .. R.  The reference record of a point is the plan's own at a knot (r = 0, r = R)
and numpy's Hermite (replay_ref.hermite) at sigma = tau_r / h in between; on the edge m -> m' its speed is s_r = sqrt(((R - r) s_m^2 + r
s_m'^2) / R) (the lattice doubles themselves at r = 0 and R), its state retime_ref.state_at(record, s_r, d).  The reference decision of a
state is balance_ref.reference at that JOINT-SPACE state -- accepted when rho_ref <= EPS max(|b|, 1), DECIDED when |rho_ref - EPS max(|b|,
1)| > RHO_TOL max(|b|, 1).  The states of an edge come in the kernel's order: departing, arriving, then r = 1 .. R - 1 ascending, and the
edge stops at its first rejection; an edge is decided when every state the kernel would evaluate is, a plan when all its edges are.  On
the slide (retime_ref.slide_plans: a quintic in time, which its Hermite segments reproduce exactly) the closed form of a point's margin
is mu0 g0 - |s_r^2 c(tau) + d w(tau)|, c and w the analytic second and first derivative of the profile.

run(P, xs, params, speeds, substeps=1, start=-1, end=-1, common=False, boxes=True, form=-1, fma=False) -> dict(duration, level, reach,
edges, iters) is what a test file hands to the bodies below: the NEW entry at every substeps, 1 included."""
import ctypes as C
import os
import time
from pathlib import Path

import numpy as np

import balance_ref as R
import replay_ref as Y
import retime_ref as Q

EPS, RHO_TOL = Q.EPS, Q.RHO_TOL
NARROW = (1.11, 1.1185)      # the lattice whose lower level repairs the slide at 1.1185 between the knots


def sub_speed(s0, s1, r, Rs):
    if r == 0:
        return float(s0)
    if r == Rs:
        return float(s1)
    return float(np.sqrt((float(Rs - r) * (s0 * s0) + float(r) * (s1 * s1)) / float(Rs)))


def fine_plan(P, xs, Rs):
    """numpy's fine plan (B, N Rs + 1, 3 nq): the knots verbatim, the interior points by replay_ref.hermite"""
    xs = np.asarray(xs, dtype=np.float64)
    B, nk = xs.shape[:2]
    N, h, nq = nk - 1, float(P.dt), P.nq
    xf = np.zeros((B, N * Rs + 1, 3 * nq))
    for b in range(B):
        for i in range(N):
            xf[b, i * Rs] = xs[b, i, :3 * nq]
            for r in range(1, Rs):
                tau = float(r) * h / float(Rs)
                xf[b, i * Rs + r] = np.concatenate(Y.hermite(xs[b, i], xs[b, i + 1], h, tau / h, nq))
        xf[b, N * Rs] = xs[b, N, :3 * nq]
    return xf


def ref_masks(P, xs, params, speeds, boxes, Rs, closed=None, nominal=None):
    """retime_ref.ref_masks with the R + 1 points of an edge: dict(masks (B, ns, N, M) uint32, decided (B, ns, N, M, M) bool, evals {(b,
    sc, fine point, s, d): (accepted, decided)}, box_margin: the smallest |distance to a bound| over the box decisions, box_interior: the
    edges only an interior box cuts, near: the smallest |margin| over the closed-form evaluations, near_all: the same over every point of
    every existing edge, evaluated or not, rejected: the (b, segment, r) of the
    closed form's rejections, records: the reference evaluations made).  closed(b, i, r, s, d) -> signed margin of point r of segment i:
    a closed form in place of rho_ref (accepted iff >= 0), every decision decided.  nominal: evaluations {(b, sc, knot, s, d): ..} of the
    knots to take instead of computing them (retime_ref.ref_masks' `evals` on the same plans and scenarios)."""
    xs = np.asarray(xs)
    speeds = np.asarray(speeds, dtype=np.float64)
    params = np.asarray(params, dtype=np.float64).reshape(-1, P.nb, 10)
    B, nk, ns, M, h, nq = xs.shape[0], xs.shape[1], params.shape[0], speeds.size, float(P.dt), P.nq
    N = nk - 1
    xf = fine_plan(P, xs, Rs)
    masks = np.zeros((B, ns, N, M), dtype=np.uint32)
    decided = np.ones((B, ns, N, M, M), dtype=bool)
    evals, rejected = {}, set()
    bm, near, near_all, box_interior, count = np.inf, np.inf, np.inf, 0, 0

    for b in range(B):
        for i in range(N):
            for m in range(M):
                for mp in range(M):
                    s0, s1 = speeds[m], speeds[mp]
                    if not s0 + s1 > 0.0:
                        continue
                    d = Q.accel(s0, s1, h)
                    order = [0, Rs] + list(range(1, Rs))
                    sr = {r: sub_speed(s0, s1, r, Rs) for r in order}
                    if boxes:
                        g = [Q.box_margin(P, xf[b, i * Rs + r], sr[r], d) for r in order]
                        bm = min(bm, min(abs(v) for v in g))
                        if min(g) < 0.0:
                            box_interior += int(min(g[:2]) >= 0.0)
                            continue
                    if closed is not None:
                        near_all = min(near_all, min(abs(closed(b, i, r, sr[r], d)) for r in order))
                    for sc in range(ns):
                        ok, dec = True, True
                        for r in order:
                            if not (ok and dec):
                                break
                            key = (b, sc, i * Rs + r, sr[r], float(d))
                            if key not in evals:
                                knot = (b, sc, i + r // Rs, sr[r], float(d))
                                if closed is not None:
                                    g = closed(b, i, r, sr[r], d)
                                    near = min(near, abs(g))
                                    evals[key] = (g >= 0.0, True)
                                elif r in (0, Rs) and nominal is not None and knot in nominal:
                                    evals[key] = nominal[knot]
                                else:
                                    count += 1
                                    out = R.reference(P, Q.state_at(xf[b, i * Rs + r], sr[r], d, nq)[None], params[sc:sc + 1], False)
                                    rho, scale = float(out["rho"][0, 0]), max(float(out["bnorm"][0, 0]), 1.0)
                                    evals[key] = (rho <= EPS * scale, abs(rho - EPS * scale) > RHO_TOL * scale)
                            ok, dec = evals[key]
                            if closed is not None and not ok:
                                rejected.add((b, i, r))
                        decided[b, sc, i, m, mp] = dec
                        if ok:
                            masks[b, sc, i, m] |= np.uint32(1) << np.uint32(mp)
    return dict(masks=masks, decided=decided, evals=evals, box_margin=bm, box_interior=box_interior, near=near, near_all=near_all, rejected=rejected, records=count)


# ---- the kernel source through the host emulation -----------------------------------------------------------------------------------
def emu_lib(fma=False):
    name = "libupr_retime_sub_emu_fma.so" if fma else "libupr_retime_sub_emu.so"
    return C.CDLL(os.environ.get("UPR_RETIME_SUB_EMU_FMA_LIB" if fma else "UPR_RETIME_SUB_EMU_LIB", str(Path(__file__).resolve().parent / "emu" / name)))


def have_fma_twin():
    try:
        has_fma = " fma " in Path("/proc/cpuinfo").read_text().replace("\n", " ")
    except OSError:
        has_fma = False
    if has_fma:
        assert (Path(__file__).resolve().parent / "emu" / "libupr_retime_sub_emu_fma.so").exists(), "the host has FMA but libupr_retime_sub_emu_fma.so was not built"
    return has_fma


def blank(B, ns, nk, M, common):
    lead = (B,) if common else (B, ns)
    return dict(duration=np.full(lead, np.nan), level=np.full(lead + (nk,), -9, dtype=np.int32), reach=np.full(lead + (2,), -9, dtype=np.int32),
                edges=np.zeros((B, ns, nk - 1, M), dtype=np.uint32), iters=np.full((B, ns, nk - 1, M), -1, dtype=np.int32))


def _scenarios(P, B, params):
    """(params, per instance, n_scen); None: every instance's own body parameters, laid out per instance"""
    if params is None:
        return np.ascontiguousarray(np.repeat(np.asarray(P.body_params, dtype=np.float64)[None, None], B, axis=0)), True, 1
    params = np.ascontiguousarray(params, dtype=np.float64)
    per = params.ndim == 4
    return params, per, params.shape[1] if per else params.reshape(-1, P.nb, 10).shape[0]


def run_emu(P, xs, params, speeds, substeps=1, start=-1, end=-1, common=False, boxes=True, form=-1, fma=False):
    """emu_ret_sub_plan: the refinement, the state points, the mask jobs and the programme compiled for the host"""
    from upright_amd import _capi

    xs = np.ascontiguousarray(xs, dtype=np.float64)
    B, nk = xs.shape[:2]
    params, per, ns = _scenarios(P, B, params)
    speeds = np.ascontiguousarray(speeds, dtype=np.float64)
    out = blank(B, ns, nk, speeds.size, common)
    cp = _capi.problem_to_c(P)
    rc = emu_lib(fma).emu_ret_sub_plan(C.byref(cp), B, nk, _capi.ptr(xs), ns, _capi.ptr(params), 1 if per else 0, speeds.size, _capi.ptr(speeds), int(start),
                                       int(end), int(common), int(boxes), int(substeps), _capi.ptr(out["duration"]), _capi.iptr(out["level"]),
                                       _capi.iptr(out["reach"]), out["edges"].ctypes.data_as(C.POINTER(C.c_uint)), _capi.iptr(out["iters"]), int(form))
    assert rc == 0
    return out


def emu_fine(P, xs, Rs, fma=False):
    """the refinement kernel's body: xf (B, N Rs + 1, 3 nq)"""
    from upright_amd import _capi

    xs = np.ascontiguousarray(xs, dtype=np.float64)
    B, nk = xs.shape[:2]
    xf = np.full((B, (nk - 1) * Rs + 1, 3 * P.nq), np.nan)
    cp = _capi.problem_to_c(P)
    assert emu_lib(fma).emu_ret_sub_refine(C.byref(cp), B, nk, _capi.ptr(xs), int(Rs), _capi.ptr(xf)) == 0
    return xf


def run_device(mpc, xs, params, speeds, substeps=1, start=-1, end=-1, common=False, boxes=True):
    """upr_batch_retime_plan_substeps through ctypes on the plan xs installed with set_guess (BatchMPC.retime_plan sends substeps=1 to the
    plain entry)"""
    from upright_amd import _capi

    P = mpc.problem
    mpc.set_guess(xs, np.zeros((mpc.B, mpc.N, mpc.nu)))
    speeds = np.ascontiguousarray(speeds, dtype=np.float64)
    if params is None:
        par, per, ns = None, False, 1
    else:
        par, per, ns = _scenarios(P, mpc.B, params)
    out = blank(mpc.B, ns, mpc.N + 1, speeds.size, common)
    rc = mpc._lib.upr_batch_retime_plan_substeps(mpc._h, ns, _capi.ptr(par), int(per), speeds.size, _capi.ptr(speeds), int(start), int(end), int(common),
                                                 int(boxes), int(substeps), _capi.ptr(out["duration"]), _capi.iptr(out["level"]), _capi.iptr(out["reach"]),
                                                 out["edges"].ctypes.data_as(C.POINTER(C.c_uint)), _capi.iptr(out["iters"]))
    assert rc == 0, mpc._lib.upr_last_error()
    return out


# ---- the cases the CPU and the GPU tests share (built once per process) -------------------------------------------------------------
_CASES = {}


def slide_closed(S):
    """closed(b, i, r, s, d) of retime_ref.slide_case at substeps Rs -> the margin of point r of segment i, and the same at a path time"""
    P = S["P"]
    N, h = P.N, float(P.dt)
    Tt = N * h

    def at(b, tau_abs, s, d):
        length = S["xs"][b, -1, 0] - S["xs"][b, 0, 0]
        _, d1, d2 = Q.min_jerk(tau_abs / Tt)
        return S["bound"] - abs(s * s * length * d2 / (Tt * Tt) + d * length * d1 / Tt)

    def make(Rs):
        return lambda b, i, r, s, d: at(b, i * h + float(r) * h / float(Rs), s, d)
    return make


def slide_ref(arrangements, speeds, Rs):
    key = ("slide", tuple(speeds), Rs)
    if key not in _CASES:
        S = Q.slide_case(arrangements)
        _CASES[key] = ref_masks(S["P"], S["xs"], S["params"], np.array(speeds), False, Rs, closed=slide_closed(S)(Rs))
    return _CASES[key]


def generic_case(arrangements, name="pink_bottle", B=3, plans=2, speeds=Q.GENERIC["speeds"], Rs=3):
    """retime_ref.generic_case and the reference at substeps Rs on its first `plans` plans (key "sub"; the knots' evaluations are those
    of retime_ref's reference)"""
    key = ("generic", name, B, plans, tuple(speeds), Rs)
    if key not in _CASES:
        G = dict(Q.generic_case(arrangements, name, B, speeds))
        t0 = time.time()
        G["plans"], G["Rs"] = plans, Rs
        G["sub"] = ref_masks(G["P"], G["xs"][:plans], G["params"], G["speeds"], True, Rs, nominal=G["ref"]["evals"])
        print("retime with substeps, %s, R = %d: the reference of %d plans took %.1f s (%d evaluations beyond the knots')"
              % (name, Rs, plans, time.time() - t0, G["sub"]["records"]))
        _CASES[key] = G
    return _CASES[key]


def first_plans(out, n):
    return {k: (v[:n] if v is not None else None) for k, v in out.items()}


def same(a, b, keys=("duration", "level", "reach", "edges", "iters")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


# ---- the assertions both test files make ----------------------------------------------------------------------------------------------
def body_slide(run, arrangements, replay=None):
    """1.  replay(P, xs, params, speeds, level (B, N + 1), tick, K) -> replay_ref's dict, boxes off."""
    S = Q.slide_case(arrangements)
    P, xs, par, h, N = S["P"], S["xs"], S["params"], float(S["P"].dt), S["P"].N
    g0 = S["bound"]
    cases = [((1.1185,), Rs) for Rs in (1, 2, 4, 8)] + [(NARROW, Rs) for Rs in (1, 2, 4, 8)] + [(Q.SLIDE_SPEEDS, Rs) for Rs in (2, 4, 8)]
    refs = {c: slide_ref(arrangements, *c) for c in cases}
    print("retime with substeps, slide: the closest closed-form decision, in mu0 g0: %s" % {c: "%.2e" % (refs[c]["near"] / g0) for c in cases})
    print("retime with substeps, slide: ... over every point of every existing edge, evaluated or not: %s" % {c: "%.2e" % (refs[c]["near_all"] / g0) for c in cases})
    assert all(refs[c]["near_all"] >= 1e-6 * g0 for c in cases)  # (on the closed form alone, before any answer is looked at)
    # what the closed form says, before any answer is looked at
    one = (1.1185,)
    assert not refs[one, 1]["rejected"] and not refs[one, 2]["rejected"]            # (the sigma = 1 / 2 points miss the peak: not claimed)
    assert abs(refs[one, 1]["near"] / g0 - 1.5e-3) < 1e-4 and abs(refs[one, 2]["near"] / g0 - 1.5e-3) < 1e-4
    for b in range(xs.shape[0]):
        assert {(i, r) for bb, i, r in refs[one, 4]["rejected"] if bb == b} == {(4, 1), (15, 3)}
    assert abs(refs[one, 4]["near"] / g0 - 8.1e-4) < 1e-5 and abs(refs[one, 8]["near"] / g0 - 1.5e-4) < 1e-5
    assert all(abs(refs[Q.SLIDE_SPEEDS, Rs]["near_all"] / g0 - v) < 0.03 * v for Rs, v in ((2, 1.7e-3), (4, 1.05e-3), (8, 2.8e-4)))
    outs = {}
    for c in cases:
        speeds, Rs = np.array(c[0]), c[1]
        out = outs[c] = run(P, xs, par, speeds, substeps=Rs, boxes=False)
        assert np.array_equal(out["edges"], refs[c]["masks"]), c
        Q.check_invariants(out, speeds, h)
        for b in range(xs.shape[0]):
            want = Q.programme(refs[c]["masks"][b, 0], speeds, h)
            dur = float(out["duration"][b, 0])
            assert dur == want["duration"] or abs(dur - want["duration"]) <= 1e-12 * want["duration"], (c, b, dur, want["duration"])
            assert np.array_equal(out["level"][b, 0], want["level"]), (c, b)
    uniform = N * h / 1.1185
    assert abs(uniform - 1.788109) < 1e-6
    for Rs in (1, 2):
        assert np.all(np.abs(outs[one, Rs]["duration"] - uniform) <= 1e-12 * uniform) and np.all(outs[one, Rs]["level"] == 0)
        assert np.all(np.abs(outs[NARROW, Rs]["duration"] - uniform) <= 1e-12 * uniform) and np.all(outs[NARROW, Rs]["level"] == 1)
    for Rs in (4, 8):
        assert np.all(np.isinf(outs[one, Rs]["duration"])) and np.all(outs[one, Rs]["level"] == -1)
        assert np.all(outs[one, Rs]["reach"] == np.array([4, 16]))
        assert np.all(np.abs(outs[NARROW, Rs]["duration"] - 1.789473) < 1e-6)
        want = np.ones(N + 1, dtype=np.int32)
        want[[5, 15]] = 0
        assert np.all(outs[NARROW, Rs]["level"] == want), outs[NARROW, Rs]["level"]
    for Rs in (2, 4, 8):
        assert np.all(np.abs(outs[Q.SLIDE_SPEEDS, Rs]["duration"] - 1.856566) < 1e-6)     # (retime_ref's law: the peaks lie on knots)
    # the R = 4 law on a 10 ms clock rejects no sample, the R = 1 law rejects 37-39 and 140-142 (replay_ref's closed form, then the call)
    sp = np.array(NARROW)
    for Rs, want in ((4, []), (1, [37, 38, 39, 140, 141, 142])):
        level = outs[NARROW, Rs]["level"][:, 0]
        K = Y.default_K(level, sp, h, 0.01, 0.0)
        rp = Y.replay(P, xs[0], level[0], sp, 0.01, 0.0, K)
        m = Y.slide_margins(S, rp)
        assert np.abs(m).min() >= 1e-6 and np.flatnonzero(m < 0).tolist() == want, (Rs, np.abs(m).min(), np.flatnonzero(m < 0))
        if Rs == 4:
            print("retime with substeps, slide: the R = 4 law on a 10 ms clock: %d samples, the smallest closed-form margin %.2e mu0 g0" % (rp["count"], m.min()))
            assert abs(m.min() - 3.6e-3) < 1e-4
        if replay is not None:
            got = replay(P, xs, par, sp, level, 0.01, K)
            assert np.all(got["count"] == rp["count"]) and np.all(got["verdict"][:, 0, 2] == len(want))
            assert np.flatnonzero(~(got["excess"][0, :rp["count"], 0] <= EPS)).tolist() == want
    return outs


def body_r1_is_the_plain_retiming(run, plain, arrangements, forms=(-1, 0)):
    """2.  plain(P, xs, params, speeds, start, end, common, boxes, form) -> the dict of upr_batch_retime_plan (retime_ref's runners)"""
    G, S = Q.generic_case(arrangements), Q.slide_case(arrangements)
    n = 0
    for form in forms:
        for P, xs, params, speeds, kw in ((G["P"], G["xs"], G["params"], G["speeds"], dict()),
                                          (G["P"], G["xs"], Q.with_vertex(G["P"]), G["speeds"], dict(common=True)),
                                          (S["P"], S["xs"], S["params"], S["speeds"], dict(boxes=False)),
                                          (S["P"], S["xs"], S["params"], S["speeds"], dict(start=0, end=0))):
            a = run(P, xs, params, speeds, substeps=1, form=form, **kw)
            b = plain(P, xs, params, speeds, form=form, **kw)
            assert same(a, b), (form, kw)
            n += 1
    return n


def body_reference(run, arrangements, name="pink_bottle", B=3, plans=2, speeds=Q.GENERIC["speeds"], Rs=3, **kw):
    """3. (and 8. on another form)"""
    G = generic_case(arrangements, name, B, plans, speeds, Rs)
    ref = G["sub"]
    share = Q.undecided_share(ref)
    assert share <= 0.10, share                               # (conditions on the reference alone, before any answer is looked at)
    assert ref["box_margin"] >= 1e-9, ref["box_margin"]
    out = run(G["P"], G["xs"], G["params"], G["speeds"], substeps=Rs, **kw)
    h = float(G["P"].dt)
    n_dec, n_lvl = Q.against_reference(first_plans(out, plans), ref, G["speeds"], h)
    Q.check_invariants(out, G["speeds"], h)
    print("retime with substeps, %s, R = %d: undecided edges %.3f of %d, box margin %.1e, edges an interior box alone cuts %d, decided plans %d of %d, "
          "levels compared on %d; durations %s" % (name, Rs, share, ref["decided"].size, ref["box_margin"], ref["box_interior"], n_dec, plans * 2, n_lvl,
                                                   np.round(out["duration"][:plans].ravel(), 4).tolist()))
    assert n_dec >= 1 and n_lvl >= 1
    return out


def body_nesting(run, arrangements):
    """4.  The point sets nest: on the slide (every edge decided by the closed form) and on plan 0 of the generic case, on the edges the
    references at R = 1, 2 and 4 all decide."""
    S = Q.slide_case(arrangements)
    for speeds in (S["speeds"], np.array(NARROW)):
        outs = [run(S["P"], S["xs"], S["params"], speeds, substeps=Rs, boxes=False) for Rs in (1, 2, 4)]
        for fine, coarse in zip(outs[1:], outs[:-1]):
            assert not np.any(fine["edges"] & ~coarse["edges"]) and np.all(fine["duration"] >= coarse["duration"])
    assert np.any(outs[2]["edges"] != outs[0]["edges"])          # (the narrow lattice: R = 4 sees the peaks between the knots)
    G2, G4 = generic_case(arrangements, plans=1, Rs=2), generic_case(arrangements, plans=1, Rs=4)
    G = Q.generic_case(arrangements)
    bits = Q.decided_bits(G["ref"]["decided"][:1] & G2["sub"]["decided"] & G4["sub"]["decided"])
    assert 1.0 - float((G["ref"]["decided"][:1] & G2["sub"]["decided"] & G4["sub"]["decided"]).mean()) <= 0.10
    outs = [run(G["P"], G["xs"], G["params"], G["speeds"], substeps=Rs) for Rs in (1, 2, 4)]
    for fine, coarse in zip(outs[1:], outs[:-1]):
        assert not np.any(fine["edges"][:1] & bits & ~(coarse["edges"][:1] & bits))
    if G["ref"]["decided"][0].all() and G2["sub"]["decided"][0].all() and G4["sub"]["decided"][0].all():
        assert np.all(outs[2]["duration"][0] >= outs[1]["duration"][0]) and np.all(outs[1]["duration"][0] >= outs[0]["duration"][0])
    cut = [int(np.count_nonzero(o["edges"][:1] & bits)) for o in outs]
    print("retime with substeps, nesting: admissible decided rows of plan 0 at R = 1, 2, 4: %s; durations %s" % (cut, [np.round(o["duration"][0], 4).tolist() for o in outs]))
    return outs


def substates(P, xs, level, speeds, Rs):
    """numpy's (t, x) of BatchMPC.retimed_substates without a handle: level (B, ns, N + 1), t (B, ns, N, Rs + 1), x (.., 3 nq)"""
    speeds = np.asarray(speeds, dtype=np.float64)
    B, ns, nk = level.shape
    N, h, nq = nk - 1, float(P.dt), P.nq
    xf = fine_plan(P, xs, Rs)
    t, x = np.full((B, ns, N, Rs + 1), np.nan), np.full((B, ns, N, Rs + 1, 3 * nq), np.nan)
    for b in range(B):
        for sc in range(ns):
            if level[b, sc, 0] < 0:
                continue
            s = speeds[level[b, sc]]
            T = np.concatenate([[0.0], np.cumsum(2.0 * h / (s[:-1] + s[1:]))])
            for i in range(N):
                d = Q.accel(s[i], s[i + 1], h)
                for r in range(Rs + 1):
                    sr = sub_speed(s[i], s[i + 1], r, Rs)
                    t[b, sc, i, r] = T[i] + 2.0 * (float(r) * h / float(Rs)) / (s[i] + sr)
                    x[b, sc, i, r] = Q.state_at(xf[b, i * Rs + r], sr, d, nq)
    return t, x


def body_fine_records(arrangements, fma=False):
    """5. the refinement through the emulation against numpy's Hermite; the knots bit for bit.  Returns the largest errors."""
    G = Q.generic_case(arrangements)
    errs = np.zeros(3)
    for Rs in (1, 2, 3, 16):
        xf, ref = emu_fine(G["P"], G["xs"], Rs, fma), fine_plan(G["P"], G["xs"], Rs)
        assert xf.shape == ref.shape and np.array_equal(xf[:, ::Rs], G["xs"])
        errs = np.maximum(errs, Y.assert_states(xf, ref, Rs))
    return errs


def body_substates_are_balanced(run, arrangements, balance, Rs=3):
    """5. every substate of every feasible generic law through the balance check: balance(P, x (n, 3 nq), theta (nb, 10)) -> rho (n,);
    accepted wherever the reference calls it decided"""
    G = generic_case(arrangements, Rs=Rs)
    P, nq, plans = G["P"], G["P"].nq, G["plans"]
    out = first_plans(run(P, G["xs"], G["params"], G["speeds"], substeps=Rs), plans)
    t, x = substates(P, G["xs"][:plans], out["level"], G["speeds"], Rs)
    n = n_dec = 0
    for b, sc in np.argwhere(np.isfinite(out["duration"])):
        # (t[i, R] and t[i + 1, 0] are the same knot time summed in two ways: equal to rounding)
        assert np.all(np.diff(t[b, sc].reshape(-1)) >= -1e-12) and np.all(np.diff(t[b, sc], axis=-1) > 0) and abs(t[b, sc, -1, -1] - out["duration"][b, sc]) <= 1e-12 * out["duration"][b, sc]
        pts = x[b, sc].reshape(-1, 3 * nq)
        ref = R.reference(P, pts, G["params"][sc:sc + 1], False)
        scale = np.maximum(ref["bnorm"][:, 0], 1.0)
        dec = np.abs(ref["rho"][:, 0] - EPS * scale) > RHO_TOL * scale
        rho = balance(P, pts, G["params"][sc])
        assert np.all(rho[dec] <= EPS * scale[dec]), (b, sc, rho[dec].max())
        assert np.all(ref["rho"][dec, 0] <= EPS * scale[dec])
        n += pts.shape[0]; n_dec += int(dec.sum())
    print("retime with substeps, substates: %d states of the laws at R = %d, %d decided on the reference, all accepted" % (n, Rs, n_dec))
    assert n_dec >= 40
    return out


def body_boxes(run, arrangements, Rs=4):
    """6. retime_ref's box case (joint 0 at 0.9 of its velocity bound at speed 1) at R = 4"""
    P = R.table_problem(arrangements, "pink_bottle")
    nq, h = P.nq, float(P.dt)
    vmax = float(np.asarray(P.x_ub)[nq])
    xs, c, w = Q.slide_plans(P, 1, seed=6, v_peak=0.9 * vmax)
    S = dict(P=P, xs=xs, bound=float(P.contact_mu[0]) * R.G0)
    speeds = np.array(Q.SLIDE_SPEEDS)
    closed = slide_closed(S)(Rs)
    par = np.asarray(P.body_params)[None]
    with_b, without = ref_masks(P, xs, par, speeds, True, Rs, closed=closed), ref_masks(P, xs, par, speeds, False, Rs, closed=closed)
    print("retime with substeps, boxes, R = %d: the closest box decision lies %.2e from its bound, the closest balance decision %.2e mu0 g0; an interior box "
          "alone cuts %d edges" % (Rs, with_b["box_margin"], without["near"] / S["bound"], with_b["box_interior"]))
    assert with_b["box_margin"] >= 1e-9 and without["near"] >= 1e-6 * S["bound"]
    assert np.count_nonzero(without["masks"] & ~with_b["masks"]) >= 5
    on, off = run(P, xs, par, speeds, substeps=Rs, boxes=True), run(P, xs, par, speeds, substeps=Rs, boxes=False)
    assert np.array_equal(on["edges"], with_b["masks"]) and np.array_equal(off["edges"], without["masks"])
    Q.check_invariants(on, speeds, h)
    Q.check_invariants(off, speeds, h)
    return with_b["box_interior"]


def body_common(run, arrangements, Rs=3):
    """7."""
    G = Q.generic_case(arrangements)
    P, h = G["P"], float(G["P"].dt)
    for params in (Q.shifted(P), Q.with_vertex(P)):
        one = run(P, G["xs"], params, G["speeds"], substeps=Rs, common=True)
        each = run(P, G["xs"], params, G["speeds"], substeps=Rs)
        assert np.array_equal(one["edges"], each["edges"]) and one["duration"].shape == (G["xs"].shape[0],)
        Q.check_invariants(one, G["speeds"], h, common=True)     # (the law equals numpy's programme on the AND of the returned masks)
        assert np.all(one["duration"] >= each["duration"].max(axis=1))
    assert np.all(np.isinf(one["duration"]))                      # (the vertex scenario admits nothing)


def agree(a, b, ref, plans, exact=False):
    """8. two builds of the same source: masks equal on decided edges; exact (device against the emulation of what it runs): iters on
    decided rows, duration, level and reach on decided plans.  Returns the decided rows."""
    dec = ref["decided"]
    bits = Q.decided_bits(dec)
    assert np.array_equal(a["edges"][:plans] & bits, b["edges"][:plans] & bits)
    rows = dec.all(axis=-1)
    if exact:
        assert np.array_equal(a["iters"][:plans][rows], b["iters"][:plans][rows])
        ok = dec.all(axis=(2, 3, 4))
        for k in ("duration", "level", "reach"):
            assert np.array_equal(a[k][:plans][ok], b[k][:plans][ok]), k
    return int(rows.sum())


def body_layouts(run, arrangements, Rs=3):
    """9. params NULL, shared and per instance"""
    G = Q.generic_case(arrangements)
    P, xs, sp = G["P"], G["xs"], G["speeds"]
    B = xs.shape[0]
    shared = run(P, xs, G["params"], sp, substeps=Rs)
    per = run(P, xs, np.repeat(G["params"][None], B, axis=0), sp, substeps=Rs)
    assert same(shared, per)
    flipped = run(P, xs, np.stack([G["params"], G["params"][::-1], G["params"]]), sp, substeps=Rs)
    assert np.array_equal(flipped["edges"][1, 0], shared["edges"][1, 1]) and np.array_equal(flipped["edges"][1, 1], shared["edges"][1, 0])
    assert np.array_equal(flipped["edges"][2], shared["edges"][2]) and np.any(shared["edges"][:, 0] != shared["edges"][:, 1])
    none = run(P, xs, None, sp, substeps=Rs)
    own = run(P, xs, G["params"][:1], sp, substeps=Rs)
    assert none["duration"].shape == (B, 1) and same(none, own)
