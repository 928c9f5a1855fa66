"""CPU reference of the retiming with a reserve (upright_amd/csrc/upr_retime_rsv.h) and the assertions its CPU and GPU tests share.  The
plans, the lattice, the boxes and the programme are retime_ref's, the displacement is disturb_ref's; neither module is changed.

The reference decision of a RECORD of an end state (knot k at speed s and path acceleration d, scenario sc) is balance_ref.reference at
the joint-space state disturb_ref.displaced(P, retime_ref.state_at(x_k, s, d, nq), u_world, +-r), u_world the direction rotated in
numpy by the oracle's C_we of the knot (tray frame) -- accepted when rho_ref <= EPS max(|b|, 1), DECIDED when |rho_ref - EPS max(|b|, 1)|
> RHO_TOL max(|b|, 1).  The records of an end state come in the kernel's order: the nominal one (retime_ref's own decision, taken from
its case where it is there), then k ascending, +r before -r, and the end state stops at its first rejection.  An end state is decided
when every record the kernel would evaluate is; an edge when its departing state is and, if that is accepted, its arriving state.

run(P, xs, params, speeds, dirs=None, reserve=None, frame="tray", start=-1, end=-1, common=False, boxes=True, form=-1, fma=False) ->
dict(duration, level, reach, edges, iters) is what a test file hands to the bodies below; reserve=None is the plain retiming."""
import ctypes as C
import os
import time
from pathlib import Path

import numpy as np

import balance_ref as R
import disturb_ref as D
import retime_ref as Q
from oracle.oracle import Oracle

EPS, RHO_TOL = Q.EPS, Q.RHO_TOL
RESERVE = 0.25                      # m/s^2, the generic case; the slide case takes 0.25 mu0 g0
LADDER = (0.0, 0.25, 0.5, 1.0)      # the reserves of the monotonicity check


def tray3(P):
    """(3, 6): (0, span_0), (0, span_1), (0, e_z) of contact 0, tray frame"""
    return D.tray_dirs(P)[:3]


def ref_masks(P, xs, params, speeds, boxes, dirs, frame, r, nominal=None):
    """retime_ref.ref_masks with the end states judged record by record: dict(masks, decided, ends {(b, sc, knot, s, d): (accepted,
    decided)}, box_margin, records: the reference evaluations made).  nominal: evaluations {(b, sc, knot, s, d): (accepted, decided)}
    of the nominal records to take instead of computing them (retime_ref.ref_masks' `evals` on the same plans and scenarios)."""
    xs = np.asarray(xs)
    speeds = np.asarray(speeds, dtype=np.float64)
    params = np.asarray(params, dtype=np.float64).reshape(-1, P.nb, 10)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 6)
    B, nk, ns, M, h, nq = xs.shape[0], xs.shape[1], params.shape[0], speeds.size, float(P.dt), P.nq
    N = nk - 1
    O = Oracle(P)
    masks = np.zeros((B, ns, N, M), dtype=np.uint32)
    decided = np.ones((B, ns, N, M, M), dtype=bool)
    ends, bm, count = {}, np.inf, [0]
    uw = {}

    def world(b, k):
        if (b, k) not in uw:
            Cm = D.ee_of(O, xs[b, k])[0]
            uw[b, k] = np.concatenate([dirs[:, :3] @ Cm.T, dirs[:, 3:] @ Cm.T], axis=1) if frame == "tray" else dirs
        return uw[b, k]

    def record(x, sc):
        count[0] += 1
        out = R.reference(P, x[None], params[sc:sc + 1], False)
        rho, scale = float(out["rho"][0, 0]), max(float(out["bnorm"][0, 0]), 1.0)
        return rho <= EPS * scale, abs(rho - EPS * scale) > RHO_TOL * scale

    def judge(b, sc, k, s, d):
        key = (b, sc, k, float(s), float(d))
        if key not in ends:
            x = Q.state_at(xs[b, k], s, d, nq)
            ok, dec = nominal[key] if nominal is not None and key in nominal else record(x, sc)
            if ok and dec and r > 0.0:
                for u in world(b, k):
                    for sign in (1.0, -1.0):
                        if ok and dec:
                            ok, dec = record(D.displaced(P, x, u, sign * r), sc)
            ends[key] = (ok, dec)
        return ends[key]

    for b in range(B):
        for i in range(N):
            for m in range(M):
                for mp in range(M):
                    s0, s1 = speeds[m], speeds[mp]
                    if not s0 + s1 > 0.0:
                        continue
                    d = Q.accel(s0, s1, h)
                    if boxes:
                        g0, g1 = Q.box_margin(P, xs[b, i], s0, d), Q.box_margin(P, xs[b, i + 1], s1, d)
                        bm = min(bm, abs(g0), abs(g1))
                        if g0 < 0.0 or g1 < 0.0:
                            continue
                    for sc in range(ns):
                        ok, dec = judge(b, sc, i, s0, d)
                        if ok and dec:
                            ok, dec = judge(b, sc, i + 1, s1, d)
                        decided[b, sc, i, m, mp] = dec
                        if ok:
                            masks[b, sc, i, m] |= np.uint32(1) << np.uint32(mp)
    return dict(masks=masks, decided=decided, ends=ends, box_margin=bm, records=count[0])


# ---- the kernel source through the host emulation -----------------------------------------------------------------------------------
def emu_lib(fma=False):
    name = "libupr_retime_rsv_emu_fma.so" if fma else "libupr_retime_rsv_emu.so"
    return C.CDLL(os.environ.get("UPR_RETIME_RSV_EMU_FMA_LIB" if fma else "UPR_RETIME_RSV_EMU_LIB", str(Path(__file__).resolve().parent / "emu" / name)))


def have_fma_twin():
    try:
        has_fma = " fma " in Path("/proc/cpuinfo").read_text().replace("\n", " ")
    except OSError:
        has_fma = False
    if has_fma:
        assert (Path(__file__).resolve().parent / "emu" / "libupr_retime_rsv_emu_fma.so").exists(), "the host has FMA but libupr_retime_rsv_emu_fma.so was not built"
    return has_fma


def run_emu(P, xs, params, speeds, dirs=None, reserve=None, frame="tray", start=-1, end=-1, common=False, boxes=True, form=-1, fma=False):
    """emu_ret_rsv_plan; reserve=None: retime_ref.run_emu, the plain retiming's emulation"""
    from upright_amd import _capi

    if reserve is None:
        return Q.run_emu(P, xs, params, speeds, start, end, common, boxes, form, fma)
    xs = np.ascontiguousarray(xs, dtype=np.float64)
    B, nk = xs.shape[:2]
    params = np.ascontiguousarray(params, dtype=np.float64)
    per = params.ndim == 4
    ns = params.shape[1] if per else params.reshape(-1, P.nb, 10).shape[0]
    speeds = np.ascontiguousarray(speeds, dtype=np.float64)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 6)
    M = speeds.size
    lead = (B,) if common else (B, ns)
    out = dict(duration=np.full(lead, np.nan), level=np.full(lead + (nk,), -9, dtype=np.int32), reach=np.full(lead + (2,), -9, dtype=np.int32),
               edges=np.zeros((B, ns, nk - 1, M), dtype=np.uint32), iters=np.full((B, ns, nk - 1, M), -1, dtype=np.int32))
    cp = _capi.problem_to_c(P)
    rc = emu_lib(fma).emu_ret_rsv_plan(C.byref(cp), B, nk, _capi.ptr(xs), ns, _capi.ptr(params), nk if per else 0, M, _capi.ptr(speeds), int(start), int(end),
                                       int(common), int(boxes), dirs.shape[0], _capi.ptr(dirs), D.FRAMES[frame], C.c_double(reserve),
                                       _capi.ptr(out["duration"]), _capi.iptr(out["level"]), _capi.iptr(out["reach"]),
                                       out["edges"].ctypes.data_as(C.POINTER(C.c_uint)), _capi.iptr(out["iters"]), int(form))
    assert rc == 0
    return out


def run_device(mpc, xs, params, speeds, dirs=None, reserve=None, frame="tray", start=None, end=None, common=False, boxes=True):
    """The same through BatchMPC.retime_plan on the plan xs installed with set_guess"""
    mpc.set_guess(xs, np.zeros((mpc.B, mpc.N, mpc.nu)))
    dur, level, reach, edges, iters = mpc.retime_plan(speeds, params, start=start, end=end, common=common, boxes=boxes, want_reach=True, want_edges=True,
                                                      want_iters=True, reserve=reserve, dirs=dirs, frame=frame)
    return dict(duration=dur, level=level, reach=reach, edges=edges, iters=iters)


# ---- the cases the CPU and the GPU tests share (built once per process) -------------------------------------------------------------
_CASES = {}


def slide_case(arrangements):
    """retime_ref.slide_case with the reserve r = 0.25 mu0 g0 and, per direction of tray3, the closed form of an end state's margin --
    lateral (span_0, span_1: the pyramid is the L1 one) mu0 g0 - r - |s^2 c_k + d w_k|, vertical (e_z) mu0 (g0 - r) - |s^2 c_k + d w_k| --
    the masks on it and `near`, the smallest |margin| over the decisions"""
    if "slide" not in _CASES:
        S = dict(Q.slide_case(arrangements))
        P, c, w, speeds, h = S["P"], S["c"], S["w"], S["speeds"], float(S["P"].dt)
        mu0 = float(P.contact_mu[0])
        r = 0.25 * S["bound"]
        lateral = lambda b, k, s, d: S["bound"] - r - abs(s * s * c[k] + d * w[k])   # noqa: E731
        vertical = lambda b, k, s, d: mu0 * (R.G0 - r) - abs(s * s * c[k] + d * w[k])   # noqa: E731
        S["r"], S["dirs"], S["closed"], S["refs"], S["nears"] = r, tray3(P), [lateral, lateral, vertical], [], []
        for f in S["closed"]:
            S["refs"].append(Q.ref_masks(P, S["xs"], S["params"], speeds, False, closed=f))
            S["nears"].append(min(abs(f(0, k, s0 if e == 0 else s1, Q.accel(s0, s1, h))) for i in range(P.N) for s0 in speeds for s1 in speeds if s0 + s1 > 0
                                  for e, k in ((0, i), (1, i + 1))))
        _CASES["slide"] = S
    return _CASES["slide"]


def generic_case(arrangements, name="pink_bottle", B=3, plans=2, speeds=Q.GENERIC["speeds"], n_dir=3, r=RESERVE):
    """retime_ref.generic_case and the reference with the reserve r along the first n_dir directions of tray3 on its first `plans`
    plans (key "rsv"; the nominal records are those of retime_ref's reference)"""
    key = ("generic", name, B, plans, tuple(speeds), n_dir, r)
    if key not in _CASES:
        G = dict(Q.generic_case(arrangements, name, B, speeds))
        t0 = time.time()
        G["dirs"], G["r"], G["plans"] = tray3(G["P"])[:n_dir], r, plans
        G["rsv"] = ref_masks(G["P"], G["xs"][:plans], G["params"], G["speeds"], True, G["dirs"], "tray", r, nominal=G["ref"]["evals"])
        print("retime with a reserve, %s: the reference of %d plans took %.1f s (%d records beyond the nominal ones)"
              % (name, plans, time.time() - t0, G["rsv"]["records"]))
        _CASES[key] = G
    return _CASES[key]


def first_plans(out, n):
    return {k: (v[:n] if v is not None else None) for k, v in out.items()}


# ---- the assertions both test files make ----------------------------------------------------------------------------------------------
def body_closed_form(run, arrangements):
    """1."""
    S = slide_case(arrangements)
    P, speeds, h = S["P"], S["speeds"], float(S["P"].dt)
    print("retime with a reserve, slide: the closest closed-form decisions lie %s mu0 g0 from their bounds (span_0, span_1, e_z)"
          % ", ".join("%.2e" % (n / S["bound"]) for n in S["nears"]))
    assert all(n >= 1e-6 * S["bound"] for n in S["nears"])     # (on the closed form alone, before any answer is looked at)
    want0 = Q.programme(S["refs"][0]["masks"][0, 0], speeds, h)
    want2 = Q.programme(S["refs"][2]["masks"][0, 0], speeds, h)
    assert abs(want0["duration"] - 2.351804) < 1e-6 and abs(want2["duration"] - 1.856566) < 1e-6, (want0, want2)
    assert want0["level"].tolist() == [5, 4, 3, 3] + [2] * 13 + [3, 3, 4, 5], want0["level"]
    plain = run(P, S["xs"], S["params"], speeds, boxes=False)
    outs = []
    for k in range(3):
        out = run(P, S["xs"], S["params"], speeds, dirs=S["dirs"][k:k + 1], reserve=S["r"], boxes=False)
        ref = S["refs"][k]
        assert np.array_equal(out["edges"], ref["masks"]), k
        for b in range(S["xs"].shape[0]):
            want = Q.programme(ref["masks"][b, 0], speeds, h)
            dur = float(out["duration"][b, 0])
            assert abs(dur - want["duration"]) <= 1e-12 * want["duration"], (k, b, dur, want["duration"])
            assert np.array_equal(out["level"][b, 0], want["level"]), (k, b, out["level"][b, 0], want["level"])
        Q.check_invariants(out, speeds, h)
        outs.append(out)
    assert np.array_equal(outs[0]["edges"], outs[1]["edges"])
    assert np.all(outs[0]["duration"] > plain["duration"])
    assert np.array_equal(outs[2]["duration"], plain["duration"])    # (a vertical reserve of that size does not bind the law)
    print("retime with a reserve, slide: durations plain %.6f, span_0 %.6f, e_z %.6f; levels with span_0 %s"
          % (plain["duration"][0, 0], outs[0]["duration"][0, 0], outs[2]["duration"][0, 0], outs[0]["level"][0, 0].tolist()))
    return outs


def body_reference(run, arrangements, name="pink_bottle", B=3, plans=2, speeds=Q.GENERIC["speeds"], n_dir=3, r=RESERVE, **kw):
    """2. (and 8. on another shape or form)"""
    G = generic_case(arrangements, name, B, plans, speeds, n_dir, r)
    ref = G["rsv"]
    share = Q.undecided_share(ref)
    assert share <= 0.10, share                               # (conditions on the reference alone, before any answer is looked at)
    assert ref["box_margin"] >= 1e-9, ref["box_margin"]
    out = run(G["P"], G["xs"], G["params"], G["speeds"], dirs=G["dirs"], reserve=r, **kw)
    h = float(G["P"].dt)
    n_dec, n_lvl = Q.against_reference(first_plans(out, plans), ref, G["speeds"], h)
    Q.check_invariants(out, G["speeds"], h)
    print("retime with a reserve, %s: undecided edges %.3f of %d, box margin %.1e, decided plans %d of %d, levels compared on %d; durations %s"
          % (name, share, ref["decided"].size, ref["box_margin"], n_dec, plans * 2, n_lvl, np.round(out["duration"][:plans].ravel(), 4).tolist()))
    assert n_dec >= 1 and n_lvl >= 1
    return out


def body_zero_reserve(run, arrangements, forms=(-1, 0)):
    """3."""
    G, S = Q.generic_case(arrangements), Q.slide_case(arrangements)
    n = 0
    for form in forms:
        for P, xs, params, speeds, dirs, kw in ((G["P"], G["xs"], G["params"], G["speeds"], tray3(G["P"]), dict()),
                                                (S["P"], S["xs"], S["params"], S["speeds"], tray3(S["P"])[2:], dict(boxes=False)),
                                                (S["P"], S["xs"], S["params"], S["speeds"], tray3(S["P"])[:1], dict(frame="world", start=0, end=0))):
            plain = run(P, xs, params, speeds, form=form, **{k: v for k, v in kw.items() if k != "frame"})
            zero = run(P, xs, params, speeds, dirs=dirs, reserve=0.0, form=form, **kw)
            assert all(np.array_equal(plain[k], zero[k]) for k in ("duration", "level", "reach", "edges", "iters")), (form, kw)
            n += 1
    return n


def body_monotone(run, arrangements):
    """4."""
    G = Q.generic_case(arrangements)
    P, dirs = G["P"], tray3(G["P"])
    outs = [run(P, G["xs"], G["params"], G["speeds"], dirs=dirs, reserve=r) for r in LADDER]
    plain = run(P, G["xs"], G["params"], G["speeds"])
    assert np.array_equal(outs[0]["edges"], plain["edges"])
    for a, b in zip(outs[:-1], outs[1:]):
        assert not np.any(b["edges"] & ~a["edges"])
        assert np.all(b["duration"] >= a["duration"])
    assert np.any(outs[1]["edges"] != outs[0]["edges"]) and np.any(outs[3]["edges"] != outs[1]["edges"])
    for sub in ([0], [2], [0, 1], [1, 2]):
        part = run(P, G["xs"], G["params"], G["speeds"], dirs=dirs[sub], reserve=RESERVE)
        assert not np.any(outs[1]["edges"] & ~part["edges"]), sub
    print("retime with a reserve, generic: durations over the reserves %s: %s" % (LADDER, [np.round(o["duration"].ravel(), 4).tolist() for o in outs]))


def body_keeps_reserve(run, arrangements, margin):
    """5. margin(P, x (n, 3 nq), theta (nb, 10), dirs) -> (n_dir, n, 2) = (r_lo, r_hi) at r_max = 8"""
    G = generic_case(arrangements)
    P, h, nq, r, ref, plans = G["P"], float(G["P"].dt), G["P"].nq, G["r"], G["rsv"], G["plans"]
    law = first_plans(run(P, G["xs"], G["params"], G["speeds"], dirs=G["dirs"], reserve=r), plans)
    plain = first_plans(run(P, G["xs"], G["params"], G["speeds"]), plans)
    n_dec = n_short = 0
    for out, reserved in ((law, True), (plain, False)):
        _, dep, arr = Q.retimed_states(G["xs"][:plans], out["level"], G["speeds"], h, nq)
        for b, sc in np.argwhere(np.isfinite(out["duration"])):
            s = G["speeds"][out["level"][b, sc]]
            d = Q.accel(s[:-1], s[1:], h)
            x = np.concatenate([dep[b, sc], arr[b, sc]])
            win = margin(P, x, G["params"][sc], G["dirs"])
            assert win.shape == (len(G["dirs"]), x.shape[0], 2)
            keeps = (win[..., 0] <= -0.999 * r) & (win[..., 1] >= 0.999 * r)
            if not reserved:
                n_short += int((~keeps).any(axis=0).sum())
                continue
            keys = [(b, sc, i, float(s[i]), float(d[i])) for i in range(P.N)] + [(b, sc, i + 1, float(s[i + 1]), float(d[i])) for i in range(P.N)]
            dec = np.array([ref["ends"][k][1] for k in keys])
            assert all(ref["ends"][k][0] for k, ok in zip(keys, dec) if ok)
            assert keeps[:, dec].all(), (b, sc, win[:, dec][~keeps[:, dec]])
            n_dec += int(dec.sum())
    print("retime with a reserve, generic: %d decided states of the laws keep +-%.2f along every direction; %d states of the plain laws do not" % (n_dec, r, n_short))
    assert n_dec >= 40 and n_short >= 1


def body_frames_and_order(run, arrangements):
    """6."""
    S = slide_case(arrangements)
    P, xs, par, speeds, r = S["P"], S["xs"][:1], S["params"], S["speeds"], S["r"]
    dirs = S["dirs"]
    tray = run(P, xs, par, speeds, dirs=dirs, reserve=r, boxes=False)
    world = run(P, xs, par, speeds, dirs=D.world_dirs(P, xs[0, 0], dirs)[0], reserve=r, frame="world", boxes=False)
    assert np.array_equal(tray["edges"], world["edges"]) and np.array_equal(tray["duration"], world["duration"])
    assert np.array_equal(tray["edges"], S["refs"][0]["masks"][:1] & S["refs"][2]["masks"][:1])
    G = Q.generic_case(arrangements)
    gd = tray3(G["P"])
    u = gd[:1] + 0.5 * gd[2:]
    one = run(G["P"], G["xs"], G["params"], G["speeds"], dirs=u, reserve=RESERVE)
    both = run(G["P"], G["xs"], G["params"], G["speeds"], dirs=np.concatenate([u, -u]), reserve=RESERVE)
    assert np.array_equal(one["edges"], both["edges"]) and np.all(both["iters"] >= one["iters"]) and np.any(both["iters"] > one["iters"])
    a = run(G["P"], G["xs"], G["params"], G["speeds"], dirs=gd, reserve=RESERVE)
    b = run(G["P"], G["xs"], G["params"], G["speeds"], dirs=gd[[2, 0, 1]], reserve=RESERVE)
    assert np.array_equal(a["edges"], b["edges"]) and np.array_equal(a["duration"], b["duration"]) and np.array_equal(a["level"], b["level"])


def body_shapes(run, arrangements):
    """7."""
    G, S = Q.generic_case(arrangements), slide_case(arrangements)
    P, h, gd = G["P"], float(G["P"].dt), tray3(G["P"])
    for params in (Q.shifted(P), Q.with_vertex(P)):
        one = run(P, G["xs"], params, G["speeds"], dirs=gd, reserve=RESERVE, common=True)
        each = run(P, G["xs"], params, G["speeds"], dirs=gd, reserve=RESERVE)
        assert np.array_equal(one["edges"], each["edges"]) and one["duration"].shape == (G["xs"].shape[0],)
        Q.check_invariants(one, G["speeds"], h, common=True)
        Q.check_invariants(each, G["speeds"], h)
        assert np.all(one["duration"] >= each["duration"].max(axis=1))
    sp0 = np.array((0.0,) + Q.GENERIC["speeds"])
    out = run(P, G["xs"], Q.shifted(P), sp0, dirs=gd, reserve=RESERVE, start=2, end=0)
    Q.check_invariants(out, sp0, h, 2, 0)
    xs, par, r, sd = S["xs"][:1], S["params"], S["r"], S["dirs"]
    given = run(S["P"], xs, par, S["speeds"], dirs=sd[:1], reserve=r, start=0, end=0, boxes=False)
    Q.check_invariants(given, S["speeds"], h, 0, 0)
    assert np.isfinite(given["duration"][0, 0]) and given["level"][0, 0, 0] == 0 and given["level"][0, 0, -1] == 0
    sp32 = np.linspace(0.1, 1.2, 32)
    out = run(S["P"], xs, par, sp32, dirs=sd[:1], reserve=r, boxes=False)
    assert out["edges"].shape == (1, 1, S["P"].N, 32) and np.any(out["edges"] >> np.uint32(31)) and np.any(out["edges"] == 0)
    Q.check_invariants(out, sp32, h)
    assert np.isfinite(out["duration"][0, 0])
    for s, feasible in ((0.75, True), (1.0, False)):          # (|c| peaks at 0.8 mu0 g0: with the reserve 0.25 mu0 g0 speed 1 is cut)
        out = run(S["P"], xs, par, np.array([s]), dirs=sd[:1], reserve=r, boxes=False)
        Q.check_invariants(out, np.array([s]), h)
        assert np.isfinite(out["duration"][0, 0]) == feasible, (s, out["duration"])
    once = run(S["P"], xs, par, S["speeds"], dirs=sd[:1], reserve=r, boxes=False)
    many = run(S["P"], xs, par, S["speeds"], dirs=np.repeat(sd[:1], 32, axis=0), reserve=r, boxes=False)
    assert np.array_equal(once["edges"], many["edges"]) and np.array_equal(once["duration"], many["duration"])
    assert np.array_equal(once["edges"], S["refs"][0]["masks"][:1]) and many["iters"].max() > once["iters"].max()
