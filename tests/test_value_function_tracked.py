"""CPU tests of the equality multipliers in the value-function kernels (upright_amd/csrc/upr_value.h) through the test-only host
emulation tests/emu/upr_vf_nu_emu.cpp (one thread per workgroup): the copy of the QP's nu that upr_vf_instance keeps
(upr_vf_args::nu_out), and nu(t) of upr_vf_query_point against the host module's ValueFunction.equality_multiplier, which is its
specification.  The execution on the GPU, tracked mode included, is checked by tests/test_gpu_value_function_tracked.py."""
import ctypes as C
import os
from pathlib import Path

import numpy as np
import pytest

from test_emu import Emu
from test_value_function_batched import _ctg_cases, _export
from upright_amd import _capi
from upright_amd.value_function import ValueFunction

NU_EMU = Path(os.environ.get("UPR_VF_NU_EMU_LIB", str(Path(__file__).resolve().parent / "emu" / "libupr_vf_nu_emu.so")))
p = _capi.ptr
ip = _capi.iptr

_CACHE = {}


def _case(arrangements, name):
    """One emulated QP per instance of the case (headline: ne = 6, B = 2; robust: ne = 48, more rows than half a wave, B = 1) and the
    emulated cost-to-go kernel on it with the multiplier copy.  Computed once per case and shared; nothing modifies it."""
    if name not in _CACHE:
        P, x0, way, xs, us, kernel = _ctg_cases(arrangements, name)
        B = x0.shape[0]
        e = Emu(P, B)
        lin = e.linearize(way, np.zeros(B), xs, us)
        sols, pairs, stats, (ws, mult, offs) = _export(e, kernel, xs, us, x0, lin)
        assert np.all(stats[:, 2] == 0)
        n1, nx = P.N + 1, e.nx
        out = dict(Pk=np.full((B, n1, nx, nx), np.nan), pk=np.full((B, n1, nx), np.nan), J=np.full((B, n1), np.nan), X=np.full((B, n1, nx), np.nan),
                   nu=np.full((B, P.N, e.ne), np.nan))   # (device memory is not zero: every entry must be written)
        C.CDLL(str(NU_EMU)).emu_vfnu_cost_to_go(C.byref(e.cp), B, p(xs), p(us), p(lin), p(e.Df), p(ws), C.c_long(ws.shape[1]), p(mult), C.c_long(mult.shape[1]),
                                                ip(offs), p(out["Pk"]), p(out["pk"]), p(out["J"]), p(out["X"]), p(out["nu"]))
        _CACHE[name] = (P, e, sols, out)
    return _CACHE[name]


@pytest.mark.parametrize("name", ["headline", "robust"])
def test_cost_to_go_kernel_source_copies_the_multipliers(arrangements, name):
    """upr_vf_instance writes nu_out[b][k][r] = the QP's nu, exactly, for every instance, knot and row; the other outputs are written
    as without the copy (finite everywhere)."""
    P, e, sols, out = _case(arrangements, name)
    assert e.ne == (6 if name == "headline" else 48)
    for b in range(e.B):
        assert np.array_equal(out["nu"][b], sols[b]["nu"])
        assert np.abs(sols[b]["nu"]).max() > 0
    assert all(np.all(np.isfinite(v)) for v in out.values())


def _host_vf(P, t0, nu):
    """ValueFunction with the two members equality_multiplier reads (its constructor needs a solved handle)."""
    vf = ValueFunction.__new__(ValueFunction)
    vf.P, vf.t, vf.nu = P, t0 + P.dt * np.arange(P.N + 1), nu
    return vf


@pytest.mark.parametrize("name", ["headline", "robust"])
def test_query_kernel_source_multipliers_against_the_host_module(arrangements, name):
    """upr_vf_query_point's nu(t) against ValueFunction.equality_multiplier on the same nu: before the plan, inside it, exactly on a
    knot (the first, an inner one, the last two), in the last interval and past the horizon.  The same two products and one sum per
    row on both sides: 1e-15 relative to the largest multiplier of the point."""
    P, e, sols, out = _case(arrangements, name)
    B, N, h = e.B, P.N, P.dt
    t0 = np.array([0.25, -1.0])[:B]
    rel = np.array([-0.3, 0.0, 0.37 * h, 3.0 * h, 7.5 * h, (N - 1) * h, (N - 0.4) * h, N * h, N * h + 0.2])
    inst = np.repeat(np.arange(B), len(rel)).astype(np.int32)
    t = np.ascontiguousarray(t0[inst] + np.tile(rel, B))
    n = len(t)
    got = np.full((n, e.ne), np.nan)
    C.CDLL(str(NU_EMU)).emu_vfnu_query(C.byref(e.cp), n, ip(inst), p(t), p(t0), p(out["nu"]), p(got))
    vfs = [_host_vf(P, t0[b], out["nu"][b]) for b in range(B)]
    worst = 0.0
    for i in range(n):
        want = vfs[inst[i]].equality_multiplier(t[i])
        worst = max(worst, np.abs(got[i] - want).max() / np.abs(want).max())
    print("nu(t) of the query kernel source vs the host module, %s: %.2e relative" % (name, worst))
    assert worst <= 1e-15, worst
    # the ends: clamped to knot 0 before the plan; everything past the horizon holds nu[N - 1] (as does the last interval, to rounding)
    for b in range(B):
        o = b * len(rel)
        assert np.array_equal(got[o], out["nu"][b, 0]) and np.array_equal(got[o + 1], out["nu"][b, 0])
        assert np.array_equal(got[o + 8], out["nu"][b, N - 1])


def test_qp_kernel_device_text_equals_the_parents():
    """Tracked mode does not touch the QP kernel: the gfx950 .text of every upr_qp3 part the build just compiled (tools/text_hash.py on
    upright_amd/csrc/build) is byte-identical to the parent commit's, recorded in tests/golden/value_function_tracked_parent.json.
    The hash depends on the compiler as well as on the source; the file names the one it was recorded with and says when to record
    it anew."""
    import json
    import sys

    root = Path(__file__).resolve().parents[1]
    sys.path.insert(0, str(root / "tools"))
    from text_hash import text_hash

    gold = json.load(open(root / "tests" / "golden" / "value_function_tracked_parent.json"))["text_hash"]
    objs = sorted((root / "upright_amd" / "csrc" / "build").glob("upr_qp3_part*.o"))
    assert [o.name for o in objs] == sorted(gold), ([o.name for o in objs], sorted(gold))
    for o in objs:
        h, n = text_hash(o)
        assert (n, h) == (gold[o.name]["bytes"], gold[o.name]["sha256_16"]), (o.name, n, h, gold[o.name])
