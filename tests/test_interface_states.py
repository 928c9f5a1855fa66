"""upright_amd/csrc/upr_iface.h -- the functions through which upr_api.hip narrows and widens interface states
[robot x (nx) | r v a of every dynamic obstacle (9 n_dyn)] -- compiled by the host compiler (tests/emu/upr_emu.cpp) and held against
numpy slicing.  Two obstacles and three rows: a hard-coded 9 or a wrong row stride cannot pass.  Every output lies NaN-filled between
guard cells: every cell must be written and no guard touched.  ballistic() and assert_ballistic() are shared with
tests/test_gpu_interface_states.py."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from upright_amd._capi import ptr

EMU = Path(__file__).resolve().parent / "emu" / "libupr_emu.so"
SHAPES = [(27, 0), (27, 1), (27, 2), (18, 1)]
EPS = np.finfo(np.float64).eps
GUARD, SENTINEL = 8, -7.25e30


def ballistic(dyn, tau):
    """dyn[..., 9 n_dyn] a time tau later, in extended precision: r + tau v + tau^2 a / 2, v + tau a, a for every obstacle"""
    o = np.asarray(dyn, dtype=np.longdouble).reshape(dyn.shape[:-1] + (dyn.shape[-1] // 9, 3, 3))
    tau = np.asarray(tau, dtype=np.longdouble)[..., None, None]
    r, v, a = o[..., 0, :], o[..., 1, :], o[..., 2, :]
    return np.stack([r + tau * v + tau * tau * a / 2, v + tau * a, a], axis=-2).reshape(dyn.shape)


def assert_ballistic(out, dyn, tau):
    """out[..., 9 n_dyn] is the continuation of dyn after tau (a scalar, or one per leading index): r within 4 eps (|r| + |tau v| +
    |tau^2 a| / 2), v within 2 eps (|v| + |tau a|) -- the roundings of the two expressions -- and a bitwise; tau == 0 returns the
    input bits (finite input)."""
    assert out.shape == dyn.shape
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), dyn.shape[:-1])
    ref = ballistic(dyn, tau).reshape(dyn.shape[:-1] + (dyn.shape[-1] // 9, 3, 3))
    o = out.reshape(ref.shape)
    d = np.abs(np.asarray(dyn, dtype=np.longdouble)).reshape(ref.shape)
    t = np.abs(tau.astype(np.longdouble))[..., None, None]
    err = np.abs(o.astype(np.longdouble) - ref)
    assert np.all(err[..., 0, :] <= 4 * EPS * (d[..., 0, :] + t * d[..., 1, :] + t * t * d[..., 2, :] / 2))
    assert np.all(err[..., 1, :] <= 2 * EPS * (d[..., 1, :] + t * d[..., 2, :]))
    assert np.array_equal(o[..., 2, :].view(np.uint64), dyn.reshape(ref.shape)[..., 2, :].view(np.uint64))
    still = tau == 0.0
    if np.any(still):
        assert np.all(np.isfinite(dyn[still]))
        assert np.array_equal(out[still].view(np.uint64), dyn[still].view(np.uint64))


@pytest.fixture(scope="module")
def emu():
    E = C.CDLL(str(EMU))
    for f in ("emu_iface_split", "emu_iface_join", "emu_iface_join_zero", "emu_iface_join_ballistic"):
        getattr(E, f).restype = None
    return E


class Guarded:
    """an output array of `shape`, NaN, between guard cells"""

    def __init__(self, shape):
        self.buf = np.full(2 * GUARD + int(np.prod(shape)), SENTINEL)
        self.a = self.buf[GUARD:self.buf.size - GUARD].reshape(shape)
        self.a[...] = np.nan

    def checked(self):
        assert np.all(self.buf[:GUARD] == SENTINEL) and np.all(self.buf[self.buf.size - GUARD:] == SENTINEL), "guard cell written"
        assert not np.any(np.isnan(self.a)), "output cell not written"
        return self.a


def _states(nx, n_dyn, n, seed):
    """seeded random states: the obstacle blocks differ between the rows and between the obstacles"""
    x = np.random.default_rng(seed).uniform(-2.0, 2.0, (n, nx + 9 * n_dyn))
    if n_dyn:
        blocks = x[:, nx:].reshape(n * n_dyn, 9)
        assert len({b.tobytes() for b in blocks}) == n * n_dyn
    return x


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("nx,n_dyn", SHAPES)
def test_split_and_join(emu, nx, n_dyn, n):
    x = _states(nx, n_dyn, n, 100 * nx + 10 * n_dyn + n)
    xr, dyn = Guarded((n, nx)), Guarded((n, 9 * n_dyn))
    emu.emu_iface_split(nx, n_dyn, ptr(x), n, ptr(xr.a), ptr(dyn.a))
    assert np.array_equal(xr.checked(), x[:, :nx]) and np.array_equal(dyn.checked(), x[:, nx:])
    only = Guarded((n, nx))                                   # no obstacle destination: the robot block alone
    emu.emu_iface_split(nx, n_dyn, ptr(x), n, ptr(only.a), None)
    assert np.array_equal(only.checked(), x[:, :nx])
    back = Guarded(x.shape)                                   # the inverse
    emu.emu_iface_join(nx, n_dyn, ptr(np.ascontiguousarray(x[:, :nx])), ptr(np.ascontiguousarray(x[:, nx:])), n, ptr(back.a))
    assert np.array_equal(back.checked().view(np.uint64), x.view(np.uint64))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("nx,n_dyn", SHAPES)
def test_join_zero(emu, nx, n_dyn, n):
    xr = np.random.default_rng(7 * nx + n_dyn + n).uniform(-2.0, 2.0, (n, nx))
    out = Guarded((n, nx + 9 * n_dyn))
    emu.emu_iface_join_zero(nx, n_dyn, ptr(xr), n, ptr(out.a))
    want = np.concatenate([xr, np.zeros((n, 9 * n_dyn))], axis=1)
    assert np.array_equal(out.checked(), want) and not np.any(np.signbit(out.a[:, nx:]))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("nx,n_dyn", SHAPES)
def test_join_ballistic(emu, nx, n_dyn, n):
    x = _states(nx, n_dyn, n, 1000 + 100 * nx + 10 * n_dyn + n)
    xr, dyn = np.ascontiguousarray(x[:, :nx]), np.ascontiguousarray(x[:, nx:])
    for tau in (0.0, 0.05, 1.0 / 3.0, 1.7):
        out = Guarded(x.shape)
        for i in range(n):   # (one state per call, as upr_api.hip calls it)
            emu.emu_iface_join_ballistic(nx, n_dyn, ptr(xr[i]), ptr(dyn[i]), C.c_double(tau), ptr(out.a[i]))
        o = out.checked()
        assert np.array_equal(o[:, :nx], xr)
        assert_ballistic(np.ascontiguousarray(o[:, nx:]), dyn, tau)
        if n_dyn and tau:
            assert not np.array_equal(o[:, nx:nx + 6], dyn[:, :6])   # (the continuation moved something)
