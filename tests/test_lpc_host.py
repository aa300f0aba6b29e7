"""Levinson-Durbin, the Toeplitz solver and the LPC handle's argument checks, on the CPU: llz_levinson, llz_levinson1 and
llz_atlvs run on the host and must equal the reference's own results (tests/golden/lpc.npz, written by
tools/gen_golden_lpc.py) bit for bit.  levinson_py is an independent restatement in Python floats (IEEE double, no fused
multiply-add); the GPU tests use it as the reference of the batch path."""
import math
import os

import numpy as np
import pytest

from llzlab_amd import capi, filters

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ORDERS = (1, 2, 8, 10, 16, 32, 64)


def _div(a, b):
    """a / b with IEEE semantics where Python would raise"""
    if b != 0.0:
        return a / b
    if a == 0.0 or math.isnan(a):
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def levinson_py(r, p):
    """llz_levinson's recursion (acof[0..p], kcof[0..p-1], err) for r[0] != 0; silent r gives the batch path's outputs"""
    r = [float(v) for v in r]
    a = [1.0] + [0.0] * p
    k_out = [0.0] * p
    if r[0] == 0.0:
        return a, k_out, 0.0
    e = r[0]
    for i in range(1, p + 1):
        acc = r[i]
        for j in range(1, i):
            acc = acc + a[j] * r[i - j]
        k = _div(-acc, e)
        k_out[i - 1] = k
        old = a[:]
        for j in range(1, i):
            a[j] = a[j] + k * old[i - j]
        a[i] = k
        e = e * (1.0 - k * k)
    return a, k_out, e


@pytest.fixture(scope="module")
def gold():
    capi.build()
    return np.load(os.path.join(G, "lpc.npz"), allow_pickle=False)


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


@pytest.mark.parametrize("p", ORDERS)
@pytest.mark.parametrize("kind", ["rand", "ill"])
def test_levinson_bit_exact(gold, kind, p):
    key = f"{kind}_{p}"
    r = gold["r_" + key]
    for tag, fn in (("lev", filters.levinson), ("lev1", filters.levinson1)):
        acof, kcof, err = fn(r, p)
        assert _same(acof, gold[f"{tag}_acof_{key}"]), tag
        assert _same(kcof, gold[f"{tag}_kcof_{key}"]), tag
        assert _same([err], gold[f"{tag}_err_{key}"]), tag
    # llz_levinson1 is llz_levinson with the coefficients negated (same reflection coefficients)
    a0 = gold[f"lev_acof_{key}"]
    a1 = gold[f"lev1_acof_{key}"]
    assert np.allclose(a1[1:], -a0[1:], rtol=1e-6, atol=1e-9 * np.abs(a0).max())
    x, kcof, err, rc = filters.atlvs(r[:p], gold[f"atl_b_{key}"]) if p > 0 else (None, None, None, None)
    assert rc == gold[f"atl_rc_{key}"][0]
    assert _same(x, gold[f"atl_x_{key}"]) and _same(kcof, gold[f"atl_kcof_{key}"])
    if rc == 0:
        assert _same([err], gold[f"atl_err_{key}"])


@pytest.mark.parametrize("p", ORDERS)
@pytest.mark.parametrize("kind", ["rand", "ill"])
def test_python_restatement_matches_reference(gold, kind, p):
    key = f"{kind}_{p}"
    a, k, e = levinson_py(gold["r_" + key], p)
    assert _same(a, gold[f"lev_acof_{key}"])
    assert _same(k, gold[f"lev_kcof_{key}"][:p])
    assert _same([e], gold[f"lev_err_{key}"])


def test_levinson_silent_frame_quirks(gold):
    acof, kcof, err = filters.levinson(np.zeros(11), 10)
    assert _same(acof, gold["lev_silent_acof"]) and _same(kcof, gold["lev_silent_kcof"])
    assert err == gold["lev_silent_err"][0] == 0.0
    # acof[0] and kcof[0] are not written: sentinels survive
    L = capi.lib()
    r, acof, kcof, err = np.zeros(5), np.full(5, 7.0), np.full(5, 9.0), np.full(1, 3.0)
    L.llz_levinson(r.ctypes.data_as(filters._dp), 4, acof.ctypes.data_as(filters._dp), kcof.ctypes.data_as(filters._dp),
                   err.ctypes.data_as(filters._dp))
    assert acof[0] == 7.0 and kcof[0] == 9.0 and not acof[1:].any() and not kcof[1:].any() and err[0] == 0.0


def test_levinson1_defined_error():
    """the reference reads an uninitialised error for r[0] == 0 and for p == 0; here it is 0 and r[0]"""
    assert filters.levinson1(np.zeros(4), 3)[2] == 0.0
    assert filters.levinson1(np.array([2.5, 1.0]), 0)[2] == 2.5
    assert filters.levinson(np.array([2.5, 1.0]), 0)[2] == 2.5


@pytest.mark.parametrize("name", ["const", "tiny"])
def test_atlvs_singular(gold, name):
    x, kcof, err, rc = filters.atlvs(gold[f"sing_r_{name}"], gold[f"sing_b_{name}"])
    assert rc == gold[f"sing_rc_{name}"][0] == -1
    assert _same(x, gold[f"sing_x_{name}"]) and _same(kcof, gold[f"sing_kcof_{name}"])


def test_order_above_64_refused(gold):
    L = capi.lib()
    dp = filters._dp
    with pytest.raises(capi.LlzError, match="order 65"):
        filters.levinson(np.ones(66), 65)
    with pytest.raises(capi.LlzError, match="p=65"):
        filters.Lpc(65)
    assert L.llz_lpc_init(65) == capi.BAD_HANDLE
    assert "p=65" in capi.last_error()
    assert L.llz_lpc_init(-1) == capi.BAD_HANDLE
    # the C entry points themselves: message, outputs untouched
    r = np.ones(66)
    acof, kcof, err = np.full(66, 5.0), np.full(66, 6.0), np.full(1, 4.0)
    for fn in ("llz_levinson", "llz_levinson1"):
        getattr(L, fn)(r.ctypes.data_as(dp), 65, acof.ctypes.data_as(dp), kcof.ctypes.data_as(dp), err.ctypes.data_as(dp))
        assert fn in capi.last_error() and "p=65" in capi.last_error()
        assert (acof == 5.0).all() and (kcof == 6.0).all() and err[0] == 4.0
    b, x = np.ones(65), np.full(65, 2.0)
    assert L.llz_atlvs(r.ctypes.data_as(dp), 65, b.ctypes.data_as(dp), x.ctypes.data_as(dp), kcof.ctypes.data_as(dp),
                       err.ctypes.data_as(dp)) == -1
    assert "llz_atlvs" in capi.last_error() and (x == 2.0).all() and err[0] == 4.0
    # llz_lpc on a bad handle / empty frame: 0.0, outputs untouched
    assert L.llz_lpc(capi.BAD_HANDLE, r.ctypes.data_as(dp), 10, acof.ctypes.data_as(dp), kcof.ctypes.data_as(dp),
                     err.ctypes.data_as(dp)) == 0.0
    assert "llz_lpc" in capi.last_error() and (acof == 5.0).all() and err[0] == 4.0


def test_lpc_mc_arguments_refused_before_any_device_work():
    x = np.zeros((4, 32), dtype=np.float32)
    acof = np.zeros((4, 66), dtype=np.float32)
    with pytest.raises(capi.LlzError, match="p 65"):
        filters.lpc_mc(x, acof, p=65)
    with pytest.raises(capi.LlzError, match="p 32"):
        filters.lpc_mc(x, np.zeros((4, 33), dtype=np.float32), p=32)
    assert capi.lib().llz_lpc_mc(x.ctypes.data, None, None, None, None, None, None, 4, 32, 8, None) < 0
    assert "llz_lpc_mc" in capi.last_error()


def test_new_symbols_declared_and_exported():
    names = capi.declared_symbols()
    L = capi.lib()
    for n in ("llz_levinson", "llz_levinson1", "llz_atlvs", "llz_lpc_init", "llz_lpc_uninit", "llz_lpc", "llz_lpc_mc"):
        assert n in names and hasattr(L, n), n
    assert capi.lib().llz_hip_tune(b"lpc_split", -1) == 0


def test_lpc_init_without_gpu_fails_cleanly():
    L = capi.lib()
    if L.llz_hip_device_count() > 0:
        pytest.skip("GPU present")
    assert L.llz_lpc_init(16) == capi.BAD_HANDLE
    with pytest.raises(capi.LlzError):
        filters.Lpc(16)
