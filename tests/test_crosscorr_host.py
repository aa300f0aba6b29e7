"""CPU-side checks of the batched cross-correlation (include/llz_corr.h part 2: llz_crosscorr_mc, llz_corr_cof_mc and the
llz_crosscorr_fast_mc handle): the six symbols are declared, exported and bound, and every refusal returns LLZ_ERR_ARG (or
LLZ_BAD_HANDLE) with a message of its own before any device call -- so all of it runs without a GPU.  No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from llzlab_amd import capi, filters

SYMBOLS = ["llz_crosscorr_mc", "llz_corr_cof_mc", "llz_crosscorr_fast_mc_init", "llz_crosscorr_fast_mc_uninit",
           "llz_crosscorr_fast_mc", "llz_crosscorr_fast_mc_set_stream"]
ERR_ARG = -1
TAG_ACFM = 0x4C5A414D                 # the tag of a llz_autocorr_fast_mc_init handle (llz_corr_host.c)


@pytest.fixture(scope="module")
def L():
    capi.build()
    return capi.lib()


def test_symbols_declared_exported_and_bound(L):
    text = open(os.path.join(capi.INCLUDE_DIR, "llz_corr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(llz_(?:crosscorr_mc|corr_cof_mc|crosscorr_fast_mc\w*))\s*\(", text))
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)
    assert all(n in capi.declared_symbols() for n in SYMBOLS)
    for n in SYMBOLS:
        assert getattr(L, n).argtypes is not None, f"capi has no signature for {n}"
    assert L.llz_crosscorr_mc.argtypes == [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]
    assert L.llz_corr_cof_mc.argtypes == [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_void_p]
    assert L.llz_crosscorr_fast_mc.argtypes == [C.c_ulong] + [C.c_void_p] * 3 + [C.c_int] * 2
    assert L.llz_crosscorr_fast_mc_init.restype is C.c_ulong and L.llz_crosscorr_fast_mc_init.argtypes == [C.c_int] * 2
    assert callable(filters.crosscorr_mc) and callable(filters.corr_cof_mc) and hasattr(filters.CrosscorrFastMC, "run")


def refused(L, name, call, want=ERR_ARG):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the entry point's
    rc = call()
    msg = capi.last_error()
    assert rc == want and name in msg, (name, rc, msg)
    return msg


def test_direct_form_refusals_carry_a_message(L):
    buf = np.ones(4 * 300, dtype=np.float32)
    out = np.full(4 * 511, 7.0, dtype=np.float32)
    x, r = buf.ctypes.data, out.ctypes.data

    def cc(xp=x, yp=x, rp=r, frames=4, n=300, p=16, two=0):
        return refused(L, "llz_crosscorr_mc", lambda: L.llz_crosscorr_mc(xp, yp, rp, frames, n, p, two, None))
    cc(xp=None), cc(yp=None), cc(rp=None)
    cc(frames=0), cc(frames=-2), cc(n=0), cc(n=-1), cc(p=-1)
    cc(p=300), cc(p=301), cc(n=10, p=10)                     # p >= n
    cc(p=256), cc(n=300, p=299)                              # p > 255
    cc(two=2), cc(two=-1)

    def cof(ap=x, bp=x, cp=r, frames=4, n=300):
        return refused(L, "llz_corr_cof_mc", lambda: L.llz_corr_cof_mc(ap, bp, cp, frames, n, None))
    cof(ap=None), cof(bp=None), cof(cp=None), cof(frames=0), cof(n=0), cof(n=-5)
    assert (out == 7.0).all()                                # nothing was written


def test_fast_form_refusals_carry_a_message(L):
    buf = np.ones(4 * 300, dtype=np.float32)
    x = buf.ctypes.data
    for frames, n in ((4, 3), (4, 0), (4, -1), (4, 2049), (4, 4096), (0, 300), (-1, 300)):
        refused(L, "llz_crosscorr_fast_mc_init", lambda: L.llz_crosscorr_fast_mc_init(frames, n), want=capi.BAD_HANDLE)
    # a handle of another kind: the tag in front of every handle struct is not this entry point's
    other = (C.c_int * 64)(TAG_ACFM)
    for h in (0, capi.BAD_HANDLE, C.addressof(other)):
        refused(L, "llz_crosscorr_fast_mc", lambda: L.llz_crosscorr_fast_mc(h, x, x, x, 3, 0))
        refused(L, "llz_crosscorr_fast_mc_set_stream", lambda: L.llz_crosscorr_fast_mc_set_stream(h, None))
        L.llz_crosscorr_fast_mc_uninit(h)                        # harmless
    assert other[0] == TAG_ACFM


def test_fast_form_init_fails_loudly_without_gpu_and_checks_p_with_one(L):
    """a valid init: without a GPU it fails loudly (no quiet host computation); with one, p >= n, p < 0, NULL buffers and a bad
    two_sided are refused before anything is staged or launched"""
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_crosscorr_fast_mc_init(4, 300)
    if L.llz_hip_device_count() <= 0:
        assert h == capi.BAD_HANDLE and capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError):
            filters.CrosscorrFastMC(4, 300)
        return
    assert h != capi.BAD_HANDLE, capi.last_error()
    buf = np.ones(4 * 300, dtype=np.float32)
    out = np.full(4 * 601, 7.0, dtype=np.float32)
    x, r = buf.ctypes.data, out.ctypes.data
    for args in ((x, x, r, 300, 0), (x, x, r, 301, 1), (x, x, r, -1, 0), (None, x, r, 3, 0), (x, None, r, 3, 0), (x, x, None, 3, 0),
                 (x, x, r, 3, 2)):
        refused(L, "llz_crosscorr_fast_mc", lambda: L.llz_crosscorr_fast_mc(h, *args))
    assert (out == 7.0).all()
    assert L.llz_autocorr_fast_mc(h, x, r, 3) == ERR_ARG         # and it is no autocorrelation handle either
    L.llz_crosscorr_fast_mc_uninit(h)
