"""CPU-side checks of the filter bank llz_fir_bank_mc (include/llz_fir.h part 3): the nine symbols are declared and exported,
every init refusal comes with a message, the calls refuse a bad handle, and without a GPU a valid init fails loudly instead of
computing anywhere else.  No kernel is launched here."""
import re

import numpy as np
import pytest

from llzlab_amd import capi, filters

SYMBOLS = ["llz_fir_bank_mc_init", "llz_fir_bank_mc_init_f64taps", "llz_fir_bank_mc_uninit", "llz_fir_bank_mc",
           "llz_fir_bank_mc_flush", "llz_fir_bank_mc_set_taps", "llz_fir_bank_mc_flt_len", "llz_fir_bank_mc_algo",
           "llz_fir_bank_mc_set_stream"]
ERR_ARG = -1
TIME_MFMA, OLS = filters.FIR_ALGO_TIME_MFMA, filters.FIR_ALGO_OVERLAP_SAVE


@pytest.fixture(scope="module")
def L():
    capi.build()
    return capi.lib()


def test_bank_symbols_declared_and_exported(L):
    import os
    text = open(os.path.join(capi.INCLUDE_DIR, "llz_fir.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(llz_fir_bank_mc\w*)\s*\(", text))
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)
    assert all(n in capi.declared_symbols() for n in SYMBOLS)
    assert all(hasattr(L, n) for n in SYMBOLS)


def refused(L, what, *args, f64=False, names=("llz_fir_bank_mc_init",)):
    init = L.llz_fir_bank_mc_init_f64taps if f64 else L.llz_fir_bank_mc_init
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    assert init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert all(n in msg for n in names), (what, msg)
    return msg


def test_bank_init_refusals_carry_a_message(L):
    taps = np.ones((4, 258), dtype=np.float32)
    p = taps.ctypes.data
    for channels in (0, -3, 65536):
        refused(L, f"channels {channels}", channels, 1024, p, 63, 0)
    refused(L, "NULL taps", 4, 1024, None, 63, 0)
    refused(L, "NULL taps, double", 4, 1024, None, 63, 0, f64=True)
    refused(L, "flt_len 0", 4, 1024, p, 0, 0)
    refused(L, "flt_len -1", 4, 1024, p, -1, 0)
    refused(L, "frame_len 0", 4, 0, p, 63, 0)
    for algo in (TIME_MFMA, filters.FIR_ALGO_OVERLAP_SAVE_2048, filters.FIR_ALGO_OVERLAP_SAVE_4096,
                 filters.FIR_ALGO_OVERLAP_SAVE_8192, 7, -1, 99):
        msg = refused(L, f"algo {algo}", 4, 1024, p, 63, algo)
        assert "LLZ_FIR_ALGO_AUTO" in msg and "LLZ_FIR_ALGO_TIME" in msg and "LLZ_FIR_ALGO_OVERLAP_SAVE" in msg, msg
    msg = refused(L, "overlap-save with 258 taps", 4, 1024, p, 258, OLS)
    assert "257" in msg, msg
    with pytest.raises(capi.LlzError):
        filters.FirBankMC(4, 1024, np.ones(63))                   # 1-D taps: no quiet fall-back to the shared form
    with pytest.raises(capi.LlzError):
        filters.FirBankMC(4, 1024, np.ones((3, 63)))


def test_bank_calls_refuse_a_bad_handle(L):
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    for h in (0, capi.BAD_HANDLE):
        assert L.llz_fir_bank_mc(h, p, p, 16) == ERR_ARG and "llz_fir_bank_mc" in capi.last_error()
        assert L.llz_fir_bank_mc_flush(h, p) == ERR_ARG and "llz_fir_bank_mc_flush" in capi.last_error()
        assert L.llz_fir_bank_mc_set_taps(h, 0, 1, p) == ERR_ARG and "llz_fir_bank_mc_set_taps" in capi.last_error()
        assert L.llz_fir_bank_mc_flt_len(h) < 0 and L.llz_fir_bank_mc_algo(h) < 0 and L.llz_fir_bank_mc_set_stream(h, None) < 0
        L.llz_fir_bank_mc_uninit(h)                              # harmless


def test_bank_handle_is_not_a_shared_taps_handle_without_gpu(L):
    """a valid init: without a GPU it fails loudly (BAD_HANDLE and a message), with one it yields a handle of its own kind that
    the shared-taps entry points refuse"""
    taps = np.ones((4, 63), dtype=np.float32)
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_fir_bank_mc_init(4, 1024, taps.ctypes.data, 63, 0)
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        assert L.llz_fir_filter_mc_flt_len(h) < 0 and L.llz_fir_bank_mc_flt_len(h) == 63
        L.llz_fir_bank_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError):
            filters.FirBankMC(4, 1024, taps)
