"""CPU-side checks of LLZ_FIR_ALGO_PARTITIONED (include/llz_fir.h part 2): the constant and the new query exist in every
layer, init refusals carry a message, without a GPU a valid init fails loudly, and the float64 FFT convolution that stands in
for the oracle at 131073 taps agrees with the oracle where both are affordable.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import edge_checks as ec
from tests import part_checks as pc

ERR_ARG = -1


@pytest.fixture(scope="module")
def L():
    capi.build()
    return capi.lib()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, "llz_fir.h")).read(), flags=re.S)


def test_constant_in_header_capi_and_filters():
    assert re.search(r"\bLLZ_FIR_ALGO_PARTITIONED\s*=\s*7\b", header())
    assert capi.FIR_ALGO_PARTITIONED == 7 == filters.FIR_ALGO_PARTITIONED == pc.PARTITIONED


def test_partition_plan_declared_and_exported(L):
    name = "llz_fir_filter_mc_partition_plan"
    assert re.search(r"\bint\s+" + name + r"\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+\[4\]\s*\)", header())
    assert name in capi.declared_symbols() and hasattr(L, name)
    assert hasattr(filters.FirFilterMC, "partition_plan")


def test_tunes_are_named(L):
    for name in (b"part_nfft", b"part_scratch_mb"):
        assert L.llz_hip_tune(name, -1) == 0, capi.last_error()


def refused(L, what, *args, f64=False):
    init = L.llz_fir_filter_mc_init_f64taps if f64 else L.llz_fir_filter_mc_init
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    assert init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert "llz_fir_filter_mc_init" in msg, (what, msg)
    return msg


def test_init_refusals_carry_a_message(L):
    taps = np.ones(pc.MAX_TAPS + 1, dtype=np.float32)
    taps64 = np.ones(pc.MAX_TAPS + 1)
    msg = refused(L, "131074 taps", 2, 1024, taps.ctypes.data, pc.MAX_TAPS + 1, pc.PARTITIONED)
    assert "1..131073" in msg, msg
    msg = refused(L, "131074 taps, double", 2, 1024, taps64.ctypes.data, pc.MAX_TAPS + 1, pc.PARTITIONED, f64=True)
    assert "1..131073" in msg, msg
    assert "1..131073" in refused(L, "2^22 taps", 2, 1024, taps.ctypes.data, 1 << 22, pc.PARTITIONED)
    # the other algos keep their refusal: the time-domain kernel's LDS tile
    for algo in (filters.FIR_ALGO_TIME, filters.FIR_ALGO_AUTO, filters.FIR_ALGO_TIME_MFMA, filters.FIR_ALGO_OVERLAP_SAVE_8192):
        assert "LDS tile" in refused(L, f"25249 taps algo {algo}", 2, 1024, taps.ctypes.data, 25249, algo)
    for channels in (0, 65536):
        refused(L, f"channels {channels}", channels, 1024, taps.ctypes.data, 1300, pc.PARTITIONED)
    refused(L, "flt_len 0", 2, 1024, taps.ctypes.data, 0, pc.PARTITIONED)
    refused(L, "frame_len 0", 2, 0, taps.ctypes.data, 1300, pc.PARTITIONED)
    refused(L, "NULL taps", 2, 1024, None, 1300, pc.PARTITIONED)
    assert "unknown algo 8" in refused(L, "algo 8", 2, 1024, taps.ctypes.data, 63, 8)


def test_bank_still_refuses_the_partitioned_form(L):
    taps = np.ones((2, 63), dtype=np.float32)
    assert L.llz_fir_bank_mc_init(2, 1024, taps.ctypes.data, 63, pc.PARTITIONED) == capi.BAD_HANDLE
    assert "not built for a bank" in capi.last_error()


@pytest.mark.parametrize("T", [1300, 25249, pc.MAX_TAPS])
def test_valid_init_without_gpu_fails_loudly(L, T):
    """a valid algo-7 init: without a GPU BAD_HANDLE and a message that is not the parent's "unknown algo"; with one a handle
    whose plan the query reports"""
    taps = np.ones(T, dtype=np.float32)
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_fir_filter_mc_init(2, 4096, taps.ctypes.data, T, pc.PARTITIONED)
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        assert L.llz_fir_filter_mc_algo(h) == pc.PARTITIONED and L.llz_fir_filter_mc_flt_len(h) == T
        L.llz_fir_filter_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        msg = capi.last_error()
        assert msg not in ("", before) and "unknown algo" not in msg and "LDS tile" not in msg, msg
        with pytest.raises(capi.LlzError):
            filters.FirFilterMC(2, 4096, taps, algo=filters.FIR_ALGO_PARTITIONED)


def test_partition_plan_refuses_a_bad_handle(L):
    import ctypes as C
    out = (C.c_int * 4)()
    for h in (0, capi.BAD_HANDLE):
        assert L.llz_fir_filter_mc_partition_plan(h, 1024, out) == ERR_ARG
        assert "llz_fir_filter_mc_partition_plan" in capi.last_error()


@pytest.mark.parametrize("T", [6146, 25249])
def test_fft_reference_is_pinned_to_the_oracle(oracle, T):
    """the float64 FFT convolution used at 131073 taps against the oracle's time-domain loop: <= 1e-12 relative RMS, dense
    and two-ends taps, a signal longer than the filter and its zero-padded tail"""
    x = oracle.synth_f32(2, T // 4 + 1000, seed=T)
    xz = np.concatenate([x, np.zeros((2, T - 1), np.float32)], axis=1)
    for name, h in (("dense", ec.dense_taps(T, seed=T)), ("two-ends-", ec.two_ends_taps(T, -1))):
        ref = oracle.fir_batch_f32(xz, h)
        got = pc.fft_ref(xz, h)
        for c in range(2):
            rel = pc.rel_rms(got[c], ref[c])
            print(f"fft_ref against the oracle, T={T} {name} ch {c}: relative rms {rel:.3g}")
            assert rel <= 1e-12


def test_partition_limit_counts_the_partitions_that_hold_a_tap():
    x = np.ones((2, 64)) * np.array([[1.0], [2.0]])
    one = ec.ols_limit(1024, 1.0, 1.0)
    assert np.allclose(pc.partition_limit(1024, ec.one_delta_taps(1300, 0), x)[:, 0], [one, 2 * one])
    assert np.allclose(pc.partition_limit(1024, ec.two_ends_taps(1300, -1), x)[:, 0], [2 * one, 4 * one])
    assert np.allclose(pc.partition_limit(1024, ec.two_ends_taps(512, 1), x)[:, 0], np.sqrt(2.0) * np.array([one, 2 * one]))
    assert pc.partitions(512, 1024) == 1 and pc.partitions(513, 1024) == 2 and pc.partitions(pc.MAX_TAPS, 8192) == 33
