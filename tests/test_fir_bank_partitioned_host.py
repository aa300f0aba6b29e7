"""CPU-side checks of the partitioned bank (include/llz_fir.h part 4): the three symbols exist in every layer and the bank's
nine-name set is untouched, every init refusal comes with a message of its own, the plan query refuses a bad handle, without
a GPU a valid init fails loudly, and the host layer -- the one builder of the partition spectra included -- runs clean under
AddressSanitizer + UBSan in a stand-alone driver (tests/part_bank_sanitize_driver.c) at 1, 513 and 131073 taps, where the
builder's entries are held to a direct DFT.  No kernel is launched here."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import part_checks as pc
from tests.test_fir_bank_host import SYMBOLS as BANK_SYMBOLS
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

NEW = ["llz_fir_pbank_mc_init", "llz_fir_pbank_mc_init_f64taps", "llz_fir_pbank_mc_plan"]
ERR_ARG = -1


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no partitioned bank"
    return lib


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, "llz_fir.h")).read(), flags=re.S)


def test_symbols_declared_bound_and_exported(L):
    text = header()
    for name in NEW[:2]:
        taps = "float" if name == NEW[0] else "double"
        assert re.search(r"\bunsigned long\s+" + name + r"\s*\(\s*int \w+,\s*int \w+,\s*const " + taps + r" \*\w+,\s*int \w+\s*\)",
                         text), name
    assert re.search(r"\bint\s+" + NEW[2] + r"\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+\[4\]\s*\)", text)
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in NEW)
    assert all(getattr(L, n).argtypes is not None for n in NEW)
    assert hasattr(filters.FirBankMC, "partition_plan")


def test_bank_name_set_is_untouched(L):
    declared = set(re.findall(r"\b(llz_fir_bank_mc\w*)\s*\(", header()))
    assert declared == set(BANK_SYMBOLS) and len(BANK_SYMBOLS) == 9, declared ^ set(BANK_SYMBOLS)
    assert not any(n.startswith("llz_fir_bank_mc") for n in NEW)


def refused(L, what, *args, f64=False):
    init = L.llz_fir_pbank_mc_init_f64taps if f64 else L.llz_fir_pbank_mc_init
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_fir_pbank_mc_init" in msg, (what, msg)
    return msg


def test_init_refusals_carry_a_message(L):
    taps = np.ones(2 * (pc.MAX_TAPS + 1), dtype=np.float32)
    taps64 = np.ones(2 * (pc.MAX_TAPS + 1))
    for f64, p in ((False, taps.ctypes.data), (True, taps64.ctypes.data)):
        for channels in (0, -3, 65536):
            refused(L, f"channels {channels}", channels, 1024, p, 1300, f64=f64)
        refused(L, "frame_len 0", 2, 0, p, 1300, f64=f64)
        refused(L, "NULL taps", 2, 1024, None, 1300, f64=f64)
        for T in (0, -1, pc.MAX_TAPS + 1, 1 << 22):
            assert "1..131073" in refused(L, f"flt_len {T}", 2, 1024, p, T, f64=f64), T
    with pytest.raises(capi.LlzError, match="1..131073"):
        filters.FirBankMC(2, 1024, np.ones((2, pc.MAX_TAPS + 1)), algo=filters.FIR_ALGO_PARTITIONED)
    with pytest.raises(capi.LlzError):
        filters.FirBankMC(2, 1024, np.ones(1300), algo=filters.FIR_ALGO_PARTITIONED)     # 1-D taps: not a bank


def test_scratch_cap_too_small_is_refused_before_any_allocation(L):
    """2 channels x 2^20 samples at 1300 taps under a cap of 1 MiB: not one channel fits; the sizing touches no device, so
    the refusal is the same with and without a GPU"""
    taps = np.ones((2, 1300), dtype=np.float32)
    with capi.tuned(part_nfft=1024, part_scratch_mb=1):
        msg = refused(L, "scratch cap", 2, 1 << 20, taps.ctypes.data, 1300)
    assert "scratch" in msg and "cap" in msg, msg


def test_bank_init_still_refuses_algo_7_and_points_to_the_new_init(L):
    taps = np.ones((2, 63), dtype=np.float32)
    assert L.llz_fir_bank_mc_init(2, 1024, taps.ctypes.data, 63, pc.PARTITIONED) == capi.BAD_HANDLE
    msg = capi.last_error()
    assert all(n in msg for n in ("LLZ_FIR_ALGO_AUTO", "LLZ_FIR_ALGO_TIME", "LLZ_FIR_ALGO_OVERLAP_SAVE", "llz_fir_pbank_mc_init")), msg


def test_plan_refuses_a_bad_handle(L):
    out = (C.c_int * 4)()
    for h in (0, capi.BAD_HANDLE):
        L.llz_hip_tune(b"no_such_override", 0)
        assert L.llz_fir_pbank_mc_plan(h, 1024, out) == ERR_ARG
        assert "llz_fir_pbank_mc_plan" in capi.last_error()


@pytest.mark.parametrize("T", [1, 1300, 25249, pc.MAX_TAPS])
def test_valid_init_without_gpu_fails_loudly(L, T):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a bank handle of algo 7 that the bank's calls take and
    the shared-taps entry points refuse"""
    taps = np.ones((2, T), dtype=np.float32)
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_fir_pbank_mc_init(2, 4096, taps.ctypes.data, T)
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        assert L.llz_fir_bank_mc_algo(h) == pc.PARTITIONED and L.llz_fir_bank_mc_flt_len(h) == T
        assert L.llz_fir_filter_mc_algo(h) < 0
        L.llz_fir_bank_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_fir_pbank_mc_init"):
            filters.FirBankMC(2, 4096, taps, algo=filters.FIR_ALGO_PARTITIONED)


def test_host_layer_and_spectrum_builder_under_asan_ubsan(tmp_path):
    """the stand-alone driver: llz_host_part_spectra against a direct DFT, and init / plan / process / set_taps / flush /
    uninit of the partitioned bank over the stubbed device shim, at 1, 513 and 131073 taps"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    exe = tmp_path / "part_bank_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "part_bank_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "PART_BANK_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    assert len(re.findall(r"spectrum builder T=(?:1|513|131073) ", r.stdout)) == 3, r.stdout
