"""CPU-side checks of the stream convolver (include/llz_fir.h part 5, llz_fir_stream_mc): the ten symbols exist in every layer
with their prototypes and the bank's nine-name set is untouched, every init refusal comes with a message of its own for both
tap types, without a GPU a valid init fails loudly, the host layer -- the one builder of the tap spectra included -- runs clean
under AddressSanitizer + UBSan in a stand-alone driver (tests/stream_sanitize_driver.c) where the builder's entries are held to
a direct real DFT, and every case of tests/test_fir_stream_gpu.py -- its inputs, references and limits -- is run against the
numpy float32 model of the algorithm (tests/stream_checks.py).  No kernel is launched here.  On the parent of this feature the
library exports no stream convolver and every test below that touches it fails."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import edge_checks as ec
from tests import part_checks as pc
from tests import stream_checks as sc
from tests.test_fir_bank_host import SYMBOLS as BANK_SYMBOLS
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

P = "llz_fir_stream_mc"
INIT_ARGS = r"\(\s*int \w+,\s*int \w+,\s*int \w+,\s*const %s \*\w+,\s*int \w+,\s*int \w+\s*\)"
PROTOTYPES = {
    P + "_init": r"\bunsigned long\s+%s\s*" + INIT_ARGS % "float",
    P + "_init_f64taps": r"\bunsigned long\s+%s\s*" + INIT_ARGS % "double",
    P + "_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P: r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
    P + "_flush": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*float \*\w+\s*\)",
    P + "_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P + "_set_taps": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*const float \*\w+\s*\)",
    P + "_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\[4\]\s*\)",
    P + "_flt_len": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P + "_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
}
NEW = list(PROTOTYPES)


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no stream convolver"
    return lib


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, "llz_fir.h")).read(), flags=re.S)


def test_symbols_declared_bound_and_exported(L):
    text = header()
    assert len(NEW) == 10
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in NEW)
    assert all(getattr(L, n).argtypes is not None for n in NEW)
    assert set(re.findall(r"\b(llz_fir_stream_mc\w*)\s*\(", text)) == set(NEW)
    for method in ("filter", "flush", "reset", "set_taps", "plan", "close"):
        assert hasattr(filters.FirStreamMC, method), method


def test_bank_name_set_is_untouched(L):
    declared = set(re.findall(r"\b(llz_fir_bank_mc\w*)\s*\(", header()))
    assert declared == set(BANK_SYMBOLS) and len(BANK_SYMBOLS) == 9, declared ^ set(BANK_SYMBOLS)
    assert not any(n.startswith("llz_fir_bank_mc") or n.startswith("llz_fir_filter_mc") for n in NEW)


def refused(L, what, *args, f64=False):
    init = L.llz_fir_stream_mc_init_f64taps if f64 else L.llz_fir_stream_mc_init
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_fir_stream_mc_init" in msg, (what, msg)
    return msg


def test_init_refusals_carry_a_message(L):
    """(channels, block, frame_len, taps, rows, flt_len): each refusal names the init and the range it missed, and no two
    kinds of refusal share a message"""
    taps = np.ones(3 * (sc.MAX_TAPS + 1), dtype=np.float32)
    taps64 = np.ones(3 * (sc.MAX_TAPS + 1))
    for f64, p in ((False, taps.ctypes.data), (True, taps64.ctypes.data)):
        seen = {}
        for block in (0, 63, 96, 8192):
            seen["block"] = refused(L, f"block {block}", 2, block, max(block, 1), p, 1, 100, f64=f64)
            assert "64..4096" in seen["block"] and str(block) in seen["block"]
        seen["frame 0"] = refused(L, "frame_len 0", 2, 64, 0, p, 1, 100, f64=f64)
        seen["frame"] = refused(L, "frame_len 100", 2, 64, 100, p, 1, 100, f64=f64)
        assert "frame_len" in seen["frame"] and "frame_len" in seen["frame 0"]
        for T in (0, -1, sc.MAX_TAPS + 1):
            seen["taps"] = refused(L, f"flt_len {T}", 2, 64, 64, p, 1, T, f64=f64)
            assert "1..131073" in seen["taps"], T
        seen["rows"] = refused(L, "rows 2 of 3 channels", 3, 64, 64, p, 2, 100, f64=f64)
        assert "rows" in seen["rows"]
        for channels in (0, 65536):
            seen["channels"] = refused(L, f"channels {channels}", channels, 64, 64, p, 1, 100, f64=f64)
            assert "1..65535" in seen["channels"]
        seen["null"] = refused(L, "NULL taps", 2, 64, 64, None, 1, 100, f64=f64)
        assert "taps" in seen["null"]
        kinds = [re.sub(r"-?\d+", "#", m) for m in seen.values()]
        assert len(set(kinds)) == len(kinds) - 1, kinds         # the two frame_len refusals are one kind
    with pytest.raises(capi.LlzError, match="1..131073"):
        filters.FirStreamMC(2, 64, np.ones(sc.MAX_TAPS + 1))
    with pytest.raises(capi.LlzError, match="taps must be"):
        filters.FirStreamMC(3, 64, np.ones((2, 100)))             # neither shared nor a row per channel


def test_calls_refuse_a_bad_handle(L):
    import ctypes as C
    out = (C.c_int * 4)()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("llz_fir_stream_mc_plan", lambda: L.llz_fir_stream_mc_plan(h, out)),
                           ("llz_fir_stream_mc_reset", lambda: L.llz_fir_stream_mc_reset(h)),
                           ("llz_fir_stream_mc_flush", lambda: L.llz_fir_stream_mc_flush(h, out)),
                           ("llz_fir_stream_mc_set_taps", lambda: L.llz_fir_stream_mc_set_taps(h, 0, 1, out)),
                           ("llz_fir_stream_mc", lambda: L.llz_fir_stream_mc(h, out, out, 64))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1 and name in capi.last_error(), name
        assert L.llz_fir_stream_mc_flt_len(h) == -1 and L.llz_fir_stream_mc_set_stream(h, None) == -1
        L.llz_fir_stream_mc_uninit(h)


@pytest.mark.parametrize("block,T,rows", [(64, 1, 1), (512, 513, 2), (128, sc.MAX_TAPS, 1), (4096, sc.MAX_TAPS, 2)])
def test_valid_init_without_gpu_fails_loudly(L, block, T, rows):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a handle whose plan is {2 block, P, P + k - 1, k} and
    that the other forms' entry points refuse"""
    import ctypes as C
    taps = np.ones((rows, T), dtype=np.float32)
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_fir_stream_mc_init(2, block, 3 * block, taps.ctypes.data, rows, T)
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        out = (C.c_int * 4)()
        assert L.llz_fir_stream_mc_plan(h, out) == 0 and tuple(out) == (2 * block, -(-T // block), -(-T // block) + 2, 3)
        assert L.llz_fir_stream_mc_flt_len(h) == T and L.llz_fir_filter_mc_algo(h) < 0 and L.llz_fir_bank_mc_algo(h) < 0
        L.llz_fir_stream_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_fir_stream_mc_init"):
            filters.FirStreamMC(2, block, taps if rows == 2 else taps[0], frame_len=3 * block)


def test_host_layer_and_spectrum_builder_under_asan_ubsan(tmp_path):
    """the stand-alone driver: llz_host_stream_spectra against a direct real DFT, and every call of the handle layer over the
    stubbed device shim, at (block, taps) = (64, 1), (64, 65), (512, 513), (128, 131073)"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    exe = tmp_path / "stream_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "stream_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "STREAM_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    assert len(re.findall(r"stream spectra block=(?:64 T=1|64 T=65|512 T=513|128 T=131073) ", r.stdout)) == 4, r.stdout


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
def run_model(x, taps, block, k):
    return sc.model(x, taps, block, k)


@pytest.mark.parametrize("block,T", sc.SHAPES)
@pytest.mark.parametrize("channels", sc.CHANNELS)
def test_gpu_cases_hold_on_the_model(oracle, block, T, channels):
    """the parity cases of test_fir_stream_gpu.py: same inputs, references and limits, the model in the device's place"""
    sc.check_shape(run_model, oracle, block, T, channels)


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "rows"])
def test_gpu_longest_case_holds_on_the_model(oracle, per_channel):
    sc.check_shape(run_model, oracle, 128, sc.MAX_TAPS, 2, calls=6, per_channel=per_channel)


def test_gpu_ring_case_holds_on_the_model(oracle):
    """(64, 199), k = 3: R = 6, 2 R + 1 calls; and the grouping of blocks into calls does not change a bit"""
    block, T, k = 64, 199, 3
    assert sc.partitions(T, block) + k - 1 == 6
    sc.check_shape(run_model, oracle, block, T, 3, k=k, calls=13)
    x = sc.signal(oracle, 3, 13 * k * block, seed=1 + T + block)
    h = ec.dense_taps(T, seed=T)
    assert np.array_equal(sc.bits(sc.model(x, h, block, k)), sc.bits(sc.model(x, h, block, 1)))


def test_model_sees_a_wrong_delay(oracle):
    """the limits are not slack: the right taps one partition late miss the gate by orders of magnitude"""
    block, T = 64, 199
    x = sc.signal(oracle, 3, 6 * block, seed=1 + T + block)
    h = ec.dense_taps(T, seed=T)
    y = sc.model(x, np.concatenate([np.zeros(block), h])[:T], block)
    ref = sc.dense_ref(oracle, x, h)
    assert pc.rel_rms(y[:, :6 * block], ref[:, :6 * block]) > 1e3 * ec.TOL
