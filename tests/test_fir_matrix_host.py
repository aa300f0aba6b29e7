"""CPU-side checks of the matrix convolver (include/llz_fir.h part 6, llz_fir_matrix_mc: y_o = sum_i x_i * h[o][i]): the ten
symbols exist in every layer with their prototypes and the name sets of the other FIR families are untouched, every init refusal
comes with a message of its own for both tap types, set_taps ranges outside the matrix and foreign handles are refused, without
a GPU a valid init fails loudly, the host layer runs clean under AddressSanitizer + UBSan in a stand-alone driver
(tests/matrix_sanitize_driver.c), and every case of tests/test_fir_matrix_gpu.py -- its inputs, references and limits -- is run
against the numpy complex64 model of the algorithm (tests/matrix_checks.py), which misses the limits by more than 1e3 for each
planted fault.  No kernel is launched here.  On the parent of this feature the library exports no matrix convolver and every
test below that touches it fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import edge_checks as ec
from tests import matrix_checks as mc
from tests import part_checks as pc
from tests.test_fir_bank_host import SYMBOLS as BANK_SYMBOLS
from tests.test_fir_stream_host import NEW as STREAM_SYMBOLS
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

P = "llz_fir_matrix_mc"
INIT_ARGS = r"\(\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*const %s \*\w+,\s*int \w+\s*\)"
PROTOTYPES = {
    P + "_init": r"\bunsigned long\s+%s\s*" + INIT_ARGS % "float",
    P + "_init_f64taps": r"\bunsigned long\s+%s\s*" + INIT_ARGS % "double",
    P + "_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P: r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
    P + "_flush": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*float \*\w+\s*\)",
    P + "_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P + "_set_taps": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*const float \*\w+\s*\)",
    P + "_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\[6\]\s*\)",
    P + "_flt_len": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P + "_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
}
NEW = list(PROTOTYPES)
OTHER_FAMILIES = ("llz_fir_stream_mc", "llz_fir_bank_mc", "llz_fir_filter_mc", "llz_fir_pbank_mc")


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no matrix convolver"
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
    assert set(re.findall(r"\b(llz_fir_matrix_mc\w*)\s*\(", text)) == set(NEW)
    for method in ("filter", "flush", "reset", "set_taps", "plan", "close"):
        assert hasattr(filters.FirMatrixMC, method), method


def test_other_families_name_sets_are_untouched(L):
    text = header()
    assert set(re.findall(r"\b(llz_fir_stream_mc\w*)\s*\(", text)) == set(STREAM_SYMBOLS) and len(STREAM_SYMBOLS) == 10
    assert set(re.findall(r"\b(llz_fir_bank_mc\w*)\s*\(", text)) == set(BANK_SYMBOLS) and len(BANK_SYMBOLS) == 9
    assert set(re.findall(r"\b(llz_fir_pbank_mc\w*)\s*\(", text)) == {"llz_fir_pbank_mc_init", "llz_fir_pbank_mc_init_f64taps",
                                                                      "llz_fir_pbank_mc_plan"}
    assert not any(n.startswith(OTHER_FAMILIES) for n in NEW)


def refused(L, what, *args, f64=False):
    init = L.llz_fir_matrix_mc_init_f64taps if f64 else L.llz_fir_matrix_mc_init
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_fir_matrix_mc_init" in msg, (what, msg)
    return msg


def test_init_refusals_carry_a_message(L):
    """(inputs, outputs, block, frame_len, taps, flt_len): each refusal names the init and the range it missed, and no two
    kinds of refusal share a message"""
    taps = np.ones(4 * 200, dtype=np.float32)
    taps64 = np.ones(4 * 200)
    for f64, p in ((False, taps.ctypes.data), (True, taps64.ctypes.data)):
        seen = {}
        for inputs in (0, -3, 4097):
            seen["inputs"] = refused(L, f"inputs {inputs}", inputs, 2, 64, 64, p, 100, f64=f64)
            assert "inputs" in seen["inputs"] and "1..4096" in seen["inputs"] and str(inputs) in seen["inputs"]
        for outputs in (0, 4097):
            seen["outputs"] = refused(L, f"outputs {outputs}", 2, outputs, 64, 64, p, 100, f64=f64)
            assert "outputs" in seen["outputs"] and "1..4096" in seen["outputs"]
        for block in (0, 63, 96, 8192):
            seen["block"] = refused(L, f"block {block}", 2, 2, block, max(block, 1), p, 100, f64=f64)
            assert "64..4096" in seen["block"] and str(block) in seen["block"]
        seen["frame 0"] = refused(L, "frame_len 0", 2, 2, 64, 0, p, 100, f64=f64)
        seen["frame"] = refused(L, "frame_len 100", 2, 2, 64, 100, p, 100, f64=f64)
        assert "frame_len" in seen["frame"] and "frame_len" in seen["frame 0"]
        assert "1..65535" in refused(L, "65536 blocks", 2, 2, 64, 64 * 65536, p, 100, f64=f64)
        for T in (0, -1, mc.MAX_TAPS + 1):
            seen["taps"] = refused(L, f"flt_len {T}", 2, 2, 64, 64, p, T, f64=f64)
            assert "1..131073" in seen["taps"], T
        seen["null"] = refused(L, "NULL taps", 2, 2, 64, 64, None, 100, f64=f64)
        assert "no taps" in seen["null"]
        kinds = [re.sub(r"-?\d+", "#", m) for m in seen.values()]
        assert len(set(kinds)) == len(kinds) - 1, kinds         # the two frame_len refusals are one kind
    with pytest.raises(capi.LlzError, match="taps must be"):
        filters.FirMatrixMC(3, 2, 64, np.ones((3, 2, 100)))      # [inputs, outputs, T]: the wrong way round
    with pytest.raises(capi.LlzError, match="taps must be"):
        filters.FirMatrixMC(3, 2, 64, np.ones((2, 100)))


def test_calls_refuse_bad_and_foreign_handles(L):
    out = (C.c_int * 6)()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("llz_fir_matrix_mc_plan", lambda: L.llz_fir_matrix_mc_plan(h, out)),
                           ("llz_fir_matrix_mc_reset", lambda: L.llz_fir_matrix_mc_reset(h)),
                           ("llz_fir_matrix_mc_flush", lambda: L.llz_fir_matrix_mc_flush(h, out)),
                           ("llz_fir_matrix_mc_set_taps", lambda: L.llz_fir_matrix_mc_set_taps(h, 0, 1, 0, 1, out)),
                           ("llz_fir_matrix_mc", lambda: L.llz_fir_matrix_mc(h, out, out, 64))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1 and name in capi.last_error(), name
        assert L.llz_fir_matrix_mc_flt_len(h) == -1 and L.llz_fir_matrix_mc_set_stream(h, None) == -1
        L.llz_fir_matrix_mc_uninit(h)


@pytest.mark.parametrize("block,T,inputs,outputs", [(64, 1, 2, 2), (512, 513, 8, 2), (128, mc.MAX_TAPS, 1, 2)])
def test_valid_init_without_gpu_fails_loudly(L, block, T, inputs, outputs):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a handle with the expected plan that the other forms'
    entry points refuse, that refuses set_taps ranges outside the matrix, and that counts its connected paths"""
    taps = np.ones((outputs, inputs, T), dtype=np.float32)
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_fir_matrix_mc_init(inputs, outputs, block, 3 * block, taps.ctypes.data, T)
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        out = (C.c_int * 6)()
        assert L.llz_fir_matrix_mc_plan(h, out) == 0 and tuple(out) == mc.expected_plan(block, T, inputs, outputs, 3)
        assert L.llz_fir_matrix_mc_flt_len(h) == T and L.llz_fir_filter_mc_algo(h) < 0 and L.llz_fir_bank_mc_algo(h) < 0
        assert L.llz_fir_stream_mc_flt_len(h) < 0
        for rng in ((outputs, 1, 0, 1), (0, outputs + 1, 0, 1), (0, 1, inputs, 1), (0, 1, 0, inputs + 1), (-1, 1, 0, 1)):
            assert L.llz_fir_matrix_mc_set_taps(h, *rng, taps.ctypes.data) == -1
            assert "llz_fir_matrix_mc_set_taps" in capi.last_error() and "outside" in capi.last_error()
        L.llz_fir_matrix_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_fir_matrix_mc_init"):
            filters.FirMatrixMC(inputs, outputs, block, taps, frame_len=3 * block)


def test_host_layer_under_asan_ubsan(tmp_path):
    """the stand-alone driver over the generated shim stub: init, calls, set_taps of sub-matrices and the connection table,
    flush (in passes too), reset, plan and every refusal; nothing is loaded into python"""
    stub_text = gen_stub()
    for entry in ("llzs_fir_matrix_fwd_f32", "llzs_fir_matrix_mac_f32", "llzs_fir_matrix_inv_f32"):
        assert re.search(r"\bint " + entry + r"\(", stub_text), entry
    stub = tmp_path / "shim_stub.c"
    stub.write_text(stub_text)
    exe = tmp_path / "matrix_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "matrix_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "MATRIX_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    assert len(re.findall(r"matrix handle block=(?:64 T=1 2x2|64 T=65 3x2|512 T=513 2x3|128 T=131073 1x2) ok", r.stdout)) == 4


def test_group_function_covers_both_kinds():
    """the parity list holds a shape with G > 1 and a ragged last group, and one with G = 1; G never exceeds the inputs"""
    gs = {s: mc.groups(s[2], s[3], s[0]) for s in mc.SHAPES}
    assert any(G > 1 and s[2] % G for s, (G, _) in gs.items()), gs
    assert any(G == 1 for G, _ in gs.values()), gs
    assert mc.groups(37, 2, 64) == (19, 2) and mc.groups(64, 2, 128) == (32, 2) and mc.groups(2, 64, 128) == (2, 1)
    for inputs in (1, 2, 3, 31, 33, 64, 100, 4096):
        for outputs in (1, 2, 64, 1024, 4096):
            for block in (64, 512, 1024, 4096):
                G, size = mc.groups(inputs, outputs, block)
                assert 1 <= G <= min(inputs, 32) and (G - 1) * size < inputs <= G * size


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
def run_model(x, taps, block, k):
    return mc.model(x, taps, block, k)


@pytest.mark.parametrize("block,T,inputs,outputs", mc.SHAPES)
def test_gpu_cases_hold_on_the_model(oracle, block, T, inputs, outputs):
    """the parity cases of test_fir_matrix_gpu.py: same inputs, references and limits, the model in the device's place"""
    mc.check_shape(run_model, oracle, block, T, inputs, outputs)


def test_gpu_longest_case_holds_on_the_model(oracle):
    block, T, inputs, outputs = mc.LONGEST
    mc.check_shape(run_model, oracle, block, T, inputs, outputs, calls=6)


def test_gpu_ring_case_holds_on_the_model(oracle):
    """(64, 199), k = 3, 3 -> 2: R = 6, 2 R + 1 calls; and the grouping of blocks into calls does not change a bit"""
    block, T, k = 64, 199, 3
    mc.check_shape(run_model, oracle, block, T, 3, 2, k=k, calls=13)
    x, _ = mc.case_signal(oracle, block, T, 3, k, 13)
    h = mc.dense_matrix(T, 3, 2)
    assert np.array_equal(mc.bits(mc.model(x, h, block, k)), mc.bits(mc.model(x, h, block, 1)))


def test_model_skips_unconnected_paths(oracle):
    """h[0][1] all zero and NaN / Inf blocks in x_1: output 0 finite and equal to the run with x_1 zeroed"""
    block, T = 64, 199
    x, n = mc.case_signal(oracle, block, T, 3)
    h = mc.dense_matrix(T, 3, 2).copy()
    h[0, 1] = 0.0
    xn = x.copy()
    xn[1, block:2 * block] = np.nan
    xn[1, 3 * block] = np.inf
    xz = x.copy()
    xz[1] = 0.0
    y, yz = mc.model(xn, h, block), mc.model(xz, h, block)
    assert np.isfinite(y[0]).all() and np.array_equal(y[0], yz[0]) and np.isnan(y[1, block:2 * block]).all()


@pytest.mark.parametrize("fault", ["transposed", "late", "group"])
def test_model_sees_each_planted_fault(oracle, fault):
    """the limits are not slack: H indexed (i, o), one path applied a partition late, the last input group left out of the
    inverse's sum -- each misses the dense gate and the sparse limit by more than 1e3"""
    block, T, inputs, outputs = 64, 199, 5, 3
    assert mc.groups(inputs, outputs, block)[0] > 1
    x, n = mc.case_signal(oracle, block, T, inputs)
    h = mc.dense_matrix(T, inputs, outputs)
    ref = mc.dense_ref(oracle, x, h)
    assert mc.dense_ratio(mc.model(x, h, block), ref, n) <= 1.0
    miss = mc.dense_ratio(mc.model(x, h, block, fault=fault), ref, n)
    hs = mc.sparse_matrix(T, inputs, outputs)
    sref, lim = mc.sparse_ref(x, hs, block)
    smiss = float(np.max(np.abs(mc.model(x, hs, block, fault=fault).astype(np.float64) - sref) / lim))
    print(f"{fault}: {miss:.3g} x the dense gate, {smiss:.3g} x the sparse limit")
    assert miss > 1e3 and smiss > 1e3, (fault, miss, smiss)


def test_gpu_flush_in_passes_case_holds_on_the_model(oracle):
    """16 -> 8 at block 4096 and 81921 taps: the flush of 20 blocks exceeds the partial-spectra scratch (16 blocks)"""
    block, T, inputs, outputs = mc.PASSES
    x, n = mc.case_signal(oracle, block, T, inputs, calls=1)
    h = mc.dense_matrix(T, inputs, outputs)
    pc.check_dense(mc.model(x, h, block), mc.dense_ref(oracle, x, h), n, "matrix flush in passes (model)")
