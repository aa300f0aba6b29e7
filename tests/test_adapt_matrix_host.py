"""CPU-side checks of the multi-reference adaptive filter (include/llz_adapt_matrix.h, llz_adapt_matrix_mc): the nine symbols
exist in every layer with their prototypes, every refusal comes with a message of its own, a bad handle is refused by every call,
without a GPU a valid init fails loudly, the input groups come from the one function the matrix convolver uses, the host layer
runs clean under AddressSanitizer + UBSan in a stand-alone driver (tests/adapt_matrix_sanitize_driver.c) whose sub-matrix
set_taps -> get_taps round trip is held to 2 u |h|_2 per tap, cases 2 to 7 of tests/test_adapt_matrix_gpu.py run against the
numpy float32 model of the definition (tests/adapt_matrix_checks.py) under the same limits (where the device is held to another
handle's bits, the model to the 1e-5 gate against that handle's numpy model; case 5, the update's grouping under the adapt_ppw
override, has no counterpart in a model without workgroups), and five planted faults each miss a limit at
shapes 2 and 4.  No kernel is launched here.  On the parent of this feature the library exports no llz_adapt_matrix_mc and the
tests below that touch it fail."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import adapt_checks as ac
from tests import adapt_matrix_checks as xc
from tests import matrix_checks as mc
from tests import stream_checks as sc
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

P = "llz_adapt_matrix_mc"
PROTOTYPES = {
    P + "_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*float \w+,\s*float \w+\s*\)",
    P + "_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P: r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*const float \*\w+,\s*float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
    P + "_set_step": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*const float \*\w+\s*\)",
    P + "_set_taps": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*const float \*\w+\s*\)",
    P + "_get_taps": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*float \*\w+\s*\)",
    P + "_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\s*\)",
    P + "_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\[6\]\s*\)",
    P + "_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
}
NEW = list(PROTOTYPES)


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no multi-reference adaptive filter"
    return lib


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, "llz_adapt_matrix.h")).read(), flags=re.S)


def test_symbols_declared_bound_and_exported(L):
    text = header()
    assert len(NEW) == 9
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in NEW)
    assert all(getattr(L, n).argtypes is not None for n in NEW)
    assert set(re.findall(r"\b(llz_adapt_matrix_mc\w*)\s*\(", text)) == set(NEW)
    for method in ("process", "set_step", "set_taps", "get_taps", "reset", "plan", "set_stream", "close"):
        assert hasattr(filters.AdaptMatrixMC, method), method
    doc = open(os.path.join(capi.INCLUDE_DIR, "llz_adapt_matrix.h")).read()
    assert "graph capture is not" in doc and "NaN" in doc


def test_both_handles_take_their_groups_from_one_function():
    host = os.path.join(CSRC, "host")
    for fn in ("llz_fir_matrix_host.c", "llz_adapt_matrix_host.c"):
        text = open(os.path.join(host, fn)).read()
        assert len(re.findall(r"\bllz_host_matrix_groups\s*\(", text)) == 1, fn
    assert "llz_host_matrix_groups" in open(os.path.join(host, "llz_host.h")).read()


def test_both_adaptive_handles_take_their_shared_steps_from_the_core():
    """the init's refusals, the step sizes, get_taps and the staged call are llz_adapt_core.c's: both handles call them, and
    neither keeps a copy of the messages that went there"""
    host = os.path.join(CSRC, "host")
    header = open(os.path.join(host, "llz_host.h")).read()
    core = open(os.path.join(host, "llz_adapt_core.c")).read()
    calls = ("llz_adapt_refuse", "llz_adapt_steps_create", "llz_adapt_steps_destroy", "llz_adapt_steps_set", "llz_adapt_get_taps",
             "llz_adapt_io_begin", "llz_adapt_io_end", "llz_adapt_io_release")
    moved = ("outside 0..2", "is not built", "is not a power of two", "is not k x block", "is not a finite value",
             "in-place filtering is not supported", "of step sizes", "of weight spectra")
    for name in calls:
        assert name in header and len(re.findall(r"\b%s\s*\(" % name, core)) == 1, name
    for text in moved:
        assert text in core, text
    for fn in ("llz_adapt_host.c", "llz_adapt_matrix_host.c"):
        text = open(os.path.join(host, fn)).read()
        for name in calls:
            assert re.search(r"\b%s\s*\(" % name, text), (fn, name)
        for other in moved + ("llz_refuse_device_overlap", "llz_stage_in", "llz_stage_out", "llz_host_stream_taps"):
            assert other not in text, (fn, other)


def refused(L, what, *args):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert L.llz_adapt_matrix_mc_init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_adapt_matrix_mc_init" in msg, (what, msg)
    return msg


def test_init_refusals_carry_a_message(L):
    """(inputs, outputs, block, frame_len, flt_len, mu, delta): each refusal names the init and the range it missed, and no two
    kinds of refusal share a message"""
    seen = {}
    for ports in (0, 4097):
        seen["inputs"] = refused(L, f"inputs {ports}", ports, 2, 64, 64, 100, 0.5, 0.064)
        assert "inputs" in seen["inputs"] and "1..4096" in seen["inputs"]
        seen["outputs"] = refused(L, f"outputs {ports}", 2, ports, 64, 64, 100, 0.5, 0.064)
        assert "outputs" in seen["outputs"] and "1..4096" in seen["outputs"]
    for block in (0, 63, 96, 8192):
        seen["block"] = refused(L, f"block {block}", 2, 2, block, max(block, 1), 100, 0.5, 0.064)
        assert "64..2048" in seen["block"] and str(block) in seen["block"]
    seen["4096"] = refused(L, "block 4096", 2, 2, 4096, 4096, 100, 0.5, 0.064)
    assert "4096 is not built" in seen["4096"] and "64..2048" in seen["4096"]
    seen["frame 0"] = refused(L, "frame_len 0", 2, 2, 64, 0, 100, 0.5, 0.064)
    seen["frame"] = refused(L, "frame_len 100", 2, 2, 64, 100, 100, 0.5, 0.064)
    assert "frame_len" in seen["frame"] and "frame_len" in seen["frame 0"]
    for T in (0, -1, sc.MAX_TAPS + 1):
        seen["taps"] = refused(L, f"flt_len {T}", 2, 2, 64, 64, T, 0.5, 0.064)
        assert "1..131073" in seen["taps"], T
    for mu in (-0.25, 2.5, float("nan"), float("inf")):
        seen["mu"] = refused(L, f"mu {mu}", 2, 2, 64, 64, 100, mu, 0.064)
        assert "mu" in seen["mu"] and "0..2" in seen["mu"]
    for delta in (0.0, -1.0, float("nan"), float("inf")):
        seen["delta"] = refused(L, f"delta {delta}", 2, 2, 64, 64, 100, 0.5, delta)
        assert "delta" in seen["delta"]
    kinds = [re.sub(r"-?\d+(\.\d+)?|nan|inf", "#", m) for m in seen.values()]
    assert len(set(kinds)) == len(kinds) - 1, kinds             # the two frame_len refusals are one kind
    with pytest.raises(capi.LlzError, match="1..131073"):
        filters.AdaptMatrixMC(2, 2, 64, sc.MAX_TAPS + 1)
    with pytest.raises(capi.LlzError, match="64..2048"):
        filters.AdaptMatrixMC(2, 2, 4096, 100)


def test_calls_refuse_a_bad_handle(L):
    out = (C.c_float * 64)()
    plan = (C.c_int * 6)()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("llz_adapt_matrix_mc_plan", lambda: L.llz_adapt_matrix_mc_plan(h, plan)),
                           ("llz_adapt_matrix_mc_reset", lambda: L.llz_adapt_matrix_mc_reset(h, 0)),
                           ("llz_adapt_matrix_mc_set_step", lambda: L.llz_adapt_matrix_mc_set_step(h, 0, 1, out)),
                           ("llz_adapt_matrix_mc_set_taps", lambda: L.llz_adapt_matrix_mc_set_taps(h, 0, 1, 0, 1, out)),
                           ("llz_adapt_matrix_mc_get_taps", lambda: L.llz_adapt_matrix_mc_get_taps(h, 0, 1, 0, 1, out)),
                           ("llz_adapt_matrix_mc_set_stream", lambda: L.llz_adapt_matrix_mc_set_stream(h, None)),
                           ("llz_adapt_matrix_mc:", lambda: L.llz_adapt_matrix_mc(h, out, out, out, None, 64))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1 and name in capi.last_error(), name
        L.llz_adapt_matrix_mc_uninit(h)


@pytest.mark.parametrize("block,T", [(64, 1), (512, 513), (128, sc.MAX_TAPS)])
def test_valid_init_without_gpu_fails_loudly(L, block, T):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a handle whose plan is {2 block, P, P + k - 1, k, G, inputs
    per group} and that the other forms' entry points refuse"""
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_adapt_matrix_mc_init(3, 2, block, 3 * block, T, 0.5, 3e-3 * block)
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        out = (C.c_int * 6)()
        want = (2 * block, -(-T // block), -(-T // block) + 2, 3) + mc.groups(3, 2, block)
        assert L.llz_adapt_matrix_mc_plan(h, out) == 0 and tuple(out) == want
        assert L.llz_fir_matrix_mc_plan(h, out) < 0 and L.llz_adapt_mc_reset(h, 0) < 0 and L.llz_fir_stream_mc_reset(h) < 0
        L.llz_adapt_matrix_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_adapt_matrix_mc_init"):
            filters.AdaptMatrixMC(3, 2, block, T, frame_len=3 * block)


def test_host_layer_under_asan_ubsan(tmp_path):
    """the stand-alone driver: every entry point and refusal of the handle layer over the stubbed device shim, and the
    set_taps -> get_taps round trip of a sub-matrix within 2 u |h|_2 per tap, at (block, taps) = (64, 1), (64, 65), (512, 513),
    (128, 131073)"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    exe = tmp_path / "adapt_matrix_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "adapt_matrix_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "ADAPT_MATRIX_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    ratios = re.findall(r"adapt matrix round trip block=(?:64 T=1|64 T=65|512 T=513|128 T=131073) P=\d+: worst ratio to 2 u \|h\| (\S+)",
                        r.stdout)
    assert len(ratios) == 4 and all(float(v) <= 1.0 for v in ratios), r.stdout


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
@pytest.mark.parametrize("block,T,inputs,outputs,nblocks", xc.SHAPES)
def test_gpu_parity_cases_hold_on_the_model(oracle, block, T, inputs, outputs, nblocks):
    """case 3 of test_adapt_matrix_gpu.py: same inputs, reference and limits, the float32 model in the device's place; error
    and taps stay below half their limits (the misalignment's limit is twice the model's: 0.5 there says 'the model's')"""
    m = xc.check_parity(xc.model32, oracle, block, T, inputs, outputs, nblocks)
    assert m["error"] <= 0.5 and m["taps"] <= 0.5


def matrix_model(x, h, block):
    """the matrix convolver's numpy float32 model (tests/matrix_checks.py) in FirMatrixMC's place: the frames"""
    return mc.model(x, h, block)[:, :x.shape[1]]


def test_gpu_frozen_case_holds_on_the_model(oracle):
    xc.check_frozen(xc.model32, matrix_model, oracle, exact=False)


def test_one_input_is_the_single_reference_model(oracle):
    """case 1 between the two numpy models: with one input the float32 model gives adapt_checks.Model's values"""
    block, T, nblocks = 64, 199, 12
    x, d, _ = xc.case(oracle, block, T, 1, 3, nblocks)
    a = xc.model32(1, 3, block, T, delta=xc.delta_for(block, 1))
    b = ac.model32(3, block, T, delta=xc.delta_for(block, 1))
    (ea, ya), (eb, yb) = a.process(x, d), b.process(np.repeat(x, 3, axis=0), d)
    assert np.all(xc.rms(ea - eb, axis=1) <= xc.TOL * xc.rms(d, axis=1)) and np.all(xc.rms(ya - yb, axis=1) <= xc.TOL * xc.rms(d, axis=1))
    assert np.all(xc.row_norm(a.get_taps() - b.get_taps()[:, None]) <= xc.TOL)


def test_gpu_handover_case_holds_on_the_model(oracle):
    xc.check_handover(xc.model32, matrix_model, oracle, exact=False)


def test_gpu_grouping_case_holds_on_the_model(oracle):
    xc.check_grouping(xc.model32, oracle)


def test_gpu_isolation_cases_hold_on_the_model(oracle):
    xc.check_isolation(xc.model32, oracle)
    xc.check_freeze_one(xc.model32, oracle)


def test_gpu_reset_and_sub_matrix_cases_hold_on_the_model(oracle):
    xc.check_reset(xc.model32, oracle)
    xc.check_submatrix(xc.model32, oracle)


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("shape", xc.FAULT_SHAPES, ids=["shape2", "shape4"])
@pytest.mark.parametrize("fault", xc.FAULTS)
def test_limits_see_a_planted_fault(oracle, fault, shape):
    """the limits are not slack: each fault in the float32 model misses one by the factor printed"""
    def faulty(i, o, b, t, frame_len=None, mu=xc.MU, delta=None):
        return xc.Model(i, o, b, t, frame_len, mu, delta, prec=32, fault=fault)
    factor = xc.worst_miss(faulty, oracle, *shape)
    print(f"planted fault {fault} at {shape}: misses a limit by a factor of {factor:.3g}")
    assert factor > 100.0, (fault, shape)
