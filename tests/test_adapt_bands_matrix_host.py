"""CPU-side checks of the multi-reference per-band adaptive filter (include/llz_adapt_bands_matrix.h, llz_adapt_bands_matrix_mc):
the symbols exist in every layer with their prototypes, every init refusal comes with a message of its own, every call refuses a
bad handle, without a GPU a valid init fails loudly, the host layer runs scripted streams clean under AddressSanitizer + UBSan in
a stand-alone driver (tests/adapt_bands_matrix_sanitize_driver.c) whose frame counters, launches and history buffers equal the
script's line for line, the numpy float32 model of the algorithm (tests/adapt_bands_matrix_checks.py) stays inside half of the
limits on every GPU case, the model equals the definition written out as loops, five planted faults each miss the limits, two
references do what one cannot, and the float64 chain of the end-to-end case reaches the tenth its GPU test asks for.  No kernel is
launched here.  On the parent of this feature the library exports no llz_adapt_bands_matrix_mc and every test below fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import adapt_bands_matrix_checks as mc
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

P = "llz_adapt_bands_matrix_mc"
PROTOTYPES = {
    P + "_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*float \w+,\s*float \w+\s*\)",
    P + "_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P: r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*const float \*\w+,\s*const float \*\w+,\s*const float \*\w+,"
       r"\s*float \*\w+,\s*float \*\w+,\s*float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
    P + "_set_step": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*const float \*\w+\s*\)",
    P + "_set_taps": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*const float \*\w+,"
                     r"\s*const float \*\w+\s*\)",
    P + "_get_taps": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*float \*\w+,\s*float \*\w+\s*\)",
    P + "_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\s*\)",
    P + "_frames": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*long long \*\w+\s*\)",
    P + "_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\[5\]\s*\)",
    P + "_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
}
NEW = list(PROTOTYPES)
SHIMS = {"llzs_matrix_bands_nlms_f32", "llzs_matrix_bands_nlms_plan"}
GOOD = (2, 3, 33, 8, 0.5, 1e-3)        # inputs, outputs, bins, taps, mu, delta


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no multi-reference per-band adaptive filter"
    return lib


def test_symbols_declared_bound_and_exported(L):
    raw = open(os.path.join(capi.INCLUDE_DIR, "llz_adapt_bands_matrix.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert len(NEW) == 10
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert set(re.findall(r"\b(llz_\w+)\s*\(", text)) == set(NEW)
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in NEW)
    assert all(getattr(L, n).argtypes is not None for n in NEW)
    for fn in ("llz_adapt.h", "llz_adapt_matrix.h", "llz_adapt_bands.h"):
        assert "llz_adapt_bands_matrix" not in open(os.path.join(capi.INCLUDE_DIR, fn)).read(), fn
    shim = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "llz_shim.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(llzs_matrix_bands\w*)\s*\(", shim)) == SHIMS
    assert all(("int " + n + "(") in gen_stub() for n in SHIMS)
    for method in ("process", "set_step", "set_taps", "get_taps", "reset", "frames", "plan", "set_stream", "close"):
        assert hasattr(filters.AdaptBandsMatrixMC, method), method


def refused(L, what, args):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert L.llz_adapt_bands_matrix_mc_init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_adapt_bands_matrix_mc_init" in msg, (what, msg)
    return msg


def with_arg(index, value, base=GOOD):
    args = list(base)
    args[index] = value
    return args


def test_init_refusals_carry_a_message(L):
    """each refusal names the init and what it missed, and no two kinds of refusal share a message"""
    seen = {}
    for v in (0, -1, 9):
        seen["inputs"] = refused(L, f"inputs {v}", with_arg(0, v, (2, 3, 33, 1, 0.5, 1e-3)))
        assert "1..8" in seen["inputs"] and f"inputs {v}" in seen["inputs"]
    for v in (0, -1, 4097):
        seen["outputs"] = refused(L, f"outputs {v}", with_arg(1, v))
        assert "1..4096" in seen["outputs"] and f"outputs {v}" in seen["outputs"]
    for v in (0, -5, 4098):
        seen["bins"] = refused(L, f"bins {v}", with_arg(2, v))
        assert "1..4097" in seen["bins"] and f"bins {v}" in seen["bins"]
    for v in (0, -1, 65):
        seen["taps"] = refused(L, f"taps {v}", with_arg(3, v, (1, 3, 33, 8, 0.5, 1e-3)))
        assert "1..64" in seen["taps"] and f"taps {v}" in seen["taps"]
    for inputs, taps in ((5, 13), (8, 9), (2, 33), (3, 22)):
        seen["entries"] = refused(L, f"{inputs} x {taps}", (inputs, 3, 33, taps, 0.5, 1e-3))
        assert f"{inputs} x {taps} = {inputs * taps} regressor entries" in seen["entries"] and "above 64" in seen["entries"]
    assert "= 65 " in refused(L, "65 entries", (5, 3, 33, 13, 0.5, 1e-3))
    for v in (-0.5, 2.5, float("nan")):
        seen["mu"] = refused(L, f"mu {v}", with_arg(4, v))
        assert "outside 0..2" in seen["mu"] and "mu" in seen["mu"]
    for v in (0.0, -1.0, float("inf"), float("nan")):
        seen["delta"] = refused(L, f"delta {v}", with_arg(5, v))
        assert "delta" in seen["delta"] and "finite" in seen["delta"]
    kinds = [re.sub(r"-?\d+(\.\d+)?|nan|inf", "#", m) for m in seen.values()]
    assert len(set(kinds)) == len(kinds) == 7, kinds
    with pytest.raises(capi.LlzError, match="1..8"):
        filters.AdaptBandsMatrixMC(9, 2, 33, 1)
    with pytest.raises(capi.LlzError, match="1..4096"):
        filters.AdaptBandsMatrixMC(2, 4097, 33, 1)


def test_calls_refuse_a_bad_handle(L):
    f4, i5, n = (C.c_float * 64)(), (C.c_int * 5)(), C.c_longlong()
    M = "llz_adapt_bands_matrix_mc"
    for h in (0, capi.BAD_HANDLE):
        for name, call in ((M + "_plan", lambda: L.llz_adapt_bands_matrix_mc_plan(h, i5)),
                           (M + "_reset", lambda: L.llz_adapt_bands_matrix_mc_reset(h, 1)),
                           (M + "_frames", lambda: L.llz_adapt_bands_matrix_mc_frames(h, C.byref(n))),
                           (M + "_set_stream", lambda: L.llz_adapt_bands_matrix_mc_set_stream(h, None)),
                           (M + "_set_step", lambda: L.llz_adapt_bands_matrix_mc_set_step(h, 0, 1, f4)),
                           (M + "_set_taps", lambda: L.llz_adapt_bands_matrix_mc_set_taps(h, 0, 1, 0, 1, f4, f4)),
                           (M + "_get_taps", lambda: L.llz_adapt_bands_matrix_mc_get_taps(h, 0, 1, 0, 1, f4, f4)),
                           (M, lambda: L.llz_adapt_bands_matrix_mc(h, f4, f4, f4, f4, f4, f4, None, None, 1))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1 and name in capi.last_error() and "bad handle" in capi.last_error(), name
        L.llz_adapt_bands_matrix_mc_uninit(h)


@pytest.mark.parametrize("inputs,outputs,bins,taps", [(1, 1, 1, 1), (2, 3, 129, 16), (8, 4096, 5, 8), (1, 2, 4097, 64)])
def test_valid_init_without_gpu_fails_loudly(L, inputs, outputs, bins, taps):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a handle whose plan names the instance and that another
    family's entry point refuses"""
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_adapt_bands_matrix_mc_init(inputs, outputs, bins, taps, 0.5, 1e-3)
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        out = (C.c_int * 6)()
        assert L.llz_adapt_bands_matrix_mc_plan(h, out) == 0
        assert tuple(out[:2]) == (inputs, mc.ceiling(inputs, taps)) and out[4] == 1
        assert L.llz_adapt_bands_mc_plan(h, out) < 0 and L.llz_adapt_matrix_mc_plan(h, out) < 0
        L.llz_adapt_bands_matrix_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_adapt_bands_matrix_mc_init"):
            filters.AdaptBandsMatrixMC(inputs, outputs, bins, taps)


# ------------------------------------------------------------------------------------------------ the host layer under sanitizers
SCRIPT = (
    [("init", 3, 2, 33, 5)] + [("call", n, y) for n, y in ((0, 1), (1, 1), (1, 0), (7, 1), (50, 0), (0, 0))]
    + [("taps",), ("step",), ("call", 3, 1), ("refuse",), ("call", 2, 0), ("fail", 4), ("call", 1, 1), ("fail", 1), ("refuse",),
       ("call", 6, 0)]                                                                              # refused between issued ones
    + [("reset", 0), ("call", 2, 0), ("reset", 1), ("call", 1, 1), ("call", 1, 1), ("reset", 0), ("reset", 1), ("call", 3, 0),
       ("taps",)]                                                                                   # resets at either buffer
    + [("init", 1, 1, 1, 1), ("call", 1, 1), ("call", 33, 0), ("taps",), ("reset", 1), ("call", 2, 1)]       # no history at all
    + [("init", 2, 5, 7, 2), ("call", 1, 1), ("call", 1, 0), ("call", 0, 0), ("call", 1, 1), ("reset", 0), ("call", 1, 0)]  # one row
    + [("init", 4, 37, 129, 16), ("call", 2, 1), ("step",), ("call", 1, 0), ("fail", 20), ("call", 20, 1), ("taps",)]
    + [("init", 8, 4096, 3, 8), ("call", 1, 1), ("call", 9, 0), ("taps",), ("step",), ("reset", 0), ("call", 2, 1)]
    + [("init", 2, 1, 4097, 32), ("call", 0, 1), ("call", 3, 1), ("reset", 0), ("call", 1, 1), ("call", 40, 0)]   # the widest row
)


def lines_of_script(script):
    """what the driver prints behind every command: the frame counter, the launches since the init, and which of the two history
    buffers the last launch read -- buffer 0 first, then in turn behind every launch that was ISSUED; a reset clears where it is"""
    lines, n, launches, cur, read = [], 0, 0, 0, -1
    for cmd in script:
        if cmd[0] == "init":
            n, launches, cur, read = 0, 0, 0, -1
        elif cmd[0] == "reset":
            n = 0
        elif cmd[0] == "call" and cmd[1] > 0:
            n, launches, read, cur = n + cmd[1], launches + 1, cur, cur ^ 1
        lines.append(f"{cmd[0]} frames {n} launches {launches} read {read}")
    return lines


def test_host_layer_under_asan_ubsan(tmp_path):
    """the stand-alone driver over the stubbed device shim, with the driver's own history step in the place of the kernel's:
    refused inits and calls, calls of 0, 1 and many frames with and without y on host buffers of exactly the stated sizes, calls
    the shim refuses between issued ones, set_taps / get_taps round trips of sub-matrices, set_step, both resets at either
    buffer, one tap (no history), 4096 outputs, the widest row.  Every launch reads the history the script fed; the frame
    counter, the launches and the buffer read equal the script's line for line"""
    entry = "llzs_matrix_bands_nlms_f32"
    text = gen_stub().splitlines()
    assert sum(ln.startswith(f"int {entry}(") for ln in text) == 1
    stub = tmp_path / "shim_stub.c"
    stub.write_text("\n".join(ln for ln in text if not ln.startswith(f"int {entry}(")) + "\n")       # the driver brings its own
    script = tmp_path / "script.txt"
    script.write_text("".join(" ".join(str(v) for v in cmd) + "\n" for cmd in SCRIPT))
    exe = tmp_path / "adapt_bands_matrix_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "adapt_bands_matrix_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ADAPT_BANDS_MATRIX_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    got = [ln for ln in r.stdout.splitlines() if " frames " in ln]
    assert got == lines_of_script(SCRIPT)
    assert any(ln.endswith("read 1") for ln in got) and any(ln.startswith("reset") and ln.endswith("read 0") for ln in got)


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
@pytest.mark.parametrize("inputs,outputs,taps,bins,frames", mc.SHAPES + [mc.LONG])
def test_gpu_case_holds_on_the_model(oracle, inputs, outputs, taps, bins, frames):
    """the condition of the GPU list: the float32 model of the algorithm stays below half of the error and tap limits, inside
    the misalignment limit, and converges wherever the float64 model does"""
    mc.check_parity(mc.model32, oracle, inputs, outputs, taps, bins, frames, share=0.5)


def test_model_matches_the_definition_written_out(oracle):
    """the vectorised float64 model against the definition as plain loops over Python complex numbers, on a tiny case; a frozen
    output keeps its weights and still filters"""
    inputs, outputs, taps, bins, frames = 3, 2, 3, 5, 40
    x, d, _ = mc.case(oracle, inputs, outputs, taps, bins, frames)
    m = mc.Model(inputs, outputs, bins, taps, prec=64)
    e, y = m.process(x[:, :25], d[:, :25])
    m.set_step(1, 0.0)
    w_frozen = m.W[1].copy()
    e2, y2 = m.process(x[:, 25:], d[:, 25:])
    assert np.array_equal(m.W[1], w_frozen) and m.frames() == frames
    for k in (0, 2, 4):
        ee, yy, ww = mc.definition_loops(x[:, :, k], d[0, :, k], taps, mc.MU, mc.DELTA)
        assert np.max(np.abs(np.concatenate([e[0, :, k], e2[0, :, k]]) - ee)) < 1e-12
        assert np.max(np.abs(np.concatenate([y[0, :, k], y2[0, :, k]]) - yy)) < 1e-12
        assert np.max(np.abs(m.W[0, :, :, k] - ww)) < 1e-12
    ee, yy, ww = mc.definition_loops(x[:, :25, 3], d[1, :25, 3], taps, mc.MU, mc.DELTA)
    assert np.max(np.abs(w_frozen[:, :, 3] - ww)) < 1e-12
    want = sum(ww[i, q] * x[i, 30 - q, 3] for q in range(taps) for i in range(inputs))
    assert abs(y2[1, 5, 3] - want) < 1e-12 and abs(e2[1, 5, 3] - (d[1, 30, 3] - want)) < 1e-12


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault", mc.FAULTS)
def test_limits_see_a_planted_fault(oracle, fault):
    """the limits are not slack: each fault planted in the float32 model misses one by more than 1e3 at (3, 2, 5, 33, 300)"""
    assert mc.FAULT_SHAPE == (3, 2, 5, 33, 300)
    worst = mc.worst_miss(lambda *a: mc.Model(*a, prec=32, fault=fault), oracle, *mc.FAULT_SHAPE)
    print(f"planted fault {fault}: misses a limit by a factor of {worst:.3g}")
    assert worst > 1e3, fault


# ------------------------------------------------------------------------------------------------ the point of the feature
def test_two_references_do_what_one_cannot(oracle):
    """d = h_0 * x_0 + h_1 * x_1, paths of equal norms, on the float64 models: the single-reference filter on x_0 takes x_1's echo
    for noise and keeps its last run's error (rms over the run's 16 frames and all bins) above half of its first run's; the
    two-reference filter falls below a tenth in every bin"""
    one, two = mc.two_against_one(oracle)
    print(f"last / first run's error: one reference {one:.3g}, two references at most {np.max(two):.3g}")
    assert one > 0.5
    assert np.all(two < 0.1)


# ------------------------------------------------------------------------------------------------ the end-to-end case
def test_end_to_end_case_reaches_a_tenth_in_float64(oracle):
    """the case of the GPU suite's end-to-end test, through pfb_checks' float64 bank and the float64 model: the synthesised
    residual's rms over the last quarter is below a tenth of the synthesised d's on every output"""
    res = mc.e2e_float64(oracle)
    print("float64 chain: residual / d over the last quarter per output:", " ".join(f"{r:.3g}" for r in res))
    assert res.shape == (mc.E2E["outputs"],) and np.all(res < 0.1)
