"""CPU-side checks of the per-band adaptive filter (include/llz_adapt_bands.h, llz_adapt_bands_mc): the symbols exist in every
layer with their prototypes, every init refusal comes with a message of its own, every call refuses a bad handle, without a GPU a
valid init fails loudly, the host layer runs scripted streams clean under AddressSanitizer + UBSan in a stand-alone driver
(tests/adapt_bands_sanitize_driver.c) whose frame counters equal the script's, the numpy float32 model of the algorithm
(tests/adapt_bands_checks.py) stays inside the limits on every GPU case, the model equals the definition written out as loops,
four planted faults each miss the limits, and the float64 chain of the end-to-end case reaches the tenth its GPU test asks for.
No kernel is launched here.  On the parent of this feature the library exports no llz_adapt_bands_mc and every test below fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import adapt_bands_checks as bc
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

P = "llz_adapt_bands_mc"
PROTOTYPES = {
    P + "_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*int \w+,\s*float \w+,\s*float \w+\s*\)",
    P + "_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P: r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*const float \*\w+,\s*const float \*\w+,\s*const float \*\w+,"
       r"\s*float \*\w+,\s*float \*\w+,\s*float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
    P + "_set_step": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*const float \*\w+\s*\)",
    P + "_set_taps": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*const float \*\w+,\s*const float \*\w+\s*\)",
    P + "_get_taps": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*float \*\w+,\s*float \*\w+\s*\)",
    P + "_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\s*\)",
    P + "_frames": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*long long \*\w+\s*\)",
    P + "_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\[4\]\s*\)",
    P + "_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
}
NEW = list(PROTOTYPES)
SHIMS = {"llzs_bands_nlms_f32", "llzs_bands_nlms_plan"}
GOOD = (2, 33, 8, 0.5, 1e-3)           # channels, bins, taps, mu, delta


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no per-band adaptive filter"
    return lib


def test_symbols_declared_bound_and_exported(L):
    raw = open(os.path.join(capi.INCLUDE_DIR, "llz_adapt_bands.h")).read()
    assert "llz_pfb" not in raw and "llz_asrc" not in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert len(NEW) == 10
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert set(re.findall(r"\b(llz_\w+)\s*\(", text)) == set(NEW)
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in NEW)
    assert all(getattr(L, n).argtypes is not None for n in NEW)
    for fn in ("llz_adapt.h", "llz_adapt_matrix.h"):
        assert "llz_adapt_bands" not in open(os.path.join(capi.INCLUDE_DIR, fn)).read(), fn
    shim = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "llz_shim.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(llzs_bands\w*)\s*\(", shim)) == SHIMS
    assert all(("int " + n + "(") in gen_stub() for n in SHIMS)
    for method in ("process", "set_step", "set_taps", "get_taps", "reset", "frames", "plan", "set_stream", "close"):
        assert hasattr(filters.AdaptBandsMC, method), method


def refused(L, what, args):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert L.llz_adapt_bands_mc_init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_adapt_bands_mc_init" in msg, (what, msg)
    return msg


def with_arg(index, value):
    args = list(GOOD)
    args[index] = value
    return args


def test_init_refusals_carry_a_message(L):
    """each refusal names the init and what it missed, and no two kinds of refusal share a message"""
    seen = {}
    for v in (0, -1, 65536):
        seen["channels"] = refused(L, f"channels {v}", with_arg(0, v))
        assert "1..65535" in seen["channels"] and f"channels {v}" in seen["channels"]
    for v in (0, -5, 4098):
        seen["bins"] = refused(L, f"bins {v}", with_arg(1, v))
        assert "1..4097" in seen["bins"] and f"bins {v}" in seen["bins"]
    for v in (0, -1, 65):
        seen["taps"] = refused(L, f"taps {v}", with_arg(2, v))
        assert "1..64" in seen["taps"] and f"taps {v}" in seen["taps"]
    for v in (-0.5, 2.5, float("nan")):
        seen["mu"] = refused(L, f"mu {v}", with_arg(3, v))
        assert "outside 0..2" in seen["mu"] and "mu" in seen["mu"]
    for v in (0.0, -1.0, float("inf"), float("nan")):
        seen["delta"] = refused(L, f"delta {v}", with_arg(4, v))
        assert "delta" in seen["delta"] and "finite" in seen["delta"]
    kinds = [re.sub(r"-?\d+(\.\d+)?|nan|inf", "#", m) for m in seen.values()]
    assert len(set(kinds)) == len(kinds) == 5, kinds
    with pytest.raises(capi.LlzError, match="1..64"):
        filters.AdaptBandsMC(2, 33, 65)


def test_calls_refuse_a_bad_handle(L):
    f4, i4, n = (C.c_float * 64)(), (C.c_int * 4)(), C.c_longlong()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("llz_adapt_bands_mc_plan", lambda: L.llz_adapt_bands_mc_plan(h, i4)),
                           ("llz_adapt_bands_mc_reset", lambda: L.llz_adapt_bands_mc_reset(h, 1)),
                           ("llz_adapt_bands_mc_frames", lambda: L.llz_adapt_bands_mc_frames(h, C.byref(n))),
                           ("llz_adapt_bands_mc_set_stream", lambda: L.llz_adapt_bands_mc_set_stream(h, None)),
                           ("llz_adapt_bands_mc_set_step", lambda: L.llz_adapt_bands_mc_set_step(h, 0, 1, f4)),
                           ("llz_adapt_bands_mc_set_taps", lambda: L.llz_adapt_bands_mc_set_taps(h, 0, 1, f4, f4)),
                           ("llz_adapt_bands_mc_get_taps", lambda: L.llz_adapt_bands_mc_get_taps(h, 0, 1, f4, f4)),
                           ("llz_adapt_bands_mc", lambda: L.llz_adapt_bands_mc(h, f4, f4, f4, f4, f4, f4, None, None, 1))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1 and name in capi.last_error() and "bad handle" in capi.last_error(), name
        L.llz_adapt_bands_mc_uninit(h)


@pytest.mark.parametrize("bins,taps", [(1, 1), (129, 16), (4097, 64)])
def test_valid_init_without_gpu_fails_loudly(L, bins, taps):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a handle whose plan names the tap ceiling and that another
    family's entry point refuses"""
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_adapt_bands_mc_init(2, bins, taps, 0.5, 1e-3)
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        out = (C.c_int * 4)()
        assert L.llz_adapt_bands_mc_plan(h, out) == 0 and out[0] == bc.ceiling(taps) and out[3] == 1
        assert L.llz_adapt_mc_plan(h, out) < 0 and L.llz_pfb_mc_bins(h) < 0
        L.llz_adapt_bands_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_adapt_bands_mc_init"):
            filters.AdaptBandsMC(2, bins, taps)


# ------------------------------------------------------------------------------------------------ the host layer under sanitizers
SCRIPT = (
    [("init", 3, 33, 5)] + [("call", n, y) for n, y in ((0, 1), (1, 1), (1, 0), (7, 1), (50, 0), (0, 0))]
    + [("taps",), ("step",), ("call", 3, 1), ("reset", 0), ("call", 2, 0), ("reset", 1), ("call", 1, 1), ("taps",)]
    + [("init", 2, 1, 1), ("call", 1, 1), ("call", 33, 0), ("taps",), ("reset", 1)]                  # no history at all
    + [("init", 37, 129, 64), ("call", 2, 1), ("step",), ("call", 1, 0), ("taps",)]
    + [("init", 1, 4097, 33), ("call", 0, 1), ("call", 3, 1), ("reset", 0), ("call", 1, 1)]          # the widest row
)


def counters_of_script(script):
    lines, n = [], 0
    for cmd in script:
        if cmd[0] in ("init", "reset"):
            n = 0
        elif cmd[0] == "call":
            n += cmd[1]
        lines.append(f"{cmd[0]} frames {n}")
    return lines


def test_host_layer_under_asan_ubsan(tmp_path):
    """the stand-alone driver over the stubbed device shim: refused inits and calls, calls of 0, 1 and many frames with and
    without y on host buffers of exactly the stated sizes, set_taps / get_taps round trips, set_step, both resets, one tap (no
    history), the widest row; the frame counter equals the script's line for line"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    script = tmp_path / "script.txt"
    script.write_text("".join(" ".join(str(v) for v in cmd) + "\n" for cmd in SCRIPT))
    exe = tmp_path / "adapt_bands_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "adapt_bands_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ADAPT_BANDS_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    got = [ln for ln in r.stdout.splitlines() if " frames " in ln]
    assert got == counters_of_script(SCRIPT)


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
@pytest.mark.parametrize("channels", bc.CHANNELS)
@pytest.mark.parametrize("taps,bins,frames", bc.SHAPES)
def test_gpu_case_holds_on_the_model(oracle, taps, bins, frames, channels):
    """the float32 model of the algorithm stays inside the limits, converges and keeps the zero bins on every GPU case"""
    bc.check_parity(bc.model32, oracle, taps, bins, frames, channels)


def test_long_rows_hold_on_the_model(oracle):
    taps, bins, frames, channels = bc.LONG
    bc.check_parity(bc.model32, oracle, taps, bins, frames, channels)


def test_model_matches_the_definition_written_out(oracle):
    """the vectorised float64 model against the definition as plain loops over Python complex numbers, on a tiny case; a frozen
    channel keeps its weights and still filters"""
    taps, bins, frames, channels = 3, 5, 40, 2
    x, d, _ = bc.case(oracle, taps, bins, frames, channels)
    m = bc.Model(channels, bins, taps, prec=64)
    e, y = m.process(x[:, :25], d[:, :25])
    m.set_step(1, 0.0)
    w_frozen = m.W[1].copy()
    e2, y2 = m.process(x[:, 25:], d[:, 25:])
    assert np.array_equal(m.W[1], w_frozen) and m.frames() == frames
    for k in (0, bc.ZERO_X, 4):
        ee, yy, ww = bc.definition_loops(x[0, :, k], d[0, :, k], taps, bc.MU, bc.DELTA)
        assert np.max(np.abs(np.concatenate([e[0, :, k], e2[0, :, k]]) - ee)) < 1e-12
        assert np.max(np.abs(np.concatenate([y[0, :, k], y2[0, :, k]]) - yy)) < 1e-12
        assert np.max(np.abs(m.W[0, :, k] - ww)) < 1e-12
    ee, yy, ww = bc.definition_loops(x[1, :25, 3], d[1, :25, 3], taps, bc.MU, bc.DELTA)
    assert np.max(np.abs(w_frozen[:, 3] - ww)) < 1e-12
    want = sum(ww[q] * x[1, 30 - q, 3] for q in range(taps))
    assert abs(y2[1, 5, 3] - want) < 1e-12 and abs(e2[1, 5, 3] - (d[1, 30, 3] - want)) < 1e-12


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault", bc.FAULTS)
def test_limits_see_a_planted_fault(oracle, fault):
    """the limits are not slack: each fault planted in the float32 model misses one by more than 1e3 (5 taps: three taps of the
    ceiling of 8 do not exist)"""
    taps, bins, frames = bc.SHAPES[2]
    assert bc.ceiling(taps) > taps
    worst = bc.worst_miss(lambda *a: bc.Model(*a, prec=32, fault=fault), oracle, taps, bins, frames, 3)
    print(f"planted fault {fault}: misses a limit by a factor of {worst:.3g}")
    assert worst > 1e3, fault


# ------------------------------------------------------------------------------------------------ the end-to-end case
def test_end_to_end_case_reaches_a_tenth_in_float64(oracle):
    """the case of the GPU suite's end-to-end test, through pfb_checks' float64 bank and the float64 model: the synthesised
    residual's rms over the last quarter is below a tenth of the synthesised d's on every channel"""
    res = bc.e2e_float64(oracle)
    print("float64 chain: residual / d over the last quarter per channel:", " ".join(f"{r:.3g}" for r in res))
    assert res.shape == (bc.E2E["channels"],) and np.all(res < 0.1)
