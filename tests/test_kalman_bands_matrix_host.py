"""CPU-side checks of the multi-reference per-band Kalman filter (include/llz_kalman_bands_matrix.h, llz_kalman_bands_matrix_mc):
the symbols exist in every layer with their prototypes, every init refusal comes with a message of its own (inputs x taps above 32
included), every call refuses a bad handle, without a GPU a valid init fails loudly, the host file stands on the shared core and
copies none of its messages, the host layer runs scripted streams clean under AddressSanitizer + UBSan in a stand-alone driver
(tests/kalman_bands_matrix_sanitize_driver.c) that does the kernel's history step itself and whose counters equal the script's,
the numpy float32 model of the algorithm (tests/kalman_bands_matrix_checks.py) stays below a quarter of every limit on every GPU
case, the model equals the definition written out as loops and, with one input, kalman_bands_checks' model bit for bit, five
planted faults each miss a limit, and the double-talk properties hold in float64.  No kernel is launched here.  On the parent of
this feature the library exports no llz_kalman_bands_matrix_mc and every test below fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import kalman_bands_checks as kc
from tests import kalman_bands_matrix_checks as kx
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

P = "llz_kalman_bands_matrix_mc"
OUTS = r"\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*"
PATHS = OUTS + r"int \w+,\s*int \w+,\s*"
PROTOTYPES = {
    P + "_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*float \w+,\s*float \w+,\s*float \w+,"
                 r"\s*float \w+\s*\)",
    P + "_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P: r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*const float \*\w+,\s*const float \*\w+,\s*const float \*\w+,"
       r"\s*float \*\w+,\s*float \*\w+,\s*float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
    P + "_set_adapt": r"\bint\s+%s" + OUTS + r"const int \*\w+\s*\)",
    P + "_set_taps": r"\bint\s+%s" + PATHS + r"const float \*\w+,\s*const float \*\w+\s*\)",
    P + "_get_taps": r"\bint\s+%s" + PATHS + r"float \*\w+,\s*float \*\w+\s*\)",
    P + "_set_variance": r"\bint\s+%s" + PATHS + r"const float \*\w+\s*\)",
    P + "_get_variance": r"\bint\s+%s" + PATHS + r"float \*\w+\s*\)",
    P + "_get_noise": r"\bint\s+%s" + OUTS + r"float \*\w+\s*\)",
    P + "_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\s*\)",
    P + "_frames": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*long long \*\w+\s*\)",
    P + "_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\[5\]\s*\)",
    P + "_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
}
NEW = list(PROTOTYPES)
SHIMS = {"llzs_mkalman_bands_f32", "llzs_mkalman_bands_plan"}
GOOD = (2, 3, 33, 8, 0.999, 0.9, 1.0, 1e-3)         # inputs, outputs, bins, taps, a, lam, p0, delta
HOST_FILE = os.path.join(CSRC, "host", "llz_kalman_bands_matrix_host.c")


@pytest.fixture(scope="module", autouse=True)
def L():
    """the library with the feature in it: every test of this file, the models' own included, stands on it"""
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no multi-reference per-band Kalman filter"
    return lib


def test_symbols_declared_bound_and_exported(L):
    raw = open(os.path.join(capi.INCLUDE_DIR, "llz_kalman_bands_matrix.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert len(NEW) == 13
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert set(re.findall(r"\b(llz_\w+)\s*\(", text)) == set(NEW)
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in NEW)
    assert all(getattr(L, n).argtypes is not None for n in NEW)
    for fn in ("llz_adapt_bands.h", "llz_adapt_bands_matrix.h", "llz_kalman_bands.h"):
        assert "llz_kalman_bands_matrix" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, fn)).read(), flags=re.S), fn
    shim = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "llz_shim.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(llzs_mkalman\w*)\s*\(", shim)) == SHIMS
    assert all(("int " + n + "(") in gen_stub() for n in SHIMS)
    for method in ("process", "set_adapt", "set_taps", "get_taps", "set_variance", "get_variance", "get_noise", "reset", "frames",
                   "plan", "set_stream", "close"):
        assert hasattr(filters.KalmanBandsMatrixMC, method), method
    assert issubclass(filters.KalmanBandsMatrixMC, filters._BandsFilter) and filters.KalmanBandsMatrixMC._PLAN == 5


def refused(L, what, args):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert L.llz_kalman_bands_matrix_mc_init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_kalman_bands_matrix_mc_init" in msg, (what, msg)
    return msg


def with_arg(index, value):
    args = list(GOOD)
    args[index] = value
    return args


def test_init_refusals_carry_a_message(L):
    """each refusal names the init and what it missed, and no two kinds of refusal share a message; inputs x taps above 32 says
    that the state no longer fits a lane's registers and where up to 64 entries are taken"""
    seen = {}
    for v in (0, -1, 9):
        seen["inputs"] = refused(L, f"inputs {v}", with_arg(0, v))
        assert "1..8" in seen["inputs"] and f"inputs {v}" in seen["inputs"]
    for v in (0, -1, 4097):
        seen["outputs"] = refused(L, f"outputs {v}", with_arg(1, v))
        assert "1..4096" in seen["outputs"] and f"outputs {v}" in seen["outputs"]
    for v in (0, -5, 4098):
        seen["bins"] = refused(L, f"bins {v}", with_arg(2, v))
        assert "1..4097" in seen["bins"] and f"bins {v}" in seen["bins"]
    for v in (0, -1, 33, 65):
        seen["taps"] = refused(L, f"taps {v}", with_arg(3, v))
        assert "1..32" in seen["taps"] and f"taps {v}" in seen["taps"]
    for inputs, taps in ((5, 7), (8, 5), (2, 17), (3, 11)):
        args = with_arg(0, inputs)
        args[3] = taps
        seen["entries"] = m = refused(L, f"{inputs} x {taps}", args)
        assert f"{inputs} x {taps} = {inputs * taps}" in m and "registers" in m and "llz_adapt_bands_matrix_mc" in m and "64" in m \
            and "1..32" not in m, m
    for v in (0.0, -0.5, 1.5, float("nan")):
        seen["a"] = refused(L, f"a {v}", with_arg(4, v))
        assert " a " in seen["a"] and "at most 1" in seen["a"]
    for v in (-0.1, 1.0, float("nan")):
        seen["lam"] = refused(L, f"lam {v}", with_arg(5, v))
        assert "lam" in seen["lam"] and "below 1" in seen["lam"]
    for v in (0.0, -1.0, float("inf"), float("nan")):
        seen["p0"] = refused(L, f"p0 {v}", with_arg(6, v))
        assert "p0" in seen["p0"] and "finite" in seen["p0"]
    for v in (0.0, -1.0, float("inf"), float("nan")):
        seen["delta"] = refused(L, f"delta {v}", with_arg(7, v))
        assert "delta" in seen["delta"] and "finite" in seen["delta"]
    kinds = [re.sub(r"-?\d+(\.\d+)?|nan|inf", "#", m) for m in seen.values()]
    assert len(set(kinds)) == len(kinds) == 9, kinds
    # a, lam, p0 and delta are refused in llz_kalman_bands_mc_init's words
    for index, v in ((3, 0.0), (4, 1.0), (5, 0.0), (6, 0.0)):
        args = list(GOOD[1:])
        args[index] = v
        L.llz_kalman_bands_mc_init(*args)
        parent = capi.last_error().replace("llz_kalman_bands_mc_init", "llz_kalman_bands_matrix_mc_init")
        assert refused(L, f"parameter {index}", with_arg(index + 1, v)) == parent
    with pytest.raises(capi.LlzError, match="registers"):
        filters.KalmanBandsMatrixMC(3, 2, 33, 11)


def test_calls_refuse_a_bad_handle(L):
    f4, i5, n = (C.c_float * 64)(), (C.c_int * 5)(), C.c_longlong()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("_plan", lambda: L.llz_kalman_bands_matrix_mc_plan(h, i5)),
                           ("_reset", lambda: L.llz_kalman_bands_matrix_mc_reset(h, 1)),
                           ("_frames", lambda: L.llz_kalman_bands_matrix_mc_frames(h, C.byref(n))),
                           ("_set_stream", lambda: L.llz_kalman_bands_matrix_mc_set_stream(h, None)),
                           ("_set_adapt", lambda: L.llz_kalman_bands_matrix_mc_set_adapt(h, 0, 1, i5)),
                           ("_set_taps", lambda: L.llz_kalman_bands_matrix_mc_set_taps(h, 0, 1, 0, 1, f4, f4)),
                           ("_get_taps", lambda: L.llz_kalman_bands_matrix_mc_get_taps(h, 0, 1, 0, 1, f4, f4)),
                           ("_set_variance", lambda: L.llz_kalman_bands_matrix_mc_set_variance(h, 0, 1, 0, 1, f4)),
                           ("_get_variance", lambda: L.llz_kalman_bands_matrix_mc_get_variance(h, 0, 1, 0, 1, f4)),
                           ("_get_noise", lambda: L.llz_kalman_bands_matrix_mc_get_noise(h, 0, 1, f4)),
                           ("", lambda: L.llz_kalman_bands_matrix_mc(h, f4, f4, f4, f4, f4, f4, None, None, 1))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1 and (P + name + ":") in capi.last_error() and "bad handle" in capi.last_error(), name
        L.llz_kalman_bands_matrix_mc_uninit(h)


@pytest.mark.parametrize("inputs,bins,taps", [(1, 1, 1), (3, 129, 5), (8, 4097, 4), (2, 33, 16)])
def test_valid_init_without_gpu_fails_loudly(L, inputs, bins, taps):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a handle whose plan names the inputs and the entry ceiling
    and that other families' entry points refuse"""
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_kalman_bands_matrix_mc_init(inputs, 2, bins, taps, *GOOD[4:])
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        out = (C.c_int * 5)()
        assert L.llz_kalman_bands_matrix_mc_plan(h, out) == 0
        assert tuple(out) == (inputs, kx.ceiling(inputs, taps), 64, -(-2 * bins // 64), 1)
        assert L.llz_kalman_bands_mc_plan(h, out) < 0 and L.llz_adapt_bands_matrix_mc_plan(h, out) < 0 and L.llz_pfb_mc_bins(h) < 0
        L.llz_kalman_bands_matrix_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_kalman_bands_matrix_mc_init"):
            filters.KalmanBandsMatrixMC(inputs, 2, bins, taps)


def test_the_host_file_stands_on_the_core():
    """test_bands_core_host.py's rule for a fifth handle: the staged call, the counter, the range checks, the copies and the flag
    upload are the core's, no message of the core is repeated, no buffer is staged or classified here, the one fill is the
    shim's, and the handle has a tag of its own"""
    text = open(HOST_FILE).read()
    for call in ("llz_bands_begin(", "llz_bands_end(", "llz_bands_frames(", "llz_bands_refuse_count(", "llz_bands_refuse_range(",
                 "llz_bands_refuse_call(", "llz_bands_flags(", "llz_bands_copy(", "llz_bands_zero_pair(", "llz_bands_out(",
                 "LLZ_BANDS_XDEY(plane * (size_t)f->inputs, plane * (size_t)f->outputs)", "llzs_fill_f32(", "llz_adapt_refuse_delta("):
        assert call in text, call
    moved = ("outside %d..%d", "frames x bins below 2^31", "must both be NULL or both be set", "NULL buffer", "no out",
             "outside the handle's", "no device memory to stage", "(x) and %zu B", "no host memory for %zu B of %s", "outside 0..2",
             "is not a finite value", "llz_refuse_device_overlap", "llz_stage_in", "llz_stage_out", "llzs_is_device_ptr")
    for other in moved:
        assert other not in text, other
    values = re.findall(r"(LLZ_TAG_\w+) = (0x[0-9a-f]+)", open(os.path.join(CSRC, "host", "llz_host.h")).read())
    assert len({v for _, v in values}) == len(values) and "LLZ_TAG_KALX" in dict(values)
    assert set(re.findall(r"LLZ_TAG_\w+", text)) == {"LLZ_TAG_KALX"}


# ------------------------------------------------------------------------------------------------ the host layer under sanitizers
SCRIPT = (
    [("init", 3, 2, 33, 5)] + [("call", n, y) for n, y in ((0, 1), (1, 1), (1, 0), (7, 1), (50, 0), (0, 0))]
    + [("taps",), ("variance",), ("adapt",), ("call", 3, 1), ("fail", 4), ("call", 2, 0), ("fail", 1), ("call", 6, 0)]
    + [("reset", 0), ("call", 2, 0), ("reset", 1), ("call", 1, 1), ("call", 1, 1), ("reset", 0), ("reset", 1), ("call", 3, 0),
       ("taps",), ("variance",)]                                                                    # resets at either buffer
    + [("init", 1, 1, 1, 1), ("call", 1, 1), ("call", 33, 0), ("taps",), ("variance",), ("reset", 1), ("call", 2, 1)]   # one tap
    + [("init", 8, 3, 7, 1), ("call", 1, 1), ("call", 5, 0), ("variance",), ("taps",)]               # one tap of eight inputs
    + [("init", 8, 37, 129, 4), ("call", 2, 1), ("adapt",), ("call", 1, 0), ("fail", 20), ("call", 20, 1), ("taps",),
       ("variance",), ("reset", 1), ("call", 1, 1)]                                                 # 8 x 4 entries
    + [("init", 2, 1, 4097, 16), ("call", 0, 1), ("call", 3, 1), ("reset", 0), ("call", 1, 1), ("call", 40, 0)]   # the widest row
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
    the shim refuses between issued ones, sub-matrix set / get round trips of taps and variances with negative, NaN and infinite
    variances refused and nothing changed, get_noise, set_adapt, both resets at either buffer, one tap (no history), 8 x 4
    entries, the widest row.  Every launch reads the history the script fed and the header's float32 constants; the frame
    counter, the launches and the buffer read equal the script's line for line"""
    entry = "llzs_mkalman_bands_f32"
    text = gen_stub().splitlines()
    assert sum(ln.startswith(f"int {entry}(") for ln in text) == 1
    stub = tmp_path / "shim_stub.c"
    stub.write_text("\n".join(ln for ln in text if not ln.startswith(f"int {entry}(")) + "\n")       # the driver brings its own
    script = tmp_path / "script.txt"
    script.write_text("".join(" ".join(str(v) for v in cmd) + "\n" for cmd in SCRIPT))
    exe = tmp_path / "kalman_bands_matrix_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "kalman_bands_matrix_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "KALMAN_BANDS_MATRIX_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    got = [ln for ln in r.stdout.splitlines() if " frames " in ln]
    assert got == lines_of_script(SCRIPT)
    assert any(ln.endswith("read 1") for ln in got) and any(ln.startswith("reset") and ln.endswith("read 0") for ln in got)


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
def output_counts(shape):
    """the shape's own outputs and, where it is not the long row, kalman_bands_matrix_checks.OUTPUTS"""
    return sorted({shape[1]} | (set() if shape == kx.LONG else set(kx.OUTPUTS)))


@pytest.mark.parametrize("shape", kx.SHAPES + [kx.LONG], ids=lambda s: "x".join(map(str, s)))
def test_gpu_case_holds_on_the_model(oracle, shape):
    """the condition of the GPU list: the float32 model of the algorithm stays below a quarter of all four limits and keeps the
    zero bins, at the shape's own outputs and at 2 and 37.  Measured over all of them, the worst: e 0.047, w 0.027, P 0.116, psi
    0.031 of their limits"""
    inputs, _, taps, bins, frames = shape
    for outputs in output_counts(shape):
        kx.check_parity(kx.model32, oracle, inputs, outputs, taps, bins, frames, share=0.25)


def test_model_matches_the_definition_written_out(oracle):
    """the vectorised float64 model against the definition as plain loops over Python numbers, on a tiny case of 2 inputs x 3
    taps; a frozen output keeps w, P and psi and still filters, on a history that has moved on"""
    inputs, outputs, taps, bins, frames = 2, 2, 3, 5, 40
    x, d, _ = kx.case(oracle, inputs, outputs, taps, bins, frames)
    m = kx.Model(inputs, outputs, bins, taps, prec=64)
    e, y = m.process(x[:, :25], d[:, :25])
    m.set_adapt(1, 0)
    frozen = m.W[1].copy(), m.P[1].copy(), m.psi[1].copy()
    e2, y2 = m.process(x[:, 25:], d[:, 25:])
    assert all(np.array_equal(a, b) for a, b in zip((m.W[1], m.P[1], m.psi[1]), frozen)) and m.frames() == frames
    for k in (0, kx.ZERO_X, 4):
        ee, yy, ww, pp, psi = kx.definition_loops(x[:, :, k], d[0, :, k], taps)
        assert np.max(np.abs(np.concatenate([e[0, :, k], e2[0, :, k]]) - ee)) < 1e-12
        assert np.max(np.abs(np.concatenate([y[0, :, k], y2[0, :, k]]) - yy)) < 1e-12
        assert np.max(np.abs(m.W[0, :, :, k] - ww)) < 1e-12 and np.max(np.abs(m.P[0, :, :, k] - pp) / pp) < 1e-12
        assert abs(m.psi[0, k] - psi) <= 1e-12 * psi
    ee, yy, ww, pp, psi = kx.definition_loops(x[:, :25, 3], d[1, :25, 3], taps)
    assert np.max(np.abs(frozen[0][:, :, 3] - ww)) < 1e-12 and np.max(np.abs(frozen[1][:, :, 3] - pp) / pp) < 1e-12
    assert abs(frozen[2][3] - psi) <= 1e-12 * psi
    want = sum(ww[i, q] * x[i, 30 - q, 3] for q in range(taps) for i in range(inputs))
    assert abs(y2[1, 5, 3] - want) < 1e-12 and abs(e2[1, 5, 3] - (d[1, 30, 3] - want)) < 1e-12


@pytest.mark.parametrize("taps", [1, 5, 32])
def test_one_input_is_the_single_reference_model(oracle, taps):
    """the float32 model run with one input equals kalman_bands_checks.model32 fed that reference on every channel, bit for bit
    in e, y, w, P and psi: the matrix model's sums are the single model's with j in the place of q"""
    outputs, bins, frames = 3, 17, 60
    x, d, _ = kx.case(oracle, 1, outputs, taps, bins, frames)
    a = kx.model32(1, outputs, bins, taps)
    b = kc.model32(outputs, bins, taps)
    ea, ya = a.process(x, d)
    eb, yb = b.process(np.repeat(x, outputs, axis=0), d)
    assert np.array_equal(kx.cbits(ea), kx.cbits(eb)) and np.array_equal(kx.cbits(ya), kx.cbits(yb))
    assert np.array_equal(kx.cbits(a.get_taps()[:, 0]), kx.cbits(b.get_taps()))
    assert np.array_equal(a.get_variance()[:, 0].view(np.uint32), b.get_variance().view(np.uint32))
    assert np.array_equal(a.get_noise().view(np.uint32), b.get_noise().view(np.uint32))


def test_variances_stay_non_negative_in_float32():
    """the header's argument, seen on the float32 model where it is tightest: one tap of two strong references and a delta far
    below them, so that s is carried by the u and u r comes close to 1; P and psi never go below zero"""
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((2, 300, 64)) + 1j * rng.standard_normal((2, 300, 64))).astype(np.complex64) * np.float32(1e3)
    x[1, ::3] *= np.float32(1e-4)                               # every third frame one reference carries s alone
    d = (x[0] * np.complex64(0.5 - 0.25j) + x[1] * np.complex64(0.1j))[None]
    m = kx.Model(2, 1, 64, 1, delta=1e-6, prec=32)
    for o in range(0, 300, 10):
        m.process(x[:, o:o + 10], d[:, o:o + 10])
        assert np.all(m.P >= 0) and np.all(m.psi >= 0) and np.all(np.isfinite(m.P))


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault", kx.FAULTS)
def test_limits_see_a_planted_fault(oracle, fault):
    """the limits are not slack: each fault planted in the float32 model misses at least one of them, at 3 inputs x 3 taps (9
    entries: seven of the ceiling of 16 do not exist).  The first three are the matrix's own: s summed over the first reference
    only, weights and variances laid out [q][i], the last input a frame late.  Measured: 1.4e5, 5.1e6, 8.2e6, 40 and 1.5e4"""
    inputs, outputs, taps, bins, frames = kx.FAULT_SHAPE
    assert (inputs, taps) == (3, 3) and kx.ceiling(inputs, taps) > inputs * taps
    worst = kx.worst_miss(lambda *a: kx.Model(*a, prec=32, fault=fault), oracle, inputs, outputs, taps, bins, frames)
    print(f"planted fault {fault}: misses a limit by a factor of {worst:.3g}")
    assert worst > 1.0, fault


# ------------------------------------------------------------------------------------------------ double-talk
def test_double_talk_in_float64():
    """2 references x 4 taps, 33 bins, 900 frames of unit-variance bands, noise 40 dB below the echo, a near-end burst 10 dB above
    it over frames 500..599.  Behind the burst's last frame the joint Kalman model's misalignment is below the joint NLMS model's
    (mu = 0.5) in EVERY bin; behind the last frame the case's misalignment (the rms over the bins) is back below twice its value
    before the burst.  Both are conditions, not tuned numbers.  Measured: Kalman before / at the end of / after the burst, median
    (max) over the bins: 0.0088 (0.015) / 0.13 (0.28) / 0.0088 (0.014), rms over the bins 0.0095 before and 0.0094 after; NLMS
    0.0063 (0.0089) / 1.89 (2.8, its best bin 1.28) / 0.0060 (0.0085)."""
    kal, nlms, _ = kx.dt_float64()
    print(kx.dt_report("joint Kalman, float64", kal))
    print(kx.dt_report("joint NLMS mu = 0.5, float64", nlms))
    before, after = (float(np.sqrt(np.mean(kal[k] ** 2))) for k in (0, 2))
    print(f"Kalman: rms over the bins {before:.3g} before the burst, {after:.3g} behind the last frame; worst bin after / before "
          f"{np.max(kal[2] / kal[0]):.3g}; bins below NLMS at the burst's end: {int(np.sum(kal[1] < nlms[1]))} of {kal.shape[1]}")
    assert kal.shape == nlms.shape == (3, kx.DT["bins"]) and (kx.DT["inputs"], kx.DT["taps"]) == (2, 4)
    assert kx.DT_MARKS == (499, 599, 899) and kx.DT["burst"] == (500, 600) and kx.DT["frames"] == 900
    assert np.all(kal[1] < nlms[1]), "a bin ends the burst further from the echo paths than NLMS does"
    assert after < 2 * before, "the filter has not come back behind the burst"


def test_joint_filter_does_what_a_bank_of_single_ones_cannot():
    """the same case through two single-reference Kalman float64 models, each fed d: each takes the other reference's echo for
    near-end noise, its psi swallows that echo and its step closes.  The joint model's misalignment is below theirs in every bin
    at frames 499 and 899 (not asserted at 599, inside the burst's wake, where single bins cross).  Measured: the bank's median
    (max) over the bins 0.18 (0.25) at 499 and 0.16 (0.30) at 899, against 0.0088 (0.015) and 0.0088 (0.014); at 599 the joint
    model is below in 32 of 33 bins."""
    kal, _, singles = kx.dt_float64()
    print(kx.dt_report("a bank of single-reference Kalman models, float64", singles))
    print("bins in which the joint model is below the bank: " +
          ", ".join(f"frame {m}: {int(np.sum(kal[k] < singles[k]))} of {kal.shape[1]}" for k, m in enumerate(kx.DT_MARKS)))
    assert singles.shape == kal.shape
    assert np.all(kal[0] < singles[0]) and np.all(kal[2] < singles[2])


# ------------------------------------------------------------------------------------------------ the end-to-end case
def test_end_to_end_case_in_float64(oracle):
    """the case of the GPU suite's end-to-end test, through pfb_checks' float64 bank and the float64 model: behind a near-end
    burst the synthesised residual's rms over the last quarter is below a tenth of the synthesised d's on every output"""
    res = kx.e2e_float64(oracle)
    print("float64 chain: residual / d over the last quarter per output:", " ".join(f"{r:.3g}" for r in res))
    assert res.shape == (kx.E2E["outputs"],) and np.all(res < 0.1)
