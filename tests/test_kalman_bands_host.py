"""CPU-side checks of the per-band Kalman filter (include/llz_kalman_bands.h, llz_kalman_bands_mc): the symbols exist in every
layer with their prototypes, every init refusal comes with a message of its own (33 taps included), every call refuses a bad
handle, without a GPU a valid init fails loudly, the host layer runs scripted streams clean under AddressSanitizer + UBSan in a
stand-alone driver (tests/kalman_bands_sanitize_driver.c) whose frame counters equal the script's, the numpy float32 model of the
algorithm (tests/kalman_bands_checks.py) stays below a quarter of every limit on every GPU case, the model equals the definition
written out as loops, five planted faults each miss a limit, and the double-talk property holds in float64.  No kernel is
launched here.  On the parent of this feature the library exports no llz_kalman_bands_mc and every test below fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import kalman_bands_checks as kc
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

P = "llz_kalman_bands_mc"
RANGE = r"\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*"
PROTOTYPES = {
    P + "_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*int \w+,\s*float \w+,\s*float \w+,\s*float \w+,\s*float \w+\s*\)",
    P + "_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P: r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*const float \*\w+,\s*const float \*\w+,\s*const float \*\w+,"
       r"\s*float \*\w+,\s*float \*\w+,\s*float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
    P + "_set_adapt": r"\bint\s+%s" + RANGE + r"const int \*\w+\s*\)",
    P + "_set_taps": r"\bint\s+%s" + RANGE + r"const float \*\w+,\s*const float \*\w+\s*\)",
    P + "_get_taps": r"\bint\s+%s" + RANGE + r"float \*\w+,\s*float \*\w+\s*\)",
    P + "_set_variance": r"\bint\s+%s" + RANGE + r"const float \*\w+\s*\)",
    P + "_get_variance": r"\bint\s+%s" + RANGE + r"float \*\w+\s*\)",
    P + "_get_noise": r"\bint\s+%s" + RANGE + r"float \*\w+\s*\)",
    P + "_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\s*\)",
    P + "_frames": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*long long \*\w+\s*\)",
    P + "_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\[4\]\s*\)",
    P + "_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
}
NEW = list(PROTOTYPES)
SHIMS = {"llzs_kalman_bands_f32", "llzs_kalman_bands_plan"}
GOOD = (2, 33, 8, 0.999, 0.9, 1.0, 1e-3)           # channels, bins, taps, a, lam, p0, delta


@pytest.fixture(scope="module", autouse=True)
def L():
    """the library with the feature in it: every test of this file, the models' own included, stands on it"""
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no per-band Kalman filter"
    return lib


def test_symbols_declared_bound_and_exported(L):
    raw = open(os.path.join(capi.INCLUDE_DIR, "llz_kalman_bands.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert len(NEW) == 13
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert set(re.findall(r"\b(llz_\w+)\s*\(", text)) == set(NEW)
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in NEW)
    assert all(getattr(L, n).argtypes is not None for n in NEW)
    for fn in ("llz_adapt_bands.h", "llz_adapt_bands_matrix.h"):
        assert "llz_kalman" not in open(os.path.join(capi.INCLUDE_DIR, fn)).read(), fn
    shim = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "llz_shim.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(llzs_kalman\w*)\s*\(", shim)) == SHIMS
    assert all(("int " + n + "(") in gen_stub() for n in SHIMS)
    for method in ("process", "set_adapt", "set_taps", "get_taps", "set_variance", "get_variance", "get_noise", "reset", "frames",
                   "plan", "set_stream", "close"):
        assert hasattr(filters.KalmanBandsMC, method), method


def refused(L, what, args):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert L.llz_kalman_bands_mc_init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_kalman_bands_mc_init" in msg, (what, msg)
    return msg


def with_arg(index, value):
    args = list(GOOD)
    args[index] = value
    return args


def test_init_refusals_carry_a_message(L):
    """each refusal names the init and what it missed, and no two kinds of refusal share a message; 33..64 taps, which the NLMS
    filter takes, have a message of their own"""
    seen = {}
    for v in (0, -1, 65536):
        seen["channels"] = refused(L, f"channels {v}", with_arg(0, v))
        assert "1..65535" in seen["channels"] and f"channels {v}" in seen["channels"]
    for v in (0, -5, 4098):
        seen["bins"] = refused(L, f"bins {v}", with_arg(1, v))
        assert "1..4097" in seen["bins"] and f"bins {v}" in seen["bins"]
    for v in (0, -1, 65):
        seen["taps"] = refused(L, f"taps {v}", with_arg(2, v))
        assert "1..32" in seen["taps"] and f"taps {v}" in seen["taps"]
    for v in (33, 64):
        seen["taps above 32"] = refused(L, f"taps {v}", with_arg(2, v))
        assert f"taps {v}" in seen["taps above 32"] and "registers" in seen["taps above 32"] and "1..32" not in seen["taps above 32"]
    for v in (0.0, -0.5, 1.5, float("nan")):
        seen["a"] = refused(L, f"a {v}", with_arg(3, v))
        assert " a " in seen["a"] and "at most 1" in seen["a"]
    for v in (-0.1, 1.0, float("nan")):
        seen["lam"] = refused(L, f"lam {v}", with_arg(4, v))
        assert "lam" in seen["lam"] and "below 1" in seen["lam"]
    for v in (0.0, -1.0, float("inf"), float("nan")):
        seen["p0"] = refused(L, f"p0 {v}", with_arg(5, v))
        assert "p0" in seen["p0"] and "finite" in seen["p0"]
    for v in (0.0, -1.0, float("inf"), float("nan")):
        seen["delta"] = refused(L, f"delta {v}", with_arg(6, v))
        assert "delta" in seen["delta"] and "finite" in seen["delta"]
    kinds = [re.sub(r"-?\d+(\.\d+)?|nan|inf", "#", m) for m in seen.values()]
    assert len(set(kinds)) == len(kinds) == 8, kinds
    with pytest.raises(capi.LlzError, match="registers"):
        filters.KalmanBandsMC(2, 33, 33)


def test_calls_refuse_a_bad_handle(L):
    f4, i4, n = (C.c_float * 64)(), (C.c_int * 4)(), C.c_longlong()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("_plan", lambda: L.llz_kalman_bands_mc_plan(h, i4)),
                           ("_reset", lambda: L.llz_kalman_bands_mc_reset(h, 1)),
                           ("_frames", lambda: L.llz_kalman_bands_mc_frames(h, C.byref(n))),
                           ("_set_stream", lambda: L.llz_kalman_bands_mc_set_stream(h, None)),
                           ("_set_adapt", lambda: L.llz_kalman_bands_mc_set_adapt(h, 0, 1, i4)),
                           ("_set_taps", lambda: L.llz_kalman_bands_mc_set_taps(h, 0, 1, f4, f4)),
                           ("_get_taps", lambda: L.llz_kalman_bands_mc_get_taps(h, 0, 1, f4, f4)),
                           ("_set_variance", lambda: L.llz_kalman_bands_mc_set_variance(h, 0, 1, f4)),
                           ("_get_variance", lambda: L.llz_kalman_bands_mc_get_variance(h, 0, 1, f4)),
                           ("_get_noise", lambda: L.llz_kalman_bands_mc_get_noise(h, 0, 1, f4)),
                           ("", lambda: L.llz_kalman_bands_mc(h, f4, f4, f4, f4, f4, f4, None, None, 1))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1 and (P + name + ":") in capi.last_error() and "bad handle" in capi.last_error(), name
        L.llz_kalman_bands_mc_uninit(h)


@pytest.mark.parametrize("bins,taps", [(1, 1), (129, 16), (4097, 32)])
def test_valid_init_without_gpu_fails_loudly(L, bins, taps):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a handle whose plan names the tap ceiling and that another
    family's entry point refuses"""
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_kalman_bands_mc_init(2, bins, taps, *GOOD[3:])
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        out = (C.c_int * 4)()
        assert L.llz_kalman_bands_mc_plan(h, out) == 0 and out[0] == kc.ceiling(taps) and out[3] == 1
        assert L.llz_adapt_bands_mc_plan(h, out) < 0 and L.llz_pfb_mc_bins(h) < 0
        L.llz_kalman_bands_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_kalman_bands_mc_init"):
            filters.KalmanBandsMC(2, bins, taps)


# ------------------------------------------------------------------------------------------------ the host layer under sanitizers
SCRIPT = (
    [("init", 3, 33, 5)] + [("call", n, y) for n, y in ((0, 1), (1, 1), (1, 0), (7, 1), (50, 0), (0, 0))]
    + [("taps",), ("variance",), ("adapt",), ("call", 3, 1), ("reset", 0), ("call", 2, 0), ("reset", 1), ("call", 1, 1), ("taps",)]
    + [("init", 2, 1, 1), ("call", 1, 1), ("call", 33, 0), ("taps",), ("variance",), ("reset", 1)]   # no history at all
    + [("init", 37, 129, 32), ("call", 2, 1), ("adapt",), ("call", 1, 0), ("variance",), ("taps",)]
    + [("init", 1, 4097, 17), ("call", 0, 1), ("call", 3, 1), ("reset", 0), ("call", 1, 1)]          # the widest row
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
    without y on host buffers of exactly the stated sizes, set / get round trips of taps and variances with negative, NaN and
    infinite variances refused, get_noise, set_adapt, both resets, one tap (no history), the widest row; the frame counter
    equals the script's line for line"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    script = tmp_path / "script.txt"
    script.write_text("".join(" ".join(str(v) for v in cmd) + "\n" for cmd in SCRIPT))
    exe = tmp_path / "kalman_bands_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "kalman_bands_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "KALMAN_BANDS_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    got = [ln for ln in r.stdout.splitlines() if " frames " in ln]
    assert got == counters_of_script(SCRIPT)


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
@pytest.mark.parametrize("channels", kc.CHANNELS)
@pytest.mark.parametrize("taps,bins,frames", kc.SHAPES)
def test_gpu_case_holds_on_the_model(oracle, taps, bins, frames, channels):
    """the float32 model of the algorithm stays below a quarter of every limit and keeps the zero bins on every GPU case"""
    kc.check_parity(kc.model32, oracle, taps, bins, frames, channels, share=0.25)


def test_long_rows_hold_on_the_model(oracle):
    taps, bins, frames, channels = kc.LONG
    kc.check_parity(kc.model32, oracle, taps, bins, frames, channels, share=0.25)


def test_model_matches_the_definition_written_out(oracle):
    """the vectorised float64 model against the definition as plain loops over Python numbers, on a tiny case; a frozen channel
    keeps w, P and psi and still filters"""
    taps, bins, frames, channels = 3, 5, 40, 2
    x, d, _ = kc.case(oracle, taps, bins, frames, channels)
    m = kc.Model(channels, bins, taps, prec=64)
    e, y = m.process(x[:, :25], d[:, :25])
    m.set_adapt(1, 0)
    frozen = m.W[1].copy(), m.P[1].copy(), m.psi[1].copy()
    e2, y2 = m.process(x[:, 25:], d[:, 25:])
    assert all(np.array_equal(a, b) for a, b in zip((m.W[1], m.P[1], m.psi[1]), frozen)) and m.frames() == frames
    for k in (0, kc.ZERO_X, 4):
        ee, yy, ww, pp, psi = kc.definition_loops(x[0, :, k], d[0, :, k], taps)
        assert np.max(np.abs(np.concatenate([e[0, :, k], e2[0, :, k]]) - ee)) < 1e-12
        assert np.max(np.abs(np.concatenate([y[0, :, k], y2[0, :, k]]) - yy)) < 1e-12
        assert np.max(np.abs(m.W[0, :, k] - ww)) < 1e-12 and np.max(np.abs(m.P[0, :, k] - pp) / pp) < 1e-12
        assert abs(m.psi[0, k] - psi) <= 1e-12 * psi
    ee, yy, ww, pp, psi = kc.definition_loops(x[1, :25, 3], d[1, :25, 3], taps)
    assert np.max(np.abs(frozen[0][:, 3] - ww)) < 1e-12 and np.max(np.abs(frozen[1][:, 3] - pp) / pp) < 1e-12
    want = sum(ww[q] * x[1, 30 - q, 3] for q in range(taps))
    assert abs(y2[1, 5, 3] - want) < 1e-12 and abs(e2[1, 5, 3] - (d[1, 30, 3] - want)) < 1e-12


def test_variances_stay_non_negative_in_float32(oracle):
    """the header's argument, seen on the float32 model where it is tightest: a single tap on a strong reference and a delta far
    below it, so that s = u in float32 and u r rounds to 1; P and psi never go below zero"""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((1, 300, 64)) + 1j * rng.standard_normal((1, 300, 64))).astype(np.complex64) * np.float32(1e3)
    m = kc.Model(1, 64, 1, delta=1e-6, prec=32)
    for o in range(0, 300, 10):
        m.process(x[:, o:o + 10], x[:, o:o + 10] * np.complex64(0.5 - 0.25j))
        assert np.all(m.P >= 0) and np.all(m.psi >= 0) and np.all(np.isfinite(m.P))


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault", kc.FAULTS)
def test_limits_see_a_planted_fault(oracle, fault):
    """the limits are not slack: each fault planted in the float32 model misses at least one of them (5 taps: three taps of the
    ceiling of 8 do not exist)"""
    taps, bins, frames = kc.SHAPES[2]
    assert kc.ceiling(taps) > taps
    worst = kc.worst_miss(lambda *a: kc.Model(*a, prec=32, fault=fault), oracle, taps, bins, frames, 3)
    print(f"planted fault {fault}: misses a limit by a factor of {worst:.3g}")
    assert worst > 1.0, fault


# ------------------------------------------------------------------------------------------------ double-talk
def test_double_talk_in_float64():
    """8 taps, 33 bins, 900 frames of unit-variance bands, noise 40 dB below the echo, a near-end burst 10 dB above it over frames
    500..599.  Behind the burst's last frame the Kalman model's misalignment is below the NLMS model's (mu = 0.5) in EVERY bin;
    behind the last frame the case's misalignment (the rms over the bins) is back below twice its value before the burst.  Both
    are conditions, not tuned numbers.  Measured: Kalman before / at the end of / after the burst, median (max) over the bins:
    0.0086 (0.014) / 0.15 (0.27) / 0.0099 (0.014), rms over the bins 0.0091 before and 0.0096 after; NLMS 0.0059 (0.0095) / 1.83
    (2.9, its best bin 0.87) / 0.0060 (0.0095)."""
    kal, nlms = kc.dt_float64()
    print(kc.dt_report("Kalman, float64", kal))
    print(kc.dt_report("NLMS mu = 0.5, float64", nlms))
    before, after = (float(np.sqrt(np.mean(kal[k] ** 2))) for k in (0, 2))
    print(f"Kalman: rms over the bins {before:.3g} before the burst, {after:.3g} behind the last frame; worst bin after / before "
          f"{np.max(kal[2] / kal[0]):.3g}; bins below NLMS at the burst's end: {int(np.sum(kal[1] < nlms[1]))} of {kal.shape[1]}")
    assert kal.shape == nlms.shape == (3, kc.DT["bins"])
    assert np.all(kal[1] < nlms[1]), "a bin ends the burst further from the echo path than NLMS does"
    assert after < 2 * before, "the filter has not come back behind the burst"
