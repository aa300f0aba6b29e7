"""CPU-side checks of the time-delay estimator (include/llz_tde.h, llz_tde_mc): the nine symbols exist in every layer with their
prototypes and pinned argtypes, every refusal that needs no device comes with a message naming its function, without a GPU a valid
init fails loudly, the frame grid's arithmetic, the host layer runs clean under AddressSanitizer + UBSan in a stand-alone driver
(tests/tde_sanitize_driver.c), and the limits of tests/tde_checks.py hold together: the float32 model stays inside them on every
GPU case, the float64 model finds every planted delay in every frame and meets the margin condition on every (pair, frame), and
each planted fault misses a limit by more than 1e2.  No kernel is launched here.  On the parent of this feature the library exports
none of the symbols and every test below that touches them fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import tde_checks as tk
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

PROTOTYPES = {
    "llz_tde_mc_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*const int \*\w+,\s*int \w+,\s*int \w+,\s*win_t \w+,\s*"
                       r"int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*float \w+,\s*float \w+\s*\)",
    "llz_tde_mc_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    "llz_tde_mc_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
    "llz_tde_mc_frames_for": r"\blong\s+%s\s*\(\s*unsigned long \w+,\s*long \w+\s*\)",
    "llz_tde_mc_process": r"\blong\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*long \w+,\s*float \*\w+,\s*float \*\w+,\s*"
                          r"long \w+\s*\)",
    "llz_tde_mc_frames": r"\blong\s+%s\s*\(\s*unsigned long \w+\s*\)",
    "llz_tde_mc_read": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*float \*\w+\s*\)",
    "llz_tde_mc_set_forget": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*float \w+\s*\)",
    "llz_tde_mc_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
}
ARGTYPES = {
    "llz_tde_mc_init": (C.c_ulong, [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_float, C.c_float]),
    "llz_tde_mc_uninit": (None, [C.c_ulong]),
    "llz_tde_mc_set_stream": (C.c_int, [C.c_ulong, C.c_void_p]),
    "llz_tde_mc_frames_for": (C.c_long, [C.c_ulong, C.c_long]),
    "llz_tde_mc_process": (C.c_long, [C.c_ulong, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_long]),
    "llz_tde_mc_frames": (C.c_long, [C.c_ulong]),
    "llz_tde_mc_read": (C.c_int, [C.c_ulong, C.c_int, C.c_void_p]),
    "llz_tde_mc_set_forget": (C.c_int, [C.c_ulong, C.c_float]),
    "llz_tde_mc_reset": (C.c_int, [C.c_ulong]),
}
NEW = list(PROTOTYPES)
FAULT_CASES = [0, 2, 4, 5, 6]


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no llz_tde_mc"
    return lib


def test_symbols_declared_bound_and_exported(L):
    raw = open(os.path.join(capi.INCLUDE_DIR, "llz_tde.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert set(re.findall(r"\b(llz_\w+)\s*\(", text)) == set(NEW)
    assert all(n in capi.declared_symbols() for n in NEW)
    for name, (res, args) in ARGTYPES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert re.search(r"enum\s*\{\s*LLZ_TDE_CC\s*=\s*0,\s*LLZ_TDE_PHAT,\s*LLZ_TDE_SCOT\s*\}", text)
    assert re.search(r"enum\s*\{\s*LLZ_TDE_CURVE\s*=\s*0,\s*LLZ_TDE_STATE\s*\}", text)
    assert (capi.TDE_CC, capi.TDE_PHAT, capi.TDE_SCOT) == (tk.CC, tk.PHAT, tk.SCOT) == (0, 1, 2)
    assert (capi.TDE_CURVE, capi.TDE_STATE) == (0, 1)
    # the header says that a NaN stays in the state until reset, and which way the sign goes
    assert re.search(r"NaN.*STAYS IN THE STATE.*until llz_tde_mc_reset", raw, flags=re.S) and "PEAKS AT tau = +D0" in raw
    shim = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "llz_shim.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(llzs_tde\w*)\s*\(", shim)) == {"llzs_tde_frames_f32"} and "int llzs_tde_frames_f32(" in gen_stub()
    for method in ("process", "frames_for", "frames", "curve", "state", "set_forget", "reset", "set_stream", "close"):
        assert hasattr(filters.TdeMC, method), method


def refused_init(L, what, channels=2, pairs=2, table=(0, 1, 1, 0), fft_len=256, hop=128, win=capi.HAMMING, max_lag=16,
                 weight=capi.TDE_PHAT, k_lo=1, k_hi=127, lam=0.9, delta=0.0):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    arr = (C.c_int * len(table))(*table) if table is not None else None
    assert L.llz_tde_mc_init(channels, pairs, arr, fft_len, hop, win, max_lag, weight, k_lo, k_hi, lam, delta) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_tde_mc_init" in msg, (what, msg)
    return msg


def test_init_refusals_carry_a_message(L):
    assert "channels 0" in refused_init(L, "channels", channels=0)
    assert "pairs 0" in refused_init(L, "pairs", pairs=0)
    refused_init(L, "no table", table=None)
    for n in (32, 8192, 384, 0, -256):
        assert f"fft_len {n}" in refused_init(L, "fft_len", fft_len=n, hop=n // 2) and "64..4096" in capi.last_error()
    for hop in (32, 0, -128, 255, 512):
        assert f"hop {hop}" in refused_init(L, "hop", hop=hop)
    assert "channel 1" in refused_init(L, "pair index high", channels=1)
    assert "channel -1" in refused_init(L, "pair index low", table=(0, 1, 1, -1)) and "pair 1" in capi.last_error()
    assert "unknown window 9" in refused_init(L, "window", win=9)
    for lag in (0, -1, 128, 4096):
        assert f"max_lag {lag}" in refused_init(L, "max_lag", max_lag=lag) and "1..127" in capi.last_error()
    for w in (-1, 3):
        assert f"weight {w}" in refused_init(L, "weight", weight=w)
    assert "k_lo -1" in refused_init(L, "k_lo", k_lo=-1)
    assert "k_lo 9 k_hi 8" in refused_init(L, "band order", k_lo=9, k_hi=8)
    assert "k_hi 129" in refused_init(L, "k_hi", k_hi=129)
    for lam in (1.0, -0.5, float("nan"), 1.5):
        assert "lam" in refused_init(L, "lam", lam=lam) and "[0, 1)" in capi.last_error()
    for delta in (-1.0, float("nan"), float("inf")):
        assert "delta" in refused_init(L, "delta", delta=delta)
    with pytest.raises(capi.LlzError, match="llz_tde_mc_init.*hop 100"):
        filters.TdeMC(2, [(0, 1)], 256, 100, 16)


def test_calls_refuse_a_foreign_handle_with_the_entry_point_named(L):
    buf = (C.c_float * 64)()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("llz_tde_mc_process", lambda: L.llz_tde_mc_process(h, buf, 64, buf, None, 64)),
                           ("llz_tde_mc_frames_for", lambda: L.llz_tde_mc_frames_for(h, 64)),
                           ("llz_tde_mc_frames", lambda: L.llz_tde_mc_frames(h)),
                           ("llz_tde_mc_read", lambda: L.llz_tde_mc_read(h, 0, buf)),
                           ("llz_tde_mc_set_forget", lambda: L.llz_tde_mc_set_forget(h, 0.5)),
                           ("llz_tde_mc_reset", lambda: L.llz_tde_mc_reset(h)),
                           ("llz_tde_mc_set_stream", lambda: L.llz_tde_mc_set_stream(h, None))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1, name
            assert name in capi.last_error() and "bad handle" in capi.last_error(), (name, capi.last_error())
        L.llz_tde_mc_uninit(h)


def test_valid_init_without_gpu_fails_loudly(L):
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    table = (C.c_int * 4)(0, 1, 1, 1)
    h = L.llz_tde_mc_init(2, 2, table, 256, 64, capi.HAMMING, 16, capi.TDE_PHAT, 1, 127, 0.9, 0.0)
    msg = capi.last_error()
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, msg
        buf = np.zeros(2 * 129 * 4, dtype=np.float32)
        assert L.llz_tde_mc_read(h, 0, buf.ctypes.data) == -1 and "no frame yet" in capi.last_error()
        assert L.llz_tde_mc_process(h, buf.ctypes.data, 65, buf.ctypes.data, None, 4) == -1 and "llz_tde_mc_process" in capi.last_error()
        L.llz_tde_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert msg not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_tde_mc_init"):
            filters.TdeMC(2, [(0, 1), (1, 1)], 256, 64, 16)


def test_host_layer_under_asan_ubsan(tmp_path, L):
    """the stand-alone driver over the stubbed device shim: nothing is loaded into python.  The driver checks frames_for, the
    frame counts and the untouched row tails against the integer model of the frame grid over ragged calls, reset and set_forget"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    exe = tmp_path / "tde_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "tde_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "TDE_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    assert len(re.findall(r"tde channels=\d+ pairs=\d+ fft_len=\d+ hop=\d+ ok", r.stdout)) == 8


# ------------------------------------------------------------------------------------------------ the GPU cases on the models
def test_case_table_covers_the_shapes():
    shapes = {(c[0], c[1]) for c in tk.CASES}
    assert {(64, 16), (256, 128), (1024, 256), (1024, 1024), (4096, 2048)} <= shapes
    assert {c[2] for c in tk.CASES} == {tk.CC, tk.PHAT, tk.SCOT}
    assert {len(c[5]) for c in tk.CASES} == {1, 3, 37}
    lags = {(c[3], c[0]) for c in tk.CASES}
    assert any(L == 1 for L, N in lags) and any(L == N // 8 for L, N in lags) and any(L == N // 2 - 1 for L, N in lags)
    assert any(c[4] == (0, c[0] // 2) for c in tk.CASES) and any(c[4][0] > 1 and c[4][1] < c[0] // 2 - 1 for c in tk.CASES)
    assert {c[7] for c in tk.CASES} == {12, 40} and all(c[6] == 0.8 for c in tk.CASES if c[7] == 40)
    assert all(any(tk.DSWITCH in p for p in c[5]) == (c[7] == 40) for c in tk.CASES)
    assert any(c[6] == 0.0 for c in tk.CASES)
    full = tk.CASES[0][5]
    assert full[tk.AUTO] == (tk.A, tk.A) and full[tk.REPEATED[0]] == full[tk.REPEATED[1]]
    assert full[tk.SWAP[0]] == full[tk.SWAP[1]][::-1] and (tk.A, tk.DFRAC) in full
    x = tk.signals(64, 16, 12)
    assert x.shape == (tk.CHANNELS, tk.samples(64, 16, 12)) and x.dtype == np.float32
    assert len({x[c].tobytes() for c in range(tk.CHANNELS)}) == tk.CHANNELS
    # the noise on y sits at 0.3 of the signal's level
    assert abs(np.std(x[tk.D0].astype(np.float64) - x[tk.A]) / np.std(x[tk.A].astype(np.float64)) - tk.NOISE) < 0.02


def test_sign_convention():
    """y[t] = x[t - D0] peaks at tau = +D0 in the float64 model"""
    N, hop, D0 = 256, 128, 7
    rng = np.random.default_rng(5)
    a = rng.standard_normal(N + 3 * hop + D0)
    x = np.stack([a[D0:], a[:-D0]] + 6 * [a[D0:]]).astype(np.float32)
    case = (N, hop, tk.PHAT, 20, (1, 127), [(0, 1), (1, 0)], 0.5, 4)
    ref = tk.model64(x, filters.window(tk.HAMMING, N).astype(np.float32), case)
    assert np.all(ref["tau"][:, 0] == D0) and np.all(ref["tau"][:, 1] == -D0)


def case_data(ci):
    case = tk.CASES[ci]
    N, hop = case[0], case[1]
    x = tk.signals(N, hop, case[7])
    w32 = filters.window(tk.window_of(N), N).astype(np.float32)
    return case, x, w32, tk.model64(x, w32, case)


@pytest.mark.parametrize("ci", range(len(tk.CASES)), ids=tk.CASE_IDS)
def test_gpu_cases_hold_on_the_float32_model(L, ci):
    """the float32 model inside every limit, the margin condition on every (pair, frame), the planted delays found by the
    float64 model in every frame"""
    case, x, w32, ref = case_data(ci)
    assert np.isfinite(ref["lim_r"]).all() and (ref["lim_r"] > 0).all() and (ref["lim_d"] < 1).all()
    tk.check(tk.model_f32(x, w32, case), ref, f"float32 model {tk.CASE_IDS[ci]}")
    pl = tk.planted(case[0])
    found = 0
    for p, (cx, cy) in enumerate(case[5]):
        if cx == tk.A and cy in pl and abs(pl[cy]) <= case[3]:
            assert np.all(ref["tau"][:, p] == pl[cy]), (p, ref["tau"][:, p])
            found += 1
        if (cx, cy) == (tk.A, tk.DFRAC):
            # (a parabola through a sinc peak 0.25 off the grid reads 0.143, not 0.25: the fraction is on the right side of the
            #  lag and away from both the lag and the half)
            assert np.all((ref["delay"][:, p] > 5.05) & (ref["delay"][:, p] < 5.45)), ref["delay"][:, p]
        if (cx, cy) == (tk.A, tk.DSWITCH):
            assert ref["tau"][0, p] == tk.SWITCH_FROM and ref["tau"][-1, p] == tk.SWITCH_TO
    assert found or any(tk.DSWITCH in p for p in case[5])


@pytest.mark.parametrize("fault", tk.FAULTS)
@pytest.mark.parametrize("ci", FAULT_CASES, ids=[tk.CASE_IDS[i] for i in FAULT_CASES])
def test_planted_faults_are_caught(L, ci, fault):
    """each fault misses a limit by more than 1e2: the limits are not loose"""
    case, x, w32, ref = cached_case(ci)
    r = tk.ratios(tk.model_f32(x, w32, case, fault=fault), ref)
    worst = max(r[k] for k in ("curve", "peak", "delay", "state"))
    print(f"{fault} {tk.CASE_IDS[ci]}: curve {r['curve']:.3g}, peak {r['peak']:.3g}, delay {r['delay']:.3g}, "
          f"state {r['state']:.3g} of their limits, {r['lags']} integer lags differ")
    assert worst > 1e2, r


_CASES = {}


def cached_case(ci):
    if ci not in _CASES:
        _CASES[ci] = case_data(ci)
    return _CASES[ci]


def test_frames_for_follows_the_frame_grid():
    """the arithmetic llz_tde_mc_frames_for and the kernel's frame walk rest on: frames after h hops = max(0, h - (N / hop - 1)),
    and the samples a call's frames cover stay inside history + x (the driver runs the C side of it under the sanitizers)"""
    for N, hop in ((64, 16), (256, 128), (1024, 1024)):
        lead, keep = N // hop - 1, N - hop
        hops = 0
        for call in (1, 1, 2, 5, 1, 9):
            lo, hi = max(0, hops - lead), max(0, hops + call - lead)
            n = call * hop
            for f in range(lo, hi):
                t0 = (f - hops) * hop
                assert -keep <= t0 and t0 + N <= n
            hops += call
        assert max(0, hops - lead) == hops - lead
