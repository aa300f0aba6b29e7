"""CPU-side checks of the Welch cross-spectra (include/llz_spectral.h, llz_csd_mc): the ten symbols exist in every layer with
their prototypes and pinned argtypes, the tune is listed, every refusal that needs no device comes with a message naming its
function, without a GPU a valid init fails loudly, the host layer runs clean under AddressSanitizer + UBSan in a stand-alone
driver (tests/csd_sanitize_driver.c: init -> updates that start, continue and end runs -> slab walks -> read -> reset -> uninit),
and the limits of tests/csd_checks.py hold together: the plain float32 model stays within a quarter of them on every GPU case, and
each planted fault is caught.  No kernel is launched here.  On the parent of this feature the library exports none of the
symbols and every test below that touches them fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import csd_checks as cc
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

PROTOTYPES = {
    "llz_csd_mc_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*const int \*\w+,\s*int \w+,\s*int \w+,\s*win_t \w+\s*\)",
    "llz_csd_mc_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    "llz_csd_mc_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
    "llz_csd_mc_update": r"\blong\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*long \w+\s*\)",
    "llz_csd_mc_frames": r"\blong\s+%s\s*\(\s*unsigned long \w+\s*\)",
    "llz_csd_mc_read": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*float \*\w+\s*\)",
    "llz_csd_mc_read_raw": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*double \*\w+\s*\)",
    "llz_csd_mc_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
    "llz_csd_mc_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*long \w+,\s*int \w+\[4\]\s*\)",
}
ARGTYPES = {
    "llz_csd_mc_init": (C.c_ulong, [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int]),
    "llz_csd_mc_uninit": (None, [C.c_ulong]),
    "llz_csd_mc_set_stream": (C.c_int, [C.c_ulong, C.c_void_p]),
    "llz_csd_mc_update": (C.c_long, [C.c_ulong, C.c_void_p, C.c_long]),
    "llz_csd_mc_frames": (C.c_long, [C.c_ulong]),
    "llz_csd_mc_read": (C.c_int, [C.c_ulong, C.c_int, C.c_void_p]),
    "llz_csd_mc_read_raw": (C.c_int, [C.c_ulong, C.c_void_p]),
    "llz_csd_mc_reset": (C.c_int, [C.c_ulong]),
    "llz_csd_mc_plan": (C.c_int, [C.c_ulong, C.c_long, C.POINTER(C.c_int)]),
}
NEW = list(PROTOTYPES)
# (check, pair, fft_len) on which plain float32 does not stay within a quarter: the pooled gate on the tone pairs from 512 points
# on.  The gate holds an RMS over the bins to 1e-5 of a MEAN over the bins; a line spectrum has its power, and with it its
# rounding error, in a few bins of the N/2 + 1, which makes the gate sqrt(bins / lines) harsher than on noise and harsher with
# the size: the model reaches 0.06 of it at 64, 0.19 at 128, 0.14 at 256, and 0.26 at 512, 0.54 at 1024, 0.29 at 2048, 0.65 at 4096.
# At those four sizes the model is held to the whole gate on the tone pairs; everywhere else, and on the per-bin limit (which
# it meets at 3 %), to the quarter.  (The device's compensated sums stay below 0.14 of the gate at every size.)
GATE_QUARTER_MISSED = {(p, N) for p in (3, 4) for N in (512, 1024, 2048, 4096)}


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no llz_csd_mc"
    return lib


def test_symbols_declared_bound_and_exported(L):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, "llz_spectral.h")).read(), flags=re.S)
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert set(re.findall(r"\b(llz_\w+)\s*\(", text)) == set(NEW)
    assert all(n in capi.declared_symbols() for n in NEW)
    for name, (res, args) in ARGTYPES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert re.search(r"#define\s+LLZ_CSD_RUN\s+32\b", text) and capi.CSD_RUN == cc.RUN == 32
    assert re.search(r"enum\s*\{\s*LLZ_SPEC_PXX\s*=\s*0,\s*LLZ_SPEC_PYY,\s*LLZ_SPEC_CSD,\s*LLZ_SPEC_COHERENCE,\s*LLZ_SPEC_TF\s*\}", text)
    assert "two-sided" in open(os.path.join(capi.INCLUDE_DIR, "llz_spectral.h")).read().lower()
    for method in ("update", "frames", "psd_x", "psd_y", "csd", "coherence", "transfer", "raw", "reset", "plan", "set_stream",
                   "close"):
        assert hasattr(filters.CsdMC, method), method


def test_tune_is_appended(L):
    """behind the tunes that were there before it: their indices did not move"""
    names = []
    while L.llz_hip_tune_name(len(names)) is not None:
        names.append(L.llz_hip_tune_name(len(names)).decode())
    assert names.index("csd_scratch_kb") == names.index("ols_superblock") + 1 == 27
    with capi.tuned(csd_scratch_kb=64):
        pass


def refused_init(L, what, channels, pairs, table, fft_len, hop, win=capi.HAMMING):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    arr = (C.c_int * len(table))(*table) if table is not None else None
    assert L.llz_csd_mc_init(channels, pairs, arr, fft_len, hop, win) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_csd_mc_init" in msg, (what, msg)
    return msg


def test_init_refusals_carry_a_message(L):
    t = [0, 1, 1, 0]
    assert "channels 0" in refused_init(L, "channels", 0, 2, t, 256, 128)
    assert "pairs 0" in refused_init(L, "pairs", 2, 0, t, 256, 128)
    refused_init(L, "no table", 2, 2, None, 256, 128)
    for n in (32, 8192, 384, 0, -256):
        assert f"fft_len {n}" in refused_init(L, "fft_len", 2, 2, t, n, n // 2) and "64..4096" in capi.last_error()
    for hop in (32, 0, -128, 255, 512):
        assert f"hop {hop}" in refused_init(L, "hop", 2, 2, t, 256, hop)
    assert "channel 1" in refused_init(L, "pair index high", 1, 2, t, 256, 128)
    assert "channel -1" in refused_init(L, "pair index low", 2, 2, [0, 1, 1, -1], 256, 128) and "pair 1" in capi.last_error()
    assert "unknown window 9" in refused_init(L, "window", 2, 2, t, 256, 128, 9)
    with pytest.raises(capi.LlzError, match="llz_csd_mc_init.*hop 100"):
        filters.CsdMC(2, [(0, 1)], 256, 100)


def test_calls_refuse_a_foreign_handle_with_the_entry_point_named(L):
    buf = (C.c_float * 64)()
    raw = (C.c_double * 64)()
    plan = (C.c_int * 4)()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("llz_csd_mc_update", lambda: L.llz_csd_mc_update(h, buf, 64)),
                           ("llz_csd_mc_frames", lambda: L.llz_csd_mc_frames(h)),
                           ("llz_csd_mc_read", lambda: L.llz_csd_mc_read(h, 0, buf)),
                           ("llz_csd_mc_read_raw", lambda: L.llz_csd_mc_read_raw(h, raw)),
                           ("llz_csd_mc_reset", lambda: L.llz_csd_mc_reset(h)),
                           ("llz_csd_mc_plan", lambda: L.llz_csd_mc_plan(h, 64, plan)),
                           ("llz_csd_mc_set_stream", lambda: L.llz_csd_mc_set_stream(h, None))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1, name
            assert name in capi.last_error() and "bad handle" in capi.last_error(), (name, capi.last_error())
        L.llz_csd_mc_uninit(h)


def test_valid_init_without_gpu_fails_loudly(L):
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    table = (C.c_int * 4)(0, 1, 1, 1)
    h = L.llz_csd_mc_init(2, 2, table, 256, 64, capi.HAMMING)
    msg = capi.last_error()
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, msg
        buf = np.zeros(2 * 129, dtype=np.float32)
        assert L.llz_csd_mc_read(h, 0, buf.ctypes.data) == -1 and "no frame yet" in capi.last_error()
        assert L.llz_csd_mc_update(h, buf.ctypes.data, 65) == -1 and "llz_csd_mc_update" in capi.last_error()
        L.llz_csd_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert msg not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_csd_mc_init"):
            filters.CsdMC(2, [(0, 1), (1, 1)], 256, 64)


def test_host_layer_under_asan_ubsan(tmp_path, L):
    """the stand-alone driver over the stubbed device shim: nothing is loaded into python"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    exe = tmp_path / "csd_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "csd_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "CSD_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    assert len(re.findall(r"csd channels=\d+ pairs=\d+ fft_len=\d+ hop=\d+ ok", r.stdout)) == 8 and "csd slabs ok" in r.stdout


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
def test_case_table_covers_the_sizes():
    assert {c[0] for c in cc.CASES if not c[2]} == set(cc.SIZES) == {c[0] for c in cc.CASES if c[2]}
    for N in (256, 1024):
        assert {N // hop for n, hop, g in cc.CASES if n == N and not g} == {1, 2, 4}
    assert cc.K_FRAMES == 2 * cc.RUN + 3 and cc.samples(4096, 2048) < 150000
    kinds = {cc.PAIRS[p] for p in range(len(cc.PAIRS))}
    assert {(cc.A, cc.A), (cc.A, cc.B), (cc.B, cc.A), (cc.C_SIN, cc.D_COS), (cc.D_COS, cc.C_SIN), (cc.A, cc.E_ZERO),
            (cc.E_ZERO, cc.E_ZERO)} <= kinds and len(kinds) < len(cc.PAIRS)
    assert cc.PAIRS[cc.REPEATED[0]] == cc.PAIRS[cc.REPEATED[1]] and cc.PAIRS[cc.MINUS4_PAIR] == (cc.A, cc.A_M4)
    x = cc.signals(64, 16)
    assert x.shape == (cc.CHANNELS, cc.samples(64, 16)) and not x[cc.E_ZERO].any()
    assert len({x[c].tobytes() for c in range(cc.CHANNELS)}) == cc.CHANNELS
    assert np.array_equal(x[cc.A_HI], x[cc.A] * 1024) and np.array_equal(x[cc.A_LO], np.ldexp(x[cc.A], -20))


@pytest.mark.parametrize("N,hop", cc.SHAPES)
def test_gpu_cases_hold_on_the_float32_model(L, N, hop):
    """plain float32 within a quarter of the per-bin limit on every pair and of the gate on every pair but the tones from 512
    points on (GATE_QUARTER_MISSED: within the whole gate there)"""
    x = cc.signals(N, hop)
    w32 = filters.window(cc.window_of(N), N).astype(np.float32)
    ref, lim, gate = cc.reference(x, w32, N, hop)
    per_bin, pooled = cc.ratios(cc.model_f32(x, w32, N, hop), ref, lim, gate)
    print(f"float32 model {N}/{hop}: {per_bin.max():.3g} of the per-bin limit, {pooled.max():.3g} of the gate")
    assert per_bin.max() <= 0.25, per_bin
    for p in range(len(cc.PAIRS)):
        assert pooled[p] <= (1.0 if (p, N) in GATE_QUARTER_MISSED else 0.25), (p, pooled[p])


@pytest.mark.parametrize("fault", cc.FAULTS)
@pytest.mark.parametrize("N,hop", [(64, 16), (256, 64), (1024, 512), (4096, 2048)])
def test_planted_faults_are_caught(L, N, hop, fault):
    """each fault misses the gate on the correlated noise pair and the per-bin limit on the sine / cosine pair"""
    x = cc.signals(N, hop)
    w32 = filters.window(cc.window_of(N), N).astype(np.float32)
    ref, lim, gate = cc.reference(x, w32, N, hop)
    per_bin, pooled = cc.ratios(cc.model_f32(x, w32, N, hop, fault=fault), ref, lim, gate)
    print(f"{fault} {N}/{hop}: noise pair {pooled[cc.NOISE_PAIR]:.3g} of the gate, tone pair {per_bin[cc.TONE_PAIR]:.3g} of the limit")
    assert pooled[cc.NOISE_PAIR] > 1.0 and per_bin[cc.TONE_PAIR] > 1.0


def test_model_sums_do_not_depend_on_the_grid_origin():
    """the model's runs sit on the absolute frame grid, as the handle's do: the conjugate pair and the repeated pair are exact"""
    N, hop = 128, 64
    x = cc.signals(N, hop)
    w32 = filters.window(cc.window_of(N), N).astype(np.float32)
    m = cc.model_f32(x, w32, N, hop)
    a, b = cc.CONJ_PAIRS
    assert np.array_equal(m[a][:, [1, 0, 2]], m[b][:, [0, 1, 2]]) and np.array_equal(m[a][:, 3], -m[b][:, 3])
    assert np.array_equal(m[cc.REPEATED[0]], m[cc.REPEATED[1]])
    for p in cc.AUTO_PAIRS:
        assert np.array_equal(m[p][:, 2], m[p][:, 0]) and not m[p][:, 3].any()
