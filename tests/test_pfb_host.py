"""CPU-side checks of the polyphase DFT filter bank (include/llz_pfb.h, llz_pfb_mc): the symbols exist in every layer with their
prototypes, the tune name is appended behind the ones that were there, every init refusal comes with a message of its own, every
call refuses a bad handle, without a GPU a valid init fails loudly, the host layer runs scripted streams clean under
AddressSanitizer + UBSan in a stand-alone driver (tests/pfb_sanitize_driver.c) whose frame counters equal the script's, the numpy
float32 model of the algorithm (tests/pfb_checks.py) stays inside the limits on every GPU case, and five planted faults each miss
them.  No kernel is launched here.  On the parent of this feature the library exports no llz_pfb_mc and every test below that
touches it fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import pfb_checks as pc
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

P = "llz_pfb_mc"
PROTOTYPES = {
    P + "_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*const float \*\w+,\s*const float \*\w+,\s*int \w+\s*\)",
    P + "_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P + "_bins": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P + "_delay": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P + "_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
    P + "_analysis": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
    P + "_synthesis": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*const float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
    P + "_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P + "_frames": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*long long \*\w+,\s*long long \*\w+\s*\)",
    P + "_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+\[8\]\s*\)",
}
NEW = list(PROTOTYPES)
W = np.ones(256, np.float32)
GOOD = (2, 64, 32, 4, W.ctypes.data, None, capi.PFB_PHASE_FRAME)       # channels, bands, hop, taps_per_band, w, g, phase


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no polyphase filter bank"
    return lib


def test_symbols_declared_bound_and_exported(L):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, "llz_pfb.h")).read(), flags=re.S)
    assert len(NEW) == 10
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert set(re.findall(r"\b(llz_\w+)\s*\(", text)) == set(NEW)
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in NEW)
    assert all(getattr(L, n).argtypes is not None for n in NEW)
    for fn in sorted(os.listdir(capi.INCLUDE_DIR)):
        if fn.endswith(".h") and fn != "llz_pfb.h":
            assert "llz_pfb" not in open(os.path.join(capi.INCLUDE_DIR, fn)).read(), fn
    shim = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "llz_shim.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(llzs_pfb\w*)\s*\(", shim)) == {"llzs_pfb_analysis_f32", "llzs_pfb_inverse_f32", "llzs_pfb_ola_f32",
                                                            "llzs_pfb_plan"}
    assert all(("int " + n + "(") in gen_stub() for n in ("llzs_pfb_analysis_f32", "llzs_pfb_inverse_f32", "llzs_pfb_ola_f32", "llzs_pfb_plan"))
    for method in ("analysis", "synthesis", "reset", "plan", "frames", "set_stream", "close"):
        assert hasattr(filters.PfbMC, method), method
    assert callable(filters.pfb_prototype) and (filters.PFB_PHASE_FRAME, filters.PFB_PHASE_TIME) == (0, 1)


def test_tune_is_appended(L):
    """behind the tunes that were there before it: their indices did not move"""
    names = []
    while L.llz_hip_tune_name(len(names)) is not None:
        names.append(L.llz_hip_tune_name(len(names)).decode())
    assert names[-1] == "pfb_global" and names.index("pfb_global") == names.index("asrc_table_global") + 1
    assert names.index("ols_wg_per_cu") == 0
    with capi.tuned(pfb_global=1):
        pass


def refused(L, what, args):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert L.llz_pfb_mc_init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_pfb_mc_init" in msg, (what, msg)
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
    for v in (0, 4, 48, 100, 8192, -64):
        seen["bands"] = refused(L, f"bands {v}", with_arg(1, v))
        assert "power of two in 8..4096" in seen["bands"] and f"bands {v}" in seen["bands"]
    for v in (0, -32, 4, 3, 48, 128):
        seen["hop"] = refused(L, f"hop {v}", with_arg(2, v))
        assert "1, 2, 4 or 8" in seen["hop"] and f"hop {v}" in seen["hop"]
    for v in (0, -1, 17):
        seen["taps"] = refused(L, f"taps_per_band {v}", with_arg(3, v))
        assert "1..16" in seen["taps"] and f"taps_per_band {v}" in seen["taps"]
    big = np.ones(16 * 4096, np.float32)
    for bands, taps in ((4096, 9), (4096, 16)):
        seen["length"] = refused(L, f"{bands} x {taps}", [2, bands, bands, taps, big.ctypes.data, None, 0])
        assert "32768" in seen["length"] and str(bands * taps) in seen["length"]
    seen["w"] = refused(L, "w NULL", with_arg(4, None))
    assert "NULL" in seen["w"] and "window" in seen["w"]
    for v in (-1, 2, 7):
        seen["phase"] = refused(L, f"phase {v}", with_arg(6, v))
        assert f"unknown phase {v}" in seen["phase"]
    kinds = [re.sub(r"-?\d+", "#", m) for m in seen.values()]
    assert len(set(kinds)) == len(kinds) == 7, kinds
    with pytest.raises(capi.LlzError, match="1, 2, 4 or 8"):
        filters.PfbMC(2, 64, 5, 1, np.ones(64, np.float32))
    with pytest.raises(capi.LlzError, match="holds 10 values"):
        filters.PfbMC(2, 64, 32, 1, np.ones(10, np.float32))


def test_calls_refuse_a_bad_handle(L):
    f4, i8 = (C.c_float * 64)(), (C.c_int * 8)()
    a, s = C.c_longlong(), C.c_longlong()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("llz_pfb_mc_plan", lambda: L.llz_pfb_mc_plan(h, 4, i8)),
                           ("llz_pfb_mc_reset", lambda: L.llz_pfb_mc_reset(h)),
                           ("llz_pfb_mc_bins", lambda: L.llz_pfb_mc_bins(h)),
                           ("llz_pfb_mc_delay", lambda: L.llz_pfb_mc_delay(h)),
                           ("llz_pfb_mc_frames", lambda: L.llz_pfb_mc_frames(h, C.byref(a), C.byref(s))),
                           ("llz_pfb_mc_set_stream", lambda: L.llz_pfb_mc_set_stream(h, None)),
                           ("llz_pfb_mc_analysis", lambda: L.llz_pfb_mc_analysis(h, f4, f4, f4, 1)),
                           ("llz_pfb_mc_synthesis", lambda: L.llz_pfb_mc_synthesis(h, f4, f4, f4, 1))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1 and name in capi.last_error(), name
        L.llz_pfb_mc_uninit(h)


@pytest.mark.parametrize("M,Pt,os", [(8, 1, 1), (1024, 8, 4), (4096, 8, 1)])
def test_valid_init_without_gpu_fails_loudly(L, M, Pt, os):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a handle with the header's bins and delay that another
    family's entry point refuses"""
    w = np.ones(M * Pt, np.float32)
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_pfb_mc_init(2, M, M // os, Pt, w.ctypes.data, None, capi.PFB_PHASE_TIME)
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        assert L.llz_pfb_mc_bins(h) == M // 2 + 1 and L.llz_pfb_mc_delay(h) == M * Pt - M // os
        assert L.llz_stft_mc_bins(h) < 0
        L.llz_pfb_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_pfb_mc_init"):
            filters.PfbMC(2, M, M // os, Pt, w)


# ------------------------------------------------------------------------------------------------ the host layer under sanitizers
SCRIPT = (
    [("init", 3, 64, 32, 4, 1, 1)] + [("analysis", n) for n in (0, 1, 7, 8, 9, 300)] + [("synthesis", n) for n in (1, 0, 7, 8, 9, 300)]
    + [("reset",), ("analysis", 5), ("synthesis", 2), ("analysis", 1)]
    + [("init", 2, 8, 8, 1, 0, 0), ("analysis", 1), ("synthesis", 1), ("analysis", 33), ("synthesis", 33)]       # no history at all
    + [("init", 37, 256, 32, 16, 1, 0), ("analysis", 127), ("synthesis", 128), ("synthesis", 129), ("reset",), ("synthesis", 1)]
    + [("init", 5, 4096, 4096, 8, 1, 1), ("synthesis", 3), ("analysis", 2)]                                       # the longest prototype
)


def counters_of_script(script):
    lines, a, s = [], 0, 0
    for cmd in script:
        if cmd[0] in ("init", "reset"):
            a = s = 0
            lines.append(f"{cmd[0]} 0 frames 0 0")
        else:
            a, s = (a + cmd[1], s) if cmd[0] == "analysis" else (a, s + cmd[1])
            lines.append(f"{cmd[0]} {cmd[1]} frames {a} {s}")
    return lines


def test_host_layer_under_asan_ubsan(tmp_path):
    """the stand-alone driver over the stubbed device shim: refused inits, calls of 0, 1 and many frames in both directions with
    host buffers of exactly the stated sizes, reset, a shape without history, R = 128 and the longest prototype;
    the frame counters equal the script's line for line"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    script = tmp_path / "script.txt"
    script.write_text("".join(" ".join(str(v) for v in cmd) + "\n" for cmd in SCRIPT))
    exe = tmp_path / "pfb_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "pfb_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "PFB_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    got = [ln for ln in r.stdout.splitlines() if " frames " in ln]
    assert got == counters_of_script(SCRIPT)


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
@pytest.mark.parametrize("phase", pc.PHASES)
@pytest.mark.parametrize("channels", pc.CHANNELS)
@pytest.mark.parametrize("M,Pt,os", pc.SHAPES)
def test_gpu_case_holds_on_the_model(M, Pt, os, channels, phase):
    """the float32 model of the algorithm stays inside the derived limits and the dense gate on every GPU case"""
    worst, dense = pc.check_analysis(pc.model_analysis_run(M, Pt, os, phase), channels, M, Pt, os, phase, "float32 model")
    assert worst <= 1.0 and dense <= pc.GATE
    worst, dense = pc.check_synthesis(pc.model_synthesis_run(M, Pt, os, phase), channels, M, Pt, os, phase, "float32 model")
    assert worst <= 1.0 and dense <= pc.GATE


def test_model_matches_the_definition_written_out():
    """the vectorised float64 reference against the definition's sums written as loops, on a small bank in TIME phase"""
    M, Pt, os, phase = 8, 3, 4, pc.TIME
    D, Lw, R = pc.geometry(M, Pt, os)
    w, g = pc.windows(M, Pt)
    frames = 2 * R + 3
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, frames * D)).astype(np.float32)
    X, _ = pc.analysis(x, w, M, Pt, os, phase)
    xs = lambda t: float(x[0, t]) if 0 <= t < x.shape[1] else 0.0
    for m in (0, 1, R - 1, R, frames - 1):
        s = (m + 1) * D - Lw
        for k in range(M // 2 + 1):
            want = sum(float(w[i]) * xs(s + i) * np.exp(-2j * np.pi * k * (s + i) / M) for i in range(Lw))
            assert abs(X[0, m, k] - want) < 1e-12 * Lw
    re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
    y, _ = pc.synthesis(re, im, g, M, Pt, os, phase)
    Xf = np.concatenate([re + 1j * im, np.conj(re + 1j * im)[:, :, -2:0:-1]], axis=2)[0]
    for q in range(frames * D):
        t, want = q - (Lw - D), 0.0
        for m in range(frames):
            i = t - ((m + 1) * D - Lw)
            if 0 <= i < Lw:
                rot = ((m + 1) * D) % M
                u = np.real(np.sum(Xf[m] * np.exp(2j * np.pi * np.arange(M) * ((i + rot) % M) / M)) / M)
                want += float(g[i]) * u
        assert abs(y[0, q] - want) < 1e-12 * Lw


# ------------------------------------------------------------------------------------------------ planted faults
FAULT_FACTOR = {"fold_stride": 1e3, "window_reversed": 1e3, "rotation_sign": 1e3, "frame_late": 1e3, "tail_order": 1e3}


@pytest.mark.parametrize("fault", pc.FAULTS)
def test_limits_see_a_planted_fault(fault):
    """the limits are not slack: each fault planted in the float32 model misses them by more than the stated factor"""
    M, Pt, os, channels, phase = 16, 3, 4, 3, pc.TIME            # (M / D = 4: a rotation of the wrong sign is another rotation)
    if fault == "tail_order":
        worst, _ = pc.check_synthesis(pc.model_synthesis_run(M, Pt, os, phase, fault), channels, M, Pt, os, phase, f"fault {fault}")
    elif fault == "rotation_sign":
        worst = max(pc.check_analysis(pc.model_analysis_run(M, Pt, os, phase, fault), channels, M, Pt, os, phase, f"fault {fault}")[0],
                    pc.check_synthesis(pc.model_synthesis_run(M, Pt, os, phase, fault), channels, M, Pt, os, phase, f"fault {fault}")[0])
    else:
        worst, _ = pc.check_analysis(pc.model_analysis_run(M, Pt, os, phase, fault), channels, M, Pt, os, phase, f"fault {fault}")
    print(f"planted fault {fault}: misses the limit by a factor of {worst:.3g}")
    assert worst > FAULT_FACTOR[fault], fault
