"""CPU-side checks of the per-band postfilter (include/llz_suppress_bands.h, llz_suppress_bands_mc): the symbols exist in every
layer with their prototypes, every init refusal comes with a message of its own, every call refuses a bad handle, without a GPU a
valid init fails loudly, the host layer runs scripted streams clean under AddressSanitizer + UBSan in a stand-alone driver
(tests/suppress_bands_sanitize_driver.c) whose frame counters equal the script's, the numpy float32 model of the algorithm
(tests/suppress_bands_checks.py) stays below half of every limit on every GPU case, the models equal the definition written out as
loops, five planted faults each miss a limit by more than 1e3, the header's invariants hold on the float32 model, and the
properties hold on the float64 model.  No kernel is launched here.  On the parent of this feature the library exports no
llz_suppress_bands_mc and every test below fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import suppress_bands_checks as sc
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

P = "llz_suppress_bands_mc"
RANGE = r"\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*"
PROTOTYPES = {
    P + "_default_cfg": r"\bvoid\s+%s\s*\(\s*llz_suppress_cfg \*\w+\s*\)",
    P + "_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*const llz_suppress_cfg \*\w+\s*\)",
    P + "_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P: r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*const float \*\w+,\s*const float \*\w+,\s*const float \*\w+,"
       r"\s*float \*\w+,\s*float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
    P + "_set_floor": r"\bint\s+%s" + RANGE + r"const float \*\w+\s*\)",
    P + "_set_leak": r"\bint\s+%s" + RANGE + r"const float \*\w+\s*\)",
    P + "_set_enable": r"\bint\s+%s" + RANGE + r"const int \*\w+\s*\)",
    P + "_get_state": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*float \*\w+\s*\)",
    P + "_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P + "_frames": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*long long \*\w+\s*\)",
    P + "_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\[4\]\s*\)",
    P + "_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
}
NEW = list(PROTOTYPES)
SHIMS = {"llzs_suppress_bands_f32", "llzs_suppress_bands_plan"}
FIELDS = ("window", "as_", "aq", "ad", "t0", "t1", "beta", "rho", "delta")


@pytest.fixture(scope="module", autouse=True)
def L():
    """the library with the feature in it: every test of this file, the models' own included, stands on it"""
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no per-band postfilter"
    return lib


def default_cfg(L, **kw):
    cfg = filters.SuppressCfg()
    L.llz_suppress_bands_mc_default_cfg(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_symbols_declared_bound_and_exported(L):
    raw = open(os.path.join(capi.INCLUDE_DIR, "llz_suppress_bands.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert len(NEW) == 12
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert set(re.findall(r"\b(llz_\w+)\s*\(", text)) == set(NEW)
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in NEW)
    assert all(getattr(L, n).argtypes is not None for n in NEW)
    for name, value in zip(("S", "SMIN", "STMP", "Q", "N", "R", "Z", "STATES"), range(8)):
        assert re.search(r"\bLLZ_SUPPRESS_%s = %d\b" % (name, value), text), name
    for fn in ("llz_adapt_bands.h", "llz_adapt_bands_matrix.h", "llz_kalman_bands.h"):
        assert "llz_suppress" not in open(os.path.join(capi.INCLUDE_DIR, fn)).read(), fn
    shim = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "llz_shim.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(llzs_suppress\w*)\s*\(", shim)) == SHIMS
    assert all(("int " + n + "(") in gen_stub() for n in SHIMS)
    for method in ("process", "set_floor", "set_leak", "set_enable", "get_state", "reset", "frames", "plan", "set_stream", "close"):
        assert hasattr(filters.SuppressBandsMC, method), method
    assert filters.SuppressBandsMC.STATES == sc.STATES


def test_default_cfg_and_the_struct(L):
    """the defaults are the header's, and the Python struct has the header's fields in the header's order"""
    cfg = default_cfg(L)
    want = dict(sc.DEFAULTS)
    assert cfg.window == want.pop("window")
    for k, v in want.items():
        assert getattr(cfg, k) == np.float32(v), k
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, "llz_suppress_bands.h")).read(), flags=re.S)
    body = re.search(r"typedef struct llz_suppress_cfg \{(.*?)\} llz_suppress_cfg;", text, flags=re.S).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert tuple(n + "_" if n == "as" else n for n in names) == FIELDS == tuple(f[0] for f in filters.SuppressCfg._fields_)
    L.llz_suppress_bands_mc_default_cfg(None)


def refused(L, what, channels, bins, **kw):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert L.llz_suppress_bands_mc_init(channels, bins, C.byref(default_cfg(L, **kw))) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_suppress_bands_mc_init" in msg, (what, msg)
    return msg


def test_init_refusals_carry_a_message(L):
    """each refusal names the init and what it missed, and no two kinds of refusal share a message"""
    seen = {}
    nan, inf = float("nan"), float("inf")
    for v in (0, -1, 65536):
        seen["channels"] = refused(L, f"channels {v}", v, 33)
        assert "1..65535" in seen["channels"] and f"channels {v}" in seen["channels"]
    for v in (0, -5, 4098):
        seen["bins"] = refused(L, f"bins {v}", 2, v)
        assert "1..4097" in seen["bins"] and f"bins {v}" in seen["bins"]
    for v in (1, 0, -3, 65536):
        seen["window"] = refused(L, f"window {v}", 2, 33, window=v)
        assert "2..65535" in seen["window"] and f"window {v}" in seen["window"]
    for name in ("as_", "aq", "ad", "beta", "rho"):
        for v in (1.0, -0.1, 1.5, nan):
            seen[name] = refused(L, f"{name} {v}", 2, 33, **{name: v})
            assert f" {name.rstrip('_')} " in seen[name] and "below 1" in seen[name]
    for t0, t1 in ((0.0, 5.0), (-1.0, 5.0), (5.0, 5.0), (6.0, 5.0), (nan, 5.0), (2.0, nan), (2.0, inf)):
        seen["t"] = refused(L, f"t0 {t0} t1 {t1}", 2, 33, t0=t0, t1=t1)
        assert "t0" in seen["t"] and "t0 < t1" in seen["t"]
    for v in (0.0, -1.0, inf, nan):
        seen["delta"] = refused(L, f"delta {v}", 2, 33, delta=v)
        assert "delta" in seen["delta"] and "finite" in seen["delta"]
    kinds = [re.sub(r"-?\d+(\.\d+)?(e-?\d+)?|nan|inf", "#", m) for m in seen.values()]
    assert len(set(kinds)) == len(kinds) == 10, kinds
    with pytest.raises(capi.LlzError, match="window 1 "):
        filters.SuppressBandsMC(2, 33, window=1)


def test_calls_refuse_a_bad_handle(L):
    f4, i4, n = (C.c_float * 64)(), (C.c_int * 4)(), C.c_longlong()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("_plan", lambda: L.llz_suppress_bands_mc_plan(h, i4)),
                           ("_reset", lambda: L.llz_suppress_bands_mc_reset(h)),
                           ("_frames", lambda: L.llz_suppress_bands_mc_frames(h, C.byref(n))),
                           ("_set_stream", lambda: L.llz_suppress_bands_mc_set_stream(h, None)),
                           ("_set_enable", lambda: L.llz_suppress_bands_mc_set_enable(h, 0, 1, i4)),
                           ("_set_floor", lambda: L.llz_suppress_bands_mc_set_floor(h, 0, 1, f4)),
                           ("_set_leak", lambda: L.llz_suppress_bands_mc_set_leak(h, 0, 1, f4)),
                           ("_get_state", lambda: L.llz_suppress_bands_mc_get_state(h, 0, 0, 1, f4)),
                           ("", lambda: L.llz_suppress_bands_mc(h, f4, f4, None, None, f4, f4, None, 1))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1 and (P + name + ":") in capi.last_error() and "bad handle" in capi.last_error(), name
        L.llz_suppress_bands_mc_uninit(h)


@pytest.mark.parametrize("bins,window", [(1, 2), (129, 128), (4097, 65535)])
def test_valid_init_without_gpu_fails_loudly(L, bins, window):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a handle with a plan that another family's entry point
    refuses"""
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_suppress_bands_mc_init(2, bins, C.byref(default_cfg(L, window=window)))
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        out = (C.c_int * 4)()
        assert L.llz_suppress_bands_mc_plan(h, out) == 0 and tuple(out) == (0, 64, -(-2 * bins // 64), 1)
        assert L.llz_kalman_bands_mc_plan(h, out) < 0 and L.llz_pfb_mc_bins(h) < 0
        L.llz_suppress_bands_mc_uninit(h)
        h = L.llz_suppress_bands_mc_init(2, bins, None)         # a NULL cfg: the defaults
        assert h != capi.BAD_HANDLE, capi.last_error()
        L.llz_suppress_bands_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_suppress_bands_mc_init"):
            filters.SuppressBandsMC(2, bins, window=window)


# ------------------------------------------------------------------------------------------------ the host layer under sanitizers
SCRIPT = (
    [("init", 3, 33, 16)] + [("call", n, y, g) for n, y, g in ((0, 1, 1), (1, 1, 1), (1, 0, 0), (7, 1, 0), (50, 0, 1), (0, 0, 0))]
    + [("floor",), ("leak",), ("enable",), ("state",), ("call", 3, 1, 1), ("reset",), ("call", 2, 0, 0), ("state",)]
    + [("init", 2, 1, 2), ("call", 1, 1, 1), ("call", 33, 0, 1), ("floor",), ("leak",), ("state",), ("reset",)]   # one bin, W = 2
    + [("init", 37, 129, 0), ("call", 2, 1, 1), ("enable",), ("call", 1, 0, 0), ("leak",), ("floor",), ("state",)]  # a NULL cfg
    + [("init", 1, 4097, 65535), ("call", 0, 1, 1), ("call", 3, 1, 1), ("reset",), ("call", 1, 1, 0), ("state",)]  # the widest row
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
    """the stand-alone driver over the stubbed device shim: refused configurations and calls, calls of 0, 1 and many frames with
    and without y and g on host buffers of exactly the stated sizes, floors and leakages with NaN, negative and too large values
    refused, set_enable, get_state of every value, resets, one bin, a NULL cfg, the widest row; the frame counter equals the
    script's line for line"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    script = tmp_path / "script.txt"
    script.write_text("".join(" ".join(str(v) for v in cmd) + "\n" for cmd in SCRIPT))
    exe = tmp_path / "suppress_bands_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "suppress_bands_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "SUPPRESS_BANDS_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    got = [ln for ln in r.stdout.splitlines() if " frames " in ln]
    assert got == counters_of_script(SCRIPT)


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
@pytest.mark.parametrize("channels", sc.CHANNELS)
@pytest.mark.parametrize("bins,frames,W", sc.SHAPES)
def test_gpu_case_holds_on_the_model(oracle, bins, frames, W, channels):
    """the float32 model of the algorithm stays below half of every limit and keeps the zero bin on every GPU case (measured: at
    most 0.18 of g's limit, 0.13 of o's, 0.09 of N's, below 0.05 of the others)"""
    sc.check_parity(sc.model32, oracle, bins, frames, W, channels, share=0.5)


@pytest.mark.parametrize("bins,frames,W", [sc.SHAPES[0], sc.SHAPES[2]])
def test_gpu_case_without_y_holds_on_the_model(oracle, bins, frames, W):
    m = sc.check_parity(sc.model32, oracle, bins, frames, W, 3, share=0.5, with_y=False, want_g=True)
    assert m["R"] == 0


def test_long_rows_hold_on_the_model(oracle):
    bins, frames, W, channels = sc.LONG
    sc.check_parity(sc.model32, oracle, bins, frames, W, channels, share=0.5)


def test_models_match_the_definition_written_out(oracle):
    """the vectorised float64 model against the definition as plain loops over Python numbers, on a tiny scene across n = W and
    three window swaps, in a plain, a burst and an echo bin; a disabled channel returns e, a gain of 1 and keeps its state while
    the count goes on"""
    bins, frames, W, channels = 9, 70, 16, 3
    e, y, eta = sc.scene(oracle, bins, frames, W, channels)
    m = sc.Model(channels, bins, window=W, prec=64)
    m.set_leak(0, eta)
    o, g = m.process(e[:, :25], y[:, :25])
    m.set_enable(1, 0)
    kept = {k: m.st[k][1].copy() for k in sc.STATES}
    o2, g2 = m.process(e[:, 25:], y[:, 25:])
    assert all(np.array_equal(m.st[k][1], kept[k]) for k in sc.STATES) and m.frames() == frames
    assert np.array_equal(o2[1], e[1, 25:].astype(np.complex128)) and np.all(g2[1] == 1)
    for c, k in ((0, 0), (0, sc.ZERO_BIN), (0, 4), (2, 8), (2, 3)):
        oo, gg, st = sc.definition_loops(e[c, :, k], y[c, :, k], eta=eta[c], window=W)
        assert np.max(np.abs(np.concatenate([o[c, :, k], o2[c, :, k]]) - oo)) < 1e-12
        assert np.max(np.abs(np.concatenate([g[c, :, k], g2[c, :, k]]) - gg)) < 1e-12
        for name in sc.STATES:
            assert abs(m.st[name][c, k] - st[name]) <= 1e-12 * max(abs(st[name]), 1e-30), (c, k, name)
    oo, gg, st = sc.definition_loops(e[1, :25, 3], y[1, :25, 3], eta=eta[1], window=W)
    assert all(abs(kept[name][3] - st[name]) <= 1e-12 * abs(st[name]) for name in sc.STATES)


def test_invariants_in_float32(oracle):
    """the header's arguments, seen on the float32 model where they are tightest: bands of 1e3 and of 1e-3 times unit level with
    the default delta, a floor of 0 and of 1; N >= 0, S >= 0, Q >= delta, 0 <= G <= 1, q in [0, 1] in every frame"""
    e, y, eta = sc.scene(oracle, 33, 300, 64, 3)
    for scale in (1e3, 1e-3):
        m = sc.model32(3, 33, window=64)
        m.set_leak(0, eta)
        m.set_floor(0, [0.0, 1.0, sc.GMIN])
        for at in range(0, 300, 10):
            _, g = m.process(e[:, at:at + 10] * np.complex64(scale), y[:, at:at + 10] * np.complex64(scale))
            assert np.all(g >= 0) and np.all(g <= 1) and np.all(g[1] == 1) and np.all(g[2] >= np.float32(sc.GMIN))
            assert all(np.all(m.st[k] >= 0) and np.all(np.isfinite(m.st[k])) for k in sc.STATES)
            assert np.all(m.st["q"] <= 1) and np.all((m.st["N"] + m.delta) + m.st["R"] >= m.delta)


def test_a_nan_stays_in_its_bin(oracle):
    """a NaN in one frame of one bin makes that bin's S and N NaN until reset and reaches nothing else"""
    e, y, eta = sc.scene(oracle, 33, 300, 64, 3)
    bad = e[:, :100].copy()
    bad[1, 40, 7] = np.nan
    a, b = sc.model32(3, 33, window=64), sc.model32(3, 33, window=64)
    oa, ga = a.process(e[:, :100])
    with np.errstate(invalid="ignore"):
        ob, gb = b.process(bad)
    assert np.isnan(b.st["S"][1, 7]) and np.isnan(b.st["N"][1, 7]) and np.all(np.isnan(ob[1, 40:, 7]))
    mask = np.ones((3, 33), bool)
    mask[1, 7] = False
    for k in sc.STATES:
        assert np.array_equal(a.st[k][mask], b.st[k][mask]), k
    for c in range(3):
        assert np.array_equal(oa[c][:, mask[c]], ob[c][:, mask[c]]) and np.array_equal(ga[c][:, mask[c]], gb[c][:, mask[c]])
    assert np.array_equal(oa[1, :40, 7], ob[1, :40, 7])
    b.reset()
    ob2, _ = b.process(e[:, :100])
    assert np.array_equal(oa, ob2)


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault", sc.FAULTS)
def test_limits_see_a_planted_fault(oracle, fault):
    """the limits are not slack: each fault planted in the float32 model misses at least one of them by more than 1e3 on the
    scene (measured: between 9e4 and 6e7)"""
    bins, frames, W = sc.SHAPES[1]
    worst = sc.worst_miss(lambda *a, **kw: sc.Model(*a, prec=32, fault=fault, **kw), oracle, bins, frames, W, 3)
    print(f"planted fault {fault}: misses a limit by a factor of {worst:.3g}")
    assert worst > 1e3, fault


# ------------------------------------------------------------------------------------------------ the properties
def test_properties_in_float64(oracle):
    """the property case at the defaults (W = 128, gmin = 0.1), figures of the float64 model, each asserted with a margin of 1 dB
    (0.05 for a gain):
      noise only, frames 300..699: the output lies 19.88 dB below the input (the floor bounds it at 20 dB);
      a burst 20 dB up over 40 frames in every 8th bin: median g 0.971 from its fifth frame on, 0.100 (the floor) 20 frames behind
        it, N in its bins at most 3.09 times its value before;
      a noise step of +10 dB: the median N is 1.05 dB below the new level 2 W frames behind it;
      the echo section's first W frames: 3.42 dB of attenuation at eta = 0, 19.97 dB at eta = 0.01."""
    f = sc.prop_float64(oracle)
    print("properties, float64 model: " + ", ".join(f"{k} {v:.4g}" for k, v in f.items()))
    for k, v in sc.PROP_FIGURES.items():
        assert abs(f[k] - v) <= 0.01 * max(abs(v), 1.0), (k, f[k], v)      # the figures written down are the model's
    sc.prop_check(f)
    sc.prop_check(sc.prop_figures(sc.model32(sc.PROP["channels"], sc.PROP["bins"]), oracle))
