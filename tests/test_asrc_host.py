"""CPU-side checks of the arbitrary-ratio resampler (include/llz_asrc.h, llz_asrc_mc): the eleven symbols exist in every layer with
their prototypes and no other family's name set grows, every init refusal comes with a message of its own naming the range it
missed, every call refuses a bad handle, without a GPU a valid init fails loudly, the host layer runs scripted streams clean
under AddressSanitizer + UBSan in a stand-alone driver (tests/asrc_sanitize_driver.c) whose counts and times equal the integer
model's, the numpy float32 model of the definition (tests/asrc_checks.py) passes the limits of the GPU cases, and five planted
faults each miss them.  No kernel is launched here.  On the parent of this feature the library exports no llz_asrc_mc and every
test below that touches it fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import asrc_checks as ac
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

P = "llz_asrc_mc"
PROTOTYPES = {
    P + "_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*int \w+,\s*int \w+,\s*double \w+,\s*double \w+,\s*win_t \w+,\s*double \w+\s*\)",
    P + "_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P + "_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
    P: r"\blong\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*long \w+,\s*float \*\w+,\s*long \w+,\s*int \*\w+\s*\)",
    P + "_out_len": r"\blong\s+%s\s*\(\s*unsigned long \w+,\s*long \w+,\s*int \*\w+\s*\)",
    P + "_set_step": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*const double \*\w+,\s*long \w+\s*\)",
    P + "_get_step": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*double \*\w+,\s*long \*\w+\s*\)",
    P + "_next_time": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+,\s*long long \*\w+,\s*unsigned int \*\w+\s*\)",
    P + "_get_table": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*float \*\w+,\s*int \w+\s*\)",
    P + "_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
    P + "_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+\[4\]\s*\)",
}
NEW = list(PROTOTYPES)
GOOD = (2, 1000, 32, 512, 0.9, 1.0, capi.KAISER, 1.0)      # channels, frame_len, taps, phases, cutoff, gain, win, step


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no arbitrary-ratio resampler"
    return lib


def test_symbols_declared_bound_and_exported(L):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, "llz_asrc.h")).read(), flags=re.S)
    assert len(NEW) == 11
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert set(re.findall(r"\b(llz_\w+)\s*\(", text)) == set(NEW)
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in NEW)
    assert all(getattr(L, n).argtypes is not None for n in NEW)
    # no other family's set grows: the new names are in no other header, and none starts with another family's prefix
    for fn in sorted(os.listdir(capi.INCLUDE_DIR)):
        if fn.endswith(".h") and fn != "llz_asrc.h":
            assert "llz_asrc" not in open(os.path.join(capi.INCLUDE_DIR, fn)).read(), fn
    assert not any(n.startswith(p) for n in NEW for p in ("llz_resample", "llz_fir_", "llz_adapt_", "llz_hip_"))
    shim = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "llz_shim.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(llzs_asrc\w*)\s*\(", shim)) == {"llzs_asrc_f32", "llzs_asrc_advance"}
    for method in ("process", "out_len", "set_step", "next_time", "table", "reset", "plan", "set_stream", "close"):
        assert hasattr(filters.AsrcMC, method), method


def test_tune_is_appended(L):
    """behind the tunes that were there before it: their indices did not move"""
    names = []
    while L.llz_hip_tune_name(len(names)) is not None:
        names.append(L.llz_hip_tune_name(len(names)).decode())
    assert names.index("asrc_table_global") == names.index("adapt_ppw") + 1
    with capi.tuned(asrc_table_global=1):
        pass


def refused(L, what, args):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert L.llz_asrc_mc_init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_asrc_mc_init" in msg, (what, msg)
    return msg


def with_arg(index, value):
    args = list(GOOD)
    args[index] = value
    return args


def test_init_refusals_carry_a_message(L):
    """(channels, frame_len, taps, phases, cutoff, gain, win, step): each refusal names the init and the range it missed, and
    no two kinds of refusal share a message"""
    seen = {}
    for v in (0, -3, 65536):
        seen["channels"] = refused(L, f"channels {v}", with_arg(0, v))
        assert "1..65535" in seen["channels"] and f"channels {v}" in seen["channels"]
    for v in (0, -1, (1 << 22) + 1):
        seen["frame_len"] = refused(L, f"frame_len {v}", with_arg(1, v))
        assert "1..4194304" in seen["frame_len"] and f"frame_len {v}" in seen["frame_len"]
    for v in (0, 2, 3, 33, 130, 129):
        seen["taps"] = refused(L, f"taps {v}", with_arg(2, v))
        assert "4..128" in seen["taps"] and "even" in seen["taps"] and f"taps {v}" in seen["taps"]
    for v in (0, 128, 384, 513, 8192):
        seen["phases"] = refused(L, f"phases {v}", with_arg(3, v))
        assert "256..4096" in seen["phases"] and "power of two" in seen["phases"] and f"phases {v}" in seen["phases"]
    for v in (0.0, -0.5, 1.0001, float("nan"), float("inf")):
        seen["cutoff"] = refused(L, f"cutoff {v}", with_arg(4, v))
        assert "cutoff" in seen["cutoff"] and "(0, 1]" in seen["cutoff"]
    for v in (0.0, float("nan"), float("inf"), -float("inf")):
        seen["gain"] = refused(L, f"gain {v}", with_arg(5, v))
        assert "gain" in seen["gain"] and "finite" in seen["gain"]
    for v in (-1, 3, 9):
        seen["win"] = refused(L, f"window {v}", with_arg(6, v))
        assert f"unknown window {v}" in seen["win"]
    for v in (0.0, 0.0624, 16.0001, -1.0, float("nan"), float("inf")):
        seen["step"] = refused(L, f"step {v}", with_arg(7, v))
        assert "step" in seen["step"] and "1/16..16" in seen["step"]
    kinds = [re.sub(r"-?\d+(\.\d+)?(e[-+]?\d+)?|nan|inf", "#", m) for m in seen.values()]
    assert len(set(kinds)) == len(kinds) == 8, kinds
    with pytest.raises(capi.LlzError, match="4..128"):
        filters.AsrcMC(2, 100, taps=5)
    with pytest.raises(capi.LlzError, match="1/16..16"):
        filters.AsrcMC(2, 100, step=17.0)


def test_calls_refuse_a_bad_handle(L):
    f4, i4, d4 = (C.c_float * 64)(), (C.c_int * 4)(), (C.c_double * 4)()
    l4, ll4, u4 = (C.c_long * 4)(), (C.c_longlong * 4)(), (C.c_uint * 4)()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("llz_asrc_mc_plan", lambda: L.llz_asrc_mc_plan(h, i4)),
                           ("llz_asrc_mc_reset", lambda: L.llz_asrc_mc_reset(h)),
                           ("llz_asrc_mc_set_step", lambda: L.llz_asrc_mc_set_step(h, 0, 1, d4, 0)),
                           ("llz_asrc_mc_get_step", lambda: L.llz_asrc_mc_get_step(h, 0, 1, d4, l4)),
                           ("llz_asrc_mc_next_time", lambda: L.llz_asrc_mc_next_time(h, 0, 1, ll4, u4)),
                           ("llz_asrc_mc_get_table", lambda: L.llz_asrc_mc_get_table(h, f4, 64)),
                           ("llz_asrc_mc_out_len", lambda: L.llz_asrc_mc_out_len(h, 16, i4)),
                           ("llz_asrc_mc_set_stream", lambda: L.llz_asrc_mc_set_stream(h, None)),
                           ("llz_asrc_mc:", lambda: L.llz_asrc_mc(h, f4, 16, f4, 16, i4))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1 and name in capi.last_error(), name
        L.llz_asrc_mc_uninit(h)


@pytest.mark.parametrize("T,phases,form", [(4, 256, 0), (32, 512, 0), (128, 4096, 1)])
def test_valid_init_without_gpu_fails_loudly(L, T, phases, form):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a handle whose plan is {T, phases, T - 1, table form}, whose
    table is the model's bit for bit, and that another family's entry point refuses"""
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_asrc_mc_init(2, 1000, T, phases, 0.9, 1.0, capi.KAISER, 1.0)
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        out = (C.c_int * 4)()
        assert L.llz_asrc_mc_plan(h, out) == 0 and tuple(out) == (T, phases, T - 1, form)
        assert L.llz_resample_mc_sub_len(h) < 0 and L.llz_adapt_mc_plan(h, out) < 0
        L.llz_asrc_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_asrc_mc_init"):
            filters.AsrcMC(2, 1000, taps=T, phases=phases)


# ------------------------------------------------------------------------------------------------ the host layer under sanitizers
FRAME = 1000
SCRIPT = (
    [("init", 6, FRAME, 32, 512, 0.9, 1.0, capi.KAISER, 1.0)]
    + [("step", c, 1, s, 0) for c, s in enumerate(ac.STEPS)]
    + [("call", n, 16 * FRAME + 64) for n in (0, 1, 257, FRAME, 1, 0, 257)]
    + [("step", 0, 1, 1.0, 1), ("step", 1, 1, 0.5, 7), ("step", 2, 2, 1.003, 1000), ("step", 5, 1, 2.0, 600)]
    + [("call", n, 16 * FRAME + 64) for n in (257, 1, 0, 400)]
    + [("step", 2, 1, 0.997, 600)]                              # inside the glide of channel 2; channel 3 runs on
    + [("call", n, 16 * FRAME + 64) for n in (1, 130, 130, 130, FRAME)]
    + [("call", FRAME, 900), ("call", FRAME, 16 * FRAME + 64)]  # out_pitch too small: refused, then the same call with room
    + [("reset",), ("call", 257, 16 * FRAME + 64), ("call", 1, 16 * FRAME + 64)]
    + [("init", 3, 64, 4, 256, 1.0, 2.0, capi.HAMMING, 16.0), ("call", 64, 1), ("call", 64, 4), ("call", 1, 0), ("call", 1, 1)]
    + [("init", 2, 1 << 22, 128, 4096, 0.5, 1.0, capi.BLACKMAN, 1.0 / 16), ("step", 1, 1, 16.0, 0), ("call", 1 << 14, 1 << 18)]
)


def model_of_script(script):
    """the lines the driver must print: the integer model of tests/asrc_checks.py over the same commands"""
    lines, ch, T, received = [], [], 0, 0
    for cmd in script:
        if cmd[0] == "init":
            _, channels, _, T, phases, _, _, _, step = cmd
            ch, received = [ac.Channel(ac.to_inc(step)) for _ in range(channels)], 0
            lines.append(f"init {channels} {cmd[2]} {T} {phases}")
        elif cmd[0] == "step":
            for c in range(cmd[1], cmd[1] + cmd[2]):
                ch[c].set_step(cmd[3], cmd[4])
        elif cmd[0] == "reset":
            received = 0
            for c in ch:
                c.reset()
        else:
            _, n_in, pitch = cmd
            limit = received + n_in - 1 - T // 2
            import copy
            trial = [copy.copy(c) for c in ch]
            counts = [len(c.take(limit)) for c in trial]
            if max(counts) > pitch:
                ret = -1
            else:
                ret, ch, received = max(counts), trial, received + n_in
            lines.append(f"call {n_in} ret {ret} counts " + " ".join(map(str, counts)) + " times "
                         + " ".join(f"{c.t >> 32}:{c.t & 0xFFFFFFFF}" for c in ch))
    return lines


def test_host_layer_under_asan_ubsan(tmp_path):
    """the stand-alone driver over the stubbed device shim: steps 1/16, 0.3337, 1, 1 + 2^-32, 160/147 and 16, glides of 1, 7 and
    1000 outputs and one spanning three calls, a set_step inside a glide, calls of 0, 1, 257 and frame_len samples, a refused
    too-small out_pitch followed by the same call with room, a reset, the smallest table at step 16 and the largest frame_len;
    counts and times equal the integer model's line for line"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    script = tmp_path / "script.txt"
    script.write_text("".join(" ".join(repr(v) if isinstance(v, float) else str(v) for v in cmd) + "\n" for cmd in SCRIPT))
    exe = tmp_path / "asrc_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "asrc_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ASRC_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    got = [ln for ln in r.stdout.splitlines() if ln.startswith(("init", "call"))]
    want = model_of_script(SCRIPT)
    assert sum("ret -1" in ln for ln in want) == 2 and r.stdout.count("refused: llz_asrc_mc: channel") == 2
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    print("\n".join(got[:12]))


# ------------------------------------------------------------------------------------------------ the GPU cases on the model
@pytest.mark.parametrize("T,phases", ac.SHAPES)
@pytest.mark.parametrize("channels", ac.CHANNELS)
def test_gpu_dense_case_holds_on_the_model(oracle, T, phases, channels):
    assert ac.check_against(ac.model32, oracle, channels, T, phases, what="dense (float32 model)") <= 1.0


@pytest.mark.parametrize("name", sorted(ac.LONG))
def test_gpu_long_call_cases_hold_on_the_model(oracle, name):
    """the limit, counts and times; the model has no tiles, so the comparison with short calls is the device's alone"""
    assert ac.check_long(ac.model32, oracle, name, grouping=False, what="long (float32 model)") <= 1.0


def test_gpu_glide_case_holds_on_the_model(oracle):
    assert ac.check_glides(ac.model32, oracle, what="glides (float32 model)") <= 1.0


def test_gpu_sine_case_holds_on_the_model():
    err_m, worst = ac.check_sine(ac.model32, what="sine (float32 model)")
    assert worst <= 1.0


def test_model_table_and_identity():
    """cutoff 1, gain 1: row 0 of G is a unit impulse at k = T / 2 for every allowed number of phases, and row phases is row 0
    moved by one tap; at step 1 the float64 model returns its input"""
    for T, phases in ((4, 256), (32, 512), (32, 1024), (6, 2048), (128, 4096)):
        g = ac.table(T, phases, cutoff=1.0)
        unit = np.zeros(T, np.float32)
        unit[T // 2] = 1.0
        assert np.array_equal(g[0], unit), (T, phases)
        assert np.array_equal(g[phases][:-1], g[0][1:]) and g.shape == (phases + 1, T)
    x = np.arange(1.0, 201.0, dtype=np.float32)[None, :]
    ys, _, _ = ac.Model(1, 200, taps=32, phases=512, cutoff=1.0).process(x)
    assert np.array_equal(ys[0], x[0, :200 - 16])


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault", ac.FAULTS)
def test_limits_see_a_planted_fault(oracle, fault):
    """the limit is not slack: each fault in the float32 model misses it by the factor printed"""
    T, phases, channels = 32, 512, 4
    x, (ym, A, counts_m, _) = ac.reference(oracle, channels, T, phases, ac.GLIDE_CALLS, ac.GLIDE_SCRIPT, steps=ac.GLIDE_STEPS)

    def faulty(*args, **kw):
        return ac.Model(*args, prec=32, fault=fault, **kw)
    y, _, counts, _ = ac.run_stream(faulty, channels, ac.GLIDE_CALLS, x, T, phases, script=ac.GLIDE_SCRIPT, steps=ac.GLIDE_STEPS)
    worst = 0.0
    for c in range(channels):
        n = min(len(y[c]), len(ym[c]))
        worst = max(worst, ac.ratio_to_limit(y[c][:n], ym[c][:n], A[c][:n], T))
    print(f"planted fault {fault}: misses the limit by a factor of {worst:.3g}")
    assert worst > 10.0, fault
