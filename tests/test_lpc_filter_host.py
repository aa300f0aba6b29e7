"""CPU-side checks of the LPC filters (include/llz_lpc.h part 3, llz_lpc_filter_mc): the seven symbols exist in every layer with
their prototypes and the earlier llz_lpc* names are untouched, every init and call refusal comes with a message of its own,
without a GPU a valid init fails loudly, the host layer runs clean under AddressSanitizer + UBSan in a stand-alone driver
(tests/lpc_filter_sanitize_driver.c), and the models, families and limits of tests/lpc_filter_checks.py hold together: every GPU
case with the unfused float32 model in the device's place, the off-by-one-frame bug caught at every frame edge of every channel,
and the float64 round trip on the static family.  No kernel is launched here.  On the parent of this feature the library
exports none of the seven symbols and every test below that touches them fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import lpc_filter_checks as lc
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

PROTOTYPES = {
    "llz_lpc_filter_mc_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*int \w+\s*\)",
    "llz_lpc_filter_mc_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    "llz_lpc_filter_mc_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
    "llz_lpc_filter_mc_reset": r"\bint\s+%s\s*\(\s*unsigned long \w+\s*\)",
    "llz_lpc_residual_mc": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*const float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
    "llz_lpc_synth_mc": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*const float \*\w+,\s*float \*\w+,\s*int \w+\s*\)",
}
NEW = list(PROTOTYPES)
BEFORE = ["llz_lpc_init", "llz_lpc_uninit", "llz_lpc", "llz_lpc_mc"]


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no LPC filters"
    return lib


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(capi.INCLUDE_DIR, "llz_lpc.h")).read(), flags=re.S)


def test_symbols_declared_bound_and_exported(L):
    """(the issue counts seven symbols with llz_lpc_filter_mc itself as the family's name; six functions carry it)"""
    text = header()
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert all(n in capi.declared_symbols() and hasattr(L, n) for n in NEW)
    assert all(getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) >= 1 for n in NEW)
    assert set(re.findall(r"\b(llz_lpc\w*)\s*\(", text)) == set(NEW) | set(BEFORE)
    assert all(hasattr(L, n) for n in BEFORE)
    for method in ("residual", "synth", "reset", "close"):
        assert hasattr(filters.LpcFilterMC, method), method


def refused_init(L, what, *args):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert L.llz_lpc_filter_mc_init(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and "llz_lpc_filter_mc_init" in msg, (what, msg)
    return msg


def test_init_refusals_carry_a_message(L):
    seen = {
        "channels": refused_init(L, "channels 0", 0, 160, 16),
        "p low": refused_init(L, "p -1", 4, 160, -1),
        "p high": refused_init(L, "p 65", 4, 160, 65),
        "frame_len": refused_init(L, "frame_len == p", 4, 16, 16),
    }
    assert "channels 0" in seen["channels"] and ">= 1" in seen["channels"]
    assert "p -1" in seen["p low"] and "p 65" in seen["p high"] and "0..64" in seen["p high"]
    assert "frame_len 16" in seen["frame_len"] and "p 16" in seen["frame_len"]
    kinds = {re.sub(r"-?\d+", "#", m) for m in seen.values()}
    assert len(kinds) == 3, kinds                                   # the two p refusals are one kind
    refused_init(L, "frame_len 0 at p 0", 4, 0, 0)
    with pytest.raises(capi.LlzError, match="0..64"):
        filters.LpcFilterMC(4, 160, 65)


def test_calls_refuse_a_bad_handle_with_the_entry_point_named(L):
    buf = (C.c_float * 64)()
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("llz_lpc_residual_mc", lambda: L.llz_lpc_residual_mc(h, buf, buf, buf, 1)),
                           ("llz_lpc_synth_mc", lambda: L.llz_lpc_synth_mc(h, buf, buf, buf, 1)),
                           ("llz_lpc_filter_mc_reset", lambda: L.llz_lpc_filter_mc_reset(h)),
                           ("llz_lpc_filter_mc_set_stream", lambda: L.llz_lpc_filter_mc_set_stream(h, None))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() < 0, name
            assert name in capi.last_error() and "bad handle" in capi.last_error(), (name, capi.last_error())
        L.llz_lpc_filter_mc_uninit(h)


def test_valid_init_without_gpu_fails_loudly(L):
    """a valid init: without a GPU BAD_HANDLE and a message; with one a handle whose calls refuse frames 0 and NULL buffers,
    each with a message of its own"""
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_lpc_filter_mc_init(3, 160, 16)
    msg = capi.last_error()
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        buf = np.zeros(3 * 160, dtype=np.float32)
        cof = np.zeros(3 * 17, dtype=np.float32)
        seen = set()
        for name in ("llz_lpc_residual_mc", "llz_lpc_synth_mc"):
            fn = getattr(L, name)
            assert fn(h, buf.ctypes.data, cof.ctypes.data, buf.ctypes.data, 0) < 0
            assert name in capi.last_error() and "frames 0" in capi.last_error()
            seen.add(capi.last_error())
            assert fn(h, None, cof.ctypes.data, buf.ctypes.data, 1) < 0 and "NULL" in capi.last_error()
            seen.add(capi.last_error())
        assert len(seen) == 4
        L.llz_lpc_filter_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert msg not in ("", before) and "llz_lpc_filter_mc_init" in msg
        with pytest.raises(capi.LlzError, match="llz_lpc_filter_mc_init"):
            filters.LpcFilterMC(3, 160, 16)


def test_host_layer_under_asan_ubsan(tmp_path, L):
    """the stand-alone driver over the stubbed device shim: nothing is loaded into python"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    exe = tmp_path / "lpc_filter_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "lpc_filter_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "LPC_FILTER_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    assert len(re.findall(r"lpc filter channels=\d+ frame_len=\d+ p=\d+ frames<=\d+ ok", r.stdout)) == 6, r.stdout


# ------------------------------------------------------------------------------------------------ the GPU cases on the models
def test_case_table_covers_the_shapes():
    assert {c[0] for c in lc.CASES} == set(lc.CHANNELS) and {c[1] for c in lc.CASES} == set(lc.ORDERS)
    assert {c[3] for c in lc.CASES} == set(range(1, 8))
    for p in lc.ORDERS:
        assert {c[2] for c in lc.CASES if c[1] == p} == set(lc.frame_lens(p)) and p + 1 in lc.frame_lens(p)
    assert all(fl > p for (_c, p, fl, _f) in lc.CASES) and len(lc.SPLIT_CASES) >= 12
    # every template edge of the synthesis kernel, a partial wave of lanes, and rows of more than one 1024-sample tile
    assert {8, 9, 16, 17, 32, 33, 64} <= set(lc.ORDERS) and 130 in lc.CHANNELS
    assert any(fl * fr > 1024 for (_c, _p, fl, fr) in lc.CASES)


@pytest.mark.parametrize("fam", lc.FAMILIES)
@pytest.mark.parametrize("channels,p,frame_len,frames", lc.CASES)
def test_gpu_cases_hold_on_the_float32_model(L, channels, p, frame_len, frames, fam):
    """the unfused float32 model stays within the GPU's limit on every GPU case, zero coefficient sets return x's bits, the
    synthesis reference is finite, and the off-by-one-frame bug exceeds the limit at every frame edge of every channel"""
    d = lc.case_data(channels, p, frame_len, frames, fam)
    lc.check_residual(lc.residual32(d["x"], d["a"], frame_len), d, "float32 model")
    assert np.isfinite(d["y"]).all()
    if p == 0 or frames == 1:
        return
    late = np.abs(lc.residual64(d["x"], d["a"], frame_len, late=True) - d["e64"]) > d["lim"]
    edges = late.reshape(channels, frames, frame_len)[:, 1:, :p]
    assert edges.any(axis=2).all(), "the limit would hide a frame-edge error"
    assert not late.reshape(channels, frames, frame_len)[:, :, p:].any() and not late[:, :frame_len].any()


def test_synth_model_continues_from_its_state():
    """the model's state argument is the handle's: splitting a stream leaves every bit where it was"""
    channels, p, fl, frames = 3, 9, 50, 4
    d = lc.case_data(channels, p, fl, frames, "random")
    whole = lc.synth_model(d["x"], d["a"], fl)
    cut = fl
    first = lc.synth_model(d["x"][:, :cut], d["a"][:, :1], fl)
    rest = lc.synth_model(d["x"][:, cut:], d["a"][:, 1:], fl, state=first[:, :-p - 1:-1])
    assert np.array_equal(np.concatenate([first, rest], axis=1).view(np.uint64), whole.view(np.uint64))


@pytest.mark.parametrize("p", [2, 9, 16, 32, 64])
def test_models_round_trip_on_the_static_family(L, p):
    """float64: synth_model(residual64(x)) returns x within 1e-12 sum |g| on family (iv), whose impulse responses decay"""
    channels, fl, frames = 5, 160, 3
    x = lc.signal(channels, frames * fl, 50 + p)
    a = lc.family("static", channels, frames, p, 60 + p)
    g = lc.impulse_response(a[:, 0, :])
    back = lc.synth_model(lc.residual64(x, a, fl), a, fl)
    assert (np.abs(back - x) <= 1e-12 * np.abs(g).sum(axis=1, keepdims=True)).all()
