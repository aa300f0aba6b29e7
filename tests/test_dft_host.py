"""CPU-side checks of the DFT of any length and the zoom transform (include/llz_dft.h, llz_dft_mc / llz_czt_mc): the thirteen
symbols exist in every layer with their prototypes and pinned argtypes, no process-wide tune is added, every refusal that needs no
device comes with a message naming its function, without a GPU a valid init fails loudly, the case table covers the shapes, the
float32 model of tests/dft_checks.py stays inside both limits on every GPU case, each planted fault misses a limit by the factor
printed, the tables the host layer builds are the model's bit for bit, and the host layer runs clean under AddressSanitizer +
UBSan in a stand-alone driver (tests/dft_sanitize_driver.c).  No kernel is launched here.  On the parent of this feature the
library exports none of the symbols and every test below that touches them fails."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import dft_checks as dk
from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

CALL = r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+,\s*long \w+,\s*float \*\w+,\s*long \w+,\s*int \w+\s*\)"
CALLS = ("llz_dft_mc_forward", "llz_dft_mc_inverse", "llz_dft_mc_real_forward", "llz_dft_mc_real_inverse", "llz_czt_mc_forward",
         "llz_czt_mc_real_forward")
PROTOTYPES = {
    "llz_dft_mc_init": r"\bunsigned long\s+%s\s*\(\s*int \w+\s*\)",
    "llz_czt_mc_init": r"\bunsigned long\s+%s\s*\(\s*int \w+,\s*int \w+,\s*double \w+,\s*double \w+\s*\)",
    "llz_dft_mc_uninit": r"\bvoid\s+%s\s*\(\s*unsigned long \w+\s*\)",
    "llz_dft_mc_set_stream": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*void \*\w+\s*\)",
    "llz_dft_mc_set_window": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*const float \*\w+\s*\)",
    "llz_dft_mc_configure": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \w+\s*\)",
    "llz_dft_mc_plan": r"\bint\s+%s\s*\(\s*unsigned long \w+,\s*int \w+,\s*int \*\w+\s*\)",
    **{name: CALL for name in CALLS},
}
ARGTYPES = {
    "llz_dft_mc_init": (C.c_ulong, [C.c_int]),
    "llz_czt_mc_init": (C.c_ulong, [C.c_int, C.c_int, C.c_double, C.c_double]),
    "llz_dft_mc_uninit": (None, [C.c_ulong]),
    "llz_dft_mc_set_stream": (C.c_int, [C.c_ulong, C.c_void_p]),
    "llz_dft_mc_set_window": (C.c_int, [C.c_ulong, C.c_void_p]),
    "llz_dft_mc_configure": (C.c_int, [C.c_ulong, C.c_int, C.c_int]),
    "llz_dft_mc_plan": (C.c_int, [C.c_ulong, C.c_int, C.POINTER(C.c_int)]),
    **{name: (C.c_int, [C.c_ulong, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int]) for name in CALLS},
}
NEW = list(PROTOTYPES)
SHIM = {"llzs_dft_plan", "llzs_dft_fused_f32", "llzs_dft_pack_f32", "llzs_dft_mul_f32", "llzs_dft_extract_f32"}
OPS = ("forward", "inverse", "rforward", "rinverse")


@pytest.fixture(scope="module")
def L():
    capi.build()
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NEW), "the library exports no llz_dft_mc"
    return lib


def test_symbols_declared_bound_and_exported(L):
    raw = open(os.path.join(capi.INCLUDE_DIR, "llz_dft.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, proto in PROTOTYPES.items():
        assert re.search(proto % re.escape(name), text), name
    assert set(re.findall(r"\b(llz_\w+)\s*\(", text)) == set(NEW)
    assert all(n in capi.declared_symbols() for n in NEW)
    for name, (res, args) in ARGTYPES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert re.search(r"enum\s*\{\s*LLZ_DFT_FUSED\s*=\s*0,\s*LLZ_DFT_COMPOSED\s*\}", text)
    assert (capi.DFT_FUSED, capi.DFT_COMPOSED) == (0, 1)
    assert "INPUT ROWS MAY OVERLAP" in raw and "DEPEND ON NOTHING BUT THAT ROW" in raw
    shim = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "llz_shim.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(llzs_dft\w*)\s*\(", shim)) == SHIM and all(("int " + n + "(") in gen_stub() for n in SHIM)
    host = open(os.path.join(CSRC, "host", "llz_host.h")).read()
    assert "LLZ_TAG_DFTM" in host and "llz_host_dft_tables" in host
    for method in ("forward", "inverse", "rforward", "rinverse", "set_window", "configure", "plan", "set_stream", "close"):
        assert hasattr(filters.DftMC, method), method
    for method in ("forward", "rforward", "plan", "set_window", "configure", "set_stream", "close"):
        assert hasattr(filters.CztMC, method), method


def test_no_tune_is_added(L):
    """the form and the scratch cap are set per handle (llz_dft_mc_configure): no name joins the process-wide overrides"""
    names = []
    while L.llz_hip_tune_name(len(names)) is not None:
        names.append(L.llz_hip_tune_name(len(names)).decode())
    assert names and not [n for n in names if "dft" in n]
    assert L.llz_hip_tune(b"dft_composed", 1) == -1 and L.llz_hip_tune(b"dft_scratch_mb", 1) == -1


def refused(L, what, init, *args):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
    before = capi.last_error()
    assert getattr(L, init)(*args) == capi.BAD_HANDLE, what
    msg = capi.last_error()
    assert msg != before and init in msg, (what, msg)
    return msg


def test_init_refusals_carry_a_message(L):
    for n in (1, 0, -480, 1048577, 1 << 30):
        assert f"n {n} " in refused(L, "n", "llz_dft_mc_init", n) and "2..1048576" in capi.last_error()
    assert "n 0" in refused(L, "n", "llz_czt_mc_init", 0, 8, 0.0, 0.1)
    assert "k 0" in refused(L, "k", "llz_czt_mc_init", 8, 0, 0.0, 0.1)
    assert "k -3" in refused(L, "k", "llz_czt_mc_init", 8, -3, 0.0, 0.1)
    assert "n + k - 1 <= 4096" in refused(L, "m", "llz_czt_mc_init", 2048, 2050, 0.0, 0.1)
    assert "n + k - 1 <= 4096" in refused(L, "m", "llz_czt_mc_init", 4097, 1, 0.0, 0.1)
    refused(L, "overflow", "llz_czt_mc_init", 2 ** 31 - 1, 2 ** 31 - 1, 0.0, 0.1)
    for df in (0.51, -0.75, float("nan"), float("inf")):
        assert "|df| <= 0.5" in refused(L, "df", "llz_czt_mc_init", 8, 8, 0.0, df)
    for f0 in (float("nan"), float("inf"), -float("inf")):
        assert "f0" in refused(L, "f0", "llz_czt_mc_init", 8, 8, f0, 0.1)
    with pytest.raises(capi.LlzError, match="llz_dft_mc_init.*n 1 "):
        filters.DftMC(1)
    with pytest.raises(capi.LlzError, match="llz_czt_mc_init.*df 0.7"):
        filters.CztMC(8, 8, 0.0, 0.7)


def test_calls_refuse_a_foreign_handle_with_the_entry_point_named(L):
    buf = (C.c_float * 64)()
    plan = (C.c_int * 5)()
    for h in (0, capi.BAD_HANDLE):
        calls = [(name, lambda name=name: getattr(L, name)(h, buf, 4, buf, 4, 1)) for name in CALLS]
        calls += [("llz_dft_mc_set_window", lambda: L.llz_dft_mc_set_window(h, buf)),
                  ("llz_dft_mc_configure", lambda: L.llz_dft_mc_configure(h, 1, 4)),
                  ("llz_dft_mc_set_stream", lambda: L.llz_dft_mc_set_stream(h, None)),
                  ("llz_dft_mc_plan", lambda: L.llz_dft_mc_plan(h, 1, plan))]
        for name, call in calls:
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == -1, name
            assert name in capi.last_error() and "bad handle" in capi.last_error(), (name, capi.last_error())
        L.llz_dft_mc_uninit(h)


def test_valid_init_without_gpu_fails_loudly(L):
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_dft_mc_init(480)
    msg = capi.last_error()
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, msg
        buf = np.zeros(2 * 480, dtype=np.float32)
        assert L.llz_dft_mc_forward(h, buf.ctypes.data, 480, buf.ctypes.data, 479, 1) == -1 and "out_pitch 479" in capi.last_error()
        assert L.llz_czt_mc_forward(h, buf.ctypes.data, 480, buf.ctypes.data, 480, 1) == -1 and "DFT handle" in capi.last_error()
        assert L.llz_dft_mc_configure(h, 2, 4) == -1 and "composed 2" in capi.last_error()
        L.llz_dft_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert msg not in ("", before)
        with pytest.raises(capi.LlzError, match="llz_dft_mc_init"):
            filters.DftMC(480)
        with pytest.raises(capi.LlzError, match="llz_czt_mc_init"):
            filters.CztMC(1000, 64, 0.1, 1e-4)


def test_host_layer_under_asan_ubsan(tmp_path, L):
    """the stand-alone driver over the stubbed device shim: nothing is loaded into python.  The driver runs init, set_window,
    plan, every entry point on exact host buffers with overlapping input rows and gaps between output rows, the refusals, and a
    composed call that walks two slabs"""
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    exe = tmp_path / "dft_sanitize"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "dft_sanitize_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "DFT_SANITIZE_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    assert len(re.findall(r"dft n=\d+ form=\d m=\d+ ok", r.stdout)) == 7 and len(re.findall(r"czt n=\d+ k=\d+ m=\d+ ok", r.stdout)) == 4
    assert "dft two slabs ok" in r.stdout and "dft configure ok" in r.stdout


# ------------------------------------------------------------------------------------------------ the GPU cases on the models
def test_case_table_covers_the_shapes():
    assert dk.FUSED_N == (2, 3, 5, 7, 17, 127, 251, 441, 480, 960, 1000, 1023, 1024, 1025, 1920, 2047, 2048)
    assert dk.COMPOSED_N == (2049, 4800, 65537) and dk.FORCED_N == (7, 480, 2047) and dk.ROWS == (3, 37)
    assert dk.ZOOMS == ((1000, 64, 0.1, 1e-4), (2048, 2049, 0.0, 1.0 / 4096), (300, 3797, 0.25, 0.37 / 3797), (1, 1, 0.3, 0.1))
    ms = [dk.m_of(n, n) for n in dk.FUSED_N]
    assert set(ms) == {8, 16, 64, 256, 512, 1024, 2048, 4096}
    # both sides of every M step the list crosses, and the step to the composed form
    for lo, hi in ((1024, 1025), (2048, 2049)):
        assert dk.m_of(lo, lo) * 2 == dk.m_of(hi, hi)
    assert dk.m_of(2048, 2048) == 4096 and dk.m_of(2049, 2049) == 8192 and dk.m_of(65537, 65537) == 1 << 18
    assert all(dk.m_of(n, k) <= 4096 for n, k, _f0, _df in dk.ZOOMS) and dk.m_of(2048, 2049) == 4096 and dk.m_of(1, 1) == 8
    # rows per workgroup from 256 to 1, and a count they do not divide
    tpw = {dk.tpw_of(m, 300) for m in ms}
    assert tpw == {256, 128, 32, 8, 4, 2, 1}
    assert any(37 % dk.tpw_of(m, 37) for m in ms) and any(3 % dk.tpw_of(m, 3) for m in ms)
    x = dk.rows(480, 37)
    assert x.shape == (37, 480) and x.dtype == np.complex64 and dk.dense(37) == list(range(0, 37, 3))
    assert np.count_nonzero(x[2]) == 1 and x[2, 479] != 0
    spectrum = np.abs(np.fft.fft(x[1].astype(np.complex128)))
    assert np.sort(spectrum)[-2] > 0.2 * spectrum.max()          # an off-bin tone: its energy is in two bins at the least


def case_input(op, n, count):
    x = dk.rows(n, count, real=op == "rforward")
    return x[:, :n // 2 + 1].copy() if op == "rinverse" else x


@pytest.mark.parametrize("n", dk.FUSED_N + dk.COMPOSED_N)
def test_gpu_cases_hold_on_the_float32_model(n):
    for count in dk.ROWS if n < 65537 else dk.ROWS[:1]:
        for op in OPS:
            x = case_input(op, n, count)
            dk.check(dk.model_f32(op, x, n), dk.ref64(op, x, n), dk.bin_limit(op, x, n), dk.dense(count),
                     f"float32 model {op} n={n} rows={count}")


@pytest.mark.parametrize("n,k,f0,df", dk.ZOOMS)
def test_zoom_cases_hold_on_the_float32_model(n, k, f0, df):
    for count in dk.ROWS:
        for real in (False, True):
            x = dk.rows(n, count, real=real)
            dk.check(dk.model_f32("zoom", x, n, k, f0, df), dk.ref64("zoom", x, n, k, f0, df), dk.bin_limit("zoom", x, n, k),
                     dk.dense(count), f"float32 model zoom n={n} k={k} real={real} rows={count}")


def test_windowed_model_and_zoom_as_dft():
    n = 480
    w = np.hanning(n + 2)[1:-1].astype(np.float32)
    for op in OPS:
        x = case_input(op, n, 3)
        dk.check(dk.model_f32(op, x, n, w=w), dk.ref64(op, x, n, w=w), dk.bin_limit(op, x, n, w=w), dk.dense(3), f"hann {op}")
    x = dk.rows(n, 3)
    dk.check(dk.model_f32("zoom", x, n, n, 0.0, 1.0 / n), dk.ref64("forward", x, n), dk.bin_limit("forward", x, n), dk.dense(3),
             "zoom as the DFT")


@pytest.mark.parametrize("fault", dk.FAULTS)
@pytest.mark.parametrize("n", dk.FAULT_N)
def test_planted_faults_are_caught(n, fault):
    """each fault misses a limit by the factor printed: the limits are not loose.  Phases from a float32 pi n^2 / N stay inside the
    worst-case per-bin limit and must breach the RMS gate from N = 480 on; every other fault misses by more than 1e3"""
    op = "inverse" if fault == "fwd_chirp_inverse" else "forward"
    x = dk.rows(n, 3)
    per_bin, rms = dk.ratios(dk.model_f32(op, x, n, fault=fault), dk.ref64(op, x, n), dk.bin_limit(op, x, n), dk.dense(3))
    print(f"{fault} n={n}: worst bin at {per_bin:.3g} of its limit, dense rows at {rms:.3g} of the RMS gate")
    if fault == "f32_phase":
        assert n < 480 or rms > 1.0, (n, rms)
    else:
        assert max(per_bin, rms) > 1e3, (per_bin, rms)


def host_tables(L, n, k, zoom, f0, df, inverse, natural, w):
    fn = L.llz_host_dft_tables                                   # the host layer's builder, internal to the library: no device
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int] + 4 * [C.c_void_p]
    pre, v, post = np.zeros(n, np.complex64), np.zeros(dk.m_of(n, k), np.complex64), np.zeros(k, np.complex64)
    assert fn(n, k, zoom, f0, df, inverse, natural, None if w is None else w.ctypes.data, pre.ctypes.data, v.ctypes.data,
              post.ctypes.data) == 0, capi.last_error()
    return pre, v, post


@pytest.mark.parametrize("n,k,zoom,f0,df", [(3, 3, 0, 0.0, 0.0), (480, 480, 0, 0.0, 0.0), (2047, 2047, 0, 0.0, 0.0),
                                            (65537, 65537, 0, 0.0, 0.0), (1000, 64, 1, 0.1, 1e-4)])
def test_host_tables_equal_the_models_bit_for_bit(L, n, k, zoom, f0, df):
    w = (0.5 + 0.25 * np.cos(np.arange(n))).astype(np.float32)
    for inverse in (0,) if zoom else (0, 1):
        for natural, win in ((0, None), (1, w)) if n > 4096 else ((0, None), (0, w), (1, w)):
            got = host_tables(L, n, k, zoom, f0, df, inverse, natural, win)
            want = dk.tables(n, k, bool(zoom), f0, df, bool(inverse), bool(natural), win)
            for name, a, b in zip(("pre", "v", "post"), got, want):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, inverse, natural, win is not None)
