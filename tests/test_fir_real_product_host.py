"""CPU: the table of the real spectrum product of the 1024-point overlap-save FIR (llzlab_amd/csrc/host/llz_fir_host.c:
llz_host_ols_real_rows decides K from the float taps, llz_host_ols_real_table builds Re DFT_1024(g) / 1024 of the taps centred
at index 0, in double; the device table is its cast to float).  tests/ols_real_table_driver.c is compiled with the host layer
against the generated shim stub of test_host_sanitizers.py and run on the library's own designs; numpy computes the same table
from the taps the driver prints."""
import glob
import os
import subprocess

import numpy as np
import pytest

from tests.test_host_sanitizers import CSRC, ROOT, gen_stub

TUNE_STUB = "int llzs_tune(int id) { (void)id; return -1; }"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ols_real_table")
    text = gen_stub()
    assert TUNE_STUB in text
    stub = tmp / "shim_stub.c"
    stub.write_text(text.replace(TUNE_STUB, "int g_test_tune[LLZS_TUNE_COUNT]; int llzs_tune(int id) { return g_test_tune[id] - 1; }"))
    exe = tmp / "ols_real_table_driver"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    subprocess.check_call(["gcc", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "ols_real_table_driver.c"),
                           str(stub)] + srcs + ["-lm", "-o", str(exe)])

    def run(kind, T, mode="plain"):
        r = subprocess.run([str(exe), kind, str(T), mode], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (kind, T, mode, r.stderr[-2000:])
        out = {}
        for line in r.stdout.splitlines():
            key, _, rest = line.partition(" ")
            out[key] = [float.fromhex(v) for v in rest.split()]
        return int(out["K"][0]), np.array(out["taps"]), out.get("imag", [None])[0], np.array(out.get("table", []))
    return run


@pytest.mark.parametrize("kind", ["lpf", "hpf", "bp"])
@pytest.mark.parametrize("T", [65, 129, 193, 257])
def test_real_table_is_the_spectrum_of_the_centred_taps(driver, kind, T):
    K, taps, imag, table = driver(kind, T)
    c = (T - 1) // 2
    assert len(taps) == T and K == c // 32 and len(table) == 1024
    assert np.array_equal(taps, taps[::-1]), "the designed float32 taps mirror bit for bit"
    g = np.zeros(1024)
    g[(np.arange(T) - c) % 1024] = taps
    G = np.fft.fft(g) / 1024
    peak = np.abs(G.real).max()
    print(f"{kind} {T}: K {K} table error {np.abs(table - G.real).max() / peak:.3g} of the peak, "
          f"dropped imag {imag / peak:.3g}, numpy's {np.abs(G.imag).max() / peak:.3g}")
    assert np.abs(table - G.real).max() <= 1e-12 * peak
    assert imag < 1e-12 * peak and np.abs(G.imag).max() < 1e-12 * peak


@pytest.mark.parametrize("kind,T,mode", [("lpf", 63, "plain"), ("lpf", 255, "plain"), ("lpf", 128, "plain"), ("lpf", 256, "plain"),
                                         ("lpf", 257, "ulp"), ("lpf", 257, "tune0"), ("lpf", 33, "plain"), ("lpf", 321, "plain")])
def test_every_other_tap_set_keeps_the_complex_product(driver, kind, T, mode):
    """a centre that is no multiple of 32 (63, 255 taps), an even length, one tap one ulp off its mirror image, the
    ols_real_product = 0 tune; and centres outside 32 .. 128"""
    K, taps, _, table = driver(kind, T, mode)
    assert K == 0 and len(table) == 0 and len(taps) == T
    if mode == "ulp":
        assert not np.array_equal(taps, taps[::-1])
