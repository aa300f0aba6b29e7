"""The tables of the frequency-domain FIR forms, byte for byte: the host layer builds every form's tap spectra in one place
(csrc/host/llz_spectra.c), and the stand-alone driver tests/fir_tables_driver.c reads the uploaded tables back over the stubbed
device shim, under AddressSanitizer + UBSan, to hold it to what that promises: equal taps give equal float32 entries in the shared
and the per-row handles, set_taps replaces one row and nothing else, and rows beyond one staging chunk arrive whole.  No kernel
is launched here."""
import glob
import os
import re
import subprocess

from tests.test_host_sanitizers import CSRC, ROOT, gen_stub


def test_fir_tables_agree_byte_for_byte_under_asan_ubsan(tmp_path):
    stub = tmp_path / "shim_stub.c"
    stub.write_text(gen_stub())
    exe = tmp_path / "fir_tables"
    srcs = sorted(glob.glob(os.path.join(CSRC, "host", "*.c")))
    cmd = ["gcc", "-g", "-O1", "-std=c99", "-D_GNU_SOURCE", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "fir_tables_driver.c"),
           str(stub)] + srcs + ["-lm", "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "FIR_TABLES_OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-6000:])
    assert len(re.findall(r"partitioned T=(?:1 N=1024 P=1|513 N=1024 P=2|2049 N=2048 P=3|8193 N=8192 P=3): shared", r.stdout)) == 4
    assert len(re.findall(r"stream B=(?:64 T=1|64 T=65|512 T=513) P=\d+: one tap set", r.stdout)) == 3
    assert len(re.findall(r"(?:bank overlap-save|partitioned bank|stream rows|matrix) T=\d+: set_taps keeps", r.stdout)) == 4
    assert "stream B=128 T=131073: 9 rows in 2 uploads of at most 7 rows" in r.stdout, r.stdout
