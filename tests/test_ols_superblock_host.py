"""The geometry of the super-block walk of the headline overlap-save FIR (llzlab_amd/csrc/kernels/ols_superblock.h, walked by
k_fir_ols_chain_f32), checked on the CPU: tests/ols_superblock_driver.cpp replays the walk on sample indices through the
header's own functions.  For every n in 1 .. 3 * 16384 + 2 and keep = 1, 128, 256: every output sample in [0, n) is stored
exactly once, the 256 predecessors of every stored sample are in the block that stores it, no request leaves [-keep, n), and
no live super-block index reaches the plan's total.  The sweep runs as a plain executable; the lengths around every boundary
(a row's start, the region and super-block ends) run again under AddressSanitizer + UBSan.  No GPU, no library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "llzlab_amd", "csrc", "kernels")
DRIVER = os.path.join(ROOT, "tests", "ols_superblock_driver.cpp")
UNIT = 16384
N_MAX = 3 * UNIT + 2
CHUNK = 4096
BASE = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-I" + KERNELS, DRIVER]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("ols_sb")
    plain, san = str(d / "driver"), str(d / "driver_san")
    subprocess.check_call(BASE + ["-o", plain])
    subprocess.check_call(BASE + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                                  "-o", san])
    return plain, san


def run(exe, lo, hi, keep):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(lo), str(hi), str(keep)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and f"OLS_SB_OK n={lo}..{hi} keep={keep}" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("keep", [1, 128, 256])
@pytest.mark.parametrize("lo", range(1, N_MAX + 1, CHUNK))
def test_every_length_stores_each_sample_once_from_a_complete_block(exes, lo, keep):
    run(exes[0], lo, min(lo + CHUNK - 1, N_MAX), keep)


@pytest.mark.parametrize("keep", [1, 128, 256])
def test_boundary_lengths_under_asan_ubsan(exes, keep):
    for lo, hi in ((1, 1100), (UNIT // 2 - 300, UNIT // 2 + 300), (UNIT - 300, UNIT + 300),
                   (UNIT + UNIT // 2 - 300, UNIT + UNIT // 2 + 800), (N_MAX - 300, N_MAX)):
        run(exes[1], lo, hi, keep)
