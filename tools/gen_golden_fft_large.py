"""Writes tests/golden/fft_large.npz: the reference's own llz_fft / llz_ifft at 8192 points (inputs and outputs only),
through oracle/_ref/libllzref.so, the reference's C files compiled by oracle/Makefile's `ref` recipe (python -c "from
oracle import pyoracle; pyoracle.build()" makes it where the reference tree is present).  No test, smoke() or bench.py runs
this.

    python tools/gen_golden_fft_large.py [--out tests/golden/fft_large.npz]

x: seeded complex128 input; fwd = llz_fft(x); inv = llz_ifft(fwd) (the round trip, rounding included).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import pyoracle  # noqa: E402

N = 8192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fft_large.npz"))
    a = ap.parse_args()
    if not pyoracle.have_ref():
        sys.exit("oracle/_ref/libllzref.so is missing: build it first")
    ref = pyoracle.Ref()
    rng = np.random.default_rng(8192)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    fwd = ref.fft(x)
    inv = ref.fft(fwd, inverse=True)
    np.savez(a.out, x=x, fwd=fwd, inv=inv)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
