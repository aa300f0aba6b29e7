"""Writes tests/golden/stft_large.npz: the reference's own llz_analysis_fft / llz_synthesis_fft at fft_len 8192 (frame_len
2048, 3/4 overlap, Blackman window; inputs and outputs only), through oracle/_ref/libllzref.so, the reference's C files
compiled by oracle/Makefile's `ref` recipe (python -c "from oracle import pyoracle; pyoracle.build()" makes it where the
reference tree is present).  No test, smoke() or bench.py runs this.

    python tools/gen_golden_stft_large.py [--out tests/golden/stft_large.npz]

x: seeded float64 samples, FRAMES frames; re, im = llz_analysis_fft frame by frame ([FRAMES][4097]); syn =
llz_synthesis_fft of those spectra frame by frame (the 0.812 output scale included).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import pyoracle  # noqa: E402

HINT, FRAME_LEN, WIN, FRAMES = 0, 2048, pyoracle.BLACKMAN, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "stft_large.npz"))
    a = ap.parse_args()
    if not pyoracle.have_ref():
        sys.exit("oracle/_ref/libllzref.so is missing: build it first")
    ref = pyoracle.Ref()
    rng = np.random.default_rng(8192)
    x = rng.uniform(-1, 1, FRAMES * FRAME_LEN)
    re, im = ref.stft_analysis(HINT, FRAME_LEN, WIN, x)
    syn = ref.stft_synthesis(HINT, FRAME_LEN, WIN, re, im)
    np.savez(a.out, hint=HINT, frame_len=FRAME_LEN, win=WIN, x=x, re=re, im=im, syn=syn)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
