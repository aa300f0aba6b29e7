"""Windowed-FFT frames above 2048 points, on the CPU: the size contract of llz_analysis_fft_init / llz_synthesis_fft_init
(fft_len a power of two in 2..2^24) and llz_stft_mc_init (8..2^24), the fixture of tools/gen_golden_stft_large.py against
the checker, and the checker against the reference's own llz_analysis_fft / llz_synthesis_fft (oracle/_ref) up to 2^20."""
import os

import numpy as np
import pytest

from llzlab_amd import capi
from oracle import pyoracle as po

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (overlap_hint, frame_len) with fft_len 4096 .. 2^24
NEW = [(0, 1 << k) for k in range(10, 23)] + [(1, 1 << k) for k in range(11, 24)]


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def _size_refusal(msg):
    return "power of two" in msg


def test_new_sizes_pass_the_size_check_without_gpu(L):
    """On a box without a GPU the new sizes get past the size check and fail on the device, as every constructor does."""
    if L.llz_hip_device_count() > 0:
        pytest.skip("GPU present")
    for hint, frame_len in NEW:
        for init in (L.llz_analysis_fft_init, L.llz_synthesis_fft_init):
            assert init(hint, frame_len, po.HAMMING) == capi.BAD_HANDLE
            msg = capi.last_error()
            assert msg != "" and not _size_refusal(msg), (hint, frame_len, msg)
        assert L.llz_stft_mc_init(2, hint, frame_len, po.HAMMING) == capi.BAD_HANDLE
        msg = capi.last_error()
        assert msg != "" and not _size_refusal(msg), (hint, frame_len, msg)


# fft_len 2^25 (both overlaps), not a power of two, frame_len 0 / negative / huge, and an unknown overlap_hint
@pytest.mark.parametrize("hint,frame_len", [(0, 1 << 23), (1, 1 << 24), (0, 3000), (1, 6144), (0, 0), (1, -4096),
                                            (0, 1 << 30), (2, 2048), (-1, 4096)])
def test_other_shapes_still_refused_with_the_new_range(L, hint, frame_len):
    for init in (L.llz_analysis_fft_init, L.llz_synthesis_fft_init):
        assert init(hint, frame_len, po.HAMMING) == capi.BAD_HANDLE
        msg = capi.last_error()
        assert _size_refusal(msg) and "2..16777216" in msg, msg
    assert L.llz_stft_mc_init(2, hint, frame_len, po.HAMMING) == capi.BAD_HANDLE
    msg = capi.last_error()
    assert _size_refusal(msg) and "8..16777216" in msg, msg


def test_fixture_is_the_checker_at_8192(oracle):
    d = np.load(os.path.join(G, "stft_large.npz"), allow_pickle=False)
    hint, frame_len, win = int(d["hint"]), int(d["frame_len"]), int(d["win"])
    assert frame_len << (2 if hint == 0 else 1) == 8192
    re, im = oracle.stft_analysis(hint, frame_len, win, d["x"])
    assert re.shape == (len(d["x"]) // frame_len, 4097)
    assert np.array_equal(re, d["re"]) and np.array_equal(im, d["im"])
    assert np.array_equal(oracle.stft_synthesis(hint, frame_len, win, d["re"], d["im"]), d["syn"])


@pytest.mark.parametrize("hint,frame_len,win", [(0, 2048, po.HAMMING), (1, 8192, po.BLACKMAN), (0, 16384, po.KAISER),
                                                (1, 131072, po.HAMMING), (0, 262144, po.BLACKMAN)])
def test_oracle_equals_reference_library(oracle, ref, hint, frame_len, win):
    frames = 3
    rng = np.random.default_rng(frame_len + hint)
    x = rng.uniform(-1, 1, frames * frame_len)
    re, im = ref.stft_analysis(hint, frame_len, win, x)
    ore, oim = oracle.stft_analysis(hint, frame_len, win, x)
    assert np.array_equal(ore, re) and np.array_equal(oim, im)
    assert np.array_equal(oracle.stft_synthesis(hint, frame_len, win, re, im), ref.stft_synthesis(hint, frame_len, win, re, im))
