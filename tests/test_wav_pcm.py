"""WAV container and PCM ingest: the oracle's restatement of libllzaudio/llz_wavfmt.c is pinned
against the reference's own reader / writer (their results recorded in tests/golden/wav.npz by oracle/gen_golden.py), the product's
host parser against the oracle, and the device de-interleaver against the oracle's PCM functions."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402


def make_wav(channels, rate, frames, seed, extra_before_fmt=b"", extra_before_data=b"", fmt_extra=b"", bits=16):
    rng = np.random.default_rng(seed)
    pcm = rng.integers(-32768, 32768, (frames, channels)).astype("<i2")
    block = channels * ((bits + 7) // 8)
    fmt = struct.pack("<HHIIHH", 1, channels, rate, rate * block, block, bits) + fmt_extra
    body = b"WAVE" + extra_before_fmt + b"fmt " + struct.pack("<I", len(fmt)) + fmt + extra_before_data + \
        b"data" + struct.pack("<I", pcm.nbytes) + pcm.tobytes()
    return b"RIFF" + struct.pack("<I", len(body)) + body, pcm


def chunk(cid, payload):
    return cid + struct.pack("<I", len(payload)) + payload


CASES = [dict(channels=1, rate=48000, frames=100, seed=1),
         dict(channels=2, rate=44100, frames=333, seed=2, extra_before_data=chunk(b"LIST", b"x" * 26)),
         dict(channels=6, rate=96000, frames=57, seed=3, extra_before_fmt=chunk(b"JUNK", b"\0" * 12), fmt_extra=b"\0\0"),
         dict(channels=64, rate=16000, frames=40, seed=4, extra_before_fmt=chunk(b"bext", b"b" * 8),
              extra_before_data=chunk(b"fact", b"1234") + chunk(b"LIST", b"yy"))]
WRITER_CASES = ((1, 44100, 216090 // 2), (2, 48000, 1000), (8, 16000, 12345))
WAV_FIELDS = ("format", "channels", "samplerate", "bytes_per_sample", "block_align", "frames", "data_offset")


def case_id(case):
    return f"{case['channels']}ch"


@pytest.fixture(scope="module")
def oracle():
    return po.Oracle()


@pytest.fixture(scope="module")
def ref_wav():
    """the reference's own reader / writer results on these images (tests/golden/wav.npz, oracle/gen_golden.py)"""
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wav.npz"), allow_pickle=False)


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_oracle_wav_parse_matches_the_reference_reader(oracle, ref_wav, case):
    """(a chunk in FRONT of "fmt " is left out here: the reference's skip loop never re-reads the chunk id after its fseek,
    llz_wavfmt.c:108-114, and spins forever on such a file; the restatement re-reads it -- those images are compared between
    oracle and product only)"""
    img, _pcm = make_wav(**{k: v for k, v in case.items() if k != "extra_before_fmt"})
    assert img == ref_wav[f"read_{case_id(case)}_img"].tobytes(), "the image differs from the one the fixture was made on"
    ref = dict(zip(WAV_FIELDS, (int(v) for v in ref_wav[f"read_{case_id(case)}"])))
    got = oracle.wav_parse(img)
    assert got == ref


def test_oracle_wav_header_matches_the_reference_writer(oracle, ref_wav):
    for ch, rate, frames in WRITER_CASES:
        ref = ref_wav[f"write_{ch}_{rate}_{frames}"].tobytes()
        assert len(ref) == 44 and oracle.wav_header(ch, rate, 2, frames) == ref


def test_oracle_wav_known_answers(oracle):
    """fixture-free pins: the 44-byte header of a 2-channel 48 kHz file, and refusals"""
    h = oracle.wav_header(2, 48000, 2, 10)
    assert h == b"RIFF" + struct.pack("<I", 76) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, 48000, 192000, 4, 16) + \
        b"data" + struct.pack("<I", 40)
    assert oracle.wav_parse(h + b"\0" * 40) == {"format": 1, "channels": 2, "samplerate": 48000, "bytes_per_sample": 2,
                                                 "block_align": 4, "frames": 10, "data_offset": 44}
    assert oracle.wav_parse(b"RIFX" + h[4:]) is None
    assert oracle.wav_parse(h[:30]) is None
    img, _ = make_wav(1, 8000, 4, 9)
    assert oracle.wav_parse(img.replace(struct.pack("<HH", 1, 1), struct.pack("<HH", 3, 1), 1)) is None     # float format


def test_oracle_pcm_functions(oracle):
    il = np.array([[1, -2], [32767, -32768], [0, 255]], dtype=np.int16)
    pl = oracle.pcm_deinterleave(il)
    assert np.array_equal(pl, il.T.astype(np.float32) / np.float32(32768))
    x = np.array([[0.99999, -1.5, 0.5 / 32768, -0.5 / 32768, 1.0, -1.0, 2.6 / 32768, -2.6 / 32768]], dtype=np.float32)
    assert oracle.pcm_interleave(x).ravel().tolist() == [32767, -32768, 0, 0, 32767, -32768, 2, -2]


@pytest.mark.parametrize("case", CASES, ids=[f"{c['channels']}ch" for c in CASES])
def test_product_wav_parse_matches_oracle(oracle, case):
    """llz_wav_parse / llz_wav_write_header are host C in the product library: no GPU needed"""
    from llzlab_amd import capi
    L = capi.lib()
    img, _pcm = make_wav(**case)
    info = capi.WavInfo()
    assert L.llz_wav_parse(img, len(img), C.byref(info)) == 0, capi.last_error()
    assert info.as_dict() == oracle.wav_parse(img)
    hdr = (C.c_ubyte * 44)()
    assert L.llz_wav_write_header(hdr, C.byref(info)) == 0
    assert bytes(hdr) == oracle.wav_header(info.channels, info.samplerate, info.bytes_per_sample, info.frames)
    for bad in (b"RIFX" + img[4:], img[:20], img.replace(b"data", b"dat_")):
        assert L.llz_wav_parse(bad, len(bad), C.byref(info)) < 0 and capi.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{c['channels']}ch" for c in CASES])
def test_wav_ingest_on_the_device_matches_oracle(oracle, case):
    import torch
    from llzlab_amd import capi
    assert torch.cuda.is_available()
    L = capi.lib()
    capi.check(L.llz_hip_set_device(0), "set_device")
    img, pcm = make_wav(**case)
    info = capi.WavInfo()
    out = torch.empty(case["channels"], case["frames"], dtype=torch.float32, device="cuda:0")
    n = L.llz_wav_ingest_f32(img, len(img), out.data_ptr(), case["frames"], C.byref(info), None)
    assert n == case["frames"], capi.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), oracle.pcm_deinterleave(pcm))
    # a truncated file: only the frames that are there
    cut = img[:len(img) - 3 * info.block_align - 1]
    out2 = torch.empty(case["channels"], case["frames"] - 4, dtype=torch.float32, device="cuda:0")
    n2 = L.llz_wav_ingest_f32(cut, len(cut), out2.data_ptr(), case["frames"], C.byref(info), None)
    assert n2 == case["frames"] - 4
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy(), oracle.pcm_deinterleave(pcm[:n2]))
