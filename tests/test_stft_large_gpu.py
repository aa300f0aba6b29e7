"""Windowed-FFT frames above 2048 points on the GPU: llz_analysis_fft / llz_synthesis_fft bit-identical to the reference
(the fixture of tools/gen_golden_stft_large.py and the CPU checker) up to 2^24 points, and the float32 batch llz_stft_mc_*
against the checker from 4096 to 2^20 points -- the one-launch kernels (4096), the composed form (above 4096, and 4096
under the fft_generic tune), chunk boundaries of the composed form, host buffers and a torch stream."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-5                      # the tolerance of test_stft_mc_vs_oracle_streaming
CHUNK_POINTS = 1 << 24          # LLZS_STFT_CHUNK_POINTS: points per chunk of the composed form


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def fft_len(hint, frame_len):
    return frame_len << (2 if hint == 0 else 1)


def run_symbols(hint, frame_len, win, x, re_in=None, im_in=None):
    """analysis of x frame by frame, then synthesis of (re_in, im_in) -- the analysis output when not given"""
    a = filters.AnalysisFft(hint, frame_len, win)
    frames = len(x) // frame_len
    res = [a.frame(x[f * frame_len:(f + 1) * frame_len]) for f in range(frames)]
    a.close()
    re, im = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    re_in, im_in = (re, im) if re_in is None else (re_in, im_in)
    s = filters.SynthesisFft(hint, frame_len, win)
    syn = np.concatenate([s.frame(re_in[f], im_in[f]) for f in range(frames)])
    s.close()
    return re, im, syn


def test_symbols_8192_vs_reference_fixture(dev):
    d = np.load(os.path.join(G, "stft_large.npz"), allow_pickle=False)
    hint, frame_len, win = int(d["hint"]), int(d["frame_len"]), int(d["win"])
    re, im, syn = run_symbols(hint, frame_len, win, d["x"])
    assert np.array_equal(re, d["re"]) and np.array_equal(im, d["im"])
    assert np.array_equal(syn, d["syn"])


@pytest.mark.parametrize("hint,frame_len,win,frames", [(0, 1 << 11, po.HAMMING, 5), (1, 1 << 13, po.BLACKMAN, 3),
                                                       (0, 1 << 13, po.KAISER, 4), (1, 1 << 15, po.HAMMING, 3),
                                                       (0, 1 << 15, po.BLACKMAN, 3), (1, 1 << 17, po.KAISER, 3),
                                                       (0, 1 << 17, po.HAMMING, 3), (1, 1 << 19, po.BLACKMAN, 2),
                                                       (0, 1 << 22, po.KAISER, 2)])
def test_symbols_exact_vs_oracle(dev, oracle, hint, frame_len, win, frames):
    """fft_len 2^13 .. 2^20 and 2^24: spectra and overlap-add output bit for bit, the 0.812 scale at 3/4 overlap included"""
    rng = np.random.default_rng(frame_len * 3 + hint)
    x = rng.uniform(-1, 1, frames * frame_len)
    ref_re, ref_im = oracle.stft_analysis(hint, frame_len, win, x)
    re, im, syn = run_symbols(hint, frame_len, win, x)
    assert np.array_equal(re, ref_re) and np.array_equal(im, ref_im)
    assert np.array_equal(syn, oracle.stft_synthesis(hint, frame_len, win, ref_re, ref_im))


def stft_mc_vs_oracle(dev, oracle, hint, frame_len, win, channels, frames, seed):
    """test_stft_mc_vs_oracle_streaming's check at the new sizes: two calls per direction, synthesis of the checker's own
    spectra (as float32)"""
    rng = np.random.default_rng(seed)
    n = frames * frame_len
    x = rng.uniform(-1, 1, (channels, 2 * n)).astype(np.float32)
    ref = [oracle.stft_analysis(hint, frame_len, win, row.astype(np.float64)) for row in x]
    ref_re = np.stack([r[0] for r in ref])
    ref_im = np.stack([r[1] for r in ref])
    ref_x = np.stack([oracle.stft_synthesis(hint, frame_len, win, ref_re[c].astype(np.float32), ref_im[c].astype(np.float32))
                      for c in range(channels)])
    f = filters.StftMC(channels, hint, frame_len, win)
    bins = f.bins
    assert bins == fft_len(hint, frame_len) // 2 + 1
    got_re, got_im, got_x = [], [], []
    for half in range(2):
        xd = torch.from_numpy(np.ascontiguousarray(x[:, half * n:(half + 1) * n])).to(dev)
        re = torch.empty(channels, frames, bins, dtype=torch.float32, device=dev)
        im = torch.empty_like(re)
        f.analysis(xd, re, im)
        got_re.append(re.cpu().numpy())
        got_im.append(im.cpu().numpy())
        sre = torch.from_numpy(np.ascontiguousarray(ref_re[:, half * frames:(half + 1) * frames]).astype(np.float32)).to(dev)
        sim = torch.from_numpy(np.ascontiguousarray(ref_im[:, half * frames:(half + 1) * frames]).astype(np.float32)).to(dev)
        xo = torch.empty(channels, n, dtype=torch.float32, device=dev)
        f.synthesis(sre, sim, xo)
        got_x.append(xo.cpu().numpy())
    f.close()
    got_re, got_im = np.concatenate(got_re, axis=1), np.concatenate(got_im, axis=1)
    got_x = np.concatenate(got_x, axis=1)
    scale = max(np.sqrt(np.mean(ref_re ** 2 + ref_im ** 2)), 1e-30)
    err = np.sqrt(np.mean((got_re - ref_re) ** 2 + (got_im - ref_im) ** 2))
    assert err <= TOL * max(scale, 1.0) and err / scale <= TOL, (err, scale)
    err_x = float(np.sqrt(np.mean((got_x - ref_x) ** 2)))
    assert err_x <= TOL and err_x / max(float(np.sqrt(np.mean(ref_x ** 2))), 0.05) <= TOL, err_x


MC_CASES = [(0, 1 << 10, po.HAMMING, 3, 7), (1, 1 << 11, po.BLACKMAN, 2, 1),        # 4096
            (0, 1 << 11, po.KAISER, 5, 3), (1, 1 << 12, po.HAMMING, 1, 5),          # 8192
            (0, 1 << 12, po.BLACKMAN, 2, 3), (1, 1 << 13, po.KAISER, 3, 1),         # 16384
            (1, 1 << 15, po.HAMMING, 2, 3), (0, 1 << 14, po.BLACKMAN, 1, 5),        # 65536
            (0, 1 << 18, po.KAISER, 2, 1), (1, 1 << 19, po.HAMMING, 1, 3)]          # 2^20


@pytest.mark.parametrize("hint,frame_len,win,channels,frames", MC_CASES)
def test_stft_mc_new_sizes_vs_oracle(dev, oracle, hint, frame_len, win, channels, frames):
    stft_mc_vs_oracle(dev, oracle, hint, frame_len, win, channels, frames, frame_len + 10 * hint + channels)


@pytest.mark.parametrize("hint,frame_len,win,channels,frames", [c for c in MC_CASES if fft_len(c[0], c[1]) <= 8192])
def test_stft_mc_composed_form_vs_oracle(dev, oracle, hint, frame_len, win, channels, frames):
    """fft_len 4096 and 8192 under the fft_generic tune: the composed form at both"""
    with capi.tuned(fft_generic=1):
        stft_mc_vs_oracle(dev, oracle, hint, frame_len, win, channels, frames, frame_len + 10 * hint + channels + 1)


@pytest.mark.parametrize("hint,frame_len", [(0, 1024), (1, 2048)])
def test_one_launch_and_composed_forms_agree(dev, hint, frame_len):
    """fft_len 4096: the one-launch kernels and the composed form (the fft_generic tune), both directions, to float32
    rounding, on spectra that are NOT Hermitian-consistent at bins 0 and N/2"""
    channels, frames = 3, 11
    N = fft_len(hint, frame_len)
    rng = np.random.default_rng(N + hint)
    x = torch.from_numpy(rng.uniform(-1, 1, (channels, frames * frame_len)).astype(np.float32)).to(dev)
    sre = torch.from_numpy(rng.uniform(-1, 1, (channels, frames, N // 2 + 1)).astype(np.float32)).to(dev)
    sim = torch.from_numpy(rng.uniform(-1, 1, (channels, frames, N // 2 + 1)).astype(np.float32)).to(dev)
    outs = []
    for generic in (-1, 1):
        with capi.tuned(fft_generic=generic):
            f = filters.StftMC(channels, hint, frame_len, po.KAISER)
            re = torch.empty(channels, frames, f.bins, dtype=torch.float32, device=dev)
            im = torch.empty_like(re)
            xo = torch.empty_like(x)
            for half in (slice(0, 6), slice(6, frames)):                    # streamed in two calls
                r, i = re[:, half].contiguous(), im[:, half].contiguous()
                f.analysis(x[:, half.start * frame_len:half.stop * frame_len].contiguous(), r, i)
                re[:, half], im[:, half] = r, i
                xh = torch.empty(channels, (half.stop - half.start) * frame_len, dtype=torch.float32, device=dev)
                f.synthesis(sre[:, half].contiguous(), sim[:, half].contiguous(), xh)
                xo[:, half.start * frame_len:half.stop * frame_len] = xh
            torch.cuda.synchronize()
            outs.append((re.cpu().numpy(), im.cpu().numpy(), xo.cpu().numpy()))
            f.close()
    for a, b in zip(outs[0], outs[1]):
        assert np.abs(a - b).max() <= 2e-5 * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("hint,frame_len,channels,frames", [(1, 1 << 19, 2, 9), (0, 1 << 14, 3, 100)])
def test_composed_form_across_chunks_vs_oracle(dev, oracle, hint, frame_len, channels, frames):
    """more transforms in one call than one scratch chunk holds (2^20: 16 per chunk, 65536: 256), a chunk boundary inside
    a channel: still the checker's results"""
    assert channels * frames > CHUNK_POINTS // fft_len(hint, frame_len)
    win = po.BLACKMAN
    rng = np.random.default_rng(frames)
    x = rng.uniform(-1, 1, (channels, frames * frame_len)).astype(np.float32)
    f = filters.StftMC(channels, hint, frame_len, win)
    xd = torch.from_numpy(x).to(dev)
    re = torch.empty(channels, frames, f.bins, dtype=torch.float32, device=dev)
    im = torch.empty_like(re)
    f.analysis(xd, re, im)
    ref = [oracle.stft_analysis(hint, frame_len, win, row.astype(np.float64)) for row in x]
    ref_re, ref_im = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    got_re, got_im = re.cpu().numpy(), im.cpu().numpy()
    scale = np.sqrt(np.mean(ref_re ** 2 + ref_im ** 2))
    assert np.sqrt(np.mean((got_re - ref_re) ** 2 + (got_im - ref_im) ** 2)) / scale <= TOL
    xo = torch.empty_like(xd)
    f.synthesis(re, im, xo)
    ref_x = np.stack([oracle.stft_synthesis(hint, frame_len, win, got_re[c], got_im[c]) for c in range(channels)])
    err_x = float(np.sqrt(np.mean((xo.cpu().numpy() - ref_x) ** 2)))
    assert err_x <= TOL and err_x / max(float(np.sqrt(np.mean(ref_x ** 2))), 0.05) <= TOL, err_x
    f.close()


def test_host_buffers_and_torch_stream(dev, oracle):
    """fft_len 16384: host numpy buffers (staged), then device buffers on a torch stream, against the checker"""
    hint, frame_len, win, channels, frames = 0, 4096, po.HAMMING, 2, 3
    rng = np.random.default_rng(16384)
    x = rng.uniform(-1, 1, (channels, frames * frame_len)).astype(np.float32)
    ref = [oracle.stft_analysis(hint, frame_len, win, row.astype(np.float64)) for row in x]
    ref_re, ref_im = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    ref_x = np.stack([oracle.stft_synthesis(hint, frame_len, win, ref_re[c].astype(np.float32), ref_im[c].astype(np.float32))
                      for c in range(channels)])
    scale = np.sqrt(np.mean(ref_re ** 2 + ref_im ** 2))

    def check(re, im, xo):
        assert np.sqrt(np.mean((re - ref_re) ** 2 + (im - ref_im) ** 2)) / scale <= TOL
        assert float(np.sqrt(np.mean((xo - ref_x) ** 2))) <= TOL

    f = filters.StftMC(channels, hint, frame_len, win)
    re = np.zeros((channels, frames, f.bins), dtype=np.float32)
    im = np.zeros_like(re)
    f.analysis(x, re, im)
    xo = np.zeros_like(x)
    f.synthesis(ref_re.astype(np.float32), ref_im.astype(np.float32), xo)
    check(re, im, xo)
    f.close()

    s = torch.cuda.Stream()
    f = filters.StftMC(channels, hint, frame_len, win, stream=s)
    with torch.cuda.stream(s):
        xd = torch.from_numpy(x).to(dev)
        red = torch.empty(channels, frames, f.bins, dtype=torch.float32, device=dev)
        imd = torch.empty_like(red)
        sre = torch.from_numpy(ref_re.astype(np.float32)).to(dev)
        sim = torch.from_numpy(ref_im.astype(np.float32)).to(dev)
        xod = torch.empty_like(xd)
        f.analysis(xd, red, imd)
        f.synthesis(sre, sim, xod)
    s.synchronize()
    check(red.cpu().numpy(), imd.cpu().numpy(), xod.cpu().numpy())
    f.close()
