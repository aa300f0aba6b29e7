"""The float32 transforms on the GPU, every bin, sample, row, channel and frame: llz_fft_batch, llz_stft_mc_*, llz_mdct_batch and
llz_mdct_frames_mc_* on the signal rows of tests/transform_checks.py (impulses, single-bin tones, a zero row, one noise row and
its copies times 2^-20 .. 2^+10), each element against the limit derived there from the double oracle, scaled rows bit for bit
against their base row, exact zeros where the input is silent.  Every kernel family at the smallest size that reaches it, both
directions, in its default form and under its tune; the batch counts leave a partial last workgroup; outputs are pre-filled
with 7.0 so that an unwritten element is a wrong element.  Each test prints the worst fraction of its limit (DESIGN.md keeps
the observed ones; none is a gate)."""
import contextlib

import numpy as np
import pytest

from tests import transform_checks as tc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def _tuned(name, value=1):
    return capi.tuned(**{name: value}) if name else contextlib.nullcontext()


def _filled(dev, *shape):
    return torch.full(shape, tc.SENTINEL, dtype=torch.float32, device=dev)


def _up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------ FftBatch
@pytest.mark.parametrize("n,generic", tc.FFT_CASES)
def test_fft_batch_signals(dev, oracle, n, generic):
    count = tc.fft_count(n, generic)
    specs = tc.fft_specs(n, count, tc.fft_group(n, generic)[0])
    x = tc.make_rows(n, specs)
    base_of, exps = tc.scaled_pairs(specs)
    got = {False: [], True: []}
    with _tuned("fft_generic" if generic else None):
        fb = filters.FftBatch(n)
        for o in range(0, len(specs), count):                          # one call per `count` rows
            for inverse in (False, True):
                zd = _up(dev, x[o:o + count].view(np.float32))
                (fb.ifft if inverse else fb.fft)(zd, count)
                got[inverse].append(zd.cpu().numpy().view(np.complex64).reshape(count, n))
        fb.close()
    silent = ~np.any(x != 0, axis=1)[:, None]
    worst = {}
    for inverse, name in ((False, "forward"), (True, "inverse")):
        g = np.concatenate(got[inverse])
        ref = tc.fft_reference(lambda z, inv: oracle.fft(z, inverse=inv), n, specs, x, inverse)
        worst[name] = tc.limit_check(g, ref, tc.fft_limit(x, n, inverse), f"fft batch {n} {name}")
        tc.scaled_equal(g, base_of, exps, f"fft batch {n} {name}")
        tc.zero_where_silent(g, silent, f"fft batch {n} {name}")
    print(f"FRACTION | {tc.fft_family(n, generic)} | FftBatch {n}{' fft_generic' if generic else ''} | "
          f"forward {worst['forward']:.3f} | inverse {worst['inverse']:.3f}")


# ------------------------------------------------------------------------------------------------ StftMC
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("hint", [0, 1])
@pytest.mark.parametrize("fft_len,tune", tc.STFT_CASES)
def test_stft_mc_signals(dev, oracle, fft_len, tune, hint, which):
    N = fft_len
    F = N >> (2 if hint == 0 else 1)
    win = tc.stft_window(N, hint)
    T = tc.frames_total(N)
    calls = tc.frame_calls(which, T)
    x, base_of, exps, names, info = tc.frame_channels(which, F, N, calls)
    C = x.shape[0]
    w = oracle.window(win, N)
    ref = tc.stft_analysis_ref(oracle, x, base_of, hint, F, win)
    S32 = ref.astype(np.complex64)                                     # the synthesis is given the oracle's own spectra
    ref_x = tc.stft_synthesis_ref(oracle, S32, base_of, hint, F, win)
    res, xs, o = [], [], 0
    with _tuned(tune):
        f = filters.StftMC(C, hint, F, win)
        assert f.bins == N // 2 + 1
        for frames in calls:
            re, im = _filled(dev, C, frames, f.bins), _filled(dev, C, frames, f.bins)
            f.analysis(_up(dev, x[:, o * F:(o + frames) * F]), re, im)
            res.append(re.cpu().numpy() + 1j * im.cpu().numpy())
            xo = _filled(dev, C, frames * F)
            f.synthesis(_up(dev, S32.real[:, o:o + frames]), _up(dev, S32.imag[:, o:o + frames]), xo)
            xs.append(xo.cpu().numpy())
            o += frames
        f.close()
    got, out = np.concatenate(res, axis=1).astype(np.complex64), np.concatenate(xs, axis=1)
    what = f"stft {N} hint {hint} {which}"
    wa = tc.limit_check(got, ref, tc.stft_analysis_limit(x, w, F, N), what + " analysis")
    tc.scaled_equal(got, base_of, exps, what + " analysis")
    tc.zero_where_silent(got, tc.silent_frames(x, F, N), what + " analysis")
    tc.zero_where_ref_zero(got.imag[:, :, [0, N // 2]], ref.imag[:, :, [0, N // 2]], what + " analysis, bins 0 and N/2")
    for c, fr in tc.centre_frames(x, F, N):
        tc.zero_where_ref_zero(got[c, fr].imag, ref[c, fr].imag, what + " analysis, impulse at the window centre")
    ws = tc.limit_check(out, ref_x, tc.stft_synthesis_limit(S32, w, hint, F, N, tc.stft_half(N, tune)), what + " synthesis")
    tc.scaled_equal(out, base_of, exps, what + " synthesis")
    tc.zero_where_silent(out, tc.silent_samples(S32, F, N), what + " synthesis")
    print(f"FRACTION | {tc.stft_family(N, tune)} | StftMC fft_len {N} hint {hint} channels {which} | analysis {wa:.3f} | synthesis {ws:.3f}")


# ------------------------------------------------------------------------------------------------ MdctBatch
@pytest.mark.parametrize("n", tc.MDCT_SIZES)
def test_mdct_batch_signals(dev, oracle, n):
    count = tc.mdct_count(n)
    worst = {}
    m = filters.MdctBatch(n)
    for inverse, name in ((False, "forward"), (True, "inverse")):
        n_in, n_out = (n // 2, n) if inverse else (n, n // 2)
        specs = tc.fft_specs(n_in, count, tc.MDCT_E.get(n))
        x = tc.make_rows(n_in, specs, real=True)
        base_of, exps = tc.scaled_pairs(specs)
        outs = []
        for o in range(0, len(specs), count):
            yd = _filled(dev, count, n_out)
            (m.inverse if inverse else m.forward)(_up(dev, x[o:o + count]), yd)
            outs.append(yd.cpu().numpy())
        got = np.concatenate(outs)
        run = (lambda r: oracle.imdct(2, r)) if inverse else (lambda r: oracle.mdct(2, r))
        ref = tc.real_reference(run, specs, x, n_out)
        worst[name] = tc.limit_check(got, ref, tc.imdct_limit(x, n) if inverse else tc.mdct_limit(x, n), f"mdct batch {n} {name}")
        tc.scaled_equal(got, base_of, exps, f"mdct batch {n} {name}")
        tc.zero_where_silent(got, ~np.any(x != 0, axis=1)[:, None], f"mdct batch {n} {name}")
    m.close()
    print(f"FRACTION | {tc.mdct_family(n)} | MdctBatch {n} | forward {worst['forward']:.3f} | inverse {worst['inverse']:.3f}")


# ------------------------------------------------------------------------------------------------ MdctFramesMC
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("F,win,run", tc.MDCT_FRAME_CASES)
def test_mdct_frames_mc_signals(dev, oracle, F, win, run, which):
    T = tc.frames_total(2 * F)
    calls = tc.frame_calls(which, T)
    x, base_of, exps, names, info = tc.frame_channels(which, F, 2 * F, calls)
    C = x.shape[0]
    w = oracle.mdct_window(win, 2 * F)
    ref = tc.mdct_frames_analysis_ref(oracle, x, base_of, F, win)
    X32 = ref.astype(np.float32)                                       # the synthesis is given the oracle's own coefficients
    ref_x = tc.mdct_frames_synthesis_ref(oracle, X32, base_of, w, F)
    Xs, ys, o = [], [], 0
    with _tuned("mdct_run" if run else None, run):
        m = filters.MdctFramesMC(C, F, win)
        for frames in calls:
            Xd, yd = _filled(dev, C, frames, F), _filled(dev, C, frames * F)
            m.analysis(_up(dev, x[:, o * F:(o + frames) * F]), Xd)
            m.synthesis(_up(dev, X32[:, o:o + frames]), yd)
            Xs.append(Xd.cpu().numpy())
            ys.append(yd.cpu().numpy())
            o += frames
        m.close()
    got, out = np.concatenate(Xs, axis=1), np.concatenate(ys, axis=1)
    what = f"mdct frames {F} window {win} {which}"
    wa = tc.limit_check(got, ref, tc.mdct_frames_analysis_limit(x, w, F), what + " analysis")
    tc.scaled_equal(got, base_of, exps, what + " analysis")
    tc.zero_where_silent(got, tc.silent_frames(x, F, 2 * F), what + " analysis")
    ws = tc.limit_check(out, ref_x, tc.mdct_frames_synthesis_limit(X32, w, F), what + " synthesis")
    tc.scaled_equal(out, base_of, exps, what + " synthesis")
    tc.zero_where_silent(out, tc.silent_samples(X32, F, 2 * F), what + " synthesis")
    print(f"FRACTION | {tc.mdct_family(2 * F)} frames{f', runs of {run}' if run else ''} | MdctFramesMC frame_len {F} window {win} "
          f"channels {which} | analysis {wa:.3f} | synthesis {ws:.3f}")
