"""GPU: one result whatever kind of buffer the caller hands over.  The host layer of the transform and analysis family uses device
memory where it lies and stages everything else (csrc/host/llz_util.c: llz_stage_in / llz_stage_out, the llz_vec_stage_* of the
16-byte rule, llz_bind of the one-shot calls); every entry point below is run on the same input

  * with host buffers,
  * with device buffers,
  * with device buffers on a stream of the caller's (set_stream, or the stream argument of the one-shot calls),
  * and, for the handles whose kernels take rows on a 16-byte boundary, with device buffers one element off such a boundary,

and every output must be bit-identical across the variants.  What the kernels compute is the parity tests' matter
(test_gpu_parity.py, test_transform_signals_gpu.py), and offsets against the oracle between guard bands are
test_buffer_contract_gpu.py's; the shapes here are the smallest that reach each path: the register and the LDS form of the direct
correlation (p 5 / 40), the fused and the split LPC, the one-launch and the composed STFT (fft_len 64 / 8192), the register / LDS
and the large transform (8 / 8192 points), all three fixed-point MDCT forms, streaming handles called twice."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi  # noqa: E402

HOST, DEV, STREAM, OFF = "host", "device", "device+stream", "device+1 element"
F32, I32, I16, F64 = np.float32, np.int32, np.int16, np.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


class Buffers:
    """The caller's buffers of one variant: numpy arrays, or views of device tensors at offset 0 or 1 element."""

    def __init__(self, kind, dev):
        self.kind, self.dev, self.keep = kind, dev, []
        self.torch_stream = torch.cuda.Stream(device=dev) if kind == STREAM else None
        self.stream = self.torch_stream.cuda_stream if kind == STREAM else None

    def buf(self, a):
        """a buffer holding `a` (an output: any array of its shape); returns (pointer, fetch)"""
        a = np.ascontiguousarray(a)
        if self.kind == HOST:
            h = a.copy()
            self.keep.append(h)
            return h.ctypes.data, lambda: h.copy()
        off = 1 if self.kind == OFF else 0
        t = torch.zeros(a.size + 4, dtype=getattr(torch, a.dtype.name), device=self.dev)
        v = t[off:off + a.size]
        v.copy_(torch.from_numpy(a.reshape(-1)))
        self.keep.append(t)
        assert v.data_ptr() % 16 == off * a.itemsize
        return v.data_ptr(), lambda: v.cpu().numpy().reshape(a.shape).copy()

    def ready(self):
        torch.cuda.synchronize()        # the inputs are in place before a call on another stream reads them

    def done(self):
        torch.cuda.synchronize()


def rnd(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


def ok(rc, what, want=0):
    assert rc == want, f"{what}: {rc} ({capi.last_error()})"


# ---- the cases: case(L, b) -> list of output arrays ----

def one_shot_corr(which, p, two_sided=0, alias=False):
    def case(L, b):
        x, y = rnd(1, 3, 80), rnd(2, 3, 80)
        px, _ = b.buf(x)
        py = px if alias else b.buf(y)[0]
        width = {"auto": p + 1, "cross": 2 * p + 1 if two_sided else p + 1, "cof": 1}[which]
        pr, get = b.buf(np.zeros((3, width), F32))
        b.ready()
        if which == "auto":
            ok(L.llz_autocorr_mc(px, pr, 3, 80, p, b.stream), "llz_autocorr_mc")
        elif which == "cross":
            ok(L.llz_crosscorr_mc(px, py, pr, 3, 80, p, two_sided, b.stream), "llz_crosscorr_mc")
        else:
            ok(L.llz_corr_cof_mc(px, py, pr, 3, 80, b.stream), "llz_corr_cof_mc")
        b.done()
        return [get()]
    return case


def lpc_mc(split, window):
    def case(L, b):
        frames, n, p = 3, 64, 4
        px, _ = b.buf(rnd(3, frames, n))
        pw = b.buf(np.hanning(n).astype(F32))[0] if window else None
        outs = [b.buf(np.zeros(s, F32)) for s in ((frames, p + 1), (frames, p), (frames,), (frames,), (frames, p + 1))]
        b.ready()
        with capi.tuned(**({"lpc_split": 1} if split else {})):
            ok(L.llz_lpc_mc(px, pw, *[o[0] for o in outs], frames, n, p, b.stream), "llz_lpc_mc")
        b.done()
        return [o[1]() for o in outs]
    return case


def handle(L, b, init, uninit, set_stream, *args):
    h = init(*args)
    assert h != capi.BAD_HANDLE, capi.last_error()
    if b.stream is not None:
        ok(set_stream(h, b.stream), "set_stream")
    return h, lambda: uninit(h)


def fast_corr(cross):
    def case(L, b):
        px, py = b.buf(rnd(4, 3, 30))[0], b.buf(rnd(5, 3, 30))[0]
        pr, get = b.buf(np.zeros((3, 11 if cross else 6), F32))
        b.ready()
        if cross:
            h, close = handle(L, b, L.llz_crosscorr_fast_mc_init, L.llz_crosscorr_fast_mc_uninit, L.llz_crosscorr_fast_mc_set_stream, 3, 30)
            ok(L.llz_crosscorr_fast_mc(h, px, py, pr, 5, 1), "llz_crosscorr_fast_mc")
        else:
            h, close = handle(L, b, L.llz_autocorr_fast_mc_init, L.llz_autocorr_fast_mc_uninit, L.llz_autocorr_fast_mc_set_stream, 3, 30)
            ok(L.llz_autocorr_fast_mc(h, px, pr, 5), "llz_autocorr_fast_mc")
        b.done()
        close()
        return [get()]
    return case


def lpc_filter(L, b):
    ch, flen, p, frames = 2, 32, 4, 2
    acof = np.zeros((ch, frames, p + 1), F32)
    acof[..., 0] = 1
    acof[..., 1:] = 0.1 * rnd(6, ch, frames, p)            # |a| small: a stable all-pole filter
    h, close = handle(L, b, L.llz_lpc_filter_mc_init, L.llz_lpc_filter_mc_uninit, L.llz_lpc_filter_mc_set_stream, ch, flen, p)
    got = []
    for call in range(2):
        px, pa = b.buf(rnd(7 + call, ch, frames * flen))[0], b.buf(acof)[0]
        (pe, get_e), (py, get_y) = b.buf(np.zeros((ch, frames * flen), F32)), b.buf(np.zeros((ch, frames * flen), F32))
        b.ready()
        ok(L.llz_lpc_residual_mc(h, px, pa, pe, frames), "llz_lpc_residual_mc", frames)
        ok(L.llz_lpc_synth_mc(h, pe, pa, py, frames), "llz_lpc_synth_mc", frames)
        b.done()
        got += [get_e(), get_y()]
    close()
    return got


def stft(channels, frame_len, frames, calls):
    def case(L, b):
        h, close = handle(L, b, L.llz_stft_mc_init, L.llz_stft_mc_uninit, L.llz_stft_mc_set_stream, channels, capi.OVERLAP_LOW,
                          frame_len, capi.HAMMING)
        bins = L.llz_stft_mc_bins(h)
        got = []
        for call in range(calls):
            px = b.buf(rnd(9 + call, channels, frames * frame_len))[0]
            (pre, get_re), (pim, get_im) = b.buf(np.zeros((channels, frames, bins), F32)), b.buf(np.zeros((channels, frames, bins), F32))
            py, get_y = b.buf(np.zeros((channels, frames * frame_len), F32))
            b.ready()
            ok(L.llz_stft_mc_analysis(h, px, pre, pim, frames), "llz_stft_mc_analysis", frames)
            ok(L.llz_stft_mc_synthesis(h, pre, pim, py, frames), "llz_stft_mc_synthesis", frames)
            b.done()
            got += [get_re(), get_im(), get_y()]
        close()
        return got
    return case


def mdct_batch(L, b):
    n, count = 32, 3
    h, close = handle(L, b, L.llz_mdct_batch_init, L.llz_mdct_batch_uninit, L.llz_mdct_batch_set_stream, n)
    px = b.buf(rnd(11, count, n))[0]
    (pX, get_X), (py, get_y) = b.buf(np.zeros((count, n // 2), F32)), b.buf(np.zeros((count, n), F32))
    b.ready()
    ok(L.llz_mdct_batch(h, px, pX, count), "llz_mdct_batch", count)
    ok(L.llz_imdct_batch(h, pX, py, count), "llz_imdct_batch", count)
    b.done()
    close()
    return [get_X(), get_y()]


def mdct_frames(L, b):
    ch, flen, frames = 2, 128, 2
    h, close = handle(L, b, L.llz_mdct_frames_mc_init, L.llz_mdct_frames_mc_uninit, L.llz_mdct_frames_mc_set_stream, ch, flen,
                      capi.MDCT_SINE)
    got = []
    for call in range(2):
        px = b.buf(rnd(12 + call, ch, frames * flen))[0]
        (pX, get_X), (py, get_y) = b.buf(np.zeros((ch, frames, flen), F32)), b.buf(np.zeros((ch, frames * flen), F32))
        b.ready()
        ok(L.llz_mdct_frames_mc_analysis(h, px, pX, frames), "llz_mdct_frames_mc_analysis", frames)
        ok(L.llz_mdct_frames_mc_synthesis(h, pX, py, frames), "llz_mdct_frames_mc_synthesis", frames)
        b.done()
        got += [get_X(), get_y()]
    close()
    return got


def mdct_fixed(form):
    def case(L, b):
        n, count = 64, 2
        h, close = handle(L, b, L.llz_mdct_fixed_init, L.llz_mdct_fixed_uninit, L.llz_mdct_fixed_set_stream, form, n)
        x = np.random.default_rng(14).integers(-(1 << 20), 1 << 20, (count, n)).astype(I32)
        px = b.buf(x)[0]
        (pX, get_X), (py, get_y) = b.buf(np.zeros((count, n // 2), I32)), b.buf(np.zeros((count, n), I32))
        b.ready()
        ok(L.llz_mdct_fixed_batch(h, px, pX, count), "llz_mdct_fixed_batch", count)
        ok(L.llz_imdct_fixed_batch(h, pX, py, count), "llz_imdct_fixed_batch", count)
        b.done()
        close()
        return [get_X(), get_y()]
    return case


def fft_batch(size, fixed):
    def case(L, b):
        count = 2
        if fixed:
            h, close = handle(L, b, L.llz_fft_fixed_init, L.llz_fft_fixed_uninit, L.llz_fft_fixed_set_stream, size)
            data = np.random.default_rng(15).integers(-(1 << 20), 1 << 20, (count, 2 * size)).astype(I32)
            fwd, inv = L.llz_fft_fixed_batch, L.llz_ifft_fixed_batch
        else:
            h, close = handle(L, b, L.llz_fft_batch_init, L.llz_fft_batch_uninit, L.llz_fft_batch_set_stream, size)
            data = rnd(16, count, 2 * size)
            fwd, inv = L.llz_fft_batch, L.llz_ifft_batch
        pd, get = b.buf(data)
        b.ready()
        ok(fwd(h, pd, count), "forward transform")
        b.done()
        got = [get()]
        ok(inv(h, pd, count), "inverse transform")
        b.done()
        close()
        return got + [get()]
    return case


def csd(L, b):
    ch, pairs, n_fft, hop, bins = 2, 2, 64, 32, 33
    table = (C.c_int * 4)(0, 1, 1, 1)
    h, close = handle(L, b, L.llz_csd_mc_init, L.llz_csd_mc_uninit, L.llz_csd_mc_set_stream, ch, pairs, table, n_fft, hop, capi.HAMMING)
    for call in range(2):
        px = b.buf(rnd(17 + call, ch, 5 * hop))[0]
        b.ready()
        assert L.llz_csd_mc_update(h, px, 5 * hop) == 5 * (call + 1) - 1, capi.last_error()
    got = []
    for what in (capi.SPEC_PXX, capi.SPEC_PYY, capi.SPEC_CSD, capi.SPEC_COHERENCE, capi.SPEC_TF):
        po, get = b.buf(np.zeros((pairs, bins, 2 if what in (capi.SPEC_CSD, capi.SPEC_TF) else 1), F32))
        ok(L.llz_csd_mc_read(h, what, po), "llz_csd_mc_read")
        b.done()
        got.append(get())
    po, get = b.buf(np.zeros((pairs, bins, 4), F64))
    ok(L.llz_csd_mc_read_raw(h, po), "llz_csd_mc_read_raw")
    b.done()
    got.append(get())
    close()
    return got


def pcm(L, b):
    ch, n = 3, 17
    s = np.random.default_rng(19).integers(-32768, 32768, (n, ch)).astype(I16)
    ps = b.buf(s)[0]
    (pf, get_f), (pb, get_b) = b.buf(np.zeros((ch, n), F32)), b.buf(np.zeros((n, ch), I16))
    b.ready()
    ok(L.llz_pcm_deinterleave_i16_f32(ps, pf, ch, n, 1.0 / 32768, b.stream), "llz_pcm_deinterleave_i16_f32")
    ok(L.llz_pcm_interleave_f32_i16(pf, pb, ch, n, 32768.0, b.stream), "llz_pcm_interleave_f32_i16")
    b.done()
    return [get_f(), get_b()]


PLAIN, VEC = (HOST, DEV, STREAM), (HOST, DEV, STREAM, OFF)     # VEC: the handles under the 16-byte rule
CASES = {
    "autocorr_mc p5": (one_shot_corr("auto", 5), PLAIN), "autocorr_mc p40": (one_shot_corr("auto", 40), PLAIN),
    "crosscorr_mc p5": (one_shot_corr("cross", 5), PLAIN), "crosscorr_mc p40": (one_shot_corr("cross", 40), PLAIN),
    "crosscorr_mc p5 two-sided": (one_shot_corr("cross", 5, 1), PLAIN),
    "crosscorr_mc p40 two-sided": (one_shot_corr("cross", 40, 1), PLAIN),
    "crosscorr_mc y == x": (one_shot_corr("cross", 5, 1, alias=True), PLAIN),
    "corr_cof_mc": (one_shot_corr("cof", 0), PLAIN), "corr_cof_mc b == a": (one_shot_corr("cof", 0, alias=True), PLAIN),
    "lpc_mc": (lpc_mc(0, 0), PLAIN), "lpc_mc window": (lpc_mc(0, 1), PLAIN),
    "lpc_mc split": (lpc_mc(1, 0), PLAIN), "lpc_mc split window": (lpc_mc(1, 1), PLAIN),
    "autocorr_fast_mc": (fast_corr(0), PLAIN), "crosscorr_fast_mc": (fast_corr(1), PLAIN),
    "lpc_residual_mc, lpc_synth_mc": (lpc_filter, PLAIN),
    "stft_mc 2 x 32": (stft(2, 32, 3, 2), PLAIN), "stft_mc 1 x 4096 composed": (stft(1, 4096, 2, 1), PLAIN),
    "mdct_batch": (mdct_batch, VEC), "mdct_frames_mc": (mdct_frames, VEC),
    "mdct_fixed origin": (mdct_fixed(0), PLAIN), "mdct_fixed fft": (mdct_fixed(1), PLAIN), "mdct_fixed fft4": (mdct_fixed(2), PLAIN),
    "fft_batch 8": (fft_batch(8, 0), VEC), "fft_batch 8192": (fft_batch(8192, 0), VEC), "fft_fixed_batch 64": (fft_batch(64, 1), VEC),
    "csd_mc": (csd, PLAIN), "pcm": (pcm, PLAIN),
}


@pytest.mark.parametrize("name", list(CASES))
def test_every_kind_of_buffer_gives_the_same_bits(dev, name):
    case, kinds = CASES[name]
    L = capi.lib()
    want = None
    for kind in kinds:
        got = case(L, Buffers(kind, dev))
        assert all(np.isfinite(g).all() for g in got), (name, kind)
        if want is None:
            want = got
            assert any(np.any(g != 0) for g in want), name      # the call wrote something
            continue
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape
            assert g.tobytes() == w.tobytes(), f"{name}: output {k} with {kind} buffers differs from {HOST}: " \
                                               f"{int(np.sum(g != w))} of {g.size} elements"
