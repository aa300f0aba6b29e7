"""GPU: the buffer contract of every batch entry point.  The parity tests check what a kernel computes, on fresh, 256-byte
aligned, padded tensors next to memory nobody looks at; here every caller buffer is carved out of a flat allocation
(tests/buffer_checks.py) at a chosen element offset from an aligned address, between guard bands:

  * outputs and their bands hold a sentinel NaN / 0x5a5a: after the call both bands are bit-unchanged (nothing was written
    outside the buffer) and the buffer meets the oracle under the gate of that path's parity test, every element compared;
  * inputs sit between poisoned bands (a quiet NaN; for integers +max and then -max-1, the two results bit-identical): a read
    in front of or behind a frame reaches the output, and view and bands are bit-unchanged after the call;
  * streaming handles are called twice, so the second call must take its history from the handle;
  * offsets (input, output) in elements take both sides of every pointer-alignment branch: 4-byte types (0,0) (1,0) (0,1)
    (1,3), int16 (0,0) (1,0) (2,0) (0,1) (4,2); several inputs or outputs get the same offset in allocations of their own.
    The in-place transforms have one buffer: offsets 0, 1, 3.

Each path runs one shape that fills its last tile and one that leaves it partial, none larger than its parity test's.
The second half pins aliasing: every out-of-place entry point refuses device input and output ranges that intersect, before
it stages or launches anything (llz_refuse_device_overlap, llz_util.c)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import rs_ragged_checks as rr  # noqa: E402
from tests.edge_checks import TOL, rms_check  # noqa: E402
from tests.test_lpc_host import levinson_py  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OFF32 = [(0, 0), (1, 0), (0, 1), (1, 3)]
OFF16 = [(0, 0), (1, 0), (2, 0), (0, 1), (4, 2)]
OFF_INPLACE = [(0, 0), (1, 1), (3, 3)]
F32, I32, I16 = torch.float32, torch.int32, torch.int16
ERR_ARG = -1                    # LLZ_ERR_ARG (include/llz_hip.h)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


_REFS = {}


def cached(key, make):
    """inputs and oracle results of a case, computed once and shared by its offsets (never modified)"""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


class Io:
    """the guarded buffers of one call sequence: inp() / out() carve them, verify() checks bands and inputs"""

    def __init__(self, dev, off, which="nan"):
        self.dev, self.off, self.which, self.ins, self.outs = dev, off, which, [], []

    def inp(self, data, *shape):
        buf = bc.carve_input(self.dev, data, self.off[0], which=self.which)
        self.ins.append((buf, bc.snapshot(buf)))
        return buf.shaped(*(shape or np.shape(data)))

    def out(self, dtype, *shape):
        buf = bc.carve(self.dev, dtype, int(np.prod(shape)), self.off[1])
        self.outs.append(buf)
        return buf.shaped(*shape)

    def inout(self, data):
        """the buffer of an in-place transform: its data between poisoned bands, which must survive"""
        buf = bc.carve_input(self.dev, data, self.off[0], which=self.which)
        self.outs.append(buf)
        return buf.view

    def verify(self, what):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                            # a faulted device serves no later test either: end the session here
            pytest.exit(f"{what}: the device reported an error, nothing more is run on it: {e}", returncode=3)
        for k, buf in enumerate(self.outs):
            bc.check_bands(buf, f"{what}: output {k}")
        for k, (buf, snap) in enumerate(self.ins):
            bc.check_untouched(buf, snap, f"{what}: input {k}")


def host(t):
    return t.detach().cpu().numpy().copy()


def equal_gate(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = np.flatnonzero(got.reshape(-1).view(np.uint8) != ref.reshape(-1).view(np.uint8))
    assert bad.size == 0, f"{what}: differs from the oracle in {bad.size} bytes, the first in element {bad[0] // got.itemsize}"


def scaled_rms_gate(got, ref, what):
    """the gate of the IIR wave-form and STFT parity tests: RMS error <= TOL absolute at unit scale and relative above it"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err, scale = float(np.sqrt(np.mean((got - ref) ** 2))), float(np.sqrt(np.mean(ref ** 2)))
    print(f"{what}: rms {err:.3g} scale {scale:.3g}")
    assert err <= TOL * max(1.0, scale) and err / max(scale, 1e-30) <= TOL, (what, err, scale)


# ================================================================================================ adapters
# adapter(dev, oracle, io, **case) -> {name: array}: the outputs, already gated against the oracle; the caller verifies the
# bands and, for integer inputs, compares the outputs of the two band fills
def run_fir(dev, oracle, io, algo, T, channels, n):
    def make():
        taps = oracle.fir_design(po.LPF, T, 0.2, 0.0, po.KAISER)
        x = oracle.synth_f32(channels, 2 * n, seed=T + n)
        xz = np.concatenate([x, np.zeros((channels, T - 1), np.float32)], axis=1)
        return taps, x, oracle.fir_batch_f32(xz, taps.astype(np.float32).astype(np.float64))
    taps, x, ref = cached(("fir", algo, T, channels, n), make)
    f = filters.FirFilterMC(channels, n, taps, algo=algo)
    assert f.algo == algo
    ys = []
    for o in (0, n):                                       # the second frame takes its history from the handle
        y = io.out(F32, channels, n)
        f.filter(io.inp(x[:, o:o + n]), y)
        ys.append(y)
    tail = io.out(F32, channels, T - 1)
    f.flush(tail)
    io.verify(f"fir algo {algo}")
    f.close()
    got = np.concatenate([host(t) for t in ys + [tail]], axis=1)
    rms_check(got, ref, f"fir algo {algo} T={T} {channels}x{n} + flush")
    return {"y": got}


def low_q(stages, radius):
    rows = []
    for k in range(stages):
        r, th = radius - 0.02 * k, 0.4 + 0.3 * k
        a1, a2 = -2 * r * np.cos(th), r * r
        rows.append([(1 + a1 + a2) / 4, (1 + a1 + a2) / 2, (1 + a1 + a2) / 4, 1.0, a1, a2])
    return np.array(rows)


def fixture_sections():
    d = np.load(os.path.join(G, "iir.npz"), allow_pickle=False)
    lo, hi = np.concatenate([d["b2"], d["a2"]]), np.concatenate([d["bq"], d["aq"]])
    return np.stack([lo, hi, lo, hi, lo])


def run_iir_cascade(dev, oracle, io, coef, tune, channels, n, precision=None):
    spec, coef = coef, fixture_sections() if coef == "fixture" else low_q(*coef)

    def make():
        x = oracle.synth_f32(channels, 2 * n, seed=n + channels)
        return x, oracle.iir_cascade_batch_f32(x, coef)
    x, ref = cached(("iirc", coef.tobytes(), channels, n), make)
    with capi.tuned(**tune):
        f = filters.IirCascadeMC(channels, coef)
        assert precision is None or f.precision == precision
        ys = []
        for o in (0, n):
            y = io.out(F32, channels, n)
            f.filter(io.inp(x[:, o:o + n]), y)
            ys.append(y)
        io.verify(f"iir cascade {tune}")
        f.close()
    got = np.concatenate([host(t) for t in ys], axis=1)
    # the parity tests' gates: rms_check for the fixture sections, at the output's scale for the resonant sets of the wave forms
    (rms_check if isinstance(spec, str) else scaled_rms_gate)(got, ref, f"iir cascade {tune} {channels}x{n}")
    return {"y": got}


def run_iir_mc(dev, oracle, io, a, b, channels, n):
    N = len(b) - 1

    def make():
        x = oracle.synth_f32(channels, 2 * n, seed=len(a) * 10 + len(b) + n)
        return x, np.stack([np.concatenate(oracle.iir_stream(np.array(a), np.array(b), row.astype(np.float64), flush=True))
                            for row in x])
    x, ref = cached(("iirg", tuple(a), tuple(b), channels, n), make)
    f = filters.IirMC(channels, a, b)
    ys = []
    for o in (0, n):
        y = io.out(F32, channels, n)
        f.filter(io.inp(x[:, o:o + n]), y)
        ys.append(y)
    tail = io.out(F32, channels, N)
    assert f.flush(tail) == N
    io.verify("iir_mc")
    f.close()
    got = np.concatenate([host(t) for t in ys + [tail]], axis=1)
    rms_check(got, ref, f"iir_mc M={len(a) - 1} N={N} {channels}x{n} + flush")
    return {"y": got}


def run_resample(dev, oracle, io, fmt, tune, L, M, win, channels, lens, gate="equal"):
    f32 = fmt == filters.PCM_F32

    def make():
        n = sum(lens)
        x = oracle.synth_f32(channels, n, seed=L + 2 * M) if f32 else oracle.synth_i16(channels, n, seed=L * 31 + M)
        # (ref_i16: the reference's frame loop; a length that is no whole number of its frames is zero-padded and cut)
        return x, (rr.ref_f32 if f32 else rr.ref_i16)(oracle, x, L, M, 1.0, win)
    x, ref = cached(("rs", f32, L, M, win, channels, tuple(lens)), make)
    with capi.tuned(**tune):
        r = filters.ResampleMC(channels, L, M, 1.0, win, fmt)
        ys, o = [], 0
        for n_in in lens:
            y = io.out(F32 if f32 else I16, channels, r.out_len(n_in))
            assert r.process(io.inp(x[:, o:o + n_in]), y) == y.shape[1]
            ys.append(y)
            o += n_in
        io.verify(f"resample {L}:{M} {tune}")
        r.close()
    got = np.concatenate([host(t) for t in ys], axis=1)
    what = f"resample {L}:{M} fmt {fmt} {tune} calls {lens}"
    if f32:
        rms_check(got, ref, what)
    elif gate == "equal":
        equal_gate(got, ref, what)
    else:                                                    # LLZ_PCM_I16_FAST on the float32-sum kernel: within one LSB
        diff = got.astype(np.int32) - ref.astype(np.int32)
        assert np.abs(diff).max() <= 1 and np.sqrt(np.mean(diff.astype(np.float64) ** 2)) <= 1e-5 * 32768, what
        assert np.mean(diff != 0) < 0.05, what
    return {"y": got}


def run_fft_batch(dev, oracle, io, n, count, tune):
    def make():
        rng = np.random.default_rng(n * 1000 + count)
        z = (rng.uniform(-1, 1, (count, n)) + 1j * rng.uniform(-1, 1, (count, n))).astype(np.complex64)
        return z, np.stack([oracle.fft(row.astype(np.complex128)) for row in z])
    z, ref = cached(("fftb", n, count), make)
    with capi.tuned(**tune):
        f = filters.FftBatch(n)
        data = io.inout(z.view(np.float32))
        f.fft(data, count)
        io.verify(f"fft_batch {n}")
        got = host(data).view(np.complex64).reshape(count, n)
        assert np.sqrt(np.mean(np.abs(got - ref) ** 2)) / np.sqrt(np.mean(np.abs(ref) ** 2)) < 1e-6, (n, count)
        f.ifft(data, count)                                  # round trip = identity
        io.verify(f"ifft_batch {n}")
        back = host(data).view(np.complex64).reshape(count, n)
        assert np.sqrt(np.mean(np.abs(back - z) ** 2)) < 1e-6, (n, count)
        f.close()
    return {"fwd": got, "back": back}


def run_fft_fixed(dev, oracle, io, n, count):
    def make():
        q = np.random.default_rng(n * 1000 + count).integers(-8000, 8001, (count, 2 * n)).astype(np.int32)
        fwd = np.stack([oracle.fft_fixed(row) for row in q])
        return q, fwd, np.stack([oracle.fft_fixed(row, inverse=True) for row in fwd])
    q, fwd, back = cached(("fftx", n, count), make)
    f = filters.FftFixed(n)
    data = io.inout(q)
    f.fft_batch(data, count)
    io.verify(f"fft_fixed_batch {n}")
    got = host(data).reshape(count, 2 * n)
    equal_gate(got, fwd, f"fft_fixed_batch {n} x {count}")
    f.ifft_batch(data, count)
    io.verify(f"ifft_fixed_batch {n}")
    got_back = host(data).reshape(count, 2 * n)
    equal_gate(got_back, back, f"ifft_fixed_batch {n} x {count}")
    f.close()
    return {"fwd": got, "back": got_back}


def run_autocorr(dev, oracle, io, tune, frames, n, p):
    def make():
        x = oracle.synth_f32(frames, n, seed=n + p)
        return x, np.stack([oracle.autocorr(row.astype(np.float64), p) for row in x])
    x, ref = cached(("acf", frames, n, p), make)
    r = io.out(F32, frames, p + 1)
    with capi.tuned(**tune):
        filters.autocorr_mc(io.inp(x), r, p)
        io.verify(f"autocorr_mc {tune}")
    got = host(r)
    assert np.max(np.abs(got.astype(np.float64) - ref)) <= 1e-5 * ref[:, 0].max(), (tune, frames, n, p)
    return {"r": got}


def run_autocorr_fast(dev, oracle, io, frames, n, p):
    def make():
        x = oracle.synth_f32(frames, n, seed=n)
        return x, np.stack([oracle.autocorr_fast(row.astype(np.float64), p) for row in x])
    x, ref = cached(("acff", frames, n, p), make)
    f = filters.AutocorrFastMC(frames, n)
    r = io.out(F32, frames, p + 1)
    f.run(io.inp(x), r, p)
    io.verify("autocorr_fast_mc")
    f.close()
    got = host(r)
    assert np.max(np.abs(got.astype(np.float64) - ref)) <= 1e-5 * np.abs(ref).max(), (frames, n, p)
    return {"r": got}


def lpc_expected(r, n, p):
    """float32(llz_levinson((double) r)) of one frame, as tests/test_lpc_gpu.py states it: acof, kcof, err, gain"""
    a, k, e = levinson_py(np.asarray(r, dtype=np.float32).astype(np.float64), p)
    gain = float(np.float32(r[0])) / e if e > 0 else 0.0
    with np.errstate(all="ignore"):
        return (np.array(a, dtype=np.float32), np.array(k, dtype=np.float32)[:p], np.float32(np.float64(e) / n), np.float32(gain))


def run_lpc(dev, oracle, io, tune, p, n, frames):
    def make():
        x = (np.random.default_rng(1000 * p + n + frames).standard_normal((frames, n)) * 0.3).astype(np.float32)
        return x, np.stack([oracle.autocorr(row.astype(np.float64), p) for row in x])
    x, r_ref = cached(("lpc", p, n, frames), make)
    acof, kcof, r = io.out(F32, frames, p + 1), io.out(F32, frames, p), io.out(F32, frames, p + 1)
    err, gain = io.out(F32, frames), io.out(F32, frames)
    with capi.tuned(**tune):
        filters.lpc_mc(io.inp(x), acof, kcof=kcof, err=err, gain=gain, r=r, p=p)
        io.verify(f"lpc_mc {tune}")
    got = {k: host(v) for k, v in (("acof", acof), ("kcof", kcof), ("err", err), ("gain", gain), ("r", r))}
    # r against the oracle under llz_autocorr_mc's gate; the recursion on those float32 values bit for bit
    assert np.max(np.abs(got["r"].astype(np.float64) - r_ref)) <= 1e-5 * r_ref[:, 0].max(), (tune, p, n, frames)
    want = [lpc_expected(got["r"][f], n, p) for f in range(frames)]
    for k, name in enumerate(("acof", "kcof", "err", "gain")):
        equal_gate(got[name], np.stack([w[k] for w in want]).reshape(got[name].shape), f"lpc_mc {tune} p={p}: {name}")
    return got


def run_stft(dev, oracle, io, tune, hint, frame_len, win, channels, frames):
    n = frames * frame_len

    def make():
        x = np.random.default_rng(hint * 1000 + frame_len + channels).uniform(-1, 1, (channels, 2 * n)).astype(np.float32)
        ref = [oracle.stft_analysis(hint, frame_len, win, row.astype(np.float64)) for row in x]
        re, im = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
        sx = np.stack([oracle.stft_synthesis(hint, frame_len, win, re[c].astype(np.float32), im[c].astype(np.float32))
                       for c in range(channels)])
        return x, re, im, sx
    x, ref_re, ref_im, ref_x = cached(("stft", hint, frame_len, win, channels, frames), make)
    with capi.tuned(**tune):
        f = filters.StftMC(channels, hint, frame_len, win)
        bins = f.bins
        res, ims, xs = [], [], []
        for half in range(2):                                # the second call takes history and overlap-add tail from the handle
            re, im = io.out(F32, channels, frames, bins), io.out(F32, channels, frames, bins)
            f.analysis(io.inp(x[:, half * n:(half + 1) * n]), re, im)
            xo = io.out(F32, channels, n)
            sl = slice(half * frames, (half + 1) * frames)
            f.synthesis(io.inp(ref_re[:, sl].astype(np.float32)), io.inp(ref_im[:, sl].astype(np.float32)), xo)
            res.append(re); ims.append(im); xs.append(xo)
        io.verify(f"stft {frame_len} {tune}")
        f.close()
    got_re, got_im = np.concatenate([host(t) for t in res], axis=1), np.concatenate([host(t) for t in ims], axis=1)
    got_x = np.concatenate([host(t) for t in xs], axis=1)
    scale = max(np.sqrt(np.mean(ref_re ** 2 + ref_im ** 2)), 1e-30)
    err = np.sqrt(np.mean((got_re - ref_re) ** 2 + (got_im - ref_im) ** 2))
    assert err <= TOL * max(scale, 1.0) and err / scale <= TOL, (err, scale)
    err_x = float(np.sqrt(np.mean((got_x - ref_x) ** 2)))
    assert err_x <= TOL and err_x / max(float(np.sqrt(np.mean(ref_x ** 2))), 0.05) <= TOL, err_x
    return {"re": got_re, "im": got_im, "x": got_x}


def run_mdct_frames(dev, oracle, io, F, win, channels, calls):
    def make():
        x = oracle.synth_f32(channels, sum(calls) * F, seed=F + channels)
        ref = [oracle.mdct_frames(F, win, row.astype(np.float64)) for row in x]
        return x, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    x, ref_X, ref_y = cached(("mdctf", F, win, channels, tuple(calls)), make)
    m = filters.MdctFramesMC(channels, F, win)
    Xs, ys, o = [], [], 0
    for frames in calls:
        X, y = io.out(F32, channels, frames, F), io.out(F32, channels, frames * F)
        m.analysis(io.inp(x[:, o * F:(o + frames) * F]), X)
        m.synthesis(io.inp(ref_X[:, o:o + frames].astype(np.float32)), y)
        Xs.append(X); ys.append(y)
        o += frames
    io.verify(f"mdct_frames {F}")
    m.close()
    got_X = np.concatenate([host(t) for t in Xs], axis=1)
    got_y = np.concatenate([host(t) for t in ys], axis=1)
    for c in range(channels):
        Xr = ref_X[c].reshape(got_X[c].shape)
        assert np.sqrt(np.mean((got_X[c] - Xr) ** 2)) <= TOL * max(1.0, np.sqrt(np.mean(Xr ** 2))), (F, c)
        assert np.sqrt(np.mean((got_y[c] - ref_y[c]) ** 2)) <= TOL, (F, c)
    return {"X": got_X, "y": got_y}


def run_mdct_batch(dev, oracle, io, n, count):
    def make():
        x = np.random.default_rng(n + count).uniform(-1, 1, (count, n)).astype(np.float32)
        X = np.stack([oracle.mdct(2, row.astype(np.float64)) for row in x])
        return x, X, np.stack([oracle.imdct(2, row.astype(np.float32)) for row in X])
    x, ref_X, ref_x = cached(("mdctb", n, count), make)
    m = filters.MdctBatch(n)
    X, xo = io.out(F32, count, n // 2), io.out(F32, count, n)
    m.forward(io.inp(x), X)
    m.inverse(io.inp(ref_X.astype(np.float32)), xo)
    io.verify(f"mdct_batch {n}")
    m.close()
    got_X, got_x = host(X), host(xo)
    assert float(np.sqrt(np.mean((got_X - ref_X) ** 2))) / float(np.sqrt(np.mean(ref_X ** 2))) <= TOL, (n, count)
    rms_check(got_x, ref_x, f"imdct batch n={n} x {count}")
    return {"X": got_X, "x": got_x}


def run_mdct_fixed(dev, oracle, io, t, n, count):
    def make():
        rng = np.random.default_rng(1000 * t + n + count)
        x = rng.integers(-(1 << 20), 1 << 20, (count, n), dtype=np.int32)
        x[0, : n // 2] = rng.integers(-(1 << 31), (1 << 31) - 1, n // 2, dtype=np.int64).astype(np.int32)   # wraps
        X = np.stack([oracle.mdct_fixed(t, row) for row in x])
        return x, X, np.stack([oracle.mdct_fixed(t, row, inverse=True) for row in X])
    x, ref_X, ref_y = cached(("mdctx", t, n, count), make)
    m = filters.MdctFixed(t, n)
    X, y = io.out(I32, count, n // 2), io.out(I32, count, n)
    m.forward_batch(io.inp(x), X)
    m.inverse_batch(io.inp(ref_X), y)
    io.verify(f"mdct_fixed_batch type {t} n {n}")
    m.close()
    got_X, got_y = host(X), host(y)
    equal_gate(got_X, ref_X, f"mdct_fixed_batch type {t} n {n} x {count}")
    equal_gate(got_y, ref_y, f"imdct_fixed_batch type {t} n {n} x {count}")
    return {"X": got_X, "y": got_y}


def run_pcm_deinterleave(dev, oracle, io, channels, n):
    il = cached(("pcm16", channels, n),
                lambda: np.random.default_rng(channels * 7 + n).integers(-32768, 32768, (n, channels)).astype(np.int16))
    pl = io.out(F32, channels, n)
    filters.pcm_deinterleave(io.inp(il), pl)
    io.verify("pcm_deinterleave")
    got = host(pl)
    equal_gate(got, oracle.pcm_deinterleave(il), f"pcm_deinterleave {channels}x{n}")
    return {"planar": got}


def run_pcm_interleave(dev, oracle, io, channels, n):
    x = cached(("pcm32", channels, n),
               lambda: np.random.default_rng(channels * 7 + n).uniform(-1.5, 1.5, (channels, n)).astype(np.float32))
    il = io.out(I16, n, channels)
    filters.pcm_interleave(io.inp(x), il)
    io.verify("pcm_interleave")
    got = host(il)
    equal_gate(got, oracle.pcm_interleave(x), f"pcm_interleave {channels}x{n}")
    return {"interleaved": got}


def run_synth(dev, oracle, io, dtype, channels, n):
    dst = io.out(dtype, channels, n)
    (filters.synth_f32 if dtype == F32 else filters.synth_i16)(dst, seed=7)
    io.verify("synth")
    got = host(dst)
    equal_gate(got, (oracle.synth_f32 if dtype == F32 else oracle.synth_i16)(channels, n, 7), f"synth {dtype} {channels}x{n}")
    return {"pcm": got}


# ================================================================================================ cases
T, TM = filters.FIR_ALGO_TIME, filters.FIR_ALGO_TIME_MFMA
O1, O2, O4, O8 = (filters.FIR_ALGO_OVERLAP_SAVE, filters.FIR_ALGO_OVERLAP_SAVE_2048, filters.FIR_ALGO_OVERLAP_SAVE_4096,
                  filters.FIR_ALGO_OVERLAP_SAVE_8192)
WAVE = {"iir_wave_min_items": 0}
RS = filters.PCM_F32, filters.PCM_I16, filters.PCM_I16_FAST
RS_F32 = {"fir_mfma_f32": ({}, 1, 3), "resample_dec_f32": ({"rs_dec_valu": 1}, 1, 3),
          "resample_mfma_f32-phase-tile": ({"rs_mfma_form": -1}, 147, 160), "resample_mfma_f32-period-tile": ({"rs_mfma_form": 1}, 147, 160),
          "resample_f32": ({}, 2, 3), "resample_f32-rs_generic1": ({"rs_generic": 1}, 147, 160),
          "resample_f32-rs_generic2": ({"rs_generic": 2}, 147, 160)}          # PATHS of tests/test_resample_probe_gpu.py
WINS = (po.BLACKMAN, po.HAMMING, po.KAISER)

# (id, adapter, case, offsets); "full" / "part": the shape that fills its last tile / leaves it partial
CASES = []


def add(name, fn, offsets, full, part):
    CASES.append((name + "-full", fn, full, offsets))
    CASES.append((name + "-part", fn, part, offsets))


# FIR: 2048-output tiles (time domain), jobs of two blocks less the overlap (overlap-save)
add("fir-time", run_fir, OFF32, dict(algo=T, T=63, channels=3, n=4096), dict(algo=T, T=63, channels=2, n=1000))
add("fir-time-mfma", run_fir, OFF32, dict(algo=TM, T=63, channels=3, n=4096), dict(algo=TM, T=63, channels=2, n=1000))
add("fir-ols1024", run_fir, OFF32, dict(algo=O1, T=257, channels=3, n=4096), dict(algo=O1, T=257, channels=3, n=1000))
add("fir-ols2048", run_fir, OFF32, dict(algo=O2, T=513, channels=3, n=6144), dict(algo=O2, T=513, channels=3, n=5000))
add("fir-ols4096", run_fir, OFF32, dict(algo=O4, T=2049, channels=2, n=8192), dict(algo=O4, T=2049, channels=2, n=2048 * 5 + 1))
add("fir-ols8192", run_fir, OFF32, dict(algo=O8, T=3073, channels=2, n=20480), dict(algo=O8, T=3073, channels=2, n=10240 * 3 + 5))
# IIR cascade: 1024-sample chunks (pipeline, 16 per lane), 2048 (32 per lane), 64-sample tiles of the remainder kernel
add("iirc-pipe", run_iir_cascade, OFF32, dict(coef="fixture", tune={"iir_pipe": 1}, channels=3, n=1024 * 5),
    dict(coef="fixture", tune={"iir_pipe": 1}, channels=2, n=1024 * 3 + 777))
for prec, radius in ((32, 0.5), (64, 0.99)):
    add(f"iirc-wave16-f{prec}", run_iir_cascade, OFF32, dict(coef=(4, radius), tune=WAVE, channels=3, n=1024, precision=prec),
        dict(coef=(4, radius), tune=WAVE, channels=3, n=1024 + 40, precision=prec))
    add(f"iirc-wave32-f{prec}", run_iir_cascade, OFF32, dict(coef=(4, radius), tune=WAVE, channels=3, n=4096, precision=prec),
        dict(coef=(4, radius), tune=WAVE, channels=3, n=4096 + 1024 + 40, precision=prec))
add("iirc-remainder", run_iir_cascade, OFF32, dict(coef="fixture", tune={}, channels=64, n=832),
    dict(coef="fixture", tune={}, channels=70, n=777))
add("iirc-segs-pipe", run_iir_cascade, OFF32, dict(coef=(4, 0.5), tune={"iir_segs": 2, "iir_pipe": 1}, channels=3, n=1024 * 16),
    dict(coef=(4, 0.5), tune={"iir_segs": 3, "iir_pipe": 1}, channels=3, n=1024 * 16 + 100))
add("iirc-segs-wave", run_iir_cascade, OFF32, dict(coef=(4, 0.5), tune={"iir_segs": 2, **WAVE}, channels=3, n=2048 * 8),
    dict(coef=(4, 0.5), tune={"iir_segs": 3, **WAVE}, channels=3, n=2048 * 8 + 1024 + 40))
# general direct form I: blocks of 16 samples per lane
add("iir-mc", run_iir_mc, OFF32, dict(a=[1.0, -0.3695, 0.1958, 0.0], b=[1.0, 0.2066, 0.4131, 0.2066], channels=5, n=1024),
    dict(a=[1.0, -1.2, 0.9, -0.35, 0.12, -0.02], b=[0.05, 0.1, 0.05], channels=5, n=1003))
# resampler, float32: every path of the probe test, whole and odd period counts, two calls
for name, (tune, L, M) in RS_F32.items():
    win = WINS[(L + M) % 3]
    add("rs-f32-" + name, run_resample, OFF32, dict(fmt=RS[0], tune=tune, L=L, M=M, win=win, channels=3, lens=[256 * M, 64 * M]),
        dict(fmt=RS[0], tune=tune, L=L, M=M, win=win, channels=3, lens=[203 * M, 49 * M]))
# resampler, int16 (whole reference frames in all: 1536 samples at 1:3 and 2:3, 147 periods of 160 at 147:160)
add("rs-i16-screened-1:M", run_resample, OFF16, dict(fmt=RS[1], tune={}, L=1, M=3, win=po.BLACKMAN, channels=5, lens=[1536, 3072]),
    dict(fmt=RS[1], tune={}, L=1, M=3, win=po.BLACKMAN, channels=5, lens=[3 * 201, 3 * 311]))
add("rs-i16-screened-L:M", run_resample, OFF16, dict(fmt=RS[1], tune={}, L=147, M=160, win=po.BLACKMAN, channels=5, lens=[160 * 64, 160 * 83]),
    dict(fmt=RS[1], tune={}, L=147, M=160, win=po.BLACKMAN, channels=5, lens=[160 * 37, 160 * 110]))
add("rs-i16-double", run_resample, OFF16, dict(fmt=RS[1], tune={"rs_i16_path": 1}, L=2, M=3, win=po.HAMMING, channels=5, lens=[1536, 3072]),
    dict(fmt=RS[1], tune={"rs_i16_path": 1}, L=2, M=3, win=po.HAMMING, channels=5, lens=[3 * 201, 3 * 311]))
add("rs-i16-fast", run_resample, OFF16, dict(fmt=RS[2], tune={"rs_i16_path": 1}, L=1, M=3, win=po.BLACKMAN, channels=7, lens=[1536 * 2, 1536], gate="lsb"),
    dict(fmt=RS[2], tune={"rs_i16_path": 1}, L=1, M=3, win=po.BLACKMAN, channels=7, lens=[3 * 201, 3 * 311], gate="lsb"))
# ratios with a common factor, the first call ending and the second starting inside a period of L outputs (the matrix-core
# entries store whole periods: the handle runs such calls on its fallback entry, tests/test_resample_ragged_gpu.py)
CASES.append(("rs-f32-resample_mfma_f32-294:320-ragged", run_resample, dict(fmt=RS[0], tune={}, L=294, M=320, win=po.BLACKMAN, channels=3,
                                                                           lens=[160 * 129, 160 * 131]), OFF32))
CASES.append(("rs-i16-screened-L:M-ragged", run_resample, dict(fmt=RS[1], tune={}, L=4, M=6, win=po.BLACKMAN, channels=5,
                                                              lens=[3 * 1001, 3 * 999]), OFF16))
# float32 transforms in place: 256 / E transforms per workgroup of the register kernels (E lanes each), 8 at 1024 points
for n, per in ((64, 32), (256, 16), (128, 32), (512, 16), (2048, 8), (1024, 8)):
    add(f"fft-batch-{n}", run_fft_batch, OFF_INPLACE, dict(n=n, count=per, tune={}), dict(n=n, count=per + 1, tune={}))
add("fft-batch-4096", run_fft_batch, OFF_INPLACE, dict(n=4096, count=4, tune={}), dict(n=4096, count=3, tune={}))
add("fft-batch-staged-256", run_fft_batch, OFF_INPLACE, dict(n=256, count=8, tune={"fft_generic": 1}), dict(n=256, count=9, tune={"fft_generic": 1}))
add("fft-batch-staged-16", run_fft_batch, OFF_INPLACE, dict(n=16, count=128, tune={}), dict(n=16, count=130, tune={}))
add("fft-batch-staged-8", run_fft_batch, OFF_INPLACE, dict(n=8, count=256, tune={}), dict(n=8, count=9, tune={}))
add("fft-batch-8192", run_fft_batch, OFF_INPLACE, dict(n=8192, count=1, tune={}), dict(n=8192, count=3, tune={}))
add("fft-fixed-256", run_fft_fixed, OFF_INPLACE, dict(n=256, count=16), dict(n=256, count=17))
add("fft-fixed-2048", run_fft_fixed, OFF_INPLACE, dict(n=2048, count=8), dict(n=2048, count=3))
add("fft-fixed-16", run_fft_fixed, OFF_INPLACE, dict(n=16, count=128), dict(n=16, count=130))
# correlation: a wave per frame, four per workgroup, 512-sample steps
for name, tune in (("reg", {}), ("lds", {"acf_lds": 1})):
    add("acf-" + name, run_autocorr, OFF32, dict(tune=tune, frames=8, n=512, p=16), dict(tune=tune, frames=7, n=300, p=16))
for fft_len, n, p, full, part in ((128, 64, 20, 32, 13), (512, 200, 33, 16, 13), (1024, 300, 31, 8, 13), (2048, 1000, 63, 8, 7),
                                  (4096, 1025, 16, 4, 5)):
    add(f"acf-fast-{fft_len}", run_autocorr_fast, OFF32, dict(frames=full, n=n, p=p), dict(frames=part, n=n, p=p))
for name, tune in (("fused", {}), ("split", {"lpc_split": 1})):
    add("lpc-" + name, run_lpc, OFF32, dict(tune=tune, p=16, n=37, frames=64), dict(tune=tune, p=10, n=300, frames=65))
# windowed-FFT frames: lane-group kernels (fft_len 512), 1024, the composed form at 8192
add("stft-512", run_stft, OFF32, dict(tune={}, hint=0, frame_len=128, win=po.HAMMING, channels=2, frames=16),
    dict(tune={}, hint=0, frame_len=128, win=po.HAMMING, channels=3, frames=7))
add("stft-1024", run_stft, OFF32, dict(tune={}, hint=1, frame_len=512, win=po.HAMMING, channels=2, frames=8),
    dict(tune={}, hint=1, frame_len=512, win=po.HAMMING, channels=3, frames=7))
add("stft-8192", run_stft, OFF32, dict(tune={}, hint=0, frame_len=2048, win=po.KAISER, channels=2, frames=2),
    dict(tune={}, hint=1, frame_len=4096, win=po.HAMMING, channels=1, frames=5))
add("mdct-frames", run_mdct_frames, OFF32, dict(F=128, win=0, channels=4, calls=(8, 8)), dict(F=256, win=1, channels=3, calls=(1, 6)))
add("mdct-batch-256", run_mdct_batch, OFF32, dict(n=256, count=32), dict(n=256, count=33))
add("mdct-batch-32", run_mdct_batch, OFF32, dict(n=32, count=8), dict(n=32, count=5))
add("mdct-fixed-fft1", run_mdct_fixed, OFF32, dict(t=1, n=256, count=8), dict(t=1, n=256, count=5))
add("mdct-fixed-fft4", run_mdct_fixed, OFF32, dict(t=2, n=512, count=8), dict(t=2, n=64, count=5))
add("pcm-deinterleave", run_pcm_deinterleave, OFF16, dict(channels=64, n=4096), dict(channels=6, n=1000))
add("pcm-interleave", run_pcm_interleave, [(i, o) for (o, i) in OFF16], dict(channels=64, n=4096), dict(channels=6, n=1000))
add("synth-f32", run_synth, OFF32, dict(dtype=F32, channels=3, n=4096), dict(dtype=F32, channels=6, n=1001))
add("synth-i16", run_synth, OFF16, dict(dtype=I16, channels=3, n=4096), dict(dtype=I16, channels=6, n=1001))

INT_INPUT = {run_resample: lambda case: case["fmt"] != filters.PCM_F32, run_fft_fixed: lambda case: True,
             run_mdct_fixed: lambda case: True, run_pcm_deinterleave: lambda case: True}
PARAMS = [pytest.param(fn, case, off, id=f"{name}-in{off[0]}-out{off[1]}") for (name, fn, case, offsets) in CASES for off in offsets]


@pytest.mark.parametrize("fn,case,off", PARAMS)
def test_guarded_buffers(dev, oracle, fn, case, off):
    if INT_INPUT.get(fn, lambda case: False)(case):
        # integer inputs have no NaN: bands of +max, then of -max-1; what lies outside the buffer must not reach the result
        hi = fn(dev, oracle, Io(dev, off, "max"), **case)
        lo = fn(dev, oracle, Io(dev, off, "min"), **case)
        for k in hi:
            assert np.array_equal(hi[k], lo[k]), f"{k}: the result depends on what lies outside the input buffer"
    else:
        fn(dev, oracle, Io(dev, off, "nan"), **case)


# ================================================================================================ aliasing
def dptr(t):
    return C.c_void_p(t.data_ptr())


def refused(pairs, call, name, others=()):
    """every (in, out) pair of overlap_cases is refused by `call`, with a message that names the entry point, and in, out and
    the `others` buffers are bit-unchanged afterwards (nothing was staged or launched)"""
    for k, (a, b) in enumerate(pairs):
        before = [bc.bits(t).copy() for t in (a, b) + tuple(others)]
        rc, msg = call(a, b), capi.last_error()
        assert rc == ERR_ARG and name in msg, (k, rc, msg)
        if k > 0:                                            # (an exact alias may meet an entry point's older in-place check first)
            assert "may not overlap" in msg and "(device memory)" in msg, (k, msg)
        torch.cuda.synchronize()
        for t, was in zip((a, b) + tuple(others), before):
            assert np.array_equal(bc.bits(t), was), f"{name}: case {k} changed a buffer it refused"


def test_overlap_refused_fir_iir(dev, oracle):
    L = capi.lib()
    taps = oracle.fir_design(po.LPF, 63, 0.2, 0.0, po.KAISER)
    f = filters.FirFilterMC(2, 1000, taps, algo=T)
    refused(bc.overlap_cases(2000, device=dev), lambda a, b: L.llz_fir_filter_mc(f.handle, dptr(a), dptr(b), 1000), "llz_fir_filter_mc")
    f.close()
    g = filters.IirMC(2, [1.0, -0.5], [0.5, 0.5])
    refused(bc.overlap_cases(2000, device=dev), lambda a, b: L.llz_iir_mc(g.handle, dptr(a), dptr(b), 1000), "llz_iir_mc")
    g.close()
    for tune in ({}, {"iir_segs": 2, "iir_pipe": 1}):
        with capi.tuned(**tune):
            h = filters.IirCascadeMC(2, low_q(4, 0.5))
            refused(bc.overlap_cases(2 * 16384, device=dev), lambda a, b: L.llz_iir_cascade_mc(h.handle, dptr(a), dptr(b), 16384),
                    "llz_iir_cascade_mc")
            h.close()


def test_overlap_refused_resample_pcm(dev):
    L = capi.lib()
    for fmt, dtype in ((filters.PCM_F32, F32), (filters.PCM_I16, I16)):
        for (l, m) in ((1, 3), (3, 2)):
            r = filters.ResampleMC(2, l, m, 1.0, po.BLACKMAN, fmt)
            n_in = 600
            refused(bc.overlap_cases(2 * n_in, 2 * n_in * l // m, device=dev, dtype=dtype),
                    lambda a, b: L.llz_resample_mc(r.handle, dptr(a), n_in, dptr(b)), "llz_resample_mc")
            r.close()
    ch, n = 6, 1000
    # int16 in, float32 out over one allocation counted in int16 elements (the ranges are what matters: plain pointers)
    refused(bc.overlap_cases(ch * n, 2 * ch * n, device=dev, dtype=I16),
            lambda a, b: L.llz_pcm_deinterleave_i16_f32(dptr(a), dptr(b), ch, n, 1.0 / 32768.0, None), "llz_pcm_deinterleave_i16_f32")
    refused(bc.overlap_cases(2 * ch * n, ch * n, device=dev, dtype=I16),
            lambda a, b: L.llz_pcm_interleave_f32_i16(dptr(a), dptr(b), ch, n, 32768.0, None), "llz_pcm_interleave_f32_i16")


def test_overlap_refused_transforms(dev):
    L = capi.lib()
    ch, frames = 2, 3
    s = filters.StftMC(ch, 0, 128, po.HAMMING)
    nx, nb = ch * frames * 128, ch * frames * s.bins
    spare = bc.carve(dev, F32, nb, 0, guard=64).view
    for which in ("re", "im"):
        refused(bc.overlap_cases(nx, nb, device=dev),
                lambda a, b: L.llz_stft_mc_analysis(s.handle, dptr(a), dptr(b if which == "re" else spare),
                                                    dptr(spare if which == "re" else b), frames), "llz_stft_mc_analysis", (spare,))
        refused(bc.overlap_cases(nb, nx, device=dev),
                lambda a, b: L.llz_stft_mc_synthesis(s.handle, dptr(a if which == "re" else spare),
                                                     dptr(spare if which == "re" else a), dptr(b), frames), "llz_stft_mc_synthesis", (spare,))
    s.close()
    m = filters.MdctBatch(256)
    refused(bc.overlap_cases(5 * 256, 5 * 128, device=dev), lambda a, b: L.llz_mdct_batch(m.handle, dptr(a), dptr(b), 5), "llz_mdct_batch")
    refused(bc.overlap_cases(5 * 128, 5 * 256, device=dev), lambda a, b: L.llz_imdct_batch(m.handle, dptr(a), dptr(b), 5), "llz_imdct_batch")
    m.close()
    fm = filters.MdctFramesMC(ch, 128, 0)
    refused(bc.overlap_cases(ch * 3 * 128, device=dev), lambda a, b: L.llz_mdct_frames_mc_analysis(fm.handle, dptr(a), dptr(b), 3),
            "llz_mdct_frames_mc_analysis")
    refused(bc.overlap_cases(ch * 3 * 128, device=dev), lambda a, b: L.llz_mdct_frames_mc_synthesis(fm.handle, dptr(a), dptr(b), 3),
            "llz_mdct_frames_mc_synthesis")
    fm.close()
    mx = filters.MdctFixed(1, 256)
    refused(bc.overlap_cases(5 * 256, 5 * 128, device=dev, dtype=I32), lambda a, b: L.llz_mdct_fixed_batch(mx.handle, dptr(a), dptr(b), 5),
            "llz_mdct_fixed_batch")
    refused(bc.overlap_cases(5 * 128, 5 * 256, device=dev, dtype=I32), lambda a, b: L.llz_imdct_fixed_batch(mx.handle, dptr(a), dptr(b), 5),
            "llz_imdct_fixed_batch")
    mx.close()


def test_overlap_refused_correlation_lpc(dev):
    L = capi.lib()
    frames, n, p = 7, 300, 16
    refused(bc.overlap_cases(frames * n, frames * (p + 1), device=dev),
            lambda a, b: L.llz_autocorr_mc(dptr(a), dptr(b), frames, n, p, None), "llz_autocorr_mc")
    f = filters.AutocorrFastMC(frames, n)
    refused(bc.overlap_cases(frames * n, frames * (p + 1), device=dev),
            lambda a, b: L.llz_autocorr_fast_mc(f.handle, dptr(a), dptr(b), p), "llz_autocorr_fast_mc")
    f.close()
    sizes = {"acof": frames * (p + 1), "kcof": frames * p, "err": frames, "gain": frames, "r": frames * (p + 1)}
    for tune in ({}, {"lpc_split": 1}):
        for name in sizes:                                   # x against each output in turn, the others in buffers of their own
            own = {k: bc.carve(dev, F32, v, 0, guard=64).view for k, v in sizes.items() if k != name}

            def call(a, b):
                o = dict(own, **{name: b})
                return L.llz_lpc_mc(dptr(a), None, dptr(o["acof"]), dptr(o["kcof"]), dptr(o["err"]), dptr(o["gain"]), dptr(o["r"]),
                                    frames, n, p, None)
            with capi.tuned(**tune):
                refused(bc.overlap_cases(frames * n, sizes[name], device=dev), call, "llz_lpc_mc", tuple(own.values()))


def test_iir_cascade_host_in_place_equals_out_of_place(dev, oracle):
    """host buffers are staged through the handle's own device memory, so x == y on the host is ordered: the same bits as the
    out-of-place host call, time segments forced so that warm-up chunks are read in front of every later segment"""
    x = oracle.synth_f32(2, 1024 * 16, seed=3)
    outs = []
    with capi.tuned(iir_segs=2, iir_pipe=1):
        for in_place in (False, True):
            f = filters.IirCascadeMC(2, low_q(4, 0.5))
            buf = x.copy()
            y = buf if in_place else np.full_like(x, np.nan)
            f.filter(buf, y)
            f.close()
            outs.append(y.copy())
            assert in_place or np.array_equal(buf, x)
    equal_gate(outs[1], outs[0], "llz_iir_cascade_mc, host x == y")
    rms_check(outs[0], oracle.iir_cascade_batch_f32(x, low_q(4, 0.5)), "llz_iir_cascade_mc, host buffers")


def test_in_place_transforms_are_untouched_by_the_overlap_rule(dev, oracle):
    """llz_fft_batch and llz_fft_fixed_batch work in place by contract: one buffer, never refused"""
    z = np.random.default_rng(1).uniform(-1, 1, (3, 2 * 256)).astype(np.float32)
    zd = torch.from_numpy(z.copy()).to(dev)
    f = filters.FftBatch(256)
    f.fft(zd, 3)
    f.close()
    got = zd.cpu().numpy().view(np.complex64)
    ref = np.stack([oracle.fft(row.view(np.complex64).astype(np.complex128)) for row in z])
    assert np.sqrt(np.mean(np.abs(got - ref) ** 2)) / np.sqrt(np.mean(np.abs(ref) ** 2)) < 1e-6
    q = np.random.default_rng(2).integers(-8000, 8001, (3, 2 * 256)).astype(np.int32)
    qd = torch.from_numpy(q).to(dev)
    fx = filters.FftFixed(256)
    fx.fft_batch(qd, 3)
    fx.close()
    equal_gate(qd.cpu().numpy(), np.stack([oracle.fft_fixed(row) for row in q]), "llz_fft_fixed_batch in place")
