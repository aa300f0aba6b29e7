"""Shared pieces of the polyphase filter bank's tests (test_pfb_gpu.py, test_pfb_host.py): the cases, a float64 reference that is
the definition of include/llz_pfb.h written directly in numpy, a float32 model of the algorithm (float32 fold with p ascending, a
complex64 radix-2 transform, the same overlap-add order), and the limits.  Plain numpy; nothing here opens a GPU.

THE LIMITS, u = 2^-24.  They are derived, not fitted to a device.

  analysis, per bin    |X - X_ref| <= 8 u (log2 M + P) sqrt(M) ||a_m||_2,   a_m[r] = sum_p |w[r + p M] x[s_m + r + p M]|
      The fold's P products and P - 1 sums err by at most P u a_m[r] per residue, at most P u ||a_m||_1 <= P u sqrt(M) ||a_m||_2
      in any bin.  A radix-2 transform's error norm is at most a small constant times log2 M u ||X||_2 = log2 M u sqrt(M) ||u_m||_2
      <= log2 M u sqrt(M) ||a_m||_2, and no bin errs by more than the norm.  The front factor is the project's 8
      (partition_limit, tests/stream_checks.py).
  synthesis, per sample  |y - y_ref| <= 8 u (log2 M + R) sum_m |g[t - s_m]| B_m,   B_m = sqrt(sum over all M Hermitian bins
      |X_m[k]|^2 / M) = ||u_m||_2 >= every |u_m[r]|
      The inverse transform errs by at most a small constant times log2 M u ||u_m||_2 per value, the product by u, and a sum
      of at most R terms by R u times the sum of their magnitudes.
  dense gate           rms(err) / rms(ref) <= 1e-5 per channel and direction, on the channels with random input

A case: one stream of calls of 1, R - 1, R, R + 1 and 300 frames (R - 1 = 0 for R = 1: a call that touches nothing).  Channel c
is dense (Gaussian) unless c % 3 == 1; those channels are sparse: analysis input with +-1 at every position of one hop and zeros
elsewhere (each frame that covers it folds ONE product per residue, and the R frames between them hit every (r, p)), synthesis
input with one frame whose spectrum is a single +-1 bin (its L windowed samples land on every tail position one term at a time).
The hop / frame chosen differs per channel and a second one follows more than R frames later, inside the long call."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from numpy.lib.stride_tricks import as_strided

U = 2.0 ** -24
FRAME, TIME = 0, 1
SHAPES = [(8, 1, 1), (16, 3, 4), (64, 4, 2), (256, 16, 8), (1024, 8, 4), (4096, 8, 1)]      # (M, P, M / D)
CHANNELS = (3, 37)
PHASES = (FRAME, TIME)
LONG = 300
GATE = 1e-5
FAULTS = ("fold_stride", "window_reversed", "rotation_sign", "frame_late", "tail_order")


def geometry(M, P, os):
    """(D, L, R)"""
    D = M // os
    return D, P * M, P * os


def call_frames(M, P, os):
    R = P * os
    return [1, R - 1, R, R + 1, LONG]


def windows(M, P):
    """(w, g): two different, asymmetric float32 prototypes -- a tilted windowed sinc each, so that a reversed or swapped
    window is a different filter"""
    L = P * M
    i = np.arange(L, dtype=np.float64)
    core = np.sinc((i - (L - 1) / 2.0) / M) * (0.5 - 0.5 * np.cos(2 * np.pi * (i + 0.5) / L))
    w = core * (1.0 + 0.5 * i / L)
    g = core * (1.3 - 0.4 * i / L) * (1.0 / P)
    return w.astype(np.float32), g.astype(np.float32)


def is_sparse(c):
    return c % 3 == 1


def sparse_frames(c, M, P, os):
    """the two hops (analysis) / frames (synthesis) of sparse channel c that are not zero"""
    R = P * os
    first = 1 + (c // 3) % (2 * R + 3)
    return first, first + 2 * R + 7


def case_x(channels, M, P, os, seed=1):
    """[channels, frames D] float32 for the whole stream of call_frames"""
    D, L, R = geometry(M, P, os)
    frames = sum(call_frames(M, P, os))
    rng = np.random.default_rng(seed * 7919 + M * 31 + P * 7 + os)
    x = rng.standard_normal((channels, frames * D), dtype=np.float32)
    for c in range(channels):
        if is_sparse(c):
            x[c] = 0
            for b in sparse_frames(c, M, P, os):
                x[c, b * D:(b + 1) * D] = rng.choice([-1.0, 1.0], D)
        else:
            x[c] *= np.float32(2.0 ** ((c % 5) - 2))
    return x


def case_spectra(channels, M, P, os, seed=2):
    """(re, im) [channels, frames, M/2 + 1] float32; the imaginary parts of bins 0 and M/2 are zero"""
    frames = sum(call_frames(M, P, os))
    bins = M // 2 + 1
    rng = np.random.default_rng(seed * 104729 + M * 31 + P * 7 + os)
    re = rng.standard_normal((channels, frames, bins), dtype=np.float32)
    im = rng.standard_normal((channels, frames, bins), dtype=np.float32)
    for c in range(channels):
        if is_sparse(c):
            re[c] = 0
            im[c] = 0
            for n, b in enumerate(sparse_frames(c, M, P, os)):
                k = (3 * c + 5 * n + 1) % bins
                if 0 < k < M // 2 and n == 1:
                    im[c, b, k] = -1.0
                else:
                    re[c, b, k] = 1.0 if c % 2 else -1.0
    im[:, :, 0] = 0
    im[:, :, -1] = 0
    return re, im


def rotations(frames, M, D, phase, sign=1):
    """(m + 1) D mod M per frame in TIME phase, zeros in FRAME phase"""
    m = np.arange(frames, dtype=np.int64)
    return (sign * (m + 1) * D) % M if phase == TIME else np.zeros(frames, dtype=np.int64)


# ---------------------------------------------------------------------------------------------- the complex64 radix-2 transform
@functools.lru_cache(maxsize=None)
def _bitrev(M):
    n = M.bit_length() - 1
    idx = np.arange(M)
    rev = np.zeros(M, dtype=np.int64)
    for b in range(n):
        rev |= ((idx >> b) & 1) << (n - 1 - b)
    return rev


def fft32(z, inverse=False):
    """unscaled radix-2 decimation-in-time transform over the last axis in complex64 arithmetic"""
    M = z.shape[-1]
    lead = z.shape[:-1]
    a = np.ascontiguousarray(z[..., _bitrev(M)], dtype=np.complex64)
    b = np.empty_like(a)
    h = 1
    while h < M:
        tw = np.exp((2j if inverse else -2j) * np.pi * np.arange(h) / (2 * h)).astype(np.complex64)
        a3, b3 = a.reshape(lead + (M // (2 * h), 2, h)), b.reshape(lead + (M // (2 * h), 2, h))
        o = a3[..., 1, :] * tw
        np.add(a3[..., 0, :], o, out=b3[..., 0, :])
        np.subtract(a3[..., 0, :], o, out=b3[..., 1, :])
        a, b = b, a
        h *= 2
    return a


def _each(one, channels):
    """one(c) for every channel; the channels are independent and numpy releases the lock, so a few threads share them"""
    if channels <= 4:
        for c in range(channels):
            one(c)
    else:
        with ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(one, range(channels)))


# ---------------------------------------------------------------------------------------------- analysis
def _fold(x, w, M, D, P, dtype, fault=None):
    """one channel: (u [frames, M] in dtype summed with p ascending, a [frames, M] float64)"""
    L = P * M
    frames = x.shape[0] // D
    lead = L - D + (D if fault == "frame_late" else 0)
    xp = np.concatenate([np.zeros(lead, dtype), x.astype(dtype)])
    if fault == "window_reversed":
        w = w[::-1]
    stride = M - 1 if fault == "fold_stride" else M
    u = a = None
    for p in range(P):
        seg = as_strided(xp[p * stride:], shape=(frames, M), strides=(D * xp.strides[0], xp.strides[0]))
        term = w[p * stride:p * stride + M].astype(dtype) * seg
        u = term if u is None else u + term
        if dtype == np.float64:                                       # |w x| = |w| |x|
            a = np.abs(term) if a is None else a + np.abs(term)
    return u, a


def analysis(x, w, M, P, os, phase, prec=64, fault=None):
    """x [channels, frames D] float32 -> (X complex [channels, frames, M/2 + 1], limit [channels, frames]).  prec 64: the
    definition in float64; prec 32: the float32 model (its limit is not computed: zeros)."""
    D, L, R = geometry(M, P, os)
    channels, frames = x.shape[0], x.shape[1] // D
    dtype = np.float64 if prec == 64 else np.float32
    rot = rotations(frames, M, D, phase, -1 if fault == "rotation_sign" else 1)
    src = (np.arange(M)[None, :] - rot[:, None]) % M                  # placed[(r + rot) % M] = u[r]
    X = np.zeros((channels, frames, M // 2 + 1), dtype=np.complex128 if prec == 64 else np.complex64)
    lim = np.zeros((channels, frames))
    front = 8 * U * (np.log2(M) + P) * np.sqrt(M)
    def one(c):
        u, a = _fold(x[c], w, M, D, P, dtype, fault)
        placed = np.take_along_axis(u, src, axis=1) if rot.any() else u
        if prec == 64:
            X[c] = np.fft.rfft(placed, axis=1)
            lim[c] = front * np.sqrt(np.sum(a * a, axis=1))
        else:
            X[c] = fft32(placed.astype(np.complex64))[:, :M // 2 + 1]
    _each(one, channels)
    return X, lim


# ---------------------------------------------------------------------------------------------- synthesis
def synthesis(re, im, g, M, P, os, phase, prec=64, fault=None, edges=()):
    """re, im [channels, frames, M/2 + 1] float32 -> (y [channels, frames D], limit [channels, frames D]).  prec 32: the float32
    model, overlap-added oldest frame first.  edges (fault tail_order only): the call edges of the stream, in frames."""
    D, L, R = geometry(M, P, os)
    channels, frames = re.shape[0], re.shape[1]
    dtype = np.float64 if prec == 64 else np.float32
    rot = rotations(frames, M, D, phase, -1 if fault == "rotation_sign" else 1)
    src = (np.arange(M)[None, :] + rot[:, None]) % M                  # u[r] = z[(r + rot) % M]
    gd = g.astype(dtype)
    y = np.zeros((channels, frames * D), dtype=dtype)
    lim = np.zeros((channels, frames * D))
    front = 8 * U * (np.log2(M) + R)
    order = range(R) if fault == "tail_order" else range(R - 1, -1, -1)     # segment j of frame m lands on block m + j
    def one(c):
        Xc = re[c].astype(np.complex128) + 1j * im[c].astype(np.complex128)
        if prec == 64:
            z = np.fft.irfft(Xc, n=M, axis=1)
            power = np.abs(Xc[:, 0].real) ** 2 + np.abs(Xc[:, -1].real) ** 2 + 2 * np.sum(np.abs(Xc[:, 1:-1]) ** 2, axis=1)
            B = np.sqrt(power / M)
            limb = np.zeros((frames + R - 1, D))
            for j in range(R):
                limb[j:j + frames] += np.abs(g[j * D:(j + 1) * D].astype(np.float64))[None, :] * B[:, None]
            lim[c] = front * limb[:frames].reshape(-1)
        else:
            full = np.zeros((frames, M), dtype=np.complex64)
            half = (Xc * (1.0 / M)).astype(np.complex64)
            full[:, :M // 2 + 1] = half
            full[:, M // 2 + 1:] = np.conj(half[:, 1:M // 2][:, ::-1])
            z = fft32(full, inverse=True).real.astype(np.float32)
        u = np.take_along_axis(z, src, axis=1) if rot.any() else z
        blocks = np.zeros((frames + R - 1, D), dtype=dtype)
        for j in order:
            seg = gd[j * D:(j + 1) * D][None, :] * u[:, (j * D) % M:(j * D) % M + D]     # i mod M: D divides M
            if fault == "tail_order" and j == 1:
                for e in edges:                                       # frame e - 1's block on the far side of a call edge
                    if 0 < e < frames:
                        seg[e - 1] = 0
            blocks[j:j + frames] += seg
        y[c] = blocks[:frames].reshape(-1)
    _each(one, channels)
    return y, lim


# ---------------------------------------------------------------------------------------------- ratios
def ratio(err, lim):
    """the largest err / lim; inf where something is off at a limit of zero (an exact zero is asked for there)"""
    err, lim = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(lim, dtype=np.float64))
    if np.any(np.isnan(err)):
        return float("inf")
    if np.any((lim == 0) & (err > 0)):
        return float("inf")
    ok = lim > 0
    return float(np.max(err[ok] / lim[ok])) if ok.any() else 0.0


def gate(got, ref, channels):
    """the largest rms(err) / rms(ref) over the dense channels"""
    worst = 0.0
    for c in range(channels):
        if not is_sparse(c):
            e = np.asarray(got[c], dtype=ref.dtype) - ref[c]
            worst = max(worst, float(np.sqrt(np.mean(np.abs(e) ** 2) / np.mean(np.abs(ref[c]) ** 2))))
    return worst


def _phase_key(os, phase):
    """at M / D = 1 the TIME phase's rotation is zero for every frame: one reference serves both phases"""
    return FRAME if os == 1 else phase


def reference_analysis(channels, M, P, os, phase):
    return _reference_analysis(channels, M, P, os, _phase_key(os, phase))


def reference_synthesis(channels, M, P, os, phase):
    return _reference_synthesis(channels, M, P, os, _phase_key(os, phase))


@functools.lru_cache(maxsize=4)
def _reference_analysis(channels, M, P, os, phase):
    w, _ = windows(M, P)
    x = case_x(channels, M, P, os)
    X, lim = analysis(x, w, M, P, os, phase)
    for a in (x, X, lim):
        a.setflags(write=False)
    return x, X, lim


@functools.lru_cache(maxsize=4)
def _reference_synthesis(channels, M, P, os, phase):
    _, g = windows(M, P)
    re, im = case_spectra(channels, M, P, os)
    y, lim = synthesis(re, im, g, M, P, os, phase)
    for a in (re, im, y, lim):
        a.setflags(write=False)
    return re, im, y, lim


def check_analysis(run, channels, M, P, os, phase, what):
    """run(x, w, calls) -> complex [channels, frames, bins]; returns (worst ratio to the per-bin limit, dense gate)"""
    x, X, lim = reference_analysis(channels, M, P, os, phase)
    got = run(x, windows(M, P)[0], call_frames(M, P, os))
    assert got.shape == X.shape, (got.shape, X.shape)
    worst = ratio(np.abs(got.astype(np.complex128) - X), lim[..., None])
    dense = gate(got.astype(np.complex128), X, channels)
    print(f"{what} analysis M={M} P={P} M/D={os} phase={phase} channels={channels}: worst |err| / limit {worst:.3g}, "
          f"dense rms ratio {dense:.3g}")
    return worst, dense


def check_synthesis(run, channels, M, P, os, phase, what):
    """run(re, im, g, calls) -> [channels, frames D]; returns (worst ratio to the per-sample limit, dense gate)"""
    re, im, y, lim = reference_synthesis(channels, M, P, os, phase)
    got = run(re, im, windows(M, P)[1], call_frames(M, P, os))
    assert got.shape == y.shape, (got.shape, y.shape)
    worst = ratio(np.abs(got.astype(np.float64) - y), lim)
    dense = gate(got.astype(np.float64), y, channels)
    print(f"{what} synthesis M={M} P={P} M/D={os} phase={phase} channels={channels}: worst |err| / limit {worst:.3g}, "
          f"dense rms ratio {dense:.3g}")
    return worst, dense


def model_analysis_run(M, P, os, phase, fault=None):
    return lambda x, w, calls: analysis(x, w, M, P, os, phase, prec=32, fault=fault)[0]


def model_synthesis_run(M, P, os, phase, fault=None):
    def run(re, im, g, calls):
        return synthesis(re, im, g, M, P, os, phase, prec=32, fault=fault, edges=tuple(np.cumsum(calls)))[0]
    return run
