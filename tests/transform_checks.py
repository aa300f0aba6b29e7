"""Shared pieces of the transform signal tests (test_transform_checks_host.py, test_transform_signals_gpu.py): the signal rows
that single out one bin, one sample or one row of a batch, the limits every element of a float32 transform is held to, plain
float32 models of the transforms to show that the limits ask nothing float32 cannot give, and faults to plant in the models.
Plain numpy (the double oracle is passed in where a transform has to be run); nothing here touches a GPU.

Why: the float32 FFT, STFT and MDCT kernels have a twiddle table layout, a lane-group transpose and a bin-to-lane map per
size, and were held to the double oracle by one RMS pooled over the whole output of uniform noise of one scale.  That cannot
see one bin slightly wrong, a twiddle from the neighbouring table index (2 pi / N on the touched bins), leakage into a bin
that must be empty, a quiet row beside loud ones, or a row that is never compared.

Signals, no two rows of a batch alike (fft_specs / real rows for the MDCT; frame_channels for the STFT and the MDCT frames):
impulses of amplitude 1 - 0.5j (1 where the input is real) at 0, 1, N/2-1, N/2, N-1 and at (row * 251 + N // 3) % N; tones
exp(+2 pi j b n / N) rounded to float32 at b = 0, 1, N/2, N-1, the lane-group edges E-1, E, N/E, N/E+1 and a bin that moves
with the row; a zero row; one noise row (magnitudes in [1/4, 1): no sample so small that a scaled product could leave the
normal range) with copies times 2^e, e in -20 .. +10, the copy at 2^-20 next to the one at 2^+10; and, as the last two rows
(the partial workgroup's), an impulse row times 2^-19 and 2^-20.  At the tiny sizes N positions and N bins cannot tell
2 (2048 / N) + 1 rows apart: the fill there is further noise rows.  The reference of an impulse is analytic
(a exp(-+2 pi j ((k m) mod N) / N), the phase reduced as integers), of a scaled copy the base row's times 2^e, of every other
row the oracle's double transform of the float32 input (a float32-rounded tone has true content of order u sqrt(N) in
every bin: the reference is not an ideal delta).

Limits, per element, derived and not measured (u = 2^-24; l1 = the sum of the magnitudes of the transform's input):
  * forward FFT, every bin of every row: |got[k] - ref[k]| <= 6 log2(N) u ||x||_1.  A radix-2 stage a +- w b with a
    correctly rounded table twiddle adds at most (1 + sqrt(5) + 1) u = 4.24 u times the stage's partial l1 sum (twiddle
    rounding 1, complex product without fma sqrt(5), the add 1); the partial sums of every stage are bounded by ||x||_1.  An
    inter-pass twiddle (square_core, the 2x step, the outer passes, the factored passes' W^(r k)) adds 3.24 u, the store or
    the inverse's 1/N 1 u: 4.24 log2 N + 4.24 <= 6 log2 N for N >= 8, the smallest float32 batch size (N = 2 and 4, which
    the MDCT's inner transform never reaches either, would run radix-2 with no inter-pass twiddle: 4.24 log2 N + 1 <
    6 log2 N).  Every table in these kernels is a direct pick from the host-built float table
    (k_fft_tables, load_tw1024, k_fft_large_twb): no product-of-twiddles term.  fma contraction only lowers the error.
  * inverse FFT: the same with ||X||_1 / N.
  * STFT analysis, every bin of every frame: (6 log2 N + 2) u sum_j |w_j x_j| over the frame's N windowed samples; the 2 u
    per sample are the float window table and the window product.  The analysis kernels transform the real frame as a
    complex one with a zero imaginary part: no packing step, no extra stage.
  * STFT synthesis, every output sample: a frame's inverse transform is within 6 (log2 N + h) u A_f of the double one, A_f =
    ||X_f||_1 / N over all N bins of the Hermitian extension, which also bounds every sample of that inverse; h = 1 where
    the kernel takes one half-size transform per real frame (k_stft_synthesis_reg_f32<.., HALF>, fft_len 512 and 2048: the
    split into even- and odd-sample spectra is one more twiddled butterfly per bin), else 0.  Sample i of block t is
    magic sum_{r < R} w[r F + i] y_{t-r}[r F + i]: per term the inverse's error, 2 u for the window table and product, R u
    for the overlap-add sums and 2 u for the float magic and its product:
    limit = (6 (log2 N + h) + R + 4) u magic sum_r |w[r F + i]| A_{t-r}.
  * MDCT and IMDCT (the N/4-point-FFT algorithm), every coefficient or sample: S = log2(N / 4) + 2 stages (the transform's,
    and the pre- and the post-rotation counted as a stage each), times the largest entry of the transform's matrix as the
    oracle scales it (1 forward, 4 / N inverse), times ||x||_1; the fold's one add per input adds 1 u: (6 S + 1) u ||x||_1
    forward.  The inverse's scale is two float factors, g = 8 f(1/sqrt N) applied to the post-rotated value and f(1/sqrt N)
    applied at the store (k_mdct_reg_f32, unrot2 / unrot4): the rounding of f(1/sqrt N) twice and the two products are 4 u
    the forward does not have, no fold: (6 S + 4) u (4 / N) ||X||_1.
  * MDCT frames: analysis (6 S + 1 + 2) u sum_i |w_i xbuf_i| (window table and product); synthesis, sample i of frame f,
    (6 S + 4 + 2 + 1) u (|w_i| A_f + |w_{F+i}| A_{f-1}), A_f = (4 / N) ||X_f||_1 (window table and product, and the one add
    of the two-term overlap-add).
Condition on every limit: the plain float32 models below (textbook radix-2 with float-rounded double twiddles, separate
float32 multiplies and adds, the STFT and MDCT built on it in the obvious way) stay at or below a QUARTER of the limit on
every signal row used; tests/test_transform_checks_host.py asserts it for every (transform, N, row kind) the GPU test uses.
A pair that does not meet the quarter would be listed in F32_DROPPED with the reason; none is.

Exact checks beside the limits: scaled_equal (a row that is 2^e times a base row gives the base row's output times 2^e bit
for bit: float32 arithmetic commutes with a power of two above the subnormal range, which the exponents keep clear of; this
pins row independence and addressing on every row without a reference), zero_where_silent (a silent row, channel or frame
gives exact zeros), zero_where_ref_zero (imaginary parts that are exactly zero in the oracle -- bins 0 and N/2 of a real
frame, every bin of a frame whose only sample sits at the window centre -- are exactly zero).
"""
import numpy as np

U = 2.0 ** -24
TOL = 1e-5                  # RMS, the pooled gate of the STFT and MDCT tests (tests/test_gpu_parity.py)
FFT_TOL = 1e-6              # relative RMS, the pooled gate of the FFT batch tests
TINY = 2.0 ** -126          # the smallest normal float32
SENTINEL = 7.0              # outputs are pre-filled with it: an unwritten element is a wrong element
HAMMING, BLACKMAN, KAISER = 0, 1, 2
IMP = 1.0 - 0.5j
CHANNEL_EXPS = (0, -20, 10, -3, 0)     # the five channels of the STFT and MDCT-frame batches
COPY_EXPS = (-20, 10, -7, 3)           # the noise row's scaled copies, in batch order: 2^-20 next to 2^+10
# (transform, row kind) pairs on which plain float32 does not stay within a quarter of the limit: none
F32_DROPPED = set()

# lane-group width E of the register kernel that serves a size (fft.hip: llzs_fft_f32, mdct_reg_launch)
FFT_E = {64: 8, 256: 16, 4096: 64, 128: 8, 512: 16, 2048: 32}
MDCT_E = {256: 8, 512: 8, 1024: 16, 2048: 16, 4096: 32, 8192: 32}


# the cases of tests/test_transform_signals_gpu.py; the host test runs the plain float32 models over the same ones
# (llz_fft_batch_init takes 8 points and up: 2 and 4 exist only in the double and Q15 forms, which are compared bit for bit)
FFT_CASES = [(n, False) for n in (8, 16, 32, 64, 256, 4096, 128, 512, 2048, 1024, 8192, 16384,
                                  1 << 15, 1 << 16, 1 << 17, 1 << 18, 1 << 19)] + \
            [(n, True) for n in (64, 128, 256, 512, 1024, 2048, 4096)]             # under fft_generic
# (fft_len, tune): staged; reg, HALF synthesis and full; 1024; one launch and composed at 4096; composed without / with an outer pass
STFT_CASES = [(64, None), (256, None), (512, None), (512, "stft_full"), (2048, None), (2048, "stft_full"), (1024, None),
              (4096, None), (4096, "fft_generic"), (8192, None), (32768, None)]
MDCT_SIZES = (64, 256, 512, 1024, 2048, 4096, 8192)
# (frame_len, window, mdct_run or None)
MDCT_FRAME_CASES = [(F, win, None) for F in (128, 256, 1024, 4096) for win in (0, 1)] + [(128, 0, 3), (512, 0, 3), (512, 1, None)]


def frames_total(N):
    """frames per channel over both calls: about 40 at the small sizes (the synthesis splits a channel into several runs)"""
    return max(5, min(41, 65536 // N + 1))


def frame_calls(which, T):
    """two calls of unequal frame counts, one of them a single frame"""
    return (T - 1, 1) if which == "a" else (1, T - 1)


def stft_window(fft_len, hint):
    return (HAMMING, KAISER, BLACKMAN)[(log2i(fft_len) + hint) % 3]


def stft_half(fft_len, tune):
    """does the synthesis take one half-size transform per frame (k_stft_synthesis_reg_f32<.., HALF>)?"""
    return fft_len in (512, 2048) and tune is None


def log2i(n):
    k = int(n).bit_length() - 1
    assert 1 << k == n, n
    return k


# ------------------------------------------------------------------------------------------------ batch geometry
def fft_group(n, generic=False):
    """(E, transforms per workgroup) of the kernel that serves an n-point FftBatch; E is None off the lane-group kernels"""
    if n > 4096:
        return None, 1
    if not generic and n in FFT_E:
        return FFT_E[n], 256 // FFT_E[n]
    if not generic and n == 1024:
        return 32, 8                                   # one half-wave per transform
    return None, max(1, 2048 // n)                     # k_fft_radix2: 2048 points per workgroup


def fft_count(n, generic=False):
    """rows per call: two full workgroups and a partial one up to 4096 points, 3 rows above"""
    return 3 if n > 4096 else 2 * fft_group(n, generic)[1] + 1


def fft_family(n, generic=False):
    if n > 16384:
        return f"k_fft_outer<G={min(4, log2i(n) - 14)}> + k_fft_block" + (" + k_fft_bitrev" if n >= 1 << 19 else "")
    if n > 4096:
        return f"k_fft_block FULL ({512 if n == 8192 else 1024} threads)"
    if generic or n < 64:
        return "k_fft_radix2<f32>"
    return "k_fft1024_f32" if n == 1024 else f"k_fft_{'square' if n in (64, 256, 4096) else '2xsquare'}_f32<{FFT_E[n]}>"


def stft_family(fft_len, tune=None):
    if fft_len > 4096 or tune == "fft_generic":
        return "composed STFT on " + fft_family(fft_len, tune == "fft_generic")
    if fft_len in (256, 512, 2048):
        half = ", HALF synthesis" if stft_half(fft_len, tune) else ", full-size synthesis" if fft_len != 256 else ""
        return f"k_stft_*_reg_f32{half}"
    return "k_stft_*1024_f32" if fft_len == 1024 else "k_stft_*_f32 (staged)"


def mdct_family(n):
    return f"k_mdct_reg_f32<{MDCT_E[n]}{', TWO' if n in (512, 2048, 8192) else ''}>" if n in MDCT_E else "k_mdct4_f32"


def mdct_count(n):
    return 2 * (256 // MDCT_E[n]) + 1 if n in MDCT_E else 2 * (2048 // n) + 1


# ------------------------------------------------------------------------------------------------ signal rows
def _unique(seq, n):
    out = []
    for v in seq:
        if 0 <= v < n and v not in out:
            out.append(v)
    return out


def fft_specs(n, count, E=None, lean=False):
    """The rows of an n-point batch as specs, a multiple of `count` of them (one call each `count` rows):
    ("imp", position) | ("tone", bin) | ("zero",) | ("noise", seed) | ("scaled", index of the base row, e).
    lean: one row per kind and position class (the host's quarter condition at the sizes where every row costs seconds)."""
    pos = _unique([0, 1, n // 2 - 1, n // 2, n - 1], n)
    bins = _unique([0, 1, n // 2, n - 1] + ([E - 1, E, n // E, n // E + 1] if E else []), n)
    if lean:
        pos, bins = _unique([n // 2 - 1, n - 1], n), _unique([n - 1, 1], n)
    core = [("imp", p) for p in pos] + [("tone", b) for b in bins] + [("zero",), ("noise", 1)]
    nb = len(core) - 1
    core += [("scaled", nb, e) for e in COPY_EXPS]
    imp_base = len(pos) - 1                                            # the impulse at n - 1
    tail = [("scaled", imp_base, -19), ("scaled", imp_base, -20)]
    total = -(-(len(core) + 2) // count) * count
    seen = set(core) | {("scaled", nb, 0)}
    while len(core) + 2 < total:                                       # the fill: rows that move with the row index
        r = len(core)
        m = (r * 251 + n // 3) % n
        cands = [("imp", m), ("tone", m), ("scaled", nb, -20 + (r * 7) % 31)]
        cand = cands[r % 3]
        if cand in seen:
            cand = next((c for c in cands if c not in seen), ("noise", r))
        seen.add(cand)
        core.append(cand)
    return core + tail


def noise_row(n, seed, real=False):
    """magnitudes uniform in [1/4, 1), random signs"""
    rng = np.random.default_rng(1000 * seed + n % 997)

    def part():
        return rng.uniform(0.25, 1.0, n) * rng.choice([-1.0, 1.0], n)
    return part().astype(np.float32) if real else (part() + 1j * part()).astype(np.complex64)


def tone_row(n, b, real=False):
    ang = 2 * np.pi * ((b * np.arange(n, dtype=np.int64)) % n) / n
    return np.cos(ang).astype(np.float32) if real else (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64)


def make_rows(n, specs, real=False):
    """[len(specs), n] complex64 (float32 if real)"""
    x = np.zeros((len(specs), n), dtype=np.float32 if real else np.complex64)
    for r, s in enumerate(specs):
        if s[0] == "imp":
            x[r, s[1]] = 1.0 if real else IMP
        elif s[0] == "tone":
            x[r] = tone_row(n, s[1], real)
        elif s[0] == "noise":
            x[r] = noise_row(n, s[1], real)
        elif s[0] == "scaled":
            assert specs[s[1]][0] != "scaled" and s[1] < r
            x[r] = np.ldexp(x[s[1]].view(np.float32), s[2]).view(x.dtype)
    return x


def scaled_pairs(specs):
    """(base_of, exps) for scaled_equal: row r is row base_of[r] times 2^exps[r]"""
    base_of = np.arange(len(specs))
    exps = np.zeros(len(specs), dtype=np.int64)
    for r, s in enumerate(specs):
        if s[0] == "scaled":
            base_of[r], exps[r] = s[1], s[2]
    return base_of, exps


def fft_reference(fft, n, specs, x, inverse=False):
    """[rows, n] complex128.  fft(z, inverse) is the oracle's double transform (forward unscaled, inverse / N)."""
    ref = np.zeros((len(specs), n), dtype=np.complex128)
    k = np.arange(n, dtype=np.int64)
    for r, s in enumerate(specs):
        if s[0] == "imp":
            ph = 2 * np.pi * ((k * s[1]) % n) / n
            ref[r] = IMP * (np.cos(ph) + 1j * np.sin(ph)) / n if inverse else IMP * (np.cos(ph) - 1j * np.sin(ph))
        elif s[0] == "scaled":
            ref[r] = np.ldexp(ref[s[1]].view(np.float64), s[2]).view(np.complex128)
        elif s[0] != "zero":
            ref[r] = fft(x[r].astype(np.complex128), inverse)
    return ref


def fft_limit(x, n, inverse=False):
    """[rows, 1]: 6 log2(n) u ||x||_1, over n for the inverse"""
    return 6 * log2i(n) * U * np.abs(x).astype(np.float64).sum(axis=-1, keepdims=True) / (n if inverse else 1)


def worst_by_kind(specs, got, ref, limit):
    """{row kind: worst fraction of the limit over the rows of that kind} (nothing asserted)"""
    out = {}
    for r, s in enumerate(specs):
        out[s[0]] = max(out.get(s[0], 0.0), limit_check(got[r], ref[r], np.broadcast_to(limit, ref.shape)[r], "", check=False))
    return out


def real_reference(run, specs, x, out_len):
    """[rows, out_len] float64 of a real transform: run(row as float64) per distinct base, copies times 2^e"""
    ref = np.zeros((len(specs), out_len))
    for r, s in enumerate(specs):
        if s[0] == "scaled":
            ref[r] = np.ldexp(ref[s[1]], s[2])
        elif s[0] != "zero":
            ref[r] = run(x[r].astype(np.float64))
    return ref


# ------------------------------------------------------------------------------------------------ frames: STFT, MDCT frames
def frame_channels(which, F, N, calls):
    """x [5, T F] float32 for two calls of calls[0] and calls[1] frames, channel c at 2^CHANNEL_EXPS[c]; returns
    (x, base_of, exps, names, info).  which "a": one-frame, noise 2^-20, noise 2^+10, DC 2^-3, impulses; the silent-but-one-frame
    channel holds noise in a middle frame.  which "b": impulses, one-frame 2^-20, one-frame 2^+10, tone 2^-3, noise; the one frame
    is the LAST of the first call, so the history and the overlap-add tail the handle carries hold it.
    Impulses: the first and the last sample of each call (the first of a call is also the first of a frame, which sits at
    the window centre N/2 of a later frame) and the first and the last sample of two frames inside the longer call."""
    T = sum(calls)
    n = T * F
    c1 = calls[0]
    fo = T // 2 if which == "a" else c1 - 1
    one = np.zeros(n, dtype=np.float32)
    one[fo * F:(fo + 1) * F] = noise_row(F, 3, real=True)
    noise = noise_row(n, 4, real=True)
    lo, hi = (0, c1) if c1 > 1 else (c1, T)                            # the longer call's frames
    fa, fb = lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3
    pos = sorted({0, c1 * F - 1, c1 * F, n - 1, fa * F, (fb + 1) * F - 1})
    imp = np.zeros(n, dtype=np.float32)
    imp[pos] = 1.0
    dc = np.full(n, 0.7, dtype=np.float32)
    b = N // 8 + 1                                                     # the tone: a bin off every lane-group edge
    tone = np.cos(2 * np.pi * ((b * np.arange(n, dtype=np.int64)) % N) / N).astype(np.float32)
    if which == "a":
        bases, names = [one, noise, noise, dc, imp], ["oneframe", "noise", "noise", "dc", "impulses"]
        base_of = np.array([0, 1, 1, 3, 4])
    else:
        bases, names = [imp, one, one, tone, noise], ["impulses", "oneframe", "oneframe", "tone", "noise"]
        base_of = np.array([0, 1, 1, 3, 4])
    x = np.stack([np.ldexp(v, e) for v, e in zip(bases, CHANNEL_EXPS)]).astype(np.float32)
    exps = np.array(CHANNEL_EXPS) - np.array(CHANNEL_EXPS)[base_of]    # relative to the base channel
    return x, base_of, exps, names, {"oneframe": fo, "impulses": pos, "quiet": 1}


def frame_windows(x, F, N):
    """[channels, T, N]: frame f's buffer = samples [(f+1)F - N, (f+1)F) of the stream, zeros in front of it"""
    xp = np.concatenate([np.zeros((x.shape[0], N - F), dtype=x.dtype), x], axis=1)
    return np.lib.stride_tricks.sliding_window_view(xp, N, axis=1)[:, ::F]


def stft_len(hint, F):
    return F << (2 if hint == 0 else 1)


def stft_magic(hint):
    return 0.812 if hint == 0 else 1.0


def stft_analysis_ref(oracle, x, base_of, hint, F, win):
    """complex128 [channels, T, bins]"""
    def run(row):
        re, im = oracle.stft_analysis(hint, F, win, row)
        return re + 1j * im
    N = stft_len(hint, F)
    T = x.shape[1] // F
    out = np.zeros((x.shape[0], T, N // 2 + 1), dtype=np.complex128)
    done = {}
    for c in range(x.shape[0]):
        b = int(base_of[c])
        if b not in done:
            done[b] = run(x[b].astype(np.float64))
        out[c] = done[b] * 2.0 ** int(CHANNEL_EXPS[c] - CHANNEL_EXPS[b])
    return out


def stft_analysis_limit(x, w, F, N):
    """[channels, T, 1]: (6 log2 N + 2) u sum_j |w_j x_j|"""
    l1 = frame_windows(np.abs(x).astype(np.float64), F, N) @ np.abs(w)
    return ((6 * log2i(N) + 2) * U * l1)[:, :, None]


def spectrum_l1(S, N):
    """[.., T]: the l1 norm of the Hermitian extension of bins 0..N/2"""
    a = np.abs(S)
    return a[..., 0] + a[..., N // 2] + 2 * a[..., 1:N // 2].sum(axis=-1)


def stft_synthesis_ref(oracle, S32, base_of, hint, F, win):
    """float64 [channels, T F] from the float32 spectra the kernel is given"""
    out = np.zeros((S32.shape[0], S32.shape[1] * F))
    for c in range(S32.shape[0]):
        b = int(base_of[c])
        out[c] = oracle.stft_synthesis(hint, F, win, S32[c].real, S32[c].imag) if b == c else \
            out[b] * 2.0 ** int(CHANNEL_EXPS[c] - CHANNEL_EXPS[b])
    return out


def stft_synthesis_limit(S32, w, hint, F, N, half):
    """[channels, T F]: (6 (log2 N + h) + R + 4) u magic sum_r |w[r F + i]| A_{t-r}"""
    R = N // F
    A = spectrum_l1(S32.astype(np.complex128), N) / N                 # [channels, T]
    T = A.shape[1]
    aw = np.abs(w).reshape(R, F)
    acc = np.zeros((A.shape[0], T, F))
    for r in range(R):
        acc[:, r:] += A[:, :T - r, None] * aw[r]
    return ((6 * (log2i(N) + (1 if half else 0)) + R + 4) * U * stft_magic(hint) * acc).reshape(A.shape[0], T * F)


def mdct_stages(n):
    return log2i(n // 4) + 2


def mdct_limit(x, n):
    """[rows, 1]: (6 S + 1) u ||x||_1"""
    return (6 * mdct_stages(n) + 1) * U * np.abs(x).astype(np.float64).sum(axis=-1, keepdims=True)


def imdct_limit(X, n):
    """[rows, 1]: (6 S + 4) u (4 / n) ||X||_1"""
    return (6 * mdct_stages(n) + 4) * U * (4.0 / n) * np.abs(X).astype(np.float64).sum(axis=-1, keepdims=True)


def mdct_frames_analysis_limit(x, w, F):
    """[channels, T, 1]: (6 S + 3) u sum_i |w_i xbuf_i|"""
    l1 = frame_windows(np.abs(x).astype(np.float64), F, 2 * F) @ np.abs(w)
    return ((6 * mdct_stages(2 * F) + 3) * U * l1)[:, :, None]


def mdct_frames_analysis_ref(oracle, x, base_of, F, win):
    """float64 [channels, T, F]"""
    out = np.zeros((x.shape[0], x.shape[1] // F, F))
    for c in range(x.shape[0]):
        b = int(base_of[c])
        out[c] = oracle.mdct_frames(F, win, x[c].astype(np.float64))[0] if b == c else \
            out[b] * 2.0 ** int(CHANNEL_EXPS[c] - CHANNEL_EXPS[b])
    return out


def mdct_frames_synthesis_ref(oracle, X32, base_of, w, F):
    """float64 [channels, T F]: the oracle's double IMDCT of every float32 coefficient frame, windowed, the second half of
    frame f-1 added to the first half of frame f (two terms: the sum does not depend on their order)"""
    C, T = X32.shape[:2]
    out = np.zeros((C, T, F))
    for c in range(C):
        b = int(base_of[c])
        if b != c:
            out[c] = out[b] * 2.0 ** int(CHANNEL_EXPS[c] - CHANNEL_EXPS[b])
            continue
        prev = np.zeros(F)
        for f in range(T):
            y = (oracle.imdct(2, X32[c, f].astype(np.float64)) if np.any(X32[c, f]) else np.zeros(2 * F)) * w
            out[c, f] = prev + y[:F]
            prev = y[F:]
    return out.reshape(C, T * F)


def mdct_frames_synthesis_limit(X32, w, F):
    """[channels, T F]: (6 S + 7) u (|w_i| A_f + |w_{F+i}| A_{f-1})"""
    A = (4.0 / (2 * F)) * np.abs(X32).astype(np.float64).sum(axis=-1)  # [channels, T]
    aw = np.abs(w)
    acc = A[:, :, None] * aw[:F]
    acc[:, 1:] += A[:, :-1, None] * aw[F:]
    return ((6 * mdct_stages(2 * F) + 7) * U * acc).reshape(A.shape[0], -1)


# ------------------------------------------------------------------------------------------------ plain float32 models
def _bitrev(n):
    k = log2i(n)
    r = np.zeros(n, dtype=np.int64)
    for b in range(k):
        r |= ((np.arange(n) >> b) & 1) << (k - 1 - b)
    return r


def plain_f32_fft(x, inverse=False, fault=None, unscaled_rows=()):
    """Textbook radix-2 (decimation in frequency, bit reversal last) in numpy float32: twiddles cos, -sin of 2 pi k / N in
    double rounded to float32, every product and every sum rounded to float32; the inverse is the conjugate of the forward
    of the conjugate, times 1 / N (exact: a power of two).  It shows that a limit is attainable; it is never a reference.
    fault: {"stage": s, "group": g, "rows": [...]}: in stage s (0 = the first, span N) butterfly group g of those rows picks its
    twiddles one table index too far.  unscaled_rows: rows whose inverse omits the 1 / N."""
    x = np.asarray(x, dtype=np.complex64)
    rows, n = x.shape
    if inverse:
        x = np.conj(x)
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    k = np.arange(max(1, n // 2))
    c, s = np.cos(2 * np.pi * k / n).astype(np.float32), (-np.sin(2 * np.pi * k / n)).astype(np.float32)
    span, stage = n, 0
    while span >= 2:
        half, groups = span // 2, n // span
        R, I = re.reshape(rows, groups, 2, half), im.reshape(rows, groups, 2, half)
        ar, br, ai, bi = R[:, :, 0], R[:, :, 1], I[:, :, 0], I[:, :, 1]
        idx = np.broadcast_to(np.arange(half) * groups, (rows, groups, half))
        if fault is not None and fault["stage"] == stage:
            idx = idx.copy()
            idx[np.asarray(fault["rows"]), fault["group"]] = (idx[0, 0] + 1) % max(1, n // 2)
        wr, wi = c[idx], s[idx]
        dr, di = ar - br, ai - bi
        re = np.stack([ar + br, dr * wr - di * wi], axis=2).reshape(rows, n)
        im = np.stack([ai + bi, dr * wi + di * wr], axis=2).reshape(rows, n)
        span, stage = half, stage + 1
    out = (re + 1j * im).astype(np.complex64)[:, _bitrev(n)]
    if inverse:
        scale = np.full((rows, 1), 1.0 / n, dtype=np.float32)
        scale[list(unscaled_rows)] = 1.0
        out = (np.conj(out) * scale).astype(np.complex64)
    return out


def plain_f32_stft_analysis(x, w, F, N, calls=None, history_from=None):
    """complex64 [channels, T, bins]: float32 window table times the frame, plain_f32_fft, bins 0..N/2.
    history_from = (c, d): in the second call channel c's history (the samples before the call) is channel d's."""
    fr = frame_windows(np.asarray(x, dtype=np.float32), F, N).copy()
    if history_from is not None:
        c, d = history_from
        other = frame_windows(np.asarray(x, dtype=np.float32), F, N)
        for f in range(calls[0], min(calls[0] + N // F - 1, fr.shape[1])):
            keep = (f + 1 - calls[0]) * F                               # samples of the frame that belong to the second call
            fr[c, f, :N - keep] = other[d, f, :N - keep]
    C, T = fr.shape[:2]
    z = (fr * np.asarray(w, dtype=np.float32)).reshape(C * T, N).astype(np.complex64)
    return plain_f32_fft(z).reshape(C, T, N)[:, :, :N // 2 + 1]


def plain_f32_stft_synthesis(S, w, hint, F, N):
    """float32 [channels, T F]: Hermitian extension, plain inverse transform, float32 window product, overlap-add oldest frame
    first, times the float32 magic"""
    S = np.asarray(S, dtype=np.complex64)
    C, T = S.shape[:2]
    full = np.concatenate([S, np.conj(S[:, :, N // 2 - 1:0:-1])], axis=2).reshape(C * T, N)
    y = plain_f32_fft(full, inverse=True).real.reshape(C, T, N) * np.asarray(w, dtype=np.float32)
    R = N // F
    acc = np.zeros((C, T, F), dtype=np.float32)
    for r in range(R - 1, -1, -1):                                      # oldest frame first
        acc[:, r:] += y[:, :T - r, r * F:(r + 1) * F]
    return (acc * np.float32(stft_magic(hint))).reshape(C, T * F)


def _mdct_tw(n):
    k = np.arange(n // 4)
    return (np.cos(-2 * np.pi * (k + 0.125) / n).astype(np.float32), np.sin(-2 * np.pi * (k + 0.125) / n).astype(np.float32))


def plain_f32_mdct(x):
    """[rows, n] -> [rows, n/2]: the N/4-point-FFT algorithm in float32 (fold, pre-rotation, plain_f32_fft, post-rotation)"""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[1]
    n2, n4 = n // 2, n // 4
    c, s = _mdct_tw(n)
    rot = np.concatenate([-x[:, 3 * n4:], x[:, :3 * n4]], axis=1)
    k = np.arange(n4)
    re, im = rot[:, 2 * k] - rot[:, n - 1 - 2 * k], rot[:, n2 - 1 - 2 * k] - rot[:, n2 + 2 * k]
    h = np.float32(0.5)
    z = plain_f32_fft((h * (re * c - im * s) + 1j * (h * (re * s + im * c))).astype(np.complex64))
    X = np.zeros((x.shape[0], n2), dtype=np.float32)
    X[:, 2 * k] = np.float32(2) * (z.real * c - z.imag * s)
    X[:, n2 - 1 - 2 * k] = np.float32(-2) * (z.real * s + z.imag * c)
    return X


def plain_f32_imdct(X):
    """[rows, n/2] -> [rows, n]; the scale as two float32 factors 8 f(1/sqrt n) and f(1/sqrt n)"""
    X = np.asarray(X, dtype=np.float32)
    n2 = X.shape[1]
    n, n4 = 2 * n2, n2 // 2
    c, s = _mdct_tw(n)
    k = np.arange(n4)
    re, im = X[:, 2 * k], X[:, n2 - 1 - 2 * k]
    h, cof = np.float32(0.5), np.float32(1.0 / np.sqrt(n))
    z = plain_f32_fft((h * (re * c - im * s) + 1j * (h * (re * s + im * c))).astype(np.complex64))
    g = np.float32(8) * cof
    rot = np.zeros((X.shape[0], n), dtype=np.float32)
    rot[:, 2 * k] = g * (z.real * c - z.imag * s)
    rot[:, n2 + 2 * k] = g * (z.real * s + z.imag * c)
    odd = np.arange(1, n, 2)
    rot[:, odd] = -rot[:, n - 1 - odd]
    return np.concatenate([rot[:, n4:], -rot[:, :n4]], axis=1) * cof


def plain_f32_mdct_frames_analysis(x, w, F):
    """float32 [channels, T, F]"""
    fr = frame_windows(np.asarray(x, dtype=np.float32), F, 2 * F) * np.asarray(w, dtype=np.float32)
    C, T = fr.shape[:2]
    return plain_f32_mdct(fr.reshape(C * T, 2 * F)).reshape(C, T, F)


def plain_f32_mdct_frames_synthesis(X, w, F, drop_tail=None):
    """float32 [channels, T F].  drop_tail = (c, f): the second half of channel c's frame f never reaches frame f + 1."""
    X = np.asarray(X, dtype=np.float32)
    C, T = X.shape[:2]
    y = plain_f32_imdct(X.reshape(C * T, F)).reshape(C, T, 2 * F) * np.asarray(w, dtype=np.float32)
    tail = y[:, :, F:].copy()
    if drop_tail is not None:
        tail[drop_tail[0], drop_tail[1]] = 0
    out = y[:, :, :F].copy()
    out[:, 1:] += tail[:, :-1]
    return out.reshape(C, T * F)


# ------------------------------------------------------------------------------------------------ checks
def pooled_rms_passes(got, ref, fft=False):
    """the old gates: one RMS over the whole output.  fft: relative 1e-6 (test_fft_batch_f32_vs_oracle); else TOL against the
    larger of the reference's RMS and 1, and relative (test_stft_mc_vs_oracle_streaming and the MDCT tests)"""
    err = float(np.sqrt(np.mean(np.abs(np.asarray(got).astype(np.complex128) - ref) ** 2)))
    scale = float(np.sqrt(np.mean(np.abs(ref) ** 2)))
    if fft:
        return err / scale < FFT_TOL
    return err <= TOL * max(1.0, scale) and err / scale <= TOL


def limit_check(got, ref, limit, what, check=True):
    """|got - ref| <= limit at every element (limit broadcasts against ref); names the worst element; returns the worst
    fraction of the limit (0 / 0 = 0, x / 0 = inf).  check=False only measures (the host's quarter condition)."""
    got = np.asarray(got)
    err = np.abs(got.astype(np.complex128 if np.iscomplexobj(got) or np.iscomplexobj(ref) else np.float64) - ref)
    limit = np.broadcast_to(limit, err.shape)
    assert np.all(np.isfinite(got)), f"{what}: not finite"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / limit)
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[w])
    if check:
        print(f"{what}: worst {worst:.3g} of its limit ({float(err[w]):.3g} of {float(limit[w]):.3g}) at {tuple(int(i) for i in w)}")
        assert worst <= 1.0, (f"{what}: {int(np.count_nonzero(ratio > 1))} elements over their limit; worst {float(err[w]):.3g} > "
                              f"{float(limit[w]):.3g} at {tuple(int(i) for i in w)}: got {got[w]!r} ref {ref[w]!r}")
    return worst


def scaled_equal(got, base_of, exps, what):
    """Row r carried the input of row base_of[r] times 2^exps[r], so its output must equal that row's output times 2^exps[r]
    bit for bit, wherever that value is zero or a normal float32.  Returns the number of elements compared.
    (Inputs are zero or at least 2^-22, window values at least 1e-17, a table's rounded zero 6e-17: the one product that can
    leave the normal range is an end-of-window sample of a 2^-20 row times such a table entry, 2^-50 of the term it is then
    added to.)"""
    got = np.asarray(got)
    g = np.ascontiguousarray(got).view(np.float32).reshape(got.shape[0], -1)
    compared = 0
    for r in range(g.shape[0]):
        b, e = int(base_of[r]), int(exps[r])
        if b == r:
            continue
        want = np.ldexp(g[b], e).astype(np.float32, copy=False)
        ok = (g[b] == 0) | ((np.abs(g[b]) >= TINY) & (np.abs(want) >= TINY) & (np.abs(want) < 2.0 ** 127))
        bad = np.flatnonzero(ok & (g[r] != want))
        assert bad.size == 0, (f"{what}: row {r} is not row {b} x 2^{e} at {bad.size} floats, first {int(bad[0])}: "
                               f"got {float(g[r][bad[0]]):.9g} want {float(want[bad[0]]):.9g}")
        assert np.all(np.isfinite(g[r])), f"{what}: row {r} not finite"
        compared += int(np.count_nonzero(ok))
    assert compared > 0, f"{what}: no scaled rows"
    return compared


def zero_where_silent(got, silent, what):
    """exact zeros wherever `silent` (broadcast against got) says linearity demands them; returns how many"""
    got = np.asarray(got)
    m = np.broadcast_to(silent, got.shape)
    bad = np.argwhere(m & (got != 0))
    assert bad.size == 0, f"{what}: {len(bad)} elements of silent input are not zero, first at {tuple(int(i) for i in bad[0])}: {got[tuple(bad[0])]!r}"
    return int(np.count_nonzero(m))


def zero_where_ref_zero(got_im, ref_im, what):
    """an imaginary part that is exactly zero in the oracle is exactly zero"""
    bad = np.argwhere((np.asarray(ref_im) == 0) & (np.asarray(got_im) != 0))
    assert bad.size == 0, f"{what}: {len(bad)} imaginary parts are zero in the oracle and not here, first at {tuple(int(i) for i in bad[0])}"
    return int(np.count_nonzero(np.asarray(ref_im) == 0))


def silent_frames(x, F, N):
    """[channels, T, 1] bool: frames whose N buffered samples are all zero"""
    return ~np.any(frame_windows(np.asarray(x) != 0, F, N), axis=2)[:, :, None]


def silent_samples(S, F, N):
    """[channels, T F] bool: output samples all of whose R = N / F contributing frames are all-zero spectra / coefficients"""
    live = np.any(np.asarray(S) != 0, axis=2)                           # [channels, T]
    T = live.shape[1]
    any_live = live.copy()
    for r in range(1, N // F):
        any_live[:, r:] |= live[:, :T - r]
    return np.repeat(~any_live, F, axis=1)


def centre_frames(x, F, N):
    """[(channel, frame)] whose buffer holds exactly one non-zero sample, at the window centre N/2"""
    fr = frame_windows(np.asarray(x) != 0, F, N)
    return [(int(c), int(f)) for c, f in np.argwhere((fr.sum(axis=2) == 1) & fr[:, :, N // 2])]
