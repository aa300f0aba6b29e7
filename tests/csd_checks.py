"""Shared pieces of the Welch cross-spectra tests (test_csd_host.py, test_csd_gpu.py; include/llz_spectral.h): the signals, the
double reference, the limits, a plain float32 model and the faults to plant in it.  Plain numpy; nothing here touches a GPU.

Signals (signals): eight channels, no two alike, K = 2 RUN + 3 frames (two full runs and a ragged one):
  0 a: noise, magnitudes in [1/4, 1)          1 b: (0.5 a delayed by 3 samples + own noise) 2^-20
  2 c, 3 d: sine and cosine at bin N/8 + 0.3 (the imaginary cross term is of full size)
  4 e: zeros                                  5, 6: a times 2^10 and 2^-20, neighbours          7: -4 a
PAIRS: (a,a), (a,b), (b,a), (c,d), (d,c), copies against b, a and each other, (a,e), (e,a), (e,e), (a,b) again, (a,-4a), (b,b).

Reference (reference): per frame numpy's float64 FFT of float64(x32) float64(w32), w32 the float32 window table; summed over the
frames in float64.  raw layout [pairs, bins, 4] = Sxx, Syy, Re Sxy, Im Sxy with Sxy = sum_f conj(X_f) Y_f.

Limits, derived and not measured (u = 2^-24, S_f = sum_j |w_j x_j| over frame f):
  * per bin: |got - ref| <= (12 log2 N + 12 + RUN) u sum_f Sx_f Sy_f for Re Sxy and Im Sxy -- two analysis errors of
    (6 log2 N + 2) u S (tests/transform_checks.py) with |X_f| <= Sx_f, 4 u for the complex product, RUN u for the float32 sums
    inside a run, the rest for the second-order terms and the one conversion;
  * pooled per pair: rms_k |got - ref| <= 1e-5 sqrt(mean_k Sxx_ref mean_k Syy_ref) for the complex Sxy, the project's 1e-5 gate
    with the Cauchy-Schwarz normaliser.
  * Sxx and Syy of a pair (x, y) are the Sxy of the pairs (x, x) and (y, y) and are held to THOSE pairs' limits (sum_f Sx_f^2
    and mean_k Sxx_ref; the y side likewise): the limits are per channel scale.  With the cross normaliser on all four sums a
    loud x beside a quiet y (2^0 against 2^-20 here) would have its own Sxx held to 2^-20 of what float32 can give, and beside a
    silent y to zero.
Condition on both: the plain float32 model (model_f32: tc.plain_f32_fft per frame, float32 products, float32 sums in runs of
RUN, double across runs) stays at or below a QUARTER of each on every case; test_csd_host.py asserts it, and that each planted
fault (FAULTS) misses the gate on the noise pair and the per-bin limit on the tone pair.  (The kernels' run sums are compensated
float32 sums and land well inside the model's figures; the model stays plain: it shows what the limits must leave room for.)"""
import numpy as np

from tests import transform_checks as tc

U = 2.0 ** -24
RUN = 32
TOL = 1e-5
K_FRAMES = 2 * RUN + 3
HAMMING, BLACKMAN, KAISER = 0, 1, 2
SIZES = (64, 128, 256, 512, 1024, 2048, 4096)
REGISTER_SIZES = (256, 512, 1024)                 # the sizes with a register form (2048 spills: staged)
# fft_len / hop: every hop at 256 and 1024, one elsewhere; under fft_generic one per size
RATIOS = {64: (4,), 128: (2,), 256: (1, 2, 4), 512: (1,), 1024: (1, 2, 4), 2048: (4,), 4096: (2,)}
GENERIC_RATIO = {64: 1, 128: 4, 256: 2, 512: 4, 1024: 4, 2048: 2, 4096: 1}
CASES = [(N, N // r, False) for N in SIZES for r in RATIOS[N]] + [(N, N // GENERIC_RATIO[N], True) for N in SIZES]
SHAPES = sorted({(N, hop) for N, hop, _g in CASES})

A, B, C_SIN, D_COS, E_ZERO, A_HI, A_LO, A_M4 = range(8)
CHANNELS = 8
PAIRS = [(A, A), (A, B), (B, A), (C_SIN, D_COS), (D_COS, C_SIN), (A_HI, B), (A_LO, B), (A_HI, A), (A_LO, A_HI),
         (A, E_ZERO), (E_ZERO, A), (E_ZERO, E_ZERO), (A, B), (A, A_M4), (B, B)]
NOISE_PAIR, TONE_PAIR, CONJ_PAIRS, REPEATED, MINUS4_PAIR = 1, 3, (1, 2), (1, 12), 13
# (pair, base pair, ex, ey): the pair's x is the base's times 2^ex, its y the base's times 2^ey
SCALED = [(5, 1, 10, 0), (6, 1, -20, 0), (7, 0, 10, 0), (8, 0, -20, 10)]
AUTO_PAIRS = (0, 14)                              # (a, a), (b, b): Sxy == Sxx, imaginary part exactly 0
FAULTS = ("conj", "late", "window", "drop")


def window_of(N):
    return (HAMMING, KAISER, BLACKMAN)[tc.log2i(N) % 3]


def samples(N, hop, frames=K_FRAMES):
    return (frames - 1) * hop + N


def signals(N, hop):
    """x [8, n] float32, n = (K - 1) hop + N"""
    n = samples(N, hop)
    a = tc.noise_row(n, 11, real=True).astype(np.float64)
    own = tc.noise_row(n, 12, real=True).astype(np.float64)
    delayed = np.concatenate([np.zeros(3), a[:-3]])
    t = np.arange(n, dtype=np.float64)
    ang = 2 * np.pi * (N / 8 + 0.3) * t / N
    rows = [a, (0.5 * delayed + 0.5 * own) * 2.0 ** -20, np.sin(ang), np.cos(ang), np.zeros(n), a * 2.0 ** 10, a * 2.0 ** -20,
            -4.0 * a]
    return np.stack(rows).astype(np.float32)


def frames_of(x, N, hop):
    """[channels, K, N]: frame f = samples [f hop, f hop + N), no padding"""
    return np.lib.stride_tricks.sliding_window_view(x, N, axis=1)[:, ::hop]


def sums(X, Y):
    """[bins, 4] float64 from two [K, bins] complex spectra"""
    sxy = (np.conj(X) * Y).sum(axis=0)
    return np.stack([(np.abs(X) ** 2).sum(axis=0), (np.abs(Y) ** 2).sum(axis=0), sxy.real, sxy.imag], axis=-1)


def reference(x, w32, N, hop, pairs=PAIRS):
    """(ref [pairs, bins, 4] float64, lim [pairs, 1, 4], gate [3, pairs]: Sxx, Syy, Sxy)"""
    fr = frames_of(x.astype(np.float64), N, hop) * w32.astype(np.float64)
    S = np.fft.rfft(fr, axis=2)
    l1 = np.abs(fr).sum(axis=2)                                         # [channels, K]
    ref = np.stack([sums(S[cx], S[cy]) for cx, cy in pairs])
    c = (12 * tc.log2i(N) + 12 + RUN) * U
    lim = np.array([[c * (l1[cx] * l1[cx]).sum(), c * (l1[cy] * l1[cy]).sum()] + 2 * [c * (l1[cx] * l1[cy]).sum()]
                    for cx, cy in pairs])
    mx, my = ref[:, :, 0].mean(axis=1), ref[:, :, 1].mean(axis=1)
    gate = TOL * np.stack([mx, my, np.sqrt(mx * my)])
    return ref, lim[:, None, :], gate


def model_f32(x, w32, N, hop, pairs=PAIRS, fault=None):
    """[pairs, bins, 4] float64 the way plain float32 would get there; fault: one of FAULTS, planted on the y side"""
    fr = frames_of(np.asarray(x, dtype=np.float32), N, hop)
    Cn, K = fr.shape[:2]
    w32 = np.asarray(w32, dtype=np.float32)

    def spectra(w):
        z = (fr * w).reshape(Cn * K, N).astype(np.complex64)
        return tc.plain_f32_fft(z).reshape(Cn, K, N)[:, :, :N // 2 + 1]
    SX = spectra(w32)
    SY = spectra(np.roll(w32, 1)) if fault == "window" else SX
    if fault == "late":
        SY = np.roll(SY, -1, axis=1)                                    # y's frame f is taken one hop later
    out = np.zeros((len(pairs), N // 2 + 1, 4))
    last = K - 1 if fault == "drop" else K
    for p, (cx, cy) in enumerate(pairs):
        xr, xi = SX[cx].real, SX[cx].imag
        yr, yi = SY[cy].real, SY[cy].imag
        if fault == "conj":
            xi, yi = -xi, -yi                                           # X conj(Y) instead of conj(X) Y
        terms = np.stack([xr * xr + xi * xi, yr * yr + yi * yi, xr * yr + xi * yi, xr * yi - xi * yr], axis=-1)   # float32
        for f0 in range(0, last, RUN):
            part = np.zeros(terms.shape[1:], dtype=np.float32)
            for f in range(f0, min(f0 + RUN, last)):
                part = part + terms[f]
            out[p] += part.astype(np.float64)
    return out


def ratios(got, ref, lim, gate):
    """(worst fraction of the per-bin limit [pairs], worst fraction of the gate [pairs]); 0 / 0 = 0, x / 0 = inf"""
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_bin = np.where(err == 0, 0.0, err / np.broadcast_to(lim, err.shape)).max(axis=(1, 2))
        rms = np.stack([np.sqrt((err[:, :, 0] ** 2).mean(axis=1)), np.sqrt((err[:, :, 1] ** 2).mean(axis=1)),
                        np.sqrt((err[:, :, 2] ** 2 + err[:, :, 3] ** 2).mean(axis=1))])
        pooled = np.where(rms == 0, 0.0, rms / gate).max(axis=0)
    return per_bin, pooled


def check_raw(got, ref, lim, gate, what, fraction=1.0):
    """both limits on every pair; prints the worst ratio of each before it asserts; returns them"""
    assert np.all(np.isfinite(got)), f"{what}: not finite"
    per_bin, pooled = ratios(got, ref, lim, gate)
    print(f"{what}: worst {per_bin.max():.3g} of the per-bin limit (pair {int(per_bin.argmax())}), "
          f"{pooled.max():.3g} of the gate (pair {int(pooled.argmax())})")
    assert per_bin.max() <= fraction, f"{what}: per-bin limit missed, fractions per pair {np.round(per_bin, 3)}"
    assert pooled.max() <= fraction, f"{what}: pooled gate missed, fractions per pair {np.round(pooled, 3)}"
    return float(per_bin.max()), float(pooled.max())


def readouts64(raw, frames, u_sum):
    """the five read-outs from the handle's own raw sums, in float64: psd_x, psd_y [pairs, bins]; csd, tf [pairs, bins, 2];
    coherence [pairs, bins]"""
    sxx, syy, re, im = (raw[..., k] for k in range(4))
    ku = frames * u_sum
    with np.errstate(divide="ignore", invalid="ignore"):
        den = sxx * syy
        coh = np.where(den == 0, np.nan, (re * re + im * im) / den)
        tf = np.stack([np.where(sxx == 0, np.nan, re / sxx), np.where(sxx == 0, np.nan, im / sxx)], axis=-1)
    return {"psd_x": sxx / ku, "psd_y": syy / ku, "csd": np.stack([re / ku, im / ku], axis=-1), "coherence": coh, "transfer": tf}


def within_ulps(got32, want64, ulps, what):
    """|got - float32(want)| <= ulps float32 ulp of the wanted value; NaN exactly where NaN is wanted"""
    got32 = np.asarray(got32, dtype=np.float32)
    want32 = want64.astype(np.float32)
    assert np.array_equal(np.isnan(got32), np.isnan(want32)), f"{what}: NaN pattern differs"
    ok = ~np.isnan(want32)
    err = np.abs(got32[ok].astype(np.float64) - want32[ok].astype(np.float64))
    room = ulps * np.spacing(np.abs(want32[ok])).astype(np.float64)
    assert np.all(err <= room), f"{what}: {int(np.count_nonzero(err > room))} values off by more than {ulps} ulp"
