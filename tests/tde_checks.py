"""Shared pieces of the time-delay estimator's tests (test_tde_host.py, test_tde_gpu.py; include/llz_tde.h): the signals, the
float64 model of the header's definition, the limits, a float32 model with the recursion's rounding order and the faults to plant
in it.  Plain numpy; nothing here touches a GPU.

Signals (signals): eight channels from one seeded white row a (magnitudes in [1/4, 1), random signs):
  0 a          1..5  a delayed by 0, 1, -3, N/8, -N/8 samples          6  a delayed by 5.25 samples (a phase ramp over the whole row)
  7 a delayed by 5 samples in front of sample SWITCH_FRAME hop and by 17 samples from there on
each of 1..7 with independent white noise of its own at 0.3 of the signal's level.

Model (model64): per frame numpy's float64 rfft of float64(x32) float64(w32); the recursion with the float32 lam and the float32
g = (float)(1 - (double)lam) as float64 values; W, irfft, the peak and its parabola as the header writes them.

Limits, derived and not measured (u = 2^-24; everything from the model's own quantities):
  * eX_f[k] = (6 log2 N + 2) u sum_j |w_j x_j|: a forward transform's error per bin (tests/transform_checks.py);
  * eP_f = eX |Y| + eY |X| + eX eY + 4 u |X| |Y| for P = conj(X) Y (two rounded products and a rounded sum per part), and
    2 eX |X| + eX^2 + 4 u |X|^2 for gx, the same for gy;
  * eS_f = lam eS_{f-1} + g eP_f + 3 u A_f with A_f = lam A_{f-1} + g |P_f| >= |S_f| (two rounded products, one rounded sum);
    eS_0 = eP_0; eGx, eGy likewise -- these are the state read-out's per-bin limits (lim_state);
  * eW: CC eS;  PHAT and SCOT, W = S / d with d = |S| + delta or sqrt(Gx Gy) + delta and ed the error of d (eS for PHAT,
    sqrt(Gx Gy) (eGx / Gx + eGy / Gy) for SCOT, twice the first-order term):  |W^ - W| <= (eS + |W| ed) / (d - ed) + 8 u |W|,
    which is about 2 eS / (|S| + delta), capped at 2 (|W| <= 1 on both sides); a bin whose d is 0 has eW = 2 unless eS is 0 too;
  * lim_r = (1 / N) sum over the Hermitian extension of eW + 6 log2 N u (1 / N) sum |W~| for the inverse transform: one value per
    (frame, pair), the same for every lag;
  * delay: the parabola's partial derivatives in a, b, c with |den| lessened by the 4 lim_r it may be off by,
    lim_d = lim_r (|d/da| + |d/db| + |d/dc|) + 4 u max(1, |tau*|), capped at 1 (the clamp keeps both sides within 0.5).
The integer lag is compared only where the model's peak exceeds every other lag in range by more than 2 lim_r (margin_ok); the
tests assert that this holds on every (pair, frame) of every case."""
import numpy as np

from tests import transform_checks as tc

U = 2.0 ** -24
HAMMING, BLACKMAN, KAISER = 0, 1, 2
CC, PHAT, SCOT = 0, 1, 2
CHANNELS = 8
A, D0, D1, DM3, DP8, DM8, DFRAC, DSWITCH = range(8)
SWITCH_FRAME, SWITCH_FROM, SWITCH_TO = 10, 5, 17
FRAC = 5.25
NOISE = 0.3
FAULTS = ("conj", "late", "window", "hermitian", "mirror")

# the pairs every table below draws from: the planted delays, the auto pair, a repeated pair, a pair and its swap
BASE = [(A, D0), (A, D1), (A, DM3), (A, DP8), (A, DM8), (A, DFRAC), (A, A), (A, D1), (D1, A), (DM3, A), (D0, D0)]
AUTO, REPEATED, SWAP = 6, (1, 7), (1, 8)
PAIRS37 = [BASE[i % len(BASE)] for i in range(37)]


def planted(N):
    """{channel: its integer delay against channel a}"""
    return {D0: 0, D1: 1, DM3: -3, DP8: N // 8, DM8: -(N // 8)}


# (N, hop, weight, max_lag, (k_lo, k_hi), pairs, lam, frames)
#   (64, 16): fewer bins than lanes; (4096, 2048): a ragged ninth bin slot; every weighting; max_lag 1, N/8 and N/2 - 1; the full
#   band and interior bands; 1, 3 and 37 pairs; lam 0; 12 frames, 40 through the switch at lam 0.8
CASES = [
    (64, 16, PHAT, 31, (0, 32), PAIRS37, 0.9, 12),
    (256, 128, SCOT, 32, (8, 96), [(A, DP8), (A, DM8), (A, DFRAC)], 0.9, 12),
    (1024, 256, CC, 1, (1, 511), [(A, D0), (A, D1), (D1, A)], 0.9, 12),
    (1024, 256, CC, 128, (16, 400), [(A, DP8), (A, DM3), (DM3, A)], 0.9, 12),
    (1024, 1024, PHAT, 511, (0, 512), [(A, DP8)], 0.0, 12),
    (4096, 2048, PHAT, 512, (1, 2047), PAIRS37, 0.9, 12),
    (256, 128, PHAT, 127, (1, 127), [(A, DSWITCH), (A, D0), (A, A)], 0.8, 40),
    (4096, 2048, SCOT, 2047, (0, 2048), [(A, DSWITCH), (DSWITCH, A), (A, DM8)], 0.8, 40),
]
CASE_IDS = [f"{c[0]}-{c[1]}-{('cc', 'phat', 'scot')[c[2]]}-L{c[3]}-p{len(c[5])}-f{c[7]}" for c in CASES]


def window_of(N):
    return (HAMMING, KAISER, BLACKMAN)[tc.log2i(N) % 3]


def samples(N, hop, frames):
    return (frames - 1) * hop + N


def signals(N, hop, frames):
    """x [8, n] float32, n = (frames - 1) hop + N"""
    n = samples(N, hop, frames)
    pad = N                                                  # |delay| <= N / 8, and the phase ramp's wrap-around stays in the pad
    base = tc.noise_row(n + 2 * pad, 21, real=True).astype(np.float64)
    t = np.arange(n)

    def delayed(d):
        return base[pad + t - d]
    spec = np.fft.rfft(base)
    k = np.arange(len(spec))
    frac = np.fft.irfft(spec * np.exp(-2j * np.pi * k * FRAC / len(base)), len(base))[pad:pad + n]
    switch = np.where(t < SWITCH_FRAME * hop, delayed(SWITCH_FROM), delayed(SWITCH_TO))
    rows = [delayed(0)] + [delayed(d) for d in (0, 1, -3, N // 8, -(N // 8))] + [frac, switch]
    level = np.sqrt(np.mean(base ** 2))
    for c in range(1, CHANNELS):
        own = tc.noise_row(n, 30 + c, real=True).astype(np.float64)
        rows[c] = rows[c] + NOISE * level * own / np.sqrt(np.mean(own ** 2))
    return np.stack(rows).astype(np.float32)


def frames_of(x, N, hop):
    """[channels, K, N]: frame f = samples [f hop, f hop + N), no padding"""
    return np.lib.stride_tricks.sliding_window_view(x, N, axis=1)[:, ::hop]


def lam_pair(lam):
    lam32 = np.float32(lam)
    return lam32, np.float32(1.0 - float(lam32))


def peak_of(r, L, dtype):
    """(tau*, delay, peak) of one curve r[0 .. 2 L] (lags -L .. L) with its circular neighbours lo = r[-L - 1], hi = r[L + 1]"""
    curve, lo, hi = r
    if np.isnan(curve).any():
        return 0, dtype(np.nan), dtype(np.nan)
    j = int(np.argmax(curve))                                # the first maximum: the lowest lag among equal values
    a = dtype(curve[j - 1] if j > 0 else lo)
    b = dtype(curve[j])
    c = dtype(curve[j + 1] if j < 2 * L else hi)
    den = dtype(dtype(a - dtype(dtype(2) * b)) + c)
    frac = dtype(0)
    if den < 0:
        frac = dtype(min(max(dtype(dtype(dtype(0.5) * dtype(a - c)) / den), dtype(-0.5)), dtype(0.5)))
    return j - L, dtype(dtype(j - L) + frac), b


def model64(x, w32, case, lams=None):
    """The header's definition in float64 with the limits.  lams: {frame: lam} applied from that frame on (set_forget).
    Returns a dict of arrays over [frames, pairs, ...]: curve [.., 2 L + 1], tau, delay, peak, state [.., bins, 4], lim_r, lim_d,
    lim_state [.., bins, 4], margin (the peak's lead over every other lag in range)."""
    N, hop, weight, L, (k_lo, k_hi), pairs, lam, K = case
    bins, log2n = N // 2 + 1, tc.log2i(N)
    fr = frames_of(x.astype(np.float64), N, hop)[:, :K] * w32.astype(np.float64)
    S = np.fft.rfft(fr, axis=2)                                               # [channels, K, bins]
    eX = (6 * log2n + 2) * U * np.abs(fr).sum(axis=2)[:, :, None]             # [channels, K, 1]
    herm = np.full(bins, 2.0)
    herm[0] = herm[-1] = 1.0
    band = np.zeros(bins, dtype=bool)
    band[k_lo:k_hi + 1] = True
    idx = np.arange(-L, L + 1) % N
    out = {k: np.zeros((K, len(pairs)) + s) for k, s in (("curve", (2 * L + 1,)), ("tau", ()), ("delay", ()), ("peak", ()),
                                                         ("state", (bins, 4)), ("lim_r", ()), ("lim_d", ()),
                                                         ("lim_state", (bins, 4)), ("margin", ()))}
    for p, (cx, cy) in enumerate(pairs):
        l32, g32 = lam_pair(lam)
        st = err = env = None
        for f in range(K):
            if lams and f in lams:
                l32, g32 = lam_pair(lams[f])
            lm, g = float(l32), float(g32)
            X, Y, ex, ey = S[cx, f], S[cy, f], eX[cx, f], eX[cy, f]
            ax, ay = np.abs(X), np.abs(Y)
            P = np.conj(X) * Y
            term = np.stack([P.real, P.imag, ax ** 2, ay ** 2], axis=-1)
            eP = ex * ay + ey * ax + ex * ey + 4 * U * ax * ay
            eterm = np.stack([eP, eP, 2 * ex * ax + ex ** 2 + 4 * U * ax ** 2, 2 * ey * ay + ey ** 2 + 4 * U * ay ** 2], axis=-1)
            aterm = np.stack([np.abs(P), np.abs(P), ax ** 2, ay ** 2], axis=-1)
            if f == 0 or lm == 0.0:
                st, err, env = term, eterm, aterm
            else:
                st = lm * st + g * term
                env = lm * env + g * aterm
                err = lm * err + g * eterm + 3 * U * env
            Sc = st[:, 0] + 1j * st[:, 1]
            eS = err[:, 0]
            if weight == CC:
                W, eW = Sc, eS
            else:
                if weight == PHAT:
                    mag, ed = np.abs(Sc), eS
                else:
                    mag = np.sqrt(st[:, 2] * st[:, 3])
                    with np.errstate(divide="ignore", invalid="ignore"):
                        ed = np.where(mag > 0, mag * (err[:, 2] / st[:, 2] + err[:, 3] / st[:, 3]), np.inf)
                d = mag + float(np.float32(case_delta(case)))
                with np.errstate(divide="ignore", invalid="ignore"):
                    W = np.where(d == 0, 0.0, Sc / d)
                    eW = np.where(d > ed, (eS + np.abs(W) * ed) / (d - ed) + 8 * U * np.abs(W), 2.0)
                eW = np.where((d == 0) & (eS == 0), 0.0, np.minimum(eW, 2.0))
            W = np.where(band, W, 0.0)
            eW = np.where(band, eW, 0.0)
            r = np.fft.irfft(W, N)
            lim_r = (herm * eW).sum() / N + 6 * log2n * U * (herm * np.abs(W)).sum() / N
            curve = r[idx]
            tau, delay, peak = peak_of((curve, r[(-L - 1) % N], r[(L + 1) % N]), L, np.float64)
            j = tau + L
            a, b, c = r[(tau - 1) % N], r[tau % N], r[(tau + 1) % N]
            den = abs(a - 2 * b + c) - 4 * lim_r
            if den > 0:
                dd = 0.5 / den + 0.5 * (abs(a - c) + 2 * lim_r) / den ** 2
                lim_d = min(1.0, lim_r * (2 * dd + (abs(a - c) + 2 * lim_r) / den ** 2) + 4 * U * max(1, abs(tau)))
            else:
                lim_d = 1.0
            others = np.delete(curve, j)
            out["curve"][f, p], out["tau"][f, p], out["delay"][f, p], out["peak"][f, p] = curve, tau, delay, peak
            out["state"][f, p], out["lim_state"][f, p] = st, err
            out["lim_r"][f, p], out["lim_d"][f, p], out["margin"][f, p] = lim_r, lim_d, b - others.max()
    return out


def case_delta(case):
    """the handle's delta: 0 for PHAT (the denominator-0 rule is the guard), a small absolute floor for SCOT"""
    return 0.0 if case[2] != SCOT else 1e-6


def margin_ok(ref):
    """[frames, pairs] bool: the model's peak leads every other lag in range by more than 2 lim_r"""
    return ref["margin"] > 2 * ref["lim_r"]


def model_f32(x, w32, case, fault=None, lams=None):
    """the same outputs (curve, tau, delay, peak, state) the way plain float32 gets there: tc.plain_f32_fft forward and inverse,
    the recursion with every product and sum rounded to float32; fault: one of FAULTS"""
    N, hop, weight, L, (k_lo, k_hi), pairs, lam, K = case
    bins = N // 2 + 1
    f32 = np.float32
    fr = frames_of(np.asarray(x, dtype=f32), N, hop)[:, :K]
    Cn = fr.shape[0]
    w32 = np.asarray(w32, dtype=f32)
    win = np.ones(N, dtype=f32) if fault == "window" else w32
    SP = tc.plain_f32_fft((fr * win).reshape(Cn * K, N).astype(np.complex64)).reshape(Cn, K, N)[:, :, :bins]
    delta = f32(case_delta(case))
    band = np.zeros(bins, dtype=bool)
    band[k_lo:k_hi + 1] = True
    idx = np.arange(-L, L + 1) % N
    out = {k: np.zeros((K, len(pairs)) + s) for k, s in (("curve", (2 * L + 1,)), ("tau", ()), ("delay", ()), ("peak", ()),
                                                         ("state", (bins, 4)))}
    for p, (cx, cy) in enumerate(pairs):
        l32, g32 = lam_pair(lam)
        st = None
        prev = None
        for f in range(K):
            if lams and f in lams:
                l32, g32 = lam_pair(lams[f])
            xr, xi = SP[cx, f].real, SP[cx, f].imag
            yr, yi = SP[cy, f].real, SP[cy, f].imag
            if fault == "conj":
                xi, yi = -xi, -yi                                            # X conj(Y) instead of conj(X) Y
            term = np.stack([xr * yr + xi * yi, xr * yi - xi * yr, xr * xr + xi * xi, yr * yr + yi * yi], axis=-1)   # float32
            assert term.dtype == f32
            now = term
            if fault == "late" and f > 0:
                now = prev                                                   # the recursion takes frame f - 1's products
            prev = term
            st = now if (f == 0 or l32 == 0) else (l32 * st + g32 * now)
            assert st.dtype == f32
            if weight == CC:
                wr, wi = st[:, 0], st[:, 1]
            else:
                mag = np.hypot(st[:, 0], st[:, 1]) if weight == PHAT else np.sqrt(st[:, 2]) * np.sqrt(st[:, 3])
                d = (mag + delta).astype(f32)
                with np.errstate(divide="ignore", invalid="ignore"):
                    wr = np.where(d == 0, f32(0), st[:, 0] / d).astype(f32)
                    wi = np.where(d == 0, f32(0), st[:, 1] / d).astype(f32)
            W = np.where(band, wr + 1j * wi, 0).astype(np.complex64)
            W[0] = W[0].real
            W[-1] = W[-1].real
            upper = W[1:-1][::-1] if fault == "hermitian" else np.conj(W[1:-1][::-1])
            full = np.concatenate([W, upper]).astype(np.complex64)
            r = tc.plain_f32_fft(full[None, :], inverse=True)[0].real.astype(f32)
            if fault == "mirror":
                r = r[(-np.arange(N)) % N]
            curve = r[idx]
            tau, delay, peak = peak_of((curve, r[(-L - 1) % N], r[(L + 1) % N]), L, f32)
            out["curve"][f, p], out["tau"][f, p], out["delay"][f, p], out["peak"][f, p] = curve, tau, delay, peak
            out["state"][f, p] = st
    return out


def ratios(got, ref):
    """worst fractions of the limits over the (frame, pair)s got holds: {"curve", "peak", "delay", "state"}, and the count of
    integer lags that differ where the margin condition lets them be compared; got's arrays may hold fewer frames than ref's
    (the curve and the state: any leading shape that broadcasts, compared against ref's frames given by `frames`)"""
    ok = margin_ok(ref)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        def frac(err, lim):
            return float(np.where(err == 0, 0.0, err / lim).max())
        out["curve"] = frac(np.abs(got["curve"] - ref["curve"]), ref["lim_r"][..., None])
        out["peak"] = frac(np.abs(got["peak"] - ref["peak"]), ref["lim_r"])
        out["delay"] = frac(np.where(ok, np.abs(got["delay"] - ref["delay"]), 0.0), ref["lim_d"])
        out["state"] = frac(np.abs(got["state"] - ref["state"]), ref["lim_state"])
    out["lags"] = int(np.count_nonzero(ok & (got["tau"] != ref["tau"])))
    return out


def check(got, ref, what):
    """every limit on every (frame, pair); prints the worst ratio of each before it asserts; returns them"""
    r = ratios(got, ref)
    print(f"{what}: curve {r['curve']:.3g}, peak {r['peak']:.3g}, delay {r['delay']:.3g}, state {r['state']:.3g} of their limits; "
          f"{r['lags']} integer lags differ; margin >= {ref['margin'].min():.3g}, lim_r <= {ref['lim_r'].max():.3g}")
    assert int(np.count_nonzero(~margin_ok(ref))) == 0, f"{what}: (pair, frame)s outside the margin condition"
    for k in ("curve", "peak", "delay", "state"):
        assert r[k] <= 1.0, f"{what}: {k} limit missed: {r[k]:.3g}"
    assert r["lags"] == 0, f"{what}: {r['lags']} integer lags differ from the model's"
    return r
