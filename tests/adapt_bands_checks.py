"""Shared pieces of the per-band adaptive filter's tests (test_adapt_bands_host.py, test_adapt_bands_gpu.py; llz_adapt_bands_mc,
include/llz_adapt_bands.h): the MODEL of the definition in float64 (the reference everywhere) and in float32 / complex64 (the
device's stand-in on a machine without a GPU), the case generator, the device runner and the checks.  The model is written from
the definition in llz_adapt_bands.h in plain numpy and knows nothing of the kernel: a shift register of frames per (channel,
bin), no tap ceiling, no lanes.

The definition, per (channel, bin): K complex weights w_q, initially zero, a history x[m - q], zero before frame 0.  For frame m:
y = sum_{q < K} w_q x[m - q] (no conjugate on w); e = d[m] - y; where the channel's mu != 0: p = sum_{q < K} |x[m - q]|^2,
g = mu e / (p + delta), w_q += g conj(x[m - q]).

Limits (none of them taken from the device's results), TOL = edge_checks.TOL = 1e-5, the project's gate:
  * the error: per (channel, bin, run of RUN = 16 frames) rms(e - e_ref) <= TOL rms(d of that channel and bin over the case);
  * the taps: per (channel, bin) |w - w_ref|_2 <= TOL |h|_2;
  * the misalignment |w - h|_2 at most max(2 x the float64 model's, the model's + TOL |h|_2) (the second where the model's own
    lies below a float32 rounding of the taps: what the tap gate implies by the triangle inequality);
  * convergence: the last run's error rms below a tenth of the first run's wherever the float64 model's is;
  * the zero bins of channel 0: x = 0 and d = 0 gives e, y and weights exactly zero; x = 0 and d != 0 gives e bit-equal to d and
    weights exactly zero;
  * e bit-equal to float32(d) - y everywhere.
The float32 model sits at a few percent of the first two; the planted faults of test_adapt_bands_host.py miss them."""
import numpy as np

from tests import adapt_checks as ac
from tests import edge_checks as ec

TOL = ec.TOL
U = 2.0 ** -24
MU = 0.5
DELTA = 1e-3
RUN = 16
CEILINGS = (4, 8, 16, 32, 64)
# (taps, bins, frames): the smallest that reach every instance and its mask -- one tap, a full and a just exceeded ceiling of 4,
# full ceilings of 16 and 64, one tap past 32; bins of 5 and 33 put several channels into one wave, 129 and 65 straddle rows
SHAPES = [(1, 5, 200), (4, 33, 200), (5, 33, 200), (16, 129, 300), (33, 65, 400), (64, 33, 600)]
CHANNELS = (3, 37)
LONG = (8, 2049, 64, 3)         # taps, bins, frames, channels: a row longer than any workgroup
ZERO_BOTH, ZERO_X = 1, 2        # bins of channel 0 with x = 0: d = 0 as well, and d as it was
FAULTS = ("not_conjugated", "one_frame_late", "newest_power_only", "ceiling_taps_live")
cached = ac.cached
bits = ac.bits


def ceiling(taps):
    return next(c for c in CEILINGS if taps <= c)


# ------------------------------------------------------------------------------------------------ the cases
def gaussian(oracle, channels, frames, bins, seed):
    """[channels, frames, bins] complex64 of unit variance from the oracle's generator (adapt_checks.gaussian)"""
    g = ac.gaussian(oracle, channels, 2 * frames * bins, seed).reshape(channels, 2, frames, bins)
    return ((g[:, 0] + 1j * g[:, 1]) * np.float32(np.sqrt(0.5))).astype(np.complex64)


def responses(channels, taps, bins, seed):
    """[channels, taps, bins] complex128 of float32 values: complex Gaussian times exp(-q / (K / 4 + 1)), of unit norm per
    (channel, bin)"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((channels, taps, bins)) + 1j * rng.standard_normal((channels, taps, bins))
    h *= np.exp(-np.arange(taps) / (taps / 4 + 1))[None, :, None]
    h /= np.sqrt(np.sum(np.abs(h) ** 2, axis=1, keepdims=True))
    return h.astype(np.complex64).astype(np.complex128)


def convolve(x, h):
    """d[c, m, k] = sum_q h[c, q, k] x[c, m - q, k] in complex128"""
    d = np.zeros(x.shape, np.complex128)
    for q in range(h.shape[1]):
        d[:, q:] += h[:, q][:, None, :] * x[:, :x.shape[1] - q].astype(np.complex128)
    return d


def case(oracle, taps, bins, frames, channels):
    """(x, d, h): x, d [channels, frames, bins] complex64, h [channels, taps, bins]; d = h * x rounded to float32, then the two
    zero bins of channel 0"""
    def make():
        x = gaussian(oracle, channels, frames, bins, seed=101 + 7 * taps + bins).copy()
        h = responses(channels, taps, bins, seed=taps + 1000 * bins)
        d = convolve(x, h).astype(np.complex64)
        assert bins > ZERO_X
        x[0, :, ZERO_BOTH] = 0
        d[0, :, ZERO_BOTH] = 0
        x[0, :, ZERO_X] = 0
        assert np.all(d[0, :, ZERO_X] != 0)
        for a in (x, d, h):
            a.setflags(write=False)
        return x, d, h
    return cached(("bands case", taps, bins, frames, channels), make)


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """llz_adapt_bands_mc from the definition.  prec: 64 (the reference) or 32 (float32 components, complex64 products).  fault:
    None or one of FAULTS, for the tests that show the limits are not slack."""

    def __init__(self, channels, bins, taps, mu=MU, delta=DELTA, prec=64, fault=None):
        assert fault is None or fault in FAULTS
        self.rt, self.ct = (np.float32, np.complex64) if prec == 32 else (np.float64, np.complex128)
        self.channels, self.bins, self.taps, self.fault = channels, bins, taps, fault
        self.live = ceiling(taps) if fault == "ceiling_taps_live" else taps          # the taps that filter and update
        self.delta = self.rt(delta)
        self.mu = np.full(channels, mu, self.rt)
        self.W = np.zeros((channels, self.live, bins), self.ct)
        self.reset(False)

    def reset(self, clear_taps=False):
        self.X = np.zeros((self.channels, self.live + 1, self.bins), self.ct)        # X[:, q] = x[m - q]; one more for the late fault
        self.count = 0
        if clear_taps:
            self.W[:] = 0

    def set_step(self, first, mu):
        mu = np.atleast_1d(np.asarray(mu, self.rt))
        self.mu[first:first + len(mu)] = mu

    def set_taps(self, first, w):
        w = np.asarray(w, np.complex64)
        w = w[None] if w.ndim == 2 else w
        self.W[first:first + w.shape[0], :self.taps] = w

    def get_taps(self):
        return self.W[:, :self.taps].astype(np.complex64)

    def frames(self):
        return self.count

    def process(self, x, d):
        """x, d complex [channels, frames, bins] -> (e, y) in the model's precision"""
        ct, rt, K = self.ct, self.rt, self.live
        x, d = np.asarray(x).astype(ct), np.asarray(d).astype(ct)
        e, y = np.empty(x.shape, ct), np.empty(x.shape, ct)
        on = self.mu != 0
        mu = self.mu[:, None]
        for m in range(x.shape[1]):
            self.X[:, 1:] = self.X[:, :-1].copy()
            self.X[:, 0] = x[:, m]
            X = self.X[:, :K]
            ym = np.zeros((self.channels, self.bins), ct)
            for q in range(K):                                  # q ascending
                ym = (ym + self.W[:, q] * X[:, q]).astype(ct)
            em = (d[:, m] - ym).astype(ct)
            y[:, m], e[:, m] = ym, em
            if on.any():
                span = X[:, :1] if self.fault == "newest_power_only" else X
                p = np.zeros((self.channels, self.bins), rt)
                for q in range(span.shape[1]):
                    p = (p + (span[:, q].real ** 2 + span[:, q].imag ** 2).astype(rt)).astype(rt)
                den = (p + self.delta).astype(rt)
                g = ((mu * em.real).astype(rt) / den + 1j * ((mu * em.imag).astype(rt) / den)).astype(ct)
                Xu = self.X[:, 1:K + 1] if self.fault == "one_frame_late" else X
                Xu = Xu if self.fault == "not_conjugated" else np.conj(Xu)
                self.W[on] = (self.W[on] + g[on][:, None, :] * Xu[on]).astype(ct)
        self.count += x.shape[1]
        return e, y

    def close(self):
        pass


def model32(channels, bins, taps, mu=MU, delta=DELTA):
    """the device's stand-in: the float32 model behind the runners' interface"""
    return Model(channels, bins, taps, mu, delta, prec=32)


def definition_loops(x, d, taps, mu, delta):
    """one (channel, bin) stream from the definition written out as plain loops over Python complex numbers: (e, y, w)"""
    w = [0j] * taps
    e, y = [], []
    hist = lambda m, q: complex(x[m - q]) if m - q >= 0 else 0j          # noqa: E731
    for m in range(len(x)):
        ym = sum(w[q] * hist(m, q) for q in range(taps))
        em = complex(d[m]) - ym
        if mu != 0:
            p = sum(abs(hist(m, q)) ** 2 for q in range(taps))
            g = mu * em / (p + delta)
            for q in range(taps):
                w[q] += g * hist(m, q).conjugate()
        e.append(em)
        y.append(ym)
    return np.array(e), np.array(y), np.array(w)


# ------------------------------------------------------------------------------------------------ the device
def split(z):
    """complex [...] -> (re, im) float32, contiguous"""
    z = np.asarray(z)
    return np.ascontiguousarray(z.real, dtype=np.float32), np.ascontiguousarray(z.imag, dtype=np.float32)


class Device:
    """filters.AdaptBandsMC behind the model's interface: complex numpy in and out through device tensors, outputs preset to NaN.
    calls: how process() groups its frames into calls (None: all at once; a number: that many per call; a list: those counts in
    turn, repeated)"""

    def __init__(self, dev, channels, bins, taps, mu=MU, delta=DELTA, calls=None):
        from llzlab_amd import filters
        self.dev, self.channels, self.bins, self.taps, self.calls = dev, channels, bins, taps, calls
        self.f = filters.AdaptBandsMC(channels, bins, taps, mu=mu, delta=delta)
        plan = self.f.plan()
        assert plan == (ceiling(taps), plan[1], -(-channels * bins // plan[1]), 1) and plan[1] % 64 == 0, plan

    def sizes(self, frames):
        if self.calls is None:
            return [frames]
        steps = [self.calls] if isinstance(self.calls, int) else list(self.calls)
        out, k = [], 0
        while sum(out) < frames:
            out.append(min(steps[k % len(steps)], frames - sum(out)))
            k += 1
        return out

    def process(self, x, d, want_y=True):
        import torch
        up = lambda a: torch.from_numpy(a).to(self.dev)           # noqa: E731
        es, ys, o = [], [], 0
        for n in self.sizes(x.shape[1]):
            bufs = [up(a) for z in (x[:, o:o + n], d[:, o:o + n]) for a in split(z)]
            outs = [torch.full((self.channels, n, self.bins), float("nan"), dtype=torch.float32, device=self.dev)
                    for _ in range(4 if want_y else 2)]
            self.f.process(*bufs, *outs)
            got = [t.cpu().numpy() for t in outs]
            es.append(got[0] + 1j * got[1])
            ys.append(got[2] + 1j * got[3] if want_y else None)
            o += n
        e = np.concatenate(es, axis=1).astype(np.complex64)
        return e, (np.concatenate(ys, axis=1).astype(np.complex64) if want_y else None)

    def set_step(self, first, mu):
        self.f.set_step(first, mu)

    def set_taps(self, first, w):
        self.f.set_taps(first, w)

    def get_taps(self):
        return self.f.get_taps()

    def reset(self, clear_taps=False):
        self.f.reset(clear_taps)

    def frames(self):
        return self.f.frames()

    def close(self):
        self.f.close()


def device(dev, calls=None):
    return lambda *a, **kw: Device(dev, *a, calls=calls, **kw)


# ------------------------------------------------------------------------------------------------ the checks
def cbits(z):
    """the bits of a complex64 array's components"""
    return np.ascontiguousarray(z, dtype=np.complex64).view(np.uint32)


def run_power(a):
    """sum |a|^2 per (channel, run of RUN frames, bin) and the frames of each run; a: complex [channels, frames, bins]"""
    p = np.abs(np.asarray(a, np.complex128)) ** 2
    starts = np.arange(0, a.shape[1], RUN)
    return np.add.reduceat(p, starts, axis=1), np.diff(np.append(starts, a.shape[1]))


def run_rms(a):
    """[channels, runs, bins]"""
    s, n = run_power(a)
    return np.sqrt(s / n[None, :, None])


def ratio(err, lim):
    """the largest err / lim; inf where something is off at a limit of zero (an exact zero is asked for there) or is NaN"""
    err, lim = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(lim, np.float64))
    if not np.all(np.isfinite(err)):
        return float("inf")
    if np.any((lim == 0) & (err != 0)):
        return float("inf")
    ok = lim > 0
    return float(np.max(err[ok] / lim[ok])) if ok.any() else 0.0


def reference(oracle, taps, bins, frames, channels):
    """the float64 model over the whole case: (e, y, w, misalignment per (channel, bin)), computed once"""
    def make():
        x, d, h = case(oracle, taps, bins, frames, channels)
        m = Model(channels, bins, taps, prec=64)
        e, y = m.process(x, d)
        return e, y, m.W.copy(), np.sqrt(np.sum(np.abs(m.W - h) ** 2, axis=1))
    return cached(("bands ref", taps, bins, frames, channels), make)


def measure_parity(make, oracle, taps, bins, frames, channels):
    """one case through `make(channels, bins, taps, mu, delta)` against the float64 model: each figure as a ratio to its limit --
    'error' (per channel, bin and run, the worst), 'taps', 'misalignment' -- , 'converges' (the error falls wherever the model's
    does), and the zero bins and e = d - y checked on the way"""
    x, d, h = case(oracle, taps, bins, frames, channels)
    e_ref, _, w_ref, mis_ref = reference(oracle, taps, bins, frames, channels)
    what = f"bands K={taps} bins={bins} {channels}ch x {frames} frames"
    r = make(channels, bins, taps, MU, DELTA)
    e, y = r.process(x, d)
    w = r.get_taps()
    assert r.frames() == frames, f"{what}: frames() is {r.frames()}"
    r.close()
    assert e.shape == x.shape and y.shape == x.shape and w.shape == (channels, taps, bins)
    assert np.array_equal(cbits(e), cbits(d - y)), f"{what}: e is not the float32 difference d - y"
    assert not np.any(e[0, :, ZERO_BOTH]) and not np.any(y[0, :, ZERO_BOTH]) and not np.any(w[0, :, ZERO_BOTH]), \
        f"{what}: the bin with x = 0 and d = 0 is not exactly zero"
    assert np.array_equal(cbits(e[0, :, ZERO_X]), cbits(d[0, :, ZERO_X])) and not np.any(w[0, :, ZERO_X]), \
        f"{what}: the bin with x = 0 and d != 0 does not return d with zero weights"
    d_rms = np.sqrt(np.mean(np.abs(d.astype(np.complex128)) ** 2, axis=1))          # [channels, bins]
    err = run_rms(e.astype(np.complex128) - e_ref)
    error = ratio(err, TOL * np.broadcast_to(d_rms[:, None, :], err.shape))
    hn = np.sqrt(np.sum(np.abs(h) ** 2, axis=1))
    w64 = w.astype(np.complex128)
    tap = ratio(np.sqrt(np.sum(np.abs(w64 - w_ref[:, :taps]) ** 2, axis=1)), TOL * hn)
    mis = np.sqrt(np.sum(np.abs(w64 - h) ** 2, axis=1))
    mis_ratio = ratio(mis, np.maximum(2.0 * mis_ref, mis_ref + TOL * hn))
    runs, runs_ref = run_rms(e), run_rms(e_ref)
    conv = runs_ref[:, -1] < 0.1 * runs_ref[:, 0]
    out = {"error": error, "taps": tap, "misalignment": mis_ratio,
           "converges": bool(np.all(runs[:, -1][conv] < 0.1 * runs[:, 0][conv]))}
    print(f"{what}: worst error ratio {error:.3g} of the gate; taps {tap:.3g} of theirs; misalignment {np.max(mis[hn > 0]):.3g} "
          f"(model {mis_ref.max():.3g}), {mis_ratio:.3g} of its limit; {int(conv.sum())} of {conv.size} (channel, bin) held to a "
          f"tenth")
    return out


def check_parity(make, oracle, taps, bins, frames, channels):
    what = f"bands K={taps} bins={bins} {channels}ch"
    m = measure_parity(make, oracle, taps, bins, frames, channels)
    assert m["error"] <= 1.0, f"{what}: error at {m['error']:.3g} of the gate"
    assert m["taps"] <= 1.0, f"{what}: taps at {m['taps']:.3g} of their limit"
    assert m["misalignment"] <= 1.0, f"{what}: misalignment at {m['misalignment']:.3g} of its limit"
    assert m["converges"], f"{what}: the error does not fall where the model's does"
    return m


def worst_miss(make, oracle, taps, bins, frames, channels):
    """the largest ratio of a figure to its limit (a run that ends in NaN or inf misses by inf)"""
    with np.errstate(all="ignore"):
        m = measure_parity(make, oracle, taps, bins, frames, channels)
    return max(m["error"], m["taps"], m["misalignment"])


# ------------------------------------------------------------------------------------------------ end to end
# an oversampled bank of modest size; the response starts LEAD samples in, so that what the bank's prototype smears in front of
# it still falls on causal band taps, and E2E_TAPS frames cover lead, response and the prototype's length at the band rate
E2E = dict(channels=3, M=64, P=4, os=4, frames=1600, taps=16, lead=48, length=64)


def e2e_case(oracle):
    """(x, d, w): x, d [channels, frames hop] float32, d = x * h with h a decaying response behind a lead-in; w the prototype"""
    def make():
        from llzlab_amd import filters
        c, M, P, os, frames = (E2E[k] for k in ("channels", "M", "P", "os", "frames"))
        n = frames * (M // os)
        x = ac.gaussian(oracle, c, n, seed=4242)
        rng = np.random.default_rng(77)
        h = np.zeros((c, E2E["lead"] + E2E["length"]))
        h[:, E2E["lead"]:] = rng.standard_normal((c, E2E["length"])) * np.exp(-np.arange(E2E["length"]) / 12.0)
        h /= np.sqrt(np.sum(h * h, axis=1, keepdims=True))
        d = np.stack([np.convolve(x[k].astype(np.float64), h[k])[:n] for k in range(c)]).astype(np.float32)
        w = filters.pfb_prototype(M, P)
        for a in (d, w):
            a.setflags(write=False)
        return x, d, w
    return cached(("bands e2e",), make)


def e2e_residual(e_time, d_time):
    """per channel: rms of the last quarter of the synthesised residual over that of the synthesised d"""
    q = e_time.shape[1] // 4
    return ac.rms(e_time[:, -q:], axis=1) / ac.rms(d_time[:, -q:], axis=1)


def e2e_float64(oracle):
    """the float64 chain: pfb_checks' float64 bank in TIME phase, the float64 model, the float64 synthesis of e and of d;
    returns the residual ratios per channel"""
    def make():
        from tests import pfb_checks as pc
        x, d, w = e2e_case(oracle)
        c, M, P, os = (E2E[k] for k in ("channels", "M", "P", "os"))
        X, _ = pc.analysis(x, w, M, P, os, pc.TIME)
        D, _ = pc.analysis(d, w, M, P, os, pc.TIME)
        X, D = X.astype(np.complex64), D.astype(np.complex64)
        m = Model(c, M // 2 + 1, E2E["taps"], delta=e2e_delta(X), prec=64)
        e, _ = m.process(X, D)
        et, _ = pc.synthesis(*split(e), w, M, P, os, pc.TIME)
        dt, _ = pc.synthesis(*split(D), w, M, P, os, pc.TIME)
        return e2e_residual(et, dt)
    return cached(("bands e2e f64",), make)


def e2e_delta(X):
    """the regularisation for bands that are not of unit variance: 1e-3 x taps x the mean band power"""
    return float(1e-3 * E2E["taps"] * np.mean(np.abs(X) ** 2))
