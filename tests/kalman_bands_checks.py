"""Shared pieces of the per-band Kalman filter's tests (test_kalman_bands_host.py, test_kalman_bands_gpu.py; llz_kalman_bands_mc,
include/llz_kalman_bands.h): the MODEL of the definition in float64 (the reference everywhere) and in float32 / complex64 (the
device's stand-in on a machine without a GPU), the device runner, the checks, the double-talk case and the end-to-end case.  The
model is written from the definition in llz_kalman_bands.h in plain numpy and knows nothing of the kernel.  The case generator,
the zero bins, the gates of e and w and the helpers are adapt_bands_checks', imported.

The definition, per (channel, bin): weights w_q = 0, history x[m - q] = 0, variances P_q = p0, noise power psi = 0 at init; the
float32 constants A2 = a a, omA2 = 1 - A2, oml = 1 - lam (the float64 model takes these float32 VALUES).  For frame m:
y = sum_{q < K} w_q x[m - q]; e = d[m] - y; where the channel adapts: psi <- lam psi + oml |e|^2; u_q = P_q |x[m - q]|^2;
s = psi + delta + sum_q u_q; r = 1 / s; w_q += (e r) P_q conj(x[m - q]); c_q = max(1 - u_q r, 0); P_q <- A2 c_q P_q + omA2 |w_q|^2
with the new w_q.

Limits (none of them taken from the device's results), TOL = 1e-5:
  * e: adapt_bands_checks' gate -- per (channel, bin, run of 16 frames) rms(e - e_ref) <= TOL rms(d of that channel and bin);
  * w: adapt_bands_checks' gate -- per (channel, bin) |w - w_ref|_2 <= TOL |h|_2;
  * P: per element |P - P_ref| <= TOL P_ref;
  * psi: per (channel, bin) |psi - psi_ref| <= TOL mean |d|^2 of that bin;
  * the zero bins of channel 0: x = 0 and d = 0 gives e, y, w exactly zero and P = the recursion with u = 0, which is P <- A2 P
    in float32, bit for bit; x = 0 and d != 0 gives e bit-equal to d and w zero;
  * e bit-equal to float32(d) - y everywhere.
The float32 model sits below a quarter of the four limits on every case; the planted faults miss them.

The cases are not adapt_bands_checks' Gaussian bands, because of P's limit.  c_q = 1 - u_q r is a difference of nearly equal
numbers wherever one u_q carries s -- in the first frames, when P = p0 is far above delta and the history is still empty -- and
its rounding error of 2^-24 is then a relative error of 2^-24 / c_q in P_q, which the recursion forgets only at the rate A2.  With
Gaussian x and an abrupt start c_q falls to 1e-4 in some bin of a few thousand, and float32 arithmetic of any form is off by 1e-4
in that P_q: the float32 model reached 1.9 of P's limit.  A reference of constant modulus that fades in from 0.1 over 6 frames
(FADE) keeps every c_q above about 0.1, and the float32 model at 0.17 of the limit at the most; d = h * x stays free of noise."""
import numpy as np

from tests import adapt_bands_checks as bc

TOL = bc.TOL
A, LAM, P0, DELTA = 0.999, 0.9, 1.0, 1e-3
CEILINGS = (4, 8, 16, 32)
# (taps, bins, frames): one tap; a full and a just exceeded ceiling of 4; a full and a just exceeded ceiling of 16; the full
# ceiling of 32.  Bins of 5 and 33 put several channels into one wave, 129 and 65 straddle rows
SHAPES = [(1, 5, 200), (4, 33, 200), (5, 33, 200), (16, 129, 300), (17, 65, 300), (32, 65, 400)]
CHANNELS = (3, 37)
LONG = (8, 2049, 64, 3)         # taps, bins, frames, channels: a row longer than any workgroup
ZERO_BOTH, ZERO_X = bc.ZERO_BOTH, bc.ZERO_X
FAULTS = ("variance_from_old_weights", "newest_u_only", "noise_left_out", "ceiling_taps_live", "not_conjugated")
cached, cbits, split, ratio = bc.cached, bc.cbits, bc.split, bc.ratio


def ceiling(taps):
    return next(c for c in CEILINGS if taps <= c)


def constants(a, lam):
    """(A2, omA2, lam, oml) as the host layer forms them: float32 operations on float32 values"""
    a, lam, one = np.float32(a), np.float32(lam), np.float32(1)
    A2 = np.float32(a * a)
    return A2, np.float32(one - A2), lam, np.float32(one - lam)


# ------------------------------------------------------------------------------------------------ the cases
def FADE(m):
    """the modulus of x in frame m"""
    return np.minimum(1.0, 0.1 * 1.5 ** np.asarray(m, np.float64))


def case(oracle, taps, bins, frames, channels):
    """(x, d, h): x, d [channels, frames, bins] complex64, h [channels, taps, bins]; x = FADE(m) times the phase of the oracle
    generator's Gaussian, d = h * x rounded to float32, then the two zero bins of channel 0"""
    def make():
        z = bc.gaussian(oracle, channels, frames, bins, seed=101 + 7 * taps + bins).astype(np.complex128)
        x = (z / np.abs(z) * FADE(np.arange(frames))[None, :, None]).astype(np.complex64)
        h = bc.responses(channels, taps, bins, seed=taps + 1000 * bins)
        d = bc.convolve(x, h).astype(np.complex64)
        assert bins > ZERO_X
        x[0, :, ZERO_BOTH] = 0
        d[0, :, ZERO_BOTH] = 0
        x[0, :, ZERO_X] = 0
        assert np.all(d[0, :, ZERO_X] != 0)
        for a in (x, d, h):
            a.setflags(write=False)
        return x, d, h
    return cached(("kalman case", taps, bins, frames, channels), make)


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """llz_kalman_bands_mc from the definition.  prec: 64 (the reference) or 32 (float32 components, complex64 products).  fault:
    None or one of FAULTS, for the tests that show the limits are not slack."""

    def __init__(self, channels, bins, taps, a=A, lam=LAM, p0=P0, delta=DELTA, prec=64, fault=None):
        assert fault is None or fault in FAULTS
        self.rt, self.ct = (np.float32, np.complex64) if prec == 32 else (np.float64, np.complex128)
        self.channels, self.bins, self.taps, self.fault = channels, bins, taps, fault
        self.live = ceiling(taps) if fault == "ceiling_taps_live" else taps          # the taps that filter and update
        self.A2, self.omA2, self.lam, self.oml = (self.rt(v) for v in constants(a, lam))
        self.p0, self.delta = self.rt(np.float32(p0)), self.rt(np.float32(delta))
        self.on = np.ones(channels, bool)
        self.W = np.zeros((channels, self.live, bins), self.ct)
        self.P = np.full((channels, self.live, bins), self.p0, self.rt)
        self.psi = np.zeros((channels, bins), self.rt)
        self.reset(False)

    def reset(self, clear=False):
        self.X = np.zeros((self.channels, self.live, self.bins), self.ct)            # X[:, q] = x[m - q]
        self.count = 0
        if clear:
            self.W[:] = 0
            self.P[:] = self.p0
            self.psi[:] = 0

    def set_adapt(self, first, on):
        on = np.atleast_1d(on) != 0
        self.on[first:first + len(on)] = on

    def set_taps(self, first, w):
        w = np.asarray(w, np.complex64)
        w = w[None] if w.ndim == 2 else w
        self.W[first:first + w.shape[0], :self.taps] = w

    def set_variance(self, first, p):
        p = np.asarray(p, np.float32)
        p = p[None] if p.ndim == 2 else p
        self.P[first:first + p.shape[0], :self.taps] = p

    def get_taps(self):
        return self.W[:, :self.taps].astype(np.complex64)

    def get_variance(self):
        return self.P[:, :self.taps].astype(np.float32)

    def get_noise(self):
        return self.psi.astype(np.float32)

    def frames(self):
        return self.count

    def process(self, x, d):
        """x, d complex [channels, frames, bins] -> (e, y) in the model's precision"""
        ct, rt, K, on = self.ct, self.rt, self.live, self.on
        x, d = np.asarray(x).astype(ct), np.asarray(d).astype(ct)
        e, y = np.empty(x.shape, ct), np.empty(x.shape, ct)
        sq = lambda z: (z.real * z.real + z.imag * z.imag).astype(rt)             # noqa: E731
        for m in range(x.shape[1]):
            self.X[:, 1:] = self.X[:, :-1].copy()
            self.X[:, 0] = x[:, m]
            X = self.X
            ym = np.zeros((self.channels, self.bins), ct)
            for q in range(K):                                  # q ascending
                ym = (ym + self.W[:, q] * X[:, q]).astype(ct)
            em = (d[:, m] - ym).astype(ct)
            y[:, m], e[:, m] = ym, em
            if not on.any():
                continue
            psi = (self.lam * self.psi + (self.oml * sq(em)).astype(rt)).astype(rt)
            u = (self.P * sq(X)).astype(rt)
            s = np.zeros_like(psi) + self.delta if self.fault == "noise_left_out" else (psi + self.delta).astype(rt)
            for q in range(1 if self.fault == "newest_u_only" else K):
                s = (s + u[:, q]).astype(rt)
            r = (rt(1) / s).astype(rt)
            g = (em.real * r + 1j * (em.imag * r)).astype(ct)
            k = (g.real[:, None] * self.P + 1j * (g.imag[:, None] * self.P)).astype(ct)
            W = (self.W + k * (X if self.fault == "not_conjugated" else np.conj(X))).astype(ct)
            c = (rt(1) - (u * r[:, None]).astype(rt)).astype(rt)
            c = np.where(c < 0, rt(0), c)
            ww = sq(self.W if self.fault == "variance_from_old_weights" else W)
            P = (((self.A2 * c).astype(rt) * self.P).astype(rt) + (self.omA2 * ww).astype(rt)).astype(rt)
            self.W[on], self.P[on], self.psi[on] = W[on], P[on], psi[on]
        self.count += x.shape[1]
        return e, y

    def close(self):
        pass


def model32(channels, bins, taps, **kw):
    """the device's stand-in: the float32 model behind the runners' interface"""
    return Model(channels, bins, taps, prec=32, **kw)


def definition_loops(x, d, taps, a=A, lam=LAM, p0=P0, delta=DELTA):
    """one (channel, bin) stream from the definition written out as plain loops over Python numbers: (e, y, w, P, psi)"""
    A2, omA2, lam, oml = (float(v) for v in constants(a, lam))
    p0, delta = float(np.float32(p0)), float(np.float32(delta))
    w, P, psi = [0j] * taps, [p0] * taps, 0.0
    e, y = [], []
    hist = lambda m, q: complex(x[m - q]) if m - q >= 0 else 0j          # noqa: E731
    for m in range(len(x)):
        ym = sum(w[q] * hist(m, q) for q in range(taps))
        em = complex(d[m]) - ym
        psi = lam * psi + oml * abs(em) ** 2
        u = [P[q] * abs(hist(m, q)) ** 2 for q in range(taps)]
        s = psi + delta + sum(u)
        for q in range(taps):
            w[q] += (em / s) * P[q] * hist(m, q).conjugate()
            P[q] = A2 * max(1 - u[q] / s, 0.0) * P[q] + omA2 * abs(w[q]) ** 2
        e.append(em)
        y.append(ym)
    return np.array(e), np.array(y), np.array(w), np.array(P), psi


# ------------------------------------------------------------------------------------------------ the device
class Device(bc.Device):
    """filters.KalmanBandsMC behind the model's interface; process() and its grouping into calls are adapt_bands_checks.Device's"""

    def __init__(self, dev, channels, bins, taps, calls=None, **kw):
        from llzlab_amd import filters
        self.dev, self.channels, self.bins, self.taps, self.calls = dev, channels, bins, taps, calls
        self.f = filters.KalmanBandsMC(channels, bins, taps, **{**dict(a=A, lam=LAM, p0=P0, delta=DELTA), **kw})
        plan = self.f.plan()
        assert plan == (ceiling(taps), 64, -(-channels * bins // 64), 1), plan

    def set_adapt(self, first, on):
        self.f.set_adapt(first, on)

    def set_variance(self, first, p):
        self.f.set_variance(first, p)

    def get_variance(self):
        return self.f.get_variance()

    def get_noise(self):
        return self.f.get_noise()


def device(dev, calls=None):
    return lambda *a, **kw: Device(dev, *a, calls=calls, **kw)


# ------------------------------------------------------------------------------------------------ the checks
def reference(oracle, taps, bins, frames, channels):
    """the float64 model over the whole case: (e, y, w, P, psi), computed once"""
    def make():
        x, d, _ = case(oracle, taps, bins, frames, channels)
        m = Model(channels, bins, taps, prec=64)
        e, y = m.process(x, d)
        return e, y, m.W.copy(), m.P.copy(), m.psi.copy()
    return cached(("kalman ref", taps, bins, frames, channels), make)


def idle_variance(frames, a=A, p0=P0):
    """P of a bin whose x is zero throughout: P <- A2 P in float32, `frames` times"""
    A2, p = constants(a, LAM)[0], np.float32(p0)
    for _ in range(frames):
        p = np.float32(A2 * p)
    return p


def measure_parity(make, oracle, taps, bins, frames, channels):
    """one case through `make(channels, bins, taps)` against the float64 model: 'error', 'taps', 'variance' and 'noise' as ratios
    to their limits (the worst over the case), the zero bins and e = d - y checked on the way"""
    x, d, h = case(oracle, taps, bins, frames, channels)
    e_ref, y_ref, w_ref, p_ref, psi_ref = reference(oracle, taps, bins, frames, channels)
    what = f"kalman K={taps} bins={bins} {channels}ch x {frames} frames"
    r = make(channels, bins, taps)
    e, y = r.process(x, d)
    w, p, psi = r.get_taps(), r.get_variance(), r.get_noise()
    assert r.frames() == frames, f"{what}: frames() is {r.frames()}"
    r.close()
    assert e.shape == x.shape and y.shape == x.shape and w.shape == p.shape == (channels, taps, bins) and psi.shape == (channels, bins)
    assert np.array_equal(cbits(e), cbits(d - y)), f"{what}: e is not the float32 difference d - y"
    idle = idle_variance(frames)
    assert not np.any(e[0, :, ZERO_BOTH]) and not np.any(y[0, :, ZERO_BOTH]) and not np.any(w[0, :, ZERO_BOTH]) and \
        psi[0, ZERO_BOTH] == 0, f"{what}: the bin with x = 0 and d = 0 is not exactly zero"
    assert np.all(p[0, :, ZERO_BOTH].view(np.uint32) == idle.view(np.uint32)) and np.all(p[0, :, ZERO_X] == idle), \
        f"{what}: P of a bin with x = 0 is not p0 under P <- A2 P ({p[0, :, ZERO_BOTH]}, {idle})"
    assert np.array_equal(cbits(e[0, :, ZERO_X]), cbits(d[0, :, ZERO_X])) and not np.any(w[0, :, ZERO_X]), \
        f"{what}: the bin with x = 0 and d != 0 does not return d with zero weights"
    d_pow = np.mean(np.abs(d.astype(np.complex128)) ** 2, axis=1)                   # [channels, bins]
    err = bc.run_rms(e.astype(np.complex128) - e_ref)
    y_err = bc.run_rms(y.astype(np.complex128) - y_ref)
    gate = TOL * np.broadcast_to(np.sqrt(d_pow)[:, None, :], err.shape)
    hn = np.sqrt(np.sum(np.abs(h) ** 2, axis=1))
    out = {"error": max(ratio(err, gate), ratio(y_err, gate)),
           "taps": ratio(np.sqrt(np.sum(np.abs(w.astype(np.complex128) - w_ref[:, :taps]) ** 2, axis=1)), TOL * hn),
           "variance": ratio(np.abs(p.astype(np.float64) - p_ref[:, :taps]), TOL * p_ref[:, :taps]),
           "noise": ratio(np.abs(psi.astype(np.float64) - psi_ref), TOL * d_pow)}
    print(f"{what}: worst ratios to the limits: e {out['error']:.3g}, w {out['taps']:.3g}, P {out['variance']:.3g}, "
          f"psi {out['noise']:.3g}")
    return out


def check_parity(make, oracle, taps, bins, frames, channels, share=1.0):
    """every figure within `share` of its limit (the float32 model is asked for a quarter)"""
    m = measure_parity(make, oracle, taps, bins, frames, channels)
    for name, v in m.items():
        assert v <= share, f"kalman K={taps} bins={bins} {channels}ch: {name} at {v:.3g} of its limit (asked: {share})"
    return m


def worst_miss(make, oracle, taps, bins, frames, channels):
    """the largest ratio of a figure to its limit (a run that ends in NaN or inf, or breaks an exact check, misses by inf)"""
    with np.errstate(all="ignore"):
        try:
            return max(measure_parity(make, oracle, taps, bins, frames, channels).values())
        except AssertionError:
            return float("inf")


# ------------------------------------------------------------------------------------------------ double-talk
# one channel of unit-variance bands, an echo path of unit norm, background noise 40 dB below the echo, and a near-end burst
# 10 dB above it over frames BURST: the misalignment |w - h|_2 per bin is read behind the frames MARKS
DT = dict(taps=8, bins=33, frames=900, burst=(500, 600), noise=1e-2, level=np.sqrt(10.0))
DT_MARKS = (499, 599, 899)      # the last frame before the burst, the burst's last frame, the last frame of the case


def dt_case():
    """(x, d, h): x, d [1, frames, bins] complex64, h [1, taps, bins]"""
    def make():
        K, B, F = DT["taps"], DT["bins"], DT["frames"]
        rng = np.random.default_rng(20061)
        x = ((rng.standard_normal((1, F, B)) + 1j * rng.standard_normal((1, F, B))) * np.sqrt(0.5)).astype(np.complex64)
        h = bc.responses(1, K, B, seed=20062)
        n = (rng.standard_normal((1, F, B)) + 1j * rng.standard_normal((1, F, B))) * np.sqrt(0.5)
        d = bc.convolve(x, h) + DT["noise"] * n
        lo, hi = DT["burst"]
        d[:, lo:hi] += DT["level"] * n[:, lo:hi]
        d = d.astype(np.complex64)
        for a in (x, d, h):
            a.setflags(write=False)
        return x, d, h
    return cached(("kalman dt case",), make)


def dt_misalignment(r):
    """runner r (a model or a device, 1 channel) over the case: |w - h|_2 per bin behind each of DT_MARKS, [3, bins]"""
    x, d, h = dt_case()
    out, o = [], 0
    for mark in DT_MARKS:
        r.process(x[:, o:mark + 1], d[:, o:mark + 1])
        o = mark + 1
        out.append(np.sqrt(np.sum(np.abs(r.get_taps().astype(np.complex128) - h) ** 2, axis=1))[0])
    r.close()
    return np.array(out)


def dt_float64():
    """(the Kalman float64 model's misalignments, the NLMS float64 model's at mu = 0.5), [3, bins] each"""
    def make():
        K, B = DT["taps"], DT["bins"]
        return dt_misalignment(Model(1, B, K, prec=64)), dt_misalignment(bc.Model(1, B, K, mu=0.5, delta=DELTA, prec=64))
    return cached(("kalman dt f64",), make)


def dt_report(name, mis):
    return f"{name}: " + "; ".join(f"frame {m}: median {np.median(v):.3g} max {v.max():.3g} min {v.min():.3g}"
                                   for m, v in zip(DT_MARKS, mis))


# ------------------------------------------------------------------------------------------------ end to end
# adapt_bands_checks.E2E's bank and case, with a near-end burst of white noise at the echo's level added to d over E2E_BURST (in
# frames of the band rate); the residual is read over the last quarter, 200 frames behind the burst's end
E2E = bc.E2E
E2E_BURST = (800, 1000)


def e2e_case(oracle):
    """(x, d, w) of adapt_bands_checks.e2e_case with the burst added to d"""
    def make():
        x, d, w = bc.e2e_case(oracle)
        hop = E2E["M"] // E2E["os"]
        lo, hi = E2E_BURST[0] * hop, E2E_BURST[1] * hop
        d = d.copy()
        near = np.random.default_rng(4243).standard_normal((d.shape[0], hi - lo))
        d[:, lo:hi] += (near * bc.ac.rms(d, axis=1)[:, None]).astype(np.float32)
        d.setflags(write=False)
        return x, d, w
    return cached(("kalman e2e",), make)


def e2e_params(X):
    """p0 and delta for bands that are not of unit variance: the weights are of order 1, the powers of order mean |X|^2"""
    return dict(p0=1.0, delta=float(1e-3 * np.mean(np.abs(X) ** 2)))


def e2e_float64(oracle):
    """the float64 chain: pfb_checks' float64 bank in TIME phase, the float64 model, the float64 synthesis of e and of d;
    returns the residual ratios per channel (adapt_bands_checks.e2e_residual: the last quarter)"""
    def make():
        from tests import pfb_checks as pc
        x, d, w = e2e_case(oracle)
        c, M, P, os = (E2E[k] for k in ("channels", "M", "P", "os"))
        X, _ = pc.analysis(x, w, M, P, os, pc.TIME)
        D, _ = pc.analysis(d, w, M, P, os, pc.TIME)
        X, D = X.astype(np.complex64), D.astype(np.complex64)
        m = Model(c, M // 2 + 1, E2E["taps"], prec=64, **e2e_params(X))
        e, _ = m.process(X, D)
        et, _ = pc.synthesis(*split(e), w, M, P, os, pc.TIME)
        dt, _ = pc.synthesis(*split(D), w, M, P, os, pc.TIME)
        return bc.e2e_residual(et, dt)
    return cached(("kalman e2e f64",), make)
