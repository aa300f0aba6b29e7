"""Shared pieces of the multi-reference per-band Kalman filter's tests (test_kalman_bands_matrix_host.py,
test_kalman_bands_matrix_gpu.py; llz_kalman_bands_matrix_mc, include/llz_kalman_bands_matrix.h): the MODEL of the definition in
float64 (the reference everywhere) and in float32 / complex64 (the device's stand-in on a machine without a GPU), the case
generator, the device runner, the checks, the double-talk case and the end-to-end case.  The model is written from the definition
in the header in plain numpy and knows nothing of the kernel: one shift register of frames per (input, bin), shared by the
outputs; no entry ceiling, no lanes, no second history buffer.

The definition, per (output o, bin k): weights w_{i,q} = 0, variances P_{i,q} = p0, one noise power psi = 0 at init; per (input i,
bin k) a history x_i[m - q], zero before frame 0; the float32 constants A2 = a a, omA2 = 1 - A2, oml = 1 - lam (the float64 model
takes these float32 VALUES).  For frame m: y = sum_q sum_i w_{i,q} x_i[m - q]; e = d[m] - y; where the output adapts:
psi <- lam psi + oml |e|^2; u_{i,q} = P_{i,q} |x_i[m - q]|^2; s = psi + delta + sum_q sum_i u_{i,q}; r = 1 / s;
w_{i,q} += (e r) P_{i,q} conj(x_i[m - q]); c_{i,q} = max(1 - u_{i,q} r, 0); P_{i,q} <- A2 c_{i,q} P_{i,q} + omA2 |w_{i,q}|^2 with
the new w.  Every sum runs q ascending and, within a q, i ascending.

Limits (kalman_bands_checks.py's, none of them taken from the device's results), TOL = 1e-5:
  * e and y: per (output, bin, run of 16 frames) rms(e - e_ref) <= TOL rms(d of that output and bin);
  * w: per (output, bin) |w - w_ref|_2 over all (i, q) <= TOL |h|_2;
  * P: per element |P - P_ref| <= TOL P_ref;
  * psi: per (output, bin) |psi - psi_ref| <= TOL mean |d|^2 of that output and bin;
  * the zero bins, where EVERY reference is zero, on output 0: d = 0 as well gives e, y, w, psi exactly zero and P <- A2 P in
    float32, bit for bit; d != 0 gives e bit-equal to d, w zero and the same P;
  * e bit-equal to float32(d) - y everywhere.
A shape is a GPU case only while the float32 model stays below a QUARTER of the four limits on the CPU
(test_kalman_bands_matrix_host.py asserts it); the planted faults of that file miss them.

The cases are kalman_bands_checks' kind, for the reason its docstring gives: c = 1 - u r is a difference of nearly equal numbers
wherever one u carries s, and its rounding error then stays in P for long.  Every reference has a constant modulus that fades
in by FADE(m), with phases that are independent per input, from the oracle's generator; d = sum_i h_{o,i} * x_i without noise,
h of unit norm per (output, bin)."""
import numpy as np

from tests import adapt_bands_checks as bc
from tests import adapt_bands_matrix_checks as mc
from tests import kalman_bands_checks as kc

TOL = kc.TOL
A, LAM, P0, DELTA = kc.A, kc.LAM, kc.P0, kc.DELTA
FADE, constants, idle_variance = kc.FADE, kc.constants, kc.idle_variance
CEILINGS = (8, 16, 32)
# (inputs, outputs, taps, bins, frames): one input; a full ceiling of 8; 9 entries, just past it; full ceilings of 32 by taps and
# by inputs; 30 entries with an input count that divides no ceiling; 8 inputs of one tap (no history at all) on 37 outputs of 5
# bins (a dozen outputs in a wave)
SHAPES = [(1, 3, 5, 33, 200), (2, 2, 4, 33, 200), (3, 2, 3, 33, 200), (2, 3, 16, 65, 300), (8, 2, 4, 33, 300),
          (5, 2, 6, 33, 300), (8, 37, 1, 5, 200)]
LONG = (2, 1, 4, 2049, 64)      # a row longer than any workgroup
OUTPUTS = (2, 37)               # every shape is also run at these output counts (the float32 model; the isolation test)
FAULT_SHAPE = SHAPES[2]
FAULTS = ("first_reference_s", "state_transposed", "one_input_late", "variance_from_old_weights", "noise_left_out")
ZERO_BOTH, ZERO_X = kc.ZERO_BOTH, kc.ZERO_X
cached, cbits, split, ratio, run_rms, gaussian = bc.cached, bc.cbits, bc.split, bc.ratio, bc.run_rms, bc.gaussian
responses, convolve = mc.responses, mc.convolve


def ceiling(inputs, taps):
    return next(c for c in CEILINGS if inputs * taps <= c)


# ------------------------------------------------------------------------------------------------ the cases
def case(oracle, inputs, outputs, taps, bins, frames):
    """(x, d, h): x [inputs, frames, bins], d [outputs, frames, bins] complex64, h [outputs, inputs, taps, bins]; x_i = FADE(m)
    times the phase of the oracle generator's Gaussian, d = sum_i h_{o,i} * x_i rounded to float32, then the two zero bins: every
    reference zero there, and output 0's d as well in the first"""
    def make():
        z = gaussian(oracle, inputs, frames, bins, seed=311 + 7 * taps + bins + 31 * inputs).astype(np.complex128)
        x = (z / np.abs(z) * FADE(np.arange(frames))[None, :, None]).astype(np.complex64)
        h = responses(outputs, inputs, taps, bins, seed=taps + 1000 * bins + 17 * inputs + outputs)
        d = convolve(x, h).astype(np.complex64)
        assert bins > ZERO_X
        x[:, :, ZERO_BOTH] = 0
        d[0, :, ZERO_BOTH] = 0
        x[:, :, ZERO_X] = 0
        assert np.all(d[0, :, ZERO_X] != 0)
        for a in (x, d, h):
            a.setflags(write=False)
        return x, d, h
    return cached(("kalman matrix case", inputs, outputs, taps, bins, frames), make)


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """llz_kalman_bands_matrix_mc from the definition.  prec: 64 (the reference) or 32 (float32 components, complex64 products, in
    kalman_bands_checks.Model's expressions, so that one input gives that model's bits).  fault: None or one of FAULTS, for the
    tests that show the limits are not slack."""

    def __init__(self, inputs, outputs, bins, taps, a=A, lam=LAM, p0=P0, delta=DELTA, prec=64, fault=None):
        assert fault is None or fault in FAULTS
        self.rt, self.ct = (np.float32, np.complex64) if prec == 32 else (np.float64, np.complex128)
        self.inputs, self.outputs, self.bins, self.taps, self.fault = inputs, outputs, bins, taps, fault
        self.A2, self.omA2, self.lam, self.oml = (self.rt(v) for v in constants(a, lam))
        self.p0, self.delta = self.rt(np.float32(p0)), self.rt(np.float32(delta))
        self.on = np.ones(outputs, bool)
        self.W = np.zeros((outputs, inputs, taps, bins), self.ct)
        self.P = np.full((outputs, inputs, taps, bins), self.p0, self.rt)
        self.psi = np.zeros((outputs, bins), self.rt)
        self.reset(False)

    def reset(self, clear=False):
        self.X = np.zeros((self.inputs, self.taps + 1, self.bins), self.ct)          # X[i, q] = x_i[m - q]; one more for the late fault
        self.count = 0
        if clear:
            self.W[:] = 0
            self.P[:] = self.p0
            self.psi[:] = 0

    def set_adapt(self, first, on):
        on = np.atleast_1d(on) != 0
        self.on[first:first + len(on)] = on

    def set_taps(self, out_first, w, in_first=0):
        w = np.asarray(w, np.complex64)
        self.W[out_first:out_first + w.shape[0], in_first:in_first + w.shape[1]] = w

    def set_variance(self, out_first, p, in_first=0):
        p = np.asarray(p, np.float32)
        self.P[out_first:out_first + p.shape[0], in_first:in_first + p.shape[1]] = p

    def _laid_out(self, a):
        if self.fault == "state_transposed":        # the memory that set_* / get_* lay out [i][q], walked as [q][i]
            return np.ascontiguousarray(a.transpose(0, 2, 1, 3).reshape(a.shape))
        return a

    def get_taps(self):
        return self._laid_out(self.W).astype(np.complex64)

    def get_variance(self):
        return self._laid_out(self.P).astype(np.float32)

    def get_noise(self):
        return self.psi.astype(np.float32)

    def frames(self):
        return self.count

    def process(self, x, d):
        """x complex [inputs, frames, bins], d complex [outputs, frames, bins] -> (e, y) in the model's precision"""
        ct, rt, K, I, on = self.ct, self.rt, self.taps, self.inputs, self.on
        x, d = np.asarray(x).astype(ct), np.asarray(d).astype(ct)
        e, y = np.empty(d.shape, ct), np.empty(d.shape, ct)
        sq = lambda z: (z.real * z.real + z.imag * z.imag).astype(rt)             # noqa: E731
        for m in range(x.shape[1]):
            self.X[:, 1:] = self.X[:, :-1].copy()
            self.X[:, 0] = x[:, m]
            X = self.X[:, :K]
            if self.fault == "one_input_late":
                X = X.copy()
                X[I - 1] = self.X[I - 1, 1:K + 1]
            ym = np.zeros((self.outputs, self.bins), ct)
            for q in range(K):                                  # q ascending, within a q i ascending
                for i in range(I):
                    ym = (ym + self.W[:, i, q] * X[i, q][None]).astype(ct)
            em = (d[:, m] - ym).astype(ct)
            y[:, m], e[:, m] = ym, em
            if not on.any():
                continue
            psi = (self.lam * self.psi + (self.oml * sq(em)).astype(rt)).astype(rt)
            u = (self.P * sq(X)[None]).astype(rt)
            s = np.zeros_like(psi) + self.delta if self.fault == "noise_left_out" else (psi + self.delta).astype(rt)
            for q in range(K):
                for i in range(1 if self.fault == "first_reference_s" else I):
                    s = (s + u[:, i, q]).astype(rt)
            r = (rt(1) / s).astype(rt)
            g = (em.real * r + 1j * (em.imag * r)).astype(ct)
            k = (g.real[:, None, None] * self.P + 1j * (g.imag[:, None, None] * self.P)).astype(ct)
            W = (self.W + k * np.conj(X)[None]).astype(ct)
            c = (rt(1) - (u * r[:, None, None]).astype(rt)).astype(rt)
            c = np.where(c < 0, rt(0), c)
            ww = sq(self.W if self.fault == "variance_from_old_weights" else W)
            P = (((self.A2 * c).astype(rt) * self.P).astype(rt) + (self.omA2 * ww).astype(rt)).astype(rt)
            self.W[on], self.P[on], self.psi[on] = W[on], P[on], psi[on]
        self.count += x.shape[1]
        return e, y

    def close(self):
        pass


def model32(inputs, outputs, bins, taps, **kw):
    """the device's stand-in: the float32 model behind the runners' interface"""
    return Model(inputs, outputs, bins, taps, prec=32, **kw)


def definition_loops(x, d, taps, a=A, lam=LAM, p0=P0, delta=DELTA):
    """one (output, bin) stream from the definition written out as plain loops over Python numbers; x [inputs, frames], d
    [frames]: (e, y, w [inputs, taps], P [inputs, taps], psi)"""
    A2, omA2, lam, oml = (float(v) for v in constants(a, lam))
    p0, delta = float(np.float32(p0)), float(np.float32(delta))
    inputs = len(x)
    w = [[0j] * taps for _ in range(inputs)]
    P = [[p0] * taps for _ in range(inputs)]
    psi = 0.0
    e, y = [], []
    hist = lambda i, m, q: complex(x[i][m - q]) if m - q >= 0 else 0j          # noqa: E731
    for m in range(len(d)):
        ym = sum(w[i][q] * hist(i, m, q) for q in range(taps) for i in range(inputs))
        em = complex(d[m]) - ym
        psi = lam * psi + oml * abs(em) ** 2
        u = [[P[i][q] * abs(hist(i, m, q)) ** 2 for q in range(taps)] for i in range(inputs)]
        s = psi + delta + sum(u[i][q] for q in range(taps) for i in range(inputs))
        for i in range(inputs):
            for q in range(taps):
                w[i][q] += (em / s) * P[i][q] * hist(i, m, q).conjugate()
                P[i][q] = A2 * max(1 - u[i][q] / s, 0.0) * P[i][q] + omA2 * abs(w[i][q]) ** 2
        e.append(em)
        y.append(ym)
    return np.array(e), np.array(y), np.array(w), np.array(P), psi


# ------------------------------------------------------------------------------------------------ the device
class Device:
    """filters.KalmanBandsMatrixMC behind the model's interface; process() and its grouping into calls are
    adapt_bands_matrix_checks.Device's"""

    def __init__(self, dev, inputs, outputs, bins, taps, calls=None, **kw):
        from llzlab_amd import filters
        self.dev, self.inputs, self.outputs, self.bins, self.taps, self.calls = dev, inputs, outputs, bins, taps, calls
        self.f = filters.KalmanBandsMatrixMC(inputs, outputs, bins, taps, **{**dict(a=A, lam=LAM, p0=P0, delta=DELTA), **kw})
        plan = self.f.plan()
        assert plan == (inputs, ceiling(inputs, taps), 64, -(-outputs * bins // 64), 1), plan

    sizes = bc.Device.sizes
    process = mc.Device.process

    def set_adapt(self, first, on):
        self.f.set_adapt(first, on)

    def set_taps(self, out_first, w, in_first=0):
        self.f.set_taps(out_first, w, in_first)

    def set_variance(self, out_first, p, in_first=0):
        self.f.set_variance(out_first, p, in_first)

    def get_taps(self):
        return self.f.get_taps()

    def get_variance(self):
        return self.f.get_variance()

    def get_noise(self):
        return self.f.get_noise()

    def reset(self, clear=False):
        self.f.reset(clear)

    def frames(self):
        return self.f.frames()

    def close(self):
        self.f.close()


def device(dev, calls=None):
    return lambda *a, **kw: Device(dev, *a, calls=calls, **kw)


# ------------------------------------------------------------------------------------------------ the checks
def reference(oracle, inputs, outputs, taps, bins, frames):
    """the float64 model over the whole case: (e, y, w, P, psi), computed once"""
    def make():
        x, d, _ = case(oracle, inputs, outputs, taps, bins, frames)
        m = Model(inputs, outputs, bins, taps, prec=64)
        e, y = m.process(x, d)
        return e, y, m.W.copy(), m.P.copy(), m.psi.copy()
    return cached(("kalman matrix ref", inputs, outputs, taps, bins, frames), make)


def measure_parity(make, oracle, inputs, outputs, taps, bins, frames):
    """one case through `make(inputs, outputs, bins, taps)` against the float64 model: 'error', 'taps', 'variance' and 'noise' as
    ratios to their limits (the worst over the case), the zero bins and e = d - y checked on the way"""
    x, d, h = case(oracle, inputs, outputs, taps, bins, frames)
    e_ref, y_ref, w_ref, p_ref, psi_ref = reference(oracle, inputs, outputs, taps, bins, frames)
    what = f"kalman matrix I={inputs} O={outputs} K={taps} bins={bins} x {frames} frames"
    r = make(inputs, outputs, bins, taps)
    e, y = r.process(x, d)
    w, p, psi = r.get_taps(), r.get_variance(), r.get_noise()
    assert r.frames() == frames, f"{what}: frames() is {r.frames()}"
    r.close()
    assert e.shape == d.shape and y.shape == d.shape and w.shape == p.shape == (outputs, inputs, taps, bins) and \
        psi.shape == (outputs, bins)
    assert np.array_equal(cbits(e), cbits(d - y)), f"{what}: e is not the float32 difference d - y"
    idle = idle_variance(frames)
    assert not np.any(e[0, :, ZERO_BOTH]) and not np.any(y[0, :, ZERO_BOTH]) and not np.any(w[0, :, :, ZERO_BOTH]) and \
        psi[0, ZERO_BOTH] == 0, f"{what}: the bin with x = 0 and d = 0 is not exactly zero"
    assert np.all(p[0, :, :, ZERO_BOTH].view(np.uint32) == idle.view(np.uint32)) and np.all(p[0, :, :, ZERO_X] == idle), \
        f"{what}: P of a bin with x = 0 is not p0 under P <- A2 P ({p[0, :, :, ZERO_BOTH]}, {idle})"
    assert np.array_equal(cbits(e[0, :, ZERO_X]), cbits(d[0, :, ZERO_X])) and not np.any(w[0, :, :, ZERO_X]), \
        f"{what}: the bin with x = 0 and d != 0 does not return d with zero weights"
    d_pow = np.mean(np.abs(d.astype(np.complex128)) ** 2, axis=1)                   # [outputs, bins]
    err = run_rms(e.astype(np.complex128) - e_ref)
    y_err = run_rms(y.astype(np.complex128) - y_ref)
    gate = TOL * np.broadcast_to(np.sqrt(d_pow)[:, None, :], err.shape)
    hn = np.sqrt(np.sum(np.abs(h) ** 2, axis=(1, 2)))
    out = {"error": max(ratio(err, gate), ratio(y_err, gate)),
           "taps": ratio(np.sqrt(np.sum(np.abs(w.astype(np.complex128) - w_ref) ** 2, axis=(1, 2))), TOL * hn),
           "variance": ratio(np.abs(p.astype(np.float64) - p_ref), TOL * p_ref),
           "noise": ratio(np.abs(psi.astype(np.float64) - psi_ref), TOL * d_pow)}
    print(f"{what}: worst ratios to the limits: e {out['error']:.3g}, w {out['taps']:.3g}, P {out['variance']:.3g}, "
          f"psi {out['noise']:.3g}")
    return out


def check_parity(make, oracle, inputs, outputs, taps, bins, frames, share=1.0):
    """every figure within `share` of its limit (the float32 model is asked for a quarter)"""
    m = measure_parity(make, oracle, inputs, outputs, taps, bins, frames)
    for name, v in m.items():
        assert v <= share, f"kalman matrix I={inputs} O={outputs} K={taps} bins={bins}: {name} at {v:.3g} of its limit (asked: {share})"
    return m


def worst_miss(make, oracle, inputs, outputs, taps, bins, frames):
    """the largest ratio of a figure to its limit (a run that ends in NaN or inf, or breaks an exact check, misses by inf)"""
    with np.errstate(all="ignore"):
        try:
            return max(measure_parity(make, oracle, inputs, outputs, taps, bins, frames).values())
        except AssertionError:
            return float("inf")


# ------------------------------------------------------------------------------------------------ double-talk
# kalman_bands_checks.DT's shape with two references of four taps: one output of unit-variance bands, echo paths of unit norm
# over both, background noise 40 dB below the echo, and a near-end burst 10 dB above it over frames BURST; the misalignment
# |w - h|_2 over all (i, q) per bin is read behind the frames DT_MARKS
DT = dict(kc.DT, inputs=2, taps=4)
DT_MARKS = kc.DT_MARKS


def dt_case():
    """(x, d, h): x [inputs, frames, bins], d [1, frames, bins] complex64, h [1, inputs, taps, bins]"""
    def make():
        I, K, B, F = DT["inputs"], DT["taps"], DT["bins"], DT["frames"]
        rng = np.random.default_rng(20071)
        x = ((rng.standard_normal((I, F, B)) + 1j * rng.standard_normal((I, F, B))) * np.sqrt(0.5)).astype(np.complex64)
        h = responses(1, I, K, B, seed=20072)
        n = (rng.standard_normal((1, F, B)) + 1j * rng.standard_normal((1, F, B))) * np.sqrt(0.5)
        d = convolve(x, h) + DT["noise"] * n
        lo, hi = DT["burst"]
        d[:, lo:hi] += DT["level"] * n[:, lo:hi]
        d = d.astype(np.complex64)
        for a in (x, d, h):
            a.setflags(write=False)
        return x, d, h
    return cached(("kalman matrix dt case",), make)


def dt_misalignment(r):
    """runner r (a joint model or a device, 1 output) over the case: |w - h|_2 per bin behind each of DT_MARKS, [3, bins]"""
    x, d, h = dt_case()
    out, o = [], 0
    for mark in DT_MARKS:
        r.process(x[:, o:mark + 1], d[:, o:mark + 1])
        o = mark + 1
        out.append(np.sqrt(np.sum(np.abs(r.get_taps().astype(np.complex128) - h) ** 2, axis=(1, 2)))[0])
    r.close()
    return np.array(out)


def dt_singles():
    """a bank of single-reference Kalman float64 models, one per reference, each fed d: the same misalignment, [3, bins]"""
    x, d, h = dt_case()
    models = [kc.Model(1, DT["bins"], DT["taps"], prec=64) for _ in range(DT["inputs"])]
    out, o = [], 0
    for mark in DT_MARKS:
        for i, m in enumerate(models):
            m.process(x[i:i + 1, o:mark + 1], d[:, o:mark + 1])
        o = mark + 1
        w = np.stack([m.W[0] for m in models])                            # [inputs, taps, bins]
        out.append(np.sqrt(np.sum(np.abs(w - h[0]) ** 2, axis=(0, 1))))
    return np.array(out)


def dt_float64():
    """(the joint Kalman float64 model's misalignments, the joint NLMS float64 model's at mu = 0.5, the bank of single-reference
    Kalman models'), [3, bins] each"""
    def make():
        I, K, B = DT["inputs"], DT["taps"], DT["bins"]
        return (dt_misalignment(Model(I, 1, B, K, prec=64)), dt_misalignment(mc.Model(I, 1, B, K, mu=0.5, delta=DELTA, prec=64)),
                dt_singles())
    return cached(("kalman matrix dt f64",), make)


dt_report = kc.dt_report


# ------------------------------------------------------------------------------------------------ end to end
# adapt_bands_matrix_checks.E2E's bank and case -- two independent white loudspeaker signals into three microphones -- with
# kalman_bands_checks' near-end burst of white noise at the echo's level added to d over E2E_BURST (in frames of the band rate);
# the residual is read over the last quarter, 200 frames behind the burst's end
E2E = mc.E2E
E2E_BURST = kc.E2E_BURST
e2e_params = kc.e2e_params


def e2e_case(oracle):
    """(x, d, w) of adapt_bands_matrix_checks.e2e_case with the burst added to d"""
    def make():
        from tests import adapt_checks as ac
        x, d, w = mc.e2e_case(oracle)
        hop = E2E["M"] // E2E["os"]
        lo, hi = E2E_BURST[0] * hop, E2E_BURST[1] * hop
        d = d.copy()
        near = np.random.default_rng(4244).standard_normal((d.shape[0], hi - lo))
        d[:, lo:hi] += (near * ac.rms(d, axis=1)[:, None]).astype(np.float32)
        d.setflags(write=False)
        return x, d, w
    return cached(("kalman matrix e2e",), make)


def e2e_float64(oracle):
    """the float64 chain: pfb_checks' float64 bank in TIME phase, the float64 model, the float64 synthesis of e and of d; returns
    the residual ratios per output (adapt_bands_checks.e2e_residual: the last quarter)"""
    def make():
        from tests import pfb_checks as pc
        x, d, w = e2e_case(oracle)
        M, P, os = (E2E[k] for k in ("M", "P", "os"))
        X, _ = pc.analysis(x, w, M, P, os, pc.TIME)
        D, _ = pc.analysis(d, w, M, P, os, pc.TIME)
        X, D = X.astype(np.complex64), D.astype(np.complex64)
        m = Model(E2E["inputs"], E2E["outputs"], M // 2 + 1, E2E["taps"], prec=64, **e2e_params(X))
        e, _ = m.process(X, D)
        et, _ = pc.synthesis(*split(e), w, M, P, os, pc.TIME)
        dt, _ = pc.synthesis(*split(D), w, M, P, os, pc.TIME)
        return bc.e2e_residual(et, dt)
    return cached(("kalman matrix e2e f64",), make)
