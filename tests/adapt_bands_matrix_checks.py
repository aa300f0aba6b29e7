"""Shared pieces of the multi-reference per-band adaptive filter's tests (test_adapt_bands_matrix_host.py,
test_adapt_bands_matrix_gpu.py; llz_adapt_bands_matrix_mc, include/llz_adapt_bands_matrix.h): the MODEL of the definition in
float64 (the reference everywhere) and in float32 / complex64 (the device's stand-in on a machine without a GPU), the case
generator, the device runner and the checks.  The model is written from the definition in the header in plain numpy and knows
nothing of the kernel: one shift register of frames per (input, bin), shared by the outputs; no entry ceiling, no lanes, no second
history buffer.

The definition, per (output o, bin k): weights w_{i,q}, i < I, q < K, complex, initially zero; per (input i, bin k) a history
x_i[m - q], zero before frame 0.  For frame m: y = sum_{q < K} sum_{i < I} w_{i,q} x_i[m - q] (no conjugate on w); e = d[m] - y;
where the output's mu != 0: p = sum_q sum_i |x_i[m - q]|^2 (the JOINT power), g = mu e / (p + delta), w_{i,q} += g conj(x_i[m - q]).

Limits (none of them taken from the device's results), TOL = edge_checks.TOL = 1e-5, the project's gate:
  * the error: per (output, bin, run of RUN = 16 frames) rms(e - e_ref) <= TOL rms(d of that output and bin over the case);
  * the taps: per (output, bin) |w - w_ref|_2 <= TOL |h|_2, over all (i, q);
  * the misalignment |w - h|_2 at most max(2 x the float64 model's, the model's + TOL |h|_2) (adapt_bands_checks.py's rule);
  * convergence: the last run's error rms below a tenth of the first run's wherever the float64 model's is;
  * e bit-equal to float32(d) - y everywhere.
A shape is a GPU case only while the float32 model stays below HALF of the first three on the CPU (test_adapt_bands_matrix_host.py
asserts it); the planted faults of that file miss them."""
import numpy as np

from tests import adapt_bands_checks as bc

TOL, U, MU, DELTA, RUN = bc.TOL, bc.U, bc.MU, bc.DELTA, bc.RUN
CEILINGS = (8, 16, 32, 64)
# (inputs, outputs, taps, bins, frames): a full and a just exceeded ceiling of 8 (8, 15 entries), full ceilings of 32 and 64 by
# few inputs of many taps and by many inputs of few, 60 entries that leave 4 of the ceiling dead, an input count that divides no
# ceiling, 8 inputs of one tap (no history at all) on 37 outputs of 5 bins (a dozen outputs in a wave), rows that straddle waves
SHAPES = [(2, 2, 4, 33, 300), (3, 2, 5, 33, 300), (2, 3, 16, 129, 400), (5, 2, 12, 33, 600), (4, 3, 16, 65, 600),
          (8, 2, 8, 33, 600), (2, 2, 32, 17, 600), (8, 37, 1, 5, 200)]
LONG = (2, 1, 4, 2049, 64)      # a row longer than any workgroup
FAULT_SHAPE = SHAPES[1]
FAULTS = ("first_reference_power", "taps_transposed", "one_input_late", "neighbours_error", "not_conjugated")
cached, cbits, split, ratio, run_rms, gaussian = bc.cached, bc.cbits, bc.split, bc.ratio, bc.run_rms, bc.gaussian


def ceiling(inputs, taps):
    return next(c for c in CEILINGS if inputs * taps <= c)


# ------------------------------------------------------------------------------------------------ the cases
def responses(outputs, inputs, taps, bins, seed):
    """[outputs, inputs, taps, bins] complex128 of float32 values: complex Gaussian times exp(-q / (K / 4 + 1)), of unit norm per
    (output, bin) over all (i, q)"""
    rng = np.random.default_rng(seed)
    shape = (outputs, inputs, taps, bins)
    h = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    h *= np.exp(-np.arange(taps) / (taps / 4 + 1))[None, None, :, None]
    h /= np.sqrt(np.sum(np.abs(h) ** 2, axis=(1, 2), keepdims=True))
    return h.astype(np.complex64).astype(np.complex128)


def convolve(x, h):
    """d[o, m, k] = sum_i sum_q h[o, i, q, k] x[i, m - q, k] in complex128"""
    frames = x.shape[1]
    d = np.zeros((h.shape[0], frames, x.shape[2]), np.complex128)
    x = x.astype(np.complex128)
    for i in range(h.shape[1]):
        for q in range(h.shape[2]):
            d[:, q:] += h[:, i, q][:, None, :] * x[i, :frames - q][None]
    return d


def case(oracle, inputs, outputs, taps, bins, frames):
    """(x, d, h): x [inputs, frames, bins], d [outputs, frames, bins] complex64, h [outputs, inputs, taps, bins]; independent
    unit-variance references, d = sum_i h_{o,i} * x_i rounded to float32"""
    def make():
        x = gaussian(oracle, inputs, frames, bins, seed=211 + 7 * taps + bins + 31 * inputs)
        h = responses(outputs, inputs, taps, bins, seed=taps + 1000 * bins + 17 * inputs + outputs)
        d = convolve(x, h).astype(np.complex64)
        for a in (x, d, h):
            a.setflags(write=False)
        return x, d, h
    return cached(("bands matrix case", inputs, outputs, taps, bins, frames), make)


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """llz_adapt_bands_matrix_mc from the definition.  prec: 64 (the reference) or 32 (float32 components, complex64 products).
    fault: None or one of FAULTS, for the tests that show the limits are not slack."""

    def __init__(self, inputs, outputs, bins, taps, mu=MU, delta=DELTA, prec=64, fault=None):
        assert fault is None or fault in FAULTS
        self.rt, self.ct = (np.float32, np.complex64) if prec == 32 else (np.float64, np.complex128)
        self.inputs, self.outputs, self.bins, self.taps, self.fault = inputs, outputs, bins, taps, fault
        self.delta = self.rt(delta)
        self.mu = np.full(outputs, mu, self.rt)
        self.W = np.zeros((outputs, inputs, taps, bins), self.ct)
        self.reset(False)

    def reset(self, clear_taps=False):
        self.X = np.zeros((self.inputs, self.taps + 1, self.bins), self.ct)          # X[i, q] = x_i[m - q]; one more for the late fault
        self.count = 0
        if clear_taps:
            self.W[:] = 0

    def set_step(self, first, mu):
        mu = np.atleast_1d(np.asarray(mu, self.rt))
        self.mu[first:first + len(mu)] = mu

    def set_taps(self, out_first, w, in_first=0):
        w = np.asarray(w, np.complex64)
        assert self.fault is None
        self.W[out_first:out_first + w.shape[0], in_first:in_first + w.shape[1]] = w

    def get_taps(self):
        if self.fault == "taps_transposed":         # the memory that set_taps / get_taps lay out [i][q], walked as [q][i]
            w = self.W.transpose(0, 2, 1, 3).reshape(self.W.shape)
            return np.ascontiguousarray(w).astype(np.complex64)
        return self.W.astype(np.complex64)

    def frames(self):
        return self.count

    def process(self, x, d):
        """x complex [inputs, frames, bins], d complex [outputs, frames, bins] -> (e, y) in the model's precision"""
        ct, rt, K, I = self.ct, self.rt, self.taps, self.inputs
        x, d = np.asarray(x).astype(ct), np.asarray(d).astype(ct)
        e, y = np.empty(d.shape, ct), np.empty(d.shape, ct)
        on = self.mu != 0
        mu = self.mu[:, None]
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
            if on.any():
                p = np.zeros(self.bins, rt)
                for q in range(K):
                    for i in range(1 if self.fault == "first_reference_power" else I):
                        p = (p + (X[i, q].real ** 2 + X[i, q].imag ** 2).astype(rt)).astype(rt)
                den = (p + self.delta).astype(rt)[None]
                drive = np.roll(em, 1, axis=0) if self.fault == "neighbours_error" else em
                g = ((mu * drive.real).astype(rt) / den + 1j * ((mu * drive.imag).astype(rt) / den)).astype(ct)
                Xu = X if self.fault == "not_conjugated" else np.conj(X)
                self.W[on] = (self.W[on] + g[on][:, None, None, :] * Xu[None]).astype(ct)
        self.count += x.shape[1]
        return e, y

    def close(self):
        pass


def model32(inputs, outputs, bins, taps, mu=MU, delta=DELTA):
    """the device's stand-in: the float32 model behind the runners' interface"""
    return Model(inputs, outputs, bins, taps, mu, delta, prec=32)


def definition_loops(x, d, taps, mu, delta):
    """one (output, bin) stream from the definition written out as plain loops over Python complex numbers; x [inputs, frames],
    d [frames]: (e, y, w [inputs, taps])"""
    inputs = len(x)
    w = [[0j] * taps for _ in range(inputs)]
    e, y = [], []
    hist = lambda i, m, q: complex(x[i][m - q]) if m - q >= 0 else 0j          # noqa: E731
    for m in range(len(d)):
        ym = sum(w[i][q] * hist(i, m, q) for q in range(taps) for i in range(inputs))
        em = complex(d[m]) - ym
        if mu != 0:
            p = sum(abs(hist(i, m, q)) ** 2 for q in range(taps) for i in range(inputs))
            g = mu * em / (p + delta)
            for i in range(inputs):
                for q in range(taps):
                    w[i][q] += g * hist(i, m, q).conjugate()
        e.append(em)
        y.append(ym)
    return np.array(e), np.array(y), np.array(w)


# ------------------------------------------------------------------------------------------------ the device
class Device:
    """filters.AdaptBandsMatrixMC behind the model's interface: complex numpy in and out through device tensors, outputs preset to
    NaN.  calls: how process() groups its frames into calls (None: all at once; a number: that many per call; a list: those counts
    in turn, repeated)"""

    def __init__(self, dev, inputs, outputs, bins, taps, mu=MU, delta=DELTA, calls=None):
        from llzlab_amd import filters
        self.dev, self.inputs, self.outputs, self.bins, self.taps, self.calls = dev, inputs, outputs, bins, taps, calls
        self.f = filters.AdaptBandsMatrixMC(inputs, outputs, bins, taps, mu=mu, delta=delta)
        plan = self.f.plan()
        assert plan == (inputs, ceiling(inputs, taps), plan[2], -(-outputs * bins // plan[2]), 1) and plan[2] % 64 == 0, plan

    sizes = bc.Device.sizes

    def process(self, x, d, want_y=True):
        import torch
        up = lambda z: tuple(torch.from_numpy(a).to(self.dev) for a in split(z))      # noqa: E731
        new = lambda n: tuple(torch.full((self.outputs, n, self.bins), float("nan"), dtype=torch.float32, device=self.dev)  # noqa: E731
                              for _ in range(2))
        es, ys, o = [], [], 0
        for n in self.sizes(x.shape[1]):
            e, y = new(n), (new(n) if want_y else None)
            self.f.process(up(x[:, o:o + n]), up(d[:, o:o + n]), e, y)
            es.append(e[0].cpu().numpy() + 1j * e[1].cpu().numpy())
            ys.append(y[0].cpu().numpy() + 1j * y[1].cpu().numpy() if want_y else None)
            o += n
        e = np.concatenate(es, axis=1).astype(np.complex64)
        return e, (np.concatenate(ys, axis=1).astype(np.complex64) if want_y else None)

    def set_step(self, first, mu):
        self.f.set_step(first, mu)

    def set_taps(self, out_first, w, in_first=0):
        self.f.set_taps(out_first, w, in_first)

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
def reference(oracle, inputs, outputs, taps, bins, frames):
    """the float64 model over the whole case: (e, y, w, misalignment per (output, bin)), computed once"""
    def make():
        x, d, h = case(oracle, inputs, outputs, taps, bins, frames)
        m = Model(inputs, outputs, bins, taps, prec=64)
        e, y = m.process(x, d)
        return e, y, m.W.copy(), np.sqrt(np.sum(np.abs(m.W - h) ** 2, axis=(1, 2)))
    return cached(("bands matrix ref", inputs, outputs, taps, bins, frames), make)


def measure_parity(make, oracle, inputs, outputs, taps, bins, frames):
    """one case through `make(inputs, outputs, bins, taps, mu, delta)` against the float64 model: each figure as a ratio to its
    limit -- 'error' (per output, bin and run, the worst), 'taps', 'misalignment' --, 'converges' (the error falls wherever the
    model's does), and e = d - y checked on the way"""
    x, d, h = case(oracle, inputs, outputs, taps, bins, frames)
    e_ref, _, w_ref, mis_ref = reference(oracle, inputs, outputs, taps, bins, frames)
    what = f"bands matrix I={inputs} O={outputs} K={taps} bins={bins} x {frames} frames"
    r = make(inputs, outputs, bins, taps, MU, DELTA)
    e, y = r.process(x, d)
    w = r.get_taps()
    assert r.frames() == frames, f"{what}: frames() is {r.frames()}"
    r.close()
    assert e.shape == d.shape and y.shape == d.shape and w.shape == (outputs, inputs, taps, bins)
    assert np.array_equal(cbits(e), cbits(d - y)), f"{what}: e is not the float32 difference d - y"
    d_rms = np.sqrt(np.mean(np.abs(d.astype(np.complex128)) ** 2, axis=1))          # [outputs, bins]
    err = run_rms(e.astype(np.complex128) - e_ref)
    error = ratio(err, TOL * np.broadcast_to(d_rms[:, None, :], err.shape))
    hn = np.sqrt(np.sum(np.abs(h) ** 2, axis=(1, 2)))
    w64 = w.astype(np.complex128)
    tap = ratio(np.sqrt(np.sum(np.abs(w64 - w_ref) ** 2, axis=(1, 2))), TOL * hn)
    mis = np.sqrt(np.sum(np.abs(w64 - h) ** 2, axis=(1, 2)))
    mis_ratio = ratio(mis, np.maximum(2.0 * mis_ref, mis_ref + TOL * hn))
    runs, runs_ref = run_rms(e), run_rms(e_ref)
    conv = runs_ref[:, -1] < 0.1 * runs_ref[:, 0]
    out = {"error": error, "taps": tap, "misalignment": mis_ratio,
           "converges": bool(np.all(runs[:, -1][conv] < 0.1 * runs[:, 0][conv])),
           "fall": float(np.max(runs_ref[:, -1] / runs_ref[:, 0]))}
    print(f"{what}: worst error ratio {error:.3g} of the gate; taps {tap:.3g} of theirs; misalignment "
          f"{np.max(mis[np.isfinite(mis)], initial=0):.3g} (model {mis_ref.max():.3g}), {mis_ratio:.3g} of its limit; {int(conv.sum())} "
          f"of {conv.size} (output, bin) held to a tenth (float64 last / first at most {out['fall']:.3g})")
    return out


def check_parity(make, oracle, inputs, outputs, taps, bins, frames, share=1.0):
    """share: the part of the error and tap limits the runner may use (0.5 for the float32 model, which admits a shape to the GPU
    list; the misalignment limit is twice the float64 model's own figure, so a faithful runner sits at half of it by construction)"""
    what = f"bands matrix I={inputs} O={outputs} K={taps} bins={bins}"
    m = measure_parity(make, oracle, inputs, outputs, taps, bins, frames)
    assert m["error"] <= share, f"{what}: error at {m['error']:.3g} of the gate"
    assert m["taps"] <= share, f"{what}: taps at {m['taps']:.3g} of their limit"
    assert m["misalignment"] <= 1.0, f"{what}: misalignment at {m['misalignment']:.3g} of its limit"
    assert m["converges"], f"{what}: the error does not fall where the model's does"
    return m


def worst_miss(make, oracle, inputs, outputs, taps, bins, frames):
    """the largest ratio of a figure to its limit (a run that ends in NaN or inf misses by inf)"""
    with np.errstate(all="ignore"):
        m = measure_parity(make, oracle, inputs, outputs, taps, bins, frames)
    return max(m["error"], m["taps"], m["misalignment"])


# ------------------------------------------------------------------------------------------------ the point of the feature
def two_against_one(oracle, taps=4, bins=33, frames=400):
    """d = h_0 * x_0 + h_1 * x_1 with paths of equal norms per bin, on the float64 models: the last run's error rms over the first
    run's -- of the single-reference filter on x_0 with the rms taken over the run's frames and all bins (one bin's 16 frames
    scatter by a factor of two around the floor that x_1's echo sets), and of the two-reference filter per bin"""
    x = gaussian(oracle, 2, frames, bins, seed=77)
    h = responses(1, 2, taps, bins, seed=78)
    h /= np.sqrt(2.0 * np.sum(np.abs(h) ** 2, axis=2, keepdims=True))          # each path of norm sqrt(1/2)
    d = convolve(x, h).astype(np.complex64)
    one = bc.Model(1, bins, taps, prec=64)
    e1, _ = one.process(x[:1], d)
    two = Model(2, 1, bins, taps, prec=64)
    e2, _ = two.process(x, d)
    r1, r2 = np.sqrt(np.mean(run_rms(e1)[0] ** 2, axis=1)), run_rms(e2)[0]
    return float(r1[-1] / r1[0]), r2[-1] / r2[0]


# ------------------------------------------------------------------------------------------------ end to end
# adapt_bands_checks.E2E's bank and length; two independent loudspeaker signals into three microphones
E2E = dict(bc.E2E, inputs=2, outputs=3)


def e2e_case(oracle):
    """(x, d, w): x [inputs, frames hop], d [outputs, frames hop] float32, d = sum_i x_i * h_{o,i} with decaying responses behind
    a lead-in, of unit norm per output over both paths; w the prototype"""
    def make():
        from llzlab_amd import filters
        from tests import adapt_checks as ac
        I, O, M, P, os, frames = (E2E[k] for k in ("inputs", "outputs", "M", "P", "os", "frames"))
        n = frames * (M // os)
        x = ac.gaussian(oracle, I, n, seed=4343)
        rng = np.random.default_rng(78)
        h = np.zeros((O, I, E2E["lead"] + E2E["length"]))
        h[:, :, E2E["lead"]:] = rng.standard_normal((O, I, E2E["length"])) * np.exp(-np.arange(E2E["length"]) / 12.0)
        h /= np.sqrt(np.sum(h * h, axis=(1, 2), keepdims=True))
        d = np.stack([sum(np.convolve(x[i].astype(np.float64), h[o, i])[:n] for i in range(I)) for o in range(O)]).astype(np.float32)
        w = filters.pfb_prototype(M, P)
        for a in (d, w):
            a.setflags(write=False)
        return x, d, w
    return cached(("bands matrix e2e",), make)


def e2e_delta(X):
    """the regularisation for bands that are not of unit variance: 1e-3 x inputs x taps x the mean band power"""
    return float(1e-3 * E2E["inputs"] * E2E["taps"] * np.mean(np.abs(X) ** 2))


def e2e_float64(oracle):
    """the float64 chain: pfb_checks' float64 bank in TIME phase, the float64 model, the float64 synthesis of e and of d; returns
    the residual ratios per output"""
    def make():
        from tests import pfb_checks as pc
        x, d, w = e2e_case(oracle)
        M, P, os = (E2E[k] for k in ("M", "P", "os"))
        X, _ = pc.analysis(x, w, M, P, os, pc.TIME)
        D, _ = pc.analysis(d, w, M, P, os, pc.TIME)
        X, D = X.astype(np.complex64), D.astype(np.complex64)
        m = Model(E2E["inputs"], E2E["outputs"], M // 2 + 1, E2E["taps"], delta=e2e_delta(X), prec=64)
        e, _ = m.process(X, D)
        et, _ = pc.synthesis(*split(e), w, M, P, os, pc.TIME)
        dt, _ = pc.synthesis(*split(D), w, M, P, os, pc.TIME)
        return bc.e2e_residual(et, dt)
    return cached(("bands matrix e2e f64",), make)
