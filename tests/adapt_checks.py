"""Shared pieces of the adaptive filter's tests (test_adapt_host.py, test_adapt_gpu.py; llz_adapt_mc, include/llz_adapt.h): the
MODEL of the definition in float64 (the reference everywhere) and in float32 / complex64 (the device's stand-in on a machine
without a GPU), the case generator, the two runners and the checks.  The model is written from the definition in llz_adapt.h in
plain numpy fft / rfft and knows nothing of the kernel: natural bin order, no packing, no power-of-two rescaling, a shift
register of spectra where the device has a ring.

The definition, per channel: block B, N = 2 B, P = ceil(T / B).  For block j: X_j = rfft(blocks (j - 1, j) of x); Y = sum_p
X_{j-p} W_p, p ascending; y = the last B samples of irfft(Y); e = d - y; where mu != 0: E = rfft([0_B, e]), D = sum_p |X_{j-p}|^2,
G = mu E / (D + delta), and for every p: dW = conj(X_{j-p}) G, dw = irfft(dW) with every sample t >= min(B, T - p B) zeroed,
W_p += rfft(dw).

Limits (none of them taken from the device's results):
  * the error: per channel and block rms(e - e_ref) <= TOL rms(d of the channel), TOL = edge_checks.TOL = 1e-5, the project's gate;
  * the taps: |w - w_ref|_2 <= TOL |h|_2, and the misalignment |w - h|_2 at most twice the float64 model's (with one tap the
    model's is 1e-8, below a float32 rounding of the tap returned: there the limit is the model's plus TOL |h|_2, which the tap
    gate implies by the triangle inequality);
  * convergence: the last block's error rms below a tenth of the first block's wherever the float64 model's is.
The float32 model sits at a few percent of the first two; the planted faults of test_adapt_host.py miss them."""
import numpy as np

from tests import edge_checks as ec

TOL = ec.TOL
MU = 0.5
# (block, taps, blocks): P = 1 with one tap and with a full partition, a last partition holding 7 and 1 taps, workgroups of one
# wave and of several, threads owning 1, 2 and 8 bins, both parities of log2 block
SHAPES = [(64, 1, 60), (64, 64, 60), (64, 199, 60), (128, 513, 60), (512, 1100, 60), (2048, 2049, 8)]
CHANNELS = (3, 37)
# (block, taps, blocks, channels) beyond the shapes above, for the paths those leave out.  (64, 7100) on 37 channels: P = 111,
# 4107 (channel, partition) pairs, past the 4096 from which an update workgroup takes 4 partitions in sequence, P not a multiple
# of 4 (the last group holds 3), and P >= 9, so the filter's ring walk runs its unrolled loop of 8 partitions in flight and the
# remainder.  (256, 2400): the 256-point instances, one bin per thread at 256 threads, P = 10, unrolled loop and remainder.
# (1024, 3500): the 1024-point instances, 4 bins per thread, 2 partitions in flight, P = 4: one unrolled step and one left.
WIDE = (64, 7100, 16, 37)
EXTRA = [WIDE, (256, 2400, 12, 3), (1024, 3500, 8, 3)]
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def delta_for(block):
    return 1e-3 * block


def partitions(T, block):
    return -(-T // block)


def blocks_per_call(nblocks):
    """how the parity cases group their blocks into calls: 4 per call where that divides, else 2"""
    return 4 if nblocks % 4 == 0 and nblocks > 8 else 2


# ------------------------------------------------------------------------------------------------ the cases
def gaussian(oracle, channels, n, seed):
    """[channels, n] float32 white Gaussian noise of unit variance: Box-Muller over two streams of the oracle's generator
    (uniform in [-1, 1))"""
    def make():
        a = oracle.synth_f32(channels, n, seed=seed).astype(np.float64)
        b = oracle.synth_f32(channels, n, seed=seed + 7919, chan0=channels).astype(np.float64)
        u1 = 1.0 - (a + 1.0) / 2.0                              # (0, 1]
        g = np.sqrt(-2.0 * np.log(u1)) * np.cos(np.pi * (b + 1.0))
        g = g.astype(np.float32)
        g.setflags(write=False)
        return g
    return cached(("x", channels, n, seed), make)


def responses(channels, T, seed):
    """[channels, T] float64 (float32 values): Gaussian times exp(-n / (T / 4 + 1)), unit norm, a draw per channel"""
    def make():
        n = np.arange(T)
        h = np.stack([np.random.default_rng(seed + 1000 * c).standard_normal(T) for c in range(channels)]) * np.exp(-n / (T / 4 + 1))
        h /= np.sqrt(np.sum(h * h, axis=1, keepdims=True))
        h = h.astype(np.float32).astype(np.float64)
        h.setflags(write=False)
        return h
    return cached(("h", channels, T, seed), make)


def case(oracle, block, T, channels, nblocks):
    """(x, d, h): x [channels, n] float32, h [channels, T], d = x * h truncated to n samples, float32"""
    def make():
        n = nblocks * block
        x = gaussian(oracle, channels, n, seed=11 + T + block)
        h = responses(channels, T, seed=T + block)
        d = np.stack([np.convolve(x[c].astype(np.float64), h[c])[:n] for c in range(channels)]).astype(np.float32)
        d.setflags(write=False)
        return x, d, h
    return cached(("case", block, T, channels, nblocks), make)


# ------------------------------------------------------------------------------------------------ the model
FAULTS = ("unconstrained", "not_conjugated", "one_partition_late", "newest_power_only")


class Model:
    """llz_adapt_mc from the definition.  prec: 64 (the reference) or 32 (float32 samples, complex64 spectra).  fault: None or
    one of FAULTS, for the tests that show the limits are not slack."""

    def __init__(self, channels, block, T, frame_len=None, mu=MU, delta=None, prec=64, fault=None):
        assert fault is None or fault in FAULTS
        self.rt, self.ct = (np.float32, np.complex64) if prec == 32 else (np.float64, np.complex128)
        self.channels, self.B, self.T, self.P = channels, block, T, partitions(T, block)
        self.delta = self.rt(delta_for(block) if delta is None else delta)
        self.mu = np.full(channels, mu, self.rt)
        self.fault = fault
        self.W = np.zeros((channels, self.P, block + 1), self.ct)
        self.reset(False)

    def reset(self, clear_taps=False):
        # X[:, p] = X_{j-p}; one more than P for the fault that reads a partition late
        self.X = np.zeros((self.channels, self.P + 1, self.B + 1), self.ct)
        self.prev = np.zeros((self.channels, self.B), self.rt)
        if clear_taps:
            self.W[:] = 0

    def set_step(self, first, mu):
        mu = np.atleast_1d(np.asarray(mu, self.rt))
        self.mu[first:first + len(mu)] = mu

    def lim(self, p):
        return min(self.B, self.T - p * self.B)

    def set_taps(self, first, taps):
        taps = np.atleast_2d(np.asarray(taps, np.float32)).astype(np.float64)
        hp = np.zeros((taps.shape[0], self.P * self.B))
        hp[:, :self.T] = taps
        self.W[first:first + taps.shape[0]] = np.fft.rfft(hp.reshape(-1, self.P, self.B), 2 * self.B, axis=2).astype(self.ct)

    def get_taps(self):
        w = np.fft.irfft(self.W.astype(np.complex128), 2 * self.B, axis=2)[:, :, :self.B].reshape(self.channels, -1)
        return w[:, :self.T].astype(np.float32)

    def process(self, x, d):
        """x, d: [channels, m B] -> (e, y) float32"""
        B, rt = self.B, self.rt
        x, d = np.asarray(x, rt), np.asarray(d, rt)
        e, y = np.empty(x.shape, np.float32), np.empty(x.shape, np.float32)
        for j in range(x.shape[1] // B):
            e[:, j * B:(j + 1) * B], y[:, j * B:(j + 1) * B] = self.block(x[:, j * B:(j + 1) * B], d[:, j * B:(j + 1) * B])
        return e, y

    def block(self, xb, db):
        B, N, P, rt, ct = self.B, 2 * self.B, self.P, self.rt, self.ct
        self.X[:, 1:] = self.X[:, :-1].copy()
        self.X[:, 0] = np.fft.rfft(np.concatenate([self.prev, xb], axis=1), axis=1).astype(ct)
        self.prev = xb.copy()
        X = self.X
        Y = np.zeros((self.channels, B + 1), ct)
        for p in range(P):                                      # p ascending
            Y = (Y + X[:, p] * self.W[:, p]).astype(ct)
        yb = np.fft.irfft(Y, N, axis=1)[:, B:].astype(rt)
        eb = (db - yb).astype(rt)
        on = self.mu != 0
        if on.any():
            E = np.fft.rfft(np.concatenate([np.zeros_like(eb), eb], axis=1), axis=1).astype(ct)
            span = X[:, :1] if (self.fault == "newest_power_only" and P > 1) else X[:, :P]
            D = np.zeros((self.channels, B + 1), rt)
            for p in range(span.shape[1]):
                D = (D + (span[:, p].real ** 2 + span[:, p].imag ** 2).astype(rt)).astype(rt)
            den = (D + self.delta).astype(rt)
            mu = self.mu[:, None]
            G = ((mu * E.real).astype(rt) / den + 1j * ((mu * E.imag).astype(rt) / den)).astype(ct)
            for p in range(P):
                Xp = X[:, p + 1] if self.fault == "one_partition_late" else X[:, p]
                dW = ((Xp if self.fault == "not_conjugated" else np.conj(Xp)) * G).astype(ct)
                if self.fault != "unconstrained":
                    dw = np.fft.irfft(dW, N, axis=1).astype(rt)
                    dw[:, self.lim(p):] = 0
                    dW = np.fft.rfft(dw, axis=1).astype(ct)
                self.W[on, p] = (self.W[on, p] + dW[on]).astype(ct)
        return eb.astype(np.float32), yb.astype(np.float32)

    def close(self):
        pass


def model32(channels, block, T, frame_len=None, mu=MU, delta=None):
    """the device's stand-in: the float32 model behind the runners' interface"""
    return Model(channels, block, T, frame_len, mu, delta, prec=32)


# ------------------------------------------------------------------------------------------------ the device
class Device:
    """filters.AdaptMC behind the model's interface: numpy in and out through device tensors, outputs preset to NaN"""

    def __init__(self, dev, channels, block, T, frame_len=None, mu=MU, delta=None):
        from llzlab_amd import filters
        self.dev, self.channels = dev, channels
        self.f = filters.AdaptMC(channels, block, T, frame_len=frame_len, mu=mu, delta=delta)
        k = (frame_len or block) // block
        assert self.f.plan() == (2 * block, partitions(T, block), partitions(T, block) + k - 1, k), self.f.plan()

    def process(self, x, d, want_y=True):
        import torch
        n = self.f.frame_len
        es, ys = [], []
        for o in range(0, x.shape[1], n):
            xi = torch.from_numpy(np.ascontiguousarray(x[:, o:o + n], dtype=np.float32)).to(self.dev)
            di = torch.from_numpy(np.ascontiguousarray(d[:, o:o + n], dtype=np.float32)).to(self.dev)
            ei = torch.full_like(xi, float("nan"))
            yi = torch.full_like(xi, float("nan")) if want_y else None
            self.f.process(xi, di, ei, yi)
            es.append(ei.cpu().numpy())
            ys.append(yi.cpu().numpy() if want_y else None)
        return np.concatenate(es, axis=1), (np.concatenate(ys, axis=1) if want_y else None)

    def set_step(self, first, mu):
        self.f.set_step(first, mu)

    def set_taps(self, first, taps):
        self.f.set_taps(first, taps)

    def get_taps(self):
        return self.f.get_taps()

    def reset(self, clear_taps=False):
        self.f.reset(clear_taps)

    def close(self):
        self.f.close()


def device(dev):
    return lambda *a, **kw: Device(dev, *a, **kw)


# ------------------------------------------------------------------------------------------------ the checks
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rms(a, axis=None):
    return np.sqrt(np.mean(np.asarray(a, np.float64) ** 2, axis=axis))


def block_rms(a, block):
    """[channels, blocks]"""
    return rms(np.asarray(a, np.float64).reshape(a.shape[0], -1, block), axis=2)


def reference(oracle, block, T, channels, nblocks):
    """the float64 model over the whole case: (e, y, w, misalignment per channel), computed once"""
    def make():
        x, d, h = case(oracle, block, T, channels, nblocks)
        m = Model(channels, block, T, prec=64)
        e, y = m.process(x.astype(np.float64), d.astype(np.float64))
        W = np.fft.irfft(m.W, 2 * block, axis=2)[:, :, :block].reshape(channels, -1)[:, :T]
        return e, y, W, np.sqrt(np.sum((W - h) ** 2, axis=1))
    return cached(("ref", block, T, channels, nblocks), make)


def measure_parity(make, oracle, block, T, channels, nblocks, mu=MU):
    """one case through `make(channels, block, T, frame_len, mu, delta)` against the float64 model: each figure as a ratio to its
    limit -- 'error' (per channel and block, the worst), 'taps', 'misalignment' -- and 'converges' (the error falls wherever the
    model's does)"""
    x, d, h = case(oracle, block, T, channels, nblocks)
    e_ref, _, w_ref, mis_ref = reference(oracle, block, T, channels, nblocks)
    what = f"adapt block {block} T={T} {channels}ch x {nblocks} blocks"
    r = make(channels, block, T, blocks_per_call(nblocks) * block, mu, delta_for(block))
    e, y = r.process(x, d)
    w = r.get_taps().astype(np.float64)
    r.close()
    assert e.shape == x.shape and e.dtype == np.float32 and w.shape == (channels, T)
    assert np.array_equal(bits(e), bits(d - y)), f"{what}: e is not the float32 difference d - y"
    ratio = block_rms(e.astype(np.float64) - e_ref, block) / (TOL * rms(d, axis=1)[:, None])
    c, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    hn = np.sqrt(np.sum(h * h, axis=1))
    tap = np.sqrt(np.sum((w - w_ref) ** 2, axis=1)) / (TOL * hn)
    # twice the model's; where the model's own lies below the tap gate (one tap: 1e-8, less than a float32 rounding of the tap
    # get_taps returns) the bound the tap gate implies by the triangle inequality, mis_ref + TOL |h|, which adds nothing to it
    mis = np.sqrt(np.sum((w - h) ** 2, axis=1))
    mis_ratio = mis / np.maximum(2.0 * mis_ref, mis_ref + TOL * hn)
    first, last = block_rms(e, block)[:, 0], block_rms(e, block)[:, -1]
    conv = block_rms(e_ref, block)[:, -1] < 0.1 * block_rms(e_ref, block)[:, 0]
    out = {"error": float(ratio.max()), "taps": float(tap.max()), "misalignment": float(mis_ratio.max()),
           "converges": bool(np.all(last[conv] < 0.1 * first[conv]))}
    print(f"{what}: worst error ratio {out['error']:.3g} of the gate (channel {c}, block {j}); taps {out['taps']:.3g} of theirs; "
          f"misalignment {mis.max():.3g} (model {mis_ref.max():.3g}), {out['misalignment']:.3g} of its limit; last / first error "
          f"rms {np.max(last / first):.3g}, {int(conv.sum())} of {channels} channels held to a tenth")
    return out


def check_parity(make, oracle, block, T, channels, nblocks):
    what = f"adapt block {block} T={T} {channels}ch"
    m = measure_parity(make, oracle, block, T, channels, nblocks)
    assert m["error"] <= 1.0, f"{what}: error at {m['error']:.3g} of the gate"
    assert m["taps"] <= 1.0, f"{what}: taps at {m['taps']:.3g} of their limit"
    assert m["misalignment"] <= 1.0, f"{what}: misalignment at {m['misalignment']:.3g} of its limit"
    assert m["converges"], f"{what}: the error does not fall where the model's does"
    return m


def worst_miss(make, oracle, block, T, channels, nblocks):
    """the largest ratio of a figure to its limit (a run that ends in NaN or inf misses by inf)"""
    with np.errstate(all="ignore"):
        m = measure_parity(make, oracle, block, T, channels, nblocks)
    worst = max(m["error"], m["taps"], m["misalignment"])
    return float("inf") if not np.isfinite(worst) else worst


RING = (64, 199, 3)             # block, taps, k: R = P + k - 1 = 6


def check_frozen(make, stream_run, oracle, exact=True, shapes=SHAPES, channels=3):
    """case 1: after set_taps(h) with every mu = 0, y is FirStreamMC's with the same rows on the same input -- bit for bit on
    the device (exact), to the gate between the two numpy models -- and e is the float32 difference np.float32(d) - y"""
    for block, T, _ in shapes:
        nblocks = partitions(T, block) + 3
        x, d, h = case(oracle, block, T, channels, nblocks)
        r = make(channels, block, T, block, 0.0, delta_for(block))
        r.set_taps(0, h)
        e, y = r.process(x, d)
        w = r.get_taps()
        r.close()
        ys = stream_run(x, h, block)
        what = f"frozen block {block} T={T}"
        if exact:
            assert np.array_equal(bits(y), bits(ys)), f"{what}: {np.count_nonzero(bits(y) != bits(ys))} samples differ from FirStreamMC's"
        else:
            assert np.all(rms(y - ys, axis=1) <= TOL * rms(ys, axis=1)), what
        assert np.array_equal(bits(e), bits(np.float32(d) - y)), f"{what}: e is not d - y"
        hn = np.sqrt(np.sum(h * h, axis=1))
        assert np.all(np.abs(w - h) <= 2 * ec.U * hn[:, None]), f"{what}: a frozen handle's taps moved"


def check_grouping(make, oracle):
    """case 4: k = 3 against k = 1 at (64, 199): R = 6; over 13 calls of 3 blocks, two wraps of the ring, e, y and get_taps are
    bit-equal"""
    block, T, k = RING
    assert partitions(T, block) + k - 1 == 6
    x, d, _ = case(oracle, block, T, 3, 13 * k)
    got = []
    for kk in (k, 1):
        r = make(3, block, T, kk * block, MU, delta_for(block))
        e, y = r.process(x, d)
        got.append((e, y, r.get_taps()))
        r.close()
    for a, b, name in zip(got[0], got[1], ("e", "y", "taps")):
        assert np.array_equal(bits(a), bits(b)), f"grouping: {name} differs between k = 3 and k = 1"


def check_isolation(make, oracle, nblocks=20):
    """case 5a: with the neighbours' x and d scaled by 2^20, zeroed or NaN, a channel's e and weights keep their bits"""
    block, T, _ = RING
    x, d, _ = case(oracle, block, T, 3, nblocks)
    mine = 1

    def run(xs, ds):
        r = make(3, block, T, 2 * block, MU, delta_for(block))
        with np.errstate(all="ignore"):
            e, y = r.process(xs, ds)
            w = r.get_taps()
        r.close()
        return e[mine], y[mine], w[mine]
    base = run(x, d)
    assert np.all(np.isfinite(base[0])) and np.any(base[2] != 0)
    for name, f in (("scaled by 2^20", lambda a: a * np.float32(2.0 ** 20)), ("zeroed", np.zeros_like),
                    ("NaN", lambda a: np.full_like(a, np.nan))):
        xs, ds = f(x), f(d)
        xs[mine], ds[mine] = x[mine], d[mine]
        for a, b, what in zip(run(xs, ds), base, ("e", "y", "taps")):
            assert np.array_equal(bits(a), bits(b)), f"isolation: neighbours {name} changed the channel's {what}"


def check_freeze_one(make, oracle, nblocks=30):
    """case 5b: a channel frozen by set_step while its neighbours adapt keeps get_taps bit for bit; unfrozen, it continues
    exactly as the model does (the float64 model on the same schedule, under the parity limits)"""
    block, T, _ = RING
    x, d, h = case(oracle, block, T, 3, nblocks)
    third = nblocks // 3 * block
    mine = 1
    runs = []
    for mk in (make, lambda *a: Model(*a, prec=64)):
        r = mk(3, block, T, block, MU, delta_for(block))
        e0, _ = r.process(x[:, :third], d[:, :third])
        w0 = r.get_taps()
        r.set_step(mine, 0.0)
        e1, _ = r.process(x[:, third:2 * third], d[:, third:2 * third])
        w1 = r.get_taps()
        r.set_step(mine, MU)
        e2, _ = r.process(x[:, 2 * third:3 * third], d[:, 2 * third:3 * third])
        w2 = r.get_taps()
        r.close()
        runs.append((np.concatenate([e0, e1, e2], axis=1), w0, w1, w2))
    (e, w0, w1, w2), (e_ref, _, w1_ref, w2_ref) = runs
    assert np.array_equal(bits(w0[mine]), bits(w1[mine])), "a frozen channel's taps moved"
    assert not np.array_equal(bits(w0[0]), bits(w1[0])) and not np.array_equal(bits(w1[mine]), bits(w2[mine]))
    ratio = block_rms(e.astype(np.float64) - e_ref, block) / (TOL * rms(d, axis=1)[:, None])
    hn = np.sqrt(np.sum(h * h, axis=1))
    tap = np.sqrt(np.sum((w2.astype(np.float64) - w2_ref) ** 2, axis=1)) / (TOL * hn)
    print(f"freeze and release: worst error ratio {ratio.max():.3g}, taps {tap.max():.3g}")
    assert ratio.max() <= 1.0 and tap.max() <= 1.0


def check_reset(make, oracle, nblocks=12):
    """case 6b, c: reset(clear_taps = 1) followed by the same input repeats a fresh handle's bits; reset(0) keeps get_taps"""
    block, T, _ = RING
    x, d, _ = case(oracle, block, T, 3, nblocks)
    r = make(3, block, T, 3 * block, MU, delta_for(block))
    e0, y0 = r.process(x, d)
    w0 = r.get_taps()
    r.reset(False)
    assert np.array_equal(bits(r.get_taps()), bits(w0)), "reset(0) changed the taps"
    r.reset(True)
    assert not np.any(r.get_taps()), "reset(1) left taps"
    e1, y1 = r.process(x, d)
    w1 = r.get_taps()
    r.close()
    for a, b, name in ((e0, e1, "e"), (y0, y1, "y"), (w0, w1, "taps")):
        assert np.array_equal(bits(a), bits(b)), f"reset(1): {name} differs from a fresh handle's"


def check_handover(make, stream_run, oracle, exact=True, nblocks=30):
    """case 6a: the taps an adapting handle hands over.  w = get_taps() goes to a FirStreamMC of the same block and, through
    set_taps, to the handle itself, frozen and with its delay line reset: the two outputs are bit-equal.  (The weights the
    handle KEEPS are 2 B float32 per partition where w has B: their output is not that of any float32 tap set to the bit; it
    is held to the gate against the stream convolver's here.)"""
    block, T, _ = RING
    x, d, _ = case(oracle, block, T, 3, nblocks)
    half = nblocks // 2 * block
    r = make(3, block, T, block, MU, delta_for(block))
    r.process(x[:, :half], d[:, :half])
    w = r.get_taps()
    r.set_step(0, np.zeros(3, np.float32))
    r.reset(False)
    _, y_kept = r.process(x[:, half:], d[:, half:])
    assert np.array_equal(bits(r.get_taps()), bits(w)), "a frozen handle's taps moved"
    r.reset(False)
    r.set_taps(0, w)
    _, y_set = r.process(x[:, half:], d[:, half:])
    r.close()
    ys = stream_run(x[:, half:], w, block)
    kept = np.max(rms(y_kept - ys, axis=1) / rms(ys, axis=1))
    print(f"hand-over: the kept weights' output against FirStreamMC(get_taps): {kept:.3g} relative rms ({kept / TOL:.3g} of the gate)")
    assert kept <= TOL
    if exact:
        assert np.array_equal(bits(y_set), bits(ys)), "hand-over: FirStreamMC(get_taps) differs from the frozen handle's y"
    else:
        assert np.all(rms(y_set - ys, axis=1) <= TOL * rms(ys, axis=1))


def check_partition_grouping(make, oracle):
    """how the update groups a channel's partitions into workgroups changes no bit: the WIDE case on its 37 channels (4107
    pairs: 4 partitions per workgroup) and its first 3 channels alone (333 pairs: one per workgroup) give those channels the same
    e, y and taps"""
    block, T, nblocks, channels = WIDE
    assert channels * partitions(T, block) >= 4096 > 3 * partitions(T, block) and partitions(T, block) % 4
    x, d, _ = case(oracle, block, T, channels, nblocks)
    got = []
    for ch in (channels, 3):
        r = make(ch, block, T, blocks_per_call(nblocks) * block, MU, delta_for(block))
        e, y = r.process(x[:ch], d[:ch])
        got.append((e[:3], y[:3], r.get_taps()[:3]))
        r.close()
    assert np.any(got[0][2] != 0)
    for a, b, name in zip(got[0], got[1], ("e", "y", "taps")):
        assert np.array_equal(bits(a), bits(b)), f"partition grouping: {name} differs between 37 and 3 channels"
