"""Shared pieces of the stream convolver's crossfade tests (test_fir_fade_host.py, test_fir_fade_gpu.py; llz_fir_xfade_stream_mc,
include/llz_fir.h part 5): the cases, a numpy float32 MODEL of the algorithm, the two handles the cases are driven through -- the
model and the device, one interface -- and the checks.  The limits are the project's (tests/edge_checks.py, tests/part_checks.py)
carried through a linear blend, and carry no tolerance of their own.  With w in float64 -- 0 before the fade, n / (F B) inside
it, 1 after:

  * dense taps (edge_checks.dense_taps(T, seed=T) fading to (T, seed=T + 7)): ref = (1 - w) ref_old + w ref_new, both from
    stream_checks.dense_ref; edge_checks.rms_check, the 1e-5 gate, a channel at a time, over the frames before the fade, the
    fade span on its own, the frames after it and the flush;
  * sparse taps (pairs of distinct families of edge_checks.sparse_families(T), the i-th with the i-th from the end): every
    sample within (1 - w) partition_limit(2 B, h_old, x) + w partition_limit(2 B, h_new, x) + 3 u (|ref_old| + |ref_new|),
    u = 2^-24: the two filters' own limits through the blend, and the blend's three roundings (the difference, the product,
    the sum) of quantities bounded by |y_old| + |y_new|.

The model is the algorithm as stream_checks.model writes it -- complex64 ring, p ascending -- with both sums and a float32 blend
fmaf(w, y_new - y_old, y_old), w = float32(n) / float32(F B).  It can apply its ramp LATE (by samples), which is the planted
fault of the host tests."""
import numpy as np

from tests import edge_checks as ec
from tests import part_checks as pc
from tests import stream_checks as sc

# (block, taps, fade_blocks): stream_checks' corners -- one tap, a last partition holding one tap, one wave and several, threads
# owning 1, 2, 8 and 16 bins (one pass over the ring up to block 1024, two from 2048) -- with fades of one block and of several
SHAPES = [(64, 1, 1), (64, 65, 5), (64, 199, 3), (128, 199, 1), (512, 513, 2), (2048, 4100, 2), (4096, 8200, 1)]
CHANNELS = (3, 37)
MAX_FADE = 4096


def weights(total, start, span):
    """float64 [total]: 0 before sample `start`, (n - start) / span inside the fade, 1 from start + span on"""
    return np.clip((np.arange(total, dtype=np.float64) - start) / span, 0.0, 1.0)


def sparse_pairs(T):
    """[(name, old, new)]: the i-th family with the i-th from the end, equal pairs skipped"""
    fam = ec.sparse_families(T)
    out = []
    for i, (name, h) in enumerate(fam):
        other, g = fam[len(fam) - 1 - i]
        if not np.array_equal(h, g):
            out.append((f"{name}->{other}", h, g))
    return out


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """the handle's calls on numpy arrays, float32 / complex64.  late: the ramp applied that many samples late (a planted
    fault: w[n] = weight(n - late), 0 before)"""

    def __init__(self, channels, block, taps, k=1, late=0):
        taps = np.asarray(taps, dtype=np.float32)
        rows = taps[None, :] if taps.ndim == 1 else taps
        self.channels, self.B, self.k, self.T, self.late = channels, block, k, rows.shape[1], late
        self.rows = rows.shape[0]
        assert self.rows in (1, channels)
        self.P = sc.partitions(self.T, block)
        self.R = self.P + k - 1
        self.H = self._spectra(rows)
        self.Hn = self.H.copy()
        self.flag = np.zeros(self.rows, bool)
        self.F = self.done = 0
        self.reset()

    def _spectra(self, rows):
        """[P, rows, B + 1] complex64"""
        hp = np.zeros((rows.shape[0], self.P * self.B), np.float64)
        hp[:, :self.T] = rows
        H = np.fft.rfft(hp.reshape(rows.shape[0], self.P, self.B), 2 * self.B, axis=2).astype(np.complex64)
        return np.ascontiguousarray(np.moveaxis(H, 1, 0))

    def reset(self):
        if self.F:
            self._adopt()
        self.ring = np.zeros((self.R, self.channels, self.B + 1), np.complex64)
        self.prev = np.zeros((self.channels, self.B), np.float32)
        self.head = 0

    def _adopt(self):
        self.H = self.Hn.copy()
        self.flag[:] = False
        self.F = self.done = 0

    def set_taps(self, first, taps):
        assert not self.F, "set_taps is refused while a fade is in flight"
        taps = np.atleast_2d(np.asarray(taps, dtype=np.float32))
        self.H[:, first:first + len(taps)] = self._spectra(taps)
        self.Hn = self.H.copy()

    def fade(self, first, taps, F):
        assert 1 <= F <= MAX_FADE and (not self.F or (self.done == 0 and F == self.F)), "a fade is in flight"
        taps = np.atleast_2d(np.asarray(taps, dtype=np.float32))
        assert 0 <= first and first + len(taps) <= self.rows and taps.shape[1] == self.T
        self.Hn[:, first:first + len(taps)] = self._spectra(taps)
        self.flag[first:first + len(taps)] = True
        self.F, self.done = F, 0

    def left(self):
        return self.F - self.done if self.F else 0

    def _sum(self, H, lead, head, first):
        """lead + sum over p > first of ring[head - p] H_p, p ascending (numpy reduces a leading axis row by row)"""
        if first + 1 >= self.P:
            return lead
        slots = (head - np.arange(first + 1, self.P)) % self.R
        return np.add.reduce(np.concatenate([lead[None], self.ring[slots] * H[first + 1:]], axis=0), axis=0, dtype=np.complex64)

    def _out(self, X, head, first):
        """one block's B samples: X = the spectrum partition `first` meets, then the ring; blended while the fade runs"""
        B = self.B

        def y(H):
            return np.fft.irfft(self._sum(H, X * H[first], head, first), 2 * B, axis=1)[:, B:].astype(np.float32)
        if not self.F:
            return y(self.H)
        if self.done >= self.F:                                    # past the end inside a call: the new taps alone
            return y(self.Hn)
        yo, yn = y(self.H), y(self.Hn)
        n = np.maximum(self.done * B + np.arange(B) - self.late, 0)
        w = n.astype(np.float32) / np.float32(self.F * B)
        d = yn - yo                                                 # float32
        return (w.astype(np.float64)[None, :] * d.astype(np.float64) + yo.astype(np.float64)).astype(np.float32)

    def filter(self, x):
        x = np.asarray(x, dtype=np.float32)
        B = self.B
        assert x.shape == (self.channels, self.k * B)
        out = np.empty_like(x)
        for j in range(self.k):
            cur = x[:, j * B:(j + 1) * B]
            X = np.fft.rfft(np.concatenate([self.prev, cur], axis=1), axis=1).astype(np.complex64)
            self.ring[self.head] = X
            out[:, j * B:(j + 1) * B] = self._out(X, self.head, 0)
            self.prev = cur
            self.head = (self.head + 1) % self.R
            if self.F:
                self.done += 1
        if self.F and self.done >= self.F:
            self._adopt()
        return out

    def flush(self):
        """zero blocks: only the spectrum of (last block, zeros) is new, and block j meets it at p = j; the fade goes on"""
        keep, B = self.T - 1, self.B
        out = np.empty((self.channels, keep), np.float32)
        last = np.fft.rfft(np.concatenate([self.prev, np.zeros_like(self.prev)], axis=1), axis=1).astype(np.complex64)
        for j in range(-(-keep // B)):
            y = self._out(last, self.head + j, j)
            m = min(B, keep - j * B)
            out[:, j * B:j * B + m] = y[:, :m]
            if self.F:
                self.done += 1
        self.reset()
        return out

    def close(self):
        pass


def on_model(late=0):
    return lambda channels, block, taps, k=1: Model(channels, block, taps, k, late=late)


# ------------------------------------------------------------------------------------------------ the device
class Device:
    """the same calls on a filters.FirStreamMC: device tensors, outputs preset to NaN"""

    def __init__(self, dev, channels, block, taps, k=1):
        from llzlab_amd import filters
        self.dev, self.channels, self.T = dev, channels, np.shape(taps)[-1]
        self.f = filters.FirStreamMC(channels, block, taps, frame_len=k * block)

    def filter(self, x):
        import torch
        xi = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.dev)
        yi = torch.full_like(xi, float("nan"))
        self.f.filter(xi, yi)
        return yi.cpu().numpy()

    def flush(self):
        import torch
        tail = torch.full((self.channels, self.T - 1), float("nan"), dtype=torch.float32, device=self.dev)
        self.f.flush(tail)
        return tail.cpu().numpy()

    def fade(self, first, taps, F):
        self.f.fade_taps(first, taps, F)

    def set_taps(self, first, taps):
        self.f.set_taps(first, taps)

    def left(self):
        return self.f.fade_left()

    def reset(self):
        self.f.reset()

    def close(self):
        self.f.close()


def on_device(dev):
    return lambda channels, block, taps, k=1: Device(dev, channels, block, taps, k)


# ------------------------------------------------------------------------------------------------ the drivers
def run_fade(make, x, old, fades, block, F, start, k=1, flush=True, at_end=None):
    """x [channels, blocks * block] through one handle on `old` taps in calls of k blocks; before block `start` (a multiple of
    k) the calls fades = [(first, taps), ...] join one fade of F blocks; then the flush: [channels, n + T - 1] float32.
    at_end(handle) runs before the flush"""
    channels, n = x.shape
    assert start % k == 0 and n % (k * block) == 0
    h = make(channels, block, old, k)
    outs = []
    for o in range(0, n, k * block):
        if o == start * block:
            for first, taps in fades:
                h.fade(first, taps, F)
            assert h.left() == F
        outs.append(h.filter(x[:, o:o + k * block]))
    if at_end:
        at_end(h)
    if flush:
        outs.append(h.flush())
    h.close()
    return np.concatenate(outs, axis=1)


def blocks_for(block, T, F):
    """(start, blocks): the fade starts after P + 1 blocks and is followed by P + 2"""
    P = sc.partitions(T, block)
    return P + 1, P + 1 + F + P + 2


def check_dense(y, ref, start, span, n, what):
    """the 1e-5 gate a channel at a time over: the frames before the fade, the fade span on its own, the frames after it, the
    flush; returns the worst ratio to the gate"""
    assert y.shape == ref.shape and y.dtype == np.float32 and np.isfinite(y).all(), what
    worst = 0.0
    parts = [("before", 0, start), ("fade", start, start + span), ("after", start + span, n), ("flush", n, y.shape[1])]
    for c in range(y.shape[0]):
        for name, a, b in parts:
            if b > a:
                err, rel = ec.rms_check(y[c, a:b], ref[c, a:b], f"{what} ch {c} {name}")
                worst = max(worst, err / ec.TOL, rel / ec.TOL)
    return worst


def sparse_limit(w, h_old, h_new, x, ref_old, ref_new, block):
    return ((1.0 - w) * pc.partition_limit(2 * block, h_old, x) + w * pc.partition_limit(2 * block, h_new, x)
            + 3.0 * ec.U * (np.abs(ref_old) + np.abs(ref_new)))


def check_sparse(y, ref, lim, what, period):
    assert y.shape == ref.shape and y.dtype == np.float32 and np.isfinite(y).all(), what
    ec.sample_check(y, ref, lim, what, period=period)
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref) / lim))


def check_shape(make, oracle, block, T, F, channels, per_channel=False, k=1, start=None, blocks=None, families=("dense", "sparse")):
    """one (block, taps, fade_blocks, channels) case through handles of `make`: dense taps under the gate, the sparse pairs at
    every sample.  per_channel: the taps as [channels, T] rows (a bank of equal rows), all of them fading.  Prints and returns
    the worst ratios (dense, sparse)"""
    s0, b0 = blocks_for(block, T, F)
    start, blocks = s0 if start is None else start, b0 if blocks is None else blocks
    n = blocks * block
    x = sc.signal(oracle, channels, n, seed=1 + T + block)
    w = weights(n + T - 1, start * block, F * block)
    what = f"fade block {block} T={T} F={F} {channels}ch{' rows' if per_channel else ''} from block {start} of {blocks}, k={k}"

    def rows(h):
        return np.tile(h, (channels, 1)) if per_channel else h
    worst_d = worst_s = 0.0
    if "dense" in families:
        old, new = ec.dense_taps(T, seed=T), ec.dense_taps(T, seed=T + 7)
        y = run_fade(make, x, rows(old), [(0, rows(new))], block, F, start, k)
        ref = (1.0 - w) * sc.dense_ref(oracle, x, old) + w * sc.dense_ref(oracle, x, new)
        worst_d = check_dense(y, ref, start * block, F * block, n, f"{what} dense")
    if "sparse" in families:
        xz = sc.padded(x, T)
        for name, old, new in sparse_pairs(T):
            y = run_fade(make, x, rows(old), [(0, rows(new))], block, F, start, k)
            ro, rn = ec.fir_ref(xz, old)[0], ec.fir_ref(xz, new)[0]
            lim = sparse_limit(w, old, new, x, ro, rn, block)
            worst_s = max(worst_s, check_sparse(y, (1.0 - w) * ro + w * rn, lim, f"{what} {name}", block))
    print(f"{what}: worst ratio to the gate {worst_d:.3g}, to the sparse limit {worst_s:.3g}")
    return worst_d, worst_s


# ------------------------------------------------------------------------------------------------ bit pins and state
def pin_case(oracle, block, T, F, channels=3):
    """inputs of the bit pins: (x, old, new, start, blocks); start a multiple of 3 so that k = 3 handles can take it"""
    P = sc.partitions(T, block)
    start = 3 * (-(-(P + 1) // 3))
    blocks = 3 * (-(-(start + F + P + 2) // 3))
    x = sc.signal(oracle, channels, blocks * block, seed=23 + T + block)
    return x, ec.dense_taps(T, seed=T), ec.dense_taps(T, seed=T + 7), start, blocks


def check_bit_pins(make, oracle, block, T, F):
    """the first faded sample is the old filter's; a fade to equal taps changes no bit; every block after the fade has the bits
    of a handle given set_taps(new) at the block where the fade ends"""
    x, old, new, start, blocks = pin_case(oracle, block, T, F)
    n = blocks * block
    faded = run_fade(make, x, old, [(0, new)], block, F, start)
    plain = run_fade(make, x, old, [], block, F, -1)
    a = start * block
    assert np.array_equal(sc.bits(faded[:, :a + 1]), sc.bits(plain[:, :a + 1])), "the first faded sample is not the old filter's"
    assert pc.rel_rms(faded[:, a:a + F * block], plain[:, a:a + F * block]) > 1e3 * ec.TOL, "the fade changed nothing"
    same = run_fade(make, x, old, [(0, old)], block, F, start)
    assert np.array_equal(sc.bits(same), sc.bits(plain)), "a fade to equal taps changed bits"
    # set_taps(new) at the block where the fade ends
    h = make(x.shape[0], block, old, 1)
    outs = []
    for j in range(blocks):
        if j == start + F:
            h.set_taps(0, new)
        outs.append(h.filter(x[:, j * block:(j + 1) * block]))
    outs.append(h.flush())
    h.close()
    switched = np.concatenate(outs, axis=1)
    e = (start + F) * block
    assert np.array_equal(sc.bits(faded[:, e:]), sc.bits(switched[:, e:])), "after the fade the handle is not set_taps(new)'s"
    assert faded.shape == (x.shape[0], n + T - 1)


def check_call_grouping(make, oracle):
    """(64, 199, F = 4): with k = 3 the fade starts with one call and ends inside another; the bits are those of k = 1"""
    block, T, F = 64, 199, 4
    x, old, new, start, blocks = pin_case(oracle, block, T, F)
    assert start % 3 == 0 and blocks % 3 == 0 and F % 3
    y3 = run_fade(make, x, old, [(0, new)], block, F, start, k=3)
    y1 = run_fade(make, x, old, [(0, new)], block, F, start, k=1)
    assert np.isfinite(y3).all() and np.array_equal(sc.bits(y3), sc.bits(y1))


BANK_ROWS = (3, 4, 5, 20)


def check_bank_isolation(make, oracle, block=64, T=199, F=3):
    """37 channels, a row each; rows 3 .. 5 and 20 fade as two calls that join one pending fade.  Every other channel keeps the
    bits of a handle that never fades; neighbours scaled by 2^20 or zeroed change no bit of the fading rows"""
    channels = 37
    start, blocks = blocks_for(block, T, F)
    x = sc.signal(oracle, channels, blocks * block, seed=31 + T)
    old = np.stack([ec.dense_taps(T, seed=T + 17 * c) for c in range(channels)])
    new = np.stack([ec.dense_taps(T, seed=T + 17 * c + 5) for c in range(channels)])
    fades = [(3, new[3:6]), (20, new[20:21])]
    plain = run_fade(make, x, old, [], block, F, -1)
    faded = run_fade(make, x, old, fades, block, F, start)
    others = [c for c in range(channels) if c not in BANK_ROWS]
    assert np.array_equal(sc.bits(faded[others]), sc.bits(plain[others])), "a channel that does not fade changed bits"
    n, a, e = blocks * block, start * block, (start + F) * block
    w = weights(n + T - 1, a, F * block)
    xz = sc.padded(x, T)
    for c in BANK_ROWS:
        assert np.array_equal(sc.bits(faded[c, :a + 1]), sc.bits(plain[c, :a + 1]))
        ref = (1.0 - w) * oracle.fir_batch_f32(xz[c:c + 1], old[c]) + w * oracle.fir_batch_f32(xz[c:c + 1], new[c])
        check_dense(faded[c:c + 1], ref, a, F * block, n, f"bank row {c}")
        assert pc.rel_rms(faded[c, e:n], plain[c, e:n]) > 1e3 * ec.TOL, f"row {c} did not change its taps"
    xb = x.copy()
    xb[[2, 19]] *= np.float32(2.0 ** 20)
    xb[[6, 21]] = 0.0
    fb = run_fade(make, xb, old, fades, block, F, start)
    assert np.array_equal(sc.bits(fb[list(BANK_ROWS)]), sc.bits(faded[list(BANK_ROWS)])), "fading rows changed with neighbours"
    assert np.all(fb[[6, 21]] == 0.0)


def check_state(make, oracle, block=64, T=199, F=4):
    """fade_left counts down across calls; set_taps and a second fade are refused mid-fade and accepted after; reset mid-fade
    gives the bits of a fresh handle on the new taps"""
    from llzlab_amd.capi import LlzError
    x, old, new, _, blocks = pin_case(oracle, block, T, F)
    refusal = (LlzError, AssertionError)                           # the model asserts where the library refuses
    h = make(3, block, old, 1)
    assert h.left() == 0
    h.filter(x[:, :block])
    h.fade(0, new, F)
    assert h.left() == F
    h.fade(0, new, F)                                               # pending: the same length replaces rows
    for j in range(1, F):
        h.filter(x[:, j * block:(j + 1) * block])
        assert h.left() == F - j
        for call in (lambda: h.set_taps(0, old), lambda: h.fade(0, old, F), lambda: h.fade(0, old, F + 1)):
            try:
                call()
            except refusal as e:
                assert isinstance(e, AssertionError) or "in flight" in str(e), e
            else:
                raise AssertionError("accepted while a fade is in flight")
    h.reset()                                                       # mid-fade: the new taps at once
    assert h.left() == 0
    again = [h.filter(x[:, j * block:(j + 1) * block]) for j in range(blocks)] + [h.flush()]
    fresh = run_fade(make, x, new, [], block, F, -1)
    assert np.array_equal(sc.bits(np.concatenate(again, axis=1)), sc.bits(fresh)), "reset mid-fade is not a fresh handle on the new taps"
    h.fade(0, old, 1)                                               # accepted after; one block ends it
    h.filter(x[:, :block])
    assert h.left() == 0
    h.set_taps(0, new)
    h.fade(0, old, 2)
    h.close()                                                       # with a fade pending


def check_flush_mid_fade(make, oracle):
    """(64, 199, F = 6): two faded blocks, then the flush goes on with the ramp through its zero blocks (four of them, the
    fade's blocks 2 .. 5) under the sparse limit, and leaves a handle that repeats a fresh new-taps handle's bits"""
    block, T, F, start, blocks = 64, 199, 6, 3, 5
    n = blocks * block
    assert -(-(T - 1) // block) == 4 and start + 2 == blocks
    x = sc.signal(oracle, 3, n, seed=41 + T)
    w = weights(n + T - 1, start * block, F * block)
    assert w[-1] < 1.0                                              # the stream ends inside the fade
    xz = sc.padded(x, T)
    worst = 0.0
    for name, old, new in sparse_pairs(T):
        h = make(3, block, old, 1)
        outs = []
        for j in range(blocks):
            if j == start:
                h.fade(0, new, F)
            outs.append(h.filter(x[:, j * block:(j + 1) * block]))
        assert h.left() == F - 2
        outs.append(h.flush())
        assert h.left() == 0
        y = np.concatenate(outs, axis=1)
        ro, rn = ec.fir_ref(xz, old)[0], ec.fir_ref(xz, new)[0]
        lim = sparse_limit(w, old, new, x, ro, rn, block)
        worst = max(worst, check_sparse(y, (1.0 - w) * ro + w * rn, lim, f"flush mid-fade {name}", block))
        again = [h.filter(x[:, j * block:(j + 1) * block]) for j in range(blocks)] + [h.flush()]
        h.close()
        fresh = run_fade(make, x, new, [], block, F, -1)
        assert np.array_equal(sc.bits(np.concatenate(again, axis=1)), sc.bits(fresh)), "after the flush: not a fresh new-taps handle"
    print(f"flush mid-fade: worst ratio to the sparse limit {worst:.3g}")
    return worst
