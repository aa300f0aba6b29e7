"""Shared pieces of the multi-reference adaptive filter's tests (test_adapt_matrix_host.py, test_adapt_matrix_gpu.py;
llz_adapt_matrix_mc, include/llz_adapt_matrix.h): the MODEL of the definition in float64 (the reference everywhere) and in
float32 / complex64 (the device's stand-in on a machine without a GPU), the cases, the runners and the checks.  The model is
written from the definition in llz_adapt_matrix.h in plain numpy rfft and knows nothing of the kernels: natural bin order, no
packing, no power-of-two rescaling, a shift register of spectra per input where the device has a ring.

The definition: I inputs, O outputs, block B, N = 2 B, P = ceil(T / B).  For block j: X_i = rfft(blocks (j - 1, j) of x_i);
Y_o = sum_i sum_p X_{i,j-p} W_{o,i,p}; y_o = the last B samples of irfft(Y_o); e_o = d_o - y_o; D = sum_i sum_p |X_{i,j-p}|^2;
where mu_o != 0: E_o = rfft([0_B, e_o]), G_o = mu_o E_o / (D + delta), and for every (i, p): dw = irfft(conj(X_{i,j-p}) G_o)
with every sample t >= min(B, T - p B) zeroed, W_{o,i,p} += rfft(dw).  In the float64 model the sum over inputs is a plain sum
(float64 is the reference); the float32 model follows the group order of the matrix convolver (matrix_checks.groups): per
group i ascending and p ascending within i, the group partials added g ascending.

Cases: white Gaussian references, independent per input (adapt_checks.gaussian); responses per path (adapt_checks.responses)
scaled by 1 / sqrt(inputs), so that every row of paths has unit norm; d_o = sum_i x_i * h[o][i].  delta = 1e-3 B I.

Limits -- K4h's (tests/adapt_checks.py), taken from the project, none from the device's results:
  * the error: per output and block rms(e - e_ref) <= TOL rms(d_o), TOL = edge_checks.TOL = 1e-5;
  * the taps: |w_o - w_ref,o|_2 <= TOL |h_o|_2 over the whole row of paths;
  * the misalignment |w_o - h_o|_2 at most max(2 x the float64 model's, the model's + TOL |h_o|_2);
  * convergence: the last block's error rms below a tenth of the first block's wherever the float64 model's is.
Block counts of shapes 1 and 2 (120 each) are chosen so that the float64 model converges on every output there; CONVERGING
names them and the parity check asserts that the set of converging outputs is not empty there."""
import numpy as np

from tests import adapt_checks as ac
from tests import edge_checks as ec
from tests import matrix_checks as mc

TOL = ec.TOL
MU = ac.MU
# (block, taps, inputs, outputs, blocks): the issue's table
SHAPES = [(64, 1, 2, 3, 120), (64, 199, 2, 3, 120), (64, 199, 3, 37, 24), (64, 70, 37, 2, 24), (64, 64, 2, 1024, 4),
          (128, 513, 5, 2, 16), (256, 2400, 2, 3, 12), (512, 1100, 2, 3, 12), (1024, 3500, 2, 2, 8), (2048, 2049, 2, 2, 8)]
CONVERGING = SHAPES[:2]         # the float64 model's error falls to a tenth on at least one output here
RING = (64, 199, 2, 3, 3)       # block, taps, inputs, outputs, k: R = P + k - 1 = 6
FAULT_SHAPES = [SHAPES[1], SHAPES[3]]
FAULTS = ("own_power", "transposed", "shifted_gradient", "unconstrained", "group")
partitions = ac.partitions
bits = ac.bits
rms = ac.rms
block_rms = ac.block_rms
cached = ac.cached


def delta_for(block, inputs):
    return 1e-3 * block * inputs


# ------------------------------------------------------------------------------------------------ the cases
def responses(inputs, outputs, T, seed):
    """[outputs, inputs, T] float64 (float32 values): adapt_checks.responses per path, over sqrt(inputs): unit-norm rows"""
    def make():
        h = np.stack([ac.responses(inputs, T, seed + 100003 * (o + 1)) for o in range(outputs)]) / np.sqrt(inputs)
        h = h.astype(np.float32).astype(np.float64)
        h.setflags(write=False)
        return h
    return cached(("xh", inputs, outputs, T, seed), make)


def case(oracle, block, T, inputs, outputs, nblocks):
    """(x, d, h): x [inputs, n] float32, h [outputs, inputs, T], d_o = sum_i x_i * h[o][i] truncated to n samples, float32"""
    def make():
        n = nblocks * block
        x = ac.gaussian(oracle, inputs, n, seed=23 + T + block + inputs)
        h = responses(inputs, outputs, T, seed=T + block)
        X = np.fft.rfft(x.astype(np.float64), 2 * n, axis=1)
        H = np.fft.rfft(h, 2 * n, axis=2)
        d = np.fft.irfft(np.einsum("if,oif->of", X, H), 2 * n, axis=1)[:, :n].astype(np.float32)
        d.setflags(write=False)
        return x, d, h
    return cached(("xcase", block, T, inputs, outputs, nblocks), make)


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """llz_adapt_matrix_mc from the definition.  prec: 64 (the reference) or 32 (float32 samples, complex64 spectra, the group
    order).  fault: None or one of FAULTS, for the tests that show the limits are not slack:
      own_power          each input normalised by its own power only
      transposed         W indexed (i, o) in the product
      shifted_gradient   input i's gradient applied to path i + 1 (cyclically)
      unconstrained      no gradient constraint
      group              the last input group left out of Y"""

    def __init__(self, inputs, outputs, block, T, frame_len=None, mu=MU, delta=None, prec=64, fault=None):
        assert fault is None or fault in FAULTS
        self.rt, self.ct = (np.float32, np.complex64) if prec == 32 else (np.float64, np.complex128)
        self.prec = prec
        self.I, self.O, self.B, self.T, self.P = inputs, outputs, block, T, partitions(T, block)
        self.delta = self.rt(delta_for(block, inputs) if delta is None else delta)
        self.mu = np.full(outputs, mu, self.rt)
        self.fault = fault
        self.G, self.gs = mc.groups(inputs, outputs, block)
        self.W = np.zeros((outputs, inputs, self.P, block + 1), self.ct)
        self.reset(False)

    def reset(self, clear_taps=False):
        self.X = np.zeros((self.I, self.P, self.B + 1), self.ct)          # X[:, p] = X_{j-p}
        self.prev = np.zeros((self.I, self.B), self.rt)
        if clear_taps:
            self.W[:] = 0

    def set_step(self, first, mu):
        mu = np.atleast_1d(np.asarray(mu, self.rt))
        self.mu[first:first + len(mu)] = mu

    def lim(self, p):
        return min(self.B, self.T - p * self.B)

    def set_taps(self, out_first, in_first, taps):
        taps = np.asarray(taps, np.float32).astype(np.float64)
        taps = taps[None, None, :] if taps.ndim == 1 else taps
        oc, ic = taps.shape[:2]
        hp = np.zeros((oc, ic, self.P * self.B))
        hp[:, :, :self.T] = taps
        self.W[out_first:out_first + oc, in_first:in_first + ic] = \
            np.fft.rfft(hp.reshape(oc, ic, self.P, self.B), 2 * self.B, axis=3).astype(self.ct)

    def get_taps64(self):
        w = np.fft.irfft(self.W.astype(np.complex128), 2 * self.B, axis=3)[:, :, :, :self.B].reshape(self.O, self.I, -1)
        return w[:, :, :self.T]

    def get_taps(self):
        return self.get_taps64().astype(np.float32)

    def process(self, x, d):
        """x [inputs, m B], d [outputs, m B] -> (e, y) float32"""
        B, rt = self.B, self.rt
        x, d = np.asarray(x, rt), np.asarray(d, rt)
        e, y = np.empty(d.shape, np.float32), np.empty(d.shape, np.float32)
        for j in range(x.shape[1] // B):
            e[:, j * B:(j + 1) * B], y[:, j * B:(j + 1) * B] = self.block(x[:, j * B:(j + 1) * B], d[:, j * B:(j + 1) * B])
        return e, y

    def product(self):
        X, W, ct = self.X, self.W, self.ct
        if self.fault == "transposed":
            W = W.reshape(self.I, self.O, self.P, self.B + 1).transpose(1, 0, 2, 3)
        if self.prec == 64 and self.fault is None:
            return np.einsum("ipb,oipb->ob", X, W)
        parts = []
        for g in range(self.G - 1 if (self.fault == "group" and self.G > 1) else self.G):
            ii = slice(g * self.gs, min((g + 1) * self.gs, self.I))
            t = (W[:, ii] * X[None, ii]).astype(ct).reshape(self.O, -1, self.B + 1)
            parts.append(np.add.reduce(np.moveaxis(t, 1, 0), axis=0, dtype=ct))      # i ascending, p ascending within i
        return np.add.reduce(np.stack(parts), axis=0, dtype=ct)                      # g ascending

    def block(self, xb, db):
        B, N, P, rt, ct = self.B, 2 * self.B, self.P, self.rt, self.ct
        self.X[:, 1:] = self.X[:, :-1].copy()
        self.X[:, 0] = np.fft.rfft(np.concatenate([self.prev, xb], axis=1), axis=1).astype(ct)
        self.prev = xb.copy()
        X = self.X
        yb = np.fft.irfft(self.product(), N, axis=1)[:, B:].astype(rt)
        eb = (db - yb).astype(rt)
        on = self.mu != 0
        if on.any():
            E = np.fft.rfft(np.concatenate([np.zeros_like(eb), eb], axis=1), axis=1).astype(ct)
            pw = (X.real ** 2 + X.imag ** 2).astype(rt)                                # [I, P, B + 1]
            if self.fault == "own_power":
                D = np.add.reduce(np.moveaxis(pw, 1, 0), axis=0, dtype=rt)[None]       # [1, I, B + 1]: every input its own
            else:
                D = np.add.reduce(pw.reshape(-1, B + 1), axis=0, dtype=rt)[None, None]  # i ascending, p ascending within i
            den = (D + self.delta).astype(rt)
            mu = self.mu[:, None, None]
            Eo = E[:, None]
            G = ((mu * Eo.real).astype(rt) / den + 1j * ((mu * Eo.imag).astype(rt) / den)).astype(ct)   # [O, 1 or I, B + 1]
            dW = (np.conj(X)[None] * G[:, :, None]).astype(ct)                         # [O, I, P, B + 1]
            if self.fault == "shifted_gradient":
                dW = np.roll(dW, 1, axis=1)
            if self.fault != "unconstrained":
                dw = np.fft.irfft(dW, N, axis=3).astype(rt)
                for p in range(P):
                    dw[:, :, p, self.lim(p):] = 0
                dW = np.fft.rfft(dw, axis=3).astype(ct)
            self.W[on] = (self.W[on] + dW[on]).astype(ct)
        return eb.astype(np.float32), yb.astype(np.float32)

    def close(self):
        pass


def model32(inputs, outputs, block, T, frame_len=None, mu=MU, delta=None):
    """the device's stand-in: the float32 model behind the runners' interface"""
    return Model(inputs, outputs, block, T, frame_len, mu, delta, prec=32)


def model64(inputs, outputs, block, T, frame_len=None, mu=MU, delta=None):
    return Model(inputs, outputs, block, T, frame_len, mu, delta, prec=64)


# ------------------------------------------------------------------------------------------------ the device
class Device:
    """filters.AdaptMatrixMC behind the model's interface: numpy in and out through device tensors, outputs preset to NaN"""

    def __init__(self, dev, inputs, outputs, block, T, frame_len=None, mu=MU, delta=None):
        from llzlab_amd import filters
        self.dev = dev
        self.f = filters.AdaptMatrixMC(inputs, outputs, block, T, frame_len=frame_len, mu=mu,
                                       delta=delta_for(block, inputs) if delta is None else delta)
        k = (frame_len or block) // block
        P = partitions(T, block)
        assert self.f.plan() == (2 * block, P, P + k - 1, k) + mc.groups(inputs, outputs, block), self.f.plan()

    def process(self, x, d, want_y=True):
        import torch
        n = self.f.frame_len
        es, ys = [], []
        for o in range(0, x.shape[1], n):
            xi = torch.from_numpy(np.ascontiguousarray(x[:, o:o + n], dtype=np.float32)).to(self.dev)
            di = torch.from_numpy(np.ascontiguousarray(d[:, o:o + n], dtype=np.float32)).to(self.dev)
            ei = torch.full_like(di, float("nan"))
            yi = torch.full_like(di, float("nan")) if want_y else None
            self.f.process(xi, di, ei, yi)
            es.append(ei.cpu().numpy())
            ys.append(yi.cpu().numpy() if want_y else None)
        return np.concatenate(es, axis=1), (np.concatenate(ys, axis=1) if want_y else None)

    def set_step(self, first, mu):
        self.f.set_step(first, mu)

    def set_taps(self, out_first, in_first, taps):
        self.f.set_taps(out_first, in_first, taps)

    def get_taps(self):
        return self.f.get_taps()

    def reset(self, clear_taps=False):
        self.f.reset(clear_taps)

    def close(self):
        self.f.close()


def device(dev):
    return lambda *a, **kw: Device(dev, *a, **kw)


# ------------------------------------------------------------------------------------------------ the checks
def row_norm(a):
    """|a_o|_2 over the whole row of paths: [outputs]"""
    a = np.asarray(a, np.float64)
    return np.sqrt(np.sum(a * a, axis=(1, 2)))


def reference(oracle, block, T, inputs, outputs, nblocks):
    """the float64 model over the whole case: (e, y, w, misalignment per output), computed once"""
    def make():
        x, d, h = case(oracle, block, T, inputs, outputs, nblocks)
        m = model64(inputs, outputs, block, T)
        e, y = m.process(x.astype(np.float64), d.astype(np.float64))
        w = m.get_taps64()
        return e, y, w, row_norm(w - h)
    return cached(("xref", block, T, inputs, outputs, nblocks), make)


def figures(e, w, d, h, e_ref, w_ref, mis_ref, block):
    """each figure as a ratio to its limit, and which outputs the reference converges on / the run converges on"""
    ratio = block_rms(e.astype(np.float64) - e_ref, block) / (TOL * rms(d, axis=1)[:, None])
    hn = row_norm(h)
    tap = row_norm(np.asarray(w, np.float64) - w_ref) / (TOL * hn)
    mis = row_norm(np.asarray(w, np.float64) - h)
    mis_ratio = mis / np.maximum(2.0 * mis_ref, mis_ref + TOL * hn)
    first, last = block_rms(e, block)[:, 0], block_rms(e, block)[:, -1]
    conv = block_rms(e_ref, block)[:, -1] < 0.1 * block_rms(e_ref, block)[:, 0]
    return ratio, tap, mis, mis_ratio, first, last, conv


def measure_parity(make, oracle, block, T, inputs, outputs, nblocks, mu=MU):
    """one case through `make(inputs, outputs, block, T, frame_len, mu, delta)` against the float64 model"""
    x, d, h = case(oracle, block, T, inputs, outputs, nblocks)
    e_ref, _, w_ref, mis_ref = reference(oracle, block, T, inputs, outputs, nblocks)
    what = f"adapt matrix block {block} T={T} {inputs}->{outputs} x {nblocks} blocks"
    r = make(inputs, outputs, block, T, ac.blocks_per_call(nblocks) * block, mu, delta_for(block, inputs))
    e, y = r.process(x, d)
    w = r.get_taps()
    r.close()
    assert e.shape == d.shape and e.dtype == np.float32 and w.shape == (outputs, inputs, T)
    assert np.array_equal(bits(e), bits(d - y)), f"{what}: e is not the float32 difference d - y"
    ratio, tap, mis, mis_ratio, first, last, conv = figures(e, w, d, h, e_ref, w_ref, mis_ref, block)
    o, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    out = {"error": float(ratio.max()), "taps": float(tap.max()), "misalignment": float(mis_ratio.max()),
           "converges": bool(np.all(last[conv] < 0.1 * first[conv])), "converging": int(conv.sum())}
    print(f"{what}: worst error ratio {out['error']:.3g} of the gate (output {o}, block {j}); taps {out['taps']:.3g} of theirs; "
          f"misalignment {mis.max():.3g} (model {mis_ref.max():.3g}), {out['misalignment']:.3g} of its limit; last / first error "
          f"rms {np.max(last / first):.3g}, {int(conv.sum())} of {outputs} outputs held to a tenth")
    return out


def check_parity(make, oracle, block, T, inputs, outputs, nblocks):
    what = f"adapt matrix block {block} T={T} {inputs}->{outputs}"
    m = measure_parity(make, oracle, block, T, inputs, outputs, nblocks)
    assert m["error"] <= 1.0, f"{what}: error at {m['error']:.3g} of the gate"
    assert m["taps"] <= 1.0, f"{what}: taps at {m['taps']:.3g} of their limit"
    assert m["misalignment"] <= 1.0, f"{what}: misalignment at {m['misalignment']:.3g} of its limit"
    assert m["converges"], f"{what}: the error does not fall where the model's does"
    if (block, T, inputs, outputs, nblocks) in CONVERGING:
        assert m["converging"] >= 1, f"{what}: the float64 model converges on no output: the convergence check is vacuous"
    return m


def worst_miss(make, oracle, block, T, inputs, outputs, nblocks):
    """the largest ratio of a figure to its limit (a run that ends in NaN or inf misses by inf)"""
    with np.errstate(all="ignore"):
        m = measure_parity(make, oracle, block, T, inputs, outputs, nblocks)
    worst = max(m["error"], m["taps"], m["misalignment"])
    return float("inf") if not np.isfinite(worst) else worst


def check_frozen(make, matrix_run, oracle, exact=True, shapes=SHAPES):
    """case 2: after set_taps(h) with every mu = 0, y is FirMatrixMC(inputs, outputs, block, h)'s on the same input -- bit for
    bit on the device (exact), to the gate between the two numpy models --, e is the float32 difference np.float32(d) - y, and
    get_taps is within 2 u |h_o| of h"""
    for block, T, inputs, outputs, _ in shapes:
        nblocks = partitions(T, block) + 3
        x, d, h = case(oracle, block, T, inputs, outputs, nblocks)
        r = make(inputs, outputs, block, T, block, 0.0, delta_for(block, inputs))
        r.set_taps(0, 0, h)
        e, y = r.process(x, d)
        w = r.get_taps()
        r.close()
        ym = matrix_run(x, h, block)
        what = f"frozen block {block} T={T} {inputs}->{outputs}"
        if exact:
            assert np.array_equal(bits(y), bits(ym)), f"{what}: {np.count_nonzero(bits(y) != bits(ym))} samples differ from FirMatrixMC's"
        else:
            assert np.all(rms(y - ym, axis=1) <= TOL * rms(ym, axis=1)), what
        assert np.array_equal(bits(e), bits(np.float32(d) - y)), f"{what}: e is not d - y"
        hn = np.sqrt(np.sum(h * h, axis=2))
        assert np.all(np.abs(w - h) <= 2 * ec.U * hn[:, :, None]), f"{what}: a frozen handle's taps moved"


def check_grouping(make, oracle):
    """case 4: k = 3 against k = 1 at (64, 199, 2 -> 3): R = 6; over 13 calls of 3 blocks, two wraps of the ring, e, y and
    get_taps are bit-equal"""
    block, T, inputs, outputs, k = RING
    assert partitions(T, block) + k - 1 == 6
    x, d, _ = case(oracle, block, T, inputs, outputs, 13 * k)
    got = []
    for kk in (k, 1):
        r = make(inputs, outputs, block, T, kk * block, MU, delta_for(block, inputs))
        e, y = r.process(x, d)
        got.append((e, y, r.get_taps()))
        r.close()
    assert np.any(got[0][2] != 0)
    for a, b, name in zip(got[0], got[1], ("e", "y", "taps")):
        assert np.array_equal(bits(a), bits(b)), f"grouping: {name} differs between k = 3 and k = 1"


def check_isolation(make, oracle, nblocks=20):
    """case 6a: with the other outputs' d scaled by 2^20, zeroed or NaN, an output's e, y and weights keep their bits"""
    block, T, inputs, outputs, _ = RING
    x, d, _ = case(oracle, block, T, inputs, outputs, nblocks)
    mine = 1

    def run(ds):
        r = make(inputs, outputs, block, T, 2 * block, MU, delta_for(block, inputs))
        with np.errstate(all="ignore"):
            e, y = r.process(x, ds)
            w = r.get_taps()
        r.close()
        return e[mine], y[mine], w[mine]
    base = run(d)
    assert np.all(np.isfinite(base[0])) and np.any(base[2] != 0)
    for name, f in (("scaled by 2^20", lambda a: a * np.float32(2.0 ** 20)), ("zeroed", np.zeros_like),
                    ("NaN", lambda a: np.full_like(a, np.nan))):
        ds = f(d)
        ds[mine] = d[mine]
        for a, b, what in zip(run(ds), base, ("e", "y", "taps")):
            assert np.array_equal(bits(a), bits(b)), f"isolation: the other outputs' d {name} changed the output's {what}"


def check_freeze_one(make, oracle, nblocks=30):
    """case 6b, c: an output frozen by set_step while the others adapt keeps get_taps bit for bit; released, it follows the
    float64 model on the same schedule under the parity limits"""
    block, T, inputs, outputs, _ = RING
    x, d, h = case(oracle, block, T, inputs, outputs, nblocks)
    third = nblocks // 3 * block
    mine = 1
    runs = []
    for mk in (make, model64):
        r = mk(inputs, outputs, block, T, block, MU, delta_for(block, inputs))
        e0, _ = r.process(x[:, :third], d[:, :third])
        w0 = r.get_taps()
        r.set_step(mine, 0.0)
        e1, _ = r.process(x[:, third:2 * third], d[:, third:2 * third])
        w1 = r.get_taps()
        r.set_step(mine, MU)
        e2, _ = r.process(x[:, 2 * third:3 * third], d[:, 2 * third:3 * third])
        w2 = r.get_taps64() if mk is model64 else r.get_taps()
        r.close()
        runs.append((np.concatenate([e0, e1, e2], axis=1), w0, w1, w2))
    (e, w0, w1, w2), (e_ref, _, _, w2_ref) = runs
    assert np.array_equal(bits(w0[mine]), bits(w1[mine])), "a frozen output's taps moved"
    assert not np.array_equal(bits(w0[0]), bits(w1[0])) and not np.array_equal(bits(w1[mine]), bits(w2[mine]))
    ratio = block_rms(e.astype(np.float64) - e_ref, block) / (TOL * rms(d, axis=1)[:, None])
    tap = row_norm(w2.astype(np.float64) - w2_ref) / (TOL * row_norm(h))
    print(f"freeze and release: worst error ratio {ratio.max():.3g}, taps {tap.max():.3g}")
    assert ratio.max() <= 1.0 and tap.max() <= 1.0


def check_reset(make, oracle, nblocks=12):
    """case 7b, c: reset(clear_taps = 1) followed by the same input repeats a fresh handle's bits; reset(0) keeps get_taps"""
    block, T, inputs, outputs, _ = RING
    x, d, _ = case(oracle, block, T, inputs, outputs, nblocks)
    r = make(inputs, outputs, block, T, 3 * block, MU, delta_for(block, inputs))
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


def check_handover(make, matrix_run, oracle, exact=True, nblocks=30):
    """case 7a: w = get_taps() goes to a FirMatrixMC of the same shape and, through set_taps, to the handle itself, frozen and
    with its delay lines reset: the two outputs are bit-equal.  (The weights the handle KEEPS are 2 B float32 per partition
    where w has B: their output is held to the gate against the matrix convolver's.)"""
    block, T, inputs, outputs, _ = RING
    x, d, _ = case(oracle, block, T, inputs, outputs, nblocks)
    half = nblocks // 2 * block
    r = make(inputs, outputs, block, T, block, MU, delta_for(block, inputs))
    r.process(x[:, :half], d[:, :half])
    w = r.get_taps()
    r.set_step(0, np.zeros(outputs, np.float32))
    r.reset(False)
    _, y_kept = r.process(x[:, half:], d[:, half:])
    assert np.array_equal(bits(r.get_taps()), bits(w)), "a frozen handle's taps moved"
    r.reset(False)
    r.set_taps(0, 0, w)
    _, y_set = r.process(x[:, half:], d[:, half:])
    r.close()
    ym = matrix_run(x[:, half:], w, block)
    kept = np.max(rms(y_kept - ym, axis=1) / rms(ym, axis=1))
    print(f"hand-over: the kept weights' output against FirMatrixMC(get_taps): {kept:.3g} relative rms ({kept / TOL:.3g} of the gate)")
    assert kept <= TOL
    if exact:
        assert np.array_equal(bits(y_set), bits(ym)), "hand-over: FirMatrixMC(get_taps) differs from the frozen handle's y"
    else:
        assert np.all(rms(y_set - ym, axis=1) <= TOL * rms(ym, axis=1))


def check_submatrix(make, oracle):
    """case 7d: set_taps of a sub-matrix touches only its own paths, and get_taps of it returns what went in within 2 u |h|"""
    block, T, inputs, outputs = 64, 199, 3, 4
    h = responses(inputs, outputs, T, seed=5)
    g = responses(2, 2, T, seed=77)
    r = make(inputs, outputs, block, T, block, 0.0, delta_for(block, inputs))
    r.set_taps(0, 0, h)
    w0 = r.get_taps()
    r.set_taps(1, 1, g)                                         # outputs 1, 2 x inputs 1, 2
    w1 = r.get_taps()
    r.close()
    inside = np.zeros((outputs, inputs), bool)
    inside[1:3, 1:3] = True
    assert np.array_equal(bits(w1[~inside]), bits(w0[~inside])), "a sub-matrix set_taps touched other paths"
    gn = np.sqrt(np.sum(g * g, axis=2))
    assert np.all(np.abs(w1[1:3, 1:3] - g) <= 2 * ec.U * gn[:, :, None]), "the sub-matrix did not come back"
    return w1
