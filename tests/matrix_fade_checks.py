"""Shared pieces of the matrix convolver's crossfade tests (test_fir_matrix_fade_host.py, test_fir_matrix_fade_gpu.py;
llz_fir_xfade_matrix_mc, include/llz_fir.h part 6): the cases, a numpy MODEL of the algorithm, the two handles the cases are driven
through -- the model and the device, one interface -- and the checks.  The limits are the project's (tests/edge_checks.py,
tests/part_checks.py, tests/matrix_checks.py) carried through a linear blend as tests/fade_checks.py carries them, and carry no
tolerance of their own.  With w in float64 -- 0 before the fade, (n - start) / (F B) inside it, 1 after (fade_checks.weights):

  * dense: old taps matrix_checks.dense_matrix(T, I, O); new taps the same matrix with the faded paths drawn as
    edge_checks.dense_taps(T, matrix_checks.seed(T, o, i) + 7) / sqrt(I), rounded to float32; ref = (1 - w) ref_old + w ref_new,
    both from matrix_checks.dense_ref; each output under edge_checks.rms_check over four spans apart: before, the fade span,
    after, the flush;
  * sparse: old taps matrix_checks.sparse_matrix; a faded path (o, i) goes to family len - 1 - ((o + i) mod len) of
    edge_checks.sparse_families(T); in the faded column row 0's OLD taps are zero (the source fades in) and row 1's NEW taps are
    zero (it fades out); every sample of output o within
        (1 - w) sum_i partition_limit(2 B, h_old[o][i], x_i) + w sum_i partition_limit(2 B, h_new[o][i], x_i)
        + 3 u (|ref_old_o| + |ref_new_o|),  u = 2^-24:
    the two matrices' limits through the blend and the blend's three roundings, as fade_checks.sparse_limit argues.

The faded set of a shape is one whole column (input inputs - 1, all outputs) joined, as a second call into the pending fade, by
the lone path (outputs - 1, 0).  The fade starts after P + 1 blocks and P + 2 follow (fade_checks.blocks_for), then the flush.

The model is matrix_checks.model's algorithm -- complex64 rings per input, groups(), a group's inputs ascending, p ascending,
partials g ascending -- as a class with two tables of spectra and two connection tables, fade_checks.Model's float32 blend, and a
blend applied only to outputs that fade.  Its planted faults: `late`, the ramp late by that many samples, and "conn", the new sum
skipping paths by the OLD connection table, so that a source fading in never arrives."""
import numpy as np

from tests import edge_checks as ec
from tests import fade_checks as fc
from tests import matrix_checks as mc
from tests import part_checks as pc

# (block, taps, inputs, outputs, fade_blocks): one tap, a last partition of one tap, 19 groups with a ragged last one, groups of
# one input, one and two bins per thread of the product, several bin tiles, the largest LDS image; fades of one block and several
SHAPES = [(64, 1, 2, 2, 1), (64, 65, 5, 3, 5), (64, 199, 37, 2, 3), (128, 199, 2, 37, 1), (512, 513, 8, 2, 2),
          (2048, 4100, 3, 2, 2), (4096, 8200, 2, 3, 1)]
LONGEST = (128, mc.MAX_TAPS, 2, 2, 2)
FAULTS_AT = (64, 65, 5, 3, 5)
MAX_FADE = 4096
weights = fc.weights
blocks_for = fc.blocks_for
bits = mc.bits


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """the handle's calls on numpy arrays, float32 / complex64.  late: the ramp applied that many samples late; fault "conn":
    while the fade runs the new sum skips paths by the old connection table"""

    def __init__(self, inputs, outputs, block, taps, k=1, late=0, fault=None):
        taps = np.asarray(taps, dtype=np.float32)
        assert taps.shape[:2] == (outputs, inputs) and fault in (None, "conn")
        self.I, self.O, self.B, self.k, self.T, self.late, self.fault = inputs, outputs, block, k, taps.shape[2], late, fault
        self.P = mc.partitions(self.T, block)
        self.R = self.P + k - 1
        self.G, self.gs = mc.groups(inputs, outputs, block)
        self.H, self.conn = self._spectra(taps), np.any(taps != 0, axis=2)
        self.Hn, self.conn_new = self.H.copy(), self.conn.copy()
        self.flag = np.zeros((outputs, inputs), bool)
        self.F = self.done = 0
        self._mix = None
        self.reset()

    def _spectra(self, taps):
        """[o, i, T] -> [o, i, P, B + 1] complex64"""
        hp = np.zeros(taps.shape[:2] + (self.P * self.B,), np.float64)
        hp[:, :, :self.T] = taps
        return np.fft.rfft(hp.reshape(taps.shape[:2] + (self.P, self.B)), 2 * self.B, axis=3).astype(np.complex64)

    def _mixed(self):
        """the matrix as set_taps(new) would leave it: (spectra, connection table)"""
        if self._mix is None:
            self._mix = (np.where(self.flag[:, :, None, None], self.Hn, self.H), np.where(self.flag, self.conn_new, self.conn))
        return self._mix

    def _adopt(self):
        self.H, self.conn = self._mixed()
        self.flag = np.zeros_like(self.flag)
        self.F = self.done = 0
        self._mix = None

    def reset(self):
        if self.F:
            self._adopt()
        self.ring = np.zeros((self.R, self.I, self.B + 1), np.complex64)
        self.prev = np.zeros((self.I, self.B), np.float32)
        self.head = 0

    @staticmethod
    def _sub(taps):
        taps = np.asarray(taps, dtype=np.float32)
        return taps[None, None, :] if taps.ndim == 1 else taps

    def set_taps(self, out_first, in_first, taps):
        assert not self.F, "set_taps is refused while a fade is in flight"
        taps = self._sub(taps)
        oo, ii = slice(out_first, out_first + taps.shape[0]), slice(in_first, in_first + taps.shape[1])
        self.H = self.H.copy()
        self.conn = self.conn.copy()
        self.H[oo, ii] = self._spectra(taps)
        self.conn[oo, ii] = np.any(taps != 0, axis=2)

    def fade(self, out_first, in_first, taps, F):
        assert 1 <= F <= MAX_FADE and (not self.F or (self.done == 0 and F == self.F)), "a fade is in flight"
        taps = self._sub(taps)
        assert 0 <= out_first and out_first + taps.shape[0] <= self.O and 0 <= in_first and in_first + taps.shape[1] <= self.I
        assert taps.shape[2] == self.T
        oo, ii = slice(out_first, out_first + taps.shape[0]), slice(in_first, in_first + taps.shape[1])
        self.Hn[oo, ii] = self._spectra(taps)
        self.conn_new[oo, ii] = np.any(taps != 0, axis=2)
        self.flag[oo, ii] = True
        self.F, self.done, self._mix = F, 0, None

    def left(self):
        return self.F - self.done if self.F else 0

    def connected(self):
        """plan()[5]: the union of both tap sets' connected paths while a fade is pending or in flight"""
        return int(np.count_nonzero(self.conn | (self.flag & self.conn_new))) if self.F else int(np.count_nonzero(self.conn))

    def _product(self, H, conn, head, first):
        """matrix_checks.model's product: [O, B + 1]"""
        slots = (head - np.arange(first, self.P)) % self.R
        X = np.moveaxis(self.ring[slots], 0, 1)
        parts = []
        for g in range(self.G):
            ii = slice(g * self.gs, min((g + 1) * self.gs, self.I))
            t = np.where(conn[:, ii, None, None], H[:, ii, first:] * X[None, ii], np.complex64(0))
            parts.append(np.add.reduce(np.moveaxis(t.reshape(self.O, -1, self.B + 1), 1, 0), axis=0, dtype=np.complex64))
        return np.add.reduce(np.stack(parts), axis=0, dtype=np.complex64)

    def _out(self, head, first):
        """one block's B samples of every output, blended for the outputs that fade while the fade runs"""
        B = self.B

        def y(H, conn):
            return np.fft.irfft(self._product(H, conn, head, first), 2 * B, axis=1)[:, B:].astype(np.float32)
        if not self.F:
            return y(self.H, self.conn)
        Hm, cm = self._mixed()
        if self.fault == "conn":
            cm = self.conn
        if self.done >= self.F:                                    # past the end inside a call: the new taps alone
            return y(Hm, cm)
        yo, yn = y(self.H, self.conn), y(Hm, cm)
        n = np.maximum(self.done * B + np.arange(B) - self.late, 0)
        w = n.astype(np.float32) / np.float32(self.F * B)
        d = yn - yo                                                 # float32
        blend = (w.astype(np.float64)[None, :] * d.astype(np.float64) + yo.astype(np.float64)).astype(np.float32)
        return np.where(self.flag.any(axis=1)[:, None], blend, yo)

    def filter(self, x):
        x = np.asarray(x, dtype=np.float32)
        B = self.B
        assert x.shape == (self.I, self.k * B)
        out = np.empty((self.O, self.k * B), np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(self.k):
                cur = x[:, j * B:(j + 1) * B]
                self.ring[self.head] = np.fft.rfft(np.concatenate([self.prev, cur], axis=1), axis=1).astype(np.complex64)
                out[:, j * B:(j + 1) * B] = self._out(self.head, 0)
                self.prev = cur
                self.head = (self.head + 1) % self.R
                if self.F:
                    self.done += 1
        if self.F and self.done >= self.F:
            self._adopt()
        return out

    def flush(self):
        """zero blocks: the spectrum of (last block, zeros) goes into slot `head`, block j meets it at p = j; the fade goes on"""
        keep, B = self.T - 1, self.B
        out = np.empty((self.O, keep), np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            self.ring[self.head] = np.fft.rfft(np.concatenate([self.prev, np.zeros_like(self.prev)], axis=1), axis=1).astype(np.complex64)
            for j in range(-(-keep // B)):
                y = self._out(self.head + j, j)
                m = min(B, keep - j * B)
                out[:, j * B:j * B + m] = y[:, :m]
                if self.F:
                    self.done += 1
        self.reset()
        return out

    def close(self):
        pass


def on_model(late=0, fault=None):
    return lambda inputs, outputs, block, taps, k=1: Model(inputs, outputs, block, taps, k, late=late, fault=fault)


# ------------------------------------------------------------------------------------------------ the device
class Device:
    """the same calls on a filters.FirMatrixMC: device tensors, outputs preset to NaN"""

    def __init__(self, dev, inputs, outputs, block, taps, k=1):
        from llzlab_amd import filters
        self.dev, self.O, self.T = dev, outputs, np.shape(taps)[-1]
        self.f = filters.FirMatrixMC(inputs, outputs, block, taps, frame_len=k * block)

    def filter(self, x):
        import torch
        xi = torch.from_numpy(np.array(x, dtype=np.float32)).to(self.dev)      # a copy: the cached signals are read-only
        yi = torch.full((self.O, xi.shape[1]), float("nan"), dtype=torch.float32, device=self.dev)
        self.f.filter(xi, yi)
        return yi.cpu().numpy()

    def flush(self):
        import torch
        tail = torch.full((self.O, self.T - 1), float("nan"), dtype=torch.float32, device=self.dev)
        self.f.flush(tail)
        return tail.cpu().numpy()

    def fade(self, out_first, in_first, taps, F):
        self.f.fade_taps(out_first, in_first, taps, F)

    def set_taps(self, out_first, in_first, taps):
        self.f.set_taps(out_first, in_first, taps)

    def left(self):
        return self.f.fade_left()

    def connected(self):
        return self.f.plan()[5]

    def reset(self):
        self.f.reset()

    def close(self):
        self.f.close()


def on_device(dev):
    return lambda inputs, outputs, block, taps, k=1: Device(dev, inputs, outputs, block, taps, k)


# ------------------------------------------------------------------------------------------------ the cases
def faded_calls(inputs, outputs):
    """[(out_first, in_first, out_count, in_count)]: the last column, then -- where there is another column -- one lone path"""
    return [(0, inputs - 1, outputs, 1)] + ([(outputs - 1, 0, 1, 1)] if inputs > 1 else [])


def paths_of(calls):
    return [(o, i) for of, inf, oc, ic in calls for o in range(of, of + oc) for i in range(inf, inf + ic)]


def fades_of(new, calls):
    """the calls as run_fade takes them: [(out_first, in_first, taps [out_count, in_count, T])]"""
    return [(of, inf, new[of:of + oc, inf:inf + ic]) for of, inf, oc, ic in calls]


def dense_pair(T, inputs, outputs, calls):
    old = mc.dense_matrix(T, inputs, outputs)
    new = old.copy()
    for o, i in paths_of(calls):
        new[o, i] = (ec.dense_taps(T, mc.seed(T, o, i) + 7) / np.sqrt(inputs)).astype(np.float32).astype(np.float64)
    return old, new


def sparse_pair(T, inputs, outputs, calls):
    """the column of calls[0]: row 0 fades in from zero taps, row 1 fades out to zero taps"""
    fams = ec.sparse_families(T)
    old = mc.sparse_matrix(T, inputs, outputs).copy()
    new = old.copy()
    for o, i in paths_of(calls):
        new[o, i] = fams[len(fams) - 1 - ((o + i) % len(fams))][1]
    col = calls[0][1]
    old[0, col] = 0.0
    new[1, col] = 0.0
    return old, new


def run_fade(make, x, old, fades, block, F, start, k=1, flush=True, at_end=None):
    """x [inputs, blocks * block] through one handle on `old` taps in calls of k blocks; before block `start` (a multiple of k)
    the calls fades = [(out_first, in_first, taps), ...] join one fade of F blocks; then the flush: [outputs, n + T - 1] float32.
    at_end(handle) runs before the flush"""
    inputs, n = x.shape
    assert start % k == 0 and n % (k * block) == 0
    h = make(inputs, np.shape(old)[0], block, old, k)
    outs = []
    for s in range(0, n, k * block):
        if s == start * block:
            for of, inf, taps in fades:
                h.fade(of, inf, taps, F)
            assert h.left() == F
        outs.append(h.filter(x[:, s:s + k * block]))
    if at_end:
        at_end(h)
    if flush:
        outs.append(h.flush())
    h.close()
    return np.concatenate(outs, axis=1)


def sparse_limit(w, x, old, new, block):
    """(reference, limit) [outputs, n + T - 1]: the two matrices' references and limits through the blend, and the blend's own
    three roundings"""
    ro, lo = mc.sparse_ref(x, old, block)
    rn, ln = mc.sparse_ref(x, new, block)
    return (1.0 - w) * ro + w * rn, (1.0 - w) * lo + w * ln + 3.0 * ec.U * (np.abs(ro) + np.abs(rn))


def dense_blend(oracle, w, x, old, new):
    return (1.0 - w) * mc.dense_ref(oracle, x, old) + w * mc.dense_ref(oracle, x, new)


def check_shape(make, oracle, block, T, inputs, outputs, F, k=1, start=None, blocks=None, families=("dense", "sparse")):
    """one (block, taps, inputs, outputs, fade_blocks) case through handles of `make`.  Prints and returns the worst ratios
    (dense gate, sparse limit)"""
    s0, b0 = blocks_for(block, T, F)
    start, blocks = s0 if start is None else start, b0 if blocks is None else blocks
    n = blocks * block
    x = mc.signal(oracle, inputs, n, seed=1 + T + block)
    w = weights(n + T - 1, start * block, F * block)
    calls = faded_calls(inputs, outputs)
    what = f"matrix fade block {block} T={T} {inputs}->{outputs} F={F} from block {start} of {blocks}, k={k}"
    worst_d = worst_s = 0.0
    if "dense" in families:
        old, new = dense_pair(T, inputs, outputs, calls)
        y = run_fade(make, x, old, fades_of(new, calls), block, F, start, k)
        assert y.shape == (outputs, n + T - 1)
        worst_d = fc.check_dense(y, dense_blend(oracle, w, x, old, new), start * block, F * block, n, f"{what} dense")
    if "sparse" in families:
        old, new = sparse_pair(T, inputs, outputs, calls)
        y = run_fade(make, x, old, fades_of(new, calls), block, F, start, k)
        ref, lim = sparse_limit(w, x, old, new, block)
        worst_s = fc.check_sparse(y, ref, lim, f"{what} sparse", block)
    print(f"{what}: worst ratio to the gate {worst_d:.3g}, to the sparse limit {worst_s:.3g}")
    return worst_d, worst_s


# ------------------------------------------------------------------------------------------------ bit pins
def pin_case(oracle, block, T, F, inputs=3, outputs=2):
    """3 -> 2 with column 1 fading: (x, old, new, fades, start, blocks); start a multiple of 3 so that k = 3 handles can take it.
    The generator's quiet row (2^-10) goes to input 0, so that the fading column carries a full-scale source"""
    P = mc.partitions(T, block)
    start = 3 * (-(-(P + 1) // 3))
    blocks = 3 * (-(-(start + F + P + 2) // 3))
    x = np.ascontiguousarray(mc.signal(oracle, inputs, blocks * block, seed=23 + T + block)[[1, 0] + list(range(2, inputs))])
    calls = [(0, 1, outputs, 1)]
    old, new = dense_pair(T, inputs, outputs, calls)
    return x, old, new, fades_of(new, calls), start, blocks


def check_bit_pins(make, oracle, block, T, F=3):
    """up to and including the first faded sample the never-fading handle's bits; a fade to equal taps changes no bit; from the
    fade's end on the bits of a handle given set_taps(new) at the block where the fade ends"""
    x, old, new, fades, start, blocks = pin_case(oracle, block, T, F)
    n = blocks * block
    faded = run_fade(make, x, old, fades, block, F, start)
    plain = run_fade(make, x, old, [], block, F, -1)
    a, e = start * block, (start + F) * block
    assert faded.shape == (2, n + T - 1) and np.isfinite(faded).all()
    assert np.array_equal(bits(faded[:, :a + 1]), bits(plain[:, :a + 1])), "the first faded sample is not the old matrix's"
    for o in range(2):
        assert pc.rel_rms(faded[o, a:e], plain[o, a:e]) > 1e3 * ec.TOL, f"output {o}: the fade changed nothing"
    same = run_fade(make, x, old, [(0, 1, old[:, 1:2])], block, F, start)
    assert np.array_equal(bits(same), bits(plain)), "a fade to equal taps changed bits"
    h = make(3, 2, block, old, 1)
    outs = []
    for j in range(blocks):
        if j == start + F:
            h.set_taps(0, 1, new[:, 1:2])
        outs.append(h.filter(x[:, j * block:(j + 1) * block]))
    outs.append(h.flush())
    h.close()
    switched = np.concatenate(outs, axis=1)
    assert np.array_equal(bits(faded[:, e:]), bits(switched[:, e:])), "after the fade the handle is not set_taps(new)'s"


def check_call_grouping(make, oracle):
    """(64, 199, F = 4, 3 -> 2): with k = 3 the fade starts with one call and ends inside another; the bits are those of k = 1"""
    block, T, F = 64, 199, 4
    x, old, new, fades, start, blocks = pin_case(oracle, block, T, F)
    assert start % 3 == 0 and blocks % 3 == 0 and F % 3
    y3 = run_fade(make, x, old, fades, block, F, start, k=3)
    y1 = run_fade(make, x, old, fades, block, F, start, k=1)
    assert np.isfinite(y3).all() and np.array_equal(bits(y3), bits(y1))


def check_one_path_is_the_stream_fade(make, make_stream, oracle, block, T, F=3):
    """3 -> 2: with every input but i zeroed and path (o, i) fading, output o equals -- value for value -- a one-channel stream
    convolver on x_i given the same fade at the same block"""
    x, old, new, _, start, blocks = pin_case(oracle, block, T, F)
    new = dense_pair(T, 3, 2, [(0, 0, 2, 3)])[1]                   # a new draw for every path
    for i in range(3):
        xi = np.zeros_like(x)
        xi[i] = x[i]
        plain = run_fade(make, xi, old, [], block, F, -1)
        e = (start + F) * block
        for o in range(2):
            y = run_fade(make, xi, old, [(o, i, new[o:o + 1, i:i + 1])], block, F, start)
            one = fc.run_fade(make_stream, x[i:i + 1], old[o, i], [(0, new[o, i])], block, F, start)
            assert np.isfinite(y[o]).all() and np.all(y[o] == one[0]), f"path ({o}, {i}) does not fade as the stream convolver"
            assert pc.rel_rms(y[o, e:], plain[o, e:]) > 1e3 * ec.TOL, f"path ({o}, {i}) did not change its taps"


ALONE = ((3, 2), (4, 2), (5, 2), (20, 4))      # the paths of check_outputs_fade_alone
ALTERED = (0, 1, 3)                            # the inputs it alters


def check_outputs_fade_alone(make, oracle, block=64, T=199, F=3):
    """5 -> 37: the paths (3..5, 2) and (20, 4) fade as two calls joining one pending fade.  Every other output keeps the bits of a
    handle that never fades; the fading outputs, whose paths from inputs 0, 1 and 3 are unconnected, keep every bit when inputs
    0 and 1 are scaled by 2^20 and input 3 is zeroed"""
    inputs, outputs = 5, 37
    rows = sorted({o for o, _ in ALONE})
    start, blocks = blocks_for(block, T, F)
    n, a, e = blocks * block, start * block, (start + F) * block
    x = mc.signal(oracle, inputs, n, seed=31 + T)
    calls = [(3, 2, 3, 1), (20, 4, 1, 1)]
    assert tuple(paths_of(calls)) == ALONE
    old, new = dense_pair(T, inputs, outputs, calls)
    old, new = old.copy(), new.copy()
    for o in rows:
        old[o, list(ALTERED)] = 0.0
        new[o, list(ALTERED)] = 0.0
    fades = fades_of(new, calls)
    plain = run_fade(make, x, old, [], block, F, -1)
    faded = run_fade(make, x, old, fades, block, F, start)
    others = [o for o in range(outputs) if o not in rows]
    assert np.isfinite(faded).all()
    assert np.array_equal(bits(faded[others]), bits(plain[others])), "an output that does not fade changed bits"
    w = weights(n + T - 1, a, F * block)
    ref = dense_blend(oracle, w, x, old, new)
    for o in rows:
        assert np.array_equal(bits(faded[o, :a + 1]), bits(plain[o, :a + 1]))
        fc.check_dense(faded[o:o + 1], ref[o:o + 1], a, F * block, n, f"fading output {o}")
        assert pc.rel_rms(faded[o, e:n], plain[o, e:n]) > 1e3 * ec.TOL, f"output {o} did not change its taps"
    xb = x.copy()
    xb[[0, 1]] *= np.float32(2.0 ** 20)
    xb[3] = 0.0
    fb = run_fade(make, xb, old, fades, block, F, start)
    assert np.array_equal(bits(fb[rows]), bits(faded[rows])), "fading outputs changed with inputs they are not connected to"


def check_fade_in_and_out(make, oracle, block=64, T=199, F=3):
    """3 -> 2, sparse taps.  Path (0, 2) has zero old taps and fades IN: a NaN block of x_2 before the fade does not reach output
    0, after it output 0 carries the source within the sparse limit.  Then path (1, 2) fades OUT to zero taps: afterwards NaN
    and Inf blocks of x_2 do not reach output 1, and the connected paths have dropped by one.  While either fade is pending or
    runs the count is the union's.  Returns the worst ratio to the sparse limit"""
    inputs, outputs = 3, 2
    P = mc.partitions(T, block)
    s1 = P + 1                                  # fade in: blocks s1 .. s1 + F - 1
    s2 = s1 + F + P + 1                         # fade out: blocks s2 .. s2 + F - 1
    bad = s2 + F                                # a NaN block, then an Inf block, of x_2
    blocks = bad + 2 + P + 2
    n = blocks * block
    fams = ec.sparse_families(T)
    old = mc.sparse_matrix(T, inputs, outputs).copy()
    old[0, 2] = 0.0
    mid = old.copy()
    mid[0, 2] = fams[0][1]
    new = mid.copy()
    new[1, 2] = 0.0
    clean = mc.signal(oracle, inputs, n, seed=47 + T).copy()
    x = clean.copy()
    for blk, v in ((0, np.nan), (bad, np.nan), (bad + 1, np.inf)):
        clean[2, blk * block:(blk + 1) * block] = 0.0
        x[2, blk * block:(blk + 1) * block] = v
    full = int(np.count_nonzero(np.any(mid != 0, axis=2)))
    h = make(inputs, outputs, block, old, 1)
    assert h.connected() == full - 1
    outs = []
    for j in range(blocks):
        if j == s1:
            h.fade(0, 2, mid[0, 2], F)
            assert h.connected() == full and h.left() == F          # the union, pending
        if j == s1 + 1:
            assert h.connected() == full and h.left() == F - 1      # in flight
        if j == s2:
            assert h.connected() == full and h.left() == 0
            h.fade(1, 2, new[1, 2], F)
            assert h.connected() == full                            # the union: the path still feeds the old sum
        if j == s2 + F:
            assert h.connected() == full - 1 and h.left() == 0      # faded out: one path less
        outs.append(h.filter(x[:, j * block:(j + 1) * block]))
    outs.append(h.flush())
    assert h.connected() == full - 1
    h.close()
    y = np.concatenate(outs, axis=1)
    w1 = weights(n + T - 1, s1 * block, F * block)
    w2 = weights(n + T - 1, s2 * block, F * block)
    worst = 0.0
    # output 0: nothing of the NaN block 0 (its path is unconnected until block s1, when that block has left the delay line);
    # from block `bad` on its connected path (0, 2) carries the NaN
    ref, lim = sparse_limit(w1, clean, old, mid, block)
    e0 = bad * block
    assert np.isfinite(y[0, :e0]).all(), "a NaN reached output 0 through a path with zero old taps"
    worst = max(worst, fc.check_sparse(y[0:1, :e0], ref[0:1, :e0], lim[0:1, :e0], "fade in: output 0", block))
    assert np.isnan(y[0, e0:e0 + block]).all(), "after the fade in, path (0, 2) carries nothing"
    assert pc.rel_rms(y[0, (s1 + F) * block:e0], mc.sparse_ref(clean, old, block)[0][0, (s1 + F) * block:e0]) > 1e3 * ec.TOL
    # output 1: connected to x_2 until the fade out is over: NaN at block 0, finite from block s1 on, the later NaN and Inf
    # blocks included
    ref, lim = sparse_limit(w2, clean, mid, new, block)
    a1 = s1 * block
    assert np.isnan(y[1, :block]).all()
    assert np.isfinite(y[1, a1:]).all(), "a NaN or an Inf reached output 1 through a path that had faded out"
    worst = max(worst, fc.check_sparse(y[1:2, a1:], ref[1:2, a1:], lim[1:2, a1:], "fade out: output 1", block))
    print(f"fade in and out: worst ratio to the sparse limit {worst:.3g}")
    return worst


# ------------------------------------------------------------------------------------------------ state
def check_state(make, oracle, block=64, T=199, F=4):
    """fade_left counts down across calls; set_taps, a second fade and a second fade of another length are refused mid-fade with
    "in flight" and accepted after; reset mid-fade gives the bits of a fresh handle on the new taps; close with a fade pending"""
    from llzlab_amd.capi import LlzError
    x, old, new, fades, _, blocks = pin_case(oracle, block, T, F)
    col_new, col_old = new[:, 1:2], old[:, 1:2]
    refusal = (LlzError, AssertionError)                           # the model asserts where the library refuses
    h = make(3, 2, block, old, 1)
    assert h.left() == 0
    h.filter(x[:, :block])
    h.fade(0, 1, col_new, F)
    assert h.left() == F
    h.fade(0, 1, col_new, F)                                        # pending: the same length replaces paths
    h.fade(1, 0, new[1, 0], F)                                      # ... and adds a lone path (equal taps here)
    assert h.left() == F
    for j in range(1, F):
        h.filter(x[:, j * block:(j + 1) * block])
        assert h.left() == F - j
        for call in (lambda: h.set_taps(0, 1, col_old), lambda: h.fade(0, 1, col_old, F), lambda: h.fade(0, 1, col_old, F + 1)):
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
    assert np.array_equal(bits(np.concatenate(again, axis=1)), bits(fresh)), "reset mid-fade is not a fresh handle on the new taps"
    h.fade(0, 1, col_old, 1)                                        # accepted after; one block ends it
    h.filter(x[:, :block])
    assert h.left() == 0
    h.set_taps(0, 1, col_new)
    h.fade(0, 0, old, 2)                                            # every path
    h.close()                                                       # with a fade pending


def check_flush_mid_fade(make, oracle):
    """(64, 199, 3 -> 2, F = 6): two faded blocks, then the flush goes on with the ramp through its four zero blocks under the
    sparse limit, and leaves a handle that repeats a fresh new-taps handle's bits"""
    block, T, F, start, blocks = 64, 199, 6, 3, 5
    n = blocks * block
    assert -(-(T - 1) // block) == 4 and start + 2 == blocks
    x = mc.signal(oracle, 3, n, seed=41 + T)
    w = weights(n + T - 1, start * block, F * block)
    assert w[-1] < 1.0                                              # the stream ends inside the fade
    calls = faded_calls(3, 2)
    old, new = sparse_pair(T, 3, 2, calls)
    h = make(3, 2, block, old, 1)
    outs = []
    for j in range(blocks):
        if j == start:
            for of, inf, taps in fades_of(new, calls):
                h.fade(of, inf, taps, F)
        outs.append(h.filter(x[:, j * block:(j + 1) * block]))
    assert h.left() == F - 2
    outs.append(h.flush())
    assert h.left() == 0 and h.connected() == int(np.count_nonzero(np.any(new != 0, axis=2)))
    ref, lim = sparse_limit(w, x, old, new, block)
    worst = fc.check_sparse(np.concatenate(outs, axis=1), ref, lim, "matrix flush mid-fade", block)
    again = [h.filter(x[:, j * block:(j + 1) * block]) for j in range(blocks)] + [h.flush()]
    h.close()
    fresh = run_fade(make, x, new, [], block, F, -1)
    assert np.array_equal(bits(np.concatenate(again, axis=1)), bits(fresh)), "after the flush: not a fresh new-taps handle"
    print(f"matrix flush mid-fade: worst ratio to the sparse limit {worst:.3g}")
    return worst


def check_flush_in_passes(make, oracle, F=24):
    """matrix_checks.PASSES (4096, 81921, 16 -> 8): one call of one block with a one-column fade of F = 24 pending, then the
    flush's 20 blocks in passes of 16 and 4 while the ramp runs; the dense gate, the reference as test_flush_in_passes takes it"""
    block, T, inputs, outputs = mc.PASSES
    x, n = mc.case_signal(oracle, block, T, inputs, calls=1)
    assert n == block and -(-(T - 1) // block) == 20 and 1 + 20 < F
    calls = [(0, inputs - 1, outputs, 1)]
    old, new = dense_pair(T, inputs, outputs, calls)
    w = weights(n + T - 1, 0, F * block)
    y = run_fade(make, x, old, fades_of(new, calls), block, F, 0)
    worst = fc.check_dense(y, dense_blend(oracle, w, x, old, new), 0, F * block, n, "matrix fade, flush in passes")
    print(f"matrix fade, flush in passes: worst ratio to the gate {worst:.3g}")
    return worst
