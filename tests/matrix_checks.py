"""Shared pieces of the matrix convolver's tests (test_fir_matrix_host.py, test_fir_matrix_gpu.py; llz_fir_matrix_mc, include/
llz_fir.h part 6: y_o = sum_i x_i * h[o][i]): the cases, their inputs and references (computed once and shared, never modified),
the two runners -- the device, and a numpy complex64 MODEL of the algorithm with its group order -- and the checks.  The limits
are the project's as they stand (tests/edge_checks.py, tests/part_checks.py) and carry no tolerance of their own:

  * dense: h[o][i] = edge_checks.dense_taps(T, seed(o, i)) / sqrt(inputs), rounded to float32, so that every output's row has
    unit norm; each output under edge_checks.rms_check (the 1e-5 gate), frames and flush apart, against the sum over inputs of
    the oracle's FIR on the zero-padded stream (part_checks.fft_ref at 131073 taps);
  * sparse: path (o, i) takes family (o + i) mod len of edge_checks.sparse_families(T); every sample of output o within
    sum_i part_checks.partition_limit(2 block, h[o][i], x_i) of the sum of edge_checks.fir_ref: each path is a partitioned
    overlap-save of its own, and the limits add.

The model is the algorithm, not the kernels: a ring of real-transform spectra per INPUT in complex64, the product summed in
complex64 over the inputs of a group ascending and p ascending within an input, the G partial spectra added g ascending, one
inverse real transform per output block.  G comes from groups(), the library's function of (inputs, outputs, block).  The model
sits at 0.0009 .. 0.015 of the limits; its planted faults (H indexed (i, o), a path one partition late, the last group left out
of the inverse's sum) miss them by more than 1e3."""
import numpy as np

from tests import edge_checks as ec
from tests import part_checks as pc
from tests import stream_checks as sc

MAX_TAPS = pc.MAX_TAPS
# (block, taps, inputs, outputs): the stream convolver's blocks and tap counts with inputs != outputs both ways; 37 -> 2 at block
# 64 runs in G = 19 groups of 2 with a last group of 1; 1 -> 2 is the smallest shape with G = 1
SHAPES = [(64, 1, 2, 2), (64, 65, 5, 3), (64, 199, 37, 2), (128, 199, 2, 37), (256, 700, 3, 5), (512, 513, 8, 2),
          (2048, 4100, 3, 2), (4096, 8200, 2, 3), (64, 65, 1, 2)]
LONGEST = (128, MAX_TAPS, 2, 2)
PASSES = (4096, 81921, 16, 8)     # a flush of 20 blocks against a partial-spectra scratch of 16 (64 MiB at G = 16, 8 outputs)
partitions = sc.partitions
calls_for = sc.calls_for
bits = sc.bits
padded = sc.padded
signal = sc.signal                  # [inputs, n] of the oracle's generator, input 1 scaled by 2^-10


def groups(inputs, outputs, block):
    """(G, inputs per group): llz_fir_matrix_host.c's firx_groups -- enough groups to bring the product to 1024 workgroups
    per block (outputs x bin tiles x groups), 32 at the most, of equal size but for a ragged last one"""
    rows = outputs * (block // 512 if block >= 1024 else 1)
    cap = min(-(-1024 // rows), 32, inputs)
    size = -(-inputs // cap)
    return -(-inputs // size), size


def seed(T, o, i):
    return T + 7919 * o + 31 * i


def dense_matrix(T, inputs, outputs):
    """[outputs, inputs, T] float64 holding float32 values: every path a Gaussian draw of its own, every row of unit norm"""
    def make():
        h = np.stack([np.stack([ec.dense_taps(T, seed(T, o, i)) for i in range(inputs)]) for o in range(outputs)])
        h = (h / np.sqrt(inputs)).astype(np.float32).astype(np.float64)
        h.setflags(write=False)
        return h
    return sc.cached(("mx-dense", T, inputs, outputs), make)


def sparse_matrix(T, inputs, outputs):
    fams = ec.sparse_families(T)
    h = np.stack([np.stack([fams[(o + i) % len(fams)][1] for i in range(inputs)]) for o in range(outputs)])
    h.setflags(write=False)
    return h


def fir1(oracle, xz, h):
    """one input row through one tap set in float64: the oracle's FIR, fft_ref where its loop is not affordable"""
    return (oracle.fir_batch_f32_mt(xz, h, threads=16) if len(h) <= 25249 else pc.fft_ref(xz, h))[0]


def dense_ref(oracle, x, h):
    """[outputs, n + T - 1] float64: sum over inputs of the oracle's FIR on the zero-padded stream; kept by the content"""
    import zlib

    def make():
        xz = padded(x, h.shape[2])
        ref = np.zeros((h.shape[0], xz.shape[1]))
        for o in range(h.shape[0]):
            for i in range(h.shape[1]):
                ref[o] += fir1(oracle, xz[i:i + 1], np.ascontiguousarray(h[o, i]))
        ref.setflags(write=False)
        return ref
    h = np.ascontiguousarray(h, dtype=np.float64)
    return sc.cached(("mx-ref", x.shape, h.shape, zlib.crc32(np.ascontiguousarray(x).tobytes()), zlib.crc32(h.tobytes())), make)


def sparse_ref(x, h, block):
    """(reference [outputs, n + T - 1], limit [outputs, 1]): the sums over inputs of fir_ref and of partition_limit"""
    xz = padded(x, h.shape[2])
    ref = np.zeros((h.shape[0], xz.shape[1]))
    lim = np.zeros((h.shape[0], 1))
    for o in range(h.shape[0]):
        for i in range(h.shape[1]):
            if np.any(h[o, i]):
                ref[o] += ec.fir_ref(xz[i:i + 1], h[o, i])[0][0]
                lim[o] += pc.partition_limit(2 * block, h[o, i], x[i:i + 1])[0]
    return ref, lim


# ------------------------------------------------------------------------------------------------ the model
def model(x, taps, block, k=1, fault=None):
    """x [inputs, calls * k * block] through the algorithm in float32 / complex64, then the flush: [outputs, n + T - 1] float32.
    taps: [outputs, inputs, T].  k only groups the blocks into calls: it cannot change a bit here either.  fault: None, or
    "transposed" (H indexed (i, o)), "late" (path (0, 0) applied one partition late), "group" (the last input group left out
    of the inverse's sum)"""
    x = np.asarray(x, dtype=np.float32)
    taps = np.asarray(taps, dtype=np.float32)
    I, n = x.shape
    O, T = taps.shape[0], taps.shape[2]
    assert taps.shape[1] == I and n % (k * block) == 0
    B, N, P = block, 2 * block, partitions(T, block)
    R = P + k - 1
    G, gs = groups(I, O, B)
    conn = np.any(taps != 0, axis=2)                                           # [O, I]
    hp = np.zeros((O, I, P * B), np.float64)
    hp[:, :, :T] = taps
    H = np.fft.rfft(hp.reshape(O, I, P, B), N, axis=3).astype(np.complex64)    # [O, I, P, B + 1]
    if fault == "transposed":
        H = np.ascontiguousarray(H.reshape(I, O, P, B + 1).transpose(1, 0, 2, 3))
        conn = np.ones_like(conn)
    if fault == "late":
        H[0, 0, 1:] = H[0, 0, :-1].copy()
        H[0, 0, 0] = 0
    ring = np.zeros((R, I, B + 1), np.complex64)
    prev = np.zeros((I, B), np.float32)
    out = np.empty((O, n + T - 1), np.float32)

    def product(head, first):
        """[O, B + 1]: per group the sum over its connected inputs ascending and p >= first ascending of ring_i[head - p]
        H[o][i][p] (numpy reduces a leading axis row by row), then the groups' partials, g ascending"""
        slots = (head - np.arange(first, P)) % R
        X = np.moveaxis(ring[slots], 0, 1)                                      # [I, P', B + 1]
        parts = []
        for g in range(G - 1 if fault == "group" else G):
            ii = slice(g * gs, min((g + 1) * gs, I))
            t = np.where(conn[:, ii, None, None], H[:, ii, first:] * X[None, ii], np.complex64(0))
            parts.append(np.add.reduce(np.moveaxis(t.reshape(O, -1, B + 1), 1, 0), axis=0, dtype=np.complex64))
        return np.add.reduce(np.stack(parts), axis=0, dtype=np.complex64)

    head = 0
    with np.errstate(invalid="ignore"):
        for j in range(n // B):
            cur = x[:, j * B:(j + 1) * B]
            ring[head] = np.fft.rfft(np.concatenate([prev, cur], axis=1), axis=1).astype(np.complex64)
            out[:, j * B:(j + 1) * B] = np.fft.irfft(product(head, 0), N, axis=1)[:, B:].astype(np.float32)
            prev = cur
            head = (head + 1) % R
        # flush: the spectrum of (last block, zeros) goes into slot `head`; block j meets it at p = j
        keep = T - 1
        ring[head] = np.fft.rfft(np.concatenate([prev, np.zeros_like(prev)], axis=1), axis=1).astype(np.complex64)
        for j in range(-(-keep // B)):
            y = np.fft.irfft(product(head + j, j), N, axis=1)[:, B:].astype(np.float32)
            m = min(B, keep - j * B)
            out[:, n + j * B:n + j * B + m] = y[:, :m]
    return out


# ------------------------------------------------------------------------------------------------ the device
def expected_plan(block, T, inputs, outputs, k, taps=None):
    P = partitions(T, block)
    paths = inputs * outputs if taps is None else int(np.count_nonzero(np.any(np.asarray(taps, dtype=np.float32) != 0, axis=2)))
    return (2 * block, P, P + k - 1, k, groups(inputs, outputs, block)[0], paths)


def stream_calls(dev, f, x):
    """x through the handle f in calls of its frame_len: the list of output frames (outputs preset to NaN)"""
    import torch
    outs = []
    for s in range(0, x.shape[1], f.frame_len):
        xi = torch.from_numpy(np.ascontiguousarray(x[:, s:s + f.frame_len])).to(dev)
        yi = torch.full((f.outputs, f.frame_len), float("nan"), dtype=torch.float32, device=dev)
        f.filter(xi, yi)
        outs.append(yi.cpu().numpy())
    return outs


def flushed(dev, f):
    import torch
    tail = torch.full((f.outputs, f.flt_len - 1), float("nan"), dtype=torch.float32, device=dev)   # one tap: empty
    f.flush(tail)
    return tail.cpu().numpy()


def device(dev, x, taps, block, k=1):
    """the same stream through one llz_fir_matrix_mc handle in calls of k blocks (device tensors, outputs preset to NaN), then
    the flush: [outputs, n + T - 1] float32.  The plan is asserted"""
    from llzlab_amd import filters
    x = np.asarray(x, dtype=np.float32)
    O, I, T = np.shape(taps)
    f = filters.FirMatrixMC(I, O, block, taps, frame_len=k * block)
    assert f.plan() == expected_plan(block, T, I, O, k, taps), (f.plan(), expected_plan(block, T, I, O, k, taps))
    outs = stream_calls(dev, f, x) + [flushed(dev, f)]
    f.close()
    return np.concatenate(outs, axis=1)


# ------------------------------------------------------------------------------------------------ the cases
def case_signal(oracle, block, T, inputs, k=1, calls=None):
    calls = calls or calls_for(block, T, k)
    n = calls * k * block
    return signal(oracle, inputs, n, seed=1 + T + block), n


def check_dense(run, oracle, block, T, inputs, outputs, k=1, calls=None):
    """one case with dense taps through `run(x, taps, block, k)`; returns the worst ratio to the gate"""
    x, n = case_signal(oracle, block, T, inputs, k, calls)
    h = dense_matrix(T, inputs, outputs)
    y = run(x, h, block, k)
    assert y.shape == (outputs, n + T - 1) and y.dtype == np.float32
    what = f"matrix block {block} T={T} {inputs}->{outputs} k={k} dense"
    pc.check_dense(y, dense_ref(oracle, x, h), n, what)
    return y


def check_sparse(run, oracle, block, T, inputs, outputs, k=1, calls=None):
    x, n = case_signal(oracle, block, T, inputs, k, calls)
    h = sparse_matrix(T, inputs, outputs)
    y = run(x, h, block, k)
    ref, lim = sparse_ref(x, h, block)
    pc.check_sparse(y, ref, lim, n, f"matrix block {block} T={T} {inputs}->{outputs} k={k} sparse", period=block)
    return y


def check_shape(run, oracle, block, T, inputs, outputs, k=1, calls=None):
    check_dense(run, oracle, block, T, inputs, outputs, k, calls)
    check_sparse(run, oracle, block, T, inputs, outputs, k, calls)


def dense_ratio(y, ref, n):
    """worst ratio of an output's error to the dense gate, frames and flush apart (what pc.check_dense asserts to be <= 1)"""
    worst = 0.0
    for o in range(y.shape[0]):
        for s in (slice(0, n), slice(n, None)):
            if y[o, s].size:
                d = np.asarray(y[o, s], dtype=np.float64) - ref[o, s]
                err = float(np.sqrt(np.mean(d ** 2)))
                worst = max(worst, err / ec.TOL, err / max(float(np.sqrt(np.mean(ref[o, s] ** 2))), 1e-30) / ec.TOL)
    return worst
