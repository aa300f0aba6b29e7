"""Shared pieces of the stream convolver's tests (test_fir_stream_host.py, test_fir_stream_gpu.py; llz_fir_stream_mc, include/
llz_fir.h part 5): the cases, their inputs and references (computed once and shared, never modified), the two runners -- the
device, and a numpy float32 MODEL of the algorithm -- and the checks.  The limits are the project's as they stand
(tests/part_checks.py, tests/edge_checks.py) and carry no tolerance of their own:

  * dense taps (edge_checks.dense_taps): edge_checks.rms_check, the 1e-5 gate, a channel at a time, frames and flush apart,
    against the oracle's FIR (part_checks.fft_ref at 131073 taps, where the oracle's loop would take hours);
  * sparse taps (edge_checks.sparse_families): every sample within part_checks.partition_limit(2 block, h, x) of
    edge_checks.fir_ref: each partition is an N = 2 block-point overlap-save of its own taps.

The model is the algorithm, not the kernel: a ring of real-transform spectra of (previous block, block) per channel in
complex64, the product summed over p ascending in complex64, the inverse real transform, float32 out.  The CPU suite runs every
GPU case through it, so a machine without a GPU already shows that the references stay inside the limits (the model sits at
0.0007 .. 0.015 of them); a partition applied at the wrong delay or a ring slot read one block off misses them by four orders
of magnitude."""
import zlib

import numpy as np

from tests import edge_checks as ec
from tests import part_checks as pc

MAX_TAPS = pc.MAX_TAPS
# (block, taps): both parities of log2 block, P = 1, a last partition holding one tap, workgroups of one wave, of several, and
# threads owning 1, 2, 8 and 16 bins
SHAPES = [(64, 1), (64, 64), (64, 65), (128, 199), (256, 700), (512, 513), (2048, 4100), (4096, 8200)]
CHANNELS = (3, 37)
QUIET = 1                       # the channel scaled by 2^-10
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def partitions(T, block):
    return -(-T // block)


def calls_for(block, T, k=1):
    """calls of k blocks that take the ring (R = P + k - 1 slots) once around and two blocks further"""
    return -(-(partitions(T, block) + k + 1) // k)


def signal(oracle, channels, n, seed):
    """[channels, n] float32 of the oracle's generator, channel QUIET scaled by 2^-10 (exact)"""
    def make():
        x = oracle.synth_f32(channels, n, seed=seed)
        if channels > QUIET:
            x[QUIET] *= np.float32(2.0 ** -10)
        x.setflags(write=False)
        return x
    return cached(("x", channels, n, seed), make)


def padded(x, T):
    return np.concatenate([x, np.zeros((x.shape[0], T - 1), np.float32)], axis=1)


def dense_ref(oracle, x, h):
    """float64 reference of the frames and the flush: the oracle's FIR on the zero-padded stream, fft_ref at the top length;
    kept by the content of x and h"""
    def make():
        xz = padded(x, len(h))
        return oracle.fir_batch_f32_mt(xz, h, threads=16) if len(h) <= 25249 else pc.fft_ref(xz, h)
    h = np.ascontiguousarray(h, dtype=np.float64)
    return cached(("dense", x.shape, zlib.crc32(np.ascontiguousarray(x).tobytes()), zlib.crc32(h.tobytes())), make)


# ------------------------------------------------------------------------------------------------ the model
def model(x, taps, block, k=1):
    """x [channels, calls * k * block] through the algorithm in float32 / complex64, then the flush: [channels, n + T - 1]
    float32.  taps: [T] (shared) or [channels, T].  k only groups the blocks into calls: it cannot change a bit here either."""
    x = np.asarray(x, dtype=np.float32)
    taps = np.asarray(taps, dtype=np.float32)
    channels, n = x.shape
    rows = taps[None, :] if taps.ndim == 1 else taps
    T = rows.shape[1]
    B, N, P = block, 2 * block, partitions(T, block)
    assert n % (k * B) == 0
    R = P + k - 1
    hp = np.zeros((rows.shape[0], P * B), np.float64)
    hp[:, :T] = rows
    H = np.fft.rfft(hp.reshape(rows.shape[0], P, B), N, axis=2).astype(np.complex64)      # [rows, P, B + 1]
    H = np.ascontiguousarray(np.moveaxis(H, 1, 0))                                          # [P, rows, B + 1]
    ring = np.zeros((R, channels, B + 1), np.complex64)
    prev = np.zeros((channels, B), np.float32)
    out = np.empty((channels, n + T - 1), np.float32)

    def product(head, first):
        """sum over p >= first of ring[head - p] H_p, p ascending (numpy reduces a leading axis row by row)"""
        slots = (head - np.arange(first, P)) % R
        return np.add.reduce(ring[slots] * H[first:], axis=0, dtype=np.complex64)

    head = 0
    for j in range(n // B):
        cur = x[:, j * B:(j + 1) * B]
        ring[head] = np.fft.rfft(np.concatenate([prev, cur], axis=1), axis=1).astype(np.complex64)
        out[:, j * B:(j + 1) * B] = np.fft.irfft(product(head, 0), N, axis=1)[:, B:].astype(np.float32)
        prev = cur
        head = (head + 1) % R
    # flush: zero blocks; only the spectrum of (last block, zeros) is new, and block j meets it at p = j
    keep = T - 1
    last = np.fft.rfft(np.concatenate([prev, np.zeros_like(prev)], axis=1), axis=1).astype(np.complex64)
    for j in range(-(-keep // B)):
        acc = last * H[j]
        if j + 1 < P:
            # ring[head - 1] is the last input block's own spectrum: partition j + 1 meets it, and so on
            slots = (head + j - np.arange(j + 1, P)) % R
            acc = np.add.reduce(np.concatenate([acc[None], ring[slots] * H[j + 1:]], axis=0), axis=0, dtype=np.complex64)
        y = np.fft.irfft(acc, N, axis=1)[:, B:].astype(np.float32)
        m = min(B, keep - j * B)
        out[:, n + j * B:n + j * B + m] = y[:, :m]
    return out


# ------------------------------------------------------------------------------------------------ the device
def device(dev, x, taps, block, k=1):
    """the same stream through one llz_fir_stream_mc handle in calls of k blocks (device tensors, outputs preset to NaN), then
    the flush: [channels, n + T - 1] float32"""
    import torch
    from llzlab_amd import filters
    x = np.asarray(x, dtype=np.float32)
    channels, n = x.shape
    T = np.shape(taps)[-1]
    f = filters.FirStreamMC(channels, block, taps, frame_len=k * block)
    assert f.plan() == (2 * block, partitions(T, block), partitions(T, block) + k - 1, k), f.plan()
    outs = stream_calls(dev, f, x)
    tail = torch.full((channels, T - 1), float("nan"), dtype=torch.float32, device=dev)     # one tap: empty, nothing to emit
    f.flush(tail)
    outs.append(tail.cpu().numpy())
    f.close()
    return np.concatenate(outs, axis=1)


def stream_calls(dev, f, x):
    """x through the handle f in calls of its frame_len: the list of output frames"""
    import torch
    outs = []
    for o in range(0, x.shape[1], f.frame_len):
        xi = torch.from_numpy(np.ascontiguousarray(x[:, o:o + f.frame_len])).to(dev)
        yi = torch.full_like(xi, float("nan"))
        f.filter(xi, yi)
        outs.append(yi.cpu().numpy())
    return outs


# ------------------------------------------------------------------------------------------------ the cases
def check_shape(run, oracle, block, T, channels, k=1, calls=None, families=("dense", "sparse"), per_channel=False):
    """one (block, taps, channels) case through `run(x, taps, block, k)`: dense taps under the RMS gate, the sparse families at
    every sample.  per_channel: the same taps as [channels, T] rows (a bank of equal rows)"""
    calls = calls or calls_for(block, T, k)
    n = calls * k * block
    x = signal(oracle, channels, n, seed=1 + T + block)
    what = f"block {block} T={T} {channels}ch x {calls} calls of {k}"

    def rows(h):
        return np.tile(h, (channels, 1)) if per_channel else h
    if "dense" in families:
        h = ec.dense_taps(T, seed=T)
        y = run(x, rows(h), block, k)
        assert y.shape == (channels, n + T - 1) and y.dtype == np.float32
        pc.check_dense(y, dense_ref(oracle, x, h), n, f"{what} dense")
    if "sparse" in families:
        for fam, h in ec.sparse_families(T):
            y = run(x, rows(h), block, k)
            ref, _ = ec.fir_ref(padded(x, T), h)
            pc.check_sparse(y, ref, pc.partition_limit(2 * block, h, x), n, f"{what} {fam}", period=block)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
