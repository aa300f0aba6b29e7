"""Shared pieces of the partitioned overlap-save tests (test_fir_partitioned_host.py, test_fir_partitioned_gpu.py): the
references, the limits and the streaming driver of LLZ_FIR_ALGO_PARTITIONED.  The limits are those of tests/edge_checks.py and
carry no tolerance of their own:

  * dense taps (edge_checks.dense_taps, unit norm): edge_checks.rms_check, the 1e-5 gate, a channel at a time, frames and flush
    apart.  Reference: the oracle up to 25249 taps; at 131073 taps, where its time-domain loop would take hours, fft_ref below,
    which test_fir_partitioned_host.py pins to the oracle (<= 1e-12 relative RMS at 6146 and 25249 taps);
  * sparse taps (edge_checks.sparse_families): every sample within sum_p ols_limit(N, rms(x_c), ||h_p||_2) over the partitions
    p that hold a non-zero tap -- each partition is an N-point overlap-save of its own taps -- against edge_checks.fir_ref.

A partition applied at the wrong delay misses either limit by four orders of magnitude."""
import numpy as np

from tests import edge_checks as ec

PARTITIONED = 7
MAX_TAPS = 131073


def fft_ref(x, h):
    """float64 FFT convolution of the rows of x (zero history) with h, as long as x: the stand-in for the oracle where its
    time-domain loop is not affordable"""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n = x.shape[1]
    size = 1 << int(np.ceil(np.log2(n + len(h) - 1)))
    return np.fft.irfft(np.fft.rfft(x, size, axis=1) * np.fft.rfft(h, size)[None, :], size, axis=1)[:, :n]


def partitions(T, N):
    return -(-T // (N // 2))


def partition_limit(N, h, x):
    """[channels, 1]: sum over the partitions of h (blocks of N / 2 taps) that hold a non-zero tap of
    ols_limit(N, rms(x_c), ||h_p||_2)"""
    B = N // 2
    x_rms = np.sqrt(np.mean(np.asarray(x, dtype=np.float64) ** 2, axis=1))
    lim = np.zeros_like(x_rms)
    for p in range(partitions(len(h), N)):
        norm = float(np.sqrt(np.sum(h[p * B:(p + 1) * B] ** 2)))
        if norm > 0:
            lim += ec.ols_limit(N, x_rms, norm)
    return lim[:, None]


def rel_rms(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-300))


def stream(dev, taps, x, n, expect=None):
    """x [channels, frames * n] through one LLZ_FIR_ALGO_PARTITIONED handle in frames of n (device tensors, outputs preset to
    NaN), then the flush: ([channels, frames * n + T - 1] float32, plan of a frame, plan of the flush).  expect: a function
    (plan, n) that asserts the shape the caller means to hit"""
    import torch
    from llzlab_amd import filters
    channels, T = x.shape[0], len(taps)
    f = filters.FirFilterMC(channels, n, taps, algo=PARTITIONED)
    assert f.algo == PARTITIONED
    plan = f.partition_plan(n)
    plan_flush = f.partition_plan(T - 1) if T > 1 else None
    assert plan[1] == partitions(T, plan[0]) and plan[3] == -(-channels // plan[2]), plan
    if expect:
        expect(plan, n)
    outs = []
    for o in range(0, x.shape[1], n):
        xi = torch.from_numpy(np.ascontiguousarray(x[:, o:o + n])).to(dev)
        yi = torch.full_like(xi, float("nan"))
        f.filter(xi, yi)
        outs.append(yi.cpu().numpy())
    if T > 1:
        tail = torch.full((channels, T - 1), float("nan"), dtype=torch.float32, device=dev)
        f.flush(tail)
        outs.append(tail.cpu().numpy())
    f.close()
    return np.concatenate(outs, axis=1), plan, plan_flush


def check_dense(y, ref, N, what):
    """frames and flush apart, a channel at a time, under the RMS gate; prints the worst ratio to the gate"""
    worst = 0.0
    for c in range(y.shape[0]):
        parts = [("frames", slice(0, N))] + ([("flush", slice(N, None))] if y.shape[1] > N else [])
        for name, s in parts:
            err, rel = ec.rms_check(y[c, s], ref[c, s], f"{what} ch {c} {name}")
            worst = max(worst, err / ec.TOL, rel / ec.TOL)
    print(f"{what}: worst ratio to the gate {worst:.3g}")
    assert np.isfinite(y).all()


def check_sparse(y, ref, lim, N, what, period):
    """every sample of every channel, frames and flush apart; prints the worst ratio to the limit"""
    ratio = float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref) / lim))
    print(f"{what}: worst ratio to the limit {ratio:.3g}")
    ec.sample_check(y[:, :N], ref[:, :N], lim, f"{what} frames", period=period)
    if y.shape[1] > N:
        ec.sample_check(y[:, N:], ref[:, N:], lim, f"{what} flush", period=period)
