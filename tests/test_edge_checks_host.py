"""CPU self-test of tests/edge_checks.py: with the oracle as both truth and "kernel", the checks accept a correct float32
result and reject every mutation that the windowed-sinc RMS tests let through -- a lost end tap, a stale overlap sample,
a misplaced output, a zeroed entry of the resampler's tap matrix."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import edge_checks as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(257, 1024), (1025, 2048), (3073, 4096), (6145, 8192)]          # taps, the transform that holds them
BLOCK = 1024                                                             # block length of the stale-overlap mutation


def _signal(oracle, T):
    return oracle.synth_f32(2, 2 * T + 4099, seed=T)


def _kernel(oracle, x, h):
    """the oracle as the kernel under test: float32 taps, double accumulate, float32 result"""
    return oracle.fir_batch_f32(x, h.astype(np.float32).astype(np.float64)).astype(np.float32)


def _convolve32(x, h):
    h32 = h.astype(np.float32)
    return np.stack([np.convolve(row, h32)[:x.shape[1]] for row in x]).astype(np.float32)


def _stale_overlap(y, x, h):
    """one stale overlap sample per block: the last tap meets x[i-T+2] instead of x[i-T+1] at every block start"""
    T = len(h)
    y = y.astype(np.float64)
    xd = x.astype(np.float64)
    for i in range(((T + BLOCK - 1) // BLOCK) * BLOCK, x.shape[1], BLOCK):
        y[:, i] += h[T - 1] * (xd[:, i - T + 2] - xd[:, i - T + 1])
    return y.astype(np.float32)


def _neighbour(y, ref):
    """one output replaced by its neighbour, at the first place past the middle where the two differ by 1e-2"""
    j = ref.shape[1] // 2
    while abs(ref[0, j] - ref[0, j - 1]) < 1e-2:
        j += 1
    y = y.copy()
    y[0, j] = y[0, j - 1]
    return y


def _mutants(oracle, x, h, ref):
    """[(name, result)] of the mutations that change this tap set's output"""
    T = len(h)
    good = _kernel(oracle, x, h)
    out = []
    if h[T - 1] != 0 and T > 1:
        cut = h.copy()
        cut[T - 1] = 0
        out.append(("last tap zeroed", _kernel(oracle, x, cut)))
        out.append(("stale overlap sample", _stale_overlap(good, x, h)))
    if h[0] != 0 and T > 1:
        cut = h.copy()
        cut[0] = 0
        out.append(("first tap zeroed", _kernel(oracle, x, cut)))
    out.append(("output replaced by its neighbour", _neighbour(good, ref)))
    return good, out


@pytest.mark.parametrize("T,nfft", SIZES)
def test_dense_taps_rms_gate_accepts_float32_and_rejects_mutations(oracle, T, nfft):
    h = ec.dense_taps(T, seed=T)
    assert abs(float(np.sum(h * h)) - 1.0) < 1e-6 and min(abs(h[0]), abs(h[-1])) > 0.2 / np.sqrt(T)
    x = _signal(oracle, T)
    ref = oracle.fir_batch_f32(x, h)
    good, mutants = _mutants(oracle, x, h, ref)
    ec.rms_check(good, ref, f"dense T={T}: float32-rounded oracle")
    ec.rms_check(_convolve32(x, h), ref, f"dense T={T}: float32 np.convolve")
    assert [m[0] for m in mutants] == ["last tap zeroed", "stale overlap sample", "first tap zeroed",
                                       "output replaced by its neighbour"]
    for name, bad in mutants:
        with pytest.raises(AssertionError):
            ec.rms_check(bad, ref, f"dense T={T}: {name}")


@pytest.mark.parametrize("T,nfft", SIZES)
def test_sparse_taps_sample_limits_accept_float32_and_reject_mutations(oracle, T, nfft):
    x = _signal(oracle, T)
    x_rms = float(np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    seen = set()
    for fam, h in ec.sparse_families(T):
        ref, A = ec.fir_ref(x, h)
        assert np.max(np.abs(ref - oracle.fir_batch_f32(x, h))) < 1e-12            # the plain reference is the oracle's
        limits = {"direct": ec.direct_limit(A, np.count_nonzero(h)),
                  "overlap-save": ec.ols_limit(nfft, x_rms, float(np.sqrt(np.sum(h * h))))}
        assert 5e-5 < limits["overlap-save"] < 1e-3
        good, mutants = _mutants(oracle, x, h, ref)
        for lname, lim in limits.items():
            ec.sample_check(good, ref, lim, f"{fam} T={T} {lname}: float32-rounded oracle")
            ec.sample_check(_convolve32(x, h), ref, lim, f"{fam} T={T} {lname}: float32 np.convolve")
            for name, bad in mutants:
                seen.add(name)
                with pytest.raises(AssertionError):
                    ec.sample_check(bad, ref, lim, f"{fam} T={T} {lname}: {name}", period=BLOCK)
    assert seen == {"last tap zeroed", "stale overlap sample", "first tap zeroed", "output replaced by its neighbour"}


@pytest.mark.parametrize("T", [1025, 3073, 6145])
def test_kaiser_taps_under_the_rms_gate_accept_a_lost_last_tap(oracle, T):
    """the gap the edge tests close, kept as a recorded fact: with the windowed-sinc taps of the parity tests the RMS gate
    passes a filter whose last tap is lost (and the dense taps do not: see above)"""
    h = oracle.fir_design(po.LPF, T, 0.2, 0.0, po.KAISER).astype(np.float32).astype(np.float64)
    assert abs(h[T - 1]) < 1e-6
    x = _signal(oracle, T)
    ref = oracle.fir_batch_f32(x, h)
    cut = h.copy()
    cut[T - 1] = 0
    assert not np.array_equal(_kernel(oracle, x, cut), _kernel(oracle, x, h)) or abs(h[T - 1]) < 1e-7
    ec.rms_check(_kernel(oracle, x, cut), ref, f"kaiser T={T}: last tap zeroed")


def test_ols_instances_match_the_kernel_table():
    """every instance of OLS_RUNGS is in the list the GPU tests are parametrised from: 18 in all"""
    with open(os.path.join(ROOT, "llzlab_amd", "csrc", "kernels", "fir_ols.hip")) as f:
        rungs = ec.ols_rungs_in_source(f.read())
    assert rungs == ec.OLS_INSTANCES
    assert sum(len(r[2]) for r in rungs) == 18
    cases = ec.ols_cases()
    assert len(cases) == 36 and len({(c[0], c[1]) for c in cases}) == 18
    for nfft, ov, T, which in cases:
        assert T - 1 <= ov and (which == "last") == (T == ov + 1)


@pytest.mark.parametrize("L,M,win,gain", [(1, 3, po.BLACKMAN, 1.0), (1, 5, po.KAISER, 2.5), (2, 3, po.HAMMING, 1.0), (8, 7, po.BLACKMAN, 0.37),
                                          (147, 160, po.BLACKMAN, 1.0), (441, 320, po.BLACKMAN, 2.5)])
def test_resampler_probe_reaches_every_tap_and_rejects_a_zeroed_one(oracle, L, M, win, gain):
    info = oracle.rs_info(2, L, M, gain, win)
    mat, Q = info["matrix"], info["cols"]
    x, positions = ec.rs_probe_signal(L, M, Q)
    lens = ec.rs_probe_cuts(positions, x.shape[1], M, Q)
    assert ec.rs_straddles(positions, lens, L, M, Q) >= 2
    ref = oracle.rs_batch_f32(x, L, M, gain, win)
    hit = ec.rs_hits(positions, ref.shape[1], L, M, Q)
    assert hit[mat != 0].all(), f"{np.count_nonzero((mat != 0) & ~hit)} non-zero taps not probed"
    # every output holds at most one product
    pos, _phase = ec.rs_index_map(ref.shape[1], L, M)
    for c in range(x.shape[0]):
        csum = np.concatenate([[0], np.cumsum(x[c] != 0)])
        assert np.max(csum[pos + 1] - csum[np.maximum(pos - Q + 1, 0)]) <= 1
    ec.rs_probe_check(ec.rs_numpy(x, mat, L, M, gain), ref, f"{L}:{M} gain {gain}: numpy restatement")
    nz = np.argwhere(mat != 0)
    order = np.argsort(np.abs(mat[mat != 0]))
    rng = np.random.default_rng(L * 1000 + M)
    pick = np.unique(np.concatenate([order[:6], order[-2:], [0, len(nz) - 1], rng.integers(0, len(nz), 14)]))
    for f, k in nz[pick]:
        m2 = mat.copy()
        m2[f, k] = 0.0
        with pytest.raises(AssertionError):
            ec.rs_probe_check(ec.rs_numpy(x, m2, L, M, gain), ref, f"{L}:{M}: entry ({f}, {k}) = {mat[f, k]:.3g} zeroed")
