"""GPU: the multi-channel FIR with taps that weigh their ends (tests/edge_checks.py), every overlap-save kernel instance at
both ends of its tap range, the time-domain kernels up to the largest filter llz_fir_filter_mc_init accepts, AUTO on both
sides of each crossover.  Dense taps against the oracle under the RMS gate; two-ends and one-delta taps against
x[n] + s x[n-T+1] (the input delayed) at every sample, under the derived limits of edge_checks.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import edge_checks as ec  # noqa: E402

ALGO_OF_NFFT = {1024: filters.FIR_ALGO_OVERLAP_SAVE, 2048: filters.FIR_ALGO_OVERLAP_SAVE_2048,
                4096: filters.FIR_ALGO_OVERLAP_SAVE_4096, 8192: filters.FIR_ALGO_OVERLAP_SAVE_8192}
NFFT_OF_ALGO = {v: k for k, v in ALGO_OF_NFFT.items()}
TIME, TIME_MFMA, AUTO = filters.FIR_ALGO_TIME, filters.FIR_ALGO_TIME_MFMA, filters.FIR_ALGO_AUTO
SPREAD = 6                                                   # channels of a wide batch that the oracle filters (dense taps)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def test_every_ols_instance_is_parametrised():
    cases = ec.ols_cases()
    assert set(NFFT_OF_ALGO) == set(ec.OLS_ALGO)
    assert len({(c[0], c[1]) for c in cases}) == 18 == sum(len(r[2]) for r in ec.OLS_INSTANCES)


def stream(dev, taps, algo, x, n, channels):
    """x [channels, frames * n] through one handle in frames of n, then the flush: ([channels, frames * n + T - 1], algo)"""
    T = len(taps)
    f = filters.FirFilterMC(channels, n, taps, algo=algo)
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
    used = f.algo
    f.close()
    return np.concatenate(outs, axis=1), used


def check_fir(dev, oracle, T, algo, channels, n, frames, what, expect_algo=None, seed=1):
    """every tap family through `frames` frames of n samples and the flush, against the zero-padded stream: the frames under
    the limit of the algorithm that ran, the flush tail (always the time-domain kernel) under the direct-form limit"""
    N = frames * n
    x = oracle.synth_f32(channels, N, seed=seed + T + n)
    xz = np.concatenate([x, np.zeros((channels, T - 1), np.float32)], axis=1)
    x_rms = float(np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    used = None
    # dense taps: the oracle under the RMS gate (on a spread of channels when the batch is wide)
    sub = np.arange(channels) if channels <= SPREAD else np.array(sorted({0, 1, 63, 64, channels // 2, channels - 1}))
    h = ec.dense_taps(T, seed=T)
    y, used = stream(dev, h, algo, x, n, channels)
    assert used == (expect_algo if expect_algo is not None else algo), (used, algo, expect_algo)
    ref = oracle.fir_batch_f32(xz[sub], h)
    ec.rms_check(y[sub, :N], ref[:, :N], f"{what} dense T={T} algo={used} frames")
    if T > 1:
        ec.rms_check(y[sub, N:], ref[:, N:], f"{what} dense T={T} algo={used} flush")
    assert np.isfinite(y).all()
    # sparse taps: every sample of every channel
    nfft = NFFT_OF_ALGO.get(used)
    for fam, h in ec.sparse_families(T):
        y, used2 = stream(dev, h, algo, x, n, channels)
        assert used2 == used
        ref, A = ec.fir_ref(xz, h)
        direct = ec.direct_limit(A, np.count_nonzero(h))
        lim = ec.ols_limit(nfft, x_rms, float(np.sqrt(np.sum(h * h)))) if nfft else direct[:, :N]
        ec.sample_check(y[:, :N], ref[:, :N], lim, f"{what} {fam} T={T} algo={used} frames",
                        period=ec.ols_job(nfft, T) if nfft else None)
        if T > 1:
            ec.sample_check(y[:, N:], ref[:, N:], direct[:, N:], f"{what} {fam} T={T} algo={used} flush")
    return used


# ------------------------------------------------------------------------------------------------ overlap-save
@pytest.mark.parametrize("nfft,overlap,T,which", ec.ols_cases(), ids=[f"{c[0]}-{c[1]}-{c[3]}-T{c[2]}" for c in ec.ols_cases()])
def test_fir_ols_instance_at_both_ends_of_its_tap_range(dev, oracle, nfft, overlap, T, which):
    """one kernel instance (transform size, overlap) forced by its algo value, at flt_len = overlap + 1 -- the last tap meets
    the oldest overlap sample -- and at the smallest flt_len that selects it; two frames of whole jobs and a ragged frame
    through one handle each, then the flush; at overlap + 1 also frames shorter than the overlap (the history spans three
    calls) and a batch of 300 channels"""
    algo = ALGO_OF_NFFT[nfft]
    job = 2 * (nfft - overlap)                                           # new samples per transform pair
    check_fir(dev, oracle, T, algo, 3, 2 * job, 2, "whole jobs")
    check_fir(dev, oracle, T, algo, 2, job + job // 3 + 1, 2, "ragged")
    if which == "last":
        check_fir(dev, oracle, T, algo, 2, overlap // 2 - 3, 3, "shorter than the overlap")
        check_fir(dev, oracle, T, algo, 300, job + 17, 1, "300 channels")


@pytest.mark.parametrize("T,expect", [(32, TIME), (33, filters.FIR_ALGO_OVERLAP_SAVE), (257, filters.FIR_ALGO_OVERLAP_SAVE),
                                      (258, filters.FIR_ALGO_OVERLAP_SAVE_2048), (513, filters.FIR_ALGO_OVERLAP_SAVE_2048),
                                      (514, filters.FIR_ALGO_OVERLAP_SAVE_4096), (1025, filters.FIR_ALGO_OVERLAP_SAVE_4096),
                                      (1026, filters.FIR_ALGO_OVERLAP_SAVE_8192), (6145, filters.FIR_ALGO_OVERLAP_SAVE_8192)])
def test_fir_auto_on_both_sides_of_each_crossover(dev, oracle, T, expect):
    check_fir(dev, oracle, T, AUTO, 3, 9000 + T, 2, "auto", expect_algo=expect)
    check_fir(dev, oracle, T, AUTO, 2, max(T // 2 - 3, 1), 3, "auto short", expect_algo=expect)


# ------------------------------------------------------------------------------------------------ time domain
@pytest.mark.parametrize("algo,T", [(TIME, t) for t in (1, 2, 16, 17, 32, 33, 601)] + [(TIME_MFMA, t) for t in (1, 2, 32, 601)])
def test_fir_time_domain_edges(dev, oracle, algo, T):
    check_fir(dev, oracle, T, algo, 3, 2 * 2048 + 77, 2, "ragged tiles")
    check_fir(dev, oracle, T, algo, 2, 2048, 2, "whole tile")
    if T > 3:
        check_fir(dev, oracle, T, algo, 2, T // 2 - 1, 3, "shorter than the history")
    check_fir(dev, oracle, T, algo, 300, 2100, 1, "300 channels")


def _accepts(T, algo):
    try:
        f = filters.FirFilterMC(2, 64, np.ones(T), algo=algo)
    except capi.LlzError:
        return None
    used = f.algo
    f.close()
    return used


@pytest.fixture(scope="module")
def largest(dev):
    """the largest flt_len llz_fir_filter_mc_init accepts per algo, by bisection; every probe is kept for the monotony check"""
    out = {}
    for algo in (TIME, TIME_MFMA, AUTO):
        probes = {}

        def ok(T):
            if T not in probes:
                probes[T] = _accepts(T, algo)
            return probes[T] is not None
        assert ok(1) and ok(601)
        hi = 1024
        while ok(hi):
            hi *= 2
            assert hi <= 1 << 24, "init accepts any length"
        lo = hi // 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if ok(mid) else (lo, mid)
        for T in (lo - 17, lo - 1, lo + 1, lo + 2, lo + 15, lo + 16, lo + 17, lo + 4096, 3 * lo, 1 << 22):   # more probes on both sides
            ok(T)
        out[algo] = (lo, probes)
    return out


def test_fir_init_acceptance_is_monotone(largest):
    for algo, (top, probes) in largest.items():
        assert all((used is not None) == (T <= top) for T, used in probes.items()), (algo, top, sorted(probes.items()))
        print(f"algo {algo}: largest flt_len {top}, {len(probes)} probes")
    assert largest[AUTO][0] == largest[TIME][0]                          # AUTO falls back to the time-domain kernel
    assert 601 <= largest[TIME_MFMA][0] <= largest[TIME][0]
    for T, used in largest[AUTO][1].items():                             # beyond the last rung: matrix cores while they fit
        if used is not None and T > 6145:
            assert used == (TIME_MFMA if T <= largest[TIME_MFMA][0] else TIME), (T, used)


@pytest.mark.parametrize("algo,which", [(TIME, "largest"), (TIME_MFMA, "largest"), (AUTO, "6146"), (AUTO, "largest")])
def test_fir_time_domain_at_the_largest_filter(dev, oracle, largest, algo, which):
    """the longest filter each time-domain kernel takes, and AUTO just past the last overlap-save rung and at the longest:
    frames longer and shorter than the history, streamed, then the flush (the flush of every handle is k_fir_td_f32)"""
    T = 6146 if which == "6146" else largest[algo][0]
    expect = algo if algo != AUTO else (TIME_MFMA if T <= largest[TIME_MFMA][0] else TIME)
    check_fir(dev, oracle, T, algo, 2, T + 2048 + 77, 2, f"{which} long frames", expect_algo=expect)
    check_fir(dev, oracle, T, algo, 2, T // 2 - 3, 3, f"{which} short frames", expect_algo=expect)
