"""GPU: the filter bank llz_fir_bank_mc -- the multi-channel FIR with a tap set per channel (time domain k_fir_td_f32<true>,
1024-point overlap-save k_fir_bank_ols_f32).  The reference is the unchanged oracle called one channel at a time with that
channel's taps; the limits are those of tests/edge_checks.py, applied PER CHANNEL, so that one wrong channel in a wide batch
is not averaged away:

  * dense taps: rms_check under TOL = 1e-5, a channel at a time;
  * sparse taps on the time-domain kernel, and every flush tail: direct_limit, every sample;
  * sparse taps through overlap-save: ols_limit(1024, rms(x_c), ||h_c||_2), every sample.

Tap families in which every channel differs from its neighbours (a channel that is given another channel's taps misses its
limit by four orders of magnitude: with 257 taps, swapped delay taps err by about 1.9 against 8.8e-5, swapped dense sets by
0.8 RMS against 1e-5):
  delays    one tap g_c = (-1)^c (1 + (c mod 8) / 8) at index (37 c + 11) mod T
  two ends  h[0] = 1, h[T-1] = (-1)^c   (T >= 2)
  dense     edge_checks.dense_taps(T, seed=1000 + c)

The bank kernel's plan is the shared 1024-point rung's (a job is 1536 samples, a wave holds two segments, a workgroup
eight), so the shapes below are written in those terms."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import edge_checks as ec  # noqa: E402
from tests import test_buffer_contract_gpu as tb  # noqa: E402

TIME, OLS, AUTO = filters.FIR_ALGO_TIME, filters.FIR_ALGO_OVERLAP_SAVE, filters.FIR_ALGO_AUTO
JOB = 1536
ERR_ARG = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ tap families
def delay_taps(T, channels, c0=0):
    h = np.zeros((channels, T))
    for i in range(channels):
        c = c0 + i
        h[i, (37 * c + 11) % T] = (-1.0) ** c * (1 + (c % 8) / 8)
    return h


def two_ends_taps(T, channels, c0=0):
    h = np.zeros((channels, T))
    h[:, 0] = 1.0
    h[:, T - 1] = [(-1.0) ** (c0 + i) for i in range(channels)]
    return h


def dense_taps(T, channels, c0=0):
    return np.stack([ec.dense_taps(T, seed=1000 + c0 + i) for i in range(channels)])


def families(T):
    fams = [("delays", delay_taps, True), ("dense", dense_taps, False)]
    if T >= 2:
        fams.insert(1, ("two-ends", two_ends_taps, True))
    return fams


# ------------------------------------------------------------------------------------------------ running and checking
def stream(dev, bank, x, n, between=None):
    """x [channels, frames * n] through the handle in frames of n, then the flush; between(k) runs after frame k"""
    outs = []
    for k, o in enumerate(range(0, x.shape[1], n)):
        xi = torch.from_numpy(np.ascontiguousarray(x[:, o:o + n])).to(dev)
        yi = torch.full_like(xi, float("nan"))
        bank.filter(xi, yi)
        outs.append(yi.cpu().numpy())
        if between:
            between(k)
    if bank.flt_len > 1:
        tail = torch.full((bank.channels, bank.flt_len - 1), float("nan"), dtype=torch.float32, device=dev)
        bank.flush(tail)
        outs.append(tail.cpu().numpy())
    return np.concatenate(outs, axis=1)


def reference(oracle, xz, h, sparse):
    """per channel: (y, A) of the zero-padded stream xz with the channel's own taps; A (sparse families only) = |h| on |x|"""
    ys, As = [], []
    for c in range(xz.shape[0]):
        if sparse:
            y, A = ec.fir_ref(xz[c:c + 1], h[c])
            As.append(A[0])
        else:
            y = oracle.fir_batch_f32(xz[c:c + 1], h[c])
        ys.append(y[0])
    return np.stack(ys), (np.stack(As) if sparse else None)


def check_channels(got, ref, A, h, x, N, used, what, channels=None):
    """got / ref [channels, N + T - 1]: the frames under the limit of the algorithm that ran, the flush under the direct-form
    limit, each channel against its own limit"""
    T = h.shape[1]
    assert np.isfinite(got).all(), what
    for c in (range(got.shape[0]) if channels is None else channels):
        tag = f"{what} ch {c}"
        if A is None:
            ec.rms_check(got[c, :N], ref[c, :N], tag + " frames")
            if T > 1:
                ec.rms_check(got[c, N:], ref[c, N:], tag + " flush")
            continue
        direct = ec.direct_limit(A[c], np.count_nonzero(h[c]))
        if used == OLS:
            x_rms = float(np.sqrt(np.mean(x[c].astype(np.float64) ** 2)))
            lim = ec.ols_limit(1024, x_rms, float(np.sqrt(np.sum(h[c] * h[c]))))
        else:
            lim = direct[:N]
        ec.sample_check(got[c, :N], ref[c, :N], lim, tag + " frames", period=JOB if used == OLS else None)
        if T > 1:
            ec.sample_check(got[c, N:], ref[c, N:], direct[N:], tag + " flush")


_X = {}


def signal(oracle, channels, N, T):
    key = (channels, N, T)
    if key not in _X:
        x = oracle.synth_f32(channels, N, seed=7 + T + N)
        _X[key] = (x, np.concatenate([x, np.zeros((channels, T - 1), np.float32)], axis=1))
    return _X[key]


def check_bank(dev, oracle, T, algo, channels, n, frames, what, expect, tune=None):
    """every family through `frames` frames of n samples and the flush, one handle per family"""
    N = frames * n
    x, xz = signal(oracle, channels, N, T)
    for fam, make, sparse in families(T):
        h = make(T, channels)
        with capi.tuned(**(tune or {})):
            bank = filters.FirBankMC(channels, n, h, algo=algo)
            assert bank.algo == expect, (bank.algo, expect)
            got = stream(dev, bank, x, n)
            bank.close()
        ref, A = reference(oracle, xz, h, sparse)
        check_channels(got, ref, A, h, x, N, expect, f"bank {what} {fam} T={T} algo={expect}")


# ------------------------------------------------------------------------------------------------ 1. time domain
@pytest.mark.parametrize("T", [1, 2, 9, 32, 300])
def test_bank_time_domain_by_auto(dev, oracle, T):
    """AUTO takes the time domain up to 32 taps and above 257; 5 channels, frames with a tile boundary (2048) inside"""
    check_bank(dev, oracle, T, AUTO, 5, 2048 + 77, 2, "time", TIME)


# ------------------------------------------------------------------------------------------------ 2. overlap-save
@pytest.mark.parametrize("T,algo", [(33, AUTO), (200, AUTO), (257, AUTO), (1, OLS)])
def test_bank_overlap_save(dev, oracle, T, algo):
    """5 channels: three segments per channel under ols_seg_len = 2 (a wave's two halves sit on different channels and a
    half-wave's next segment is another channel's), whole jobs, and frames of 125 samples (the history spans three calls)"""
    check_bank(dev, oracle, T, algo, 5, 5 * JOB + 100, 2, "three segments", OLS, tune=dict(ols_seg_len=2))
    check_bank(dev, oracle, T, algo, 5, 2 * JOB, 2, "whole jobs", OLS)
    check_bank(dev, oracle, T, algo, 5, 125, 3, "short frames", OLS)


# ------------------------------------------------------------------------------------------------ 3. grid stride
def test_bank_grid_stride_across_channels(dev, oracle):
    """300 channels x 8 jobs as 2400 one-job segments on 2048 slots (one workgroup per CU): the prefetch carried into the
    second round lands on other channels, and so does the spectrum a half-wave refills.  Every channel is checked."""
    check_bank(dev, oracle, 257, AUTO, 300, 7 * JOB + 100, 2, "grid stride", OLS, tune=dict(ols_seg_len=1, ols_wg_per_cu=1))


# ------------------------------------------------------------------------------------------------ 4. idle slots
@pytest.mark.parametrize("channels", [1, 65])
def test_bank_idle_slots_and_halves_without_partner(dev, oracle, channels):
    """one job per channel: one channel leaves seven half-waves of its workgroup idle, 65 channels leave a half without a
    partner in the last wave"""
    check_bank(dev, oracle, 257, AUTO, channels, JOB, 2, f"{channels} channels", OLS)


# ------------------------------------------------------------------------------------------------ 5. set_taps
@pytest.mark.parametrize("T,expect", [(257, OLS), (9, TIME)])
def test_bank_set_taps_between_frames(dev, oracle, T, expect):
    """frame 1, set_taps(2, new[3]), frame 2, flush: channels outside [2, 5) equal the unchanged bank; inside, frame 2 and the
    flush are the new taps on concat(last T-1 samples before them, the frame / zeros)"""
    channels, n = 7, 2 * JOB + 100
    x, xz = signal(oracle, channels, 2 * n, T)
    keep = T - 1
    for fam, make, sparse in families(T):
        h, new = make(T, channels), make(T, 3, c0=100)
        bank = filters.FirBankMC(channels, n, h, algo=AUTO)
        assert bank.algo == expect
        got = stream(dev, bank, x, n, between=lambda k: bank.set_taps(2, new) if k == 0 else None)
        with pytest.raises(capi.LlzError):
            bank.set_taps(5, new)                                        # [5, 8) leaves the bank
        L = capi.lib()
        flat = np.ascontiguousarray(new, dtype=np.float32)
        for first, count in ((-1, 1), (7, 1), (6, 2), (0, 8), (0, 0), (3, -1)):
            assert L.llz_fir_bank_mc_set_taps(bank.handle, first, count, flat.ctypes.data) == ERR_ARG, (first, count)
            assert "llz_fir_bank_mc_set_taps" in capi.last_error()
        bank.close()
        ref, A = reference(oracle, xz, h, sparse)
        # channels 2..4: frame 1 stays; frame 2 and the flush from the new taps with the samples before them as history
        tail_in = np.concatenate([x[2:5, n:], np.zeros((3, keep), np.float32)], axis=1)             # frame 2, then zeros
        for i in range(3):
            c = 2 + i
            if sparse:
                y, a = ec.fir_ref(tail_in[i:i + 1], new[i], prev=x[c:c + 1, n - keep:n])
                ref[c, n:], A[c, n:] = y[0], a[0]
            else:
                full = np.concatenate([x[c:c + 1, n - keep:n], tail_in[i:i + 1]], axis=1)
                ref[c, n:] = oracle.fir_batch_f32(full, new[i])[0, keep:]
        what = f"bank set_taps {fam} T={T}"
        check_channels(got, ref, A, h, x, 2 * n, expect, what + " unchanged", channels=(0, 1, 5, 6))
        # inside the range: frame 2 and the flush under the new taps' limits, frame 1 under the old taps'
        h_eff = h.copy()
        h_eff[2:5] = new
        check_channels(got[:, n:], ref[:, n:], None if A is None else A[:, n:], h_eff, x[:, n:], n, expect, what + " replaced",
                       channels=(2, 3, 4))
        first = got[2:5, :n]
        if sparse:
            for i in range(3):
                c = 2 + i
                direct = ec.direct_limit(A[c, :n], np.count_nonzero(h[c]))
                lim = (ec.ols_limit(1024, float(np.sqrt(np.mean(x[c, :n].astype(np.float64) ** 2))),
                                    float(np.sqrt(np.sum(h[c] ** 2)))) if expect == OLS else direct)
                ec.sample_check(first[i], ref[c, :n], lim, f"{what} ch {c} frame 1")
        else:
            for i in range(3):
                ec.rms_check(first[i], ref[2 + i, :n], f"{what} ch {2 + i} frame 1")


# ------------------------------------------------------------------------------------------------ 6. equal rows
@pytest.mark.parametrize("T,expect", [(257, OLS), (9, TIME)])
def test_bank_of_equal_rows_against_the_shared_form(dev, oracle, T, expect):
    """a bank whose rows all hold one tap set meets the same limits; the difference to FirFilterMC on the same input is
    printed (the bank mirrors the upper half of the spectrum instead of reading it: bit equality is not required)"""
    channels, n = 5, 2 * JOB + 100
    x, xz = signal(oracle, channels, 2 * n, T)
    one = ec.dense_taps(T, seed=T)
    h = np.tile(one, (channels, 1))
    bank = filters.FirBankMC(channels, n, h)
    assert bank.algo == expect
    got = stream(dev, bank, x, n)
    bank.close()
    ref, _ = reference(oracle, xz, h, False)
    check_channels(got, ref, None, h, x, 2 * n, expect, f"bank equal rows T={T}")
    shared = filters.FirFilterMC(channels, n, one)
    assert shared.algo == expect
    same = stream(dev, shared, x, n)
    shared.close()
    print(f"bank of equal rows against FirFilterMC, T={T}: max |difference| {float(np.max(np.abs(got - same))):.3g}")


def test_bank_refuses_one_dimensional_taps(dev):
    with pytest.raises(capi.LlzError):
        filters.FirBankMC(4, 1000, np.ones(63))


# ------------------------------------------------------------------------------------------------ 7. buffer contract
def run_bank(dev, oracle, io, algo, T, channels, n):
    def make():
        h = dense_taps(T, channels)
        x = oracle.synth_f32(channels, 2 * n, seed=T + n)
        xz = np.concatenate([x, np.zeros((channels, T - 1), np.float32)], axis=1)
        return h, x, reference(oracle, xz, h, False)[0]
    h, x, ref = tb.cached(("fir-bank", algo, T, channels, n), make)
    f = filters.FirBankMC(channels, n, h, algo=algo)
    assert f.algo == algo
    ys = []
    for o in (0, n):                                       # the second frame takes its history from the handle
        y = io.out(tb.F32, channels, n)
        f.filter(io.inp(x[:, o:o + n]), y)
        ys.append(y)
    tail = io.out(tb.F32, channels, T - 1)
    f.flush(tail)
    io.verify(f"fir bank algo {algo}")
    f.close()
    for k, buf in enumerate(io.outs):
        bc.check_all_written(buf, f"fir bank algo {algo}: output {k}")
    got = np.concatenate([tb.host(t) for t in ys + [tail]], axis=1)
    for c in range(channels):
        ec.rms_check(got[c], ref[c], f"fir bank algo {algo} T={T} {channels}x{n} + flush ch {c}")


BANK_CASES = [("time-full", dict(algo=TIME, T=63, channels=3, n=4096)), ("time-partial", dict(algo=TIME, T=63, channels=2, n=1000)),
              ("ols-full", dict(algo=OLS, T=257, channels=3, n=4096)), ("ols-partial", dict(algo=OLS, T=257, channels=3, n=1000))]


@pytest.mark.parametrize("off", tb.OFF32, ids=[f"in{o[0]}-out{o[1]}" for o in tb.OFF32])
@pytest.mark.parametrize("name,case", BANK_CASES, ids=[c[0] for c in BANK_CASES])
def test_bank_guarded_buffers(dev, oracle, name, case, off):
    """outputs between sentinel bands at the offsets of test_buffer_contract_gpu.py, inputs between NaN bands: bands and
    inputs bit-unchanged, every output element written, the result under the gate"""
    run_bank(dev, oracle, tb.Io(dev, off, "nan"), **case)


@pytest.mark.parametrize("name,case", BANK_CASES[1::2], ids=[c[0] for c in BANK_CASES[1::2]])
def test_bank_guarded_buffers_host_pointers(dev, oracle, name, case):
    """the same with host memory, staged through the handle"""
    run_bank(dev, oracle, tb.Io(torch.device("cpu"), (1, 3), "nan"), **case)


def test_bank_overlap_refused(dev):
    L = capi.lib()
    for algo, T in ((TIME, 63), (OLS, 257)):
        f = filters.FirBankMC(2, 1000, dense_taps(T, 2), algo=algo)
        tb.refused(bc.overlap_cases(2000, device=dev), lambda a, b: L.llz_fir_bank_mc(f.handle, tb.dptr(a), tb.dptr(b), 1000),
                   "llz_fir_bank_mc")
        a = torch.zeros(2000, device=dev)
        assert L.llz_fir_bank_mc(f.handle, C.c_void_p(a.data_ptr()), C.c_void_p(a.data_ptr()), 1000) == ERR_ARG
        assert "llz_fir_bank_mc" in capi.last_error()
        f.close()
