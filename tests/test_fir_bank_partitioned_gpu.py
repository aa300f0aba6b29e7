"""GPU: the partitioned bank -- llz_fir_pbank_mc_init, LLZ_FIR_ALGO_PARTITIONED with a tap set per channel, 1..131073 taps
(fir_part.hip: k_fir_part_fwd, k_fir_part_mac<true>, k_fir_part_inv), run through the bank's own calls.  References: the
oracle one channel at a time with that channel's taps (part_bank_checks.oracle_ref), part_checks.fft_ref at 131073 taps,
edge_checks.fir_ref for sparse sets.  Limits: part_checks.check_dense and check_sparse / partition_limit, per channel, no
tolerance of their own.  Tap families: those of test_fir_bank_gpu.py, in which every channel differs from its neighbours, so
a channel filtered with another channel's spectra -- the H pointer not advanced with a pass -- misses by four orders of
magnitude.  Every case asserts the plan it means to hit and prints its worst ratio to its limit.  The parent of this feature
has none of the three symbols: every test here fails there at the missing symbol."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import edge_checks as ec  # noqa: E402
from tests import part_bank_checks as pb  # noqa: E402
from tests import part_checks as pc  # noqa: E402
from tests import test_buffer_contract_gpu as tb  # noqa: E402
from tests import test_fir_bank_gpu as fb  # noqa: E402
from tests.test_fir_partitioned_gpu import RUN, expect_plan, own_nfft  # noqa: E402

PART = filters.FIR_ALGO_PARTITIONED
ERR_ARG = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    assert hasattr(capi.lib(), "llz_fir_pbank_mc_init")
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def padded(oracle, channels, total, T, seed):
    x = oracle.synth_f32(channels, total, seed=seed)
    return x, np.concatenate([x, np.zeros((channels, T - 1), np.float32)], axis=1)


def check_stream(dev, oracle, T, channels, n, frames, N, what, kinds=("dense", "sparse"), dense_ref="oracle", passes=1):
    """the bank's tap families (delays, two ends, dense; every channel its own set) through `frames` frames of n samples and
    the flush against the zero-padded stream, every channel against its own taps"""
    total = frames * n
    x, xz = padded(oracle, channels, total, T, 1 + T + n)
    expect = expect_plan(N, pc.partitions(T, N), passes)
    for fam, make, sparse in fb.families(T):
        if ("sparse" if sparse else "dense") not in kinds:
            continue
        h = make(T, channels)
        assert T == 1 or all(not np.array_equal(h[c], h[c + 1]) for c in range(channels - 1))
        y, _, _ = pb.stream(dev, h, x, n, expect)
        tag = f"pbank {what} {fam} T={T} N={N} {channels}x{frames}x{n}"
        if sparse:
            pc.check_sparse(y, pb.sparse_ref(xz, h), pb.limits(N, h, x), total, tag, period=N // 2)
        else:
            ref = pb.oracle_ref(oracle, xz, h) if dense_ref == "oracle" else pb.fft_ref(xz, h)
            pc.check_dense(y, ref, total, tag)


# ------------------------------------------------------------------------------------------------ 1. small transform forced
@pytest.mark.parametrize("T,P", [(1, 1), (513, 2), (1300, 3), (2049, 5)])
def test_small_transform_every_family(dev, oracle, T, P):
    """part_nfft = 1024, B = 512, 5 channels: a ragged last block with history from the handle, whole blocks, and frames
    shorter than a block and than the history"""
    B = 512
    assert pc.partitions(T, 1024) == P
    with capi.tuned(part_nfft=1024):
        check_stream(dev, oracle, T, 5, 3 * B + 77, 2, 1024, "ragged")
        check_stream(dev, oracle, T, 5, 2 * B, 2, 1024, "whole blocks")
        check_stream(dev, oracle, T, 5, 125, 3, 1024, "short frames")


# ------------------------------------------------------------------------------------------------ 2. passes
def test_channels_in_passes_each_with_its_own_spectra(dev, oracle):
    """1 MiB of scratch: two channels of 48 blocks at 3 partitions fit, 5 channels take three passes, the last with one
    channel.  The spectra must advance with the channels of a pass: every channel is held to its own taps, and the same
    output held to its neighbour's taps must miss the gate by a wide margin (two independent unit-norm tap sets differ by
    sqrt(2) relative RMS against 1e-5: asked here is 0.1, four orders above the gate), so no wrong row can pass"""
    T, n, channels = 1300, 48 * 512, 5
    h = fb.dense_taps(T, channels)
    x, xz = padded(oracle, channels, n, T, T + n)
    with capi.tuned(part_nfft=1024, part_scratch_mb=1):
        y, plan, _ = pb.stream(dev, h, x, n, expect_plan(1024, 3, 3))
        assert plan == (1024, 3, 2, 3) and channels % plan[2] != 0, plan
    pc.check_dense(y, pb.oracle_ref(oracle, xz, h), n, f"pbank passes T={T} {channels}x{n}")
    wrong = pb.oracle_ref(oracle, xz, np.roll(h, -1, axis=0))          # channel c's input, channel c + 1's taps
    for c in range(channels):
        rel = pc.rel_rms(y[c], wrong[c])
        print(f"pbank passes ch {c} against its neighbour's taps: relative rms {rel:.3g} ({rel / ec.TOL:.3g} gates)")
        assert rel > 0.1, f"channel {c} is as near to its neighbour's taps as {rel:.3g}"
    with capi.tuned(part_nfft=1024):                         # allocated under the cap, then the cap lowered: the plan follows
        f = filters.FirBankMC(channels, n, h, algo=PART)
        assert f.partition_plan(n) == (1024, 3, 5, 1)
        with capi.tuned(part_scratch_mb=1):
            assert f.partition_plan(n) == (1024, 3, 2, 3)
        f.close()


# ------------------------------------------------------------------------------------------------ 3. the library's own N
@pytest.mark.parametrize("T,N,P", [(6146, 4096, 4), (25249, 8192, 7)])
def test_own_transform(dev, oracle, T, N, P):
    """6146 taps: 4 partitions of 2048; 25249: the first length the bank of llz_fir_bank_mc_init refuses"""
    assert own_nfft(T) == N and pc.partitions(T, N) == P
    if T == 25249:
        with pytest.raises(capi.LlzError, match="LDS tile"):
            filters.FirBankMC(2, 64, np.ones((2, T)), algo=filters.FIR_ALGO_TIME)
    check_stream(dev, oracle, T, 2, T + 2048 + 77, 2, N, "long frames")
    check_stream(dev, oracle, T, 2, T // 2 - 3, 3, N, "short frames")


# ------------------------------------------------------------------------------------------------ 4. longest
def test_longest_filter(dev, oracle):
    """131073 taps, 33 partitions of 4096: the product's partition loop runs twice and ends on a partial trip of one.  Sparse
    families against fir_ref in short frames, one dense set per channel against the float64 FFT reference in one frame"""
    T = pc.MAX_TAPS
    assert own_nfft(T) == 8192 and pc.partitions(T, 8192) == 33
    check_stream(dev, oracle, T, 2, T // 2 - 3, 2, 8192, "short frames", kinds=("sparse",))
    check_stream(dev, oracle, T, 2, T + 4096 + 77, 1, 8192, "long frame", kinds=("dense",), dense_ref="fft")


def test_init_past_the_longest_is_refused(dev):
    with pytest.raises(capi.LlzError, match="1..131073"):
        filters.FirBankMC(2, 4096, np.ones((2, pc.MAX_TAPS + 1)), algo=PART)


# ------------------------------------------------------------------------------------------------ 5. equal rows
@pytest.mark.parametrize("T,forced", [(1300, 1024), (6146, None)])
def test_equal_rows_reproduce_the_shared_form_bit_for_bit(dev, oracle, T, forced):
    """one builder makes the spectra of both forms and the product sums p ascending in one thread in both: a bank whose rows
    all hold h gives the bits of FirFilterMC(algo = 7) with h, frames and flush"""
    N = forced or own_nfft(T)
    channels, n = 3, 3 * (N // 2) + 77
    x = oracle.synth_f32(channels, 2 * n, seed=T)
    h = ec.dense_taps(T, seed=T)
    expect = expect_plan(N, pc.partitions(T, N))
    with capi.tuned(**({"part_nfft": forced} if forced else {})):
        shared, plan_s, _ = pc.stream(dev, h, x, n, expect)
        bank, plan_b, _ = pb.stream(dev, np.tile(h, (channels, 1)), x, n, expect)
    assert plan_s == plan_b and shared.shape == bank.shape == (channels, 2 * n + T - 1) and np.isfinite(bank).all()
    differ = int(np.count_nonzero(pb.bits(shared) != pb.bits(bank)))
    print(f"pbank equal rows T={T} N={N}: {differ} of {bank.size} samples differ in their bits from the shared form")
    assert differ == 0


# ------------------------------------------------------------------------------------------------ 6. set_taps
@pytest.mark.parametrize("fam", ["delays", "dense"])
def test_set_taps_between_frames(dev, oracle, fam):
    """7 channels, 1300 taps at 1024 points: after frame 0 a range leaving the bank is refused (the handle goes on working),
    then channels [2, 5) get new rows.  Those channels: frame 0 from the old taps, frame 1 and the flush from the new taps over
    the same raw input -- the history is input samples.  The others: the bits of a run without set_taps"""
    T, channels, N = 1300, 7, 1024
    n = 3 * 512 + 77
    make, sparse = next((m, s) for name, m, s in fb.families(T) if name == fam)
    h, new = make(T, channels), make(T, 3, c0=100)
    x, xz = padded(oracle, channels, 2 * n, T, T + n)
    expect = expect_plan(N, 3)

    def swap(bank, k):
        if k:
            return
        with pytest.raises(capi.LlzError):
            bank.set_taps(5, new)                                          # [5, 8) leaves the bank
        flat = np.ascontiguousarray(new, dtype=np.float32)
        for first, count in ((-1, 1), (7, 1), (6, 2), (0, 8), (0, 0), (3, -1)):
            assert capi.lib().llz_fir_bank_mc_set_taps(bank.handle, first, count, flat.ctypes.data) == ERR_ARG, (first, count)
            assert "llz_fir_bank_mc_set_taps" in capi.last_error()
        bank.set_taps(2, new)

    with capi.tuned(part_nfft=N):
        plain, _, _ = pb.stream(dev, h, x, n, expect)
        got, _, _ = pb.stream(dev, h, x, n, expect, between=swap)
    for c in (0, 1, 5, 6):
        assert np.array_equal(pb.bits(got[c]), pb.bits(plain[c])), f"channel {c} changed with set_taps(2, 3 rows)"
    h_eff = h.copy()
    h_eff[2:5] = new
    ref_fn = pb.sparse_ref if sparse else (lambda a, b: pb.oracle_ref(oracle, a, b))
    ref_old, ref_new = ref_fn(xz, h), ref_fn(xz, h_eff)
    ref = np.concatenate([ref_old[:, :n], ref_new[:, n:]], axis=1)
    tag = f"pbank set_taps {fam} T={T}"
    if sparse:
        # frame 0 under the old taps' limit, frame 1 and the flush under the new taps'
        pc.check_sparse(got[:, :n], ref[:, :n], pb.limits(N, h, x), n, tag + " frame 0", period=N // 2)
        pc.check_sparse(got[:, n:], ref[:, n:], pb.limits(N, h_eff, x), n, tag + " frame 1", period=N // 2)
    else:
        pc.check_dense(got[:, :n], ref[:, :n], n, tag + " frame 0")
        pc.check_dense(got[:, n:], ref[:, n:], n, tag + " frame 1")
    for c in (2, 3, 4):                                      # and the replaced rows did change something
        assert not np.array_equal(got[c, n:], plain[c, n:]), f"channel {c}: set_taps changed nothing"
        assert np.array_equal(pb.bits(got[c, :n]), pb.bits(plain[c, :n])), f"channel {c}: frame 0 changed"


# ------------------------------------------------------------------------------------------------ 7. channel independence
@pytest.mark.parametrize("T,forced", [(1300, 1024), (6146, None)])
def test_channels_are_independent_to_the_bit(dev, oracle, T, forced):
    """run B = run A with channels 1 and 4 zeroed and channels 2 and 5 scaled by 2^20, every channel with its own taps: the
    untouched channels keep their bits, the zeroed ones are exactly 0.0, the scaled ones are 2^20 times run A bit for bit;
    and run A on a fresh handle repeats its bits"""
    N = forced or own_nfft(T)
    n = 3 * (N // 2) + 77
    xa = oracle.synth_f32(6, 2 * n, seed=T)
    xb = xa.copy()
    xb[[1, 4]] = 0.0
    xb[[2, 5]] *= np.float32(2.0 ** 20)
    h = fb.dense_taps(T, 6)
    expect = expect_plan(N, pc.partitions(T, N))
    with capi.tuned(**({"part_nfft": forced} if forced else {})):
        ya, _, _ = pb.stream(dev, h, xa, n, expect)
        ya2, _, _ = pb.stream(dev, h, xa, n, expect)
        yb, _, _ = pb.stream(dev, h, xb, n, expect)
    assert ya.shape == (6, 2 * n + T - 1) and np.isfinite(ya).all() and np.isfinite(yb).all()
    assert np.array_equal(pb.bits(ya), pb.bits(ya2)), "the same calls on a fresh handle gave other bits"
    for c in (0, 3):
        assert np.array_equal(pb.bits(ya[c]), pb.bits(yb[c])), f"channel {c} changed with its neighbours"
    for c in (1, 4):
        assert np.all(yb[c] == 0.0), f"channel {c}: zero input, non-zero output"
    for c in (2, 5):
        assert np.array_equal(pb.bits(ya[c] * np.float32(2.0 ** 20)), pb.bits(yb[c])), f"channel {c}: not 2^20 times run A"
    xz = np.concatenate([xa, np.zeros((6, T - 1), np.float32)], axis=1)
    pc.check_dense(ya, pb.oracle_ref(oracle, xz, h), 2 * n, f"pbank independence run A T={T} N={N}")


# ------------------------------------------------------------------------------------------------ 8. wide batch
@pytest.mark.parametrize("T", [257, 1300])
def test_wide_batch(dev, oracle, T):
    """300 channels of 7 B + 100 samples at part_nfft = 1024, distinct dense taps: the channel dimension of all three grids
    and of the table, 1 and 3 partitions; all channels checked"""
    with capi.tuned(part_nfft=1024):
        check_stream(dev, oracle, T, 300, 7 * 512 + 100, 1, 1024, "300 channels", kinds=("dense",))


# ------------------------------------------------------------------------------------------------ 9. runs, odd transform
def test_runs_of_blocks_and_the_odd_transform(dev, oracle):
    """73 blocks + 100 samples at B = 512 are 37 complex blocks: two whole runs of the product kernel and one of 5; 2048
    points take the transforms' last radix-2 stage"""
    T = 1300
    with capi.tuned(part_nfft=1024):
        n = 73 * 512 + 100
        assert -(-(-(-n // 512)) // 2) == 37 and 37 > 2 * RUN and 37 % RUN
        check_stream(dev, oracle, T, 3, n, 1, 1024, "runs", kinds=("dense",))
    with capi.tuned(part_nfft=2048):
        check_stream(dev, oracle, T, 3, 3 * 1024 + 77, 2, 2048, "2048 points")


# ------------------------------------------------------------------------------------------------ 10. buffer contract
def run_guarded(dev, oracle, io, channels, n):
    T = 1300

    def make():
        h = fb.dense_taps(T, channels)
        x, xz = padded(oracle, channels, 2 * n, T, T + n)
        return h, x, pb.oracle_ref(oracle, xz, h)
    h, x, ref = tb.cached(("fir-pbank", T, channels, n), make)
    with capi.tuned(part_nfft=1024):
        f = filters.FirBankMC(channels, n, h, algo=PART)
        assert f.algo == PART and f.partition_plan(n)[:2] == (1024, 3)
        ys = []
        for o in (0, n):                                   # the second frame takes its history from the handle
            y = io.out(tb.F32, channels, n)
            f.filter(io.inp(x[:, o:o + n]), y)
            ys.append(y)
        tail = io.out(tb.F32, channels, T - 1)
        f.flush(tail)
        io.verify("fir partitioned bank")
        f.close()
    for k, buf in enumerate(io.outs):
        bc.check_all_written(buf, f"fir partitioned bank: output {k}")
    got = np.concatenate([tb.host(t) for t in ys + [tail]], axis=1)
    pc.check_dense(got, ref, 2 * n, f"pbank guarded {channels}x{n}")


@pytest.mark.parametrize("off", tb.OFF32, ids=[f"in{o[0]}-out{o[1]}" for o in tb.OFF32])
@pytest.mark.parametrize("n", [4096, 1000])
def test_guarded_buffers(dev, oracle, n, off):
    """outputs between sentinel bands, inputs between NaN bands, at every offset pair: bands and inputs bit-unchanged, every
    output element written, the result under the gate"""
    run_guarded(dev, oracle, tb.Io(dev, off, "nan"), 3, n)


@pytest.mark.parametrize("n", [4096, 1000])
def test_guarded_buffers_host_pointers(dev, oracle, n):
    run_guarded(dev, oracle, tb.Io(torch.device("cpu"), (1, 3), "nan"), 3, n)


def test_overlap_refused(dev):
    L = capi.lib()
    with capi.tuned(part_nfft=1024):
        f = filters.FirBankMC(2, 1000, fb.dense_taps(1300, 2), algo=PART)
        tb.refused(bc.overlap_cases(2000, device=dev), lambda a, b: L.llz_fir_bank_mc(f.handle, tb.dptr(a), tb.dptr(b), 1000),
                   "llz_fir_bank_mc")
        a = torch.zeros(2000, device=dev)
        assert L.llz_fir_bank_mc(f.handle, C.c_void_p(a.data_ptr()), C.c_void_p(a.data_ptr()), 1000) == ERR_ARG
        assert "llz_fir_bank_mc" in capi.last_error()
        f.close()


# ------------------------------------------------------------------------------------------------ 11. plan query
@pytest.mark.parametrize("T,forced,n", [(1300, 1024, 48 * 512), (6146, None, 9000), (pc.MAX_TAPS, None, 4096)])
def test_plan_equals_the_shared_form(dev, T, forced, n):
    channels = 5
    with capi.tuned(**({"part_nfft": forced, "part_scratch_mb": 1} if forced else {})):
        s = filters.FirFilterMC(channels, n, np.ones(T), algo=PART)
        b = filters.FirBankMC(channels, n, np.ones((channels, T)), algo=PART)
        for m in (n, T - 1, 1):
            assert b.partition_plan(m) == s.partition_plan(m), (m, b.partition_plan(m), s.partition_plan(m))
        print(f"pbank plan T={T} n={n}: {b.partition_plan(n)}")
        assert b.algo == PART == capi.lib().llz_fir_bank_mc_algo(b.handle) and b.flt_len == T
        out = (C.c_int * 4)()                                   # the shared form's query keeps refusing a bank handle
        assert capi.lib().llz_fir_filter_mc_partition_plan(b.handle, n, out) == ERR_ARG
        assert "llz_fir_filter_mc_partition_plan" in capi.last_error()
        s.close()
        b.close()


def test_plan_refuses_other_handles(dev):
    L = capi.lib()
    out = (C.c_int * 4)()
    bank = filters.FirBankMC(2, 64, np.ones((2, 300)), algo=filters.FIR_ALGO_TIME)
    shared = filters.FirFilterMC(2, 64, np.ones(1300), algo=PART)
    for f in (bank, shared):
        L.llz_hip_tune(b"no_such_override", 0)
        assert L.llz_fir_pbank_mc_plan(f.handle, 64, out) == ERR_ARG
        assert "llz_fir_pbank_mc_plan" in capi.last_error()
    with pytest.raises(capi.LlzError):
        bank.partition_plan(64)
    bank.close()
    shared.close()


def test_scratch_cap_too_small_is_refused(dev):
    with capi.tuned(part_nfft=1024, part_scratch_mb=1):
        with pytest.raises(capi.LlzError, match="scratch"):
            filters.FirBankMC(2, 1 << 20, np.ones((2, 1300)), algo=PART)
