"""GPU: LLZ_FIR_ALGO_PARTITIONED, the uniformly partitioned overlap-save of llz_fir_filter_mc (fir_part.hip: forward
k_fir_part_fwd, product k_fir_part_mac, inverse k_fir_part_inv) from 1 to 131073 taps.  References and limits:
tests/part_checks.py.  Shapes are written in terms of the block B = N / 2 and the partitions P that partition_plan reports,
and every case asserts the plan it means to hit.  The parent of this feature answers every init here with "unknown algo 7"."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import edge_checks as ec  # noqa: E402
from tests import part_checks as pc  # noqa: E402
from tests import test_buffer_contract_gpu as tb  # noqa: E402

PART = filters.FIR_ALGO_PARTITIONED
ERR_ARG = -1
RUN = 16                        # PART_RUN of fir_part.hip: complex blocks a product workgroup produces


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def own_nfft(T):
    """the library's own transform size: the smallest that keeps the filter within 4 partitions, 8192 beyond"""
    return next((n for n in (1024, 2048, 4096) if T <= 2 * n), 8192)


def expect_plan(N, P, passes=1):
    def check(plan, n):
        assert plan[0] == N and plan[1] == P and plan[3] == passes, (plan, N, P, passes)
    return check


def check_stream(dev, oracle, T, channels, n, frames, N, what, families=("dense", "sparse"), dense_ref="oracle", passes=1):
    """the tap families through `frames` frames of n samples and the flush against the zero-padded stream"""
    total = frames * n
    x = oracle.synth_f32(channels, total, seed=1 + T + n)
    xz = np.concatenate([x, np.zeros((channels, T - 1), np.float32)], axis=1)
    expect = expect_plan(N, pc.partitions(T, N), passes)
    if "dense" in families:
        h = ec.dense_taps(T, seed=T)
        y, plan, _ = pc.stream(dev, h, x, n, expect)
        ref = oracle.fir_batch_f32_mt(xz, h, threads=16) if dense_ref == "oracle" else pc.fft_ref(xz, h)
        pc.check_dense(y, ref, total, f"{what} dense T={T} N={N} {channels}x{frames}x{n}")
    if "sparse" in families:
        for fam, h in ec.sparse_families(T):
            y, plan, _ = pc.stream(dev, h, x, n, expect)
            ref, _ = ec.fir_ref(xz, h)
            pc.check_sparse(y, ref, pc.partition_limit(N, h, x), total, f"{what} {fam} T={T} N={N} {channels}x{frames}x{n}",
                            period=N // 2)


# ------------------------------------------------------------------------------------------------ 1. small transform forced
@pytest.mark.parametrize("T,P", [(1, 1), (512, 1), (513, 2), (1300, 3), (2049, 5)])
def test_small_transform_every_family(dev, oracle, T, P):
    """part_nfft = 1024, B = 512: one partition, a last tap on the edge of a partition (T - 1 a whole number of blocks at 513
    and 2049) and inside one; a ragged last block with history from the handle, whole blocks, and frames shorter than a block
    and than the history"""
    B = 512
    assert pc.partitions(T, 1024) == P
    with capi.tuned(part_nfft=1024):
        check_stream(dev, oracle, T, 5, 3 * B + 77, 2, 1024, "ragged")
        check_stream(dev, oracle, T, 5, 2 * B, 2, 1024, "whole blocks")
        check_stream(dev, oracle, T, 5, 125, 3, 1024, "short frames")


# ------------------------------------------------------------------------------------------------ 2. the library's own N
@pytest.mark.parametrize("T", [6146, 25249])
def test_own_transform_past_the_ladder_and_past_the_time_domain(dev, oracle, T):
    """6146 taps: the first length past the overlap-save ladder; 25249: the first length every other algo refuses.  The shapes
    of test_fir_time_domain_at_the_largest_filter"""
    N = own_nfft(T)
    assert N == {6146: 4096, 25249: 8192}[T]
    check_stream(dev, oracle, T, 2, T + 2048 + 77, 2, N, "long frames")
    check_stream(dev, oracle, T, 2, T // 2 - 3, 3, N, "short frames")


# ------------------------------------------------------------------------------------------------ 3. longest
def test_longest_filter(dev, oracle):
    """131073 taps, 33 partitions of 4096: the product kernel's partition loop (unrolled by 16) runs twice and ends on a
    partial trip of one.  Sparse families against fir_ref, one dense set against the float64 FFT reference"""
    T = pc.MAX_TAPS
    assert own_nfft(T) == 8192 and pc.partitions(T, 8192) == 33
    check_stream(dev, oracle, T, 2, T // 2 - 3, 2, 8192, "short frames", families=("sparse",))
    check_stream(dev, oracle, T, 2, T + 4096 + 77, 1, 8192, "long frame", dense_ref="fft")


def test_init_past_the_longest_is_refused(dev):
    with pytest.raises(capi.LlzError, match="1..131073"):
        filters.FirFilterMC(2, 4096, np.ones(pc.MAX_TAPS + 1), algo=PART)


# ------------------------------------------------------------------------------------------------ 4. passes
def test_channels_in_passes(dev, oracle):
    """1 MiB of scratch: a channel of 48 blocks at 3 partitions takes 2 x 24 + 2 spectra of 8 KB = 400 KB, so two channels
    fit and 5 channels take three passes, the last with one channel; every channel is checked"""
    T, n = 1300, 48 * 512
    with capi.tuned(part_nfft=1024, part_scratch_mb=1):
        f = filters.FirFilterMC(5, n, ec.dense_taps(T, seed=T), algo=PART)
        plan = f.partition_plan(n)
        f.close()
        assert plan == (1024, 3, 2, 3) and 5 % plan[2] != 0, plan
        check_stream(dev, oracle, T, 5, n, 2, 1024, "passes", passes=3)
    with capi.tuned(part_nfft=1024):                         # allocated under the cap, then the cap lowered: the plan follows
        f = filters.FirFilterMC(5, n, ec.dense_taps(T, seed=T), algo=PART)
        assert f.partition_plan(n) == (1024, 3, 5, 1)
        with capi.tuned(part_scratch_mb=1):
            assert f.partition_plan(n) == (1024, 3, 2, 3)
        f.close()


def test_scratch_cap_too_small_is_refused(dev):
    with capi.tuned(part_nfft=1024, part_scratch_mb=1):
        with pytest.raises(capi.LlzError, match="scratch"):
            filters.FirFilterMC(2, 1 << 20, np.ones(1300), algo=PART)


# ------------------------------------------------------------------------------------------------ 5. every loop
@pytest.mark.parametrize("T", [257, 1300])
def test_wide_batch(dev, oracle, T):
    """300 channels of 7 B + 100 samples at part_nfft = 1024: the channel dimension of all three grids, 1 and 3 partitions"""
    with capi.tuned(part_nfft=1024):
        check_stream(dev, oracle, T, 300, 7 * 512 + 100, 1, 1024, "300 channels", families=("dense",))


def test_runs_of_blocks_and_the_odd_transform(dev, oracle):
    """the kernels have no grid-stride loop: a workgroup is one (spectrum, channel), (run, bin tile, channel) or (block,
    channel), and the loops over the N points of a transform are whole by construction.  What remains:
      * the product kernel's run of 16 complex blocks: 73 blocks + 100 samples at B = 512 are 74 blocks, 37 complex blocks: two
        whole runs and one of 5 (flush: 3 blocks, 2 complex: one partial run);
      * its partition loop: twice and a partial trip at 33 partitions (test_longest_filter), one partial trip everywhere else;
      * the bin tiles: 4 at 1024 points, 8 / 16 / 32 at 2048 / 4096 / 8192;
      * the transforms' last radix-2 stage, taken when log2 N is odd: 2048 points forced here, 8192 in the cases above."""
    T = 1300
    with capi.tuned(part_nfft=1024):
        n = 73 * 512 + 100
        assert -(-(-(-n // 512)) // 2) == 37 and 37 > 2 * RUN and 37 % RUN
        check_stream(dev, oracle, T, 3, n, 1, 1024, "runs", families=("dense",))
    with capi.tuned(part_nfft=2048):
        check_stream(dev, oracle, T, 3, 3 * 1024 + 77, 2, 2048, "2048 points")


# ------------------------------------------------------------------------------------------------ 6. channel independence
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("T,forced", [(1300, 1024), (6146, None)])
def test_channels_are_independent_to_the_bit(dev, oracle, T, forced):
    """run B = run A with channels 1 and 4 zeroed and channels 2 and 5 scaled by 2^20: the untouched channels keep their bits,
    the zeroed ones are exactly 0.0, the scaled ones are 2^20 times run A bit for bit (every operation is covariant under a
    power of two), frames and flush; and run A on a fresh handle repeats its bits"""
    N = forced or own_nfft(T)
    n = 3 * (N // 2) + 77
    xa = oracle.synth_f32(6, 2 * n, seed=T)
    xb = xa.copy()
    xb[[1, 4]] = 0.0
    xb[[2, 5]] *= np.float32(2.0 ** 20)
    h = ec.dense_taps(T, seed=T)
    expect = expect_plan(N, pc.partitions(T, N))
    with capi.tuned(**({"part_nfft": forced} if forced else {})):
        ya, _, _ = pc.stream(dev, h, xa, n, expect)
        ya2, _, _ = pc.stream(dev, h, xa, n, expect)
        yb, _, _ = pc.stream(dev, h, xb, n, expect)
    assert ya.shape == (6, 2 * n + T - 1) and np.isfinite(ya).all() and np.isfinite(yb).all()
    assert np.array_equal(_bits(ya), _bits(ya2)), "the same calls on a fresh handle gave other bits"
    for c in (0, 3):
        assert np.array_equal(_bits(ya[c]), _bits(yb[c])), f"channel {c} changed with its neighbours"
    for c in (1, 4):
        assert np.all(yb[c] == 0.0), f"channel {c}: zero input, non-zero output"
    for c in (2, 5):
        assert np.array_equal(_bits(ya[c] * np.float32(2.0 ** 20)), _bits(yb[c])), f"channel {c}: not 2^20 times run A"
    xz = np.concatenate([xa, np.zeros((6, T - 1), np.float32)], axis=1)
    pc.check_dense(ya, oracle.fir_batch_f32_mt(xz, h, threads=16), 2 * n, f"independence run A T={T} N={N}")


# ------------------------------------------------------------------------------------------------ 7. buffer contract
def run_guarded(dev, oracle, io, channels, n):
    T = 1300

    def make():
        h = ec.dense_taps(T, seed=T)
        x = oracle.synth_f32(channels, 2 * n, seed=T + n)
        xz = np.concatenate([x, np.zeros((channels, T - 1), np.float32)], axis=1)
        return h, x, oracle.fir_batch_f32(xz, h)
    h, x, ref = tb.cached(("fir-part", T, channels, n), make)
    with capi.tuned(part_nfft=1024):
        f = filters.FirFilterMC(channels, n, h, algo=PART)
        assert f.algo == PART and f.partition_plan(n)[:2] == (1024, 3)
        ys = []
        for o in (0, n):                                   # the second frame takes its history from the handle
            y = io.out(tb.F32, channels, n)
            f.filter(io.inp(x[:, o:o + n]), y)
            ys.append(y)
        tail = io.out(tb.F32, channels, T - 1)
        f.flush(tail)
        io.verify("fir partitioned")
        f.close()
    for k, buf in enumerate(io.outs):
        bc.check_all_written(buf, f"fir partitioned: output {k}")
    got = np.concatenate([tb.host(t) for t in ys + [tail]], axis=1)
    pc.check_dense(got, ref, 2 * n, f"fir partitioned guarded {channels}x{n}")


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
        f = filters.FirFilterMC(2, 1000, ec.dense_taps(1300, seed=1300), algo=PART)
        tb.refused(bc.overlap_cases(2000, device=dev), lambda a, b: L.llz_fir_filter_mc(f.handle, tb.dptr(a), tb.dptr(b), 1000),
                   "llz_fir_filter_mc")
        a = torch.zeros(2000, device=dev)
        assert L.llz_fir_filter_mc(f.handle, C.c_void_p(a.data_ptr()), C.c_void_p(a.data_ptr()), 1000) == ERR_ARG
        assert "llz_fir_filter_mc" in capi.last_error()
        f.close()


# ------------------------------------------------------------------------------------------------ 8. opt-in
def test_auto_past_the_ladder_is_still_the_time_domain(dev):
    f = filters.FirFilterMC(2, 64, np.ones(6146), algo=filters.FIR_ALGO_AUTO)
    assert f.algo in (filters.FIR_ALGO_TIME_MFMA, filters.FIR_ALGO_TIME)
    with pytest.raises(capi.LlzError):
        f.partition_plan(64)                                 # the query is the partitioned form's alone
    f.close()
