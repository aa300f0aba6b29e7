"""GPU: llz_fir_stream_mc, the block convolver that keeps the spectra of its input between calls (fir_stream.hip: one fused
kernel per call, a frequency-domain delay line per channel), blocks of 64 .. 4096 samples against 1 .. 131073 taps.  Cases,
inputs, references, limits and the numpy model they were sized on: tests/stream_checks.py; tests/test_fir_stream_host.py runs
the same cases through the model on a machine without a GPU.  Device tensors, outputs preset to NaN; every parity case prints
its worst ratio to its limit (-s).  The parent of this feature has no such symbols."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import edge_checks as ec  # noqa: E402
from tests import part_checks as pc  # noqa: E402
from tests import stream_checks as sc  # noqa: E402
from tests import test_buffer_contract_gpu as tb  # noqa: E402

ERR_ARG = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def on(dev):
    return lambda x, taps, block, k: sc.device(dev, x, taps, block, k)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("block,T", sc.SHAPES)
@pytest.mark.parametrize("channels", sc.CHANNELS)
def test_parity_every_family(dev, oracle, block, T, channels):
    """both parities of log2 block, P = 1, a last partition holding one tap, workgroups of one wave (block 64), of two and of
    four, threads owning 1, 2, 8 and 16 bins; 3 and 37 channels, one of them scaled by 2^-10; the ring goes once around"""
    sc.check_shape(on(dev), oracle, block, T, channels)


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "rows"])
def test_longest_filter(dev, oracle, per_channel):
    """131073 taps in 1025 partitions of 128: 6 calls and a flush of 1024 blocks, one tap set and a row per channel"""
    sc.check_shape(on(dev), oracle, 128, sc.MAX_TAPS, 2, calls=6, per_channel=per_channel)


# ------------------------------------------------------------------------------------------------ 2. ring and call splitting
def test_ring_wraps_and_call_grouping_keeps_the_bits(dev, oracle):
    """(64, 199), k = 3: R = 6 slots, not a power of two, 2 R + 1 calls: two wraps; the same stream through a k = 1 handle gives
    the same bits -- a block's arithmetic does not depend on how calls group the blocks"""
    block, T, k, calls = 64, 199, 3, 13
    assert sc.partitions(T, block) + k - 1 == 6 and calls == 2 * 6 + 1
    sc.check_shape(on(dev), oracle, block, T, 3, k=k, calls=calls)
    x = sc.signal(oracle, 3, calls * k * block, seed=1 + T + block)
    h = ec.dense_taps(T, seed=T)
    y3, y1 = sc.device(dev, x, h, block, k), sc.device(dev, x, h, block, 1)
    assert np.isfinite(y3).all() and np.array_equal(sc.bits(y3), sc.bits(y1))


# ------------------------------------------------------------------------------------------------ 3. isolation
@pytest.mark.parametrize("block,T", [(64, 199), (512, 1300), (2048, 2300)])
def test_channels_are_independent_to_the_bit(dev, oracle, block, T):
    """run B = run A with channels 1 and 4 zeroed and channels 2 and 5 scaled by 2^20: channels 0 and 3 keep their bits, the
    zeroed ones give exactly 0.0, the scaled ones 2^20 times run A bit for bit; run A on a fresh handle repeats its bits"""
    n = sc.calls_for(block, T) * block
    xa = sc.signal(oracle, 6, n, seed=7 + T).copy()
    xb = xa.copy()
    xb[[1, 4]] = 0.0
    xb[[2, 5]] *= np.float32(2.0 ** 20)
    h = ec.dense_taps(T, seed=T)
    ya, ya2, yb = (sc.device(dev, x, h, block) for x in (xa, xa, xb))
    assert ya.shape == (6, n + T - 1) and np.isfinite(ya).all() and np.isfinite(yb).all()
    assert np.array_equal(sc.bits(ya), sc.bits(ya2)), "the same calls on a fresh handle gave other bits"
    for c in (0, 3):
        assert np.array_equal(sc.bits(ya[c]), sc.bits(yb[c])), f"channel {c} changed with its neighbours"
    for c in (1, 4):
        assert np.all(yb[c] == 0.0), f"channel {c}: zero input, non-zero output"
    for c in (2, 5):
        assert np.array_equal(sc.bits(ya[c] * np.float32(2.0 ** 20)), sc.bits(yb[c])), f"channel {c}: not 2^20 times run A"


@pytest.mark.parametrize("block,T", [(64, 199), (512, 1300), (2048, 2300)])
def test_rows_that_differ_and_rows_that_are_equal(dev, oracle, block, T):
    """a tap row per channel, every row different: each channel is held to its own taps, and its neighbour's taps miss the
    gate; rows that are all equal give the bits of the shared handle"""
    channels = 5
    n = sc.calls_for(block, T) * block
    x = sc.signal(oracle, channels, n, seed=11 + T)
    rows = np.stack([ec.dense_taps(T, seed=T + 17 * c) for c in range(channels)])
    y = sc.device(dev, x, rows, block)
    xz = sc.padded(x, T)
    for c in range(channels):
        ref = oracle.fir_batch_f32(xz[c:c + 1], rows[c])
        pc.check_dense(y[c:c + 1], ref, n, f"rows block {block} T={T} ch {c} own taps")
        other = oracle.fir_batch_f32(xz[c:c + 1], rows[(c + 1) % channels])
        assert pc.rel_rms(y[c, :n], other[0, :n]) > 1e3 * ec.TOL, f"channel {c} also fits its neighbour's taps"
    shared = sc.device(dev, x, rows[2], block)
    equal = sc.device(dev, x, np.tile(rows[2], (channels, 1)), block)
    assert np.array_equal(sc.bits(shared), sc.bits(equal)), "equal rows and the shared handle differ"


# ------------------------------------------------------------------------------------------------ 4. state
def test_set_taps_mid_stream(dev, oracle):
    """channel 1 of 3 gets new taps after call 4 of 9: channels 0 and 2 are bit-identical to a run without it; channel 1 is
    the old taps before, and from that call on the new taps applied to the WHOLE stream (the history lives as input spectra)"""
    block, T, calls, at = 128, 700, 9, 4
    n = calls * block
    x = sc.signal(oracle, 3, n, seed=5 + T)
    old = np.stack([ec.dense_taps(T, seed=T + c) for c in range(3)])
    new = ec.dense_taps(T, seed=T + 99)
    plain = sc.device(dev, x, old, block)
    f = filters.FirStreamMC(3, block, old)
    outs = sc.stream_calls(dev, f, x[:, :at * block])
    f.set_taps(1, new[None, :])
    outs += sc.stream_calls(dev, f, x[:, at * block:])
    tail = torch.full((3, T - 1), float("nan"), dtype=torch.float32, device=dev)
    f.flush(tail)
    f.close()
    y = np.concatenate(outs + [tail.cpu().numpy()], axis=1)
    for c in (0, 2):
        assert np.array_equal(sc.bits(y[c]), sc.bits(plain[c])), f"channel {c} changed with channel 1's taps"
    assert np.array_equal(sc.bits(y[1, :at * block]), sc.bits(plain[1, :at * block]))
    xz = sc.padded(x, T)
    ref = oracle.fir_batch_f32(xz[1:2], new)
    pc.check_dense(y[1:2, at * block:], ref[:, at * block:], n - at * block, "set_taps: channel 1 from the call on")
    assert pc.rel_rms(y[1, at * block:n], plain[1, at * block:n]) > 1e3 * ec.TOL, "the new taps changed nothing"
    with pytest.raises(capi.LlzError, match="llz_fir_stream_mc_set_taps"):
        g = filters.FirStreamMC(3, block, old[0])
        try:
            g.set_taps(1, new[None, :])                         # one tap set for all channels: only row 0
        finally:
            g.close()


@pytest.mark.parametrize("how", ["flush", "reset"])
def test_flush_and_reset_start_over(dev, oracle, how):
    """flush (or reset), then the same input again: the bits of a fresh handle, frames and flush"""
    block, T = 64, 199
    n = sc.calls_for(block, T) * block
    x = sc.signal(oracle, 3, n, seed=3 + T)
    h = ec.dense_taps(T, seed=T)
    fresh = sc.device(dev, x, h, block)
    f = filters.FirStreamMC(3, block, h)
    tail = torch.full((3, T - 1), float("nan"), dtype=torch.float32, device=dev)
    first = sc.stream_calls(dev, f, x[:, :5 * block])          # leaves the head mid-ring
    if how == "flush":
        f.flush(tail)
        assert np.array_equal(sc.bits(np.concatenate(first, axis=1)), sc.bits(fresh[:, :5 * block]))
    else:
        f.reset()
    again = sc.stream_calls(dev, f, x)
    tail.fill_(float("nan"))
    f.flush(tail)
    f.close()
    got = np.concatenate(again + [tail.cpu().numpy()], axis=1)
    assert np.array_equal(sc.bits(got), sc.bits(fresh)), f"after {how} the handle is not a fresh one"


def test_flush_with_one_tap_only_starts_over(dev, oracle):
    """flt_len == 1: the flush has nothing to emit (an empty buffer or None) and still resets the delay line: block 64's
    previous block is zeros again, so the same input gives the bits of a fresh handle"""
    block, n = 64, 3 * 64
    x = sc.signal(oracle, 3, n, seed=17)
    h = np.array([0.75])
    fresh = sc.device(dev, x, h, block)
    assert fresh.shape == (3, n) and np.isfinite(fresh).all()
    f = filters.FirStreamMC(3, block, h)
    sc.stream_calls(dev, f, x[:, :2 * block])
    assert f.flush(None) is None
    again = sc.stream_calls(dev, f, x)
    f.flush(torch.empty((3, 0), dtype=torch.float32, device=dev))
    f.close()
    assert np.array_equal(sc.bits(np.concatenate(again, axis=1)), sc.bits(fresh))


# ------------------------------------------------------------------------------------------------ 5. buffers
def run_guarded(dev, oracle, io, block, T, k):
    channels, calls = 3, 3
    n = calls * k * block
    x = sc.signal(oracle, channels, n, seed=9 + T)
    h = ec.dense_taps(T, seed=T)
    f = filters.FirStreamMC(channels, block, h, frame_len=k * block)
    ys = []
    for o in range(0, n, k * block):
        y = io.out(tb.F32, channels, k * block)
        f.filter(io.inp(x[:, o:o + k * block]), y)
        ys.append(y)
    tail = io.out(tb.F32, channels, T - 1)
    f.flush(tail)
    io.verify("fir stream")
    f.close()
    for i, buf in enumerate(io.outs):
        bc.check_all_written(buf, f"fir stream: output {i}")
    got = np.concatenate([tb.host(t) for t in ys + [tail]], axis=1)
    pc.check_dense(got, sc.dense_ref(oracle, x, h), n, f"fir stream guarded block {block} k={k}")
    return got


@pytest.mark.parametrize("off", tb.OFF32, ids=[f"in{o[0]}-out{o[1]}" for o in tb.OFF32])
@pytest.mark.parametrize("block,T,k", [(64, 199, 2), (1024, 1300, 1)])
def test_guarded_buffers(dev, oracle, block, T, k, off):
    """outputs between sentinel bands, inputs between NaN bands, carved at odd element offsets: bands and inputs bit-unchanged,
    every output element written, the result under the gate"""
    run_guarded(dev, oracle, tb.Io(dev, off, "nan"), block, T, k)


@pytest.mark.parametrize("block,T,k", [(64, 199, 2), (1024, 1300, 1)])
def test_host_pointers_give_the_bits_of_device_pointers(dev, oracle, block, T, k):
    a = run_guarded(dev, oracle, tb.Io(torch.device("cpu"), (1, 3), "nan"), block, T, k)
    b = run_guarded(dev, oracle, tb.Io(dev, (1, 3), "nan"), block, T, k)
    assert np.array_equal(sc.bits(a), sc.bits(b))


def test_overlap_refused(dev):
    L = capi.lib()
    f = filters.FirStreamMC(2, 64, ec.dense_taps(199, seed=199), frame_len=1024)
    tb.refused(bc.overlap_cases(2048, device=dev), lambda a, b: L.llz_fir_stream_mc(f.handle, tb.dptr(a), tb.dptr(b), 1024),
               "llz_fir_stream_mc")
    a = torch.zeros(2048, device=dev)
    assert L.llz_fir_stream_mc(f.handle, C.c_void_p(a.data_ptr()), C.c_void_p(a.data_ptr()), 1024) == ERR_ARG
    assert "llz_fir_stream_mc" in capi.last_error()
    f.close()
