"""GPU: llz_fir_xfade_stream_mc, the stream convolver's click-free change of taps (fir_stream_fade.hip: K4f's walk with a second
table of spectra, both filters on one delay line, blended per sample in the time domain).  Cases, inputs, references, limits and
the numpy model they were sized on: tests/fade_checks.py; tests/test_fir_fade_host.py runs the same cases through the model on a
machine without a GPU.  Device tensors, outputs preset to NaN; every parity case prints its worst ratio to its limits (-s).  The
parent of this feature has no such symbols."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import edge_checks as ec  # noqa: E402
from tests import fade_checks as fc  # noqa: E402
from tests import stream_checks as sc  # noqa: E402
from tests import test_buffer_contract_gpu as tb  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("block,T,F", fc.SHAPES)
@pytest.mark.parametrize("channels", fc.CHANNELS)
def test_parity_dense_and_sparse_pairs(dev, oracle, block, T, F, channels, per_channel):
    """one pass over the ring (blocks 64 .. 512) and two (2048, 4096), fades of one block and of several, P = 1 and a last
    partition of one tap; the fade starts after P + 1 blocks and P + 2 follow; a shared tap set and a row per channel"""
    fc.check_shape(fc.on_device(dev), oracle, block, T, F, channels, per_channel=per_channel)


def test_longest_filter(dev, oracle):
    """131073 taps in 1025 partitions of 128, two channels, a fade of two blocks from block 3 of 8: the flush of 1024 blocks
    behind it runs every partition of the new taps; dense reference by part_checks.fft_ref"""
    fc.check_shape(fc.on_device(dev), oracle, 128, sc.MAX_TAPS, 2, 2, start=3, blocks=8)


# ------------------------------------------------------------------------------------------------ 2. bit pins
@pytest.mark.parametrize("block,T", [(64, 199), (512, 1300), (1024, 1300), (2048, 2300)])
def test_bit_pins(dev, oracle, block, T):
    """the first faded sample equals the old-taps handle's; a fade to equal taps is bit-equal to no fade; every block after the
    fade is bit-equal to a handle given set_taps(new) at the block where the fade ends"""
    fc.check_bit_pins(fc.on_device(dev), oracle, block, T, 3)


def test_call_grouping_keeps_the_bits(dev, oracle):
    """(64, 199, F = 4) through k = 3 and k = 1 calls: the fade ends inside a call of three; the same bits"""
    fc.check_call_grouping(fc.on_device(dev), oracle)


# ------------------------------------------------------------------------------------------------ 3. bank isolation
def test_bank_rows_fade_alone(dev, oracle):
    """37 channels, rows 3 .. 5 and 20 fading as two calls that join one pending fade: every other channel keeps the bits of a
    handle that never fades, and neighbours scaled by 2^20 or zeroed change no bit of the fading rows"""
    fc.check_bank_isolation(fc.on_device(dev), oracle)


# ------------------------------------------------------------------------------------------------ 4. state
def test_fade_left_refusals_and_reset(dev, oracle):
    """fade_left counts down across calls; set_taps and a second fade are refused mid-fade and accepted after; reset mid-fade
    gives the bits of a fresh handle with the new taps"""
    fc.check_state(fc.on_device(dev), oracle)


def test_refusals_carry_their_own_messages(dev):
    """(first, count, taps, fade_blocks) on a live handle: each refusal names the function and what it missed, no two kinds
    share a message, and none of them starts a fade"""
    L = capi.lib()
    T = 199
    taps = np.ascontiguousarray(np.stack([ec.dense_taps(T, seed=T + c) for c in range(3)]), dtype=np.float32)
    f = filters.FirStreamMC(3, 64, taps)
    g = filters.FirStreamMC(3, 64, taps[0])
    seen = {}

    def refused(what, h, *args):
        L.llz_hip_tune(b"no_such_override", 0)
        assert L.llz_fir_xfade_stream_mc(h, *args) == -1, what
        msg = capi.last_error()
        assert "llz_fir_xfade_stream_mc" in msg, (what, msg)
        seen[what] = msg
    p = taps.ctypes.data
    refused("handle", 0, 0, 1, p, 3)
    refused("taps", f.handle, 0, 1, None, 3)
    refused("rows", f.handle, 2, 2, p, 3)
    assert "[0, 3)" in seen["rows"]
    refused("shared rows", g.handle, 1, 1, p, 3)
    assert "only first 0, count 1" in seen["shared rows"]
    for blocks in (0, -1, 4097):
        refused("blocks", f.handle, 0, 1, p, blocks)
        assert "1..4096" in seen["blocks"] and str(blocks) in seen["blocks"]
    assert f.fade_left() == 0 and g.fade_left() == 0
    f.fade_taps(1, taps[0], 4096)
    refused("pending", f.handle, 0, 1, p, 5)
    assert "4096 of its 4096 blocks left" in seen["pending"]
    with pytest.raises(capi.LlzError, match="llz_fir_stream_mc_set_taps.*4096 of its 4096 blocks left"):
        f.set_taps(0, taps[0])
    with pytest.raises(capi.LlzError, match="taps must be"):
        f.fade_taps(0, taps[0, :-1], 3)
    kinds = {k: v for k, v in seen.items() if k != "shared rows"}
    assert len(set(kinds.values())) == len(kinds), seen
    f.close()
    g.close()


def test_flush_mid_fade(dev, oracle):
    """(64, 199, F = 6): after two faded blocks the flush goes on with the ramp through its zero blocks, held to the sparse
    limit, and leaves a handle that repeats a fresh new-taps handle's bits"""
    assert fc.check_flush_mid_fade(fc.on_device(dev), oracle) <= 1.0


# ------------------------------------------------------------------------------------------------ 5. buffers
def run_guarded(dev, oracle, io, block, T, k, F):
    """k-block calls, the fade requested before the second one, the flush with the fade still in flight: every call and the
    flush on guarded buffers"""
    channels, calls = 3, 3
    n = calls * k * block
    assert F > (calls - 1) * k                                      # still fading when the flush comes
    x = sc.signal(oracle, channels, n, seed=9 + T)
    old, new = ec.dense_taps(T, seed=T), ec.dense_taps(T, seed=T + 7)
    f = filters.FirStreamMC(channels, block, old, frame_len=k * block)
    ys = []
    for o in range(0, n, k * block):
        if o == k * block:
            f.fade_taps(0, new, F)
        y = io.out(tb.F32, channels, k * block)
        f.filter(io.inp(x[:, o:o + k * block]), y)
        ys.append(y)
    assert f.fade_left() == F - (calls - 1) * k
    tail = io.out(tb.F32, channels, T - 1)
    f.flush(tail)
    io.verify("fir stream fade")
    assert f.fade_left() == 0
    f.close()
    for i, buf in enumerate(io.outs):
        bc.check_all_written(buf, f"fir stream fade: output {i}")
    got = np.concatenate([tb.host(t) for t in ys + [tail]], axis=1)
    w = fc.weights(n + T - 1, k * block, F * block)
    ref = (1.0 - w) * sc.dense_ref(oracle, x, old) + w * sc.dense_ref(oracle, x, new)
    fc.check_dense(got, ref, k * block, F * block, n, f"fir stream fade guarded block {block} k={k}")
    return got


@pytest.mark.parametrize("off", tb.OFF32, ids=[f"in{o[0]}-out{o[1]}" for o in tb.OFF32])
@pytest.mark.parametrize("block,T,k,F", [(64, 199, 2, 6), (2048, 2300, 1, 3)])
def test_guarded_buffers(dev, oracle, block, T, k, F, off):
    """a fading call and a fading flush (one pass at block 64, two at 2048): outputs between sentinel bands, inputs between
    NaN bands, carved at odd element offsets: bands and inputs bit-unchanged, every output element written, under the gate"""
    run_guarded(dev, oracle, tb.Io(dev, off, "nan"), block, T, k, F)


@pytest.mark.parametrize("block,T,k,F", [(64, 199, 2, 6), (2048, 2300, 1, 3)])
def test_host_pointers_give_the_bits_of_device_pointers(dev, oracle, block, T, k, F):
    a = run_guarded(dev, oracle, tb.Io(torch.device("cpu"), (1, 3), "nan"), block, T, k, F)
    b = run_guarded(dev, oracle, tb.Io(dev, (1, 3), "nan"), block, T, k, F)
    assert np.array_equal(sc.bits(a), sc.bits(b))
