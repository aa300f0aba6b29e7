"""GPU: llz_fir_xfade_matrix_mc, the matrix convolver's click-free change of paths (fir_matrix_fade.hip: K4g's product with a second
table of spectra and a second set of partial sums from one walk of the rings, the two outputs blended per sample after the sum
over inputs).  Cases, inputs, references, limits and the numpy model they were sized on: tests/matrix_fade_checks.py;
tests/test_fir_matrix_fade_host.py runs the same cases through the model on a machine without a GPU.  Device tensors, outputs
preset to NaN; every parity case prints its worst ratios to its limits (-s).  The parent of this feature has no such symbols."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import fade_checks as fc  # noqa: E402
from tests import matrix_checks as mc  # noqa: E402
from tests import matrix_fade_checks as mf  # noqa: E402
from tests import test_buffer_contract_gpu as tb  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("block,T,inputs,outputs,F", mf.SHAPES)
def test_parity_dense_and_sparse(dev, oracle, block, T, inputs, outputs, F):
    """one tap, a last partition of one tap, 19 groups with a ragged last one, groups of one input, one and two bins per thread,
    several bin tiles, the largest LDS image, fades of one block and of several; the last column fades joined by a lone path as a
    second call; in the sparse case a source fades in and another fades out"""
    mf.check_shape(mf.on_device(dev), oracle, block, T, inputs, outputs, F)


def test_longest_filter(dev, oracle):
    """131073 taps in 1025 partitions of 128, 2 -> 2, a fade of two blocks from block 3 of 8: the flush of 1024 blocks behind it
    runs every partition of the new taps; dense reference by part_checks.fft_ref"""
    block, T, inputs, outputs, F = mf.LONGEST
    mf.check_shape(mf.on_device(dev), oracle, block, T, inputs, outputs, F, start=3, blocks=8)


# ------------------------------------------------------------------------------------------------ 2. bit pins
@pytest.mark.parametrize("block,T", [(64, 199), (512, 1300), (2048, 2300)])
def test_bit_pins(dev, oracle, block, T):
    """3 -> 2, column 1 fading over F = 3: up to and including the first faded sample the never-fading handle's bits; the fade
    span differs from it; a fade to equal taps changes no bit; from the fade's end on, every block and the flush have the bits of
    a handle given set_taps(new) at the block where the fade ends"""
    mf.check_bit_pins(mf.on_device(dev), oracle, block, T, 3)


def test_call_grouping_keeps_the_bits(dev, oracle):
    """(64, 199, F = 4, 3 -> 2) through k = 3 and k = 1 calls: the fade ends inside a call of three; the same bits"""
    mf.check_call_grouping(mf.on_device(dev), oracle)


@pytest.mark.parametrize("block,T", [(64, 199), (2048, 2300)])
def test_one_path_at_a_time_is_the_stream_fade(dev, oracle, block, T):
    """3 -> 2 with every input but i zeroed and path (o, i) fading: output o equals, value for value, a one-channel FirStreamMC
    on x_i given fade_taps at the same block -- the one-pass stream kernel at block 64, the two-pass one at 2048"""
    mf.check_one_path_is_the_stream_fade(mf.on_device(dev), fc.on_device(dev), oracle, block, T)


# ------------------------------------------------------------------------------------------------ 3. outputs and paths
def test_outputs_fade_alone(dev, oracle):
    """5 -> 37: the paths (3..5, 2) and (20, 4) fade as two calls joining one pending fade: every other output keeps the bits of a
    handle that never fades, and inputs the fading outputs are not connected to, scaled by 2^20 or zeroed, change no bit of them"""
    mf.check_outputs_fade_alone(mf.on_device(dev), oracle)


def test_fade_in_and_fade_out(dev, oracle):
    """a path with zero old taps fades in (no NaN of its input before, the source within the sparse limit after); a path fades to
    zero taps (no NaN or Inf of its input afterwards, one connected path less); plan()[5] during a fade is the union's count"""
    assert mf.check_fade_in_and_out(mf.on_device(dev), oracle) <= 1.0


# ------------------------------------------------------------------------------------------------ 4. state
def test_fade_left_refusals_and_reset(dev, oracle):
    """fade_left counts down across calls; set_taps, a second fade and one of another length are refused mid-fade and accepted
    after; reset mid-fade gives the bits of a fresh handle with the new taps; close with a fade pending"""
    mf.check_state(mf.on_device(dev), oracle)


def test_refusals_carry_their_own_messages(dev):
    """(out_first, out_count, in_first, in_count, taps, fade_blocks) on a live handle: each refusal names the function and what it
    missed, no two kinds share a message, and none of them starts a fade"""
    L = capi.lib()
    T = 199
    taps = np.ascontiguousarray(mc.dense_matrix(T, 3, 2), dtype=np.float32)
    f = filters.FirMatrixMC(3, 2, 64, taps)
    seen = {}

    def refused(what, h, *args):
        L.llz_hip_tune(b"no_such_override", 0)
        assert L.llz_fir_xfade_matrix_mc(h, *args) == -1, what
        msg = capi.last_error()
        assert "llz_fir_xfade_matrix_mc" in msg, (what, msg)
        seen[what] = msg
    p = taps.ctypes.data
    refused("handle", 0, 0, 1, 0, 1, p, 3)
    refused("taps", f.handle, 0, 1, 0, 1, None, 3)
    refused("outputs", f.handle, 1, 2, 0, 1, p, 3)
    assert "outputs [1, 1 + 2)" in seen["outputs"] and "[0, 2)" in seen["outputs"]
    refused("inputs", f.handle, 0, 1, 2, 2, p, 3)
    assert "inputs [2, 2 + 2)" in seen["inputs"] and "[0, 3)" in seen["inputs"]
    for blocks in (0, -1, 4097):
        refused("blocks", f.handle, 0, 1, 0, 1, p, blocks)
        assert "1..4096" in seen["blocks"] and str(blocks) in seen["blocks"]
    assert f.fade_left() == 0 and f.plan()[5] == 6
    f.fade_taps(1, 2, taps[0, 0], 4096)
    refused("pending", f.handle, 0, 1, 0, 1, p, 5)
    assert "4096 of its 4096 blocks left" in seen["pending"] and "same fade_blocks" in seen["pending"]
    with pytest.raises(capi.LlzError, match="llz_fir_matrix_mc_set_taps.*4096 of its 4096 blocks left"):
        f.set_taps(0, 0, taps[0, 0])
    with pytest.raises(capi.LlzError, match="taps must be"):
        f.fade_taps(0, 0, taps[0, 0, :-1], 4096)
    assert f.fade_left() == 4096
    assert len(set(seen.values())) == len(seen), seen
    f.close()


def test_flush_mid_fade(dev, oracle):
    """(64, 199, 3 -> 2, F = 6): after two faded blocks the flush goes on with the ramp through its four zero blocks, held to the
    sparse limit, and leaves a handle that repeats a fresh new-taps handle's bits"""
    assert mf.check_flush_mid_fade(mf.on_device(dev), oracle) <= 1.0


def test_flush_mid_fade_in_passes(dev, oracle):
    """16 -> 8 at block 4096 and 81921 taps: one call, a one-column fade of F = 24, and the flush's 20 blocks in passes of 16 and
    4 while the ramp runs"""
    assert mf.check_flush_in_passes(mf.on_device(dev), oracle) <= 1.0


# ------------------------------------------------------------------------------------------------ 5. buffers
def run_guarded(dev, oracle, io, block, T, k, inputs, outputs, F):
    """k-block calls, the last column's fade requested before the second one, the flush with the fade still in flight: every call
    and the flush on guarded buffers"""
    calls = 3
    n = calls * k * block
    assert F > (calls - 1) * k                                      # still fading when the flush comes
    x = mc.signal(oracle, inputs, n, seed=9 + T)
    col = [(0, inputs - 1, outputs, 1)]
    old, new = mf.dense_pair(T, inputs, outputs, col)
    f = filters.FirMatrixMC(inputs, outputs, block, old, frame_len=k * block)
    ys = []
    for s in range(0, n, k * block):
        if s == k * block:
            f.fade_taps(0, inputs - 1, new[:, inputs - 1:], F)
        y = io.out(tb.F32, outputs, k * block)
        f.filter(io.inp(x[:, s:s + k * block]), y)
        ys.append(y)
    assert f.fade_left() == F - (calls - 1) * k
    tail = io.out(tb.F32, outputs, T - 1)
    f.flush(tail)
    io.verify("fir matrix fade")
    assert f.fade_left() == 0
    f.close()
    for i, buf in enumerate(io.outs):
        bc.check_all_written(buf, f"fir matrix fade: output {i}")
    got = np.concatenate([tb.host(t) for t in ys + [tail]], axis=1)
    w = mf.weights(n + T - 1, k * block, F * block)
    fc.check_dense(got, mf.dense_blend(oracle, w, x, old, new), k * block, F * block, n,
                   f"fir matrix fade guarded block {block} k={k} {inputs}->{outputs}")
    return got


GUARDED = [(64, 199, 2, 3, 2, 6), (2048, 2300, 1, 2, 3, 3)]


@pytest.mark.parametrize("off", tb.OFF32, ids=[f"in{o[0]}-out{o[1]}" for o in tb.OFF32])
@pytest.mark.parametrize("block,T,k,inputs,outputs,F", GUARDED)
def test_guarded_buffers(dev, oracle, block, T, k, inputs, outputs, F, off):
    """fading calls and a fading flush: outputs between sentinel bands, inputs between NaN bands, carved at odd element offsets:
    bands and inputs bit-unchanged, every output element written, under the gate"""
    run_guarded(dev, oracle, tb.Io(dev, off, "nan"), block, T, k, inputs, outputs, F)


@pytest.mark.parametrize("block,T,k,inputs,outputs,F", GUARDED)
def test_host_pointers_give_the_bits_of_device_pointers(dev, oracle, block, T, k, inputs, outputs, F):
    a = run_guarded(dev, oracle, tb.Io(torch.device("cpu"), (1, 3), "nan"), block, T, k, inputs, outputs, F)
    b = run_guarded(dev, oracle, tb.Io(dev, (1, 3), "nan"), block, T, k, inputs, outputs, F)
    assert np.array_equal(mf.bits(a), mf.bits(b))
