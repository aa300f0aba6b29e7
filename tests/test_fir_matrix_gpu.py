"""GPU: llz_fir_matrix_mc, the many-in, many-out stream convolver y_o = sum_i x_i * h[o][i] (fir_matrix.hip: forward transforms,
the product summed over inputs in G groups, inverse transforms; a frequency-domain delay line per input).  Cases, inputs,
references, limits and the numpy model they were sized on: tests/matrix_checks.py; tests/test_fir_matrix_host.py runs the same
cases through the model on a machine without a GPU.  Device tensors, outputs preset to NaN; every parity case prints its worst
ratio to its limit (-s).  The parent of this feature has no such symbols."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import edge_checks as ec  # noqa: E402
from tests import matrix_checks as mc  # noqa: E402
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
    return lambda x, taps, block, k: mc.device(dev, x, taps, block, k)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("block,T,inputs,outputs", mc.SHAPES)
def test_parity_dense_and_sparse(dev, oracle, block, T, inputs, outputs):
    """every block size class of the three kernels, P = 1, a last partition holding one tap, inputs != outputs both ways, one
    input scaled by 2^-10; the ring goes once around and two blocks further, then the flush; the plan -- G and the connected
    paths with it -- is asserted in mc.device.  37 -> 2 runs in 19 groups with a ragged last one, 1 -> 2 in one"""
    mc.check_shape(on(dev), oracle, block, T, inputs, outputs)


def test_group_kinds_are_on_the_list():
    gs = [mc.groups(s[2], s[3], s[0])[0] for s in mc.SHAPES]
    assert any(G > 1 and s[2] % G for s, G in zip(mc.SHAPES, gs)) and any(G == 1 for G in gs), gs


def test_longest_filter(dev, oracle):
    """131073 taps in 1025 partitions of 128, 2 -> 2: 6 calls and a flush of 1024 blocks"""
    block, T, inputs, outputs = mc.LONGEST
    mc.check_shape(on(dev), oracle, block, T, inputs, outputs, calls=6)


def test_flush_in_passes(dev, oracle):
    """16 -> 8 at block 4096 and 81921 taps: the flush's 20 blocks go through the partial-spectra scratch in passes of 16 and 4"""
    block, T, inputs, outputs = mc.PASSES
    mc.check_dense(on(dev), oracle, block, T, inputs, outputs, calls=1)


# ------------------------------------------------------------------------------------------------ 2. ring and call splitting
def test_ring_wraps_and_call_grouping_keeps_the_bits(dev, oracle):
    """(64, 199), k = 3, 3 -> 2: R = 6 slots, 2 R + 1 calls: two wraps; the same stream through a k = 1 handle gives the same
    bits, and so does a second fresh handle"""
    block, T, k, calls = 64, 199, 3, 13
    assert mc.partitions(T, block) + k - 1 == 6 and calls == 2 * 6 + 1
    mc.check_shape(on(dev), oracle, block, T, 3, 2, k=k, calls=calls)
    x, _ = mc.case_signal(oracle, block, T, 3, k, calls)
    h = mc.dense_matrix(T, 3, 2)
    y3, y3b, y1 = mc.device(dev, x, h, block, k), mc.device(dev, x, h, block, k), mc.device(dev, x, h, block, 1)
    assert np.isfinite(y3).all() and np.array_equal(mc.bits(y3), mc.bits(y1)) and np.array_equal(mc.bits(y3), mc.bits(y3b))


# ------------------------------------------------------------------------------------------------ 3. paths
@pytest.mark.parametrize("block,T", [(64, 199), (512, 1300), (2048, 2300)])
def test_one_path_at_a_time_is_the_stream_convolver(dev, oracle, block, T):
    """3 -> 2, six distinct dense tap sets: with every input but i zeroed, output o equals -- value for value -- a one-channel
    FirStreamMC with h[o][i] on x_i, frames and flush; held against h[i'][o'] of the transposed indexing it misses the gate"""
    inputs, outputs = 3, 2
    x, n = mc.case_signal(oracle, block, T, inputs)
    h = mc.dense_matrix(T, inputs, outputs)
    flat = h.reshape(inputs, outputs, T)                         # what indexing H (i, o) would pick up
    xz = mc.padded(x, T)
    for i in range(inputs):
        xi = np.zeros_like(x)
        xi[i] = x[i]
        y = mc.device(dev, xi, h, block)
        for o in range(outputs):
            one = sc.device(dev, x[i:i + 1], h[o, i], block)
            assert np.isfinite(y[o]).all() and np.all(y[o] == one[0]), f"path ({o}, {i}) is not the stream convolver's"
            wrong = mc.fir1(oracle, xz[i:i + 1], np.ascontiguousarray(flat[i, o]))
            if not np.array_equal(flat[i, o], h[o, i]):
                assert pc.rel_rms(y[o, :n], wrong[:n]) > 1e3 * ec.TOL, f"output {o} also fits the transposed path of input {i}"


def test_rows_are_independent_to_the_bit(dev, oracle):
    """3 -> 3: replacing row 1's taps leaves the bits of outputs 0 and 2, and changes output 1"""
    block, T = 64, 199
    x, n = mc.case_signal(oracle, block, T, 3)
    a = mc.dense_matrix(T, 3, 3)
    b = a.copy()
    b[1] = mc.dense_matrix(T + 1, 3, 3)[1][:, :T]
    ya, yb = mc.device(dev, x, a, block), mc.device(dev, x, b, block)
    for o in (0, 2):
        assert np.array_equal(mc.bits(ya[o]), mc.bits(yb[o])), f"output {o} changed with row 1's taps"
    assert pc.rel_rms(yb[1], ya[1]) > 1e3 * ec.TOL


def test_unconnected_paths_pass_nothing_on(dev, oracle):
    """h[0][1] all zero, NaN and Inf blocks in x_1: output 0 is finite and bit-equal to the run with x_1 zeroed, output 1 is NaN
    where the input was; plan counts O I - 1 paths, and set_taps connecting and disconnecting the path moves the count"""
    block, T, inputs, outputs = 64, 199, 3, 2
    x, n = mc.case_signal(oracle, block, T, inputs)
    h = mc.dense_matrix(T, inputs, outputs).copy()
    h[0, 1] = 0.0
    xn, xz = x.copy(), x.copy()
    xn[1, block:2 * block] = np.nan
    xn[1, 3 * block:4 * block] = np.inf
    xz[1] = 0.0
    y, yz = mc.device(dev, xn, h, block), mc.device(dev, xz, h, block)     # mc.device asserts plan()[5] == O I - 1
    assert np.isfinite(y[0]).all(), "an unconnected path passed a NaN or an Inf on"
    assert np.array_equal(mc.bits(y[0]), mc.bits(yz[0]))
    assert np.isnan(y[1, block:2 * block]).all() and not np.isfinite(y[1, 3 * block:4 * block]).any()
    f = filters.FirMatrixMC(inputs, outputs, block, h)
    assert f.plan()[5] == inputs * outputs - 1
    f.set_taps(0, 1, mc.dense_matrix(T, inputs, outputs)[0, 1])
    assert f.plan()[5] == inputs * outputs
    got = np.concatenate(mc.stream_calls(dev, f, xn), axis=1)
    assert np.isnan(got[0, block:2 * block]).all(), "the path connected by set_taps carries nothing"
    f.set_taps(0, 1, np.zeros(T))
    assert f.plan()[5] == inputs * outputs - 1
    f.reset()
    again = np.concatenate(mc.stream_calls(dev, f, xn) + [mc.flushed(dev, f)], axis=1)
    f.close()
    assert np.array_equal(mc.bits(again[0]), mc.bits(y[0])), "the path disconnected by set_taps still carries something"


# ------------------------------------------------------------------------------------------------ 4. state
def test_set_taps_mid_stream(dev, oracle):
    """(128, 700), 3 -> 3: output 1's row gets new taps after call 4 of 9: outputs 0 and 2 are bit-identical to a run without
    it; output 1 is the old taps before, and from that call on the new taps applied to the WHOLE stream"""
    block, T, calls, at = 128, 700, 9, 4
    n = calls * block
    x = mc.signal(oracle, 3, n, seed=5 + T)
    old = mc.dense_matrix(T, 3, 3)
    new = old.copy()
    new[1] = mc.dense_matrix(T + 1, 3, 3)[1][:, :T]
    plain = mc.device(dev, x, old, block)
    f = filters.FirMatrixMC(3, 3, block, old)
    outs = mc.stream_calls(dev, f, x[:, :at * block])
    f.set_taps(1, 0, new[1:2])
    outs += mc.stream_calls(dev, f, x[:, at * block:])
    y = np.concatenate(outs + [mc.flushed(dev, f)], axis=1)
    f.close()
    for o in (0, 2):
        assert np.array_equal(mc.bits(y[o]), mc.bits(plain[o])), f"output {o} changed with output 1's taps"
    assert np.array_equal(mc.bits(y[1, :at * block]), mc.bits(plain[1, :at * block]))
    ref = mc.dense_ref(oracle, x, new)
    pc.check_dense(y[1:2, at * block:], ref[1:2, at * block:], n - at * block, "set_taps: output 1 from the call on")
    assert pc.rel_rms(y[1, at * block:n], plain[1, at * block:n]) > 1e3 * ec.TOL, "the new taps changed nothing"
    g = filters.FirMatrixMC(3, 3, block, old)
    with pytest.raises(capi.LlzError, match="llz_fir_matrix_mc_set_taps"):
        g.set_taps(2, 0, new[1:3])                               # rows 2 and 3 of 3
    with pytest.raises(capi.LlzError, match="llz_fir_matrix_mc_set_taps"):
        g.set_taps(0, 2, new[:1, :2])                            # inputs 2 and 3 of 3
    g.close()


@pytest.mark.parametrize("how", ["flush", "reset"])
def test_flush_and_reset_start_over(dev, oracle, how):
    """flush (or reset) after an odd number of calls, then the same input again: the bits of a fresh handle, frames and flush"""
    block, T = 64, 199
    x, n = mc.case_signal(oracle, block, T, 3)
    h = mc.dense_matrix(T, 3, 2)
    fresh = mc.device(dev, x, h, block)
    f = filters.FirMatrixMC(3, 2, block, h)
    first = mc.stream_calls(dev, f, x[:, :5 * block])          # leaves the head mid-ring and the last blocks swapped
    if how == "flush":
        mc.flushed(dev, f)
        assert np.array_equal(mc.bits(np.concatenate(first, axis=1)), mc.bits(fresh[:, :5 * block]))
    else:
        f.reset()
    got = np.concatenate(mc.stream_calls(dev, f, x) + [mc.flushed(dev, f)], axis=1)
    f.close()
    assert np.array_equal(mc.bits(got), mc.bits(fresh)), f"after {how} the handle is not a fresh one"


def test_flush_with_one_tap_only_starts_over(dev, oracle):
    """flt_len == 1: the flush has nothing to emit (an empty buffer or None), returns 0 and still resets the delay lines"""
    block, n = 64, 3 * 64
    x = mc.signal(oracle, 2, n, seed=17)
    h = np.array([[[0.75], [0.5]], [[-0.25], [1.0]]])
    fresh = mc.device(dev, x, h, block)
    assert fresh.shape == (2, n) and np.isfinite(fresh).all()
    f = filters.FirMatrixMC(2, 2, block, h)
    mc.stream_calls(dev, f, x[:, :2 * block])
    assert capi.lib().llz_fir_matrix_mc_flush(f.handle, None) == 0
    again = mc.stream_calls(dev, f, x)
    f.flush(torch.empty((2, 0), dtype=torch.float32, device=dev))
    f.close()
    assert np.array_equal(mc.bits(np.concatenate(again, axis=1)), mc.bits(fresh))


# ------------------------------------------------------------------------------------------------ 5. buffers
def run_guarded(dev, oracle, io, block, T, k, inputs, outputs):
    calls = 3
    n = calls * k * block
    x = mc.signal(oracle, inputs, n, seed=9 + T)
    h = mc.dense_matrix(T, inputs, outputs)
    f = filters.FirMatrixMC(inputs, outputs, block, h, frame_len=k * block)
    ys = []
    for s in range(0, n, k * block):
        y = io.out(tb.F32, outputs, k * block)
        f.filter(io.inp(x[:, s:s + k * block]), y)
        ys.append(y)
    tail = io.out(tb.F32, outputs, T - 1)
    f.flush(tail)
    io.verify("fir matrix")
    f.close()
    for i, buf in enumerate(io.outs):
        bc.check_all_written(buf, f"fir matrix: output {i}")
    got = np.concatenate([tb.host(t) for t in ys + [tail]], axis=1)
    pc.check_dense(got, mc.dense_ref(oracle, x, h), n, f"fir matrix guarded block {block} k={k} {inputs}->{outputs}")
    return got


GUARDED = [(64, 199, 2, 3, 5), (1024, 1300, 1, 5, 2)]


@pytest.mark.parametrize("off", tb.OFF32, ids=[f"in{o[0]}-out{o[1]}" for o in tb.OFF32])
@pytest.mark.parametrize("block,T,k,inputs,outputs", GUARDED)
def test_guarded_buffers(dev, oracle, block, T, k, inputs, outputs, off):
    """outputs between sentinel bands, inputs between NaN bands, carved at odd element offsets, inputs != outputs: bands and
    inputs bit-unchanged, every output element written, the result under the gate"""
    run_guarded(dev, oracle, tb.Io(dev, off, "nan"), block, T, k, inputs, outputs)


@pytest.mark.parametrize("block,T,k,inputs,outputs", GUARDED)
def test_host_pointers_give_the_bits_of_device_pointers(dev, oracle, block, T, k, inputs, outputs):
    a = run_guarded(dev, oracle, tb.Io(torch.device("cpu"), (1, 3), "nan"), block, T, k, inputs, outputs)
    b = run_guarded(dev, oracle, tb.Io(dev, (1, 3), "nan"), block, T, k, inputs, outputs)
    assert np.array_equal(mc.bits(a), mc.bits(b))


def test_overlap_refused(dev):
    """3 -> 5 at frame_len 1024: in holds 3072 floats, out 5120; overlapping device ranges and in == out are refused"""
    L = capi.lib()
    f = filters.FirMatrixMC(3, 5, 64, mc.dense_matrix(199, 3, 5), frame_len=1024)
    tb.refused(bc.overlap_cases(3072, 5120, device=dev), lambda a, b: L.llz_fir_matrix_mc(f.handle, tb.dptr(a), tb.dptr(b), 1024),
               "llz_fir_matrix_mc")
    a = torch.zeros(5120, device=dev)
    assert L.llz_fir_matrix_mc(f.handle, C.c_void_p(a.data_ptr()), C.c_void_p(a.data_ptr()), 1024) == ERR_ARG
    assert "llz_fir_matrix_mc" in capi.last_error()
    f.close()
