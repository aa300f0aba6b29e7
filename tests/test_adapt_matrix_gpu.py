"""The multi-reference adaptive filter on the device (include/llz_adapt_matrix.h, llz_adapt_matrix_mc; kernels k_adaptx_power /
k_adaptx_error / k_adaptx_update of fir_adapt_matrix.hip on K4g's forward and product launches) against the float64 model of its
definition (tests/adapt_matrix_checks.py, where every limit is stated) and against the two handles it is held to bit for bit:

  1. inputs = 1: e, y and get_taps bit-equal to AdaptMC(channels = outputs) fed the one reference on every row;
  2. frozen: set_taps(h), every mu = 0: y bit-equal to FirMatrixMC(inputs, outputs, block, h), e bit-equal to float32(d) - y,
     get_taps within 2 u |h|, at every shape of the table;
  3. parity, taps, misalignment and convergence while adapting, on the table; the worst ratios are printed;
  4. call grouping: k = 3 against k = 1 over two wraps of the ring, bit-equal e, y and taps;
  5. update grouping: adapt_ppw = 1, 3 and 64 change no bit;
  6. isolation: the other outputs' d scaled by 2^20, zeroed or NaN; an output frozen among adapting ones, then released;
  7. hand-over and reset: get_taps into a FirMatrixMC and back into the frozen handle, reset(1) and reset(0), a sub-matrix;
  8. pointers and buffers: host and mixed pointers, guarded buffers at odd offsets, overlapping device ranges refused, foreign
     handles refused both ways.

test_adapt_matrix_host.py runs cases 2 to 7 with the numpy float32 model in the device's place.  On the parent of this feature
the library exports no llz_adapt_matrix_mc and every test here fails."""
import ctypes as C

import numpy as np
import pytest
import torch

from llzlab_amd import capi, filters
from tests import adapt_checks as ac
from tests import adapt_matrix_checks as xc
from tests import buffer_checks as bc
from tests import matrix_checks as mc

pytestmark = pytest.mark.gpu
F32 = torch.float32
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 3)]                  # elements past a 256-byte boundary: (inputs, outputs)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def matrix_run(dev):
    """x through a FirMatrixMC with the paths h, a block per call: the frames"""
    def run(x, h, block):
        O, I, _ = np.shape(h)
        f = filters.FirMatrixMC(I, O, block, np.asarray(h, np.float64), frame_len=block)
        y = np.concatenate(mc.stream_calls(dev, f, np.asarray(x, np.float32)), axis=1)
        f.close()
        return y
    return run


@pytest.mark.parametrize("block,T,nblocks", [(64, 199, 12), (128, 513, 12), (2048, 2049, 6)])
def test_one_input_has_the_single_reference_filters_bits(dev, oracle, block, T, nblocks):
    """case 1: 3 outputs on one reference against AdaptMC(channels = 3) with that reference on every row"""
    outputs = 3
    x, d, _ = xc.case(oracle, block, T, 1, outputs, nblocks)
    delta = xc.delta_for(block, 1)
    r = xc.Device(dev, 1, outputs, block, T, 2 * block, xc.MU, delta)
    e, y = r.process(x, d)
    w = r.get_taps()
    r.close()
    s = ac.Device(dev, outputs, block, T, 2 * block, ac.MU, delta)
    es, ys = s.process(np.repeat(x, outputs, axis=0), d)
    ws = s.get_taps()
    s.close()
    assert np.any(w != 0) and np.all(np.isfinite(e))
    for got, want, name in ((e, es, "e"), (y, ys, "y"), (w[:, 0], ws, "taps")):
        assert np.array_equal(xc.bits(got), xc.bits(want)), f"{name}: {np.count_nonzero(xc.bits(got) != xc.bits(want))} values differ"


@pytest.mark.parametrize("shape", xc.SHAPES, ids=[f"{s[0]}-{s[1]}-{s[2]}to{s[3]}" for s in xc.SHAPES])
def test_frozen_path_has_the_matrix_convolvers_bits(dev, oracle, shape):
    xc.check_frozen(xc.device(dev), matrix_run(dev), oracle, exact=True, shapes=[shape])


@pytest.mark.parametrize("block,T,inputs,outputs,nblocks", xc.SHAPES)
def test_parity_and_taps_while_adapting(dev, oracle, block, T, inputs, outputs, nblocks):
    """case 3; the worst ratios are printed (holds the measured ones)"""
    xc.check_parity(xc.device(dev), oracle, block, T, inputs, outputs, nblocks)


def test_grouping_of_blocks_into_calls_changes_no_bit(dev, oracle):
    xc.check_grouping(xc.device(dev), oracle)


def test_grouping_of_partitions_into_workgroups_changes_no_bit(dev, oracle):
    """case 5: under the adapt_ppw override at (64, 199), P = 4: groups of 3 + 1 and one group of all 4 against one each"""
    block, T, inputs, outputs, _ = xc.RING
    x, d, _ = xc.case(oracle, block, T, inputs, outputs, 12)
    got = []
    for ppw in (1, 3, 64):
        with capi.tuned(adapt_ppw=ppw):
            r = xc.Device(dev, inputs, outputs, block, T, 2 * block)
            e, y = r.process(x, d)
            got.append((e, y, r.get_taps()))
            r.close()
    assert np.any(got[0][2] != 0)
    for other in got[1:]:
        for a, b, name in zip(got[0], other, ("e", "y", "taps")):
            assert np.array_equal(xc.bits(a), xc.bits(b)), name


def test_other_outputs_cannot_reach_an_output(dev, oracle):
    xc.check_isolation(xc.device(dev), oracle)


def test_a_frozen_output_among_adapting_ones(dev, oracle):
    xc.check_freeze_one(xc.device(dev), oracle)


def test_hand_over_to_the_matrix_convolver(dev, oracle):
    xc.check_handover(xc.device(dev), matrix_run(dev), oracle, exact=True)


def test_reset(dev, oracle):
    xc.check_reset(xc.device(dev), oracle)


def test_sub_matrix_round_trip_touches_only_its_paths(dev, oracle):
    w = xc.check_submatrix(xc.device(dev), oracle)
    # get_taps of the sub-matrix alone returns the same values
    f = filters.AdaptMatrixMC(3, 4, 64, 199, mu=0.0)
    f.set_taps(0, 0, w)
    assert np.array_equal(xc.bits(f.get_taps(1, 2, 1, 2)), xc.bits(f.get_taps()[1:3, 1:3]))
    f.close()


# ------------------------------------------------------------------------------------------------ pointers and buffers
CASE = (64, 199, 2, 3, 8)       # block, taps, inputs, outputs, blocks: two blocks per call


def run_calls(f, x, d, make_in, make_out, with_y=True):
    n = f.frame_len
    es, ys = [], []
    for o in range(0, x.shape[1], n):
        e, y = make_out(), (make_out() if with_y else None)
        f.process(make_in(x[:, o:o + n]), make_in(d[:, o:o + n]), e, y)
        es.append(e)
        ys.append(y)
    return es, ys


def gather(ts):
    return np.concatenate([t.detach().cpu().numpy() if hasattr(t, "detach") else t for t in ts], axis=1)


def fresh():
    block, T, inputs, outputs, _ = CASE
    return filters.AdaptMatrixMC(inputs, outputs, block, T, frame_len=2 * block, mu=xc.MU)


@pytest.fixture(scope="module")
def plain(dev, oracle):
    """the case on ordinary device tensors: (e, y, taps)"""
    block, T, inputs, outputs, nb = CASE
    x, d, _ = xc.case(oracle, block, T, inputs, outputs, nb)
    f = fresh()
    es, ys = run_calls(f, x, d, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev),
                       lambda: torch.full((outputs, 2 * block), float("nan"), dtype=F32, device=dev))
    w = f.get_taps()
    f.close()
    assert np.any(w != 0)
    return gather(es), gather(ys), w


def test_host_pointers_give_the_device_pointers_bits(dev, oracle, plain):
    block, T, inputs, outputs, nb = CASE
    x, d, _ = xc.case(oracle, block, T, inputs, outputs, nb)
    f = fresh()
    es, ys = run_calls(f, x, d, np.ascontiguousarray, lambda: np.full((outputs, 2 * block), np.nan, np.float32))
    w = f.get_taps()
    f.close()
    for got, want, name in ((gather(es), plain[0], "e"), (gather(ys), plain[1], "y"), (w, plain[2], "taps")):
        assert np.count_nonzero(xc.bits(got) != xc.bits(want)) == 0, name
    # mixed: x on the host, d on the device, no y
    f = fresh()
    n = 2 * block
    es = []
    for o in range(0, x.shape[1], n):
        e = torch.full((outputs, n), float("nan"), dtype=F32, device=dev)
        f.process(np.ascontiguousarray(x[:, o:o + n]), torch.from_numpy(np.ascontiguousarray(d[:, o:o + n])).to(dev), e)
        es.append(e)
    f.close()
    assert np.array_equal(xc.bits(gather(es)), xc.bits(plain[0]))


@pytest.mark.parametrize("off", OFFSETS, ids=[f"in{a}-out{b}" for a, b in OFFSETS])
def test_guarded_buffers(dev, oracle, plain, off):
    """x and d between NaN bands, e and y between sentinel bands, at odd element offsets: the plain tensors' bits, every output
    element written, the bands and the inputs unchanged"""
    block, T, inputs, outputs, nb = CASE
    x, d, _ = xc.case(oracle, block, T, inputs, outputs, nb)
    ins, outs = [], []

    def make_in(a):
        buf = bc.carve_input(dev, a, off[0])
        ins.append((buf, bc.snapshot(buf)))
        return buf.shaped(*a.shape)

    def make_out():
        buf = bc.carve(dev, F32, outputs * 2 * block, off[1])
        outs.append(buf)
        return buf.shaped(outputs, 2 * block)
    f = fresh()
    es, ys = run_calls(f, x, d, make_in, make_out)
    torch.cuda.synchronize()
    w = f.get_taps()
    f.close()
    for k, buf in enumerate(outs):
        bc.check_bands(buf, f"adapt matrix output {k}")
        bc.check_all_written(buf, f"adapt matrix output {k}")
    for k, (buf, snap) in enumerate(ins):
        bc.check_untouched(buf, snap, f"adapt matrix input {k}")
    for got, want, name in ((gather(es), plain[0], "e"), (gather(ys), plain[1], "y"), (w, plain[2], "taps")):
        assert np.array_equal(xc.bits(got), xc.bits(want)), f"offsets {off}: {name} differs from the aligned buffers'"


def test_overlapping_device_ranges_and_foreign_handles_are_refused(dev):
    L = capi.lib()
    block, ports = 64, 2                                    # inputs = outputs: all four buffers have one size
    numel = ports * block
    f = filters.AdaptMatrixMC(ports, ports, block, 100)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    free = [torch.zeros(numel, dtype=F32, device=dev) for _ in range(3)]
    # (which of x, d, e, y take the overlapping pair)
    layouts = {"e over x": lambda a, b: (a, free[0], b, free[1]), "e over d": lambda a, b: (free[0], a, b, free[1]),
               "y over x": lambda a, b: (a, free[0], free[1], b), "y over d": lambda a, b: (free[0], a, free[1], b),
               "y over e": lambda a, b: (free[0], free[1], a, b)}
    for name, lay in layouts.items():
        for k, (a, b) in enumerate(bc.overlap_cases(numel, device=dev)):
            bufs = lay(a, b)
            before = [bc.bits(t).copy() for t in bufs]
            rc = L.llz_adapt_matrix_mc(f.handle, *[ptr(t) for t in bufs], block)
            msg = capi.last_error()
            assert rc == -1 and "llz_adapt_matrix_mc" in msg, (name, k, rc, msg)
            if k > 0:
                assert "may not overlap" in msg and "(device memory)" in msg, (name, k, msg)
            torch.cuda.synchronize()
            for t, was in zip(bufs, before):
                assert np.array_equal(bc.bits(t), was), f"{name}: case {k} changed a buffer it refused"
    # the handle still works; the other families' entry points refuse it, and its entry points refuse theirs
    out4, out6 = (C.c_int * 4)(), (C.c_int * 6)()
    assert L.llz_fir_stream_mc_plan(f.handle, out4) < 0 and L.llz_fir_matrix_mc_plan(f.handle, out6) < 0
    assert L.llz_adapt_mc_plan(f.handle, out4) < 0 and L.llz_fir_filter_mc_algo(f.handle) < 0
    others = [filters.FirStreamMC(ports, block, np.ones(3)), filters.AdaptMC(ports, block, 100),
              filters.FirMatrixMC(ports, ports, block, np.ones((ports, ports, 3)))]
    for s in others:
        assert L.llz_adapt_matrix_mc_plan(s.handle, out6) < 0 and "llz_adapt_matrix_mc_plan" in capi.last_error()
        assert L.llz_adapt_matrix_mc(s.handle, ptr(free[0]), ptr(free[1]), ptr(free[2]), None, block) < 0
        assert L.llz_adapt_matrix_mc_reset(s.handle, 0) < 0
        s.close()
    assert L.llz_adapt_matrix_mc(f.handle, ptr(free[0]), ptr(free[1]), ptr(free[2]), None, block) == block
    torch.cuda.synchronize()
    f.close()
