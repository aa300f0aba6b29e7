"""The adaptive filter on the device (include/llz_adapt.h, llz_adapt_mc; kernels k_adapt_filter / k_adapt_update of
fir_adapt.hip) against the float64 model of its definition (tests/adapt_checks.py, where every limit is stated):

  1. frozen path: set_taps(h), every mu = 0: y bit-equal to FirStreamMC with the same rows, e bit-equal to np.float32(d) - y;
  2. parity while adapting: per channel and block rms(e - e_ref) <= 1e-5 rms(d of the channel);
  3. the taps: |w - w_ref|_2 <= 1e-5 |h|_2, the misalignment within twice the model's, the error falling where the model's does;
  4. grouping: k = 3 against k = 1 over two wraps of the ring, bit-equal e, y and taps;
  5. isolation: neighbours scaled by 2^20, zeroed or NaN; a channel frozen among adapting ones, then released;
  6. hand-over and reset: get_taps into a FirStreamMC and back into the frozen handle, reset(1) and reset(0);
  7. pointers and buffers: host against device pointers, guarded buffers at odd offsets, overlapping device ranges refused.

test_adapt_host.py runs cases 1 to 6 with the numpy float32 model in the device's place (bit-equality against FirStreamMC becomes
the 1e-5 gate against the stream convolver's numpy model there).  On the parent of this feature the library
exports no llz_adapt_mc and every test here fails."""
import ctypes as C

import numpy as np
import pytest
import torch

from llzlab_amd import capi, filters
from tests import adapt_checks as ac
from tests import buffer_checks as bc
from tests import stream_checks as sc

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


def stream_run(dev):
    """x through a FirStreamMC with the rows h, a block per call: the frames"""
    def run(x, h, block):
        f = filters.FirStreamMC(x.shape[0], block, np.asarray(h, np.float64), frame_len=block)
        y = np.concatenate(sc.stream_calls(dev, f, np.asarray(x, np.float32)), axis=1)
        f.close()
        return y
    return run


def test_frozen_path_has_the_stream_convolvers_bits(dev, oracle):
    ac.check_frozen(ac.device(dev), stream_run(dev), oracle, exact=True)


def test_frozen_path_on_the_unrolled_ring_walk(dev, oracle):
    """the 256- and 1024-point instances with enough partitions for the walk's unrolled loop, where the power sums ride along"""
    ac.check_frozen(ac.device(dev), stream_run(dev), oracle, exact=True, shapes=[s[:3] for s in ac.EXTRA[1:]])


def test_frozen_path_many_channels(dev, oracle):
    ac.check_frozen(ac.device(dev), stream_run(dev), oracle, exact=True, shapes=[(128, 513, 0)], channels=37)


@pytest.mark.parametrize("block,T,nblocks", ac.SHAPES)
@pytest.mark.parametrize("channels", ac.CHANNELS)
def test_parity_and_taps_while_adapting(dev, oracle, block, T, nblocks, channels):
    """cases 2 and 3; the worst ratios are printed (holds the measured ones)"""
    ac.check_parity(ac.device(dev), oracle, block, T, channels, nblocks)


@pytest.mark.parametrize("block,T,nblocks,channels", ac.EXTRA)
def test_parity_on_the_paths_the_shapes_leave_out(dev, oracle, block, T, nblocks, channels):
    """adapt_checks.EXTRA: four partitions per update workgroup with a short last group, the filter's unrolled ring walk, the
    256- and 1024-point instances; the same limits"""
    ac.check_parity(ac.device(dev), oracle, block, T, channels, nblocks)


def test_grouping_of_partitions_into_workgroups_changes_no_bit(dev, oracle):
    ac.check_partition_grouping(ac.device(dev), oracle)
    # and under the adapt_ppw override at (64, 199), P = 4: groups of 3 + 1 and one group of all 4 against one each
    block, T, _ = ac.RING
    x, d, _ = ac.case(oracle, block, T, 3, 12)
    got = []
    for ppw in (1, 3, 64):
        with capi.tuned(adapt_ppw=ppw):
            r = ac.Device(dev, 3, block, T, 2 * block)
            e, y = r.process(x, d)
            got.append((e, y, r.get_taps()))
            r.close()
    for other in got[1:]:
        for a, b, name in zip(got[0], other, ("e", "y", "taps")):
            assert np.array_equal(ac.bits(a), ac.bits(b)), name


def test_grouping_of_blocks_into_calls_changes_no_bit(dev, oracle):
    ac.check_grouping(ac.device(dev), oracle)


def test_neighbours_cannot_reach_a_channel(dev, oracle):
    ac.check_isolation(ac.device(dev), oracle)


def test_a_frozen_channel_among_adapting_ones(dev, oracle):
    ac.check_freeze_one(ac.device(dev), oracle)


def test_hand_over_to_the_stream_convolver(dev, oracle):
    ac.check_handover(ac.device(dev), stream_run(dev), oracle, exact=True)


def test_reset(dev, oracle):
    ac.check_reset(ac.device(dev), oracle)


# ------------------------------------------------------------------------------------------------ pointers and buffers
CASE = (64, 199, 3, 8)          # block, taps, channels, blocks: two blocks per call


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


@pytest.fixture(scope="module")
def plain(dev, oracle):
    """the case on ordinary device tensors: (e, y, taps)"""
    block, T, ch, nb = CASE
    x, d, _ = ac.case(oracle, block, T, ch, nb)
    f = filters.AdaptMC(ch, block, T, frame_len=2 * block, mu=ac.MU)
    es, ys = run_calls(f, x, d, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev),
                       lambda: torch.full((ch, 2 * block), float("nan"), dtype=F32, device=dev))
    w = f.get_taps()
    f.close()
    return gather(es), gather(ys), w


def test_host_pointers_give_the_device_pointers_bits(dev, oracle, plain):
    block, T, ch, nb = CASE
    x, d, _ = ac.case(oracle, block, T, ch, nb)
    f = filters.AdaptMC(ch, block, T, frame_len=2 * block, mu=ac.MU)
    es, ys = run_calls(f, x, d, np.ascontiguousarray, lambda: np.full((ch, 2 * block), np.nan, np.float32))
    w = f.get_taps()
    f.close()
    for got, want, name in ((gather(es), plain[0], "e"), (gather(ys), plain[1], "y"), (w, plain[2], "taps")):
        assert np.count_nonzero(ac.bits(got) != ac.bits(want)) == 0, name
    # mixed: x on the host, d on the device, no y
    f = filters.AdaptMC(ch, block, T, frame_len=2 * block, mu=ac.MU)
    n = 2 * block
    es = []
    for o in range(0, x.shape[1], n):
        e = torch.full((ch, n), float("nan"), dtype=F32, device=dev)
        f.process(np.ascontiguousarray(x[:, o:o + n]), torch.from_numpy(np.ascontiguousarray(d[:, o:o + n])).to(dev), e)
        es.append(e)
    f.close()
    assert np.array_equal(ac.bits(gather(es)), ac.bits(plain[0]))


@pytest.mark.parametrize("off", OFFSETS, ids=[f"in{a}-out{b}" for a, b in OFFSETS])
def test_guarded_buffers(dev, oracle, plain, off):
    """x and d between NaN bands, e and y between sentinel bands, at odd element offsets: the plain tensors' bits, every output
    element written, the bands and the inputs unchanged"""
    block, T, ch, nb = CASE
    x, d, _ = ac.case(oracle, block, T, ch, nb)
    ins, outs = [], []

    def make_in(a):
        buf = bc.carve_input(dev, a, off[0])
        ins.append((buf, bc.snapshot(buf)))
        return buf.shaped(*a.shape)

    def make_out():
        buf = bc.carve(dev, F32, ch * 2 * block, off[1])
        outs.append(buf)
        return buf.shaped(ch, 2 * block)
    f = filters.AdaptMC(ch, block, T, frame_len=2 * block, mu=ac.MU)
    es, ys = run_calls(f, x, d, make_in, make_out)
    torch.cuda.synchronize()
    w = f.get_taps()
    f.close()
    for k, buf in enumerate(outs):
        bc.check_bands(buf, f"adapt output {k}")
        bc.check_all_written(buf, f"adapt output {k}")
    for k, (buf, snap) in enumerate(ins):
        bc.check_untouched(buf, snap, f"adapt input {k}")
    for got, want, name in ((gather(es), plain[0], "e"), (gather(ys), plain[1], "y"), (w, plain[2], "taps")):
        assert np.array_equal(ac.bits(got), ac.bits(want)), f"offsets {off}: {name} differs from the aligned buffers'"


def test_overlapping_device_ranges_are_refused(dev):
    L = capi.lib()
    block, ch = 64, 2
    numel = ch * block
    f = filters.AdaptMC(ch, block, 100)
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
            rc = L.llz_adapt_mc(f.handle, *[ptr(t) for t in bufs], block)
            msg = capi.last_error()
            assert rc == -1 and "llz_adapt_mc" in msg, (name, k, rc, msg)
            if k > 0:
                assert "may not overlap" in msg and "(device memory)" in msg, (name, k, msg)
            torch.cuda.synchronize()
            for t, was in zip(bufs, before):
                assert np.array_equal(bc.bits(t), was), f"{name}: case {k} changed a buffer it refused"
    # the handle still works, and the other handles' entry points refuse it
    out = (C.c_int * 4)()
    assert L.llz_fir_stream_mc_plan(f.handle, out) < 0 and L.llz_fir_filter_mc_algo(f.handle) < 0
    s = filters.FirStreamMC(ch, block, np.ones(3))
    assert L.llz_adapt_mc_plan(s.handle, out) < 0 and "llz_adapt_mc_plan" in capi.last_error()
    s.close()
    assert L.llz_adapt_mc(f.handle, ptr(free[0]), ptr(free[1]), ptr(free[2]), None, block) == block
    torch.cuda.synchronize()
    f.close()
