"""The multi-reference per-band adaptive filter on the device (include/llz_adapt_bands_matrix.h, llz_adapt_bands_matrix_mc; kernel
k_bands_matrix_nlms of adapt_bands_matrix.hip) against the float64 model of its definition (tests/adapt_bands_matrix_checks.py,
where every limit is stated):

  1. parity, taps, misalignment and convergence on every shape and on rows of 2049 bins;
  2. one input: the bits of AdaptBandsMC at taps 5, 16, 33 and 64;
  3. grouping: calls of 1, 3, taps - 1, taps, taps + 1 and all frames at once, with empty calls in between, bit-equal -- the
     history crosses its two buffers at every call;
  4. isolation: output o against a one-output handle fed its d row while the other outputs' d is scaled by 2^20, zeroed or NaN;
     a frozen output among adapting ones; a NaN in one bin of one reference reaches that bin of every output and no other bin;
  5. a silent reference at each position equals (==) the handle without it;
  6. frozen: dense taps within 8 (I K + 1) u sum |w| |x|, a single weight 1 or 1j at every (i, q) returns that input delayed by q;
  7. resets and frames();
  8. pointers and buffers: host, device and mixed pointers, guarded buffers at odd offsets, overlapping device ranges refused,
     plan() at every instance;
  9. end to end: PfbMC analysis of two loudspeaker signals and three microphones, this handle on the bands, PfbMC synthesis of e.

Every parity case prints its worst ratios.  On the parent of this feature the library exports no llz_adapt_bands_matrix_mc and
every test here fails."""
import ctypes as C

import numpy as np
import pytest
import torch

from llzlab_amd import capi, filters
from tests import adapt_bands_checks as bc
from tests import adapt_bands_matrix_checks as mc
from tests import buffer_checks as gb

pytestmark = pytest.mark.gpu
F32 = torch.float32
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 3)]                  # elements past a 256-byte boundary: (inputs, outputs)
SMALL = mc.SHAPES[1]                                        # 3 inputs, 2 outputs, 5 taps, 33 bins: both outputs in a wave, a masked ceiling
GROUPED = [mc.SHAPES[0], mc.SHAPES[1], mc.SHAPES[5]]        # (2, 2, 4), (3, 2, 5), (8, 2, 8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def same(a, b):
    return a.shape == b.shape and np.array_equal(mc.cbits(a), mc.cbits(b))


# ------------------------------------------------------------------------------------------------ 1: parity
@pytest.mark.parametrize("inputs,outputs,taps,bins,frames", mc.SHAPES)
def test_parity_and_taps_while_adapting(dev, oracle, inputs, outputs, taps, bins, frames):
    """the worst ratios are printed (holds the measured ones); calls of 37 frames"""
    mc.check_parity(mc.device(dev, calls=37), oracle, inputs, outputs, taps, bins, frames)


def test_parity_on_rows_longer_than_a_workgroup(dev, oracle):
    mc.check_parity(mc.device(dev), oracle, *mc.LONG)


# ------------------------------------------------------------------------------------------------ 2: one input
@pytest.mark.parametrize("taps", [5, 16, 33, 64])
def test_one_input_gives_the_single_reference_filters_bits(dev, oracle, taps):
    channels, bins, frames = 3, 33, 2 * taps + 21
    x = bc.gaussian(oracle, channels, frames, bins, seed=5 + taps)
    h = bc.responses(channels, taps, bins, seed=3 * taps)
    d = bc.convolve(x, h).astype(np.complex64)
    single = bc.Device(dev, channels, bins, taps, calls=[taps + 1, 9])
    e1, y1 = single.process(x, d)
    w1 = single.get_taps()
    single.close()
    assert np.all(np.isfinite(e1)) and np.any(w1 != 0)
    for c in range(channels):                               # one reference into one output, and into three that share it
        m = mc.Device(dev, 1, 1, bins, taps, calls=[taps + 1, 9])
        e, y = m.process(x[c:c + 1], d[c:c + 1])
        assert same(e[0], e1[c]) and same(y[0], y1[c]) and same(m.get_taps()[0, 0], w1[c]), (taps, c)
        m.close()
    m = mc.Device(dev, 1, channels, bins, taps, calls=7)
    e, y = m.process(x[:1], d)
    w = m.get_taps()
    m.close()
    s = bc.Device(dev, channels, bins, taps)
    es, ys = s.process(np.repeat(x[:1], channels, axis=0), d)
    assert same(e, es) and same(y, ys) and same(w[:, 0], s.get_taps()), taps
    s.close()


# ------------------------------------------------------------------------------------------------ 3: grouping
def on_device(dev):
    return (lambda a: torch.from_numpy(np.array(a, order="C")).to(dev),           # (a copy: the shared cases are read-only)
            lambda *shape: torch.full(shape, float("nan"), dtype=F32, device=dev))


def run_calls(f, x, d, sizes, up, new, with_y=True, empty_between=False):
    """x complex [inputs, frames, bins], d complex [outputs, frames, bins] through handle f in calls of `sizes` frames; up(a) makes
    an input buffer of a float32 array, new(*shape) an output buffer.  Returns (e, y) complex64 (y zeros when it is not asked for)."""
    es, ys, o = [], [], 0
    shape = lambda n: (d.shape[0], n, d.shape[2])               # noqa: E731
    host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else t  # noqa: E731
    for n in sizes:
        if empty_between:
            empty = lambda rows: tuple(up(np.zeros((rows, 0, d.shape[2]), np.float32)) for _ in range(2))  # noqa: E731
            f.process(empty(x.shape[0]), empty(d.shape[0]), empty(d.shape[0]), empty(d.shape[0]))
        xs, ds = (tuple(up(a) for a in mc.split(z[:, o:o + n])) for z in (x, d))
        e, y = tuple(new(*shape(n)) for _ in range(2)), (tuple(new(*shape(n)) for _ in range(2)) if with_y else None)
        f.process(xs, ds, e, y)
        es.append(host(e[0]) + 1j * host(e[1]))
        ys.append(host(y[0]) + 1j * host(y[1]) if with_y else host(e[0]) * 0)
        o += n
    assert o == x.shape[1]
    return np.concatenate(es, axis=1).astype(np.complex64), np.concatenate(ys, axis=1).astype(np.complex64)


def chunks(frames, n):
    return [min(n, frames - o) for o in range(0, frames, n)]


@pytest.mark.parametrize("inputs,outputs,taps,bins,total", GROUPED)
def test_grouping_of_frames_into_calls_changes_no_bit(dev, oracle, inputs, outputs, taps, bins, total):
    frames = 3 * taps + 11
    x, d, _ = mc.case(oracle, inputs, outputs, taps, bins, total)
    x, d = x[:, :frames], d[:, :frames]
    got = []
    for k, n in enumerate((frames, 1, 3, taps - 1, taps, taps + 1)):
        f = filters.AdaptBandsMatrixMC(inputs, outputs, bins, taps, mu=mc.MU, delta=mc.DELTA)
        e, y = run_calls(f, x, d, chunks(frames, n), *on_device(dev), empty_between=k % 2 == 1)
        got.append((e, y, f.get_taps(), f.frames()))
        f.close()
    assert np.all(np.isfinite(got[0][0])) and np.any(got[0][2] != 0)
    for other in got[1:]:
        for a, b, name in zip(got[0][:3], other[:3], ("e", "y", "taps")):
            assert same(a, b), f"grouping: {name} differs"
        assert other[3] == frames


# ------------------------------------------------------------------------------------------------ 4: isolation
def test_an_output_is_its_own_handle(dev, oracle):
    """output o of a three-output handle against a one-output handle fed its d row, bit for bit, while the other outputs' d is
    what it was, scaled by 2^20, zeroed or NaN; then with output 1 frozen among adapting ones"""
    inputs, _, taps, bins, frames = SMALL
    outputs, frames = 3, 120
    x, d, _ = mc.case(oracle, inputs, outputs, taps, bins, frames)
    alone = []
    for o in range(outputs):
        r = mc.Device(dev, inputs, 1, bins, taps, calls=50)
        e, y = r.process(x, d[o:o + 1])
        alone.append((e[0], y[0], r.get_taps()[0]))
        r.close()
    assert all(np.all(np.isfinite(a[0])) and np.any(a[2] != 0) for a in alone)
    others = (("as they were", lambda a: a), ("scaled by 2^20", lambda a: a * np.float32(2.0 ** 20)), ("zeroed", np.zeros_like),
              ("NaN", lambda a: np.full_like(a, np.nan + 1j * np.nan)))
    for mine in range(outputs):
        for name, f in others:
            ds = f(np.array(d))
            ds[mine] = d[mine]
            r = mc.Device(dev, inputs, outputs, bins, taps, calls=[7, 64])
            with np.errstate(all="ignore"):
                e, y = r.process(x, ds)
                w = r.get_taps()
            r.close()
            for a, b, what in zip((e[mine], y[mine], w[mine]), alone[mine], ("e", "y", "taps")):
                assert same(a, b), f"output {mine}, the others {name}: its {what} changed"
    r = mc.Device(dev, inputs, outputs, bins, taps, calls=[7, 64])
    r.set_step(1, 0.0)
    e, y = r.process(x, d)
    w = r.get_taps()
    r.close()
    assert not np.any(w[1]) and same(e[1], d[1]) and not np.any(y[1]), "a frozen output with zero weights moved"
    for o in (0, 2):
        assert same(e[o], alone[o][0]) and same(y[o], alone[o][1]) and same(w[o], alone[o][2]), f"output {o} next to a frozen one"


def test_a_frozen_output_keeps_its_taps(dev, oracle):
    inputs, outputs, taps, bins, frames = SMALL
    x, d, h = mc.case(oracle, inputs, outputs, taps, bins, frames)
    r = mc.Device(dev, inputs, outputs, bins, taps, calls=40)
    r.process(x[:, :80], d[:, :80])
    w0 = r.get_taps()
    r.set_step(1, 0.0)
    r.process(x[:, 80:160], d[:, 80:160])
    w1 = r.get_taps()
    r.set_step(1, mc.MU)
    r.process(x[:, 160:], d[:, 160:])
    w2 = r.get_taps()
    r.close()
    assert same(w0[1], w1[1]), "a frozen output's taps moved"
    assert not same(w0[0], w1[0]) and not same(w1[1], w2[1])


def test_a_nan_in_a_reference_reaches_its_bin_of_every_output_and_no_other(dev, oracle):
    inputs, outputs, taps, bins, frames = SMALL
    frames, at, k, i = 90, 30, 7, 1
    x, d, _ = mc.case(oracle, inputs, outputs, taps, bins, SMALL[4])
    x, d = x[:, :frames], d[:, :frames]
    runs = []
    for poisoned in (False, True):
        xs = np.array(x)
        if poisoned:
            xs[i, at, k] = np.nan
        r = mc.Device(dev, inputs, outputs, bins, taps, calls=[30, 1, 2])          # the NaN frame is the second call's only one
        with np.errstate(all="ignore"):
            e, y = r.process(xs, d)
            runs.append((e, y, r.get_taps()))
        r.close()
    (e0, y0, w0), (e1, y1, w1) = runs
    assert np.all(np.isfinite(e0)) and np.all(np.isfinite(w0))
    rest = np.arange(bins) != k
    assert same(e0[:, :, rest], e1[:, :, rest]) and same(y0[:, :, rest], y1[:, :, rest]) and same(w0[..., rest], w1[..., rest]), \
        "a NaN in one bin changed another bin"
    assert same(e0[:, :at, k], e1[:, :at, k]), "the bin changed before the NaN arrived"
    assert np.all(np.isnan(e1[:, at:, k].real)) and np.all(np.isnan(e1[:, at:, k].imag)) and np.all(np.isnan(y1[:, at:, k].real)), \
        "the joint power did not carry the NaN to every output"
    assert np.all(np.isnan(w1[..., k].real)) and np.all(np.isnan(w1[..., k].imag)), "a path's weights escaped the joint power's NaN"


# ------------------------------------------------------------------------------------------------ 5: a silent reference
@pytest.mark.parametrize("silent", [0, 1, 2])
def test_a_silent_reference_equals_the_handle_without_it(dev, oracle, silent):
    inputs, outputs, taps, bins, frames = SMALL
    frames = 120
    x, d, _ = mc.case(oracle, inputs - 1, outputs, taps, bins, SMALL[4])
    x, d = x[:, :frames], d[:, :frames]
    two = mc.Device(dev, inputs - 1, outputs, bins, taps, calls=50)
    e2, y2 = two.process(x, d)
    w2 = two.get_taps()
    two.close()
    keep = [i for i in range(inputs) if i != silent]
    xs = np.zeros((inputs, frames, bins), np.complex64)
    xs[keep] = x
    three = mc.Device(dev, inputs, outputs, bins, taps, calls=50)
    e3, y3 = three.process(xs, d)
    w3 = three.get_taps()
    three.close()
    assert np.any(w2 != 0) and np.all(np.isfinite(e2))
    assert np.array_equal(e3, e2) and np.array_equal(y3, y2) and np.array_equal(w3[:, keep], w2), f"silent reference {silent}"
    assert not np.any(w3[:, silent])


# ------------------------------------------------------------------------------------------------ 6: frozen
def test_exact_delays_of_every_input_and_age(dev, oracle):
    """stream s = o bins + k holds a single weight at entry n = s mod (I K), input n mod I and age n div I: 1 on the first I K
    streams, 1j on the next, and so on in turn; the history crosses every call edge and every age of the walk"""
    inputs, outputs, taps, bins, frames = SMALL
    frames, J = 120, inputs * taps
    assert outputs * bins >= 2 * J
    x = mc.gaussian(oracle, inputs, frames, bins, seed=19)
    s = np.arange(outputs * bins).reshape(outputs, bins)
    entry, turned = s % J, (s // J) % 2 == 1
    w = np.zeros((outputs, inputs, taps, bins), np.complex64)
    for o in range(outputs):
        w[o, entry[o] % inputs, entry[o] // inputs, np.arange(bins)] = np.where(turned[o], 1j, 1.0)
    r = mc.Device(dev, inputs, outputs, bins, taps, mu=0.0, calls=[1, 2, 7, 50])
    r.set_taps(0, w)
    e, y = r.process(x, np.zeros((outputs, frames, bins), np.complex64))
    assert same(r.get_taps(), w) and r.frames() == frames
    r.close()
    for o in range(outputs):
        for k in range(bins):
            i, q = entry[o, k] % inputs, entry[o, k] // inputs
            want = np.concatenate([np.zeros(q, np.complex64), x[i, :frames - q, k]])
            want = (-want.imag + 1j * want.real) if turned[o, k] else want
            assert np.all(y[o, :, k].real == want.real) and np.all(y[o, :, k].imag == want.imag), (o, k, i, q)
    assert np.all(e.real == -y.real) and np.all(e.imag == -y.imag)


@pytest.mark.parametrize("inputs,outputs,taps,bins,total", [mc.SHAPES[1], mc.SHAPES[4], mc.SHAPES[5]])
def test_frozen_dense_taps(dev, oracle, inputs, outputs, taps, bins, total):
    """the band-domain mixer: set_taps of a sub-matrix at a time, frozen"""
    frames = 120
    x, d, h = mc.case(oracle, inputs, outputs, taps, bins, total)
    x, d = x[:, :frames], d[:, :frames]
    r = mc.Device(dev, inputs, outputs, bins, taps, mu=0.0, calls=[7, 50])
    r.set_taps(0, h[:, :1])
    r.set_taps(0, h[:1, 1:], in_first=1)
    if outputs > 1:
        r.set_taps(1, h[1:, 1:], in_first=1)
    e, y = r.process(x, d)
    assert same(r.get_taps(), h.astype(np.complex64)), "a frozen handle's taps moved, or a sub-matrix landed elsewhere"
    assert same(r.f.get_taps(outputs - 1, 1, inputs - 1, 1), h[-1:, -1:].astype(np.complex64))
    r.close()
    ref = mc.convolve(x, h)
    mag = np.zeros(d.shape)
    for i in range(inputs):
        for q in range(taps):
            mag[:, q:] += np.abs(h[:, i, q])[:, None, :] * np.abs(x[i, :frames - q].astype(np.complex128))[None]
    lim = 8 * (inputs * taps + 1) * mc.U * mag
    worst = max(mc.ratio(np.abs(y.real - ref.real), lim), mc.ratio(np.abs(y.imag - ref.imag), lim))
    print(f"frozen I={inputs} K={taps}: worst |y - y_ref| at {worst:.3g} of 8 (I K + 1) u sum |w| |x|")
    assert worst <= 1.0
    assert same(e, d - y), "e is not the float32 difference d - y"


# ------------------------------------------------------------------------------------------------ 7: resets
def test_resets_and_frames(dev, oracle):
    inputs, outputs, taps, bins, frames = SMALL
    x, d, _ = mc.case(oracle, inputs, outputs, taps, bins, frames)
    r = mc.Device(dev, inputs, outputs, bins, taps, calls=[50, 1, 149])          # an odd number of calls: the reset meets the other buffer
    assert r.frames() == 0
    e0, y0 = r.process(x, d)
    w0 = r.get_taps()
    assert r.frames() == frames and np.any(w0 != 0)
    r.reset(False)
    assert r.frames() == 0 and same(r.get_taps(), w0), "reset(0) changed the taps"
    r.set_step(0, np.zeros(outputs, np.float32))                # frozen: behind a reset the first frame's y is sum_i w_{i,0} x_i[0] alone
    _, y = r.process(x[:, :1], d[:, :1])
    assert r.frames() == 1 and same(r.get_taps(), w0)
    want = np.sum(w0[:, :, 0].astype(np.complex128) * x[None, :, 0], axis=1)
    mag = np.sum(np.abs(w0[:, :, 0]) * np.abs(x[None, :, 0]), axis=1)
    assert np.all(np.abs(y[:, 0] - want) <= 4 * (inputs + 1) * mc.U * mag), "reset(0) left history"
    assert np.any(w0[:, :, 1] != 0)
    r.set_step(0, np.full(outputs, mc.MU, np.float32))
    r.reset(True)
    assert r.frames() == 0 and not np.any(r.get_taps()), "reset(1) left taps"
    e1, y1 = r.process(x, d)
    w1 = r.get_taps()
    r.close()
    for a, b, name in ((e0, e1, "e"), (y0, y1, "y"), (w0, w1, "taps")):
        assert same(a, b), f"reset(1): {name} differs from a fresh handle's"


# ------------------------------------------------------------------------------------------------ 8: pointers and buffers
CASE = (3, 2, 5, 33, 60, [1, 29, 30])          # inputs, outputs, taps, bins, frames, calls


def case_data(oracle):
    inputs, outputs, taps, bins, frames, _ = CASE
    x, d, _ = mc.case(oracle, inputs, outputs, taps, bins, SMALL[4])
    return x[:, :frames], d[:, :frames]


@pytest.fixture(scope="module")
def plain(dev, oracle):
    """the case on ordinary device tensors: (e, y, taps)"""
    inputs, outputs, taps, bins, frames, calls = CASE
    f = filters.AdaptBandsMatrixMC(inputs, outputs, bins, taps, mu=mc.MU, delta=mc.DELTA)
    e, y = run_calls(f, *case_data(oracle), calls, *on_device(dev))
    w = f.get_taps()
    f.close()
    return e, y, w


def test_host_pointers_give_the_device_pointers_bits(dev, oracle, plain):
    inputs, outputs, taps, bins, frames, calls = CASE
    x, d = case_data(oracle)
    f = filters.AdaptBandsMatrixMC(inputs, outputs, bins, taps, mu=mc.MU, delta=mc.DELTA)
    e, y = run_calls(f, x, d, calls, np.ascontiguousarray, lambda *shape: np.full(shape, np.nan, np.float32))
    w = f.get_taps()
    f.close()
    for got, want, name in ((e, plain[0], "e"), (y, plain[1], "y"), (w, plain[2], "taps")):
        assert same(got, want), name
    # mixed: x on the host, d and e on the device, no y; then x on the device and the rest on the host
    for x_on_host in (True, False):
        f = filters.AdaptBandsMatrixMC(inputs, outputs, bins, taps, mu=mc.MU, delta=mc.DELTA)
        up, new = on_device(dev)
        host_new = lambda *shape: np.full(shape, np.nan, np.float32)  # noqa: E731
        es, o = [], 0
        for n in calls:
            xs = tuple((np.ascontiguousarray if x_on_host else up)(a) for a in mc.split(x[:, o:o + n]))
            ds = tuple((up if x_on_host else np.ascontiguousarray)(a) for a in mc.split(d[:, o:o + n]))
            eb = tuple((new if x_on_host else host_new)(outputs, n, bins) for _ in range(2))
            f.process(xs, ds, eb)
            re, im = (t.cpu().numpy() if hasattr(t, "cpu") else t for t in eb)
            es.append(re + 1j * im)
            o += n
        assert same(np.concatenate(es, axis=1).astype(np.complex64), plain[0]) and same(f.get_taps(), plain[2]), x_on_host
        f.close()


@pytest.mark.parametrize("with_y", [True, False], ids=["y", "no-y"])
@pytest.mark.parametrize("off", OFFSETS, ids=[f"in{a}-out{b}" for a, b in OFFSETS])
def test_guarded_buffers(dev, oracle, plain, off, with_y):
    """x and d between NaN bands, e and y between sentinel bands, at odd element offsets: the plain tensors' bits, every output
    element written, the bands and the inputs unchanged"""
    inputs, outputs, taps, bins, frames, calls = CASE
    ins, outs = [], []

    def up(a):
        buf = gb.carve_input(dev, a, off[0])
        ins.append((buf, gb.snapshot(buf)))
        return buf.shaped(*a.shape)

    def new(*shape):
        buf = gb.carve(dev, F32, int(np.prod(shape)), off[1])
        outs.append(buf)
        return buf.shaped(*shape)
    f = filters.AdaptBandsMatrixMC(inputs, outputs, bins, taps, mu=mc.MU, delta=mc.DELTA)
    e, y = run_calls(f, *case_data(oracle), calls, up, new, with_y=with_y)
    torch.cuda.synchronize()
    w = f.get_taps()
    f.close()
    assert len(outs) == len(calls) * (4 if with_y else 2) and len(ins) == 4 * len(calls)
    for k, buf in enumerate(outs):
        gb.check_bands(buf, f"bands matrix output {k}")
        gb.check_all_written(buf, f"bands matrix output {k}")
    for k, (buf, snap) in enumerate(ins):
        gb.check_untouched(buf, snap, f"bands matrix input {k}")
    assert same(e, plain[0]) and same(w, plain[2]) and (not with_y or same(y, plain[1])), f"offsets {off}: bits differ"


def test_overlapping_device_ranges_are_refused(dev, oracle):
    L = capi.lib()
    inputs, outputs, bins, taps, frames = 2, 2, 33, 5, 4           # as many inputs as outputs: all eight buffers of one size
    numel = outputs * frames * bins
    f = filters.AdaptBandsMatrixMC(inputs, outputs, bins, taps)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    x = mc.gaussian(oracle, inputs, 3 * frames, bins, seed=3)
    first = [torch.from_numpy(a[:, :frames].reshape(-1).copy()).to(dev) for a in mc.split(x)] * 2 + \
            [torch.zeros(numel, dtype=F32, device=dev) for _ in range(4)]
    assert L.llz_adapt_bands_matrix_mc(f.handle, *[ptr(t) for t in first], frames) == frames       # an issued call in front
    torch.cuda.synchronize()
    free = [torch.zeros(numel, dtype=F32, device=dev) for _ in range(8)]
    w0 = f.get_taps()
    assert np.any(w0 != 0)
    # (slot of the input or earlier output, slot of the output laid over it) among xre xim dre dim ere eim yre yim
    for lo, hi in ((0, 4), (1, 5), (2, 6), (3, 7), (3, 4), (4, 5), (4, 6), (5, 7), (6, 7)):
        for k, (a, b) in enumerate(gb.overlap_cases(numel, device=dev)):
            bufs = list(free)
            bufs[lo], bufs[hi] = a, b
            before = [gb.bits(t).copy() for t in bufs]
            rc = L.llz_adapt_bands_matrix_mc(f.handle, *[ptr(t) for t in bufs], frames)
            msg = capi.last_error()
            assert rc == -1 and "llz_adapt_bands_matrix_mc" in msg and "may not overlap" in msg and "(device memory)" in msg, (lo, hi, k, msg)
            torch.cuda.synchronize()
            for t, was in zip(bufs, before):
                assert np.array_equal(gb.bits(t), was), f"slots {lo}, {hi}: case {k} changed a buffer it refused"
    assert f.frames() == frames and same(f.get_taps(), w0), "a refused call moved the handle"
    big = 2 ** 31 // bins + 1
    assert L.llz_adapt_bands_matrix_mc(f.handle, *[ptr(t) for t in free], big) == -1 and "2^31" in capi.last_error()
    assert L.llz_adapt_bands_matrix_mc(f.handle, *[ptr(t) for t in free[:7]], None, frames) == -1 and "yre and yim" in capi.last_error()
    # the other handles' entry points refuse it and it theirs
    out = (C.c_int * 6)()
    assert L.llz_adapt_bands_mc_plan(f.handle, out) < 0 and L.llz_adapt_matrix_mc_plan(f.handle, out) < 0
    s = filters.AdaptBandsMC(outputs, bins, taps)
    assert L.llz_adapt_bands_matrix_mc_plan(s.handle, out) < 0 and "llz_adapt_bands_matrix_mc_plan" in capi.last_error()
    s.close()
    # the handle goes on where it was: the history of the call in front of the refusals is still the one it reads
    second = [torch.from_numpy(a[:, frames:2 * frames].reshape(-1).copy()).to(dev) for a in mc.split(x)] * 2 + \
             [torch.zeros(numel, dtype=F32, device=dev) for _ in range(4)]
    assert L.llz_adapt_bands_matrix_mc(f.handle, *[ptr(t) for t in second], frames) == frames and f.frames() == 2 * frames
    torch.cuda.synchronize()
    g = filters.AdaptBandsMatrixMC(inputs, outputs, bins, taps)
    both = [torch.cat([a, b]).view(2, outputs, frames, bins).transpose(0, 1).contiguous().view(-1) for a, b in zip(first[:4], second[:4])] + \
           [torch.zeros(2 * numel, dtype=F32, device=dev) for _ in range(4)]
    assert L.llz_adapt_bands_matrix_mc(g.handle, *[ptr(t) for t in both], 2 * frames) == 2 * frames
    torch.cuda.synchronize()
    whole = both[6].view(outputs, 2 * frames, bins)[:, frames:].contiguous().view(-1)
    assert np.array_equal(gb.bits(whole), gb.bits(second[6])) and same(f.get_taps(), g.get_taps()), \
        "refused calls between two issued ones moved the history"
    f.close()
    g.close()


def test_plan_names_the_instance(dev):
    seen = set()
    for inputs in range(1, 9):
        for taps in range(1, 64 // inputs + 1):
            f = filters.AdaptBandsMatrixMC(inputs, 7, 129, taps)
            got, ceiling, threads, groups, launches = f.plan()
            entries = inputs * taps
            assert got == inputs and ceiling == mc.ceiling(inputs, taps) and ceiling in mc.CEILINGS and ceiling >= entries
            assert entries > ceiling // 2 or ceiling == 8
            assert threads % 64 == 0 and groups == -(-7 * 129 // threads) and launches == 1
            seen.add((got, ceiling))
            f.close()
    assert seen == {(i, c) for i in range(1, 9) for c in mc.CEILINGS}, "an instance no shape selects"
    with pytest.raises(capi.LlzError, match="regressor entries"):
        filters.AdaptBandsMatrixMC(5, 2, 33, 13)


# ------------------------------------------------------------------------------------------------ 9: end to end
def test_end_to_end_with_the_filter_bank(dev, oracle):
    """bank analysis of two independent noises and of d = x_0 * h_0 + x_1 * h_1 on three microphones, this handle on the bands,
    bank synthesis of e: the bands of e within the error limit of the float64 model fed with the device's own analysis bands, and
    the synthesised residual's rms over the last quarter below a tenth of the synthesised d's on every output (the float64 chain
    reaches it: test_adapt_bands_matrix_host.py)"""
    x, d, w = mc.e2e_case(oracle)
    I, O, M, P, os, frames, taps = (mc.E2E[k] for k in ("inputs", "outputs", "M", "P", "os", "frames", "taps"))
    bins, hop = M // 2 + 1, M // os
    up, new = on_device(dev)
    bands = []
    for sig in (x, d):
        bank = filters.PfbMC(sig.shape[0], M, hop, P, w, phase=filters.PFB_PHASE_TIME)
        re, im = new(sig.shape[0], frames, bins), new(sig.shape[0], frames, bins)
        bank.analysis(up(sig), re, im)
        bank.close()
        bands.append((re, im))
    X, D = (re.cpu().numpy() + 1j * im.cpu().numpy() for re, im in bands)
    delta = mc.e2e_delta(X)
    f = filters.AdaptBandsMatrixMC(I, O, bins, taps, mu=mc.MU, delta=delta)
    eb = (new(O, frames, bins), new(O, frames, bins))
    f.process(bands[0], bands[1], eb)
    f.close()
    e = (eb[0].cpu().numpy() + 1j * eb[1].cpu().numpy()).astype(np.complex64)
    model = mc.Model(I, O, bins, taps, delta=delta, prec=64)
    e_ref, _ = model.process(X, D)
    d_rms = np.sqrt(np.mean(np.abs(D.astype(np.complex128)) ** 2, axis=1))
    err = mc.run_rms(e.astype(np.complex128) - e_ref)
    error = mc.ratio(err, mc.TOL * np.broadcast_to(d_rms[:, None, :], err.shape))
    times = []
    for re, im in (eb, bands[1]):
        bank = filters.PfbMC(O, M, hop, P, w, phase=filters.PFB_PHASE_TIME)
        out = new(O, frames * hop)
        bank.synthesis(re, im, out)
        bank.close()
        times.append(out.cpu().numpy())
    res = bc.e2e_residual(*times)
    print(f"end to end: bands of e at {error:.3g} of the error limit; residual / d over the last quarter per output: "
          + " ".join(f"{r:.3g}" for r in res) + " (float64 chain: " + " ".join(f"{r:.3g}" for r in mc.e2e_float64(oracle)) + ")")
    assert error <= 1.0
    assert np.all(res < 0.1)
