"""The multi-reference per-band Kalman filter on the device (include/llz_kalman_bands_matrix.h, llz_kalman_bands_matrix_mc; kernel
k_bands_matrix_kalman of kalman_bands_matrix.hip) against the float64 model of its definition
(tests/kalman_bands_matrix_checks.py, where every limit is stated):

  1. parity of e, y, w, P and psi, e = d - y and the zero bins on every shape and on rows of 2049 bins;
  2. one input: every bit of e, y, w, P and psi is KalmanBandsMC's;
  3. a frozen output among adapting ones, output 0 included: w, P and psi keep their bits, e and y are AdaptBandsMatrixMC's bits
     at mu = 0, and the shared history moves on for the others;
  4. grouping: all frames at once, 1 frame per call, and calls of [7, 1, 0, 30] frames, with an odd and an even number of
     launches, all five arrays bit-equal;
  5. isolation: other outputs' d, other bins, 2 outputs against 37; a NaN in a reference; a silent reference;
  6. resets and frames(); set_variance / get_variance on sub-matrices;
  7. pointers and buffers: host against device pointers, guarded buffers at odd offsets, overlapping device ranges refused, plan();
  8. double-talk: the misalignment before, at the end of and after a near-end burst;
  9. end to end: PfbMC analyses of two references and of d, the filter on the bands, PfbMC synthesis of e, with a near-end burst.

Every parity case prints its worst ratios.  On the parent of this feature the library exports no llz_kalman_bands_matrix_mc and
every test here fails."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from llzlab_amd import capi, filters
from tests import adapt_bands_checks as bc
from tests import adapt_bands_matrix_checks as mc
from tests import buffer_checks as gb
from tests import kalman_bands_checks as kc
from tests import kalman_bands_matrix_checks as kx

pytestmark = pytest.mark.gpu
F32 = torch.float32
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 3)]                  # elements past a 256-byte boundary: (inputs, outputs)
SMALL = kx.SHAPES[2]                                        # 3 inputs, 2 outputs, 3 taps, 33 bins: both outputs in a wave, a masked ceiling
NAMES = ("e", "y", "w", "P", "psi")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def same(a, b):
    """bit-equal: complex64 or float32 arrays"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def state(f):
    """(w, P, psi) of a filters.KalmanBandsMatrixMC, a filters.KalmanBandsMC or one of the checks' Devices"""
    return f.get_taps(), f.get_variance(), f.get_noise()


def new_filter(inputs, outputs, bins, taps):
    return filters.KalmanBandsMatrixMC(inputs, outputs, bins, taps, a=kx.A, lam=kx.LAM, p0=kx.P0, delta=kx.DELTA)


# ------------------------------------------------------------------------------------------------ 1: parity
@pytest.mark.parametrize("inputs,outputs,taps,bins,frames", kx.SHAPES)
def test_parity_of_outputs_and_state(dev, oracle, inputs, outputs, taps, bins, frames):
    """the worst ratios are printed (holds the measured ones); calls of 37 frames"""
    kx.check_parity(kx.device(dev, calls=37), oracle, inputs, outputs, taps, bins, frames)


def test_parity_on_rows_longer_than_a_workgroup(dev, oracle):
    kx.check_parity(kx.device(dev, calls=37), oracle, *kx.LONG)


# ------------------------------------------------------------------------------------------------ 2: one input
@pytest.mark.parametrize("taps", [1, 5, 32])
def test_one_input_gives_the_single_reference_filters_bits(dev, oracle, taps):
    channels, bins, frames = 3, 33, 2 * taps + 21
    x, d, _ = kx.case(oracle, 1, channels, taps, bins, frames)
    single = kc.Device(dev, channels, bins, taps, calls=[taps + 1, 9])
    e1, y1 = single.process(np.repeat(x, channels, axis=0), d)
    s1 = state(single)
    single.close()
    assert np.all(np.isfinite(e1)) and np.any(s1[0] != 0) and np.any(s1[2] != 0)
    m = kx.Device(dev, 1, channels, bins, taps, calls=7)        # one reference into three outputs that share it
    e, y = m.process(x, d)
    w, p, psi = state(m)
    m.close()
    for a, b, name in zip((e, y, w[:, 0], p[:, 0], psi), (e1, y1) + s1, NAMES):
        assert same(a, b), f"taps {taps}: {name} is not KalmanBandsMC's"
    c = 1                                                       # and into one output
    m = kx.Device(dev, 1, 1, bins, taps, calls=[taps + 1, 9])
    e, y = m.process(x, d[c:c + 1])
    w, p, psi = state(m)
    m.close()
    for a, b, name in zip((e[0], y[0], w[0, 0], p[0, 0], psi[0]), (e1[c], y1[c], s1[0][c], s1[1][c], s1[2][c]), NAMES):
        assert same(a, b), f"taps {taps}, one output: {name} is not KalmanBandsMC's"


# ------------------------------------------------------------------------------------------------ 3: frozen
@pytest.mark.parametrize("frozen", [(1,), (0, 1)], ids=["output1", "outputs0and1"])
@pytest.mark.parametrize("inputs,taps,bins", [(3, 3, 33), (2, 16, 65), (8, 4, 33)])
def test_frozen_outputs_among_adapting_ones(dev, oracle, inputs, taps, bins, frozen):
    """outputs frozen by set_adapt behind the first third while output 2 adapts: their w, P and psi keep their bits, and their e
    and y are those of AdaptBandsMatrixMC at mu = 0 with the same weights and the same history -- which output 0's lanes write
    whether or not output 0 adapts; released, they move again"""
    outputs, frames = 3, 90
    x, d, _ = kx.case(oracle, inputs, outputs, taps, bins, 100)
    x, d = x[:, :frames], d[:, :frames]
    third = frames // 3
    r = kx.Device(dev, inputs, outputs, bins, taps, calls=[7, 23])
    r.process(x[:, :third], d[:, :third])
    s0 = state(r)
    for o in frozen:
        r.set_adapt(o, 0)
    e, y = r.process(x[:, third:2 * third], d[:, third:2 * third])
    s1 = state(r)
    for a, b, name in zip(s0, s1, NAMES[2:]):
        for o in frozen:
            assert same(a[o], b[o]), f"frozen output {o}: {name} moved"
        assert not same(a[2], b[2]), f"an adapting output's {name} stood still"
    n = mc.Device(dev, inputs, outputs, bins, taps, mu=0.0, calls=[5, 11])
    n.set_taps(0, s0[0])
    n.process(x[:, :third], d[:, :third])                       # the same history behind the first third
    e_n, y_n = n.process(x[:, third:2 * third], d[:, third:2 * third])
    n.close()
    for o in frozen:
        assert same(e[o], e_n[o]) and same(y[o], y_n[o]), f"frozen output {o}: e and y are not AdaptBandsMatrixMC's bits"
    # the adapting output next to them is the one of a handle in which nothing was ever frozen
    free = kx.Device(dev, inputs, outputs, bins, taps, calls=30)
    free.process(x[:, :third], d[:, :third])
    e_f, y_f = free.process(x[:, third:2 * third], d[:, third:2 * third])
    assert same(e[2], e_f[2]) and same(y[2], y_f[2]) and all(same(a[2], b[2]) for a, b in zip(s1, state(free)))
    free.close()
    for o in frozen:
        r.set_adapt(o, 1)
    r.process(x[:, 2 * third:], d[:, 2 * third:])
    s2 = state(r)
    assert r.frames() == frames and all(not same(a[o], b[o]) for a, b in zip(s1, s2) for o in frozen)
    r.close()


# ------------------------------------------------------------------------------------------------ 4: grouping
def on_device(dev):
    return (lambda a: torch.from_numpy(np.array(a, order="C")).to(dev),           # (a copy: the shared cases are read-only)
            lambda *shape: torch.full(shape, float("nan"), dtype=F32, device=dev))


def run_calls(f, x, d, sizes, up, new, with_y=True):
    """x complex [inputs, frames, bins], d complex [outputs, frames, bins] through handle f in calls of `sizes` frames (0 included:
    an empty call); up(a) makes an input buffer of a float32 array, new(*shape) an output buffer.  Returns (e, y) complex64 (y
    zeros when it is not asked for)."""
    es, ys, o = [], [], 0
    shape = lambda n: (d.shape[0], n, d.shape[2])               # noqa: E731
    host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else t  # noqa: E731
    for n in sizes:
        xs, ds = (tuple(up(a) for a in kx.split(z[:, o:o + n])) for z in (x, d))
        e, y = tuple(new(*shape(n)) for _ in range(2)), (tuple(new(*shape(n)) for _ in range(2)) if with_y else None)
        f.process(xs, ds, e, y)
        es.append(host(e[0]) + 1j * host(e[1]))
        ys.append(host(y[0]) + 1j * host(y[1]) if with_y else host(e[0]) * 0)
        o += n
    assert o == x.shape[1]
    return np.concatenate(es, axis=1).astype(np.complex64), np.concatenate(ys, axis=1).astype(np.complex64)


@pytest.mark.parametrize("shape,frames", [(kx.SHAPES[1], 38), (kx.SHAPES[2], 45), (kx.SHAPES[4], 38), (kx.SHAPES[5], 45)],
                         ids=["2x4-38", "3x3-45", "8x4-38", "5x6-45"])
def test_grouping_of_frames_into_calls_changes_no_bit(dev, oracle, shape, frames):
    """38 frames are 1, 38 and 3 launches, 45 frames 1, 45 and 4: the two history buffers change places an odd and an even number
    of times, and a last call of 3 frames reads whichever the grouping left"""
    inputs, outputs, taps, bins, total = shape
    x, d, _ = kx.case(oracle, inputs, outputs, taps, bins, total)
    got = []
    for calls in (None, 1, [7, 1, 0, 30]):                      # (bc.Device.sizes: None = all at once, a list = in turn, repeated)
        sizes = bc.Device.sizes(types.SimpleNamespace(calls=calls), frames)
        f = new_filter(inputs, outputs, bins, taps)
        e, y = run_calls(f, x[:, :frames], d[:, :frames], sizes, *on_device(dev))
        e2, y2 = run_calls(f, x[:, frames:frames + 3], d[:, frames:frames + 3], [3], *on_device(dev))
        got.append((np.concatenate([e, e2], axis=1), np.concatenate([y, y2], axis=1)) + state(f) + (f.frames(), sum(n > 0 for n in sizes)))
        f.close()
    assert np.all(np.isfinite(got[0][0])) and np.any(got[0][2] != 0) and np.any(got[0][4] != 0)
    assert {g[6] % 2 for g in got} == {0, 1}, "the launch counts have one parity"
    for other in got[1:]:
        for a, b, name in zip(got[0][:5], other[:5], NAMES):
            assert same(a, b), f"grouping: {name} differs"
        assert other[5] == frames + 3


# ------------------------------------------------------------------------------------------------ 5: isolation
OTHERS = (("scaled by 2^20", lambda a: a * np.float32(2.0 ** 20)), ("zeroed", np.zeros_like),
          ("NaN", lambda a: np.full_like(a, np.nan + 1j * np.nan)))


def test_an_output_is_its_own_handle(dev, oracle):
    """output o of a three-output handle against a one-output handle fed its d row, bit for bit in e, y, w, P and psi, while the
    other outputs' d is what it was, scaled by 2^20, zeroed or NaN"""
    inputs, _, taps, bins, _ = SMALL
    outputs, frames = 3, 120
    x, d, _ = kx.case(oracle, inputs, outputs, taps, bins, frames)
    alone = []
    for o in range(outputs):
        r = kx.Device(dev, inputs, 1, bins, taps, calls=50)
        e, y = r.process(x, d[o:o + 1])
        alone.append((e[0], y[0]) + tuple(a[0] for a in state(r)))
        r.close()
    assert all(np.all(np.isfinite(a[0])) and np.any(a[2] != 0) for a in alone)
    for mine in range(outputs):
        for name, f in (("as they were", lambda a: a),) + OTHERS:
            ds = f(np.array(d))
            ds[mine] = d[mine]
            r = kx.Device(dev, inputs, outputs, bins, taps, calls=[7, 64])
            with np.errstate(all="ignore"):
                e, y = r.process(x, ds)
                s = state(r)
            r.close()
            for a, b, what in zip((e[mine], y[mine]) + tuple(a[mine] for a in s), alone[mine], NAMES):
                assert same(a, b), f"output {mine}, the others {name}: its {what} changed"


def test_two_outputs_among_thirty_seven(dev, oracle):
    """no bit of an output depends on the number of outputs: outputs 0 and 1 of the 2-output case as outputs 35 and 36 of a
    37-output handle (other lanes, other waves, and another output's lanes writing the history)"""
    inputs, _, taps, bins, frames = SMALL
    frames = 80
    x, d, _ = kx.case(oracle, inputs, 2, taps, bins, SMALL[4])
    x, d = x[:, :frames], d[:, :frames]
    few = kx.Device(dev, inputs, 2, bins, taps, calls=33)
    e2, y2 = few.process(x, d)
    s2 = state(few)
    few.close()
    rng = np.random.default_rng(9)
    dd = (rng.standard_normal((37, frames, bins)) + 1j * rng.standard_normal((37, frames, bins))).astype(np.complex64)
    dd[35:] = d
    many = kx.Device(dev, inputs, 37, bins, taps, calls=[1, 40])
    e, y = many.process(x, dd)
    s = state(many)
    many.close()
    for a, b, name in zip((e[35:], y[35:]) + tuple(a[35:] for a in s), (e2, y2) + s2, NAMES):
        assert same(a, b), f"2 against 37 outputs: {name} differs"


def test_neighbouring_bins_cannot_reach_a_bin(dev, oracle):
    """with every other bin of x and d scaled by 2^20, zeroed or NaN, a bin's e, y, w, P and psi keep their bits on every output"""
    inputs, outputs, taps, bins, frames = SMALL
    frames, k = 80, 7
    x, d, _ = kx.case(oracle, inputs, outputs, taps, bins, SMALL[4])
    x, d = x[:, :frames], d[:, :frames]

    def run(xs, ds):
        r = kx.Device(dev, inputs, outputs, bins, taps, calls=64)
        with np.errstate(all="ignore"):
            e, y = r.process(xs, ds)
            w, p, psi = state(r)
        r.close()
        return e[:, :, k], y[:, :, k], w[..., k], p[..., k], psi[:, k]
    base = run(x, d)
    assert np.all(np.isfinite(base[0])) and np.any(base[2] != 0)
    for name, f in OTHERS:
        xs, ds = f(np.array(x)), f(np.array(d))
        xs[:, :, k], ds[:, :, k] = x[:, :, k], d[:, :, k]
        for a, b, what in zip(run(xs, ds), base, NAMES):
            assert same(a, b), f"isolation: the other bins {name} changed the bin's {what}"


def test_a_nan_in_a_reference_reaches_its_bin_of_every_output_and_no_other(dev, oracle):
    inputs, outputs, taps, bins, _ = SMALL
    frames, at, k, i = 90, 30, 7, 1
    x, d, _ = kx.case(oracle, inputs, outputs, taps, bins, SMALL[4])
    x, d = x[:, :frames], d[:, :frames]
    runs = []
    for poisoned in (False, True):
        xs = np.array(x)
        if poisoned:
            xs[i, at, k] = np.nan
        r = kx.Device(dev, inputs, outputs, bins, taps, calls=[30, 1, 2])          # the NaN frame is the second call's only one
        with np.errstate(all="ignore"):
            e, y = r.process(xs, d)
            runs.append((e, y) + state(r))
        r.close()
    clean, bad = runs
    assert np.all(np.isfinite(clean[0])) and np.all(np.isfinite(clean[2]))
    rest = np.arange(bins) != k
    for a, b, name in zip(clean, bad, NAMES):
        assert same(a[..., rest], b[..., rest]), f"a NaN in one bin changed another bin's {name}"
    assert same(clean[0][:, :at, k], bad[0][:, :at, k]), "the bin changed before the NaN arrived"
    e1, y1, w1, p1, psi1 = bad
    assert np.all(np.isnan(e1[:, at:, k].real)) and np.all(np.isnan(e1[:, at:, k].imag)) and np.all(np.isnan(y1[:, at:, k].real)), \
        "the joint sum s did not carry the NaN to every output"
    assert np.all(np.isnan(w1[..., k].real)) and np.all(np.isnan(w1[..., k].imag)) and np.all(np.isnan(p1[..., k])) and \
        np.all(np.isnan(psi1[:, k])), "a path's state escaped the NaN of the joint sum"


@pytest.mark.parametrize("silent", [0, 1, 2])
def test_a_silent_reference_equals_the_handle_without_it(dev, oracle, silent):
    """a reference that is zero throughout, its weights zero: e, y, psi and the other inputs' w and P equal (==) those of a handle
    without that input, and its own weights stay zero"""
    inputs, outputs, taps, bins, _ = SMALL
    frames = 120
    x, d, _ = kx.case(oracle, inputs - 1, outputs, taps, bins, SMALL[4])
    x, d = x[:, :frames], d[:, :frames]
    two = kx.Device(dev, inputs - 1, outputs, bins, taps, calls=50)
    e2, y2 = two.process(x, d)
    w2, p2, psi2 = state(two)
    two.close()
    keep = [i for i in range(inputs) if i != silent]
    xs = np.zeros((inputs, frames, bins), np.complex64)
    xs[keep] = x
    three = kx.Device(dev, inputs, outputs, bins, taps, calls=50)
    e3, y3 = three.process(xs, d)
    w3, p3, psi3 = state(three)
    three.close()
    assert np.any(w2 != 0) and np.all(np.isfinite(e2))
    assert np.array_equal(e3, e2) and np.array_equal(y3, y2) and np.array_equal(psi3, psi2), f"silent reference {silent}"
    assert np.array_equal(w3[:, keep], w2) and np.array_equal(p3[:, keep], p2), f"silent reference {silent}: the others' state"
    assert not np.any(w3[:, silent]) and np.all(p3[:, silent] == kx.idle_variance(frames))


# ------------------------------------------------------------------------------------------------ 6: resets, variances
def test_resets_and_frames(dev, oracle):
    inputs, outputs, taps, bins, frames = SMALL
    x, d, _ = kx.case(oracle, inputs, outputs, taps, bins, frames)
    r = kx.Device(dev, inputs, outputs, bins, taps, calls=[50, 1, 149])          # an odd number of calls: the reset meets the other buffer
    assert r.frames() == 0 and np.all(r.get_variance() == np.float32(kx.P0)) and not np.any(r.get_noise())
    e0, y0 = r.process(x, d)
    s0 = state(r)
    assert r.frames() == frames and np.any(s0[0] != 0)
    r.reset(False)
    assert r.frames() == 0 and all(same(a, b) for a, b in zip(state(r), s0)), "reset(0) changed w, P or psi"
    r.set_adapt(0, np.zeros(outputs))                           # frozen: behind a reset the first frame's y is sum_i w_{i,0} x_i[0] alone
    _, y = r.process(x[:, 10:11], d[:, 10:11])
    assert r.frames() == 1 and all(same(a, b) for a, b in zip(state(r), s0))
    want = np.sum(s0[0][:, :, 0].astype(np.complex128) * x[None, :, 10], axis=1)
    mag = np.sum(np.abs(s0[0][:, :, 0]) * np.abs(x[None, :, 10]), axis=1)
    assert np.all(np.abs(y[:, 0] - want) <= 4 * (inputs + 1) * bc.U * mag), "reset(0) left history"
    assert np.any(s0[0][:, :, 1] != 0)
    r.reset(True)
    w, p, psi = state(r)
    assert r.frames() == 0 and not np.any(w) and np.all(p == np.float32(kx.P0)) and not np.any(psi), "reset(1) left state"
    _, y = r.process(x[:, :3], d[:, :3])
    assert not np.any(y) and not np.any(r.get_taps()), "reset(1) released the frozen outputs"
    r.set_adapt(0, np.ones(outputs))
    r.reset(True)
    e1, y1 = r.process(x, d)
    for a, b, name in zip((e0, y0) + s0, (e1, y1) + state(r), NAMES):
        assert same(a, b), f"reset(1): {name} differs from a fresh handle's"
    r.close()


def test_set_and_get_variance_on_sub_matrices(dev, oracle):
    """a round trip on a sub-matrix keeps the bits and every other path; negative, NaN and infinite values are refused and change
    nothing; raised variances re-open a converged output while the others keep their bits"""
    inputs, _, taps, bins, frames = SMALL
    outputs = 3
    x, d, _ = kx.case(oracle, inputs, outputs, taps, bins, frames)
    r = kx.Device(dev, inputs, outputs, bins, taps)
    r.process(x[:, :150], d[:, :150])
    w0, p0, psi0 = state(r)
    new = np.random.default_rng(3).uniform(0.0, 2.0, (2, 2, taps, bins)).astype(np.float32)
    new[0, 0, 0, :4] = 0
    r.set_variance(1, new, in_first=1)                          # outputs 1 and 2, inputs 1 and 2
    p1 = r.get_variance()
    assert same(p1[1:, 1:], new) and same(p1[:1], p0[:1]) and same(p1[:, :1], p0[:, :1])
    assert same(r.f.get_variance(2, 1, 1, 1), new[1:, :1]) and same(r.f.get_variance(1, 2, 1, 2), new)
    assert same(r.get_taps(), w0) and same(r.get_noise(), psi0), "set_variance touched w or psi"
    for bad in (-1e-30, float("nan"), float("inf")):
        p = new.copy()
        p[1, 1, taps - 1, bins - 1] = bad
        with pytest.raises(capi.LlzError, match="llz_kalman_bands_matrix_mc_set_variance"):
            r.set_variance(1, p, in_first=1)
        assert "variance" in capi.last_error() and same(r.get_variance(), p1), bad
    with pytest.raises(capi.LlzError):
        r.set_variance(0, new[:, :, :taps - 1])
    with pytest.raises(capi.LlzError, match="inputs"):
        r.set_variance(0, new, in_first=2)
    r.set_variance(0, p0)
    assert same(r.get_variance(), p0)
    kept = kx.Device(dev, inputs, outputs, bins, taps)
    kept.process(x[:, :150], d[:, :150])
    r.set_variance(2, np.full((1, inputs, taps, bins), kx.P0, np.float32))
    r.process(x[:, 150:160], d[:, 150:160])
    kept.process(x[:, 150:160], d[:, 150:160])
    for a, b, name in zip(state(r), state(kept), NAMES[2:]):
        assert same(a[:2], b[:2]), f"raising output 2's variances changed another output's {name}"
    # re-opened: the weights take another way, and ten frames on every variance -- a tap's share of the step -- still lies
    # above the one the converged output holds (the float32 model: by a factor of 1.35 at the least)
    assert not same(r.get_taps()[2], kept.get_taps()[2]) and np.all(r.get_variance()[2] > kept.get_variance()[2]), \
        "raised variances did not re-open the output"
    r.close()
    kept.close()


def test_set_and_get_taps_on_sub_matrices(dev, oracle):
    inputs, outputs, taps, bins, _ = SMALL
    h = kx.responses(outputs, inputs, taps, bins, seed=4).astype(np.complex64)
    r = kx.Device(dev, inputs, outputs, bins, taps)
    r.set_taps(0, h[:, :1])
    r.set_taps(0, h[:1, 1:], in_first=1)
    r.set_taps(1, h[1:, 1:], in_first=1)
    assert same(r.get_taps(), h) and same(r.f.get_taps(outputs - 1, 1, inputs - 1, 1), h[-1:, -1:])
    assert np.all(r.get_variance() == np.float32(kx.P0)) and not np.any(r.get_noise())
    r.close()


# ------------------------------------------------------------------------------------------------ 7: pointers and buffers
CASE = (3, 2, 3, 33, 60, [1, 29, 30])          # inputs, outputs, taps, bins, frames, calls


def case_data(oracle):
    inputs, outputs, taps, bins, frames, _ = CASE
    x, d, _ = kx.case(oracle, inputs, outputs, taps, bins, SMALL[4])
    return x[:, :frames], d[:, :frames]


@pytest.fixture(scope="module")
def plain(dev, oracle):
    """the case on ordinary device tensors: (e, y, w, P, psi)"""
    inputs, outputs, taps, bins, frames, calls = CASE
    f = new_filter(inputs, outputs, bins, taps)
    e, y = run_calls(f, *case_data(oracle), calls, *on_device(dev))
    out = (e, y) + state(f)
    f.close()
    return out


def test_host_pointers_give_the_device_pointers_bits(dev, oracle, plain):
    inputs, outputs, taps, bins, frames, calls = CASE
    x, d = case_data(oracle)
    f = new_filter(inputs, outputs, bins, taps)
    e, y = run_calls(f, x, d, calls, np.ascontiguousarray, lambda *shape: np.full(shape, np.nan, np.float32))
    for got, want, name in zip((e, y) + state(f), plain, NAMES):
        assert same(got, want), name
    f.close()
    # mixed: x on the host, d and e on the device, no y; then x on the device and the rest on the host
    for x_on_host in (True, False):
        f = new_filter(inputs, outputs, bins, taps)
        up, new = on_device(dev)
        host_new = lambda *shape: np.full(shape, np.nan, np.float32)  # noqa: E731
        es, o = [], 0
        for n in calls:
            xs = tuple((np.ascontiguousarray if x_on_host else up)(a) for a in kx.split(x[:, o:o + n]))
            ds = tuple((up if x_on_host else np.ascontiguousarray)(a) for a in kx.split(d[:, o:o + n]))
            eb = tuple((new if x_on_host else host_new)(outputs, n, bins) for _ in range(2))
            f.process(xs, ds, eb)
            re, im = (t.cpu().numpy() if hasattr(t, "cpu") else t for t in eb)
            es.append(re + 1j * im)
            o += n
        assert same(np.concatenate(es, axis=1).astype(np.complex64), plain[0]), x_on_host
        assert all(same(a, b) for a, b in zip(state(f), plain[2:])), x_on_host
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
    f = new_filter(inputs, outputs, bins, taps)
    e, y = run_calls(f, *case_data(oracle), calls, up, new, with_y=with_y)
    torch.cuda.synchronize()
    s = state(f)
    f.close()
    assert len(outs) == len(calls) * (4 if with_y else 2) and len(ins) == 4 * len(calls)
    for k, buf in enumerate(outs):
        gb.check_bands(buf, f"kalman matrix output {k}")
        gb.check_all_written(buf, f"kalman matrix output {k}")
    for k, (buf, snap) in enumerate(ins):
        gb.check_untouched(buf, snap, f"kalman matrix input {k}")
    assert same(e, plain[0]) and (not with_y or same(y, plain[1])), f"offsets {off}: bits differ"
    assert all(same(a, b) for a, b in zip(s, plain[2:])), f"offsets {off}: the state's bits differ"


def test_overlapping_device_ranges_are_refused(dev, oracle):
    L = capi.lib()
    inputs, outputs, bins, taps, frames = 2, 2, 33, 5, 4           # as many inputs as outputs: all eight buffers of one size
    numel = outputs * frames * bins
    f = new_filter(inputs, outputs, bins, taps)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    x = kx.gaussian(oracle, inputs, 3 * frames, bins, seed=3)
    first = [torch.from_numpy(a[:, :frames].reshape(-1).copy()).to(dev) for a in kx.split(x)] * 2 + \
            [torch.zeros(numel, dtype=F32, device=dev) for _ in range(4)]
    assert L.llz_kalman_bands_matrix_mc(f.handle, *[ptr(t) for t in first], frames) == frames      # an issued call in front
    torch.cuda.synchronize()
    free = [torch.zeros(numel, dtype=F32, device=dev) for _ in range(8)]
    s0 = state(f)
    assert np.any(s0[0] != 0)
    # (slot of the input or earlier output, slot of the output laid over it) among xre xim dre dim ere eim yre yim
    for lo, hi in ((0, 4), (1, 5), (2, 6), (3, 7), (3, 4), (4, 5), (4, 6), (5, 7), (6, 7)):
        for k, (a, b) in enumerate(gb.overlap_cases(numel, device=dev)):
            bufs = list(free)
            bufs[lo], bufs[hi] = a, b
            before = [gb.bits(t).copy() for t in bufs]
            rc = L.llz_kalman_bands_matrix_mc(f.handle, *[ptr(t) for t in bufs], frames)
            msg = capi.last_error()
            assert rc == -1 and "llz_kalman_bands_matrix_mc:" in msg and "may not overlap" in msg and "(device memory)" in msg, (lo, hi, k, msg)
            torch.cuda.synchronize()
            for t, was in zip(bufs, before):
                assert np.array_equal(gb.bits(t), was), f"slots {lo}, {hi}: case {k} changed a buffer it refused"
    assert f.frames() == frames and all(same(a, b) for a, b in zip(state(f), s0)), "a refused call moved the handle"
    big = 2 ** 31 // bins + 1
    assert L.llz_kalman_bands_matrix_mc(f.handle, *[ptr(t) for t in free], big) == -1 and "2^31" in capi.last_error()
    assert L.llz_kalman_bands_matrix_mc(f.handle, *[ptr(t) for t in free[:7]], None, frames) == -1 and "yre and yim" in capi.last_error()
    # the other families' entry points refuse the handle and it theirs
    out = (C.c_int * 6)()
    assert L.llz_kalman_bands_mc_plan(f.handle, out) < 0 and L.llz_adapt_bands_matrix_mc_plan(f.handle, out) < 0
    for other in (filters.KalmanBandsMC(outputs, bins, taps), filters.AdaptBandsMatrixMC(inputs, outputs, bins, taps)):
        assert L.llz_kalman_bands_matrix_mc_plan(other.handle, out) < 0 and "llz_kalman_bands_matrix_mc_plan" in capi.last_error()
        assert L.llz_kalman_bands_matrix_mc(other.handle, *[ptr(t) for t in free], frames) == -1 and "bad handle" in capi.last_error()
        other.close()
    # the handle goes on where it was: the history of the call in front of the refusals is still the one it reads
    second = [torch.from_numpy(a[:, frames:2 * frames].reshape(-1).copy()).to(dev) for a in kx.split(x)] * 2 + \
             [torch.zeros(numel, dtype=F32, device=dev) for _ in range(4)]
    assert L.llz_kalman_bands_matrix_mc(f.handle, *[ptr(t) for t in second], frames) == frames and f.frames() == 2 * frames
    torch.cuda.synchronize()
    g = new_filter(inputs, outputs, bins, taps)
    both = [torch.cat([a, b]).view(2, outputs, frames, bins).transpose(0, 1).contiguous().view(-1) for a, b in zip(first[:4], second[:4])] + \
           [torch.zeros(2 * numel, dtype=F32, device=dev) for _ in range(4)]
    assert L.llz_kalman_bands_matrix_mc(g.handle, *[ptr(t) for t in both], 2 * frames) == 2 * frames
    torch.cuda.synchronize()
    whole = both[6].view(outputs, 2 * frames, bins)[:, frames:].contiguous().view(-1)
    assert np.array_equal(gb.bits(whole), gb.bits(second[6])) and all(same(a, b) for a, b in zip(state(f), state(g))), \
        "refused calls between two issued ones moved the history"
    f.close()
    g.close()


def test_plan_names_the_instance(dev):
    seen = set()
    for inputs in range(1, 9):
        for taps in range(1, 32 // inputs + 1):
            f = filters.KalmanBandsMatrixMC(inputs, 7, 129, taps)
            got, ceiling, threads, groups, launches = f.plan()
            entries = inputs * taps
            assert got == inputs and ceiling == kx.ceiling(inputs, taps) and ceiling in kx.CEILINGS and ceiling >= entries
            assert entries > ceiling // 2 or ceiling == 8
            assert threads == 64 and groups == -(-7 * 129 // threads) and launches == 1
            seen.add((got, ceiling))
            f.close()
    assert seen == {(i, c) for i in range(1, 9) for c in kx.CEILINGS}, "an instance no shape selects"
    with pytest.raises(capi.LlzError, match="registers"):
        filters.KalmanBandsMatrixMC(5, 2, 33, 7)


# ------------------------------------------------------------------------------------------------ 8: double-talk
def test_double_talk(dev):
    """kalman_bands_matrix_checks' double-talk case: the misalignment per bin before, at the end of and after the burst within
    max(2 x the float64 model's, the model's + 1e-5 |h|), and at the burst's end below the joint NLMS float64 model's in every bin"""
    kal, nlms, _ = kx.dt_float64()
    _, _, h = kx.dt_case()
    got = kx.dt_misalignment(kx.Device(dev, kx.DT["inputs"], 1, kx.DT["bins"], kx.DT["taps"], calls=[100, 33]))
    hn = np.sqrt(np.sum(np.abs(h) ** 2, axis=(1, 2)))[0]
    worst = kx.ratio(got, np.maximum(2 * kal, kal + kx.TOL * hn[None, :]))
    print(kx.dt_report("device", got))
    print(kx.dt_report("joint Kalman, float64", kal))
    print(kx.dt_report("joint NLMS mu = 0.5, float64", nlms))
    print(f"device misalignment at {worst:.3g} of its limit; device / float64 model at most {np.max(got / kal):.6g}")
    assert worst <= 1.0
    assert np.all(got[1] < nlms[1]), "a bin ends the burst further from the echo paths than NLMS does"


# ------------------------------------------------------------------------------------------------ 9: end to end
def test_end_to_end_with_the_filter_bank(dev, oracle):
    """a bank analysis of each of two independent white references and one of d = x_0 * h_0 + x_1 * h_1 on three microphones plus a
    near-end burst, this filter on the bands, bank synthesis of e: the synthesised residual's rms over the last quarter, behind
    the burst, relative to the synthesised d's, is within a factor of 2 of the float64 chain's on every output, in both
    directions"""
    x, d, w = kx.e2e_case(oracle)
    I, O, M, P, os, frames, taps = (kx.E2E[k] for k in ("inputs", "outputs", "M", "P", "os", "frames", "taps"))
    bins, hop = M // 2 + 1, M // os
    up, new = on_device(dev)

    def analysis(sig):
        bank = filters.PfbMC(sig.shape[0], M, hop, P, w, phase=filters.PFB_PHASE_TIME)
        re, im = new(sig.shape[0], frames, bins), new(sig.shape[0], frames, bins)
        bank.analysis(up(sig), re, im)
        bank.close()
        return re, im
    refs = [analysis(x[i:i + 1]) for i in range(I)]             # one bank per loudspeaker signal
    xb = tuple(torch.cat([r[part] for r in refs]).contiguous() for part in range(2))
    db = analysis(d)
    X = xb[0].cpu().numpy() + 1j * xb[1].cpu().numpy()
    f = filters.KalmanBandsMatrixMC(I, O, bins, taps, **kx.e2e_params(X))
    eb = (new(O, frames, bins), new(O, frames, bins))
    f.process(xb, db, eb)
    f.close()
    times = []
    for re, im in (eb, db):
        bank = filters.PfbMC(O, M, hop, P, w, phase=filters.PFB_PHASE_TIME)
        out = new(O, frames * hop)
        bank.synthesis(re, im, out)
        bank.close()
        times.append(out.cpu().numpy())
    res, ref = bc.e2e_residual(*times), kx.e2e_float64(oracle)
    print("end to end: residual / d over the last quarter per output: " + " ".join(f"{r:.4g}" for r in res)
          + " (float64 chain: " + " ".join(f"{r:.4g}" for r in ref) + ")")
    assert np.all(np.isfinite(res)) and np.all(res <= 2 * ref) and np.all(res >= ref / 2)
