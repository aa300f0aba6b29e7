"""The per-band Kalman filter on the device (include/llz_kalman_bands.h, llz_kalman_bands_mc; kernel k_bands_kalman of
kalman_bands.hip) against the float64 model of its definition (tests/kalman_bands_checks.py, where every limit is stated):

  1. parity of e, y, w, P and psi, e = d - y and the zero bins on every shape, 3 and 37 channels, and on rows of 2049 bins;
  2. a frozen channel among adapting ones: w, P and psi keep their bits, e and y are AdaptBandsMC's bits for the same taps;
  3. grouping: all frames at once, 1 frame per call, and calls of [7, 1, 0, 30] frames, all five arrays bit-equal;
  4. isolation: neighbouring bins and channels scaled by 2^20, zeroed or NaN;
  5. resets and frames(); set_variance / get_variance;
  6. pointers and buffers: host against device pointers, guarded buffers at odd offsets, overlapping device ranges refused, plan();
  7. double-talk: the misalignment before, at the end of and after a near-end burst;
  8. end to end: PfbMC analysis of x and d, KalmanBandsMC on the bands, PfbMC synthesis of e, with a near-end burst in d.

Every parity case prints its worst ratios.  On the parent of this feature the library exports no llz_kalman_bands_mc and every
test here fails."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from llzlab_amd import capi, filters
from tests import adapt_bands_checks as bc
from tests import buffer_checks as gb
from tests import kalman_bands_checks as kc

pytestmark = pytest.mark.gpu
F32 = torch.float32
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 3)]                  # elements past a 256-byte boundary: (inputs, outputs)
SMALL = kc.SHAPES[2]                                        # 5 taps, 33 bins, 200 frames: several channels in a wave, a masked ceiling


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
    """(w, P, psi) of a filters.KalmanBandsMC or a kalman_bands_checks.Device"""
    return f.get_taps(), f.get_variance(), f.get_noise()


NAMES = ("e", "y", "w", "P", "psi")


# ------------------------------------------------------------------------------------------------ 1: parity
@pytest.mark.parametrize("channels", kc.CHANNELS)
@pytest.mark.parametrize("taps,bins,frames", kc.SHAPES)
def test_parity_of_outputs_and_state(dev, oracle, taps, bins, frames, channels):
    """the worst ratios are printed (holds the measured ones); calls of 37 frames"""
    kc.check_parity(kc.device(dev, calls=37), oracle, taps, bins, frames, channels)


def test_parity_on_rows_longer_than_a_workgroup(dev, oracle):
    taps, bins, frames, channels = kc.LONG
    kc.check_parity(kc.device(dev), oracle, taps, bins, frames, channels)


# ------------------------------------------------------------------------------------------------ 2: frozen
@pytest.mark.parametrize("taps,bins,total", [kc.SHAPES[2], kc.SHAPES[4], kc.SHAPES[5]])
def test_a_frozen_channel_among_adapting_ones(dev, oracle, taps, bins, total):
    """channel 1 frozen by set_adapt behind the first third while its neighbours adapt: its w, P and psi keep their bits, and its
    e and y are those of AdaptBandsMC at mu = 0 with the same taps and the same history; released, it moves again"""
    frames = 90
    x, d, _ = kc.case(oracle, taps, bins, total, 3)
    x, d = x[:, :frames], d[:, :frames]
    third, mine = frames // 3, 1
    r = kc.Device(dev, 3, bins, taps, calls=[7, 23])
    r.process(x[:, :third], d[:, :third])
    s0 = state(r)
    r.set_adapt(mine, 0)
    e, y = r.process(x[:, third:2 * third], d[:, third:2 * third])
    s1 = state(r)
    for a, b, name in zip(s0, s1, NAMES[2:]):
        assert same(a[mine], b[mine]), f"a frozen channel's {name} moved"
        assert not same(a[0], b[0]), f"an adapting channel's {name} stood still"
    n = bc.Device(dev, 3, bins, taps, mu=0.0, calls=[5, 11])
    n.set_taps(0, s0[0])
    n.process(x[:, :third], d[:, :third])                       # the same history behind the first third
    e_n, y_n = n.process(x[:, third:2 * third], d[:, third:2 * third])
    n.close()
    assert same(e[mine], e_n[mine]) and same(y[mine], y_n[mine]), "a frozen channel's e and y are not AdaptBandsMC's bits"
    r.set_adapt(mine, 1)
    r.process(x[:, 2 * third:], d[:, 2 * third:])
    s2 = state(r)
    assert r.frames() == frames and all(not same(a[mine], b[mine]) for a, b in zip(s1, s2))
    r.close()


# ------------------------------------------------------------------------------------------------ 3: grouping
def on_device(dev):
    return (lambda a: torch.from_numpy(np.array(a, order="C")).to(dev),           # (a copy: the shared cases are read-only)
            lambda *shape: torch.full(shape, float("nan"), dtype=F32, device=dev))


def run_calls(f, x, d, sizes, up, new, with_y=True):
    """x, d complex [channels, frames, bins] through handle f in calls of `sizes` frames (0 included: an empty call); up(a) makes
    an input buffer of a float32 array, new(*shape) an output buffer.  Returns (e, y) complex64 (y zeros when not asked for)."""
    es, ys, o = [], [], 0
    shape = lambda n: (x.shape[0], n, x.shape[2])               # noqa: E731
    for n in sizes:
        ins = [up(a) for z in (x[:, o:o + n], d[:, o:o + n]) for a in kc.split(z)]
        outs = [new(*shape(n)) for _ in range(4 if with_y else 2)]
        f.process(*ins, *outs)
        got = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in outs]
        es.append(got[0] + 1j * got[1])
        ys.append(got[2] + 1j * got[3] if with_y else got[0] * 0)
        o += n
    assert o == x.shape[1]
    return np.concatenate(es, axis=1).astype(np.complex64), np.concatenate(ys, axis=1).astype(np.complex64)


def new_filter(ch, bins, taps):
    return filters.KalmanBandsMC(ch, bins, taps, a=kc.A, lam=kc.LAM, p0=kc.P0, delta=kc.DELTA)


@pytest.mark.parametrize("taps,bins,total", [kc.SHAPES[2], kc.SHAPES[3], kc.SHAPES[5]])
def test_grouping_of_frames_into_calls_changes_no_bit(dev, oracle, taps, bins, total):
    frames = 2 * taps + 12
    x, d, _ = kc.case(oracle, taps, bins, total, 3)
    x, d = x[:, :frames], d[:, :frames]
    got = []
    for calls in (None, 1, [7, 1, 0, 30]):                      # (bc.Device.sizes: None = all at once, a list = in turn, repeated)
        f = new_filter(3, bins, taps)
        e, y = run_calls(f, x, d, bc.Device.sizes(types.SimpleNamespace(calls=calls), frames), *on_device(dev))
        got.append((e, y) + state(f) + (f.frames(),))
        f.close()
    assert np.all(np.isfinite(got[0][0])) and np.any(got[0][2] != 0) and np.any(got[0][4] != 0)
    for other in got[1:]:
        for a, b, name in zip(got[0][:5], other[:5], NAMES):
            assert same(a, b), f"grouping: {name} differs"
        assert other[5] == frames


# ------------------------------------------------------------------------------------------------ 4: isolation
def test_neighbours_cannot_reach_a_bin(dev, oracle):
    """with every other (channel, bin) scaled by 2^20, zeroed or NaN, a (channel, bin)'s e, y, w, P and psi keep their bits"""
    taps, bins, frames = SMALL
    x, d, _ = kc.case(oracle, taps, bins, frames, 3)
    mine = (1, 7)

    def run(xs, ds):
        r = kc.Device(dev, 3, bins, taps, calls=64)
        with np.errstate(all="ignore"):
            e, y = r.process(xs, ds)
            w, p, psi = state(r)
        r.close()
        c, k = mine
        return e[c, :, k], y[c, :, k], w[c, :, k], p[c, :, k], psi[c, k:k + 1]
    base = run(x, d)
    assert np.all(np.isfinite(base[0])) and np.any(base[2] != 0)
    for name, f in (("scaled by 2^20", lambda a: a * np.float32(2.0 ** 20)), ("zeroed", np.zeros_like),
                    ("NaN", lambda a: np.full_like(a, np.nan + 1j * np.nan))):
        xs, ds = f(x), f(d)
        xs[mine[0], :, mine[1]], ds[mine[0], :, mine[1]] = x[mine[0], :, mine[1]], d[mine[0], :, mine[1]]
        for a, b, what in zip(run(xs, ds), base, NAMES):
            assert same(a, b), f"isolation: neighbours {name} changed the bin's {what}"


# ------------------------------------------------------------------------------------------------ 5: resets, variances
def test_resets_and_frames(dev, oracle):
    taps, bins, frames = SMALL
    x, d, _ = kc.case(oracle, taps, bins, frames, 3)
    r = kc.Device(dev, 3, bins, taps, calls=[50, 1, 149])
    assert r.frames() == 0 and np.all(r.get_variance() == np.float32(kc.P0)) and not np.any(r.get_noise())
    e0, y0 = r.process(x, d)
    s0 = state(r)
    assert r.frames() == frames and np.any(s0[0] != 0)
    r.reset(False)
    assert r.frames() == 0 and all(same(a, b) for a, b in zip(state(r), s0)), "reset(0) changed w, P or psi"
    r.set_adapt(0, np.zeros(3))                                 # frozen: behind a reset the first frame's y is w_0 x[0] alone
    _, y = r.process(x[:, 10:11], d[:, 10:11])
    assert r.frames() == 1 and all(same(a, b) for a, b in zip(state(r), s0))
    want = s0[0][:, 0].astype(np.complex128) * x[:, 10]
    assert np.all(np.abs(y[:, 0] - want) <= 4 * bc.U * np.abs(s0[0][:, 0]) * np.abs(x[:, 10])), "reset(0) left history"
    assert np.any(s0[0][:, 1] != 0)
    r.reset(True)
    w, p, psi = state(r)
    assert r.frames() == 0 and not np.any(w) and np.all(p == np.float32(kc.P0)) and not np.any(psi), "reset(1) left state"
    _, y = r.process(x[:, :3], d[:, :3])
    assert not np.any(y) and not np.any(r.get_taps()), "reset(1) released the frozen channels"
    r.set_adapt(0, np.ones(3))
    r.reset(True)
    e1, y1 = r.process(x, d)
    for a, b, name in zip((e0, y0) + s0, (e1, y1) + state(r), NAMES):
        assert same(a, b), f"reset(1): {name} differs from a fresh handle's"
    r.close()


def test_set_and_get_variance(dev, oracle):
    """a round trip on a channel range keeps the bits and the other channels; negative, NaN and infinite values are refused and
    change nothing; raised variances re-open a converged filter: its weights move further in the next frames than they would"""
    taps, bins, frames = SMALL
    x, d, _ = kc.case(oracle, taps, bins, frames, 3)
    r = kc.Device(dev, 3, bins, taps)
    r.process(x[:, :150], d[:, :150])
    w0, p0, psi0 = state(r)
    new = np.random.default_rng(3).uniform(0.0, 2.0, (2, taps, bins)).astype(np.float32)
    new[0, 0, :4] = 0
    r.set_variance(1, new)
    p1 = r.get_variance()
    assert same(p1[1:], new) and same(p1[:1], p0[:1]) and same(r.f.get_variance(2, 1), new[1:])
    assert same(r.get_taps(), w0) and same(r.get_noise(), psi0), "set_variance touched w or psi"
    for bad in (-1e-30, float("nan"), float("inf")):
        p = new.copy()
        p[1, taps - 1, bins - 1] = bad
        with pytest.raises(capi.LlzError, match="llz_kalman_bands_mc_set_variance"):
            r.set_variance(1, p)
        assert "variance" in capi.last_error() and same(r.get_variance(), p1), bad
    with pytest.raises(capi.LlzError):
        r.set_variance(0, new[:, :taps - 1])
    r.set_variance(0, p0)
    kept = kc.Device(dev, 3, bins, taps)
    kept.process(x[:, :150], d[:, :150])
    r.set_variance(2, np.full((taps, bins), kc.P0, np.float32))
    r.process(x[:, 150:160], d[:, 150:160])
    kept.process(x[:, 150:160], d[:, 150:160])
    assert same(r.get_taps()[:2], kept.get_taps()[:2]) and same(r.get_variance()[:2], kept.get_variance()[:2])
    assert not same(r.get_taps()[2], kept.get_taps()[2])
    r.close()
    kept.close()


# ------------------------------------------------------------------------------------------------ 6: pointers and buffers
CASE = (5, 33, 3, 60, [1, 29, 30])          # taps, bins, channels, frames, calls


@pytest.fixture(scope="module")
def plain(dev, oracle):
    """the case on ordinary device tensors: (e, y, w, P, psi)"""
    taps, bins, ch, frames, calls = CASE
    x, d, _ = kc.case(oracle, taps, bins, SMALL[2], ch)
    f = new_filter(ch, bins, taps)
    e, y = run_calls(f, x[:, :frames], d[:, :frames], calls, *on_device(dev))
    out = (e, y) + state(f)
    f.close()
    return out


def test_host_pointers_give_the_device_pointers_bits(dev, oracle, plain):
    taps, bins, ch, frames, calls = CASE
    x, d, _ = kc.case(oracle, taps, bins, SMALL[2], ch)
    x, d = x[:, :frames], d[:, :frames]
    f = new_filter(ch, bins, taps)
    e, y = run_calls(f, x, d, calls, np.ascontiguousarray, lambda *shape: np.full(shape, np.nan, np.float32))
    for got, want, name in zip((e, y) + state(f), plain, NAMES):
        assert same(got, want), name
    f.close()
    # mixed: inputs on the host, outputs on the device, no y
    f = new_filter(ch, bins, taps)
    es, o = [], 0
    for n in calls:
        ins = [a for z in (x[:, o:o + n], d[:, o:o + n]) for a in kc.split(z)]
        outs = [torch.full((ch, n, bins), float("nan"), dtype=F32, device=dev) for _ in range(2)]
        f.process(*ins, *outs)
        es.append(outs[0].cpu().numpy() + 1j * outs[1].cpu().numpy())
        o += n
    assert same(np.concatenate(es, axis=1).astype(np.complex64), plain[0])
    assert all(same(a, b) for a, b in zip(state(f), plain[2:]))
    f.close()


@pytest.mark.parametrize("with_y", [True, False], ids=["y", "no-y"])
@pytest.mark.parametrize("off", OFFSETS, ids=[f"in{a}-out{b}" for a, b in OFFSETS])
def test_guarded_buffers(dev, oracle, plain, off, with_y):
    """x and d between NaN bands, e and y between sentinel bands, at odd element offsets: the plain tensors' bits, every output
    element written, the bands and the inputs unchanged"""
    taps, bins, ch, frames, calls = CASE
    x, d, _ = kc.case(oracle, taps, bins, SMALL[2], ch)
    ins, outs = [], []

    def up(a):
        buf = gb.carve_input(dev, a, off[0])
        ins.append((buf, gb.snapshot(buf)))
        return buf.shaped(*a.shape)

    def new(*shape):
        buf = gb.carve(dev, F32, int(np.prod(shape)), off[1])
        outs.append(buf)
        return buf.shaped(*shape)
    f = new_filter(ch, bins, taps)
    e, y = run_calls(f, x[:, :frames], d[:, :frames], calls, up, new, with_y=with_y)
    torch.cuda.synchronize()
    s = state(f)
    f.close()
    assert len(outs) == len(calls) * (4 if with_y else 2) and len(ins) == 4 * len(calls)
    for k, buf in enumerate(outs):
        gb.check_bands(buf, f"kalman output {k}")
        gb.check_all_written(buf, f"kalman output {k}")
    for k, (buf, snap) in enumerate(ins):
        gb.check_untouched(buf, snap, f"kalman input {k}")
    assert same(e, plain[0]) and (not with_y or same(y, plain[1])), f"offsets {off}: bits differ"
    assert all(same(a, b) for a, b in zip(s, plain[2:])), f"offsets {off}: the state's bits differ"


def test_overlapping_device_ranges_are_refused(dev):
    L = capi.lib()
    ch, bins, taps, frames = 2, 33, 5, 4
    numel = ch * frames * bins
    f = new_filter(ch, bins, taps)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    free = [torch.zeros(numel, dtype=F32, device=dev) for _ in range(8)]
    s0 = state(f)
    # (slot of the input or earlier output, slot of the output laid over it) among xre xim dre dim ere eim yre yim
    for lo, hi in ((0, 4), (1, 5), (2, 6), (3, 7), (3, 4), (4, 5), (4, 6), (5, 7), (6, 7)):
        for k, (a, b) in enumerate(gb.overlap_cases(numel, device=dev)):
            bufs = list(free)
            bufs[lo], bufs[hi] = a, b
            before = [gb.bits(t).copy() for t in bufs]
            rc = L.llz_kalman_bands_mc(f.handle, *[ptr(t) for t in bufs], frames)
            msg = capi.last_error()
            assert rc == -1 and "llz_kalman_bands_mc:" in msg and "may not overlap" in msg and "(device memory)" in msg, (lo, hi, k, msg)
            torch.cuda.synchronize()
            for t, was in zip(bufs, before):
                assert np.array_equal(gb.bits(t), was), f"slots {lo}, {hi}: case {k} changed a buffer it refused"
    assert f.frames() == 0 and all(same(a, b) for a, b in zip(state(f), s0)), "a refused call moved the handle"
    big = 2 ** 31 // bins + 1
    assert L.llz_kalman_bands_mc(f.handle, *[ptr(t) for t in free], big) == -1 and "2^31" in capi.last_error()
    assert L.llz_kalman_bands_mc(f.handle, *[ptr(t) for t in free[:7]], None, frames) == -1 and "yre and yim" in capi.last_error()
    assert f.frames() == 0
    # the handle still works, and the other handles' entry points refuse it
    out = (C.c_int * 4)()
    assert L.llz_adapt_bands_mc_plan(f.handle, out) < 0 and L.llz_pfb_mc_bins(f.handle) < 0
    s = filters.AdaptBandsMC(ch, bins, taps)
    assert L.llz_kalman_bands_mc_plan(s.handle, out) < 0 and "llz_kalman_bands_mc_plan" in capi.last_error()
    s.close()
    assert L.llz_kalman_bands_mc(f.handle, *[ptr(t) for t in free], frames) == frames and f.frames() == frames
    torch.cuda.synchronize()
    f.close()


def test_plan_names_the_tap_ceiling(dev):
    for taps in range(1, 33):
        f = filters.KalmanBandsMC(7, 129, taps)
        ceiling, threads, groups, launches = f.plan()
        assert ceiling == kc.ceiling(taps) and ceiling in kc.CEILINGS and ceiling >= taps and (taps > ceiling // 2 or ceiling == 4)
        assert threads % 64 == 0 and groups == -(-7 * 129 // threads) and launches == 1
        f.close()


# ------------------------------------------------------------------------------------------------ 7: double-talk
def test_double_talk(dev):
    """kalman_bands_checks' double-talk case: the misalignment per bin before, at the end of and after the burst within
    max(2 x the float64 model's, the model's + 1e-5 |h|), and at the burst's end below the NLMS float64 model's in every bin"""
    kal, nlms = kc.dt_float64()
    _, _, h = kc.dt_case()
    got = kc.dt_misalignment(kc.Device(dev, 1, kc.DT["bins"], kc.DT["taps"], calls=[100, 33]))
    hn = np.sqrt(np.sum(np.abs(h) ** 2, axis=1))[0]
    worst = kc.ratio(got, np.maximum(2 * kal, kal + kc.TOL * hn[None, :]))
    print(kc.dt_report("device", got))
    print(kc.dt_report("Kalman, float64", kal))
    print(kc.dt_report("NLMS mu = 0.5, float64", nlms))
    print(f"device misalignment at {worst:.3g} of its limit; device / float64 model at most {np.max(got / kal):.6g}")
    assert worst <= 1.0
    assert np.all(got[1] < nlms[1]), "a bin ends the burst further from the echo path than NLMS does"


# ------------------------------------------------------------------------------------------------ 8: end to end
def test_end_to_end_with_the_filter_bank(dev, oracle):
    """bank analysis of white noise x and of d = x * h plus a near-end burst, KalmanBandsMC on the bands, bank synthesis of e: the
    synthesised residual's rms over the last quarter, behind the burst, relative to the synthesised d's, is within a factor of 2
    of the float64 chain's on every channel"""
    x, d, w = kc.e2e_case(oracle)
    c, M, P, os, frames, taps = (kc.E2E[k] for k in ("channels", "M", "P", "os", "frames", "taps"))
    bins, hop = M // 2 + 1, M // os
    up, new = on_device(dev)
    bands = []
    for sig in (x, d):
        bank = filters.PfbMC(c, M, hop, P, w, phase=filters.PFB_PHASE_TIME)
        re, im = new(c, frames, bins), new(c, frames, bins)
        bank.analysis(up(sig), re, im)
        bank.close()
        bands.append((re, im))
    X = bands[0][0].cpu().numpy() + 1j * bands[0][1].cpu().numpy()
    f = filters.KalmanBandsMC(c, bins, taps, **kc.e2e_params(X))
    ere, eim = new(c, frames, bins), new(c, frames, bins)
    f.process(*bands[0], *bands[1], ere, eim)
    f.close()
    times = []
    for re, im in ((ere, eim), bands[1]):
        bank = filters.PfbMC(c, M, hop, P, w, phase=filters.PFB_PHASE_TIME)
        out = new(c, frames * hop)
        bank.synthesis(re, im, out)
        bank.close()
        times.append(out.cpu().numpy())
    res, ref = bc.e2e_residual(*times), kc.e2e_float64(oracle)
    print("end to end: residual / d over the last quarter per channel: " + " ".join(f"{r:.4g}" for r in res)
          + " (float64 chain: " + " ".join(f"{r:.4g}" for r in ref) + ")")
    assert np.all(np.isfinite(res)) and np.all(res <= 2 * ref) and np.all(res >= ref / 2)
