"""The per-band adaptive filter on the device (include/llz_adapt_bands.h, llz_adapt_bands_mc; kernel k_bands_nlms of
adapt_bands.hip) against the float64 model of its definition (tests/adapt_bands_checks.py, where every limit is stated):

  1. exact delays: frozen, one weight 1 or 1j at age j, every j of K = 5 and K = 33, over calls of 1, 2, 7 and 50 frames;
  2. frozen, dense taps: per value |y - y_ref| <= 8 (K + 1) u sum_q |h_q| |x[m - q]| against the float64 sum;
  3. parity, taps, misalignment, convergence and the zero bins on every shape, 3 and 37 channels, and on rows of 2049 bins;
  4. grouping: calls of 1, 3, taps - 1, taps, taps + 1 and all frames at once, with empty calls in between, bit-equal;
  5. isolation: neighbouring bins and channels scaled by 2^20, zeroed or NaN; a channel frozen among adapting ones, then released;
  6. resets and frames();
  7. pointers and buffers: host against device pointers, guarded buffers at odd offsets, overlapping device ranges refused, plan();
  8. end to end: PfbMC analysis of x and d, AdaptBandsMC on the bands, PfbMC synthesis of e.

Every parity case prints its worst ratios.  On the parent of this feature the library exports no llz_adapt_bands_mc and every
test here fails."""
import ctypes as C

import numpy as np
import pytest
import torch

from llzlab_amd import capi, filters
from tests import adapt_bands_checks as bc
from tests import buffer_checks as gb

pytestmark = pytest.mark.gpu
F32 = torch.float32
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 3)]                  # elements past a 256-byte boundary: (inputs, outputs)
SMALL = bc.SHAPES[2]                                        # 5 taps, 33 bins, 200 frames: several channels in a wave, a masked ceiling


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def same(a, b):
    return a.shape == b.shape and np.array_equal(bc.cbits(a), bc.cbits(b))


# ------------------------------------------------------------------------------------------------ 1, 2: frozen
@pytest.mark.parametrize("taps", [5, 33])
def test_exact_delays(dev, oracle, taps):
    """stream s = c bins + k holds a single weight at age j = s mod K: 1 on the first K streams, 1j on the next K, and so on in
    turn; the history crosses every call edge and every age of the walk"""
    channels, bins, frames = 3, 33, 120
    assert channels * bins >= 2 * taps
    x = bc.gaussian(oracle, channels, frames, bins, seed=9 + taps)
    s = np.arange(channels * bins).reshape(channels, bins)
    age, turned = s % taps, (s // taps) % 2 == 1
    w = np.zeros((channels, taps, bins), np.complex64)
    for c in range(channels):
        w[c, age[c], np.arange(bins)] = np.where(turned[c], 1j, 1.0)
    r = bc.Device(dev, channels, bins, taps, mu=0.0, calls=[1, 2, 7, 50])
    r.set_taps(0, w)
    e, y = r.process(x, np.zeros_like(x))
    assert same(r.get_taps(), w) and r.frames() == frames
    r.close()
    for c in range(channels):
        for k in range(bins):
            j = age[c, k]
            want = np.concatenate([np.zeros(j, np.complex64), x[c, :frames - j, k]])
            want = (-want.imag + 1j * want.real) if turned[c, k] else want
            assert np.all(y[c, :, k].real == want.real) and np.all(y[c, :, k].imag == want.imag), (c, k, j)
    assert np.all(e.real == -y.real) and np.all(e.imag == -y.imag)


@pytest.mark.parametrize("taps,bins,total", [bc.SHAPES[2], bc.SHAPES[4], bc.SHAPES[5]])
def test_frozen_dense_taps(dev, oracle, taps, bins, total):
    frames = 120
    x, d, h = bc.case(oracle, taps, bins, total, 3)
    x, d = x[:, :frames], d[:, :frames]
    r = bc.Device(dev, 3, bins, taps, mu=0.0, calls=[7, 50])
    r.set_taps(0, h)
    e, y = r.process(x, d)
    assert same(r.get_taps(), h.astype(np.complex64)), "a frozen handle's taps moved"
    r.close()
    ref = bc.convolve(x, h)
    mag = np.zeros(x.shape)
    for q in range(taps):
        mag[:, q:] += np.abs(h[:, q])[:, None, :] * np.abs(x[:, :frames - q].astype(np.complex128))
    lim = 8 * (taps + 1) * bc.U * mag
    worst = max(bc.ratio(np.abs(y.real - ref.real), lim), bc.ratio(np.abs(y.imag - ref.imag), lim))
    print(f"frozen K={taps}: worst |y - y_ref| at {worst:.3g} of 8 (K + 1) u sum |h| |x|")
    assert worst <= 1.0
    assert same(e, d - y), "e is not the float32 difference d - y"


# ------------------------------------------------------------------------------------------------ 3: parity
@pytest.mark.parametrize("channels", bc.CHANNELS)
@pytest.mark.parametrize("taps,bins,frames", bc.SHAPES)
def test_parity_and_taps_while_adapting(dev, oracle, taps, bins, frames, channels):
    """the worst ratios are printed (holds the measured ones); calls of 37 frames"""
    bc.check_parity(bc.device(dev, calls=37), oracle, taps, bins, frames, channels)


def test_parity_on_rows_longer_than_a_workgroup(dev, oracle):
    taps, bins, frames, channels = bc.LONG
    bc.check_parity(bc.device(dev), oracle, taps, bins, frames, channels)


# ------------------------------------------------------------------------------------------------ 4: grouping
def on_device(dev):
    return (lambda a: torch.from_numpy(np.array(a, order="C")).to(dev),           # (a copy: the shared cases are read-only)
            lambda *shape: torch.full(shape, float("nan"), dtype=F32, device=dev))


def run_calls(f, x, d, sizes, up, new, with_y=True, empty_between=False):
    """x, d complex [channels, frames, bins] through handle f in calls of `sizes` frames; up(a) makes an input buffer of a float32
    array, new(*shape) an output buffer.  Returns (e, y) complex64 (y zeros when it is not asked for)."""
    es, ys, o = [], [], 0
    shape = lambda n: (x.shape[0], n, x.shape[2])               # noqa: E731
    for n in sizes:
        if empty_between:
            f.process(*[up(np.zeros(shape(0), np.float32)) for _ in range(8)])
        ins = [up(a) for z in (x[:, o:o + n], d[:, o:o + n]) for a in bc.split(z)]
        outs = [new(*shape(n)) for _ in range(4 if with_y else 2)]
        f.process(*ins, *outs)
        got = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in outs]
        es.append(got[0] + 1j * got[1])
        ys.append(got[2] + 1j * got[3] if with_y else got[0] * 0)
        o += n
    assert o == x.shape[1]
    return np.concatenate(es, axis=1).astype(np.complex64), np.concatenate(ys, axis=1).astype(np.complex64)


def chunks(frames, n):
    return [min(n, frames - o) for o in range(0, frames, n)]


@pytest.mark.parametrize("taps,bins,total", [bc.SHAPES[2], bc.SHAPES[3], bc.SHAPES[4]])
def test_grouping_of_frames_into_calls_changes_no_bit(dev, oracle, taps, bins, total):
    frames = 3 * taps + 11
    x, d, _ = bc.case(oracle, taps, bins, total, 3)
    x, d = x[:, :frames], d[:, :frames]
    got = []
    for k, n in enumerate((frames, 1, 3, taps - 1, taps, taps + 1)):
        f = filters.AdaptBandsMC(3, bins, taps, mu=bc.MU, delta=bc.DELTA)
        e, y = run_calls(f, x, d, chunks(frames, n), *on_device(dev), empty_between=k % 2 == 1)
        got.append((e, y, f.get_taps(), f.frames()))
        f.close()
    assert np.all(np.isfinite(got[0][0])) and np.any(got[0][2] != 0)
    for other in got[1:]:
        for a, b, name in zip(got[0][:3], other[:3], ("e", "y", "taps")):
            assert same(a, b), f"grouping: {name} differs"
        assert other[3] == frames


# ------------------------------------------------------------------------------------------------ 5: isolation
def test_neighbours_cannot_reach_a_bin(dev, oracle):
    """with every other (channel, bin) scaled by 2^20, zeroed or NaN, a (channel, bin)'s e, y and weights keep their bits"""
    taps, bins, frames = SMALL
    x, d, _ = bc.case(oracle, taps, bins, frames, 3)
    mine = (1, 7)

    def run(xs, ds):
        r = bc.Device(dev, 3, bins, taps, calls=64)
        with np.errstate(all="ignore"):
            e, y = r.process(xs, ds)
            w = r.get_taps()
        r.close()
        return e[mine[0], :, mine[1]], y[mine[0], :, mine[1]], w[mine[0], :, mine[1]]
    base = run(x, d)
    assert np.all(np.isfinite(base[0])) and np.any(base[2] != 0)
    for name, f in (("scaled by 2^20", lambda a: a * np.float32(2.0 ** 20)), ("zeroed", np.zeros_like),
                    ("NaN", lambda a: np.full_like(a, np.nan + 1j * np.nan))):
        xs, ds = f(x), f(d)
        xs[mine[0], :, mine[1]], ds[mine[0], :, mine[1]] = x[mine[0], :, mine[1]], d[mine[0], :, mine[1]]
        for a, b, what in zip(run(xs, ds), base, ("e", "y", "taps")):
            assert same(a, b), f"isolation: neighbours {name} changed the bin's {what}"


def test_a_frozen_channel_among_adapting_ones(dev, oracle):
    """a channel frozen by set_step while its neighbours adapt keeps get_taps bit for bit; released, it continues as the float64
    model on the same schedule does, under the parity limits"""
    taps, bins, frames = SMALL
    x, d, h = bc.case(oracle, taps, bins, frames, 3)
    third, mine = frames // 3, 1
    runs = []
    for mk in (bc.device(dev), lambda *a: bc.Model(*a, prec=64)):
        r = mk(3, bins, taps, bc.MU, bc.DELTA)
        parts, ws = [], []
        for k, mu in enumerate((None, 0.0, bc.MU)):
            if mu is not None:
                r.set_step(mine, mu)
            lo, hi = k * third, (k + 1) * third if k < 2 else frames
            parts.append(r.process(x[:, lo:hi], d[:, lo:hi])[0])
            ws.append(np.array(r.get_taps()))
        r.close()
        runs.append((np.concatenate(parts, axis=1), ws))
    (e, (w0, w1, w2)), (e_ref, (_, _, w2_ref)) = runs
    assert same(w0[mine], w1[mine]), "a frozen channel's taps moved"
    assert not same(w0[0], w1[0]) and not same(w1[mine], w2[mine])
    d_rms = np.sqrt(np.mean(np.abs(d.astype(np.complex128)) ** 2, axis=1))
    err = bc.run_rms(e.astype(np.complex128) - e_ref)
    error = bc.ratio(err, bc.TOL * np.broadcast_to(d_rms[:, None, :], err.shape))
    tap = bc.ratio(np.sqrt(np.sum(np.abs(w2.astype(np.complex128) - w2_ref.astype(np.complex128)) ** 2, axis=1)),
                   bc.TOL * np.sqrt(np.sum(np.abs(h) ** 2, axis=1)))
    print(f"freeze and release: worst error ratio {error:.3g}, taps {tap:.3g}")
    assert error <= 1.0 and tap <= 1.0


# ------------------------------------------------------------------------------------------------ 6: resets
def test_resets_and_frames(dev, oracle):
    taps, bins, frames = SMALL
    x, d, _ = bc.case(oracle, taps, bins, frames, 3)
    r = bc.Device(dev, 3, bins, taps, calls=[50, 1, 149])
    assert r.frames() == 0
    e0, y0 = r.process(x, d)
    w0 = r.get_taps()
    assert r.frames() == frames and np.any(w0 != 0)
    r.reset(False)
    assert r.frames() == 0 and same(r.get_taps(), w0), "reset(0) changed the taps"
    r.set_step(0, np.zeros(3, np.float32))                      # frozen: behind a reset the first frame's y is w_0 x[0] alone
    _, y = r.process(x[:, :1], d[:, :1])
    assert r.frames() == 1 and same(r.get_taps(), w0)
    want = w0[:, 0].astype(np.complex128) * x[:, 0]
    assert np.all(np.abs(y[:, 0] - want) <= 4 * bc.U * np.abs(w0[:, 0]) * np.abs(x[:, 0])), "reset(0) left history"
    assert np.any(w0[:, 1] != 0)
    r.set_step(0, np.full(3, bc.MU, np.float32))
    r.reset(True)
    assert r.frames() == 0 and not np.any(r.get_taps()), "reset(1) left taps"
    e1, y1 = r.process(x, d)
    w1 = r.get_taps()
    r.close()
    for a, b, name in ((e0, e1, "e"), (y0, y1, "y"), (w0, w1, "taps")):
        assert same(a, b), f"reset(1): {name} differs from a fresh handle's"


# ------------------------------------------------------------------------------------------------ 7: pointers and buffers
CASE = (5, 33, 3, 60, [1, 29, 30])          # taps, bins, channels, frames, calls


@pytest.fixture(scope="module")
def plain(dev, oracle):
    """the case on ordinary device tensors: (e, y, taps)"""
    taps, bins, ch, frames, calls = CASE
    x, d, _ = bc.case(oracle, taps, bins, SMALL[2], ch)
    f = filters.AdaptBandsMC(ch, bins, taps, mu=bc.MU, delta=bc.DELTA)
    e, y = run_calls(f, x[:, :frames], d[:, :frames], calls, *on_device(dev))
    w = f.get_taps()
    f.close()
    return e, y, w


def test_host_pointers_give_the_device_pointers_bits(dev, oracle, plain):
    taps, bins, ch, frames, calls = CASE
    x, d, _ = bc.case(oracle, taps, bins, SMALL[2], ch)
    x, d = x[:, :frames], d[:, :frames]
    f = filters.AdaptBandsMC(ch, bins, taps, mu=bc.MU, delta=bc.DELTA)
    e, y = run_calls(f, x, d, calls, np.ascontiguousarray, lambda *shape: np.full(shape, np.nan, np.float32))
    w = f.get_taps()
    f.close()
    for got, want, name in ((e, plain[0], "e"), (y, plain[1], "y"), (w, plain[2], "taps")):
        assert same(got, want), name
    # mixed: inputs on the host, outputs on the device, no y
    f = filters.AdaptBandsMC(ch, bins, taps, mu=bc.MU, delta=bc.DELTA)
    es, o = [], 0
    for n in calls:
        ins = [a for z in (x[:, o:o + n], d[:, o:o + n]) for a in bc.split(z)]
        outs = [torch.full((ch, n, bins), float("nan"), dtype=F32, device=dev) for _ in range(2)]
        f.process(*ins, *outs)
        es.append(outs[0].cpu().numpy() + 1j * outs[1].cpu().numpy())
        o += n
    assert same(np.concatenate(es, axis=1).astype(np.complex64), plain[0]) and same(f.get_taps(), plain[2])
    f.close()


@pytest.mark.parametrize("with_y", [True, False], ids=["y", "no-y"])
@pytest.mark.parametrize("off", OFFSETS, ids=[f"in{a}-out{b}" for a, b in OFFSETS])
def test_guarded_buffers(dev, oracle, plain, off, with_y):
    """x and d between NaN bands, e and y between sentinel bands, at odd element offsets: the plain tensors' bits, every output
    element written, the bands and the inputs unchanged"""
    taps, bins, ch, frames, calls = CASE
    x, d, _ = bc.case(oracle, taps, bins, SMALL[2], ch)
    ins, outs = [], []

    def up(a):
        buf = gb.carve_input(dev, a, off[0])
        ins.append((buf, gb.snapshot(buf)))
        return buf.shaped(*a.shape)

    def new(*shape):
        buf = gb.carve(dev, F32, int(np.prod(shape)), off[1])
        outs.append(buf)
        return buf.shaped(*shape)
    f = filters.AdaptBandsMC(ch, bins, taps, mu=bc.MU, delta=bc.DELTA)
    e, y = run_calls(f, x[:, :frames], d[:, :frames], calls, up, new, with_y=with_y)
    torch.cuda.synchronize()
    w = f.get_taps()
    f.close()
    assert len(outs) == len(calls) * (4 if with_y else 2) and len(ins) == 4 * len(calls)
    for k, buf in enumerate(outs):
        gb.check_bands(buf, f"bands output {k}")
        gb.check_all_written(buf, f"bands output {k}")
    for k, (buf, snap) in enumerate(ins):
        gb.check_untouched(buf, snap, f"bands input {k}")
    assert same(e, plain[0]) and same(w, plain[2]) and (not with_y or same(y, plain[1])), f"offsets {off}: bits differ"


def test_overlapping_device_ranges_are_refused(dev):
    L = capi.lib()
    ch, bins, taps, frames = 2, 33, 5, 4
    numel = ch * frames * bins
    f = filters.AdaptBandsMC(ch, bins, taps)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    free = [torch.zeros(numel, dtype=F32, device=dev) for _ in range(8)]
    w0 = f.get_taps()
    # (slot of the input or earlier output, slot of the output laid over it) among xre xim dre dim ere eim yre yim
    for lo, hi in ((0, 4), (1, 5), (2, 6), (3, 7), (3, 4), (4, 5), (4, 6), (5, 7), (6, 7)):
        for k, (a, b) in enumerate(gb.overlap_cases(numel, device=dev)):
            bufs = list(free)
            bufs[lo], bufs[hi] = a, b
            before = [gb.bits(t).copy() for t in bufs]
            rc = L.llz_adapt_bands_mc(f.handle, *[ptr(t) for t in bufs], frames)
            msg = capi.last_error()
            assert rc == -1 and "llz_adapt_bands_mc" in msg and "may not overlap" in msg and "(device memory)" in msg, (lo, hi, k, msg)
            torch.cuda.synchronize()
            for t, was in zip(bufs, before):
                assert np.array_equal(gb.bits(t), was), f"slots {lo}, {hi}: case {k} changed a buffer it refused"
    assert f.frames() == 0 and same(f.get_taps(), w0), "a refused call moved the handle"
    big = 2 ** 31 // bins + 1
    assert L.llz_adapt_bands_mc(f.handle, *[ptr(t) for t in free], big) == -1 and "2^31" in capi.last_error()
    assert L.llz_adapt_bands_mc(f.handle, *[ptr(t) for t in free[:7]], None, frames) == -1 and "yre and yim" in capi.last_error()
    # the handle still works, and the other handles' entry points refuse it
    out = (C.c_int * 4)()
    assert L.llz_adapt_mc_plan(f.handle, out) < 0 and L.llz_pfb_mc_bins(f.handle) < 0
    s = filters.AdaptMC(ch, 64, 100)
    assert L.llz_adapt_bands_mc_plan(s.handle, out) < 0 and "llz_adapt_bands_mc_plan" in capi.last_error()
    s.close()
    assert L.llz_adapt_bands_mc(f.handle, *[ptr(t) for t in free], frames) == frames and f.frames() == frames
    torch.cuda.synchronize()
    f.close()


def test_plan_names_the_tap_ceiling(dev):
    for taps in range(1, 65):
        f = filters.AdaptBandsMC(7, 129, taps)
        ceiling, threads, groups, launches = f.plan()
        assert ceiling == bc.ceiling(taps) and ceiling in bc.CEILINGS and ceiling >= taps and (taps > ceiling // 2 or ceiling == 4)
        assert threads % 64 == 0 and groups == -(-7 * 129 // threads) and launches == 1
        f.close()


# ------------------------------------------------------------------------------------------------ 8: end to end
def test_end_to_end_with_the_filter_bank(dev, oracle):
    """bank analysis of white noise x and of d = x * h, AdaptBandsMC on the bands, bank synthesis of e: the bands of e within the
    error limit of the float64 model fed with the device's own analysis bands, and the synthesised residual's rms over the last
    quarter below a tenth of the synthesised d's on every channel (the float64 chain reaches it: test_adapt_bands_host.py)"""
    x, d, w = bc.e2e_case(oracle)
    c, M, P, os, frames, taps = (bc.E2E[k] for k in ("channels", "M", "P", "os", "frames", "taps"))
    bins, hop = M // 2 + 1, M // os
    up, new = on_device(dev)
    bands = []
    for sig in (x, d):
        bank = filters.PfbMC(c, M, hop, P, w, phase=filters.PFB_PHASE_TIME)
        re, im = new(c, frames, bins), new(c, frames, bins)
        bank.analysis(up(sig), re, im)
        bank.close()
        bands.append((re, im))
    X, D = (re.cpu().numpy() + 1j * im.cpu().numpy() for re, im in bands)
    delta = bc.e2e_delta(X)
    f = filters.AdaptBandsMC(c, bins, taps, mu=bc.MU, delta=delta)
    ere, eim = new(c, frames, bins), new(c, frames, bins)
    f.process(*bands[0], *bands[1], ere, eim)
    f.close()
    e = (ere.cpu().numpy() + 1j * eim.cpu().numpy()).astype(np.complex64)
    model = bc.Model(c, bins, taps, delta=delta, prec=64)
    e_ref, _ = model.process(X, D)
    d_rms = np.sqrt(np.mean(np.abs(D.astype(np.complex128)) ** 2, axis=1))
    err = bc.run_rms(e.astype(np.complex128) - e_ref)
    error = bc.ratio(err, bc.TOL * np.broadcast_to(d_rms[:, None, :], err.shape))
    times = []
    for re, im in ((ere, eim), bands[1]):
        bank = filters.PfbMC(c, M, hop, P, w, phase=filters.PFB_PHASE_TIME)
        out = new(c, frames * hop)
        bank.synthesis(re, im, out)
        bank.close()
        times.append(out.cpu().numpy())
    res = bc.e2e_residual(*times)
    print(f"end to end: bands of e at {error:.3g} of the error limit; residual / d over the last quarter per channel: "
          + " ".join(f"{r:.3g}" for r in res) + " (float64 chain: " + " ".join(f"{r:.3g}" for r in bc.e2e_float64(oracle)) + ")")
    assert error <= 1.0
    assert np.all(res < 0.1)
