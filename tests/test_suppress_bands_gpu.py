"""The per-band postfilter on the device (include/llz_suppress_bands.h, llz_suppress_bands_mc; kernel k_bands_suppress of
suppress_bands.hip) against the float64 model of its definition (tests/suppress_bands_checks.py, where every limit is stated):

  1. parity of o, g and all seven states, o = g e and the zero bin on every shape, 3 and 37 channels, with and without y and g, and
     on rows of 2049 bins;
  2. y passed with eta = 0 gives the bits of a call without y;
  3. a disabled channel among enabled ones: e's bits out, a gain of 1, its state unchanged; re-enabled mid-stream it moves again;
  4. grouping: all frames at once, 1 frame per call, and calls of [7, 1, 0, 30] frames across n = W and a window swap, o, g and
     the states bit-equal;
  5. isolation: neighbouring bins and channels scaled by 2^20, zeroed or NaN;
  6. reset repeats a fresh handle's bits and keeps floors, leakages and flags; frames(); refused floors and leakages change nothing;
  7. pointers and buffers: host against device pointers, guarded buffers at odd offsets, overlapping device ranges refused, plan();
  8. the properties of the header on the device;
  9. end to end: PfbMC analysis of x and d, KalmanBandsMC with y, SuppressBandsMC on (e, y), PfbMC synthesis of o.

Every parity case prints its worst ratios.  On the parent of this feature the library exports no llz_suppress_bands_mc and every
test here fails."""
import ctypes as C

import numpy as np
import pytest
import torch

from llzlab_amd import capi, filters
from tests import adapt_bands_checks as bc
from tests import buffer_checks as gb
from tests import kalman_bands_checks as kc
from tests import suppress_bands_checks as sc

pytestmark = pytest.mark.gpu
F32 = torch.float32
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 3)]                  # elements past a 256-byte boundary: (inputs, outputs)
SMALL = sc.SHAPES[0]                                        # 5 bins, 200 frames, W = 16: twelve channels in a wave
MID = sc.SHAPES[1]                                          # 33 bins, 300 frames, W = 64
FORMS = [(True, True), (False, True), (True, False), (False, False)]      # (with y, with g)


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
    """[7, channels, bins] of a filters.SuppressBandsMC or a suppress_bands_checks.Device"""
    return np.stack([f.get_state(k) for k in range(7)])


# ------------------------------------------------------------------------------------------------ 1: parity
@pytest.mark.parametrize("channels", sc.CHANNELS)
@pytest.mark.parametrize("bins,frames,W", sc.SHAPES)
def test_parity_of_outputs_and_state(dev, oracle, bins, frames, W, channels):
    """the worst ratios are printed (holds the measured ones); calls of 37 frames"""
    sc.check_parity(sc.device(dev, calls=37), oracle, bins, frames, W, channels)


@pytest.mark.parametrize("with_y,with_g", FORMS[1:], ids=["no-y", "no-g", "no-y-no-g"])
@pytest.mark.parametrize("bins,frames,W", sc.SHAPES)
def test_parity_of_the_other_forms(dev, oracle, bins, frames, W, with_y, with_g):
    sc.check_parity(sc.device(dev, calls=53), oracle, bins, frames, W, 3, with_y=with_y, want_g=with_g)


def test_parity_on_rows_longer_than_a_workgroup(dev, oracle):
    bins, frames, W, channels = sc.LONG
    sc.check_parity(sc.device(dev), oracle, bins, frames, W, channels)


# ------------------------------------------------------------------------------------------------ 2: y at eta = 0
def test_y_without_leakage_is_no_y(dev, oracle):
    bins, frames, W = MID
    e, y, _ = sc.scene(oracle, bins, frames, W, 3)
    got = []
    for ys in (y, None):
        r = sc.Device(dev, 3, bins, calls=[64, 1, 100], window=W)
        o, g = r.process(e, ys)
        got.append((o, g, state(r)))
        r.close()
    assert np.any(y != 0) and all(same(a, b) for a, b in zip(*got)), "y at eta = 0 changed a bit"
    assert not np.any(got[0][2][5]), "R moved without leakage"


# ------------------------------------------------------------------------------------------------ 3: disabled channels
def test_a_disabled_channel_among_enabled_ones(dev, oracle):
    """channel 1 disabled behind the first third while its neighbours run: its o has e's bits, its g is 1, its seven state values
    keep their bits and the count goes on; re-enabled it continues from the state it kept, as the model does"""
    bins, frames, W = SMALL
    e, y, eta = sc.scene(oracle, bins, frames, W, 3)
    frames, third, mine = 90, 30, 1
    r = sc.Device(dev, 3, bins, calls=[7, 23], window=W)
    m = sc.Model(3, bins, window=W, prec=64)
    for f in (r, m):
        f.set_leak(0, eta)
        f.process(e[:, :third], y[:, :third])
    s0 = state(r)
    for f in (r, m):
        f.set_enable(mine, 0)
    o, g = r.process(e[:, third:2 * third], y[:, third:2 * third])
    m.process(e[:, third:2 * third], y[:, third:2 * third])
    s1 = state(r)
    assert same(o[mine], e[mine, third:2 * third]) and np.all(g[mine] == 1), "a disabled channel's output is not its input"
    assert same(s0[:, mine], s1[:, mine]), "a disabled channel's state moved"
    assert not same(s0[:, 0], s1[:, 0]) and not same(o[0], e[0, third:2 * third]), "an enabled channel stood still"
    for f in (r, m):
        f.set_enable(mine, 1)
    o, g = r.process(e[:, 2 * third:frames], y[:, 2 * third:frames])
    o_ref, g_ref = m.process(e[:, 2 * third:frames], y[:, 2 * third:frames])
    s2 = state(r)
    assert r.frames() == frames and not same(s1[:, mine], s2[:, mine])
    assert np.max(np.abs(g - g_ref)) <= sc.TOL and sc.ratio(np.abs(s2[4] - m.st["N"]), sc.TOL * m.st["N"]) <= 1
    r.close()


# ------------------------------------------------------------------------------------------------ 4: grouping
def on_device(dev):
    return (lambda a: torch.from_numpy(np.array(a, order="C")).to(dev),           # (a copy: the shared cases are read-only)
            lambda *shape: torch.full(shape, float("nan"), dtype=F32, device=dev))


def run_calls(f, e, y, sizes, up, new, with_g=True):
    """e, y (or None) complex [channels, frames, bins] through handle f in calls of `sizes` frames (0 included: an empty call);
    up(a) makes an input buffer of a float32 array, new(*shape) an output buffer.  Returns (o complex64, g float32 or zeros)."""
    os, gs, at = [], [], 0
    shape = lambda n: (e.shape[0], n, e.shape[2])               # noqa: E731
    for n in sizes:
        ins = [up(a) for a in sc.split(e[:, at:at + n])]
        ys = [None, None] if y is None else [up(a) for a in sc.split(y[:, at:at + n])]
        outs = [new(*shape(n)) for _ in range(3 if with_g else 2)]
        f.process(*ins, outs[0], outs[1], *ys, outs[2] if with_g else None)
        got = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in outs]
        os.append(got[0] + 1j * got[1])
        gs.append(got[2] if with_g else got[0] * 0)
        at += n
    assert at == e.shape[1]
    return np.concatenate(os, axis=1).astype(np.complex64), np.concatenate(gs, axis=1).astype(np.float32)


def new_filter(ch, bins, W, eta=None):
    f = filters.SuppressBandsMC(ch, bins, window=W)
    if eta is not None:
        f.set_leak(0, eta)
    return f


@pytest.mark.parametrize("bins,total,W", [sc.SHAPES[0], sc.SHAPES[2]])
def test_grouping_of_frames_into_calls_changes_no_bit(dev, oracle, bins, total, W):
    """2 W + 12 frames: the calls end in the start-up, cross n = W and the window swap at 2 W"""
    frames = 2 * W + 12
    e, y, eta = sc.scene(oracle, bins, total, W, 3)
    e, y = e[:, total - frames:], y[:, total - frames:]         # the scene's end: y and the echo channels are live
    got = []
    for calls in (None, 1, [7, 1, 0, 30]):
        f = new_filter(3, bins, W, eta)
        o, g = run_calls(f, e, y, sc.sizes(calls, frames), *on_device(dev))
        got.append((o, g, state(f), f.frames()))
        f.close()
    assert np.all(np.isfinite(got[0][0])) and np.any(got[0][2][5] != 0) and np.any(got[0][1] != np.float32(sc.GMIN))
    for other in got[1:]:
        for a, b, name in zip(got[0][:3], other[:3], ("o", "g", "state")):
            assert same(a, b), f"grouping: {name} differs"
        assert other[3] == frames


# ------------------------------------------------------------------------------------------------ 5: isolation
def test_neighbours_cannot_reach_a_bin(dev, oracle):
    """with every other (channel, bin) scaled by 2^20, zeroed or NaN, a (channel, bin)'s o, g and state keep their bits"""
    bins, frames, W = MID
    e, y, eta = sc.scene(oracle, bins, frames, W, 3)
    mine = (2, 8)                                               # an echo channel's burst bin

    def run(es, ys):
        r = sc.Device(dev, 3, bins, calls=64, window=W)
        r.set_leak(0, eta)
        o, g = r.process(es, ys)
        s = state(r)
        r.close()
        c, k = mine
        return o[c, :, k], g[c, :, k], s[:, c, k]
    base = run(e, y)
    assert np.all(np.isfinite(base[0])) and np.all(base[2][[0, 4, 5]] > 0)
    for name, f in (("scaled by 2^20", lambda a: a * np.float32(2.0 ** 20)), ("zeroed", np.zeros_like),
                    ("NaN", lambda a: np.full_like(a, np.nan + 1j * np.nan))):
        es, ys = f(e), f(y)
        es[mine[0], :, mine[1]], ys[mine[0], :, mine[1]] = e[mine[0], :, mine[1]], y[mine[0], :, mine[1]]
        for a, b, what in zip(run(es, ys), base, ("o", "g", "state")):
            assert same(a, b), f"isolation: neighbours {name} changed the bin's {what}"


def test_a_nan_stays_in_its_bin_until_reset(dev, oracle):
    bins, frames, W = SMALL
    e, _, _ = sc.scene(oracle, bins, frames, W, 3)
    e = e[:, :60]
    bad = e.copy()
    bad[1, 20, 3] = np.nan
    r = sc.Device(dev, 3, bins, window=W)
    o0, g0 = r.process(e)
    s0 = state(r)
    r.reset()
    o1, _ = r.process(bad)
    s1 = state(r)
    assert np.isnan(s1[0, 1, 3]) and np.isnan(s1[4, 1, 3]) and np.all(np.isnan(o1[1, 20:, 3].real))
    keep = np.ones((3, bins), bool)
    keep[1, 3] = False
    assert same(s0[:, keep], s1[:, keep]) and same(o0[:, :20], o1[:, :20])
    assert all(same(o0[c][:, keep[c]], o1[c][:, keep[c]]) for c in range(3))
    r.reset()
    o2, g2 = r.process(e)
    assert same(o0, o2) and same(g0, g2) and same(s0, state(r))
    r.close()


# ------------------------------------------------------------------------------------------------ 6: reset, setters
def test_reset_frames_and_setters(dev, oracle):
    bins, frames, W = SMALL
    e, y, eta = sc.scene(oracle, bins, frames, W, 3)
    r = sc.Device(dev, 3, bins, calls=[50, 1, 149], window=W)
    s = state(r)
    assert r.frames() == 0 and np.all(s[3] == 1) and not np.any(s[[0, 1, 2, 4, 5, 6]])
    r.set_leak(0, eta)
    r.set_floor(1, [0.5, 0.0])
    r.set_enable(0, [1, 1, 0])
    o0, g0 = r.process(e, y)
    s0 = state(r)
    assert r.frames() == frames and np.all(g0[1] >= 0.5) and np.any(g0[0] < 0.5) and same(o0[2], e[2])
    assert same(r.f.get_state("N", 1, 1), s0[4, 1:2]) and same(r.f.get_state(sc.STATES.index("Z"), 2), s0[6, 2:])
    L = capi.lib()
    for name, bad in (("set_floor", (-1e-30, 1.0000001, float("nan"))), ("set_leak", (-1e-30, float("inf"), float("nan")))):
        for v in bad:
            with pytest.raises(capi.LlzError, match="llz_suppress_bands_mc_" + name):
                getattr(r.f, name)(0, [0.2, v, 0.2])
    for which in (-1, 7):
        out = np.empty((3, bins), np.float32)
        assert L.llz_suppress_bands_mc_get_state(r.f.handle, which, 0, 3, out.ctypes.data) == -1 and "outside 0..6" in capi.last_error()
    r.reset()
    s = state(r)
    assert r.frames() == 0 and np.all(s[3] == 1) and not np.any(s[[0, 1, 2, 4, 5, 6]]), "reset left state"
    o1, g1 = r.process(e, y)
    for a, b, name in zip((o0, g0, s0), (o1, g1, state(r)), ("o", "g", "state")):
        assert same(a, b), f"reset: {name} differs (a refused setter changed something, or reset dropped floors, leakages or flags)"
    fresh = sc.Device(dev, 3, bins, window=W)
    fresh.set_leak(0, eta)
    fresh.set_floor(1, [0.5, 0.0])
    fresh.set_enable(2, 0)
    o2, g2 = fresh.process(e, y)
    assert same(o0, o2) and same(g0, g2) and same(s0, state(fresh)), "reset does not repeat a fresh handle's bits"
    fresh.close()
    r.close()


# ------------------------------------------------------------------------------------------------ 7: pointers and buffers
CASE = (33, 3, 60, 16, [1, 29, 30])          # bins, channels, frames, W, calls


def case_signals(oracle):
    bins, ch, frames, W, calls = CASE
    e, y, eta = sc.scene(oracle, bins, 300, 64, ch)
    return e[:, 300 - frames:], y[:, 300 - frames:], eta


@pytest.fixture(scope="module")
def plain(dev, oracle):
    """the case on ordinary device tensors: (o, g, state)"""
    bins, ch, frames, W, calls = CASE
    e, y, eta = case_signals(oracle)
    f = new_filter(ch, bins, W, eta)
    o, g = run_calls(f, e, y, calls, *on_device(dev))
    out = (o, g, state(f))
    f.close()
    return out


def test_host_pointers_give_the_device_pointers_bits(dev, oracle, plain):
    bins, ch, frames, W, calls = CASE
    e, y, eta = case_signals(oracle)
    f = new_filter(ch, bins, W, eta)
    o, g = run_calls(f, e, y, calls, np.ascontiguousarray, lambda *shape: np.full(shape, np.nan, np.float32))
    for got, want, name in zip((o, g, state(f)), plain, ("o", "g", "state")):
        assert same(got, want), name
    f.close()
    # mixed: inputs on the host, outputs on the device, no g
    f = new_filter(ch, bins, W, eta)
    o, _ = run_calls(f, e, y, calls, np.ascontiguousarray, on_device(dev)[1], with_g=False)
    assert same(o, plain[0]) and same(state(f), plain[2])
    f.close()


@pytest.mark.parametrize("with_y,with_g", FORMS, ids=["y-g", "no-y", "no-g", "no-y-no-g"])
@pytest.mark.parametrize("off", OFFSETS, ids=[f"in{a}-out{b}" for a, b in OFFSETS])
def test_guarded_buffers(dev, oracle, plain, off, with_y, with_g):
    """e and y between NaN bands, o and g between sentinel bands, at odd element offsets: every output element written, the bands
    and the inputs unchanged, and with y the plain tensors' bits"""
    bins, ch, frames, W, calls = CASE
    e, y, eta = case_signals(oracle)
    ins, outs = [], []

    def up(a):
        buf = gb.carve_input(dev, a, off[0])
        ins.append((buf, gb.snapshot(buf)))
        return buf.shaped(*a.shape)

    def new(*shape):
        buf = gb.carve(dev, F32, int(np.prod(shape)), off[1])
        outs.append(buf)
        return buf.shaped(*shape)
    f = new_filter(ch, bins, W, eta)
    o, g = run_calls(f, e, y if with_y else None, calls, up, new, with_g=with_g)
    torch.cuda.synchronize()
    s = state(f)
    assert f.plan()[0] == int(with_y)
    f.close()
    assert len(outs) == len(calls) * (3 if with_g else 2) and len(ins) == len(calls) * (4 if with_y else 2)
    for k, buf in enumerate(outs):
        gb.check_bands(buf, f"suppress output {k}")
        gb.check_all_written(buf, f"suppress output {k}")
    for k, (buf, snap) in enumerate(ins):
        gb.check_untouched(buf, snap, f"suppress input {k}")
    if with_y:
        assert same(o, plain[0]) and (not with_g or same(g, plain[1])) and same(s, plain[2]), f"offsets {off}: bits differ"
    else:
        echo = sc.echo_channels(ch)
        assert same(o[~echo], plain[0][~echo]) and not same(o[echo], plain[0][echo]), f"offsets {off}: bits differ"


def test_overlapping_device_ranges_are_refused(dev):
    L = capi.lib()
    ch, bins, frames = 2, 33, 4
    numel = ch * frames * bins
    f = filters.SuppressBandsMC(ch, bins, window=16)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    free = [torch.zeros(numel, dtype=F32, device=dev) for _ in range(7)]
    s0 = state(f)
    # (slot of the input or earlier output, slot of the output laid over it) among ere eim yre yim ore oim g
    for lo, hi in ((0, 4), (1, 5), (2, 6), (3, 4), (2, 5), (0, 6), (4, 5), (4, 6), (5, 6)):
        for k, (a, b) in enumerate(gb.overlap_cases(numel, device=dev)):
            bufs = list(free)
            bufs[lo], bufs[hi] = a, b
            before = [gb.bits(t).copy() for t in bufs]
            rc = L.llz_suppress_bands_mc(f.handle, *[ptr(t) for t in bufs], frames)
            msg = capi.last_error()
            assert rc == -1 and "llz_suppress_bands_mc:" in msg and "may not overlap" in msg and "(device memory)" in msg, (lo, hi, k, msg)
            torch.cuda.synchronize()
            for t, was in zip(bufs, before):
                assert np.array_equal(gb.bits(t), was), f"slots {lo}, {hi}: case {k} changed a buffer it refused"
    assert f.frames() == 0 and same(state(f), s0), "a refused call moved the handle"
    big = 2 ** 31 // bins + 1
    assert L.llz_suppress_bands_mc(f.handle, *[ptr(t) for t in free], big) == -1 and "2^31" in capi.last_error()
    half = list(free)
    half[3] = None
    assert L.llz_suppress_bands_mc(f.handle, *[ptr(t) for t in half], frames) == -1 and "yre and yim" in capi.last_error()
    assert f.frames() == 0
    # the handle still works, and the other handles' entry points refuse it
    out = (C.c_int * 4)()
    assert L.llz_kalman_bands_mc_plan(f.handle, out) < 0 and L.llz_pfb_mc_bins(f.handle) < 0
    k = filters.KalmanBandsMC(ch, bins, 4)
    assert L.llz_suppress_bands_mc_plan(k.handle, out) < 0 and "llz_suppress_bands_mc_plan" in capi.last_error()
    k.close()
    assert L.llz_suppress_bands_mc(f.handle, *[ptr(t) for t in free], frames) == frames and f.frames() == frames
    torch.cuda.synchronize()
    f.close()


def test_plan_and_frames(dev):
    for ch, bins in ((1, 1), (7, 129), (3, 4097), (100, 64)):
        f = filters.SuppressBandsMC(ch, bins)
        assert f.plan() == (0, 64, -(-ch * bins // 64), 1) and f.frames() == 0
        bufs = [torch.zeros(ch, 3, bins, dtype=F32, device=dev) for _ in range(7)]
        f.process(bufs[0], bufs[1], bufs[4], bufs[5], bufs[2], bufs[3], bufs[6])
        assert f.plan()[0] == 1 and f.frames() == 3
        f.process(bufs[0][:, :0], bufs[1][:, :0], bufs[4][:, :0], bufs[5][:, :0])      # an empty call keeps the form
        assert f.plan()[0] == 1 and f.frames() == 3
        f.process(bufs[0], bufs[1], bufs[4], bufs[5])
        assert f.plan() == (0, 64, -(-ch * bins // 64), 1) and f.frames() == 6
        with pytest.raises(capi.LlzError):
            f.process(bufs[0], bufs[1], bufs[4], bufs[5], y_re=bufs[2])
        with pytest.raises(capi.LlzError):
            f.process(bufs[0], bufs[1], bufs[4], bufs[5][:, :2])
        torch.cuda.synchronize()
        f.close()


# ------------------------------------------------------------------------------------------------ 8: properties
def test_properties_on_the_device(dev, oracle):
    """suppress_bands_checks' property case: the figures the float64 model gives, with the same margins (1 dB, 0.05 for a gain),
    and every figure within 0.01 (dB or gain) of the float64 model's"""
    ref = sc.prop_float64(oracle)
    got = sc.prop_figures(sc.Device(dev, sc.PROP["channels"], sc.PROP["bins"], calls=[100, 33]), oracle)
    print("properties, device:        " + ", ".join(f"{k} {v:.4g}" for k, v in got.items()))
    print("properties, float64 model: " + ", ".join(f"{k} {v:.4g}" for k, v in ref.items()))
    sc.prop_check(got)
    assert all(abs(got[k] - ref[k]) <= 0.01 for k in ref), (got, ref)


# ------------------------------------------------------------------------------------------------ 9: end to end
def test_end_to_end_with_the_filter_bank(dev, oracle):
    """bank analysis of white noise x and of d = x * h plus a near-end burst, KalmanBandsMC on the bands with y, SuppressBandsMC
    on (e, y) at eta = 0.01, bank synthesis of o: the synthesised output's rms over the last quarter, behind the burst, relative
    to the synthesised d's, is within a factor of 2 of the float64 chain's on every channel, and below the canceller's own
    residual (in the float64 chain the postfilter sits at its floor there: a tenth of the residual)"""
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
    D = bands[1][0].cpu().numpy() + 1j * bands[1][1].cpu().numpy()
    f = filters.KalmanBandsMC(c, bins, taps, **kc.e2e_params(X))
    e, y = (new(c, frames, bins), new(c, frames, bins)), (new(c, frames, bins), new(c, frames, bins))
    f.process(*bands[0], *bands[1], *e, *y)
    f.close()
    s = filters.SuppressBandsMC(c, bins, **sc.e2e_params(D))
    s.set_leak(0, np.full(c, sc.ETA, np.float32))
    o = new(c, frames, bins), new(c, frames, bins)
    s.process(*e, *o, *y)
    s.close()
    times = []
    for re, im in (o, e, bands[1]):
        bank = filters.PfbMC(c, M, hop, P, w, phase=filters.PFB_PHASE_TIME)
        out = new(c, frames * hop)
        bank.synthesis(re, im, out)
        bank.close()
        times.append(out.cpu().numpy())
    res, res_e = bc.e2e_residual(times[0], times[2]), bc.e2e_residual(times[1], times[2])
    ref, ref_e = sc.e2e_float64(oracle)
    print("end to end: output / d over the last quarter per channel: " + " ".join(f"{r:.4g}" for r in res)
          + " (canceller alone: " + " ".join(f"{r:.4g}" for r in res_e) + "; float64 chain: " + " ".join(f"{r:.4g}" for r in ref)
          + ", canceller alone " + " ".join(f"{r:.4g}" for r in ref_e) + ")")
    assert np.all(np.isfinite(res)) and np.all(res <= 2 * ref) and np.all(res >= ref / 2) and np.all(res < res_e)
