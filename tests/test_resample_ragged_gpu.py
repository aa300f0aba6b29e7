"""GPU: the batch resampler at ratios with a common factor, through calls that end and start inside a period of L outputs.

llz_resample_mc takes L and M as given, so with g = gcd(L, M) > 1 a valid call may hold a whole number of reduced periods
(M / g inputs) and end inside an L-output period -- which no coprime ratio can do, and every other resampler test uses coprime
ratios and whole periods.  The matrix-core entries (resample_mfma_f32, resample_i16x) store whole periods: handed such a call
they would write L - n_out % L elements past every row, into the next channel's row and, behind the last channel, past the
caller's buffer.  The handle therefore gives them whole-period calls from a period boundary only and runs every other call on
its fallback entry, mid-stream, with a start position that is no multiple of L.

Here every ratio walks rs_ragged_checks.call_plan through ONE handle: ragged from a boundary, back to a boundary, whole
periods, ragged again, a single reduced period from inside a period, back to a boundary, whole periods.  After every call:
the entry that ran (llz_resample_mc_last_entry: a ragged test that silently ran another kernel would prove nothing), both guard
bands of the output (tests/buffer_checks.py; 3 channels, so the middle row has a neighbour on both sides and the last one
only the band behind it), the input untouched.  At the end every sample of every channel against the whole-stream reference:
float32 within rs_ragged_checks.f32_limit and the project's RMS gate, int16 bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import edge_checks as ec  # noqa: E402
from tests import rs_ragged_checks as rr  # noqa: E402

WIN = po.BLACKMAN               # the window of the table in test_rs_ragged_host.py, which pins the entry each ratio reaches
MFMA, F32, I16X, I16 = "resample_mfma_f32", "resample_f32", "resample_i16x", "resample_i16"
SMALL5 = [(4, 6), (6, 4), (2, 4), (8, 6), (40, 64)]

# (name, overrides, primary, fallback, ratios)
F32_ROWS = [
    ("mfma-phase-tile", {"rs_mfma_form": -1}, MFMA, F32, rr.MFMA_RATIOS),
    ("mfma-phase-tile-tiles1", {"rs_mfma_form": -1, "rs_tiles": 1}, MFMA, F32, [(294, 320), (150, 160)]),
    ("mfma-period-tile", {"rs_mfma_form": 1}, MFMA, F32, rr.MFMA_RATIOS),
    ("lds", {}, F32, F32, SMALL5),
    ("generic1", {"rs_generic": 1}, F32, F32, [(294, 320), (150, 160)]),
    ("generic2", {"rs_generic": 2}, F32, F32, [(294, 320), (150, 160)]),
]
F32_CASES = [(name, L, M, 3, off) for (name, _t, _p, _f, ratios) in F32_ROWS for (L, M) in ratios for off in (0, 1)] + \
            [("mfma-phase-tile", 294, 320, 1, 1), ("lds", 4, 6, 1, 1)]
F32_TABLE = {name: (tune, prim, fall) for (name, tune, prim, fall, _r) in F32_ROWS}

# int16: every ratio takes the screen with its designed Blackman taps (test_rs_ragged_host.py pins llzs_resample_i16x_fits; the
# screen's verdict on the taps themselves shows in last_entry() of the first whole-period call)
I16_RATIOS = [(4, 6), (6, 4), (2, 4), (40, 64), (48, 32), (294, 320), (150, 160)]
I16_LAUNCHES = [("default", {}, I16X), ("tiles1-walk3", {"rs_i16_tiles": 1, "rs_i16_walk": 3}, I16X), ("double", {"rs_i16_path": 1}, I16)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


_CACHE = {}


def cached(key, make):
    """inputs, references and limits of a ratio: computed once, shared by its cases, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                # a faulted device serves no later test either: end the session here
        pytest.exit(f"{what}: the device reported an error, nothing more is run on it: {e}", returncode=3)


def walk_calls(dev, r, x, lens, off, what, which="nan"):
    """x through the handle r in calls of lens[] inputs, every buffer carved at element offset `off` between guard bands;
    after each call: bands, input, (float32) every element written.  Returns (outputs joined, entry of each call)."""
    ch = x.shape[0]
    f32 = x.dtype == np.float32
    outs, entries, o = [], [], 0
    for k, n_in in enumerate(lens):
        n_out = r.out_len(n_in)
        assert n_out == n_in * r.L // r.M
        xin = bc.carve_input(dev, x[:, o:o + n_in], off, which=which)
        snap = bc.snapshot(xin)
        y = bc.carve(dev, torch.float32 if f32 else torch.int16, ch * n_out, off)
        assert r.process(xin.shaped(ch, n_in), y.shaped(ch, n_out)) == n_out, capi.last_error()
        sync(what)
        tag = f"{what} call {k} ({n_in} in, {n_out} out, {n_out % r.L} past a period)"
        bc.check_bands(y, tag)
        bc.check_untouched(xin, snap, tag)
        # int16: the sentinel 0x5a5a is a legal sample; equality with the reference proves every element written
        outs.append((bc.check_all_written(y, tag) if f32 else y.host()).reshape(ch, n_out))
        entries.append(r.last_entry())
        o += n_in
    assert o == x.shape[1]
    return np.concatenate(outs, axis=1), entries


def check_entries(entries, kinds, primary, fallback, what):
    """whole-period calls from a boundary run the primary; calls that start inside a period the fallback; calls that end
    inside one either, but all of them the same"""
    print(f"{what}: entries {list(zip(kinds, entries))}")
    ragged = set()
    for kind, e in zip(kinds, entries):
        if kind == "c":
            assert e == primary, (what, kind, e)
        elif kind in ("b", "e", "f"):
            assert e == fallback, (what, kind, e)
        else:
            assert e in (primary, fallback), (what, kind, e)
            ragged.add(e)
    assert len(ragged) == 1, (what, ragged)


def f32_stream(oracle, L, M, channels, gain):
    def make():
        lens, kinds = rr.call_plan(L, M, rr.min_primary(L, M))
        info = oracle.rs_info(2, L, M, gain, WIN)
        x = oracle.synth_f32(channels, sum(lens), seed=L + 2 * M)
        ref = rr.ref_f32(oracle, x, L, M, gain, WIN)
        return lens, kinds, info, x, ref, rr.f32_limit(x, info["matrix"], L, M, gain)
    return cached(("f32", L, M, channels, gain), make)


def f32_value_checks(got, ref, lim, L, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = np.abs(np.asarray(got, dtype=np.float64) - ref)[lim > 0] / lim[lim > 0]
    print(f"{what}: worst |got - ref| / limit = {float(ratio.max()):.3g}")
    ec.sample_check(got, ref, lim, what, period=L)
    ec.rms_check(got, ref, what)


@pytest.mark.parametrize("name,L,M,channels,off", F32_CASES, ids=[f"{c[0]}-{c[1]}:{c[2]}-ch{c[3]}-off{c[4]}" for c in F32_CASES])
def test_resample_f32_ragged_calls(dev, oracle, name, L, M, channels, off):
    tune, primary, fallback = F32_TABLE[name]
    gain = 2.5 if name.endswith("tiles1") else 1.0
    lens, kinds, info, x, ref, lim = f32_stream(oracle, L, M, channels, gain)
    what = f"f32 {name} {L}:{M} ch {channels} off {off}"
    with capi.tuned(**tune):
        r = filters.ResampleMC(channels, L, M, gain, WIN, filters.PCM_F32)
        assert r.Q == info["cols"] and np.array_equal(r.matrix(), info["matrix"]) and r.last_entry() == ""
        got, entries = walk_calls(dev, r, x, lens, off, what)
        r.close()
        assert got.shape[1] == sum(lens) * L // M
        check_entries(entries, kinds, primary, fallback, what)
        f32_value_checks(got, ref, lim, L, what)
        # the same stream in one whole-period call: the same samples to the same limit
        r = filters.ResampleMC(channels, L, M, gain, WIN, filters.PCM_F32)
        got1, entries1 = walk_calls(dev, r, x, [x.shape[1]], off, what + " one call")
        r.close()
    assert entries1 == [primary]
    f32_value_checks(got1, ref, lim, L, what + " one call")


PROBES = [("mfma-phase-tile", 294, 320), ("mfma-phase-tile", 150, 160), ("mfma-period-tile", 294, 320), ("mfma-period-tile", 150, 160),
          ("lds", 4, 6), ("lds", 6, 4), ("lds", 40, 64), ("generic1", 150, 160), ("generic2", 150, 160)]


@pytest.mark.parametrize("name,L,M", PROBES, ids=[f"{c[0]}-{c[1]}:{c[2]}" for c in PROBES])
def test_resample_f32_probe_across_off_period_cuts(dev, oracle, name, L, M):
    """unit impulses, one product per output (edge_checks.rs_probe_signal): every non-zero tap alone, to 4 units of float32
    round-off, with cuts off a period boundary inside a response, so the entry changes in the middle of it"""
    tune, primary, fallback = F32_TABLE[name]
    info = oracle.rs_info(2, L, M, 1.0, WIN)
    mat, Q = info["matrix"], info["cols"]
    x, positions = ec.rs_probe_signal(L, M, Q)
    lens = rr.probe_cuts(positions, x.shape[1], L, M, Q)
    assert ec.rs_straddles(positions, lens, L, M, Q) >= 4
    ref = rr.ref_f32(oracle, x, L, M, 1.0, WIN)
    assert ec.rs_hits(positions, ref.shape[1], L, M, Q)[mat != 0].all()
    what = f"probe {name} {L}:{M} calls {lens}"
    with capi.tuned(**tune):
        r = filters.ResampleMC(3, L, M, 1.0, WIN, filters.PCM_F32)
        got, entries = walk_calls(dev, r, x, lens, 1, what)
        r.close()
    assert entries == rr.expected_entries(lens, L, M, primary, fallback), (what, entries)
    ec.rs_probe_check(got, ref, what)


def i16_stream(oracle, L, M, channels):
    def make():
        lens, kinds = rr.call_plan(L, M, rr.min_primary(L, M))
        x = rr.i16_rows(oracle, sum(lens), seed=L * 7 + M)
        x = x if channels == 9 else np.ascontiguousarray(x[-channels:])
        return lens, kinds, x, rr.ref_i16(oracle, x, L, M, 1.0, WIN)
    return cached(("i16", L, M, channels), make)


I16_CASES = [(L, M, 9) for (L, M) in I16_RATIOS] + [(4, 6, 1)]


@pytest.mark.parametrize("L,M,channels", I16_CASES, ids=[f"{c[0]}:{c[1]}-ch{c[2]}" for c in I16_CASES])
def test_resample_i16_ragged_calls_are_bit_exact(dev, oracle, L, M, channels):
    """LLZ_PCM_I16, the rows of test_resample_i16_lm_screened_is_bit_exact (the last one random PCM: a busy row in front of the
    guard band), three launches: the default screened launch, one period tile per span in walks of three, the all-double kernel"""
    lens, kinds, x, ref = i16_stream(oracle, L, M, channels)
    for k, (name, tune, primary) in enumerate(I16_LAUNCHES):
        what = f"i16 {name} {L}:{M} ch {channels}"
        with capi.tuned(**tune):
            r = filters.ResampleMC(channels, L, M, 1.0, WIN, filters.PCM_I16)
            got, entries = walk_calls(dev, r, x, lens, k % 2, what, which=("max", "min")[k % 2])
            r.close()
        check_entries(entries, kinds, primary, I16, what)
        assert got.shape == ref.shape and got.dtype == ref.dtype
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize("fmt,L,M", [(filters.PCM_F32, 294, 320), (filters.PCM_I16, 4, 6)], ids=["f32-294:320", "i16-4:6"])
def test_resample_ragged_calls_host_buffers(dev, oracle, fmt, L, M):
    """numpy in and out: the library stages both, and a store past a row would land past its own staging allocation"""
    f32 = fmt == filters.PCM_F32
    if f32:
        lens, kinds, info, x, ref, lim = f32_stream(oracle, L, M, 3, 1.0)
    else:
        lens, kinds, x, ref = i16_stream(oracle, L, M, 9)
    ch = x.shape[0]
    r = filters.ResampleMC(ch, L, M, 1.0, WIN, fmt)
    outs, entries, o = [], [], 0
    for n_in in lens:
        y = np.full((ch, r.out_len(n_in)), np.nan if f32 else 0x5a5a, dtype=x.dtype)
        assert r.process(np.ascontiguousarray(x[:, o:o + n_in]), y) == y.shape[1], capi.last_error()
        outs.append(y)
        entries.append(r.last_entry())
        o += n_in
    r.close()
    sync("host buffers")
    got = np.concatenate(outs, axis=1)
    check_entries(entries, kinds, MFMA if f32 else I16X, F32 if f32 else I16, f"host buffers {L}:{M}")
    if f32:
        f32_value_checks(got, ref, lim, L, f"host buffers f32 {L}:{M}")
    else:
        assert np.array_equal(got, ref)


def test_out_len_refuses_a_fraction_of_a_step_and_the_stream_goes_on(dev, oracle):
    """4:6, n_in = 4: n_in L % M != 0.  Refused by out_len and by the call itself, the stream position unchanged: the next
    valid call still matches the reference"""
    L, M, ch = 4, 6, 3
    lens, kinds, info, x, ref, lim = f32_stream(oracle, L, M, ch, 1.0)
    lib = capi.lib()
    r = filters.ResampleMC(ch, L, M, 1.0, WIN, filters.PCM_F32)
    first = lens[0]
    got0, _ = walk_calls(dev, r, x[:, :first], [first], 0, "before the refusal")
    assert lib.llz_resample_mc_out_len(r.handle, 4) < 0 and "not a multiple of M" in capi.last_error()
    xin = bc.carve_input(dev, x[:, first:first + 4], 0)
    y = bc.carve(dev, torch.float32, ch * 4, 0)
    assert lib.llz_resample_mc(r.handle, xin.view.data_ptr(), 4, y.view.data_ptr()) < 0
    sync("refused call")
    assert np.all(bc.bits(y.region) == y.band), "a refused call wrote its output"
    assert r.last_entry() == F32
    with pytest.raises(capi.LlzError):
        r.out_len(4)
    got1, _ = walk_calls(dev, r, x[:, first:], lens[1:], 0, "after the refusal")
    r.close()
    f32_value_checks(np.concatenate([got0, got1], axis=1), ref, lim, L, "4:6 around a refused call")
