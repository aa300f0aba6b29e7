"""GPU: the biquad bank llz_iir_bank_mc -- the multi-channel cascade with a coefficient set per channel (the tail kernel, the
stage pipeline and the float32 16-sample wave form, each with its tables per channel).  The reference is the unchanged double
oracle called one channel at a time with that channel's set; the limits are those of tests/iir_checks.py, applied to every
channel, sample and (float32) 1024-sample chunk.  Families and helpers: tests/iir_bank_checks.py; test_iir_bank_host.py shows
on the CPU that the families meet the limits' conditions and that a neighbour's set misses them by orders of magnitude.

Each case selects a form by its tunes and ASSERTS through plan() that this form ran, in this precision, split along time, and
warmed up over the maximum of the channels' probed memories.  Frames are the smallest of whole 2048-sample chunks + 1024 + 40
samples that the plan splits; two calls, so the chunked kernel, the tail kernel and the hand-over between calls take part."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import iir_bank_checks as ib  # noqa: E402
from tests import iir_checks as ic  # noqa: E402
from tests import test_buffer_contract_gpu as tb  # noqa: E402
from tests.test_iir_signals_gpu import report, smallest_split_frame, two_calls  # noqa: E402

CHANNELS = ib.CHANNELS
WAVE = {"iir_wave_min_items": 0}
PIPE = {"iir_pipe": 1}
ERR_ARG = -1
FORM = {32: "wave16", 64: "pipe"}          # what a bank runs under the WAVE tunes, by precision


def twelve():
    f = ib.family32(8)
    return np.concatenate([f, f[:, :4]], axis=1)


# id, coefficient sets [37, stages, 6], tunes, the form and precision that must run, forced segment count (None: at least 3)
CASES = [
    ("pipe-f32", ib.family32(8), PIPE, "pipe", 32, None),
    ("pipe-f64", ib.family64(8), PIPE, "pipe", 64, None),
    ("wave16-f32-8", ib.family32(8), WAVE, "wave16", 32, None),
    ("wave16-f32-5", ib.family32(5), WAVE, "wave16", 32, None),
    # a bank in double has no wave form (the bank pipeline measured faster): under the wave tunes it runs the pipeline
    ("f64-8-takes-pipe", ib.family64(8), WAVE, "pipe", 64, None),
    ("f64-3-takes-pipe", ib.family64(3), WAVE, "pipe", 64, None),
    ("wave16-f32-5-segments", ib.family32(8), dict(WAVE, iir_segs=5), "wave16", 32, 5),
    ("pipe-f64-5-segments", ib.family64(3), dict(WAVE, iir_segs=5), "pipe", 64, 5),
    ("pipe-f32-12-sections", twelve(), {}, "pipe", 32, None),
]
# the cases whose bank kernel reads host-built tables, which is all of them: a bank of equal rows is the shared form, bit for bit
EQUAL_ROW_CASES = [c for c in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def kept(x, names, base_of, precision, stages):
    """x with the rows of the F32_DROPPED pairs silenced (a float32 kernel is not held to them)"""
    for c in range(len(x)):
        if (precision, stages, c % CHANNELS, names[base_of[c]]) in ib.F32_DROPPED:
            x[c] = 0
    return x


def signals_for(plan, n, mem, coef, precision):
    """two frames of n samples: impulses at the plan's marks in both calls and at the kernel and call joins, the burst gap
    longer than the handle's memory, channel c carrying row c mod rows at 2^e_c"""
    main = ic.main_samples(plan, n)
    marks = ic.marks_of(plan, main)
    assert len(marks) == plan["segs"] - 1
    marks = marks + [(n + s, w) for s, w in marks]
    joins = sorted({main, n, n + main} - {0, 2 * n})
    rows = ib.rows_for(2 * n, marks, (mem + 1) * ic.CHUNK, joins)
    x, names, base_of = ib.bank_input(rows, coef)
    return kept(x, names, base_of, precision, coef.shape[1])


def held(oracle, got, x, coef, precision, what, plan, n, real=None):
    ic.assert_zero_rows(got, x, what)
    ref, P = ib.per_channel_ref(oracle, x, coef, precision, real)
    seg_len = plan["seg_chunks"] * plan["chunk"] or None
    report(what, plan, n, ic.local_checks(got, ref, x, precision, what, seg_len, P=P))


@pytest.mark.parametrize("case,coef,tunes,form,precision,forced", CASES, ids=[c[0] for c in CASES])
def test_bank_forms_on_signals(dev, oracle, case, coef, tunes, form, precision, forced):
    mem = ib.bank_warm(oracle, coef)
    with capi.tuned(**tunes):
        f = filters.IirBankMC(CHANNELS, coef)
        n = smallest_split_frame(f.plan, forced)
        plan = f.plan(n)
        assert (plan["form"], plan["precision"], f.precision) == (form, precision, precision), (case, plan)
        assert plan["segs"] == forced if forced else plan["segs"] >= 3, (case, plan)
        assert plan["warm"] == mem and plan["chunk"] == ic.CHUNK and plan["seg_chunks"] >= plan["warm"], (case, plan, mem)
        assert ic.main_samples(plan, n) == n - 40
        x = signals_for(plan, n, mem, coef, precision)
        got = two_calls(f, x, n, dev)
        f.close()
    held(oracle, got, x, coef, precision, f"bank {case}", plan, n)


@pytest.mark.parametrize("case,coef,tunes,form,precision,forced", EQUAL_ROW_CASES, ids=[c[0] for c in EQUAL_ROW_CASES])
def test_bank_of_equal_rows_is_the_shared_form(dev, oracle, case, coef, tunes, form, precision, forced):
    """IirBankMC(C, tile(coef_0)) == IirCascadeMC(C, coef_0) bit for bit, both under the same forced iir_segs (the two forms
    hold different numbers of waves, so their own segment counts may differ) and with equal plans.  The shared handle is put on
    the bank's form: its 16-sample float32 wave form (iir_unpacked = 2: the bank has no 32-sample ones) or the pipeline."""
    one = coef[0]
    segs = forced or 3
    same_form = {"iir_pipe": 1} if form == "pipe" else {"iir_unpacked": 2}     # what puts the shared handle on the bank's form
    with capi.tuned(**dict(tunes, iir_segs=segs, **same_form)):
        b = filters.IirBankMC(CHANNELS, np.tile(one, (CHANNELS, 1, 1)))
        s = filters.IirCascadeMC(CHANNELS, one)
        n = smallest_split_frame(b.plan, segs)
        assert b.plan(n) == s.plan(n) and b.plan(n)["form"] == form and b.precision == s.precision == precision, (b.plan(n), s.plan(n))
        x = signals_for(b.plan(n), n, ib.probe(oracle, one)[0], np.tile(one, (CHANNELS, 1, 1)), precision)
        got_b, got_s = two_calls(b, x, n, dev), two_calls(s, x, n, dev)
        b.close()
        s.close()
    assert np.array_equal(got_b.view(np.uint32), got_s.view(np.uint32)), \
        f"{case}: {np.count_nonzero(got_b != got_s)} samples of a bank of equal rows differ from the shared handle's"


@pytest.mark.parametrize("precision,stages", [(32, 8), (64, 3)])
def test_bank_many_channels_default_tuning(dev, oracle, precision, stages):
    """2051 channels (the last workgroup of the tail kernel holds a partial set), no two sets equal, default tuning, two calls:
    every channel against the oracle with its own set"""
    channels, n = 2051, 16 * 1024 + 40
    coef = ib.many(precision, stages, channels)
    f = filters.IirBankMC(channels, coef)
    plan = f.plan(n)
    assert plan["precision"] == f.precision == precision and plan["warm"] >= ib.bank_warm(oracle, coef[:3]), plan
    mem = plan["warm"]                                           # (2051 probes would take minutes: the signal cases assert the warm-up)
    main = ic.main_samples(plan, n)
    marks = ic.marks_of(plan, main)
    rows = ib.rows_for(2 * n, marks + [(n + s, w) for s, w in marks], (mem + 1) * ic.CHUNK, sorted({main, n, n + main}))
    rows = {k: rows[k] for k in ("tone_res", "impulses", "burst", "zero")}
    x, names, base_of = ib.bank_input(rows, coef)
    x = kept(x, names, base_of, precision, stages)
    got = two_calls(f, x, n, dev)
    f.close()
    held(oracle, got, x, coef, precision, f"bank 2051 channels f{precision}", plan, n)


def test_bank_precision_and_warm_up_are_the_handles(dev, oracle):
    """one channel that needs double puts the whole handle in double; one channel whose probe gives 0 stops every split"""
    coef = ib.family32(8)
    coef[17] = ic.tiled(8, 0.99, 0.25)
    with capi.tuned(**WAVE):
        f = filters.IirBankMC(CHANNELS, coef)
        mem = ib.bank_warm(oracle, coef)
        n = smallest_split_frame(f.plan, None)
        plan = f.plan(n)
        assert f.precision == 64 and plan["precision"] == 64 and plan["warm"] == mem == ib.probe(oracle, coef[17])[0], plan
        x = signals_for(plan, n, mem, coef, 64)
        got = two_calls(f, x, n, dev)
        f.close()
        held(oracle, got, x, coef, 64, "bank with one high-Q channel", plan, n)
        coef[17] = ic.tiled(8, 0.99999, 0.25)
        assert ib.probe(oracle, coef[17])[0] == 0
        f = filters.IirBankMC(CHANNELS, coef)
        plan1 = f.plan(n)
        assert f.precision == 64 and plan1["segs"] == 1 and plan1["form"] == "pipe", plan1
        got = two_calls(f, x, n, dev)
        f.close()
    held(oracle, got, x, coef, 64, "bank with one channel that never decays", plan1, n)


@pytest.mark.parametrize("precision", [32, 64])
def test_bank_identity_padding(dev, oracle, precision):
    """channel c uses the family's first 1 + c mod 8 sections, then identity sections {1,0,0,1,0,0}: held to the oracle run with
    only the real sections"""
    coef = ib.family(precision, 8)
    real = [1 + c % 8 for c in range(CHANNELS)]
    for c in range(CHANNELS):
        coef[c, real[c]:] = ib.IDENTITY
    with capi.tuned(**WAVE):
        f = filters.IirBankMC(CHANNELS, coef)
        n = smallest_split_frame(f.plan, None)
        plan = f.plan(n)
        mem = plan["warm"]
        assert plan["form"] == FORM[precision] and f.precision == precision and mem >= 1, plan
        x = signals_for(plan, n, mem, coef, precision)
        got = two_calls(f, x, n, dev)
        f.close()
    held(oracle, got, x, coef, precision, f"bank identity padding f{precision}", plan, n, real=real)


def run_frames(f, x, n, dev, between=None):
    outs = []
    for k, o in enumerate((0, n)):
        if k == 1 and between:
            between()
        xi = torch.from_numpy(np.ascontiguousarray(x[:, o:o + n])).to(dev)
        yi = torch.empty_like(xi)
        f.filter(xi, yi)
        outs.append(yi.cpu().numpy())
    return outs


@pytest.mark.parametrize("precision", [32, 64])
def test_bank_set_coef(dev, oracle, precision):
    n = 2048 + 1024 + 40
    coef = ib.family(precision, 8)
    other = ib.family(precision, 8, shift=np.full(CHANNELS, 0.011))
    x = oracle.synth_f32(CHANNELS, 2 * n, seed=11)
    with capi.tuned(**dict(WAVE, iir_segs=1)):                   # one segment: the state handed over is the true one
        # (i) rewriting every channel with its own values changes nothing
        f, g = filters.IirBankMC(CHANNELS, coef), filters.IirBankMC(CHANNELS, coef)
        a = run_frames(f, x, n, dev)
        b = run_frames(g, x, n, dev, between=lambda: g.set_coef(0, coef))
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[0], b[0])
        f.close()
        g.close()
        # (ii) set_coef before the first call == a bank initialised with those values
        mixed = coef.copy()
        mixed[5:21] = other[5:21]
        f, g = filters.IirBankMC(CHANNELS, coef), filters.IirBankMC(CHANNELS, mixed)
        f.set_coef(5, other[5:21])
        a, b = run_frames(f, x, n, dev), run_frames(g, x, n, dev)
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b))
        f.close()
        g.close()
        # (iii) between two calls, the state kept: against the double recursion with carried state
        f = filters.IirBankMC(CHANNELS, coef)
        plan = f.plan(n)
        assert f.precision == precision and (plan["form"], plan["precision"], plan["segs"]) == (FORM[precision], precision, 1), plan
        got = run_frames(f, x, n, dev, between=lambda: f.set_coef(5, other[5:21]))
        assert f.precision == precision and f.plan(n) == plan
        f.close()
    y0, st, _ = ib.df1_carried(x[:, :n], coef)
    ref0, P0 = ib.per_channel_ref(oracle, x[:, :n], coef, 64)
    assert np.all(np.abs(y0 - ref0) <= 1e-12 * P0[:, None]), "the carried-state recursion is not the oracle's on the first frame"
    y1, _, P1 = ib.df1_carried(x[:, n:], mixed, st)
    report(f"bank set_coef f{precision}, first frame", plan, n, ic.local_checks(got[0], y0, x[:, :n], precision, "first frame", P=P0))
    report(f"bank set_coef f{precision}, second frame", plan, n, ic.local_checks(got[1], y1, x[:, n:], precision, "second frame", P=P1))


def test_bank_set_coef_flips_the_precision(dev, oracle):
    """channel 17 goes to a 0.99-radius set (the handle turns to double) and back (float32 again); precision follows, and the
    untouched channels stay within the limits of the precision each frame ran in: their state survived both rebuilds"""
    n = 2048 + 1024 + 40
    coef = ib.family32(8)
    high = coef.copy()
    high[17] = ic.tiled(8, 0.99, 0.25)
    x = oracle.synth_f32(CHANNELS, 3 * n, seed=12)
    with capi.tuned(**dict(WAVE, iir_segs=1)):
        f = filters.IirBankMC(CHANNELS, coef)
        outs, precs = [], []
        for k in range(3):
            if k:
                f.set_coef(17, (high if k == 1 else coef)[17:18])
            precs.append(f.precision)
            assert f.plan(n)["precision"] == precs[-1]
            xi = torch.from_numpy(np.ascontiguousarray(x[:, k * n:(k + 1) * n])).to(dev)
            yi = torch.empty_like(xi)
            f.filter(xi, yi)
            outs.append(yi.cpu().numpy())
        f.close()
    assert precs == [32, 64, 32], precs
    others = [c for c in range(CHANNELS) if c != 17]
    ref, _ = ib.per_channel_ref(oracle, x[others], coef[others], 32)
    for k, prec in enumerate(precs):
        sl = slice(k * n, (k + 1) * n)
        # a frame in double continues a state that float32 frames left: it is held to the float32 limits like them
        ic.local_checks(outs[k][others], ref[:, sl], x[others][:, sl], 32, f"precision flip, frame {k} in f{prec}")


@pytest.mark.parametrize("precision", [32, 64])
def test_bank_ragged_and_unaligned(dev, oracle, precision):
    """frame_len 1027: every sample goes through the tail kernel; and a device input at an odd element offset, which takes a
    whole-chunk frame away from the chunked kernels"""
    coef = ib.family(precision, 8)
    f = filters.IirBankMC(CHANNELS, coef)
    x = oracle.synth_f32(CHANNELS, 2 * 1027, seed=5)
    got = two_calls(f, x, 1027, dev)
    f.close()
    ref, P = ib.per_channel_ref(oracle, x, coef, precision)
    ic.local_checks(got, ref, x, precision, f"bank f{precision} frame_len 1027", P=P)
    n = 2048
    x = oracle.synth_f32(CHANNELS, n, seed=6)
    flat = torch.zeros(CHANNELS * n + 8, dtype=torch.float32, device=dev)
    xi = flat[1:1 + CHANNELS * n]
    assert xi.data_ptr() % 16 == 4
    xi.copy_(torch.from_numpy(x.reshape(-1)))
    y = torch.empty(CHANNELS, n, dtype=torch.float32, device=dev)
    f = filters.IirBankMC(CHANNELS, coef)
    capi.check(capi.lib().llz_iir_bank_mc(f.handle, C.c_void_p(xi.data_ptr()), C.c_void_p(y.data_ptr()), n), "llz_iir_bank_mc")
    got = y.cpu().numpy()
    f.close()
    ref, P = ib.per_channel_ref(oracle, x, coef, precision)
    ic.local_checks(got, ref, x, precision, f"bank f{precision} input at an odd element offset", P=P)


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("tunes", [WAVE, PIPE], ids=["wave16", "pipe"])
def test_bank_buffer_contract(dev, oracle, where, tunes):
    """5 channels x 3112 samples between sentinel / NaN bands, two calls: bands and input bit-unchanged, every output element
    written, the result the oracle's"""
    channels, n = 5, 3112
    coef = ib.family32(8, channels)
    x = oracle.synth_f32(channels, 2 * n, seed=9)
    io = tb.Io(dev if where == "device" else torch.device("cpu"), (4, 8))      # 16-byte aligned rows: the chunked kernels run
    with capi.tuned(**dict(tunes, iir_segs=1)):
        f = filters.IirBankMC(channels, coef)
        assert f.plan(n)["form"] == ("wave16" if tunes is WAVE else "pipe")
        ys = []
        for o in (0, n):
            y = io.out(torch.float32, channels, n)
            f.filter(io.inp(x[:, o:o + n]), y)
            ys.append(y)
        io.verify(f"iir bank {where}")
        f.close()
    for k, buf in enumerate(io.outs):
        bc.check_all_written(buf, f"iir bank {where}: output {k}")
    got = np.concatenate([tb.host(t) for t in ys], axis=1)
    ref, _ = ib.per_channel_ref(oracle, x, coef, 32)
    ic.local_checks(got, ref, x, 32, f"iir bank buffer contract, {where}")


def test_bank_overlap_refused(dev):
    L = capi.lib()
    for tune in ({}, {"iir_segs": 2, "iir_pipe": 1}):
        with capi.tuned(**tune):
            f = filters.IirBankMC(2, ib.family32(4, 2))
            tb.refused(bc.overlap_cases(2 * 16384, device=dev),
                       lambda a, b: L.llz_iir_bank_mc(f.handle, tb.dptr(a), tb.dptr(b), 16384), "llz_iir_bank_mc")
            f.close()


def test_bank_handle_refusals(dev, oracle):
    """a live bank handle: the shared handle's entry points refuse it (and the bank's refuse a shared handle); a set_coef range
    outside [0, channels) is refused with a message that names the function, and changes nothing: the next frame is
    bit-identical to an untouched handle's"""
    L = capi.lib()
    n = 2048 + 1024 + 40
    coef = ib.family32(3, 4)
    other = np.ascontiguousarray(ib.family32(3, 8)[4:])
    x = oracle.synth_f32(4, 2 * n, seed=13)
    out = (C.c_int * 5)()
    f, g = filters.IirBankMC(4, coef), filters.IirBankMC(4, coef)
    s = filters.IirCascadeMC(4, coef[0])
    assert L.llz_iir_cascade_mc_precision(f.handle) == ERR_ARG and L.llz_iir_cascade_mc_plan(f.handle, n, out) == ERR_ARG
    assert L.llz_iir_bank_mc_precision(s.handle) == ERR_ARG and "llz_iir_bank_mc_precision" in capi.last_error()
    assert L.llz_iir_bank_mc_set_coef(s.handle, 0, 1, other.ctypes.data) == ERR_ARG
    s.close()
    before = (f.precision, f.plan(n))

    def bad_ranges():
        for first, count in ((-1, 1), (4, 1), (3, 2), (0, 5), (0, 0), (2, -1), (2147483647, 2)):
            L.llz_hip_tune(b"no_such_override", 0)                  # leaves a message that is not set_coef's
            assert L.llz_iir_bank_mc_set_coef(f.handle, first, count, other.ctypes.data) == ERR_ARG, (first, count)
            assert "llz_iir_bank_mc_set_coef" in capi.last_error(), capi.last_error()
        assert L.llz_iir_bank_mc_set_coef(f.handle, 0, 1, None) == ERR_ARG and "llz_iir_bank_mc_set_coef" in capi.last_error()
    a = run_frames(f, x, n, dev, between=bad_ranges)
    b = run_frames(g, x, n, dev)
    assert (f.precision, f.plan(n)) == before
    assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b)), "a refused set_coef changed the handle"
    f.set_coef(1, other[:3])                                     # the last valid range: channels 1..3
    f.close()
    g.close()
