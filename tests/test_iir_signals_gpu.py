"""The batch IIR forms on steps, tones, impulses and bursts: every channel, every sample, every chunk (tests/iir_checks.py).

Each case selects one kernel form by its tunes and ASSERTS through IirCascadeMC.plan() that this form ran, split at least three
ways along time.  37 channels carry every signal row at a different power-of-two amplitude; the frame is the smallest of whole
2048-sample chunks + one 1024-sample chunk + 40 samples that the plan splits; two calls, so the chunked kernels, the ragged
tail kernel and the hand-over between calls all take part.  The impulses sit where the plan puts the segment edges.

Held: a zero row gives exactly zero; a channel equals its base channel times 2^e bit for bit (float32 forms: where no section
works within 2^48 of the subnormals, iir_checks.scaled_equal); every sample (double forms) or
every sample and every 1024-sample chunk (float32 forms) is within the derived limit of the double oracle.  Each case prints
its form, its segment count and its worst ratio to the limit (IIR section, has the table).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import iir_checks as ic  # noqa: E402

CHANNELS = 37
WAVE = {"iir_wave_min_items": 0}
WAVE16 = {"iir_wave_min_items": 0, "iir_unpacked": 2}
PIPE = {"iir_pipe": 1}

# id, cascade, tunes, the form and precision that must run, forced segment count (None: the library's own, at least 3)
CASES = [
    ("pipe-f32", "8x(0.44,1.1)", PIPE, "pipe", 32, None),
    ("pipe-f32-unpacked-count", "distinct5", PIPE, "pipe", 32, None),
    ("pipe-f64", "4x(0.99-0.02k)", PIPE, "pipe", 64, None),
    ("pipe-f64-default-tuning", "fixture mix", {}, "pipe", 64, None),
    ("wave16-f32-packed", "distinct8", WAVE16, "wave16", 32, None),
    ("wave16-f32-unpacked", "distinct5", WAVE16, "wave16", 32, None),
    ("wave16-f32-high-q", "2x(0.95,1.0)", WAVE16, "wave16", 32, None),
    ("wave32-f32-packed", "8x(0.44,1.1)", WAVE, "wave32", 32, None),
    ("wave32-f32-packed-distinct", "distinct8", WAVE, "wave32", 32, None),
    ("wave32-f32-unpacked", "3x(0.7,0.5)", WAVE, "wave32", 32, None),
    ("wave16-f64", "highq3", WAVE16, "wave16", 64, None),
    ("wave16-f64-packed-count", "highq8", WAVE16, "wave16", 64, None),
    ("wave32-f64", "highq8", WAVE, "wave32", 64, None),
    ("wave32-f64-unpacked-count", "highq3", WAVE, "wave32", 64, None),
    ("wave32-f64-forced-precision", "2x(0.95,1.0)", dict(WAVE, iir_f64=1), "wave32", 64, None),
    ("pipe-f64-forced-precision", "8x(0.44,1.1)", dict(PIPE, iir_f64=1), "pipe", 64, None),
    ("pipe-f32-3-segments", "3x(0.7,0.5)", dict(PIPE, iir_segs=3), "pipe", 32, 3),
    ("wave16-f32-5-segments", "distinct8", dict(WAVE16, iir_segs=5), "wave16", 32, 5),
    ("wave32-f32-3-segments", "8x(0.44,1.1)", dict(WAVE, iir_segs=3), "wave32", 32, 3),
    ("wave32-f64-5-segments", "4x(0.99-0.02k)", dict(WAVE, iir_segs=5), "wave32", 64, 5),
    ("pipe-f64-5-segments", "fixture mix", dict(PIPE, iir_segs=5), "pipe", 64, 5),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def cascade(name):
    return ic.F32_CASCADES[name] if name in ic.F32_CASCADES else ic.F64_CASCADES[name]


def smallest_split_frame(plan_of, want):
    """the smallest frame of whole 2048-sample chunks + 1024 + 40 samples that runs as `want` segments (or, with want None,
    as at least 3)"""
    for k in range(1, 2000):
        n = 2048 * k + 1024 + 40
        segs = plan_of(n)["segs"]
        if segs == want or (want is None and segs >= 3):
            return n
    raise AssertionError(f"no frame up to 2000 x 2048 samples splits ({want})")


def two_calls(f, x, n, dev):
    outs = []
    for o in (0, n):
        xi = torch.from_numpy(np.ascontiguousarray(x[:, o:o + n])).to(dev)
        yi = torch.empty_like(xi)
        f.filter(xi, yi)
        outs.append(yi.cpu().numpy())
    return np.concatenate(outs, axis=1)


def report(what, plan, n, ratios, unit="chunks"):
    print(f"IIR-RATIO | {what} | {plan['form']} | {plan['precision']} | {plan['segs']} x {plan['seg_chunks']} {unit}, warm {plan['warm']} | "
          f"n {n} | " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


@pytest.mark.parametrize("case,name,tunes,form,precision,forced", CASES, ids=[c[0] for c in CASES])
def test_iir_cascade_forms_on_signals(dev, oracle, case, name, tunes, form, precision, forced):
    coef = cascade(name)
    mem, _, _ = ic.homogeneous_probe(oracle, coef)
    with capi.tuned(**tunes):
        f = filters.IirCascadeMC(CHANNELS, coef)
        n = smallest_split_frame(f.plan, forced)
        plan = f.plan(n)
        # the form the case is about ran, in the precision it is about, split as meant, warmed up over the probed memory
        assert (plan["form"], plan["precision"], f.precision) == (form, precision, precision), (case, plan)
        assert plan["segs"] == forced if forced else plan["segs"] >= 3, (case, plan)
        assert plan["warm"] == -(-mem * ic.CHUNK // plan["chunk"]) and plan["seg_chunks"] >= plan["warm"], (case, plan, mem)
        main = ic.main_samples(plan, n)
        assert main == (n - 40 if form != "wave32" else n - 1064)
        marks = ic.marks_of(plan, main)
        assert len(marks) == plan["segs"] - 1
        marks = marks + [(n + s, w) for s, w in marks]                          # the second call splits the same way
        joins = sorted({main, n - 40, n, n + main, 2 * n - 40})                   # kernel to kernel, call to call
        rows = ic.kept_rows(name, ic.signals(2 * n, ic.pole_angle(coef), marks, gap=(mem + 1) * ic.CHUNK, joins=joins))
        x, base_of, exps, _ = ic.scaled_input(rows, CHANNELS)
        got = two_calls(f, x, n, dev)
        f.close()
    seg_len = plan["seg_chunks"] * plan["chunk"]
    what = f"{case}: {name}"
    ic.assert_zero_rows(got, x, what)
    bases = len(rows)
    floor = ic.stage_floor(oracle, x[:bases], coef) if precision == 32 else None
    assert ic.scaled_equal(got, base_of, exps, what, floor) > 2 * (CHANNELS - bases) * n // 3   # over a third of all samples were comparable
    if precision == 64:
        ref, P = ic.section_peaks(oracle, x, coef)
    else:
        ref, P = oracle.iir_cascade_batch_f32(x, coef), None
    report(what, plan, n, ic.local_checks(got, ref, x, precision, what, seg_len, P=P))


@pytest.mark.parametrize("name,chunks,precision", [("8x(0.44,1.1)", 16, 32), ("4x(0.99-0.02k)", 32, 64)])
def test_iir_cascade_many_channels_covariance(dev, oracle, name, chunks, precision):
    """the many-channel wave path at the default tuning, 2051 channels (the last workgroup holds a partial set of items):
    channel c carries base row c mod 4 times 2^e_c and must equal its base channel's output times 2^e_c bit for bit, at
    every sample of two calls; the four base channels are held to the oracle"""
    channels, n = 2051, 1024 * chunks + 40
    coef = cascade(name)
    mem, _, _ = ic.homogeneous_probe(oracle, coef)
    f = filters.IirCascadeMC(channels, coef)
    plan = f.plan(n)
    assert plan["form"] == "wave32" and plan["precision"] == precision and (channels * plan["segs"]) % 4 != 0, plan
    main = ic.main_samples(plan, n)
    marks = ic.marks_of(plan, main)
    rows = ic.signals(2 * n, ic.pole_angle(coef), marks + [(n + s, w) for s, w in marks], gap=(mem + 1) * ic.CHUNK,
                      joins=sorted({main, n - 40, n, n + main, 2 * n - 40}))
    rows = {k: rows[k] for k in ("dc", "tone_res", "impulses", "burst")}
    x, base_of, exps, _ = ic.scaled_input(rows, channels)
    got = two_calls(f, x, n, dev)
    f.close()
    what = f"2051 channels: {name}"
    floor = ic.stage_floor(oracle, x[:4], coef) if precision == 32 else None
    assert ic.scaled_equal(got, base_of, exps, what, floor) > 2047 * n           # more than half of all samples were comparable
    if precision == 64:
        ref, P = ic.section_peaks(oracle, x[:4], coef)
    else:
        ref, P = oracle.iir_cascade_batch_f32(x[:4], coef), None
    report(what, plan, n, ic.local_checks(got[:4], ref, x[:4], precision, what, plan["seg_chunks"] * plan["chunk"], P=P))


# ------------------------------------------------------------------------------------------------ general direct form
@pytest.mark.parametrize("a,b", [
    ([1.0, -0.3695, 0.1958, 0.0], [1.0, 0.2066, 0.4131, 0.2066]),        # the reference's own order-3 call
    ([1.0, -1.8 * 0.99 * 0.95, 0.99 * 0.99], [0.01]),                     # pole radius 0.99: long memory
])
def test_iir_mc_on_signals(dev, oracle, a, b):
    """llz_iir_mc_* on the same signals, 37 channels, two calls + flush, every channel and sample: (1) iir_segs = 1 is the
    oracle's llz_iir_filter sequence rounded once, bit for bit; (2) the default launch, asserted to split at least three
    ways, within the double limit per sample and the float32 limits per sample and chunk, and exact under power-of-two
    scaling.  The frame length is odd, so no segment starts on a 4-sample boundary."""
    N = len(b) - 1
    warm = ic.df1_memory(a) + N                                           # the library's warm-up, restated
    theta = float(np.arccos(-a[1] / (2 * np.sqrt(a[2]))))
    f = filters.IirMC(CHANNELS, a, b)
    n = next(m for m in range(45, 1 << 20, 8) if f.segments(m) >= 3)
    segs = f.segments(n)
    f.close()
    seg_len = -(-n // segs)
    assert seg_len >= 8 * warm, (n, segs, warm)
    marks = [(k * seg_len, warm) for k in range(1, segs)]
    rows = ic.signals(2 * n, theta, marks + [(n + s, w) for s, w in marks], gap=warm + 64, joins=[n])
    x, base_of, exps, _ = ic.scaled_input(rows, CHANNELS)
    streams = [oracle.iir_stream(np.array(a), np.array(b), x[c].astype(np.float64), flush=True) for c in range(CHANNELS)]
    ref = np.stack([np.concatenate(s) for s in streams])
    xz = np.concatenate([x, np.zeros((CHANNELS, ref.shape[1] - 2 * n), dtype=np.float32)], axis=1)
    P = np.maximum(np.abs(x).max(axis=1), np.abs(ref).max(axis=1))
    xd = torch.from_numpy(x).to(dev)
    for tune in (1, -1):
        with capi.tuned(iir_segs=tune):
            f = filters.IirMC(CHANNELS, a, b)
            assert f.segments(n) == (1 if tune == 1 else segs)
            outs = []
            for o in (0, n):
                y = torch.empty(CHANNELS, n, dtype=torch.float32, device=dev)
                f.filter(xd[:, o:o + n].contiguous(), y)
                outs.append(y.cpu().numpy())
            tail = np.zeros((CHANNELS, max(N, 1)), dtype=np.float32)
            assert f.flush(tail) == N
            f.close()
        got = np.concatenate(outs + ([tail[:, :N]] if N else []), axis=1)
        what = f"iir_mc M={len(a) - 1} N={N}, {'one segment' if tune == 1 else f'{segs} segments'}"
        ic.assert_zero_rows(got, xz, what)
        ic.scaled_equal(got, base_of, exps, what)
        if tune == 1:
            assert np.array_equal(got, ref.astype(np.float32)), what
            continue
        ratios = {"sample64": ic.sample_check(got, ref, ic.f64_sample_limit(ref, P), what, seg_len)}
        ratios.update(ic.local_checks(got, ref, x, 32, what, seg_len))
        report(what, {"form": "df1", "precision": 64, "segs": segs, "seg_chunks": seg_len, "warm": warm}, n, ratios, unit="samples")
