"""The checks of tests/transform_checks.py, tested on the CPU: the plain float32 models stay within a quarter of every derived
limit on every (transform, size, row kind) that tests/test_transform_signals_gpu.py uses and pass every new check and the old
pooled gate; every planted fault passes the pooled gate and fails a new check."""
import numpy as np
import pytest

from tests import transform_checks as tc

QUARTER = 0.25


def _fft(oracle):
    return lambda z, inverse: oracle.fft(z, inverse=inverse)


def _quarter(transform, worst):
    for kind, v in worst.items():
        if (transform, kind) in tc.F32_DROPPED:
            continue
        assert v <= QUARTER, f"{transform}, {kind} rows: plain float32 takes {v:.3g} of the limit"
    print(f"{transform}: plain float32, worst fraction of the limit by row kind: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_nothing_dropped_beyond_the_cap():
    per = {}
    for transform, kind in tc.F32_DROPPED:
        assert kind not in ("imp", "impulses", "scaled", "noise_scaled"), "the impulse rows and the scaled rows may never be dropped"
        per.setdefault(transform, set()).add(kind)
    assert all(len(v) <= 1 for v in per.values()), "at most one row kind per transform"


def test_rows_of_a_batch_are_all_different():
    for n, generic in tc.FFT_CASES:
        count = tc.fft_count(n, generic)
        specs = tc.fft_specs(n, count, tc.fft_group(n, generic)[0])
        assert len(specs) % count == 0 and len(set(specs)) == len(specs), n
        if n <= 4096:
            x = tc.make_rows(n, specs)
            assert len({row.tobytes() for row in x}) == len(x), f"{n}: two rows alike"
        e = [s[2] for s in specs if s[0] == "scaled"]
        assert min(e) == -20 and max(e) == 10 and abs(e.index(-20) - e.index(10)) == 1
        assert specs[-2][2:] == (-19,) and specs[-1][2:] == (-20,) and specs[-1][1] == specs[-2][1]


# ------------------------------------------------------------------------------------------------ the models within the limits
@pytest.mark.parametrize("n,generic", tc.FFT_CASES)
def test_fft_plain_f32_within_a_quarter_and_passes_every_check(oracle, n, generic):
    count = tc.fft_count(n, generic)
    specs = tc.fft_specs(n, count, tc.fft_group(n, generic)[0], lean=n > 4096)
    x = tc.make_rows(n, specs)
    base_of, exps = tc.scaled_pairs(specs)
    for inverse in (False, True):
        got = tc.plain_f32_fft(x, inverse)
        ref = tc.fft_reference(_fft(oracle), n, specs, x, inverse)
        lim = tc.fft_limit(x, n, inverse)
        _quarter(f"fft {n} {'inverse' if inverse else 'forward'}", tc.worst_by_kind(specs, got, ref, lim))
        tc.limit_check(got, ref, lim, f"fft {n}")
        tc.scaled_equal(got, base_of, exps, f"fft {n}")
        tc.zero_where_silent(got, ~np.any(x != 0, axis=1)[:, None], f"fft {n}")
        assert tc.pooled_rms_passes(got, ref, fft=True)


def _stft_case(oracle, fft_len, hint, which):
    F = fft_len >> (2 if hint == 0 else 1)
    win = tc.stft_window(fft_len, hint)
    T = tc.frames_total(fft_len)
    calls = tc.frame_calls(which, T)
    x, base_of, exps, names, info = tc.frame_channels(which, F, fft_len, calls)
    w = oracle.window(win, fft_len)
    ref = tc.stft_analysis_ref(oracle, x, base_of, hint, F, win)
    return F, win, calls, x, base_of, exps, names, info, w, ref


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("hint", [0, 1])
@pytest.mark.parametrize("fft_len", sorted({n for n, _ in tc.STFT_CASES}))
def test_stft_plain_f32_within_a_quarter_and_passes_every_check(oracle, fft_len, hint, which):
    N = fft_len
    F, win, calls, x, base_of, exps, names, info, w, ref = _stft_case(oracle, N, hint, which)
    got = tc.plain_f32_stft_analysis(x, w, F, N)
    lim = tc.stft_analysis_limit(x, w, F, N)
    worst = {}
    for c, name in enumerate(names):
        worst[name] = max(worst.get(name, 0.0), tc.limit_check(got[c], ref[c], lim[c], "", check=False))
    _quarter(f"stft analysis {N} hint {hint}", worst)
    tc.limit_check(got, ref, lim, "stft analysis")
    tc.scaled_equal(got, base_of, exps, "stft analysis")
    assert tc.zero_where_silent(got, tc.silent_frames(x, F, N), "stft analysis") > 0 or tc.frames_total(N) < 17
    tc.zero_where_ref_zero(got.imag[:, :, [0, N // 2]], ref.imag[:, :, [0, N // 2]], "stft analysis, bins 0 and N/2")
    centre = tc.centre_frames(x, F, N)
    assert centre or tc.frames_total(N) < 41
    for c, f in centre:
        assert not np.any(ref[c, f].imag), "an impulse at the window centre has a real spectrum in the oracle"
        tc.zero_where_ref_zero(got[c, f].imag, ref[c, f].imag, "stft analysis, impulse at the window centre")
    assert tc.pooled_rms_passes(got, ref)
    S32 = ref.astype(np.complex64)
    for half in sorted({tc.stft_half(n, t) for n, t in tc.STFT_CASES if n == N}):
        out = tc.plain_f32_stft_synthesis(S32, w, hint, F, N)
        ref_x = tc.stft_synthesis_ref(oracle, S32, base_of, hint, F, win)
        lim_x = tc.stft_synthesis_limit(S32, w, hint, F, N, half)
        worst = {}
        for c, name in enumerate(names):
            worst[name] = max(worst.get(name, 0.0), tc.limit_check(out[c], ref_x[c], lim_x[c], "", check=False))
        _quarter(f"stft synthesis {N} hint {hint}", worst)
        tc.limit_check(out, ref_x, lim_x, "stft synthesis")
        tc.scaled_equal(out, base_of, exps, "stft synthesis")
        assert tc.zero_where_silent(out, tc.silent_samples(S32, F, N), "stft synthesis") > 0 or tc.frames_total(N) < 17
        assert tc.pooled_rms_passes(out, ref_x)


@pytest.mark.parametrize("n", tc.MDCT_SIZES)
def test_mdct_plain_f32_within_a_quarter_and_passes_every_check(oracle, n):
    count = tc.mdct_count(n)
    for inverse in (False, True):
        m = n // 2 if inverse else n
        specs = tc.fft_specs(m, count, tc.MDCT_E.get(n))
        x = tc.make_rows(m, specs, real=True)
        base_of, exps = tc.scaled_pairs(specs)
        if inverse:
            got, ref = tc.plain_f32_imdct(x), tc.real_reference(lambda r: oracle.imdct(2, r), specs, x, n)
            lim = tc.imdct_limit(x, n)
        else:
            got, ref = tc.plain_f32_mdct(x), tc.real_reference(lambda r: oracle.mdct(2, r), specs, x, n // 2)
            lim = tc.mdct_limit(x, n)
        _quarter(f"mdct {n} {'inverse' if inverse else 'forward'}", tc.worst_by_kind(specs, got, ref, lim))
        tc.limit_check(got, ref, lim, f"mdct {n}")
        tc.scaled_equal(got, base_of, exps, f"mdct {n}")
        tc.zero_where_silent(got, ~np.any(x != 0, axis=1)[:, None], f"mdct {n}")
        assert tc.pooled_rms_passes(got, ref)


def _mdct_frames_case(oracle, F, win, which):
    T = tc.frames_total(2 * F)
    calls = tc.frame_calls(which, T)
    x, base_of, exps, names, info = tc.frame_channels(which, F, 2 * F, calls)
    w = oracle.mdct_window(win, 2 * F)
    ref = tc.mdct_frames_analysis_ref(oracle, x, base_of, F, win)
    return calls, x, base_of, exps, names, info, w, ref


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("F,win", sorted({(F, win) for F, win, _ in tc.MDCT_FRAME_CASES}))
def test_mdct_frames_plain_f32_within_a_quarter_and_passes_every_check(oracle, F, win, which):
    calls, x, base_of, exps, names, info, w, ref = _mdct_frames_case(oracle, F, win, which)
    got = tc.plain_f32_mdct_frames_analysis(x, w, F)
    lim = tc.mdct_frames_analysis_limit(x, w, F)
    worst = {}
    for c, name in enumerate(names):
        worst[name] = max(worst.get(name, 0.0), tc.limit_check(got[c], ref[c], lim[c], "", check=False))
    _quarter(f"mdct frames analysis {F}", worst)
    tc.limit_check(got, ref, lim, "mdct frames analysis")
    tc.scaled_equal(got, base_of, exps, "mdct frames analysis")
    assert tc.zero_where_silent(got, tc.silent_frames(x, F, 2 * F), "mdct frames analysis") > 0
    assert tc.pooled_rms_passes(got, ref)
    X32 = ref.astype(np.float32)
    out = tc.plain_f32_mdct_frames_synthesis(X32, w, F)
    ref_x = tc.mdct_frames_synthesis_ref(oracle, X32, base_of, w, F)
    lim_x = tc.mdct_frames_synthesis_limit(X32, w, F)
    worst = {}
    for c, name in enumerate(names):
        worst[name] = max(worst.get(name, 0.0), tc.limit_check(out[c], ref_x[c], lim_x[c], "", check=False))
    _quarter(f"mdct frames synthesis {F}", worst)
    tc.limit_check(out, ref_x, lim_x, "mdct frames synthesis")
    tc.scaled_equal(out, base_of, exps, "mdct frames synthesis")
    assert tc.zero_where_silent(out, tc.silent_samples(X32, F, 2 * F), "mdct frames synthesis") > 0
    assert tc.pooled_rms_passes(out, ref_x)


def test_synthesis_reference_is_the_oracles_streaming_one(oracle):
    """the per-frame double IMDCT with the window and the two-term overlap-add, which the synthesis limit needs frame by
    frame, is the oracle's own streaming synthesis"""
    F = 128
    x = tc.noise_row(6 * F, 9, real=True)
    X, y = oracle.mdct_frames(F, 0, x.astype(np.float64))
    mine = tc.mdct_frames_synthesis_ref(oracle, X[None], np.array([0]), oracle.mdct_window(0, 2 * F), F)[0]
    assert np.abs(mine - y).max() <= 1e-13


# ------------------------------------------------------------------------------------------------ planted faults
def _fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def _fft_batch(oracle, n, inverse=False, lean=False):
    specs = tc.fft_specs(n, tc.fft_count(n), tc.fft_group(n)[0], lean=lean)
    x = tc.make_rows(n, specs)
    return specs, x, tc.fft_reference(_fft(oracle), n, specs, x, inverse), tc.fft_limit(x, n, inverse), tc.scaled_pairs(specs)


@pytest.mark.parametrize("n", [4096, 32768])
def test_fault_twiddle_index_off_by_one_in_one_butterfly_group(oracle, n):
    """Span 16, the last group, whose difference outputs carry the tone at bin N - 1 (that bin turns by 2 pi / N) and 16 bins
    of a noise row.  Planted in one transform of the batch, since the pooled gate of the FFT batch is 1e-6 relative: on a
    noise row the fault is 2 pi / N sqrt(h / N) of the row's RMS (h = 8 the group's half span: 6.8e-5 at 4096 points, 3.0e-6
    at 32768), which that gate sees once every row of a one-scale batch carries it.  Beside the loud rows of these batches
    it does not: at 4096 points the unit-scale noise row hides it from the pooled gate and the per-bin limit finds it (the
    tone's 2 pi of absolute error is 1.7e-6 of this batch, just visible); at 32768 points an l1 limit is too loose on noise
    (0.02 against 0.12) and the tone row finds it.  The quiet copy finds it at both sizes, by scaled_equal."""
    specs, x, ref, lim, (base_of, exps) = _fft_batch(oracle, n, lean=n > 4096)
    stage, group = tc.log2i(n) - 4, n // 16 - 1
    row = specs.index(("noise", 1) if n == 4096 else ("tone", n - 1))
    got = tc.plain_f32_fft(x, fault={"stage": stage, "group": group, "rows": [row]})
    assert tc.pooled_rms_passes(got, ref, fft=True)
    _fails(tc.limit_check, got, ref, lim, "twiddle fault")
    quiet = specs.index(("scaled", specs.index(("noise", 1)), -20))
    got = tc.plain_f32_fft(x, fault={"stage": stage, "group": group, "rows": [quiet]})
    assert tc.pooled_rms_passes(got, ref, fft=True)
    _fails(tc.scaled_equal, got, base_of, exps, "twiddle fault, quiet row")


def test_faults_on_rows_of_an_fft_batch(oracle):
    n = 256
    specs, x, ref, lim, (base_of, exps) = _fft_batch(oracle, n)
    good = tc.plain_f32_fft(x)
    last = len(specs) - 1
    quiet = specs.index(("scaled", specs.index(("noise", 1)), -20))
    tone = specs.index(("tone", 1))

    def swapped(g):                     # the scaled copies at 2^-19 and 2^-20 of one base
        g[[last - 1, last]] = g[[last, last - 1]]

    def zeroed(g):                      # the quiet row
        g[quiet] = 0

    def leak(g):                        # an empty bin of a tone row filled with 1e-4 of the peak
        g[tone, 9] += 1e-4 * n

    def stale(g):                       # the partial workgroup's row left holding the row before
        g[last] = g[last - 1]

    for plant, checks in ((swapped, "s"), (zeroed, "ls"), (leak, "l"), (stale, "ls")):
        got = good.copy()
        plant(got)
        assert tc.pooled_rms_passes(got, ref, fft=True), plant.__name__
        if "l" in checks:
            _fails(tc.limit_check, got, ref, lim, plant.__name__)
        if "s" in checks:
            _fails(tc.scaled_equal, got, base_of, exps, plant.__name__)


def test_fault_inverse_without_its_scale_on_one_row(oracle):
    n = 64
    specs, x, ref, lim, (base_of, exps) = _fft_batch(oracle, n, inverse=True)
    quiet = specs.index(("scaled", specs.index(("noise", 1)), -20))
    got = tc.plain_f32_fft(x, inverse=True, unscaled_rows=[quiet])
    assert tc.pooled_rms_passes(got, ref, fft=True)
    _fails(tc.limit_check, got, ref, lim, "no 1/N")
    _fails(tc.scaled_equal, got, base_of, exps, "no 1/N")


def test_fault_stft_history_from_the_neighbouring_channel(oracle):
    """channels "a", two calls of 40 frames and 1: the quiet channel's last frame sees channel 0's history, which is silent there"""
    N, hint = 256, 0
    F, win, calls, x, base_of, exps, names, info, w, ref = _stft_case(oracle, N, hint, "a")
    got = tc.plain_f32_stft_analysis(x, w, F, N, calls, history_from=(info["quiet"], 0))
    assert tc.pooled_rms_passes(got, ref)
    _fails(tc.limit_check, got, ref, tc.stft_analysis_limit(x, w, F, N), "history")
    _fails(tc.scaled_equal, got, base_of, exps, "history")


def test_fault_stft_bin_from_the_frame_before(oracle):
    """channels "b", the tone channel (2^-3), three bins beside the tone's peak (at the peak itself the pooled gate sees it)"""
    N, hint = 256, 0
    F, win, calls, x, base_of, exps, names, info, w, ref = _stft_case(oracle, N, hint, "b")
    got = tc.plain_f32_stft_analysis(x, w, F, N)
    c, f, b = names.index("tone"), 17, N // 8 + 1 + 3
    got[c, f, b] = got[c, f - 1, b]
    assert tc.pooled_rms_passes(got, ref)
    _fails(tc.limit_check, got, ref, tc.stft_analysis_limit(x, w, F, N), "stale bin")


def test_fault_mdct_frames_tail_of_the_one_frame_channel_dropped(oracle):
    """channels "b": the one frame is the first call's only frame, so its tail is what the handle carries; planted on the 2^-20 copy"""
    F, win = 128, 0
    calls, x, base_of, exps, names, info, w, ref = _mdct_frames_case(oracle, F, win, "b")
    X32 = ref.astype(np.float32)
    c = info["quiet"]
    assert names[c] == "oneframe" and info["oneframe"] == calls[0] - 1
    got = tc.plain_f32_mdct_frames_synthesis(X32, w, F, drop_tail=(c, info["oneframe"]))
    ref_x = tc.mdct_frames_synthesis_ref(oracle, X32, base_of, w, F)
    assert tc.pooled_rms_passes(got, ref_x)
    _fails(tc.limit_check, got, ref_x, tc.mdct_frames_synthesis_limit(X32, w, F), "tail")
    _fails(tc.scaled_equal, got, base_of, exps, "tail")
