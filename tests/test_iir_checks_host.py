"""CPU self-test of tests/iir_checks.py: the conditions its limits rest on hold for every cascade used, and the limits catch
faults planted in a model of the time split -- three of which the old pooled RMS gate lets through.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from llzlab_amd import capi
from tests import iir_checks as ic

N_SEG = 4096


@pytest.fixture(scope="module")
def split(oracle):
    """37 channels of every signal row at different power-of-two amplitudes through 8 x (0.44, 1.1), three segments of 4096
    samples + 40, the later two warmed up over the cascade's probed memory: (x, layout, marks, ref, P, honest model)"""
    coef = ic.F32_CASCADES["8x(0.44,1.1)"]
    mem, peak, _ = ic.homogeneous_probe(oracle, coef)
    assert 1 <= mem <= 3, (mem, peak)
    marks = [(N_SEG, mem * ic.CHUNK), (2 * N_SEG, mem * ic.CHUNK)]
    n = 3 * N_SEG + 40
    rows = ic.signals(n, ic.pole_angle(coef), marks, gap=(mem + 1) * ic.CHUNK)
    x, base_of, exps, names = ic.scaled_input(rows, 37)
    ref, P = ic.section_peaks(oracle, x, coef)
    model = ic.split_model(oracle, x, coef, marks)
    return {"coef": coef, "x": x, "base_of": base_of, "exps": exps, "names": names, "marks": marks, "ref": ref, "P": P,
            "model": model}


def new_checks(got, s, what):
    """every new check, under the limits of both precisions (the model is double arithmetic, rounded once)"""
    ic.assert_zero_rows(got, s["x"], what)
    ic.scaled_equal(got, s["base_of"], s["exps"], what)
    ic.local_checks(got, s["ref"], s["x"], 64, what, N_SEG, P=s["P"])
    ic.local_checks(got, s["ref"], s["x"], 32, what, N_SEG)


def fails_each(got, s, what, precisions=(32, 64)):
    """the fault is caught under the limits of each precision on their own"""
    for prec in precisions:
        with pytest.raises(AssertionError):
            ic.local_checks(got, s["ref"], s["x"], prec, f"{what}, limits of {prec}", N_SEG, P=s["P"])


@pytest.mark.parametrize("name", list(ic.F32_CASCADES))
def test_plain_float32_takes_a_quarter_of_the_float32_limits(oracle, name):
    """the condition on the float32 limits: the plain sequential float32 recursion stays at or below a quarter of the
    per-chunk and the per-sample limit on every (cascade, signal) pair used"""
    coef = ic.F32_CASCADES[name]
    n = 8192
    rows = ic.kept_rows(name, ic.signals(n, ic.pole_angle(coef), [(4096, 1024)], gap=3072))
    x = np.stack(list(rows.values()))
    ref = oracle.iir_cascade_batch_f32(x, coef)
    got = ic.plain_f32(x, coef)
    for c, sig in enumerate(rows):
        r = ic.local_checks(got[c:c + 1], ref[c:c + 1], x[c:c + 1], 32, f"plain float32, {name}, {sig}")
        assert r["chunk"] <= 0.25 and r["sample"] <= 0.25, (name, sig, r)


@pytest.mark.parametrize("name", list(ic.F64_CASCADES))
def test_warm_up_residue_of_the_double_cascades(oracle, name):
    """the 1e-9 P_c term of the double limit takes a homogeneous-response peak of at most 1e3 (a residue of 1e-10 per unit of
    state after a warm-up that ends 13 decades below the peak).  highq8 peaks at 9.9e3 (its gains 0.7 .. 2.1 multiply along
    eight resonant sections), so the residue itself is held as well, for every cascade: at most 1e-11 per unit of state
    after the probed memory, which keeps 2 x 16 sections x 1e-11 at a third of 1e-9"""
    mem, peak, residue = ic.homogeneous_probe(oracle, ic.F64_CASCADES[name])
    print(f"{name}: memory {mem} chunks, homogeneous peak {peak:.3g}, residue after the memory {residue:.3g}")
    assert 1 <= mem <= 62 and residue <= 1e-11, (name, mem, residue)
    if name == "highq8":
        assert 1e3 < peak <= 1e4, peak          # on record: the one cascade over 1e3
    else:
        assert peak <= 1e3, (name, peak)


def test_impulses_sit_at_every_segment_edge():
    marks = [(10240, 2048), (20480, 2048), (30720, 2048)]
    a, b = ic.impulse_positions(40000, marks)
    both = set(a.tolist()) | set(b.tolist())
    for s, w in marks:
        assert {s - w - 1, s - w, s - 1, s} <= both, (s, w)
    for r in (a, b):
        assert np.all(np.diff(r) >= 64)
    assert ic.marks_of({"segs": 4, "seg_chunks": 5, "chunk": 2048, "warm": 1}, 20 * 2048) == marks
    # the last segment of a plan may be short or, rounded away, absent
    assert ic.marks_of({"segs": 3, "seg_chunks": 5, "chunk": 1024, "warm": 2}, 10 * 1024) == [(5120, 2048)]


def test_honest_split_passes_every_check(split):
    new_checks(split["model"], split, "honest model")
    assert ic.pooled_rms_passes(split["model"], split["ref"])


def test_segment_started_from_zero_without_warm_up_is_caught(oracle, split):
    got = ic.split_model(oracle, split["x"], split["coef"], split["marks"], fault="no_warm")
    fails_each(got, split, "no warm-up")


def test_warm_up_one_sample_late_is_caught(oracle, split):
    """The impulse at s - w is the first sample a later segment sees.  With the probed warm-up its response has decayed
    13 decades by s, so to show that the row catches a lost sample the model's warm-up is cut to 16 samples: the row that
    holds s - w (and not s - w - 1) is then exact with the honest split and wrong with the late one; the other row, which
    holds s - w - 1, exposes the short warm-up itself."""
    coef = split["coef"]
    n = 2 * N_SEG
    for w, late_caught in ((16, True), (split["marks"][0][1], False)):
        marks = [(N_SEG, w)]
        rows = ic.signals(n, 1.1, marks, gap=3072)
        assert rows["impulses"][N_SEG - w - 1] == 1 and rows["impulses_alt"][N_SEG - w] == 1
        x = np.stack([rows["impulses"], rows["impulses_alt"]])
        ref, P = ic.section_peaks(oracle, x, coef)
        honest = ic.split_model(oracle, x, coef, marks)
        late = ic.split_model(oracle, x, coef, marks, fault="late")

        def check(got, row, what):
            ic.local_checks(got[row:row + 1], ref[row:row + 1], x[row:row + 1], 64, what, N_SEG, P=P[row:row + 1])
            ic.local_checks(got[row:row + 1], ref[row:row + 1], x[row:row + 1], 32, what, N_SEG)

        check(honest, 1, f"warm-up {w}: honest split, row with s - w")
        if late_caught:
            with pytest.raises(AssertionError):
                check(late, 1, f"warm-up {w}: late split, row with s - w")
            with pytest.raises(AssertionError):
                check(honest, 0, f"warm-up {w}: honest split, row with s - w - 1")
        else:
            check(honest, 0, f"warm-up {w}: honest split, row with s - w - 1")


def test_swapped_channels_pass_the_pooled_gate_and_are_caught(split):
    """two channels that carry the quiet row at small amplitudes change places"""
    q = split["names"].index("quiet")
    cand = [c for c in range(37) if split["base_of"][c] == q and c >= len(split["names"])]
    c1, c2 = sorted(cand, key=lambda c: split["exps"][c])[:2]
    assert split["exps"][c1] != split["exps"][c2]
    got = split["model"].copy()
    got[[c1, c2]] = got[[c2, c1]]
    assert ic.pooled_rms_passes(got, split["ref"])
    fails_each(got, split, "channels swapped")
    with pytest.raises(AssertionError):
        ic.scaled_equal(got, split["base_of"], split["exps"], "channels swapped")


def test_float32_recursion_scales_exactly_above_the_room(oracle):
    """scaled_equal's condition for float32 forms: the plain float32 recursion (numpy keeps subnormals, as the kernels do) on an
    impulse followed by silence equals itself under every 2^e wherever no section works below ROOM -- and, on record, not
    everywhere its output is merely normal: the tail of 8 x (0.44, 1.1) differs in the last place before it leaves the
    normal range, which is what the condition is for"""
    coef = ic.F32_CASCADES["8x(0.44,1.1)"]
    n = 512
    rows = ic.signals(n, 1.1, [], gap=64)
    rows = {k: rows[k] for k in ("impulses", "impulses_alt", "burst")}
    x, base_of, exps, _ = ic.scaled_input(rows, 28)
    got = ic.plain_f32(x, coef)
    floor = ic.stage_floor(oracle, x[:3], coef)
    assert ic.scaled_equal(got, base_of, exps, "plain float32", floor) > 25 * n // 3
    with pytest.raises(AssertionError):
        ic.scaled_equal(got, base_of, exps, "plain float32, wherever the output is normal")


def test_one_sample_per_segment_start_passes_the_pooled_gate_and_is_caught(split):
    got = split["model"].copy()
    for s, _ in split["marks"]:
        got[:, s] *= np.float32(1.001)
    assert ic.pooled_rms_passes(got, split["ref"])
    fails_each(got, split, "first sample of each later segment off by 1e-3")


def test_quiet_channel_of_zeros_passes_the_pooled_gate_and_is_caught(split):
    q = split["names"].index("quiet")
    got = split["model"].copy()
    got[q] = 0.0
    assert ic.pooled_rms_passes(got, split["ref"])
    fails_each(got, split, "quiet channel replaced by zeros")


def test_plan_queries_on_the_host():
    """the queries refuse a bad handle cleanly, and the stage pipeline's plan (host arithmetic alone) splits 37 channels
    three ways once a segment holds 8 warm-ups"""
    capi.build()
    L = capi.lib()
    out = (C.c_int * 5)()
    assert L.llz_iir_cascade_mc_plan(0, 1024, out) < 0 and L.llz_iir_cascade_mc_plan(capi.BAD_HANDLE, 1024, out) < 0
    assert L.llz_iir_mc_segments(0, 1024) < 0
    plan = L.llzs_iir_cascade_plan
    plan.restype, plan.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    p = (C.c_int * 3)()
    assert plan(-1, 37, 47 * 1024, 8, 2, p) == 0 and list(p) == [2, 24, 2]
    assert plan(-1, 37, 48 * 1024, 8, 2, p) == 0 and list(p) == [3, 16, 2]
    assert plan(-1, 37, 48 * 1024, 8, 0, p) == 0 and list(p) == [1, 48, 0]          # unknown memory: never split
    assert plan(-1, 37, 1000, 8, 2, p) < 0
    segs = L.llzs_iir_df1_mc_segments
    segs.restype, segs.argtypes = C.c_int, [C.c_long, C.c_int, C.c_int]
    assert segs(24000, 7, 100) == 7 and segs(24000, 7, 6000) == 4 and segs(10, 64, 0) == 10
