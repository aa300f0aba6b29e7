"""Shared pieces of the IIR signal tests (test_iir_checks_host.py, test_iir_signals_gpu.py): the cascades, the signals that
stress a recursion, the limits a result is held to, and a model of the time split to plant faults in.  Plain numpy (the
double oracle is passed in where a recursion has to be run); nothing here touches a GPU.

Why: the batch IIR forms split a channel along time into segments that start a warm-up early from the ZERO state, choose
float32 or double from a measured noise gain, and hand one state between up to three kernels per call.  Zero-mean noise of
one scale, a few spot channels and one RMS over the whole array cannot see a wrong channel, one wrong sample per segment
(1 / sqrt(8192) of the RMS), a quiet channel beside a loud one, or a split that never happened.

Limits (u = 2^-24, TOL = 1e-5 the project's gate), derived and not measured:
  * double forms, per sample: |got - ref| <= 1.01 u |ref| + 1e-9 P_c, P_c the largest magnitude of the input and of any
    section's output on channel c.  1.01 u |ref| is the one rounding of the store.  1e-9 P_c covers (i) double rounding
    through the noise gain: at most 16 sections x a few 2^-53 x an L1 gain of 1/A(z) below 1e4 = 1e-11 P_c, and (ii) the
    warm-up residue: a later segment misses the state of up to 16 sections, each value at most P_c, of which 1e-13 x (peak of
    the homogeneous response) is left per unit of state at its first kept sample.  The host test asserts that peak <= 1e3
    (residue 1e-10) for the double cascades used, and, since highq8 peaks at 9.9e3, the residue itself as the restated probe
    measures it: <= 1e-11 per unit state, so 2 x 16 x 1e-11 P_c = 3.2e-10 P_c (2: the probe plants (1, 1), a state may point
    elsewhere) stays a third of the term for every one of them;
  * float32 forms: the project's tolerance, local instead of pooled: per channel and 1024-sample chunk
    rms(err) <= TOL max(rms(ref chunk), rms(x_c)), and per sample |err| <= TOL max(max |ref_c|, max |x_c|).  Condition: the
    plain sequential float32 recursion (plain_f32) stays at or below a quarter of both on every (cascade, signal) pair used,
    so the limit asks nothing float32 cannot give.  8 x (0.8, 2.0) does not meet it (tone_stop 0.36 / 0.25, dc 0.20) and is
    not in F32_CASCADES; the limit is never widened.
"""
import os

import numpy as np

TOL = 1e-5                  # RMS, north_star (tests/test_gpu_parity.py)
U = 2.0 ** -24
CHUNK = 1024                # samples of the per-chunk gate and of the memory probe
TINY = 2.0 ** -126          # the smallest normal float32
ROOM = TINY * 2.0 ** 48     # float32 arithmetic below this may round on the subnormal grid (scaled_equal)
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------ cascades
def tiled(stages, radius, theta):
    """`stages` equal sections, poles radius * exp(+-i theta), b = g [1, 2, 1] with unit DC gain"""
    a1, a2 = -2 * radius * np.cos(theta), radius ** 2
    g = (1 + a1 + a2) / 4
    return np.tile(np.array([g, 2 * g, g, 1.0, a1, a2]), (stages, 1))


def distinct_low_q(stages):
    """every section different, radii 0.30 .. 0.72 (test_iir_cascade_wave_distinct_sections): float32"""
    rows = []
    for k in range(stages):
        r, th = 0.30 + 0.06 * k, 0.4 + 0.33 * k
        a1, a2 = -2 * r * np.cos(th), r * r
        b = np.array([1.0, 0.3 - 0.2 * k, 0.1 * k]) * (1 + a1 + a2) / (1.3 - 0.1 * k)
        rows.append(np.concatenate([b, [1.0, a1, a2]]))
    return np.array(rows)


def distinct_high_q(stages):
    """every section different, radii 0.99 .. 0.962 (test_iir_cascade_wave_double_distinct_sections): double"""
    rows = []
    for k in range(stages):
        r, th = 0.99 - 0.004 * k, 0.25 + 0.31 * k
        a1, a2 = -2 * r * np.cos(th), r * r
        b = np.array([1.0, 0.3 - 0.2 * k, 0.1 * k]) * (1 + a1 + a2) * (0.7 + 0.2 * k)
        rows.append(np.concatenate([b, [1.0, a1, a2]]))
    return np.array(rows)


def descending(radius):
    """4 sections of radius - 0.02 k at 0.4 + 0.3 k rad, unit DC gain (test_iir_time_segments_stream_across_calls)"""
    rows = []
    for k in range(4):
        r, th = radius - 0.02 * k, 0.4 + 0.3 * k
        a1, a2 = -2 * r * np.cos(th), r * r
        rows.append([(1 + a1 + a2) / 4, (1 + a1 + a2) / 2, (1 + a1 + a2) / 4, 1.0, a1, a2])
    return np.array(rows)


def fixture_mix():
    """the reference fixture's high-Q section around its ordinary one (test_iir_cascade_few_channels_split_along_time)"""
    d = np.load(os.path.join(G, "iir.npz"), allow_pickle=False)
    hq, lo = np.concatenate([d["bq"], d["aq"]]), np.concatenate([d["b2"], d["a2"]])
    return np.stack([hq, lo, hq])


# name -> coefficient rows {b0, b1, b2, a0, a1, a2}; the precision the library chooses for each is known from the tests named
F32_CASCADES = {
    "8x(0.44,1.1)": tiled(8, 0.44, 1.1),
    "3x(0.7,0.5)": tiled(3, 0.7, 0.5),
    "2x(0.95,1.0)": tiled(2, 0.95, 1.0),
    "distinct5": distinct_low_q(5),         # odd: the unpacked float32 kernel
    "distinct8": distinct_low_q(8),         # even: the packed one
    # 8 x (0.8, 2.0) is left out: plain float32 takes 0.36 / 0.25 of the limits on tone_stop (see the module docstring)
}
# (cascade, signal) pairs on which plain float32 does not stay within a quarter of the float32 limits, so no float32 kernel is
# held to them there (8192 samples, worst chunk / worst sample as fractions of the limit):
#   distinct8, dc        1.33 / 0.77
#   distinct8, tone_res  63 / 8.6
# The later sections of distinct8 have their poles near Nyquist and gain up to 63 there, so the rounding noise of the early
# sections (white) leaves the cascade amplified some 1e4 times: about 1e-3 absolute, whatever the input.  Under white noise
# the output is as large and the error relative to it is small; under DC or a low tone the output is of order 1 and the
# same noise is 1e-3 of it.  The library runs distinct8 in float32 all the same (its criterion weighs each section's own
# noise gain, not the gain of the sections behind it): DESIGN.md, IIR section, records that.
F32_DROPPED = {("distinct8", "dc"), ("distinct8", "tone_res")}


def kept_rows(name, rows):
    """the signal rows a cascade is held to: all but its F32_DROPPED pairs"""
    return {k: v for k, v in rows.items() if (name, k) not in F32_DROPPED}


F64_CASCADES = {
    "4x(0.99-0.02k)": descending(0.99),
    "highq3": distinct_high_q(3),
    "highq8": distinct_high_q(8),
    "fixture mix": fixture_mix(),
}


def pole_angle(coef):
    """angle of the first section's pole pair"""
    a1, a2 = coef[0][4], coef[0][5]
    return float(np.arccos(np.clip(-a1 / (2 * np.sqrt(a2)), -1.0, 1.0)))


# ------------------------------------------------------------------------------------------------ the plan, in samples
def marks_of(plan, n_main):
    """[(s, w)] for every later segment of a launch of n_main samples run as `plan` (IirCascadeMC.plan): s its first written
    sample, w its warm-up in samples.  Segment k covers chunks [k seg_chunks, (k + 1) seg_chunks) of plan['chunk'] samples."""
    seg = plan["seg_chunks"] * plan["chunk"]
    w = plan["warm"] * plan["chunk"]
    return [(k * seg, w) for k in range(1, plan["segs"]) if k * seg < n_main]


def main_samples(plan, n):
    """the samples of an n-sample frame that the planned launch takes: its whole chunks"""
    n4 = n - n % CHUNK if n % 4 == 0 else 0
    return n4 - n4 % plan["chunk"]


# ------------------------------------------------------------------------------------------------ signals
def impulse_positions(n, marks):
    """(row_a, row_b): for a segment (s, w) the four places s - w - 1 (the last sample it never sees), s - w (the first it
    does), s - 1 and s.  Neighbours cannot share a row 64 apart, so odd-numbered marks put the first of each pair into row_a
    and the second into row_b, even-numbered ones the other way round; then each row is thinned to 64 samples apart."""
    rows = ([], [])
    for k, (s, w) in enumerate(marks):
        for first, second in ((s - w - 1, s - w), (s - 1, s)):
            rows[k % 2].append(first)
            rows[1 - k % 2].append(second)
    out = []
    for r in rows:
        kept = []
        for p in sorted(set(p for p in r if 0 <= p < n)):
            if not kept or p - kept[-1] >= 64:
                kept.append(p)
        out.append(np.array(kept, dtype=np.int64))
    return tuple(out)


def signals(n, theta, marks, gap, seed=1, joins=()):
    """{name: float32 row of n samples}.  marks: [(s, w)] from the plan (marks_of); gap: the silence inside `burst`, in samples
    (longer than the cascade's memory); joins: further places p where one kernel or call hands the state to the next, which
    get impulses at p - 1 and p.  Without marks the impulse rows hold one impulse at n // 3 and n // 3 + 1."""
    marks = list(marks) + [(p, 0) for p in joins]
    t = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(seed)
    noise = [rng.uniform(-1.0, 1.0, n).astype(np.float32) for _ in range(3)]
    rows = {
        "dc": np.full(n, 0.7, dtype=np.float32),
        "tone_res": (0.9 * np.sin(theta * t)).astype(np.float32),
        "tone_stop": (0.9 * np.sin(3.0 * t)).astype(np.float32),
    }
    pa, pb = impulse_positions(n, marks) if marks else (np.array([n // 3]), np.array([n // 3 + 1]))
    for name, pos in (("impulses", pa), ("impulses_alt", pb)):
        r = np.zeros(n, dtype=np.float32)
        r[pos] = 1.0
        rows[name] = r
    burst = noise[0].copy()
    g0 = max(64, min(n // 4, n - gap - 64))
    burst[g0:g0 + gap] = 0.0
    rows["burst"] = burst
    rows["quiet"] = noise[1] * np.float32(2.0 ** -10)
    rows["loud"] = noise[2] * np.float32(2.0 ** 10)
    rows["zero"] = np.zeros(n, dtype=np.float32)
    return rows


def exponents(channels, bases):
    """e_c: 0 for the base channels c < bases, else in [-12, 12] and different between neighbours"""
    e = np.array([(c * 7) % 25 - 12 for c in range(channels)], dtype=np.int64)
    e[:bases] = 0
    assert np.all(np.diff(e[bases:]) != 0)
    return e


def scaled_input(rows, channels):
    """[channels, n] float32: channel c carries row c mod len(rows) times 2^e_c (exact); returns (x, base_of, exps, names)"""
    names = list(rows)
    base_of = np.arange(channels) % len(names)
    exps = exponents(channels, len(names))
    x = np.stack([np.ldexp(rows[names[b]], int(e)) for b, e in zip(base_of, exps)]).astype(np.float32)
    return x, base_of, exps, names


# ------------------------------------------------------------------------------------------------ reference side
def section_peaks(oracle, x, coef):
    """(ref, P): the double oracle's output [channels, n] and P_c = the largest magnitude of the input and of any section's
    output on channel c (the oracle run on the prefixes coef[:k])"""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 6)
    P = np.abs(x).max(axis=1).astype(np.float64)
    ref = None
    for k in range(1, len(coef) + 1):
        ref = oracle.iir_cascade_batch_f32(x, coef[:k])
        P = np.maximum(P, np.abs(ref).max(axis=1))
    return ref, P


def stage_floor(oracle, x, coef):
    """[rows, n]: at each sample the smallest non-zero magnitude among the input and every section's output (the double
    oracle on the prefixes coef[:k]); inf where all of them are exactly zero.  It says how close to the subnormals a
    float32 recursion works at that sample (scaled_equal)."""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 6)
    low = np.where(x != 0, np.abs(x).astype(np.float64), np.inf)
    for k in range(1, len(coef) + 1):
        y = np.abs(oracle.iir_cascade_batch_f32(x, coef[:k]))
        low = np.minimum(low, np.where(y != 0, y, np.inf))
    return low


def homogeneous_probe(oracle, coef, max_chunks=64):
    """The library's memory probe, restated from its definition (include/llz_iir.h, time segments): unit outputs planted in
    each section in turn (y[-1] = y[-2] = 1, every other state zero), zero input; env[k] = the largest magnitude at any
    section output in 1024-sample chunk k.  Returns (memory, peak, residue): the first chunk count after which env stays
    below 1e-13 x peak, plus one chunk of margin (0: not within max_chunks); peak = max(1, max env); and the largest env
    from chunk `memory` on, which is what a segment warmed up over `memory` chunks still misses of a unit state.

    A section's response to that state is the zero-state response of 1 / A(z) to the two samples (-a1 - a2, -a2), so the
    oracle runs it: a section {1, 0, 0, 1, a1, a2} in place of section s0, the sections behind it unchanged.  (The oracle
    takes float32 input: the two samples carry a rounding of 6e-8, nothing to a peak or to a level 13 decades down.)"""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 6)
    S = len(coef)
    n = max_chunks * CHUNK
    env = np.zeros(max_chunks)
    for s0 in range(S):
        a1, a2 = coef[s0][4], coef[s0][5]
        x = np.zeros((1, n), dtype=np.float32)
        x[0, 0], x[0, 1] = -a1 - a2, -a2
        rows = np.concatenate([[[1.0, 0.0, 0.0, 1.0, a1, a2]], coef[s0 + 1:]])
        for k in range(1, len(rows) + 1):
            y = np.abs(oracle.iir_cascade_batch_f32(x, rows[:k])[0])
            if not np.all(y < 1e300):
                return 0, float("inf"), float("inf")
            env = np.maximum(env, y.reshape(max_chunks, CHUNK).max(axis=1))
    peak = max(1.0, float(env.max()))
    loud = np.flatnonzero(env >= 1e-13 * peak)
    last = int(loud[-1]) if loud.size else -1
    mem = 0 if last >= max_chunks - 2 else last + 2
    return mem, peak, (float(env[mem:].max()) if mem else float("inf"))


def df1_memory(a, limit=1 << 16):
    """the general direct form's probe (llz_iir_mc): 1 / A(z) from the unit state (every y delay = 1), zero input; the index
    of the last sample above 1e-13 of the largest seen, plus one (0: has not died out)"""
    a = np.asarray(a, dtype=np.float64)
    M = len(a) - 1
    if M == 0:
        return 1
    y = [1.0] * M
    peak, last = 1.0, 0
    for t in range(limit):
        acc = 0.0
        for k in range(1, M + 1):
            acc -= a[k] * y[k - 1]
        y = [acc] + y[:-1]
        m = abs(acc)
        if not m < 1e300:
            return 0
        peak = max(peak, m)
        if m > 1e-13 * peak:
            last = t
    return last + 1 if last < limit - limit // 8 else 0


def plain_f32(x, coef):
    """the sequential direct-form-I cascade in numpy float32 (every product and sum rounded to float32), rows in parallel.
    It shows that a float32 limit is attainable; it is never a reference for a kernel."""
    x = np.asarray(x, dtype=np.float32)
    c = np.asarray(coef, dtype=np.float64).reshape(-1, 6).astype(np.float32)
    S, (C, n) = len(c), x.shape
    st = np.zeros((S, 4, C), dtype=np.float32)          # x1, x2, y1, y2
    out = np.empty_like(x)
    for t in range(n):
        v = x[:, t]
        for s in range(S):
            x1, x2, y1, y2 = st[s]
            acc = c[s, 0] * v + c[s, 1] * x1 + c[s, 2] * x2 - c[s, 4] * y1 - c[s, 5] * y2
            st[s, 1], st[s, 0], st[s, 3], st[s, 2] = x1, v, y1, acc
            v = acc
        out[:, t] = v
    return out


def split_model(oracle, x, coef, marks, fault=None):
    """A model of the time split in the oracle's own arithmetic: segment 0 from the true state, the segment at (s, w) from
    ZERO state at sample s - w, kept from s to the next mark; rounded to float32 like a kernel's store.
    fault: None, "no_warm" (w = 0) or "late" (the warm-up starts at s - w + 1: the sample at s - w is lost)."""
    n = x.shape[1]
    edges = [0] + [s for s, _ in marks] + [n]
    out = np.empty(x.shape, dtype=np.float32)
    out[:, :edges[1]] = oracle.iir_cascade_batch_f32(x[:, :edges[1]], coef)
    for k, (s, w) in enumerate(marks):
        start = s if fault == "no_warm" else s - w + (1 if fault == "late" else 0)
        assert 0 <= start <= s
        y = oracle.iir_cascade_batch_f32(np.ascontiguousarray(x[:, start:edges[k + 2]]), coef)
        out[:, s:edges[k + 2]] = y[:, s - start:]
    return out


# ------------------------------------------------------------------------------------------------ checks
def pooled_rms_passes(got, ref):
    """the old gate: one RMS over every channel and sample, as the many-channel IIR tests of test_gpu_parity.py apply it"""
    got = np.asarray(got, dtype=np.float64)
    err, scale = float(np.sqrt(np.mean((got - ref) ** 2))), float(np.sqrt(np.mean(ref ** 2)))
    return err <= TOL * max(1.0, scale) and err / scale <= TOL


def _where(w, seg_len):
    s = f"channel {w[0]} index {w[1]}"
    return s + (f" (index mod segment {seg_len} = {w[1] % seg_len})" if seg_len else "")


def _ratio(err, limit):
    """err / limit, with 0 / 0 = 0 and x / 0 = inf"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / limit)


def sample_check(got, ref, limit, what, seg_len=None):
    """|got - ref| <= limit at every sample (limit broadcasts against ref); names the worst channel, index and index modulo
    the segment length; returns the worst ratio to the limit"""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    limit = np.broadcast_to(limit, err.shape)
    ratio = _ratio(err, limit)
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[w])
    print(f"{what}: per sample, worst {worst:.3g} of its limit ({float(err[w]):.3g} of {float(limit[w]):.3g}) at {_where(w, seg_len)}")
    assert worst <= 1.0, (f"{what}: {int(np.count_nonzero(ratio > 1))} samples over their limit; worst {float(err[w]):.3g} > "
                          f"{float(limit[w]):.3g} at {_where(w, seg_len)}: got {float(got[w]):.9g} ref {float(ref[w]):.9g}")
    return worst


def chunk_check(got, ref, x, what, seg_len=None):
    """float32 forms: per channel and 1024-sample chunk (the last may be ragged) rms(err) <= TOL max(rms(ref chunk), rms(x_c))"""
    got = np.asarray(got, dtype=np.float64)
    n = ref.shape[1]
    starts = np.arange(0, n, CHUNK)
    counts = np.minimum(starts + CHUNK, n) - starts
    e2 = np.add.reduceat((got - ref) ** 2, starts, axis=1) / counts
    r2 = np.add.reduceat(ref ** 2, starts, axis=1) / counts
    x2 = np.mean(np.asarray(x, dtype=np.float64) ** 2, axis=1, keepdims=True)
    err, limit = np.sqrt(e2), TOL * np.sqrt(np.maximum(r2, x2))
    ratio = _ratio(err, limit)
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[w])
    where = f"channel {w[0]} chunk {w[1]} (samples from {int(starts[w[1]])}" + \
            (f", mod segment {seg_len} = {int(starts[w[1]]) % seg_len})" if seg_len else ")")
    print(f"{what}: per chunk, worst {worst:.3g} of its limit (rms {float(err[w]):.3g} of {float(limit[w]):.3g}) at {where}")
    assert worst <= 1.0, (f"{what}: {int(np.count_nonzero(ratio > 1))} chunks over their limit; worst rms {float(err[w]):.3g} > "
                          f"{float(limit[w]):.3g} at {where}")
    return worst


def f32_sample_limit(ref, x):
    """float32 forms, per sample: TOL max(max |ref_c|, max |x_c|), one value per channel"""
    return TOL * np.maximum(np.abs(ref).max(axis=1), np.abs(np.asarray(x, dtype=np.float64)).max(axis=1))[:, None]


def f64_sample_limit(ref, P):
    """double forms, per sample: 1.01 u |ref| + 1e-9 P_c"""
    return 1.01 * U * np.abs(ref) + 1e-9 * np.asarray(P)[:, None]


def local_checks(got, ref, x, precision, what, seg_len=None, P=None):
    """the limits of the form's precision; returns {check: worst ratio}"""
    if precision == 64:
        return {"sample": sample_check(got, ref, f64_sample_limit(ref, P), what, seg_len)}
    return {"chunk": chunk_check(got, ref, x, what, seg_len),
            "sample": sample_check(got, ref, f32_sample_limit(ref, x), what, seg_len)}


def scaled_equal(got, base_of, exps, what, floor=None):
    """Power-of-two covariance, no tolerance: channel c carried the input of channel base_of[c] times 2^exps[c], so its output
    must equal that channel's output times 2^exps[c] exactly (IEEE arithmetic commutes with a power of two away from under-
    and overflow).  Evaluated where the base output and its scaled value are normal float32 (an impulse tail decays
    through the subnormals, where it does not).  Returns the number of samples compared.

    floor (float32 forms): stage_floor of the base channels, [bases, n].  A form that computes in double rounds to float32
    once, at the store, so a normal output is all the property needs.  A float32 form rounds every section's output, every
    partial sum and every carried state, and an impulse tail takes those through the subnormals while the cascade's
    output is still normal: after k equal sections the tail is (t^(k-1) / (k-1)!) r^t, which at t = 100 stands 2^34 above
    the first section's r^t.  One result rounded on the subnormal grid (spacing 2^-149, whatever the scale) in one of the
    two channels, and the outputs behind it differ in the last place.  So a sample of a float32 form is compared where, in
    both channels, no input or section output is non-zero and below ROOM = 2^48 x the smallest normal.  The first 2^24:
    a sum of terms that are at least 2^24 above the smallest normal is a multiple of 2^-149 however far it cancels, so it
    is exact even where it is subnormal.  The second 2^24: a product with a coefficient, a partial sum or a state carried
    between lanes that is smaller still against the section outputs is below their last place.  What a tail left in the
    state while below ROOM is at most 2^-126; once signal returns (at least 2^-32 here: amplitude 2^-12, the smallest
    gain 2^-19) it is 2^-70 of a last place of anything it is added to."""
    got = np.asarray(got, dtype=np.float32)
    compared = 0
    for c in range(got.shape[0]):
        b, e = int(base_of[c]), int(exps[c])
        if b == c:
            assert e == 0
            continue
        want = np.ldexp(got[b], e).astype(np.float32, copy=False)         # exact wherever the result is normal
        ok = (np.abs(got[b]) >= TINY) & (np.abs(want) >= TINY) & (np.abs(want) < 2.0 ** 127)
        if floor is not None:
            ok &= floor[b] * 2.0 ** min(e, 0) >= ROOM                     # the oracle is double: its floor scales exactly
        bad = np.flatnonzero(ok & (got[c] != want))
        assert bad.size == 0, (f"{what}: channel {c} is not channel {b} x 2^{e} at {bad.size} samples, first index {int(bad[0])}: "
                               f"got {float(got[c][bad[0]]):.9g} want {float(want[bad[0]]):.9g}")
        assert np.all(np.isfinite(got[c]))
        compared += int(np.count_nonzero(ok))
    print(f"{what}: {compared} samples equal their base channel's times 2^e, bit for bit")
    return compared


def assert_zero_rows(got, x, what):
    """a zero row gives exactly zero"""
    for c in np.flatnonzero(~np.any(np.asarray(x) != 0, axis=1)):
        nz = np.flatnonzero(np.asarray(got)[c] != 0)
        assert nz.size == 0, f"{what}: channel {c} is all zero on input and has {nz.size} non-zero outputs, first at {int(nz[0])}"
