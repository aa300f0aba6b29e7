"""Shared pieces of the biquad-bank tests (test_iir_bank_host.py, test_iir_bank_gpu.py): coefficient families in which every
channel differs from its neighbours, the per-channel reference, and a double recursion with carried state for a coefficient
change between calls.  Plain numpy; the double oracle is passed in.  The limits are those of tests/iir_checks.py, unchanged,
applied with each channel's own reference.

Families, 37 channels, channel c, section k, b = g [1, 2, 1] with unit DC gain (as iir_checks.tiled):
  float32   r = 0.30 + 0.006 c + 0.03 k,  theta = 0.4 + 0.03 c + 0.28 k    (radii 0.30 .. 0.73: noise gain at most 10.8 of 16)
  double    r = 0.99 - 0.0005 c - 0.004 k, theta = 0.25 + 0.02 c + 0.31 k  (memory 2 .. 4 chunks, different between channels)
A family of fewer sections is the first sections of the longer one.
"""
import numpy as np

from tests import iir_checks as ic

CHANNELS = 37
IDENTITY = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])


def section(r, theta):
    a1, a2 = -2 * r * np.cos(theta), r * r
    g = (1 + a1 + a2) / 4
    return [g, 2 * g, g, 1.0, a1, a2]


def family32(stages, channels=CHANNELS, shift=None):
    """[channels, stages, 6]; shift: per-channel addition to theta (None: zeros)"""
    shift = np.zeros(channels) if shift is None else shift
    return np.array([[section(0.30 + 0.006 * (c % CHANNELS) + 0.03 * k, 0.4 + 0.03 * (c % CHANNELS) + 0.28 * k + shift[c])
                      for k in range(stages)] for c in range(channels)])


def family64(stages, channels=CHANNELS, shift=None):
    shift = np.zeros(channels) if shift is None else shift
    return np.array([[section(0.99 - 0.0005 * (c % CHANNELS) - 0.004 * k, 0.25 + 0.02 * (c % CHANNELS) + 0.31 * k + shift[c])
                      for k in range(stages)] for c in range(channels)])


def family(precision, stages, channels=CHANNELS, shift=None):
    return (family32 if precision == 32 else family64)(stages, channels, shift)


def many(precision, stages, channels):
    """set c mod 37 of the family with theta shifted by 1e-3 (c // 37): no two channels equal"""
    return family(precision, stages, channels, shift=1e-3 * (np.arange(channels) // CHANNELS))


# (precision, stages, channel, signal) on which plain float32 does not stay within a quarter of the float32 limits, so no
# float32 kernel is held to them there (test_iir_bank_host.py measures every pair; none is widened).  Empty: the float32
# family was chosen with radii low enough for every pair.
F32_DROPPED = set()


def rows_for(n, marks, gap, joins):
    """the signal rows of iir_checks.signals, in its order; tone_res is a placeholder that bank_input replaces per channel"""
    return ic.signals(n, 0.0, marks, gap, joins=joins)


def bank_input(rows, coef):
    """[channels, n] float32: channel c carries row c mod len(rows) at 2^e_c (iir_checks.exponents), tone_res at the channel's
    own pole angle; returns (x, names, base_of)"""
    channels = len(coef)
    x, base_of, exps, names = ic.scaled_input(rows, channels)
    t = np.arange(x.shape[1], dtype=np.float64)
    for c in range(channels):
        if names[base_of[c]] == "tone_res":
            x[c] = np.ldexp((0.9 * np.sin(ic.pole_angle(coef[c]) * t)).astype(np.float32), int(exps[c]))
    return x, names, base_of


def per_channel_ref(oracle, x, coef, precision, real=None):
    """(ref, P): every channel through the oracle with its own set (real[c]: only its first real[c] sections); P the section
    peaks of iir_checks.section_peaks for the double limit, None for float32"""
    ref = np.empty(x.shape, dtype=np.float64)
    P = np.empty(len(x)) if precision == 64 else None
    for c in range(len(x)):
        cf = coef[c] if real is None else coef[c][:real[c]]
        if precision == 64:
            r, p = ic.section_peaks(oracle, x[c:c + 1], cf)
            ref[c], P[c] = r[0], p[0]
        else:
            ref[c] = oracle.iir_cascade_batch_f32(x[c:c + 1], cf)[0]
    return ref, P


_PROBED = {}        # coefficient set (bytes) -> iir_checks.homogeneous_probe's answer: a probe takes 0.03 .. 0.6 s, so each set is probed once


def probe(oracle, cf):
    key = np.ascontiguousarray(cf, dtype=np.float64).tobytes()
    if key not in _PROBED:
        _PROBED[key] = ic.homogeneous_probe(oracle, cf)
    return _PROBED[key]


def bank_warm(oracle, coef):
    """the handle's warm-up restated: the maximum over the channels of the memory probe, 0 if one of them gives 0"""
    mems = [probe(oracle, cf)[0] for cf in coef]
    return 0 if min(mems) == 0 else max(mems)


def plain_f32_bank(x, coef):
    """iir_checks.plain_f32 with a coefficient set per row: the sequential direct-form-I cascade in numpy float32 (every product
    and sum rounded to float32).  x [rows, n], coef [rows, S, 6].  Shows that a float32 limit is attainable; never a reference."""
    x = np.asarray(x, dtype=np.float32)
    c = np.asarray(coef, dtype=np.float64).astype(np.float32)
    R, n = x.shape
    S = c.shape[1]
    st = np.zeros((S, 4, R), dtype=np.float32)
    out = np.empty_like(x)
    for t in range(n):
        v = x[:, t]
        for s in range(S):
            x1, x2, y1, y2 = st[s]
            acc = c[:, s, 0] * v + c[:, s, 1] * x1 + c[:, s, 2] * x2 - c[:, s, 4] * y1 - c[:, s, 5] * y2
            st[s, 1], st[s, 0], st[s, 3], st[s, 2] = x1, v, y1, acc
            v = acc
        out[:, t] = v
    return out


def df1_carried(x, coef, state=None):
    """Direct form I in numpy double, rows in parallel, a coefficient set per row and the state carried: x [rows, n] float32,
    coef [rows, S, 6], state [rows, S, 4] = x1, x2, y1, y2 (None: zeros).  Returns (y [rows, n] double, the end state, P [rows] =
    the largest magnitude of the input and of any section's output, as iir_checks.section_peaks).  The reference of a
    coefficient change between two calls, where the oracle (which starts from zero state) cannot serve; the tests pin it to
    the oracle on an unchanged frame."""
    x = np.asarray(x, dtype=np.float64)
    c = np.asarray(coef, dtype=np.float64)
    R, n = x.shape
    S = c.shape[1]
    st = np.zeros((S, 4, R)) if state is None else np.array(np.transpose(state, (1, 2, 0)), dtype=np.float64)
    out = np.empty((R, n))
    peak = np.zeros((S, n, R))
    for t in range(n):
        v = x[:, t]
        for s in range(S):
            x1, x2, y1, y2 = st[s]
            acc = c[:, s, 0] * v + c[:, s, 1] * x1 + c[:, s, 2] * x2 - c[:, s, 4] * y1 - c[:, s, 5] * y2
            st[s, 1], st[s, 0], st[s, 3], st[s, 2] = x1, v, y1, acc
            peak[s, t] = acc
            v = acc
        out[:, t] = v
    P = np.maximum(np.abs(x).max(axis=1), np.abs(peak).max(axis=(0, 1)))
    return out, np.transpose(st, (2, 0, 1)), P


def sample_ratio(got, ref, limit):
    """the worst |got - ref| / limit per row, without asserting (iir_checks._ratio's conventions)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return ic._ratio(err, np.broadcast_to(limit, err.shape)).max(axis=1)


def chunk_ratio(got, ref, x):
    """the worst per-chunk ratio of iir_checks.chunk_check per row, without asserting"""
    got = np.asarray(got, dtype=np.float64)
    n = ref.shape[1]
    starts = np.arange(0, n, ic.CHUNK)
    counts = np.minimum(starts + ic.CHUNK, n) - starts
    e2 = np.add.reduceat((got - ref) ** 2, starts, axis=1) / counts
    r2 = np.add.reduceat(ref ** 2, starts, axis=1) / counts
    x2 = np.mean(np.asarray(x, dtype=np.float64) ** 2, axis=1, keepdims=True)
    return ic._ratio(np.sqrt(e2), ic.TOL * np.sqrt(np.maximum(r2, x2))).max(axis=1)
