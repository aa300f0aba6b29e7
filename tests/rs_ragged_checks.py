"""Shared pieces of the ragged-call resampler tests (test_rs_ragged_host.py, test_resample_ragged_gpu.py): call plans that make a
handle end and start calls inside an L-output period, the whole-stream references, and the per-sample float32 limit.  Plain
numpy; nothing here touches a GPU.

Why: llz_resample_mc takes L and M as given.  With g = gcd(L, M) > 1 a valid call holds a whole number of REDUCED periods
(step = M / g inputs in, L / g outputs out) and may end inside a period of L outputs; with coprime ratios that cannot happen.
Position is counted in steps: a call boundary at `s` steps is a period boundary when s % g == 0, and a call from a period
boundary to residue r = s % g has n_out % L = r L / g: a kernel that stores whole periods writes (g - r) L / g elements past
the row.

Limits, derived and not measured:
  * float32: edge_checks.direct_limit(A, Q), A_i = |gain| sum_k |g[i % L][k]| |x[pos_i - k]| in float64: a float32 sum of Q
    products in any order stays inside it (edge_checks.py, "direct-form kernels");
  * int16: equality with the reference's own frame loop.  The filter is causal and its history starts at zero, so the first
    n L / M outputs of the input zero-padded to whole reference frames are the outputs of the n inputs themselves.
"""
from math import gcd

import numpy as np

from tests import edge_checks as ec

# ratios with a common factor (L, M): the first four take resample_mfma_f32 with Blackman taps, the others resample_f32's
# LDS kernel; all take the int16 screen.  None is in the register-window kernel's list (coprime pairs only).
MFMA_RATIOS = [(294, 320), (320, 294), (150, 160), (160, 150)]
SMALL_RATIOS = [(4, 6), (2, 4), (6, 4), (8, 6), (40, 64), (48, 32)]
RATIOS = MFMA_RATIOS + SMALL_RATIOS


def min_primary(L, M):
    """inputs a call needs so that the matrix-core entry does not decline it as too short: k_resample_mfma_pt_f32 needs
    n_in >= 16 * 64 * waves <= 16384; k_resample_i8d 8 * ngroups, about 1000 at 4:6"""
    return 20000 if (L, M) in MFMA_RATIOS else 3000


def call_plan(L, M, min_primary):
    """([n_in per call], [kind per call]) for one handle.  Every length is a multiple of step = M / g.  Kinds, in order:
      'a'  from a period boundary, ends inside a period (residue g - 1: the smallest overshoot a whole-period store can
           make, L / g elements), >= min_primary inputs
      'b'  starts inside a period, ends on a boundary (several blocks of the fallback kernels)
      'c'  whole periods from a boundary (an odd count), >= min_primary inputs
      'd'  like 'a', >= min_primary inputs; for g > 2 it ends at residue 1 (the largest overshoot)
      'e'  exactly one step, starts inside a period
      'a1' g = 2 only, where 'e' itself lands on a boundary: one step from that boundary, so that 'f' starts inside a period
      'f'  starts inside a period, returns to a boundary
      'c'  whole periods from a boundary, >= min_primary inputs
    """
    g = gcd(L, M)
    assert g > 1, (L, M)
    step = M // g
    need = -(-min_primary // step)                           # steps that hold min_primary inputs

    def at_least(steps, residue):
        return steps + (residue - steps) % g

    r1, r2 = g - 1, 1
    steps, kinds, pos = [], [], 0

    def push(n, kind):
        nonlocal pos
        steps.append(n)
        kinds.append(kind)
        pos += n

    push(at_least(need, r1), "a")
    push(at_least(max(need // 2, -(-5 * 1024 * g // L)), -pos), "b")      # > 2 tiles of 2048 outputs (k_resample_f32_lds)
    periods = -(-need // g) + 2
    push(g * (periods | 1), "c")
    push(at_least(need, r2), "d")
    push(1, "e")
    if pos % g == 0:
        push(1, "a1")
    push(at_least(7 * g, -pos), "f")
    push(g * ((periods + 5) | 1), "c")
    assert pos % g == 0
    return [s * step for s in steps], kinds


def walk(lens, L, M):
    """[(start residue, end residue, n_in, n_out)] per call, residues in steps modulo g (0: on a period boundary)"""
    g = gcd(L, M)
    step = M // g
    out, pos = [], 0
    for n in lens:
        assert n % step == 0 and (n * L) % M == 0, (n, L, M)
        out.append((pos % g, (pos + n // step) % g, n, n * L // M))
        pos += n // step
    return out


def expected_entries(lens, L, M, primary, fallback):
    """the entry each call takes when whole-period calls from a boundary run `primary` and every other call `fallback`"""
    return [primary if (r0 == 0 and r1 == 0) else fallback for (r0, r1, _n, _o) in walk(lens, L, M)]


# ------------------------------------------------------------------------------------------------ references
def ref_f32(oracle, x, L, M, gain, win):
    """float64 whole-stream reference of the rows of x (float32), any n with n L % M == 0"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert (x.shape[1] * L) % M == 0, (x.shape, L, M)
    return oracle.rs_batch_f32(x, L, M, gain, win)


def ref_i16(oracle, x, L, M, gain, win):
    """the reference's frame loop on x zero-padded to whole reference frames, cut to the n L / M outputs of x itself"""
    x = np.ascontiguousarray(x, dtype=np.int16)
    n = x.shape[1]
    assert (n * L) % M == 0, (n, L, M)
    frame = oracle.rs_info(2, L, M, gain, win)["bytes_in"] // 2
    pad = (-n) % frame
    if pad:
        x = np.concatenate([x, np.zeros((x.shape[0], pad), dtype=np.int16)], axis=1)
    return np.ascontiguousarray(oracle.rs_batch_i16(x, L, M, gain, win)[:, :n * L // M])


def f32_limit(x, mat, L, M, gain, chunk=1 << 15):
    """[channels, n_out] per-sample limit: direct_limit(A, Q), A_i = |gain| sum_k |mat[i % L][k]| |x[pos_i - k]| in float64"""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    n_out = ax.shape[1] * L // M
    Q = mat.shape[1]
    amat = np.abs(np.asarray(mat, dtype=np.float64))
    pos, phase = ec.rs_index_map(n_out, L, M)
    A = np.empty((ax.shape[0], n_out))
    k = np.arange(Q)[None, :]
    for o in range(0, n_out, chunk):
        idx = pos[o:o + chunk, None] - k
        w = amat[phase[o:o + chunk]] * (idx >= 0)
        idx = np.maximum(idx, 0)
        for c in range(ax.shape[0]):
            A[c, o:o + chunk] = np.sum(ax[c][idx] * w, axis=1)
    return ec.direct_limit(abs(float(gain)) * A, Q)


def i16_rows(oracle, n, seed):
    """the nine input rows of the screened int16 parity test: random PCM, doubled and clipped, silence, DC 12345, silence then
    signal, both rails, alternating +-20000, and random PCM again in the last row (the row in front of the guard band)"""
    x = oracle.synth_i16(9, n, seed=seed)
    x[1] = (x[1].astype(np.int32) * 2).clip(-32768, 32767).astype(np.int16)
    x[2] = 0
    x[3] = 12345
    x[4, : n // 2] = 0
    x[5] = -32768
    x[6] = 32767
    x[7] = np.where(np.arange(n) % 2 == 0, 1, -1) * 20000
    return x


def probe_cuts(positions, n_in, L, M, Q):
    """call lengths (multiples of M / g) for edge_checks.rs_probe_signal, every cut but one inside the middle half of the
    response of an impulse: two cuts c1 < c2 off a period boundary (near a third and two thirds of the impulses that allow
    one), a one-step call behind c1, and two cuts b1 < b2 ON a period boundary (the first and the last impulse that allow
    one), wherever those fall among the others; the last call ends at n_in, a period boundary.  The call from b1 to b2 is a
    whole-period call from a boundary (the primary entry), so responses straddle a hand-over between the entries as well as
    cuts between two calls that start or end inside a period."""
    g = gcd(L, M)
    step = M // g
    p = positions[0]
    off, on = [], []                                         # cuts off / on a period boundary
    for a in range(len(p)):
        for c in range((int(p[a]) // step + 1) * step, int(p[a]) + Q, step):
            if abs(c - int(p[a]) - Q / 2) <= Q / 4 + 1:
                (on if c % M == 0 else off).append(c)
    assert len(off) >= 3 and len(on) >= 2, (L, M, Q, len(off), len(on))
    c1 = off[len(off) // 3]
    later = [c for c in off if c >= c1 + 2 * step]
    c2 = later[len(later) // 2]
    b1, b2 = min(on), max(on)
    edges = sorted({c1, c1 + step, c2, b1, b2, n_in})
    assert b1 < b2 < n_in and edges[-1] == n_in, edges
    lens = [b - a for a, b in zip([0] + edges[:-1], edges)]
    assert sum(lens) == n_in and all(v > 0 and v % step == 0 for v in lens), lens
    return lens
