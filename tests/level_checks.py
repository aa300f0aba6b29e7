"""Shared pieces of the FIR level tests (test_level_checks_host.py, test_fir_levels_gpu.py): a signal of level steps, a burst
and silence, a per-sample limit that follows the level a transform can see, float32 / complex64 MODELS of every pairing
scheme, and the check.  Plain numpy; nothing here touches a GPU.

Why: every overlap-save form puts two blocks of one channel into the real and the imaginary part of one complex transform (or
sums spectra kept for P blocks), so in float32 the rounding error of a sample scales with the loudest partner of its transform.
Under stationary noise and a limit taken from the rms of the whole row, a carried halo from the wrong sub-stream, a dead region
that is used instead of zeroed or a ring slot that is not cleared has to be about as large as the signal to be seen.  Here
a quiet zone (2^-20 of full scale) and a silent one lie next to loud ones, and the limit of a sample is taken from the
energy within the REACH of its transform alone: in silence beyond the reach the output must be +-0 exactly.

Signal (level_signal): every zoned row is LOUD | SILENT | QUIET | BURST (64 loud samples) | QUIET | LOUD.  LOUD is the oracle's
generator as it comes (uniform in [-1, 1)), QUIET the generator times 2^-20 (exact), SILENT exact zeros.  Every SILENT and
QUIET zone is at least zone_len() = 2 reach + T + margin samples (margin >= 1024), so at least 1024 consecutive samples of each
lie beyond the reach of anything louder; level_signal asserts that for every row it returns.

Limit (level_limit), u = 2^-24, derived and not measured:
    L_n = 8 u log2(nfft) ||h||_1 sqrt(E_n),   E_n = sum of x^2 over [n - (T - 1) - reach, n + reach]
the norm bound of edge_checks.ols_limit with the energy of the whole row (nfft rms^2) replaced by the energy a transform of
sample n can see.  ||h||_1 replaces ||h||_2 because it bounds all three error sources for dense taps too: the forward transform
(||h||_2 <= ||h||_1), the product and the inverse (max |H| <= ||h||_1).  Where E_n = 0 the limit is 0.  Time-domain kernels
and the flush tails that run through one keep edge_checks.direct_limit(A_n, T), which is local already and 0 in silence.

Reach per form, with the lines it is read from:
  * consecutive pair (the 1024-point segment walk, the 2048 / 4096 / 8192 rungs, the bank): 2 nfft.  A job is two CONSECUTIVE
    blocks, [s - O, s + V) real and [s + V - O, s + 2 V) imaginary (fir_ols.hip:17-19 and :33-35 for 1024, :249-252 for 2048
    -- it assembles with the 1024-point walk's ols_assemble --, :507 for 4096, :794 for 8192): an output shares its transform
    with samples at most 2 nfft - O away.
  * super-block walk: OLS_SB_REGION + nfft.  Job i is block i of region 0 with block i of region 1, OLS_SB_REGION samples
    later, the short 11th job included (ols_superblock.h:6-12).
  * partitioned and the partitioned bank: (Kh + 2) B.  Z_q = X_q + j X_{q+Kh}, Kh = ceil(K / 2), X_q the samples of blocks
    (q - 1, q), and output block q sums Z_{q-p} H_p over p < P (fir_part.hip:4-6 and :10-13, k_fir_part_fwd :73-75): a sample
    of block q sees up to block q + Kh, one of block q + Kh down to block q - P, which is (Kh + 1) B + B - 1 behind n - (T - 1).
  * stream and matrix convolvers: 2 block.  Output block j sums X_{j-p} H_p, p < P, X_q the spectrum of input blocks
    (q - 1, q) (fir_stream.hip:4-5): nothing before block j - P, which is less than 2 block behind n - (T - 1).
"""
import os
import re

import numpy as np

from tests import edge_checks as ec
from tests import matrix_checks as mc
from tests import stream_checks as sc

U = ec.U
QUIET = 2.0 ** -20
BURST = 64
MARGIN = 1024
TIGHT = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "llzlab_amd", "csrc", "kernels")


def sb_constants():
    """the constexpr ints of ols_superblock.h by name: the geometry is read from the header, not retyped"""
    with open(os.path.join(KERNELS, "ols_superblock.h")) as f:
        text = f.read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr\s+int\s+(OLS_SB_\w+)\s*=\s*(\d+)\s*;", text)}


SB = sb_constants()
SB_NFFT = 1024


# ------------------------------------------------------------------------------------------------ reach
def reach_consecutive(nfft):
    return 2 * nfft


def reach_superblock():
    return SB["OLS_SB_REGION"] + SB_NFFT


def reach_partitioned(K, B):
    return (-(-K // 2) + 2) * B


def reach_ring(block):
    return 2 * block


def zone_len(reach, T, margin=MARGIN):
    assert margin >= MARGIN
    return 2 * reach + T + margin


# ------------------------------------------------------------------------------------------------ the signal
def _on(p, shift, call, bound):
    period, phase = bound
    return ((p - shift) % call) % period == phase


def _snap(p, step, shift, call, bounds):
    """the nearest position from p on in direction step that lies `shift` behind a boundary of the call"""
    for _ in range(2 * call + 2):
        if p >= 0 and any(_on(p, shift, call, b) for b in bounds):
            return p
        p += step
    return -1 if step < 0 else 1 << 60


def _row_layout(n, Z, T, call, bounds, shift, d, lead):
    """edges of one zoned row: a (LOUD -> SILENT), q (SILENT -> QUIET), b (burst start), c (QUIET -> LOUD), and the call
    boundary `cut` that lies d samples behind the burst's end.  The edge an index prefers comes first; None: no room"""
    for m in range(1, n // call):
        cut = m * call
        b = cut - d - BURST
        if b < lead + 2 * Z:
            continue
        q = _snap(b - Z, -1, shift, call, bounds[1:2])
        if q < lead + Z:
            q = _snap(b - Z, -1, shift, call, bounds)
        a = _snap(q - Z, -1, shift, call, bounds[0:1])
        if a < lead:
            a = _snap(q - Z, -1, shift, call, bounds)
        c0 = max(b + BURST + Z, cut + 1)
        c = _snap(c0, 1, shift, call, bounds[2:3])
        if c + lead > n:
            c = _snap(c0, 1, shift, call, bounds)
        if a >= lead and q >= a + Z and c + lead <= n:
            return dict(a=a, q=q, b=b, c=c, cut=cut, shift=shift)
    return None


def level_layout(n, reach, T, call, bounds, block, zoned=3, margin=MARGIN):
    """the edges of `zoned` rows of n samples, or None where n has no room.  Row 0 has its edges on a boundary of the call
    (bounds: [(period, phase)] within a call), row 1 one sample behind one, row 2 mid-block; the call boundary lies in the second
    QUIET zone fewer than T - 1 samples behind the burst in row 0 (the history carries the burst), more than reach + T behind
    it in row 1 and within the reach in row 2"""
    Z = zone_len(reach, T, margin)
    bounds = list(bounds)
    while len(bounds) < 3:
        bounds.append(bounds[-1])
    lead = T + block
    shifts = (0, 1, block // 2 + 3)
    behind = (max(1, min((T - 1) // 2, T - 2)), reach + T + 1 + block // 3, reach // 2 + T)
    rows = []
    for r in range(zoned):
        # rows take the preferred boundary kinds in turn, so that every kind is met
        pref = bounds[r % 3:] + bounds[:r % 3]
        lay = _row_layout(n, Z, T, call, pref, shifts[r % 3] + (r // 3) * 7, behind[r % 3], lead)
        if lay is None:
            return None
        rows.append(lay)
    return rows


def level_calls(reach, T, call, bounds, block, zoned=3, margin=MARGIN):
    """the fewest calls whose samples hold every zoned row"""
    calls = max(2, -(-(3 * zone_len(reach, T, margin)) // call))
    while level_layout(calls * call, reach, T, call, bounds, block, zoned, margin) is None:
        calls += 1
        assert calls * call < 40 * zone_len(reach, T, margin), "the rows never fit"
    return calls


def default_roles(channels):
    """three zoned rows, then (with room) a quiet, a loud and a silent row, the loud one between the others; else loud rows"""
    roles = ["zoned"] * min(3, channels)
    if channels >= 6:
        roles += ["quiet", "loud", "silent"]
    return roles + ["loud"] * (channels - len(roles))


def level_signal(oracle, channels, n, reach, T, seed, call=None, bounds=None, block=None, roles=None, margin=MARGIN):
    """([channels, n] float32, info): the rows by role (default_roles), the zoned ones laid out by level_layout.  info: roles,
    edges (a dict per zoned row, None elsewhere), reach, T, Z.  The zone condition is asserted for every zoned row."""
    call = call or n
    block = block or 64
    bounds = bounds or [(call, 0)]
    roles = list(roles or default_roles(channels))
    assert len(roles) == channels and n % call == 0
    lay = level_layout(n, reach, T, call, bounds, block, roles.count("zoned"), margin)
    assert lay is not None, f"{n} samples have no room for zones of {zone_len(reach, T, margin)}"
    x = oracle.synth_f32(channels, n, seed=seed)
    edges = []
    quiet = np.float32(QUIET)
    for c, role in enumerate(roles):
        e = None
        if role == "silent":
            x[c] = 0
        elif role == "quiet":
            x[c] *= quiet
        elif role == "zoned":
            e = lay[sum(1 for r in roles[:c] if r == "zoned")]
            x[c, e["a"]:e["q"]] = 0
            x[c, e["q"]:e["b"]] *= quiet
            x[c, e["b"] + BURST:e["c"]] *= quiet
        else:
            assert role == "loud", role
        edges.append(e)
    info = dict(roles=roles, edges=edges, reach=reach, T=T, Z=zone_len(reach, T, margin), n=n, call=call)
    for c in range(channels):
        if edges[c]:
            zone_condition(x[c], edges[c], reach, T)
    x.setflags(write=False)
    return x, info


def zone_condition(row, e, reach, T):
    """the condition on one zoned row, from its samples: each SILENT and QUIET zone holds at least 1024 consecutive samples n
    whose window [n - (T - 1) - reach, n + reach] meets nothing louder than the zone"""
    a, q, b, c = e["a"], e["q"], e["b"], e["c"]
    mag = np.abs(np.asarray(row, dtype=np.float64))
    assert 0 < a < q < b < b + BURST < c < len(row), e
    assert not mag[a:q].any(), "SILENT zone is not silent"
    assert mag[q:b].max() <= QUIET and mag[b + BURST:c].max() <= QUIET and mag[q:b].any() and mag[b + BURST:c].any()
    assert mag[:a].max() > 0.5 and mag[b:b + BURST].max() > 0.5 and mag[c:].max() > 0.5, "a LOUD zone is not loud"
    assert b + BURST <= e["cut"] < c, "the call boundary lies outside the second QUIET zone"
    lo, hi = T - 1 + reach, reach
    for name, z0, z1, level, first_clean in (("SILENT", a, q, 0.0, a), ("QUIET before the burst", q, b, QUIET, a),
                                              ("QUIET behind the burst", b + BURST, c, QUIET, b + BURST)):
        n0, n1 = max(z0, first_clean + lo), z1 - hi                   # samples n0 .. n1 - 1 see [first_clean, z1) only
        assert n1 - n0 >= MARGIN, f"{name}: {n1 - n0} samples beyond the reach of anything louder, {MARGIN} are needed"
        assert mag[n0 - lo:n1 + hi].max() <= level, name


def exchanged(oracle, x, info, seed):
    """the rows of x with the neighbours of the zoned rows exchanged: loud <-> silent, quiet -> loud (another draw of the
    generator).  Returns (x2, kept): the zoned rows are kept as they are"""
    other = oracle.synth_f32(x.shape[0], x.shape[1], seed=seed + 7919)
    x2 = np.array(x)
    kept = []
    for c, role in enumerate(info["roles"]):
        if role == "zoned":
            kept.append(c)
        elif role == "loud":
            x2[c] = 0
        else:
            x2[c] = other[c]
    assert kept and len(kept) < x.shape[0]
    return x2, kept


# ------------------------------------------------------------------------------------------------ the limit
def window_energy(x, lo, hi):
    """E[r, n] = sum of x[r, n - lo .. n + hi]^2 (samples outside the row are zero), float64.  A running sum over a row that
    holds 1 and 2^-20 loses the quiet samples, so the squares are summed in bands of 2^8 by their exponent, the smallest band
    first: a window's sum is accurate to about 2^-28 of its smallest term's band, and exactly 0 where every sample is 0"""
    x2 = np.asarray(x, dtype=np.float64) ** 2
    rows, n = x2.shape
    idx = np.arange(n)
    i0, i1 = np.clip(idx - lo, 0, n), np.clip(idx + hi + 1, 0, n)
    band = np.where(x2 > 0, -np.frexp(x2)[1] // 8, -1)
    E = np.zeros((rows, n))
    for k in sorted(set(np.unique(band)) - {-1}, reverse=True):
        cs = np.concatenate([np.zeros((rows, 1)), np.cumsum(np.where(band == k, x2, 0.0), axis=1)], axis=1)
        E += np.take_along_axis(cs, np.broadcast_to(i1, (rows, n)), 1) - np.take_along_axis(cs, np.broadcast_to(i0, (rows, n)), 1)
    return E


def level_limit(x, h, nfft, reach):
    """[rows, n + T - 1]: the limit of every sample of the stream x and its flush tail.  h: [T], or [rows, T] (a bank)"""
    h = np.asarray(h, dtype=np.float64)
    T = h.shape[-1]
    l1 = np.sum(np.abs(h), axis=-1)
    E = window_energy(sc.padded(np.asarray(x, dtype=np.float32), T), T - 1 + reach, reach)
    return 8.0 * U * np.log2(nfft) * (l1[:, None] if h.ndim == 2 else l1) * np.sqrt(E)


# ------------------------------------------------------------------------------------------------ the check
def level_check(got, ref, limit, what, zoned=None):
    """ec.sample_check against the per-sample limit.  Prints the worst ratio overall and among the tight samples (0 < limit <
    1e-6), fails on any non-zero output where the limit is 0, and requires at least 1024 tight and 1024 zero-limit samples
    in every row of `zoned`.  Returns (worst ratio, worst tight ratio)"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    limit = np.broadcast_to(np.asarray(limit, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    zero = limit == 0
    tight = (limit > 0) & (limit < TIGHT)
    assert not ref[zero].any(), f"{what}: the reference is not zero where the limit is"
    err = np.abs(got - ref)
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, limit))
    worst, worst_tight = float(np.max(ratio)), float(np.max(ratio[tight])) if tight.any() else 0.0
    bad0 = np.argwhere(zero & (got != 0))
    print(f"{what}: worst ratio {worst:.3g}, on the {int(tight.sum())} tight samples {worst_tight:.3g}; "
          f"{len(bad0)} non-zero among {int(zero.sum())} zero-limit samples")
    for c in (zoned or []):
        assert tight[c].sum() >= MARGIN and zero[c].sum() >= MARGIN, \
            f"{what}: row {c} has {int(tight[c].sum())} tight and {int(zero[c].sum())} zero-limit samples, {MARGIN} are needed"
    assert np.isfinite(got).all(), f"{what}: NaN or Inf in the output"
    assert len(bad0) == 0, (f"{what}: {len(bad0)} non-zero outputs where the limit is 0, first at row {bad0[0][0]} index "
                            f"{bad0[0][1]}: {got[tuple(bad0[0])]:.3g}")
    ec.sample_check(got, ref, limit, what)
    return worst, worst_tight


def burst_snr(got, ref, info, what, rows=None):
    """measured, not asserted: rms(reference) / rms(error) over the QUIET samples that lie within the reach of the burst but
    whose own taps do not touch it, a zoned row at a time.  rows: {zoned input row: output row} (the matrix)"""
    out = []
    for i, e in enumerate(info["edges"]):
        if not e or (rows is not None and i not in rows):
            continue
        c = i if rows is None else rows[i]
        T, reach = info["T"], info["reach"]
        sel = np.r_[max(e["q"] + T - 1, e["b"] - reach):e["b"], e["b"] + BURST + T - 1:min(e["c"], e["b"] + BURST + T - 1 + reach)]
        if not len(sel):
            continue                                                   # a time-domain kernel reaches nothing but its taps
        err = np.asarray(got, dtype=np.float64)[c, sel] - ref[c, sel]
        snr = float(np.sqrt(np.mean(ref[c, sel] ** 2)) / max(np.sqrt(np.mean(err ** 2)), 1e-300))
        print(f"{what}: row {c}: signal / error = {snr:.3g} ({20 * np.log10(snr):.1f} dB) on the {len(sel)} quiet samples "
              "within reach of the burst")
        out.append(snr)
    return out


# ------------------------------------------------------------------------------------------------ the models
def _seen(x, lo, hi, s0, s1, keep):
    """x[:, lo:hi] as the call [s0, s1) reads it: zero before the history's `keep` samples and from the call's end on"""
    out = np.zeros((x.shape[0], hi - lo), np.float32)
    a, b = max(lo, s0 - keep, 0), min(hi, s1, x.shape[1])
    if b > a:
        out[:, a - lo:b - lo] = x[:, a:b]
    return out


def _spectrum(h, nfft):
    """DFT of the taps ([T] or [rows, T]) in complex64, rows kept"""
    return np.fft.fft(np.atleast_2d(np.asarray(h, dtype=np.float32).astype(np.float64)), nfft, axis=1).astype(np.complex64)


def _pair(xa, xb, H):
    """one complex transform of two real blocks: (ya, yb), complex64 throughout"""
    z = np.fft.fft((xa + 1j * xb).astype(np.complex64), axis=1).astype(np.complex64)
    y = np.fft.ifft((z * H).astype(np.complex64), axis=1).astype(np.complex64)
    return y.real.astype(np.float32), y.imag.astype(np.float32)


def _store(out, y, lo, hi, s1):
    hi = min(hi, s1)
    if hi > lo:
        out[:, lo:hi] = y[:, :hi - lo]


def model_direct(x, h):
    """time-domain kernels and time-domain flushes: float32 products summed in float32, oldest tap first"""
    x = np.asarray(x, dtype=np.float32)
    h = np.atleast_2d(np.asarray(h, dtype=np.float32))
    T = h.shape[1]
    xz = np.concatenate([np.zeros((x.shape[0], T - 1), np.float32), x, np.zeros((x.shape[0], T - 1), np.float32)], axis=1)
    n = x.shape[1] + T - 1
    y = np.zeros((x.shape[0], n), np.float32)
    for k in range(T - 1, -1, -1):
        y += h[:, k:k + 1] * xz[:, T - 1 - k:T - 1 - k + n]
    return y


def _direct_tail(out, x, h):
    T = np.shape(h)[-1]
    if T > 1:
        out[:, x.shape[1]:] = model_direct(x[:, -min(x.shape[1], T - 1):], h)[:, -(T - 1):]


def model_consecutive(x, h, nfft, overlap, call, fault=None):
    """the segment walk and the 2048 / 4096 / 8192 rungs: a job is two consecutive blocks of V = nfft - overlap new samples in
    one transform, jobs start over with every call, the flush is time-domain.  h: [T] or [rows, T].  fault "halo": block A's
    overlap taken from in front of the previous block A (the other sub-stream's carried rows)"""
    x = np.asarray(x, dtype=np.float32)
    T, V, O = np.shape(h)[-1], nfft - overlap, overlap
    H = _spectrum(h, nfft)
    n = x.shape[1]
    out = np.empty((x.shape[0], n + T - 1), np.float32)
    for s0 in range(0, n, call):
        s1 = min(s0 + call, n)
        for s in range(s0, s1, 2 * V):
            xa, xb = _seen(x, s - O, s + V, s0, s1, T - 1), _seen(x, s + V - O, s + 2 * V, s0, s1, T - 1)
            if fault == "halo":
                xa[:, :O] = _seen(x, s - V - O, s - V, s0, s1, T - 1)
            ya, yb = _pair(xa, xb, H)
            _store(out, ya[:, O:], s, s + V, s1)
            _store(out, yb[:, O:], s + V, s + 2 * V, s1)
    _direct_tail(out, x, h)
    return out


def sb_window(job):
    """ols_sb_window(job) of ols_superblock.h"""
    return job * SB["OLS_SB_VALID"] - SB["OLS_SB_HALO"] if job < SB["OLS_SB_FULL_JOBS"] else SB["OLS_SB_REGION"] - SB_NFFT


def model_superblock(x, h, call, fault=None):
    """the super-block walk: job i is block i of region 0 (real) with block i of region 1 (imaginary), OLS_SB_REGION later;
    the 11th job is short (its first 256 samples zero, its last 512 stored).  fault "halo": the two sub-streams' carried
    overlaps exchanged"""
    x = np.asarray(x, dtype=np.float32)
    T = np.shape(h)[-1]
    unit, region, halo, jobs, full = (SB[k] for k in ("OLS_SB_UNIT", "OLS_SB_REGION", "OLS_SB_HALO", "OLS_SB_JOBS",
                                                      "OLS_SB_FULL_JOBS"))
    H = _spectrum(h, SB_NFFT)
    n = x.shape[1]
    out = np.empty((x.shape[0], n + T - 1), np.float32)
    for s0 in range(0, n, call):
        s1 = min(s0 + call, n)
        for base in range(s0, s1, unit):
            for job in range(jobs):
                w = [base + r * region + sb_window(job) for r in (0, 1)]
                blk = [_seen(x, w[r], w[r] + SB_NFFT, s0, s1, T - 1) for r in (0, 1)]
                carry = halo if job < full else 2 * halo              # samples in front of the stored ones
                if job == full:
                    blk[0][:, :halo] = 0
                    blk[1][:, :halo] = 0
                if fault == "halo":
                    keep = blk[0][:, carry - halo:carry].copy()
                    blk[0][:, carry - halo:carry] = blk[1][:, carry - halo:carry]
                    blk[1][:, carry - halo:carry] = keep
                ya, yb = _pair(blk[0], blk[1], H)
                _store(out, ya[:, carry:], w[0] + carry, w[0] + SB_NFFT, s1)
                _store(out, yb[:, carry:], w[1] + carry, w[1] + SB_NFFT, s1)
    _direct_tail(out, x, h)
    return out


def model_partitioned(x, h, N, call, fault=None):
    """LLZ_FIR_ALGO_PARTITIONED and its bank: per call of K blocks Z_q = DFT(X_q + j X_{q+Kh}), Kh = ceil(K / 2), block q and
    q + Kh from the real and imaginary part of IDFT(sum_p Z_{q-p} H_p), p ascending in complex64; the flush is a call of T - 1
    zeros.  h: [T] or [rows, T].  fault "halo": the older half of the imaginary part's window taken from the real part's"""
    x = np.asarray(x, dtype=np.float32)
    hh = np.atleast_2d(np.asarray(h, dtype=np.float32).astype(np.float64))
    T, B = hh.shape[1], N // 2
    P = -(-T // B)
    hp = np.zeros((hh.shape[0], P * B))
    hp[:, :T] = hh
    H = np.fft.fft(hp.reshape(hh.shape[0], P, B), N, axis=2).astype(np.complex64)          # [rows, P, N]
    n = x.shape[1]
    xz = sc.padded(x, T)
    out = np.empty((x.shape[0], n + T - 1), np.float32)
    spans = [(s0, min(s0 + call, n)) for s0 in range(0, n, call)] + ([(n, n + T - 1)] if T > 1 else [])
    for s0, s1 in spans:
        K = -(-(s1 - s0) // B)
        Kh = -(-K // 2)
        Z = {}
        for q in range(-(P - 1), Kh):
            xa = _seen(xz, s0 + (q - 1) * B, s0 + (q + 1) * B, s0, s1, T - 1)
            xb = _seen(xz, s0 + (q + Kh - 1) * B, s0 + (q + Kh + 1) * B, s0, s1, T - 1)
            if fault == "halo":
                xb[:, :B] = xa[:, :B]
            Z[q] = np.fft.fft((xa + 1j * xb).astype(np.complex64), axis=1).astype(np.complex64)
        for q in range(Kh):
            acc = np.zeros((x.shape[0], N), np.complex64)
            for p in range(P):
                acc = (acc + Z[q - p] * H[:, p]).astype(np.complex64)
            y = np.fft.ifft(acc, axis=1).astype(np.complex64)
            _store(out, y.real[:, B:].astype(np.float32), s0 + q * B, s0 + (q + 1) * B, s1)
            _store(out, y.imag[:, B:].astype(np.float32), s0 + (q + Kh) * B, s0 + (q + Kh + 1) * B, s1)
    return out


def model_ring(x, h, block, k=1):
    """the stream convolver: stream_checks.model, a ring of real-transform spectra"""
    return sc.model(x, h, block, k)


def model_matrix(x, h, block, k=1):
    """the matrix convolver: matrix_checks.model"""
    return mc.model(x, h, block, k)


# ------------------------------------------------------------------------------------------------ the cases
TIME, TIME_MFMA, OLS, PARTITIONED = 1, 3, 2, 7           # include/llz_fir.h; the host test compares them with llzlab_amd.capi
OLS_ALGO_OF = {nfft: algo for algo, nfft in zip(sorted(ec.OLS_ALGO), (1024, 2048, 4096, 8192))}


def part_nfft(T):
    """the transform size LLZ_FIR_ALGO_PARTITIONED picks (firm_part_nfft, llz_fir_host.c); the GPU test asserts it against
    partition_plan()"""
    n = 1024
    while n < 8192 and T > 4 * (n // 2):
        n *= 2
    return n


class Case:
    """one GPU case and its CPU model.  form: direct | consecutive | superblock | partitioned | ring | matrix"""

    def __init__(self, name, form, T, channels=6, nfft=0, overlap=0, call=0, reach=0, bounds=None, block=64, calls=None,
                 algo=None, bank=False, k=1, roles=None, seed=1):
        self.name, self.form, self.T, self.channels, self.nfft, self.overlap = name, form, T, channels, nfft, overlap
        self.call, self.reach, self.bounds, self.block, self.calls = call, reach, bounds or [(block, 0)], block, calls
        self.algo, self.bank, self.k, self.roles, self.seed = algo, bank, k, roles, seed
        self.margin = max(MARGIN, nfft + BURST)        # room for the planted leak from reach + T + nfft in front

    def __repr__(self):
        return self.name


def _cases():
    out = []
    td = 2 * 2048 + 77
    for algo, name, T in ((TIME, "time", 17), (TIME, "time", 601), (TIME_MFMA, "mfma", 32), (TIME_MFMA, "mfma", 601)):
        out.append(Case(f"{name}-T{T}", "direct", T, call=td, bounds=[(2048, 0)], block=2048, algo=algo, seed=T))
    job = ec.ols_job(1024, 257)
    out.append(Case("ols1024-seg-T257", "consecutive", 257, nfft=1024, overlap=256, call=8 * job + 17, reach=reach_consecutive(1024),
                    bounds=[(job, 0)], block=job // 2, algo=OLS, seed=257))
    sbb = [(SB["OLS_SB_UNIT"], 0), (SB["OLS_SB_UNIT"], SB["OLS_SB_REGION"]),
           (SB["OLS_SB_REGION"], SB["OLS_SB_FULL_JOBS"] * SB["OLS_SB_VALID"])]
    for T in (257, 33):
        out.append(Case(f"ols1024-superblock-T{T}", "superblock", T, channels=4, nfft=1024, overlap=256, call=2 * SB["OLS_SB_UNIT"],
                        reach=reach_superblock(), bounds=sbb, block=SB["OLS_SB_VALID"], calls=3, algo=OLS, seed=T))
    out.append(Case("ols1024-superblock-ragged-T257", "superblock", 257, channels=4, nfft=1024, overlap=256,
                    call=SB["OLS_SB_UNIT"] + SB["OLS_SB_REGION"] + 769, reach=reach_superblock(), bounds=sbb, block=SB["OLS_SB_VALID"],
                    algo=OLS, seed=769))
    for nfft, _, overlaps in ec.OLS_INSTANCES[1:]:
        for ov in (overlaps[0], overlaps[-1]):
            job = 2 * (nfft - ov)
            out.append(Case(f"ols{nfft}-O{ov}", "consecutive", ov + 1, nfft=nfft, overlap=ov, call=3 * job + 17,
                            reach=reach_consecutive(nfft), bounds=[(job, 0)], block=job // 2, algo=OLS_ALGO_OF[nfft], seed=nfft + ov))
    job = ec.ols_job(1024, 257)
    out.append(Case("bank-ols1024-T257", "consecutive", 257, nfft=1024, overlap=256, call=8 * job + 17, reach=reach_consecutive(1024),
                    bounds=[(job, 0)], block=job // 2, algo=OLS, bank=True, seed=258))
    for bank in (False, True):
        for T in (2049, 6146):
            N = part_nfft(T)
            for K in (8, 9):
                out.append(Case(f"{'pbank' if bank else 'partitioned'}-T{T}-K{K}", "partitioned", T, nfft=N, call=K * (N // 2),
                                reach=reach_partitioned(K, N // 2), bounds=[(N // 2, 0)], block=N // 2, algo=PARTITIONED, bank=bank,
                                seed=T + K))
    for block, T in ((64, 65), (512, 513), (4096, 8200)):
        for k in (1, 3):
            out.append(Case(f"stream-B{block}-T{T}-k{k}", "ring", T, nfft=2 * block, call=k * block, reach=reach_ring(block),
                            bounds=[(block, 0)], block=block, k=k, seed=T + k))
    out.append(Case("matrix-B256-T700", "matrix", 700, channels=3, nfft=512, call=256, reach=reach_ring(256), bounds=[(256, 0)],
                    block=256, roles=["loud", "zoned", "silent"], seed=700))
    return out


CASES = _cases()
MATRIX_OUTPUTS = 2


def case_taps(case):
    """dense taps that weigh their ends (edge_checks.dense_taps).  A bank: a set per channel, the quiet row (or, without one,
    the first zoned row) holding the set with the largest l1 norm.  The matrix: [2, 3, T] with path (1, 0) all zero"""
    T = case.T
    if case.form == "matrix":
        h = np.stack([np.stack([ec.dense_taps(T, seed=100 * o + i) for i in range(case.channels)]) for o in range(MATRIX_OUTPUTS)])
        h[1, 0] = 0
        return h
    if not case.bank:
        return ec.dense_taps(T, seed=T)
    h = np.stack([ec.dense_taps(T, seed=1000 + c) * (1 + (c % 4) / 4) for c in range(case.channels)])
    h = h.astype(np.float32).astype(np.float64)
    roles = case.roles or default_roles(case.channels)
    want = roles.index("quiet") if "quiet" in roles else roles.index("zoned")
    top = int(np.argmax(np.sum(np.abs(h), axis=1)))
    h[[want, top]] = h[[top, want]]
    return h


def case_signal(oracle, case):
    """(x, info) of the case, computed once"""
    def make():
        calls = case.calls or level_calls(case.reach, case.T, case.call, case.bounds, case.block,
                                          (case.roles or default_roles(case.channels)).count("zoned"), case.margin)
        if case.form in ("ring", "matrix"):
            P = sc.partitions(case.T, case.block)
            calls = max(calls, -(-2 * (P + case.k - 1) // case.k) + 1)           # the ring twice around
        return level_signal(oracle, case.channels, calls * case.call, case.reach, case.T, case.seed, call=case.call,
                            bounds=case.bounds, block=case.block, roles=case.roles, margin=case.margin)
    return sc.cached(("level-x", case.name), make)


def fir_rows(oracle, xz, h):
    """the oracle's time-domain FIR of the rows of xz, float64: h [T] for all rows or [rows, T]"""
    h = np.asarray(h, dtype=np.float64)
    if h.ndim == 1:
        return oracle.fir_batch_f32_mt(xz, h, threads=16)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(16) as ex:
        return np.concatenate(list(ex.map(lambda c: oracle.fir_batch_f32(xz[c:c + 1], np.ascontiguousarray(h[c])),
                                          range(xz.shape[0]))), axis=0)


def fir_any(oracle, x, h):
    """reference of the stream and its flush tail for shared taps, a bank or the matrix ([outputs, inputs, T])"""
    h = np.asarray(h, dtype=np.float64)
    xz = sc.padded(np.asarray(x, dtype=np.float32), h.shape[-1])
    if h.ndim < 3:
        return fir_rows(oracle, xz, h)
    return np.stack([sum(fir_rows(oracle, xz, h[o])[i] for i in range(h.shape[1]) if h[o, i].any()) for o in range(h.shape[0])])


def tail_A(oracle, x, h):
    """[rows, T - 1]: |h| applied to |x| on the flush tail, where only the last T - 1 samples count"""
    T = np.shape(h)[-1]
    m = min(x.shape[1], T - 1)
    return fir_rows(oracle, sc.padded(np.abs(x[:, -m:]), T), np.abs(h))[:, m:m + T - 1]


def case_limit(oracle, case, x, h, reach=None):
    """[rows or outputs, n + T - 1]: level_limit on the frames of the transform forms, direct_limit on the time-domain
    kernels' frames and on every flush tail; the matrix: the sum over an output's inputs"""
    reach = case.reach if reach is None else reach
    T, n = case.T, x.shape[1]
    if case.form == "matrix":
        lim = np.zeros((h.shape[0], n + T - 1))
        for o in range(h.shape[0]):
            for i in range(h.shape[1]):
                lim[o] += level_limit(x[i:i + 1], h[o, i], case.nfft, reach)[0]
        # the tails: the direct-form limit alone
        for o in range(h.shape[0]):
            lim[o, n:] = sum(ec.direct_limit(tail_A(oracle, x[i:i + 1], h[o, i])[0], T) for i in range(h.shape[1]) if h[o, i].any())
        return lim
    if case.form == "direct":
        return ec.direct_limit(fir_rows(oracle, sc.padded(np.abs(x), T), np.abs(h)), T)
    lim = np.array(level_limit(x, h, case.nfft, reach))
    lim[:, n:] = ec.direct_limit(tail_A(oracle, x, h), T)
    return lim


def case_data(oracle, case):
    """x, info, taps, reference and limit of a case, computed once and shared, never modified"""
    def make():
        x, info = case_signal(oracle, case)
        h = case_taps(case)
        ref = fir_any(oracle, x, h)
        lim = case_limit(oracle, case, x, h)
        for a in (ref, lim):
            a.setflags(write=False)
        return dict(x=x, info=info, h=h, ref=ref, limit=lim, zoned=zoned_outputs(case, info, h))
    return sc.cached(("level-data", case.name), make)


def zoned_outputs(case, info, h):
    """the rows of the output that are held to the 1024-sample conditions: the zoned rows; of the matrix, the outputs whose
    only connected inputs are zoned or silent"""
    if case.form != "matrix":
        return [c for c, r in enumerate(info["roles"]) if r == "zoned"]
    return [o for o in range(h.shape[0])
            if all(info["roles"][i] != "loud" for i in range(h.shape[1]) if h[o, i].any())]


def run_model(case, x, h, fault=None):
    if case.form == "direct":
        return model_direct(x, h)
    if case.form == "consecutive":
        return model_consecutive(x, h, case.nfft, case.overlap, case.call, fault)
    if case.form == "superblock":
        return model_superblock(x, h, case.call, fault)
    if case.form == "partitioned":
        return model_partitioned(x, h, case.nfft, case.call, fault)
    assert fault is None
    return model_ring(x, h, case.block, case.k) if case.form == "ring" else model_matrix(x, h, case.block, case.k)
