"""Shared pieces of the FIR / resampler edge tests (test_edge_checks_host.py, test_fir_edges_gpu.py, test_fir_full_size_gpu.py,
test_resample_probe_gpu.py): tap sets that carry weight at their ends, the limits a result is held to, and the impulse probe
of the resampler's tap matrix.  Plain numpy; nothing here touches a GPU.

Why: a windowed sinc is ~1e-7 at its ends, so a whole-array RMS cannot see a kernel that loses its first or last taps or
reads the oldest overlap sample from the wrong place.  With the taps below one lost end tap costs 1e-2 .. 0.8 relative.

Limits (u = 2^-24, the unit round-off of float32), derived and not measured:
  * dense taps: the project's RMS gate, TOL = 1e-5 absolute and relative to rms(reference), unchanged;
  * sparse taps, direct-form kernels: |err_n| <= 4 (nnz + 1) u A_n, A_n = the same filter applied to |x| with |h|, nnz the
    non-zero taps: the worst case of any summation order over nnz products ((nnz + 1) u A_n to first order), times 4 for
    split-bf16 terms and a float-rounded gain;
  * sparse taps, overlap-save: |err_n| <= 8 u log2(nfft) sqrt(nfft) rms(x) ||h||_2: the norm bound of an FFT convolution over
    one block (forward transform, product, inverse: error ~ u log2(N) per transform in the block's norm
    sqrt(N) rms(x) ||h||_2); 1e-4 .. 5e-4 for 1024 .. 8192 points, where one misplaced sample costs about 1;
  * resampler probe: every output is one product a * gain * g, so |got - ref| <= 4 u |ref| (float-rounded tap, float-rounded
    gain, their product, the product with a) and got == 0 where ref == 0.
"""
import re

import numpy as np

TOL = 1e-5                  # RMS, north_star (tests/test_gpu_parity.py)
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ tap families
def dense_taps(T, seed):
    """default_rng(seed).standard_normal(T) at unit l2 norm, rounded to float32 (returned as float64).  A Gaussian draw can
    land near zero at an end, which would blind the test there: such a draw is refused and the next seed taken (both ends
    at least a quarter of the typical tap, 0.25 / sqrt(T))."""
    while True:
        h = np.random.default_rng(seed).standard_normal(T)
        h /= np.sqrt(np.sum(h * h))
        if min(abs(h[0]), abs(h[-1])) * np.sqrt(T) >= 0.25:
            return h.astype(np.float32).astype(np.float64)
        seed += 1000003


def two_ends_taps(T, s):
    """h[0] = 1, h[T-1] = s: y[n] = x[n] + s x[n-T+1]"""
    assert T >= 2 and s in (1, -1)
    h = np.zeros(T)
    h[0], h[T - 1] = 1.0, float(s)
    return h


def one_delta_taps(T, k):
    """a single 1.0 at index k: the output is the input delayed by k"""
    h = np.zeros(T)
    h[k] = 1.0
    return h


def sparse_families(T):
    """[(name, taps)]: two-ends with both signs and deltas at k = 0, T-1 and one interior index, as far as T has room"""
    out = []
    if T >= 2:
        out += [("two-ends+", two_ends_taps(T, 1)), ("two-ends-", two_ends_taps(T, -1))]
    for k in sorted({0, T - 1, (2 * T) // 3}):
        out.append((f"delta@{k}", one_delta_taps(T, k)))
    return out


# ------------------------------------------------------------------------------------------------ checks
def rms_check(got, ref, what):
    got = np.asarray(got, dtype=np.float64)
    err = float(np.sqrt(np.mean((got - ref) ** 2)))
    rel = err / max(float(np.sqrt(np.mean(ref ** 2))), 1e-30)
    print(f"{what}: rms {err:.3g} rel {rel:.3g}")
    assert err <= TOL and rel <= TOL, f"{what}: rms {err:.3g} rel {rel:.3g}"
    return err, rel


def direct_limit(A, nnz):
    """per-sample limit of a direct-form kernel; A = |h| applied to |x| (array)"""
    return 4.0 * (nnz + 1) * U * A


def ols_limit(nfft, x_rms, h_norm):
    """per-sample limit of an nfft-point overlap-save (a scalar)"""
    return 8.0 * U * np.log2(nfft) * np.sqrt(nfft) * x_rms * h_norm


def sample_check(got, ref, limit, what, period=None):
    """|got - ref| <= limit at every sample (limit: scalar or array like ref); a failure names the worst sample: channel,
    index and, with `period` (the kernel's job length), the index within the job"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    over = err - limit
    w = np.unravel_index(int(np.argmax(over)), err.shape)
    lim_w = float(np.broadcast_to(limit, err.shape)[w])
    where = f"channel {w[0]} index {w[-1]}" if err.ndim == 2 else f"index {w[-1]}"
    if period:
        where += f" (index mod {period} = {w[-1] % period})"
    print(f"{what}: max err {float(err.max()):.3g}, worst against its limit: {float(err[w]):.3g} of {lim_w:.3g} at {where}")
    assert over[w] <= 0, (f"{what}: {int(np.count_nonzero(over > 0))} samples over their limit; worst {float(err[w]):.3g} > "
                          f"{lim_w:.3g} at {where}: got {float(got[w]):.9g} ref {float(ref[w]):.9g}")
    return float(err.max())


def fir_ref(x, h, prev=None):
    """float64 FIR of the rows of x with zero (or `prev`: [channels, T-1]) history: (y, A) with A = |h| applied to |x|"""
    x = np.asarray(x, dtype=np.float64)
    T = len(h)
    head = np.zeros((x.shape[0], T - 1)) if prev is None else np.asarray(prev, dtype=np.float64)
    xx = np.concatenate([head, x], axis=1)
    y = np.zeros(x.shape)
    A = np.zeros(x.shape)
    n = x.shape[1]
    for k in np.flatnonzero(h):
        seg = xx[:, T - 1 - k:T - 1 - k + n]
        y += h[k] * seg
        A += abs(h[k]) * np.abs(seg)
    return y, A


# ------------------------------------------------------------------------------------------------ overlap-save instances
# algo value (include/llz_fir.h) -> transform points, the rung's smallest tap count, the overlaps instantiated: the 18 kernel
# instances of OLS_RUNGS (llzlab_amd/csrc/kernels/fir_ols.hip); the host self-test compares this list with that file
OLS_ALGO = {2: "OVERLAP_SAVE", 4: "OVERLAP_SAVE_2048", 5: "OVERLAP_SAVE_4096", 6: "OVERLAP_SAVE_8192"}
OLS_INSTANCES = [
    # (nfft, min_taps, overlaps)
    (1024, 1, (256,)),
    (2048, 2, (512, 1024)),
    (4096, 2, (512, 768, 1024, 1536, 2048, 2560, 3072)),
    (8192, 2, (1536, 2304, 2560, 3072, 3584, 4096, 5120, 6144)),
]


def ols_cases():
    """[(nfft, overlap, flt_len, which)]: every instance at flt_len = overlap + 1 ('last': its last tap meets the oldest
    overlap sample) and at the smallest flt_len that selects it ('first': previous overlap + 2, or the rung's min_taps)"""
    out = []
    for nfft, min_taps, overlaps in OLS_INSTANCES:
        for i, ov in enumerate(overlaps):
            out.append((nfft, ov, overlaps[i - 1] + 2 if i else min_taps, "first"))
            out.append((nfft, ov, ov + 1, "last"))
    return out


def ols_job(nfft, T):
    """new samples per job (two blocks) of the instance that takes T taps: the smallest overlap that holds T - 1 samples"""
    overlaps = next(r[2] for r in OLS_INSTANCES if r[0] == nfft)
    return 2 * (nfft - min(ov for ov in overlaps if ov >= T - 1))


def ols_rungs_in_source(text):
    """[(nfft, min_taps, overlaps)] as written in the OLS_RUNGS table of fir_ols.hip"""
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr\s+int\s+(\w+)\s*=\s*(\d+)\s*;", text)}
    body = text[text.index("const ols_rung OLS_RUNGS[]"):]
    body = body[:body.index("\n};")]
    body = re.sub(r"//[^\n]*", "", body)
    rungs = []
    for m in re.finditer(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*\"", body):
        rest = body[m.end():]
        lst = re.search(r"(\d+)\s*,\s*\{([\w\s,]+)\}\s*,\s*\{\s*kfn", rest)
        vals = tuple(int(v) if v.isdigit() else consts[v] for v in (s.strip() for s in lst.group(2).split(",")))
        assert len(vals) == int(lst.group(1)), (vals, lst.group(1))
        rungs.append((int(m.group(1)), int(m.group(2)), vals))
    return rungs


# ------------------------------------------------------------------------------------------------ resampler probe
def rs_index_map(n_out, L, M):
    """output i reads x[pos[i] - k] through matrix entry (phase[i], k): pos = floor(i M / L) = floor(f M / L) + t M for
    i = t L + f"""
    i = np.arange(n_out, dtype=np.int64)
    return (i * M) // L, i % L


def rs_probe_signal(L, M, Q, channels=3, min_impulses=96):
    """[channels, n_in] float32 of unit impulses with amplitudes 1.0 and -0.75 in turn, one at every residue modulo M, more
    than Q apart (so no output sees two of them), the channels shifted against each other; n_in is a whole number of
    periods and leaves Q samples and a period behind the last impulse.  Returns (x, positions per channel)."""
    stride = ((Q + 1 + M - 1) // M) * M + 1                  # > Q and = 1 modulo M: consecutive impulses walk the residues
    count = M * ((min_impulses + M - 1) // M)
    last = (channels - 1) * (M + 3) + (count - 1) * stride
    n_in = ((last + Q + 2 * M) // M + 1) * M
    x = np.zeros((channels, n_in), dtype=np.float32)
    pos = []
    for c in range(channels):
        p = c * (M + 3) + np.arange(count, dtype=np.int64) * stride
        x[c, p] = np.where((np.arange(count) + c) % 2 == 0, 1.0, -0.75).astype(np.float32)
        pos.append(p)
    return x, pos


def rs_probe_cuts(positions, n_in, M, Q):
    """call lengths (whole periods) that cut the signal inside the response of an impulse a third and two thirds along, with
    a one-period call behind the first cut"""
    p = positions[0]
    cuts = []
    for start in (len(p) // 3, (2 * len(p)) // 3):
        # among the next M impulses (all residues), the one whose response a period boundary cuts nearest to its middle
        best = None
        for a in range(start, min(start + M, len(p))):
            c = (int(p[a]) // M + 1) * M
            d = c - int(p[a])
            if 1 <= d <= Q - 1 and (best is None or abs(d - Q / 2) < best[0]):
                best = (abs(d - Q / 2), c)
        assert best is not None, (start, M, Q)
        cuts.append(best[1])
    edges = sorted({cuts[0], cuts[0] + M, cuts[1], n_in} - {0})
    edges = [e for e in edges if e <= n_in]
    lens = [b - a for a, b in zip([0] + edges[:-1], edges)]
    assert sum(lens) == n_in and all(v > 0 and v % M == 0 for v in lens), lens
    return lens


def rs_straddles(positions, lens, L, M, Q):
    """how many impulse responses lie on both sides of a call boundary: outputs of one impulse before and after the cut"""
    count = 0
    edges = np.cumsum(lens)[:-1]
    for p in np.concatenate(positions):
        for e in edges:
            # outputs with pos in [p, p + Q - 1]; the cut at input e is the output e L / M, whose pos is e
            if p < e <= p + Q - 1:
                count += 1
    return count


def rs_hits(positions, n_out, L, M, Q):
    """bool [L, Q]: the matrix entries (f, k) that some impulse reaches in some output below n_out"""
    pos, phase = rs_index_map(n_out, L, M)
    hit = np.zeros((L, Q), dtype=bool)
    for p in np.concatenate(positions):
        lo = int(np.searchsorted(pos, p, "left"))
        hi = int(np.searchsorted(pos, p + Q - 1, "right"))
        hit[phase[lo:hi], pos[lo:hi] - p] = True
    return hit


def rs_probe_check(got, ref, what):
    """every output holds at most one product: |got - ref| <= 4 u |ref| where ref != 0, got == 0 where ref == 0"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    zero = ref == 0
    bad0 = np.flatnonzero((got != 0) & zero)
    err = np.abs(got - ref)
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, np.abs(ref)))
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{what}: worst |got - ref| / |ref| = {float(ratio[w]) / U:.3g} u at {w}; {bad0.size} non-zero outputs where ref == 0")
    assert bad0.size == 0, f"{what}: {bad0.size} outputs non-zero where the reference is zero, first at flat index {bad0[0]}"
    assert ratio[w] <= 4 * U, (f"{what}: {int(np.count_nonzero(ratio > 4 * U))} outputs over 4 u; worst {float(ratio[w]) / U:.3g} u "
                              f"at {w}: got {float(got[w]):.9g} ref {float(ref[w]):.9g}")


def rs_numpy(x, mat, L, M, gain):
    """float32 restatement of the batch resampler with zero history: y[i] = gain sum_k x[pos - k] mat[phase][k], float32
    taps and gain, float32 result"""
    x = np.asarray(x, dtype=np.float32)
    n_in = x.shape[1]
    n_out = n_in * L // M
    Q = mat.shape[1]
    pos, phase = rs_index_map(n_out, L, M)
    idx = pos[:, None] - np.arange(Q)[None, :]
    g = mat.astype(np.float32).astype(np.float64)[phase] * (idx >= 0)
    idx = np.maximum(idx, 0)
    out = np.empty((x.shape[0], n_out), dtype=np.float32)
    for c in range(x.shape[0]):
        out[c] = (np.sum(x[c].astype(np.float64)[idx] * g, axis=1) * float(np.float32(gain))).astype(np.float32)
    return out
