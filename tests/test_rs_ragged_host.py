"""CPU self-test of tests/rs_ragged_checks.py and of the host predicates the ragged-call GPU tests rely on: the call plans
have the properties their docstring promises, at every ratio; the int16 reference on a zero-padded input is the prefix of the
reference on a longer signal, bit for bit; the float32 limit accepts a correct float32 result and rejects one lost tap; and
the library's own *_fits answers send each ratio to the entry the GPU tests mean to reach."""
from math import gcd

import numpy as np
import pytest

from llzlab_amd import capi
from oracle import pyoracle as po
from tests import edge_checks as ec
from tests import rs_ragged_checks as rr

# L:M -> (Q, resample_mfma_f32 fits, resample_i16x fits) with Blackman taps
FITS = {(294, 320): (47, 1, 1), (320, 294): (45, 1, 1), (150, 160): (47, 1, 1), (160, 150): (45, 1, 1), (4, 6): (67, 0, 1),
        (2, 4): (89, 0, 1), (6, 4): (45, 0, 1), (8, 6): (45, 0, 1), (40, 64): (71, 0, 1), (48, 32): (45, 0, 1)}


def test_ratio_lists_and_the_table_agree():
    assert set(FITS) == set(rr.RATIOS) and all(gcd(L, M) > 1 for L, M in rr.RATIOS)


@pytest.mark.parametrize("L,M", rr.RATIOS, ids=[f"{L}:{M}" for L, M in rr.RATIOS])
def test_call_plan_properties(L, M):
    g, need = gcd(L, M), rr.min_primary(L, M)
    step = M // g
    lens, kinds = rr.call_plan(L, M, need)
    assert kinds == ["a", "b", "c", "d", "e"] + (["a1"] if g == 2 else []) + ["f", "c"], kinds
    assert all(n > 0 and n % step == 0 for n in lens)
    w = dict()
    for kind, row in zip(kinds, rr.walk(lens, L, M)):
        w.setdefault(kind, []).append(row)
    for kind in ("a", "d", "a1"):
        for r0, r1, n_in, n_out in w.get(kind, []):
            assert r0 == 0 and r1 != 0 and n_out % L == r1 * (L // g) != 0, (kind, r0, r1)
    for kind in ("b", "f"):
        (r0, r1, n_in, n_out), = w[kind]
        assert r0 != 0 and r1 == 0, (kind, r0, r1)
    assert w["b"][0][3] > 2 * 2048, "(b) spans several tiles of the fallback kernels"
    for r0, r1, n_in, n_out in w["c"]:
        assert r0 == 0 and r1 == 0 and n_in % M == 0 and n_out % L == 0 and (n_in // M) % 2 == 1
    (r0, r1, n_in, n_out), = w["e"]
    assert r0 != 0 and n_in == step
    assert w["e"][0][1] == 0 if g == 2 else w["e"][0][1] != 0
    for kind in ("a", "c", "d"):
        assert all(row[2] >= need for row in w[kind]), kind
    assert lens[-1] >= need and sum(lens) % M == 0
    # overshoot of a whole-period store behind (a) and (d): L - n_out % L
    over_a, over_d = L - w["a"][0][3] % L, L - w["d"][0][3] % L
    assert over_a == L // g, "the smallest overshoot the ratio allows"
    if g > 2:
        assert w["a"][0][1] != w["d"][0][1] and over_d == (g - 1) * (L // g)
    if L // g <= 2:
        assert over_a in (1, 2)
    # the entries a correct handle takes: the primary exactly for whole-period calls from a boundary
    want = rr.expected_entries(lens, L, M, "P", "F")
    assert want == ["P" if k == "c" else "F" for k in kinds]
    assert sum(lens) <= 120000, "a case stays small"


@pytest.mark.parametrize("L,M", rr.RATIOS, ids=[f"{L}:{M}" for L, M in rr.RATIOS])
def test_ref_i16_is_the_prefix_of_a_longer_stream(oracle, L, M):
    """zero padding behind the signal against a longer NON-zero signal: the first n L / M outputs are bit-equal"""
    step = M // gcd(L, M)
    frame = oracle.rs_info(2, L, M, 1.0, po.BLACKMAN)["bytes_in"] // 2
    n = (frame + frame // 3) // step * step + step
    assert n % frame != 0 and (n * L) % M == 0
    long = oracle.synth_i16(2, 3 * frame, seed=L + M)
    long[1] = (long[1].astype(np.int32) * 2).clip(-32768, 32767).astype(np.int16)
    assert np.any(long[:, n:2 * frame] != 0)
    whole = oracle.rs_batch_i16(long, L, M, 1.0, po.BLACKMAN)
    got = rr.ref_i16(oracle, long[:, :n], L, M, 1.0, po.BLACKMAN)
    assert got.shape == (2, n * L // M) and got.dtype == np.int16
    assert np.array_equal(got, whole[:, :n * L // M])
    # whole frames: the plain frame loop, nothing padded or cut
    assert np.array_equal(rr.ref_i16(oracle, long, L, M, 1.0, po.BLACKMAN), whole)


@pytest.mark.parametrize("L,M,gain", [(4, 6, 1.0), (150, 160, 2.5)])
def test_f32_limit_accepts_float32_and_rejects_a_lost_tap(oracle, L, M, gain):
    info = oracle.rs_info(2, L, M, gain, po.BLACKMAN)
    mat, Q = info["matrix"], info["cols"]
    step = M // gcd(L, M)
    x = oracle.synth_f32(2, 401 * step, seed=L + M)           # a ragged length
    assert (x.shape[1] * L // M) % L != 0
    ref = rr.ref_f32(oracle, x, L, M, gain, po.BLACKMAN)
    lim = rr.f32_limit(x, mat, L, M, gain)
    assert lim.shape == ref.shape and np.all(lim >= 0) and np.all(lim[:, Q:] > 0)       # (0 where no tap meets a sample yet)
    got = ec.rs_numpy(x, mat, L, M, gain)
    worst = ec.sample_check(got, ref, lim, f"rs_numpy {L}:{M}")
    assert worst > 0
    # the limit is a few float32 round-offs of the sum of magnitudes, never a loose one: a single lost mid tap of one phase fails
    cut = mat.copy()
    cut[1, Q // 2] = 0.0
    assert mat[1, Q // 2] != 0
    with pytest.raises(AssertionError):
        ec.sample_check(ec.rs_numpy(x, cut, L, M, gain), ref, lim, "one tap lost")
    # first principles, sample by sample at a few places
    pos, phase = ec.rs_index_map(ref.shape[1], L, M)
    for i in (0, Q, ref.shape[1] - 1):
        a = sum(abs(mat[phase[i], k]) * abs(float(x[1, pos[i] - k])) for k in range(Q) if pos[i] - k >= 0) * abs(gain)
        assert np.isclose(lim[1, i], 4 * (Q + 1) * ec.U * a, rtol=1e-12)


def test_probe_cuts_fall_inside_responses_off_a_period_boundary(oracle):
    for L, M in [(294, 320), (150, 160), (4, 6), (6, 4), (40, 64)]:
        Q = oracle.rs_info(2, L, M, 1.0, po.BLACKMAN)["cols"]
        x, positions = ec.rs_probe_signal(L, M, Q)
        lens = rr.probe_cuts(positions, x.shape[1], L, M, Q)
        rows = rr.walk(lens, L, M)
        entries = rr.expected_entries(lens, L, M, "P", "F")
        print(L, M, Q, lens, entries)
        assert entries.count("P") >= 1 and entries.count("F") >= 3 and M // gcd(L, M) in lens, (L, M, rows)
        assert sum(r[1] != 0 for r in rows) >= 2 and rows[-1][1] == 0
        assert ec.rs_straddles(positions, lens, L, M, Q) >= 4
        # and every non-zero tap is reached, as in the whole-period probe
        mat = oracle.rs_info(2, L, M, 1.0, po.BLACKMAN)["matrix"]
        assert ec.rs_hits(positions, x.shape[1] * L // M, L, M, Q)[mat != 0].all()


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


@pytest.mark.parametrize("L,M", rr.RATIOS, ids=[f"{L}:{M}" for L, M in rr.RATIOS])
def test_fits_predicates_send_each_ratio_to_its_entry(lib, oracle, L, M):
    """no kernel runs: the predicates are host arithmetic.  Q is the oracle's, with the window the GPU tests use."""
    Q = oracle.rs_info(2, L, M, 1.0, po.BLACKMAN)["cols"]
    want_q, want_mfma, want_i16x = FITS[(L, M)]
    assert Q == want_q
    assert lib.llzs_resample_mfma_f32_fits(L, M, Q) == want_mfma
    assert lib.llzs_resample_i16x_fits(L, M, Q) == want_i16x
    assert ((L, M) in rr.MFMA_RATIOS) == bool(want_mfma)


def test_last_entry_refuses_a_bad_handle(lib):
    assert lib.llz_resample_mc_last_entry(capi.BAD_HANDLE) is None
    assert lib.llz_resample_mc_last_entry(0) is None
