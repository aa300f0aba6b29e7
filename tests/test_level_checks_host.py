"""CPU: the level tests' own pieces (tests/level_checks.py).  Every case of test_fir_levels_gpu.py runs here through the
float32 / complex64 model of its pairing scheme and must stay inside the same limits, with the 1024-sample conditions met, so
a machine without a GPU already shows that the references, the reaches and the limits fit together.  Then the checks are shown
to see what they are for: per model, an understated reach, a 1e-7 x[n - reach - T - nfft] leak into a quiet zone, a single
1e-30 in a silent zone and the carried halo of one sub-stream taken from the other must each FAIL level_check."""
import numpy as np
import pytest

from tests import edge_checks as ec
from tests import level_checks as lc

BY_NAME = {c.name: c for c in lc.CASES}
# one case per model for the planted faults; an understated reach: the consecutive pair's where the partner is 8192 away, an
# eighth elsewhere
FAULT_CASES = ["ols1024-seg-T257", "ols1024-superblock-T257", "partitioned-T2049-K9", "stream-B512-T513-k3", "matrix-B256-T700"]
PAIRED = FAULT_CASES[:3]


def checked(case, d, y, limit=None, what=""):
    """frames and flush tail of one run under level_check; the 1024-sample conditions hold on the frames"""
    n = d["x"].shape[1]
    limit = d["limit"] if limit is None else limit
    a = lc.level_check(y[:, :n], d["ref"][:, :n], limit[:, :n], f"{case.name}{what} frames", zoned=d["zoned"])
    b = lc.level_check(y[:, n:], d["ref"][:, n:], limit[:, n:], f"{case.name}{what} flush")
    return a, b


@pytest.fixture(scope="module")
def modelled(oracle):
    """the model's output per case, computed once and read-only"""
    cache = {}

    def get(case):
        if case.name not in cache:
            d = lc.case_data(oracle, case)
            y = lc.run_model(case, d["x"], d["h"])
            assert y.shape == d["ref"].shape and y.dtype == np.float32
            y.setflags(write=False)
            cache[case.name] = y
        return cache[case.name]
    return get


def test_constants_are_the_library_s():
    from llzlab_amd import capi
    assert (lc.TIME, lc.TIME_MFMA, lc.OLS, lc.PARTITIONED) == (capi.FIR_ALGO_TIME, capi.FIR_ALGO_TIME_MFMA,
                                                                capi.FIR_ALGO_OVERLAP_SAVE, capi.FIR_ALGO_PARTITIONED)
    assert lc.OLS_ALGO_OF == {1024: capi.FIR_ALGO_OVERLAP_SAVE, 2048: capi.FIR_ALGO_OVERLAP_SAVE_2048,
                              4096: capi.FIR_ALGO_OVERLAP_SAVE_4096, 8192: capi.FIR_ALGO_OVERLAP_SAVE_8192}
    assert lc.SB["OLS_SB_UNIT"] == 2 * lc.SB["OLS_SB_REGION"] and lc.SB["OLS_SB_HALO"] + lc.SB["OLS_SB_VALID"] == lc.SB_NFFT
    assert lc.reach_superblock() == 9216 and lc.reach_consecutive(1024) == 2048 and lc.reach_partitioned(9, 1024) == 7168


def test_window_energy_keeps_quiet_samples_next_to_loud_ones():
    """a running sum in float64 loses 2^-40 against 1e4; the banded sum does not, and silence sums to exactly 0"""
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (2, 30000)).astype(np.float32)
    x[:, 10000:20000] *= np.float32(lc.QUIET)
    x[1, 20000:25000] = 0
    E = lc.window_energy(x, 300, 200)
    exact = np.array([[float(np.sum(x[r, max(0, n - 300):n + 201].astype(np.float64) ** 2)) for n in (5, 9990, 12000, 19900, 22000, 29990)]
                      for r in range(2)])
    np.testing.assert_allclose(E[:, [5, 9990, 12000, 19900, 22000, 29990]], exact, rtol=1e-7, atol=0)
    assert E[1, 22000] == 0 and E[0, 12000] < 1e-9


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_zone_condition(oracle, case):
    """every SILENT and QUIET zone is at least 2 reach + T + 1024 long and holds 1024 samples beyond the reach of anything
    louder; the call boundary lies in the second QUIET zone: within T - 1 of the burst in one row, more than reach + T behind
    it in another; the edges sit on a boundary of the call, one sample behind one and elsewhere"""
    x, info = lc.case_signal(oracle, case)
    edges = [e for e in info["edges"] if e]
    assert edges and x.shape[1] % case.call == 0
    for c, e in enumerate(info["edges"]):
        if e:
            lc.zone_condition(x[c], e, case.reach, case.T)
            assert min(e["q"] - e["a"], e["b"] - e["q"], e["c"] - e["b"] - lc.BURST) >= lc.zone_len(case.reach, case.T)
    behind = [e["cut"] - e["b"] - lc.BURST for e in edges]
    assert 0 < behind[0] < case.T - 1
    on = [[k for k, b in enumerate(case.bounds) if lc._on(e[name], e["shift"], case.call, b)] for e in edges for name in "aqc"]
    assert all(on), "an edge lies off every boundary"
    assert {k for ks in on for k in ks} == set(range(len(case.bounds))), "a kind of boundary is never met"
    if len(edges) >= 3:
        assert behind[1] > case.reach + case.T and [e["shift"] for e in edges[:2]] == [0, 1] and edges[2]["shift"] > 1
    if case.form in ("ring", "matrix"):
        P = -(-case.T // case.block)
        assert x.shape[1] // case.block >= 2 * (P + case.k - 1), "the ring is not taken twice around"


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_model_stays_inside_the_limits(oracle, modelled, case):
    d = lc.case_data(oracle, case)
    (worst, tight), _ = checked(case, d, modelled(case))
    lc.burst_snr(modelled(case), d["ref"], d["info"], case.name, rows={1: 1} if case.form == "matrix" else None)
    if case.form != "direct":
        assert worst < 0.01, "the float32 model of a transform form sits far inside the norm bound"


# ------------------------------------------------------------------------------------------------ planted faults
def tight_after_burst(case, d):
    """per zoned input row: (row, output row, first of the 64 samples reach + T + nfft behind the burst, that distance): QUIET
    samples beyond the reach of the burst"""
    out = []
    for i, e in enumerate(d["info"]["edges"]):
        if e:
            off = case.reach + case.T + max(case.nfft, lc.BURST)     # a time-domain kernel has no transform: behind the burst's tail
            assert e["b"] + off + lc.BURST + case.reach <= e["c"]
            out.append((i, 1 if case.form == "matrix" else i, e["b"] + off, off))
    return out


@pytest.mark.parametrize("name", FAULT_CASES + ["time-T601"])
def test_a_leak_from_the_burst_fails(oracle, modelled, name):
    """1e-7 x[n - reach - T - nfft] added to the quiet samples behind the burst, one row at a time"""
    case = BY_NAME[name]
    d = lc.case_data(oracle, case)
    for i, o, n0, off in tight_after_burst(case, d):
        y = np.array(modelled(case))
        sel = np.arange(n0, n0 + lc.BURST)
        assert np.all(d["limit"][o, sel] < lc.TIGHT) and np.all(d["limit"][o, sel] > 0)
        y[o, sel] += (1e-7 * d["x"][i, sel - off]).astype(np.float32)
        with pytest.raises(AssertionError, match="over their limit"):
            checked(case, d, y, what=f" leak row {o}")


@pytest.mark.parametrize("name", FAULT_CASES + ["time-T601"])
def test_one_denormal_sized_value_in_silence_fails(oracle, modelled, name):
    case = BY_NAME[name]
    d = lc.case_data(oracle, case)
    for i, e in enumerate(d["info"]["edges"]):
        if e:
            o = 1 if case.form == "matrix" else i
            n0 = e["a"] + case.T - 1 + case.reach + 5
            assert d["limit"][o, n0] == 0
            y = np.array(modelled(case))
            y[o, n0] = 1e-30
            with pytest.raises(AssertionError, match="non-zero outputs where the limit is 0"):
                checked(case, d, y, what=f" 1e-30 row {o}")


@pytest.mark.parametrize("name", FAULT_CASES)
def test_an_understated_reach_fails(oracle, modelled, name):
    """the same output judged with too short a reach: the super-block walk with the consecutive pair's 2 nfft, every other
    form with an eighth of its own"""
    case = BY_NAME[name]
    d = lc.case_data(oracle, case)
    short = lc.reach_consecutive(case.nfft) if case.form == "superblock" else case.reach // 8
    limit = lc.case_limit(oracle, case, d["x"], d["h"], reach=short)
    with pytest.raises(AssertionError, match="non-zero outputs where the limit is 0|over their limit"):
        checked(case, d, modelled(case), limit=limit, what=f" reach {short}")


@pytest.mark.parametrize("name", PAIRED)
def test_a_halo_from_the_other_sub_stream_fails(oracle, name):
    case = BY_NAME[name]
    d = lc.case_data(oracle, case)
    y = lc.run_model(case, d["x"], d["h"], fault="halo")
    with pytest.raises(AssertionError, match="non-zero outputs where the limit is 0|over their limit"):
        checked(case, d, y, what=" halo")


def test_a_halo_fault_confined_to_quiet_samples_is_seen(oracle, modelled):
    """what the whole-row limits could not see: the super-block walk's halo fault kept only where the row is QUIET, 2^-20 of
    full scale, passes edge_checks.rms_check and fails level_check"""
    case = BY_NAME["ols1024-superblock-T257"]
    d = lc.case_data(oracle, case)
    bad = lc.run_model(case, d["x"], d["h"], fault="halo")
    y = np.array(modelled(case))
    n = d["x"].shape[1]
    e = d["info"]["edges"][0]
    sel = slice(e["q"] + case.reach + case.T, e["b"] - case.reach)
    y[0, sel] = bad[0, sel]
    assert np.any(y[0, sel] != modelled(case)[0, sel])
    ec.rms_check(y[0, :n], d["ref"][0, :n], "quiet halo fault under the whole-row gate")
    with pytest.raises(AssertionError, match="over their limit"):
        checked(case, d, y, what=" quiet halo")
