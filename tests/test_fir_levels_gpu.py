"""GPU: every FIR form on level steps, a burst and silence (tests/level_checks.py; the CPU side is test_level_checks_host.py).
Each case streams its signal through one handle in equal calls and then the flush, outputs preset to NaN, and every sample of
every channel is compared with the oracle's time-domain FIR under level_check: a limit taken from the energy within the reach
of the sample's transform (0, and so an output of +-0 exactly, in silence beyond the reach), direct_limit on the time-domain
kernels and on every flush tail.  The call boundary lies in a QUIET zone: within T - 1 samples of the burst in one row (the
history carries it), more than reach + T behind it in another.

Independence: each case runs a second time with the neighbours of the zoned rows exchanged (loud <-> silent, quiet -> loud);
the zoned rows must come out bit-identical.  The matrix: the loud input silenced, and the output that has no path from it.

Every case prints its worst ratio to the limit, overall and on the tight samples (limit below 1e-6), and -- measured, not
asserted -- the signal-to-error ratio of the quiet samples that share a transform with the burst.  Figures as recorded on an
MI355X: DESIGN.md, "FIR levels"."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import level_checks as lc  # noqa: E402
from tests import matrix_checks as mc  # noqa: E402
from tests import stream_checks as sc  # noqa: E402

ALIGN = lc.SB["OLS_SB_REGION"] * 4          # bytes of a region: the 32 KB the super-block walk wants of row bases and pitches


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    lib = capi.lib()
    lib.llzs_fir_ols_superblock.restype = C.c_int
    lib.llzs_fir_ols_superblock.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int]
    return lib


# ------------------------------------------------------------------------------------------------ the runners
def flushed(dev, f, rows):
    tail = torch.full((rows, f.flt_len - 1), float("nan"), dtype=torch.float32, device=dev)
    f.flush(tail)
    return tail.cpu().numpy()


def run_batch(dev, L, case, x, h):
    """FirFilterMC / FirBankMC of the case's algo in calls of case.call, then the flush"""
    make = filters.FirBankMC if case.bank else filters.FirFilterMC
    f = make(x.shape[0], case.call, h, algo=case.algo)
    assert f.algo == case.algo, (f.algo, case.algo)
    if case.form == "partitioned":
        plan = f.partition_plan(case.call)
        assert plan[:2] == (case.nfft, -(-case.T // (case.nfft // 2))) and case.call % (case.nfft // 2) == 0, plan
    outs = []
    for o in range(0, x.shape[1], case.call):
        xi = torch.from_numpy(np.ascontiguousarray(x[:, o:o + case.call])).to(dev)
        yi = torch.full_like(xi, float("nan"))
        f.filter(xi, yi)
        outs.append(yi.cpu().numpy())
    outs.append(flushed(dev, f, x.shape[0]))
    f.close()
    return np.concatenate(outs, axis=1)


def plane(dev, channels, pitch):
    """[channels, pitch] float32 of NaN whose rows start on 32 KB boundaries"""
    raw = torch.full((channels * pitch + ALIGN // 4,), float("nan"), dtype=torch.float32, device=dev)
    skip = ((-raw.data_ptr()) % ALIGN) // 4
    p = raw[skip:skip + channels * pitch].view(channels, pitch)
    assert p.data_ptr() % ALIGN == 0 and pitch * 4 % ALIGN == 0
    return p


def run_superblock(dev, L, case, x, h):
    """the super-block walk, forced as in test_fir_superblock_gpu.py: the ols_superblock tune, 32 KB-aligned planes, the
    pitched call; the launcher must answer that it takes that walk.  What lies behind a row's samples stays NaN"""
    channels, n = x.shape[0], case.call
    pitch = -(-n * 4 // ALIGN) * (ALIGN // 4)
    with capi.tuned(ols_superblock=1):
        f = filters.FirFilterMC(channels, n, h, algo=case.algo)
        assert f.algo == case.algo
        xin, y = plane(dev, channels, pitch), plane(dev, channels, pitch)
        took = L.llzs_fir_ols_superblock(C.c_void_p(xin.data_ptr()), C.c_void_p(y.data_ptr()), channels, n, pitch, pitch, case.T)
        assert took == 1, f"{case.name}: the launcher takes walk {took}"
        outs = []
        for o in range(0, x.shape[1], n):
            xin[:, :n] = torch.from_numpy(np.ascontiguousarray(x[:, o:o + n])).to(dev)
            y.fill_(float("nan"))
            rc = L.llz_fir_filter_mc_pitched(f.handle, C.c_void_p(xin.data_ptr()), C.c_void_p(y.data_ptr()), n, pitch, pitch)
            assert rc == n, capi.last_error()
            torch.cuda.synchronize()
            yh = y.cpu().numpy()
            assert np.isnan(yh[:, n:]).all(), f"{case.name}: stores behind the row's {n} samples"
            outs.append(yh[:, :n])
        outs.append(flushed(dev, f, channels))
        f.close()
    return np.concatenate(outs, axis=1)


def run_ring(dev, L, case, x, h):
    return sc.device(dev, x, h, case.block, case.k)


def run_matrix(dev, L, case, x, h):
    return mc.device(dev, x, h, case.block, case.k)


RUN = dict(direct=run_batch, consecutive=run_batch, partitioned=run_batch, superblock=run_superblock, ring=run_ring,
           matrix=run_matrix)


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_levels(dev, oracle, L, case):
    d = lc.case_data(oracle, case)
    x, h, ref, limit, info = d["x"], d["h"], d["ref"], d["limit"], d["info"]
    n = x.shape[1]
    got = RUN[case.form](dev, L, case, x, h)
    assert got.shape == ref.shape and got.dtype == np.float32
    # measured, not asserted: the quiet samples that share a transform with the burst
    lc.burst_snr(got, ref, info, case.name, rows={1: 1} if case.form == "matrix" else None)
    lc.level_check(got[:, :n], ref[:, :n], limit[:, :n], f"{case.name} frames", zoned=d["zoned"])
    lc.level_check(got[:, n:], ref[:, n:], limit[:, n:], f"{case.name} flush")

    # independence: the neighbours exchanged, the rows kept bit-identical
    if case.form == "matrix":
        x2, kept = np.array(x), [o for o in range(h.shape[0]) if not h[o, 0].any()]
        assert info["roles"][0] == "loud" and kept
        x2[0] = 0
    else:
        x2, kept = lc.exchanged(oracle, x, info, case.seed)
    got2 = RUN[case.form](dev, L, case, x2, h)
    for c in kept:
        diff = np.flatnonzero(sc.bits(got[c]) != sc.bits(got2[c]))
        assert diff.size == 0, (f"{case.name}: row {c} changes in {diff.size} samples with its neighbours, first at {diff[0]}: "
                                f"{got[c, diff[0]]:.9g} -> {got2[c, diff[0]]:.9g}")
    print(f"{case.name}: rows {kept} bit-identical with their neighbours exchanged")
