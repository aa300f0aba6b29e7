"""GPU: the super-block walk of the 1024-point overlap-save FIR (k_fir_ols_chain_f32; geometry in
llzlab_amd/csrc/kernels/ols_superblock.h), forced through the `ols_superblock` tune on shapes far smaller than the headline
batch that takes it by itself.  Rows come from 32 KB-aligned planes through llz_fir_filter_mc_pitched, so that a ragged length
keeps the alignment the walk needs.  Every case makes two streamed calls (the second one's first halo is the history), is
compared with oracle.fir_batch_f32 on the concatenated stream under the limit of test_fir_ols_headline_shape_full_length
(rms_check: absolute and relative RMS <= 1e-5), and asks the launcher which walk it took (llzs_fir_ols_superblock), so that
a case cannot pass on the other walk.  What lies behind a row's n samples in the output plane must stay untouched.

A super-block is 16384 samples (two regions of 8192), 11 jobs; a wave holds two, a workgroup eight."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests.test_gpu_parity import rms_check  # noqa: E402

UNIT, REGION = 16384, 8192
ALIGN = 32 * 1024
OLS = filters.FIR_ALGO_OVERLAP_SAVE


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


def plane(dev, channels, pitch, offset_bytes=0):
    """[channels, pitch] float32 of NaN whose first row starts offset_bytes behind a 32 KB boundary"""
    raw = torch.full((channels * pitch + ALIGN // 4 + 64,), float("nan"), dtype=torch.float32, device=dev)
    skip = ((-raw.data_ptr()) % ALIGN + offset_bytes) // 4
    p = raw[skip:skip + channels * pitch].view(channels, pitch)
    assert (p.data_ptr() - offset_bytes) % ALIGN == 0
    return p


def asym_taps(T, seed):
    """dense taps with no symmetry: a decaying noise burst, unit energy"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(T) * np.exp(-np.arange(T) / (0.4 * T + 1))
    return h / np.sqrt(np.sum(h * h))


def pitched(L, f, xin, y, n):
    rc = L.llz_fir_filter_mc_pitched(f.handle, C.c_void_p(xin.data_ptr()), C.c_void_p(y.data_ptr()), n, xin.stride(0), y.stride(0))
    assert rc == n, capi.last_error()


def check_case(dev, oracle, L, x, taps, n, pitch, what, superblock=True, tune=None, offset_bytes=0, channels_checked=None):
    """x [channels, 2 n] host: two calls of n samples on planes of `pitch` floats per row"""
    channels = x.shape[0]
    h = taps.astype(np.float32).astype(np.float64)
    sel = list(range(channels)) if channels_checked is None else channels_checked
    ref = oracle.fir_batch_f32(np.ascontiguousarray(x[sel]), h)
    with capi.tuned(**dict(tune or {}, ols_superblock=1)):
        f = filters.FirFilterMC(channels, n, taps, algo=OLS)
        assert f.algo == OLS
        xin, y = plane(dev, channels, pitch, offset_bytes), plane(dev, channels, pitch, offset_bytes)
        took = L.llzs_fir_ols_superblock(C.c_void_p(xin.data_ptr()), C.c_void_p(y.data_ptr()), channels, n, pitch, pitch, len(taps))
        assert took == (1 if superblock else 0), f"{what}: the launcher takes walk {took}"
        outs = []
        for o in (0, n):
            xin[:, :n] = torch.from_numpy(np.ascontiguousarray(x[:, o:o + n])).to(dev)
            y.fill_(float("nan"))
            pitched(L, f, xin, y, n)
            torch.cuda.synchronize()
            yh = y.cpu().numpy()
            assert np.isnan(yh[:, n:]).all(), f"{what}: stores behind the row's {n} samples"
            outs.append(yh[sel, :n])
        f.close()
    got = np.concatenate(outs, axis=1)
    assert np.isfinite(got).all(), what
    err, rel = rms_check(got, ref, what)
    print(f"{what}: rms {err:.3g} rel {rel:.3g}")


def test_one_super_block(dev, oracle, L):
    """1 channel x 16384: all 11 jobs of one unit, the short job on both sub-streams, the partner half idle"""
    x = oracle.synth_f32(1, 2 * UNIT, seed=41)
    check_case(dev, oracle, L, x, asym_taps(257, 1), UNIT, UNIT, "one unit")


@pytest.mark.parametrize("n", [UNIT - 1, UNIT + REGION, UNIT + REGION + 1, UNIT + REGION + 767, UNIT + REGION + 768,
                               UNIT + REGION + 769])
def test_ragged_region_1(dev, oracle, L, n):
    """3 channels on rows of 2 * 16384: a last super-block whose region 1 is absent (n = 16384 + 8192), starts (+ 1), ends
    inside its first block, at its end and in its second block (+ 767, + 768, + 769); n = 16383: one ragged unit per channel,
    an odd number of units against pairs of half-waves"""
    x = oracle.synth_f32(3, 2 * n, seed=n)
    check_case(dev, oracle, L, x, asym_taps(257, 2), n, 2 * UNIT, f"ragged n={n}")


@pytest.mark.parametrize("T", [2, 129, 257])
def test_tap_counts(dev, oracle, L, T):
    """short and full overlaps: the history of T - 1 samples in front of region 0 of the second call"""
    n = UNIT + REGION + 5
    x = oracle.synth_f32(2, 2 * n, seed=100 + T)
    check_case(dev, oracle, L, x, asym_taps(T, 3 + T), n, 2 * UNIT, f"{T} taps")


def test_boundary_impulses(dev, oracle, L):
    """unit impulses whose 257-tap tails cross the short block's store cut (7679 | 7680), its window start (7167 | 7168), the
    region boundary (8191 | 8192) and the super-block boundary (16383 | 16384), in both calls"""
    n = 2 * UNIT
    x = np.zeros((2, 2 * n), np.float32)
    for k, s in enumerate((7167, 7168, 7679, 7680, 8191, 8192, 16383, 16384)):
        for c in range(2):
            x[c, s] = 1.0 + 0.125 * k
            x[c, n + s + (REGION if c else 0)] = -1.0 - 0.125 * k       # second call; channel 1: the same cuts of region 1
    check_case(dev, oracle, L, x, asym_taps(257, 4), n, n, "boundary impulses")


def test_grid_stride_chain_across_units(dev, oracle, L):
    """1100 channels x 2 * 16384 under ols_wg_per_cu = 1: 2200 super-blocks on 2048 half-wave slots, so the short job's request
    for the next unit and its halos is used; spread channels against the oracle with a short filter"""
    channels, n = 1100, 2 * UNIT
    x = oracle.synth_f32(channels, 2 * n, seed=77)
    sel = [0, 1, 511, 512, 1023, 1024, 1025, 1098, 1099]
    check_case(dev, oracle, L, x, asym_taps(33, 5), n, n, "grid stride", tune=dict(ols_wg_per_cu=1), channels_checked=sel)


@pytest.mark.parametrize("pitch,offset_bytes", [(UNIT + 32, 0), (UNIT, 128)])
def test_unaligned_rows_take_the_segment_walk(dev, oracle, L, pitch, offset_bytes):
    """a pitch of 16384 + 32 floats, and a base 128 B behind the boundary: forced or not, the launcher keeps the segment walk"""
    x = oracle.synth_f32(3, 2 * UNIT, seed=pitch + offset_bytes)
    check_case(dev, oracle, L, x, asym_taps(257, 6), UNIT, pitch, f"fallback pitch={pitch} offset={offset_bytes}",
               superblock=False, offset_bytes=offset_bytes)


def test_pitched_call_refuses_what_it_cannot_take(dev, L):
    """llz_fir_filter_mc_pitched: a pitch below frame_len, another frame_len than the init's, host memory and overlapping spans
    are LLZ_ERR_ARG with a message; nothing is launched"""
    n = 4096
    f = filters.FirFilterMC(2, n, asym_taps(33, 7), algo=OLS)
    a, b = plane(dev, 2, 2 * n), plane(dev, 2, 2 * n)
    call = lambda x, y, m, pi, po: L.llz_fir_filter_mc_pitched(f.handle, C.c_void_p(x), C.c_void_p(y), m, pi, po)  # noqa: E731
    assert call(a.data_ptr(), b.data_ptr(), n, n - 1, 2 * n) == -1 and "pitch" in capi.last_error()
    assert call(a.data_ptr(), b.data_ptr(), n // 2, 2 * n, 2 * n) == -1
    host = np.zeros((2, 2 * n), np.float32)
    assert call(host.ctypes.data, b.data_ptr(), n, 2 * n, 2 * n) == -1 and "device memory" in capi.last_error()
    assert call(a.data_ptr(), a.data_ptr() + 4 * n, n, 2 * n, 2 * n) == -1 and "overlap" in capi.last_error()
    assert call(a.data_ptr(), b.data_ptr(), n, 2 * n, 2 * n) == n, capi.last_error()
    torch.cuda.synchronize()
    f.close()
