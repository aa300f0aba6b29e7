"""GPU: the real spectrum product of the 1024-point overlap-save FIR (ols_filter<K> in llzlab_amd/csrc/kernels/ols_walk.hpp).
Taps that are symmetric about tap c = 32 K, K = 1..4 (65, 129, 193, 257 taps: the designed filters), are filtered with the real
spectrum of the taps centred at index 0, and every block comes out K register rows early.  Modelled on
test_fir_superblock_gpu.py: NaN-filled 32 KB-aligned planes, the `ols_superblock` tune, two streamed calls (the second one's
first halo is the history), oracle.fir_batch_f32 on the concatenated stream under rms_check (absolute and relative RMS <= 1e-5),
nothing stored behind a row's n samples.  Every case asks the launcher for the walk (llzs_fir_ols_superblock) and the handle for
K (llz_fir_filter_mc_real_rows), so that no case passes on the other form."""
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
TAPS_OF_K = {1: 65, 2: 129, 3: 193, 4: 257}


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


def designed(T):
    """the library's own low-pass of T taps (Kaiser window): symmetric, also after the cast to float32"""
    h = filters.fir_design("lpf", T, 0.23, win=filters.KAISER)
    assert len(h) == T
    return h


def one_ulp_off(T):
    """the designed taps as float32 with one tap in front of the centre moved by one ulp: no longer a mirror image"""
    h = designed(T).astype(np.float32)
    h[T // 2 - 7] = np.nextafter(h[T // 2 - 7], np.float32(np.inf))
    assert h[T // 2 - 7] != h[T // 2 + 7]
    return h.astype(np.float64)


def pitched(L, f, xin, y, n):
    rc = L.llz_fir_filter_mc_pitched(f.handle, C.c_void_p(xin.data_ptr()), C.c_void_p(y.data_ptr()), n, xin.stride(0), y.stride(0))
    assert rc == n, capi.last_error()


def check_case(dev, oracle, L, x, taps, n, pitch, what, K, superblock=True, tune=None, flush=False):
    """x [channels, 2 n] host: two calls of n samples on planes of `pitch` floats per row; the walk and K are asserted"""
    channels = x.shape[0]
    h = taps.astype(np.float32).astype(np.float64)
    T = len(h)
    tail = np.zeros((channels, T - 1), np.float32)
    ref = oracle.fir_batch_f32(np.ascontiguousarray(np.concatenate([x, tail], axis=1) if flush else x), h)
    with capi.tuned(**dict(tune or {}, ols_superblock=1)):
        f = filters.FirFilterMC(channels, n, taps, algo=OLS)
        assert f.algo == OLS
        xin, y = plane(dev, channels, pitch), plane(dev, channels, pitch)
        took = L.llzs_fir_ols_superblock(C.c_void_p(xin.data_ptr()), C.c_void_p(y.data_ptr()), channels, n, pitch, pitch, T)
        assert took == (1 if superblock else 0), f"{what}: the launcher takes walk {took}"
        assert f.real_rows() == K, f"{what}: the handle takes K = {f.real_rows()}, not {K}"
        outs = []
        for o in (0, n):
            xin[:, :n] = torch.from_numpy(np.ascontiguousarray(x[:, o:o + n])).to(dev)
            y.fill_(float("nan"))
            pitched(L, f, xin, y, n)
            torch.cuda.synchronize()
            yh = y.cpu().numpy()
            assert np.isnan(yh[:, n:]).all(), f"{what}: stores behind the row's {n} samples"
            outs.append(yh[:, :n])
        if flush:
            outs.append(f.flush(np.full((channels, T - 1), np.nan, np.float32)))
        f.close()
    got = np.concatenate(outs, axis=1)
    assert np.isfinite(got).all(), what
    err, rel = rms_check(got, ref, what)
    print(f"{what}: K {K} rms {err:.3g} rel {rel:.3g}")
    if flush:
        rms_check(got[:, 2 * n:], ref[:, 2 * n:], what + " (the flushed tail alone)")


@pytest.mark.parametrize("n,pitch", [(UNIT, UNIT), (2 * UNIT + REGION + 777, 3 * UNIT), (UNIT + 100, 2 * UNIT)])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_super_block_walk(dev, oracle, L, K, n, pitch):
    """3 channels (a wave with an idle half): one whole unit; a ragged last unit with a short region 1; region 1 absent"""
    x = oracle.synth_f32(3, 2 * n, seed=1000 * K + n % 997)
    check_case(dev, oracle, L, x, designed(TAPS_OF_K[K]), n, pitch, f"super-block K={K} n={n}", K)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_segment_walk(dev, oracle, L, K):
    """5 channels x 20001 on rows of 20011 floats: unaligned, so the segment walk, forced or not"""
    n = 20001
    x = oracle.synth_f32(5, 2 * n, seed=50 + K)
    check_case(dev, oracle, L, x, designed(TAPS_OF_K[K]), n, n + 10, f"segment K={K}", K, superblock=False)


@pytest.mark.parametrize("superblock", [True, False])
def test_one_ulp_of_asymmetry_takes_the_complex_product(dev, oracle, L, superblock):
    """257 taps of which one is one float32 ulp off its mirror image: K = 0 on both walks, the same limit"""
    n = UNIT + 100 if superblock else 20001
    pitch = 2 * UNIT if superblock else n + 10
    x = oracle.synth_f32(3 if superblock else 5, 2 * n, seed=7 + superblock)
    check_case(dev, oracle, L, x, one_ulp_off(257), n, pitch, f"one ulp off, superblock={superblock}", 0, superblock=superblock)


@pytest.mark.parametrize("tune,K", [(dict(ols_real_product=0), 0), (None, 4)])
def test_tune_selects_the_product(dev, oracle, L, tune, K):
    """the same 257 symmetric taps and input under ols_real_product = 0 and without: both within the limit of the oracle"""
    n = UNIT + 100
    x = oracle.synth_f32(3, 2 * n, seed=99)
    check_case(dev, oracle, L, x, designed(257), n, 2 * UNIT, f"tune {tune}", K, tune=tune)


def test_flush_after_the_real_product(dev, oracle, L):
    """llz_fir_filter_mc_flush behind two K = 4 calls: the 256 samples the stream still owes, against the oracle's tail"""
    n = UNIT + 100
    x = oracle.synth_f32(3, 2 * n, seed=123)
    check_case(dev, oracle, L, x, designed(257), n, 2 * UNIT, "flush", 4, flush=True)
