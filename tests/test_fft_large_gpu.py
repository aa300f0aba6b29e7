"""FFT above 4096 points on the GPU: llz_fft / llz_ifft bit-identical to the reference up to 2^24 points (the fixture of
tools/gen_golden_fft_large.py and the CPU oracle), the float32 batch within the tolerance of the <= 4096 tests, on a
torch stream, through the host staging path, past 2^31 floats, and beside a live 4096-point handle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import filters  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DOUBLE_SIZES = [1 << k for k in range(13, 21)] + [1 << 22, 1 << 24]
BATCH_SIZES = [1 << k for k in range(13, 21)] + [1 << 24]


@pytest.fixture(scope="module")
def dev():
    from llzlab_amd import capi
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def rel_rms(got, ref):
    return float(np.sqrt(np.mean(np.abs(got - ref) ** 2)) / np.sqrt(np.mean(np.abs(ref) ** 2)))


def cplx64(rng, count, n):
    return (rng.uniform(-1, 1, (count, n)) + 1j * rng.uniform(-1, 1, (count, n))).astype(np.complex64)


def test_fft_double_8192_vs_reference_fixture(dev):
    d = np.load(os.path.join(G, "fft_large.npz"), allow_pickle=False)
    f = filters.Fft(8192)
    assert np.array_equal(f.fft(d["x"]), d["fwd"])
    assert np.array_equal(f.ifft(d["fwd"]), d["inv"])
    f.close()


def _double_inputs(n, rng):
    yield "random", rng.standard_normal(n) + 1j * rng.standard_normal(n)
    if n <= (1 << 20):
        imp = np.zeros(n, dtype=np.complex128)
        imp[n // 3] = 1.0 - 0.5j
        yield "impulse", imp
        yield "large", (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 1e150


@pytest.mark.parametrize("n", DOUBLE_SIZES)
def test_fft_double_exact_vs_oracle(dev, oracle, n):
    rng = np.random.default_rng(n)
    f = filters.Fft(n)
    for what, z in _double_inputs(n, rng):
        assert np.array_equal(f.fft(z), oracle.fft(z)), f"{n} forward, {what}"
        assert np.array_equal(f.ifft(z), oracle.fft(z, inverse=True)), f"{n} inverse, {what}"
    f.close()


def _batch_check(oracle, fb, zd, z, count):
    fb.fft(zd, count)
    got = zd.cpu().numpy().view(np.complex64).reshape(count, -1)
    ref = np.stack([oracle.fft(row.astype(np.complex128)) for row in z])
    r = rel_rms(got, ref)
    assert r < 1e-6, f"forward rel rms {r:.3g}"
    fb.ifft(zd, count)
    back = zd.cpu().numpy().view(np.complex64).reshape(count, -1)
    e = float(np.sqrt(np.mean(np.abs(back - z) ** 2)))
    assert e < 1e-6, f"round trip rms {e:.3g}"


@pytest.mark.parametrize("n,count", [(n, c) for n in BATCH_SIZES for c in ((1,) if n == 1 << 24 else (1, 3, 7))])
def test_fft_batch_f32_vs_oracle(dev, oracle, n, count):
    rng = np.random.default_rng(n + count)
    z = cplx64(rng, count, n)
    zd = torch.from_numpy(z.view(np.float32).copy()).to(dev)
    fb = filters.FftBatch(n)
    _batch_check(oracle, fb, zd, z, count)
    fb.close()


def test_fft_batch_on_a_torch_stream(dev, oracle):
    n, count = 1 << 16, 3
    rng = np.random.default_rng(5)
    z = cplx64(rng, count, n)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        zd = torch.from_numpy(z.view(np.float32).copy()).to(dev, non_blocking=False)
    s.synchronize()
    fb = filters.FftBatch(n, stream=s)
    fb.fft(zd, count)
    s.synchronize()
    got = zd.cpu().numpy().view(np.complex64).reshape(count, n)
    assert rel_rms(got, np.stack([oracle.fft(row.astype(np.complex128)) for row in z])) < 1e-6
    fb.ifft(zd, count)
    s.synchronize()
    assert float(np.sqrt(np.mean(np.abs(zd.cpu().numpy().view(np.complex64).reshape(count, n) - z) ** 2))) < 1e-6
    fb.close()


def test_fft_batch_host_array_through_staging(dev, oracle):
    n, count = 1 << 15, 3
    rng = np.random.default_rng(6)
    z = cplx64(rng, count, n)
    h = z.copy()
    fb = filters.FftBatch(n)
    fb.fft(h.view(np.float32), count)
    assert rel_rms(h, np.stack([oracle.fft(row.astype(np.complex128)) for row in z])) < 1e-6
    fb.ifft(h.view(np.float32), count)
    assert float(np.sqrt(np.mean(np.abs(h - z) ** 2))) < 1e-6
    fb.close()


def test_fft_batch_beyond_2_31_floats(dev, oracle):
    """16385 transforms of 65536 points: the last one starts at float 2^31; only the first and the last are checked"""
    n, count = 1 << 16, 16385
    assert (count - 1) * n * 2 == 1 << 31
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    zd = torch.rand(count * n * 2, dtype=torch.float32, device=dev, generator=gen) * 2 - 1
    ends = [zd[:2 * n].cpu().numpy().view(np.complex64).copy(), zd[-2 * n:].cpu().numpy().view(np.complex64).copy()]
    fb = filters.FftBatch(n)
    fb.fft(zd, count)
    torch.cuda.synchronize()
    got = [zd[:2 * n].cpu().numpy().view(np.complex64), zd[-2 * n:].cpu().numpy().view(np.complex64)]
    for g, z in zip(got, ends):
        assert rel_rms(g, oracle.fft(z.astype(np.complex128))) < 1e-6
    fb.close()
    del zd
    torch.cuda.empty_cache()


def test_boundary_4096_and_8192_handles_live_together(dev, oracle):
    rng = np.random.default_rng(7)
    f4, f8 = filters.Fft(4096), filters.Fft(8192)
    b4, b8 = filters.FftBatch(4096), filters.FftBatch(8192)
    for f, n in ((f4, 4096), (f8, 8192), (f4, 4096)):
        z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        assert np.array_equal(f.fft(z), oracle.fft(z)), n
        assert np.array_equal(f.ifft(z), oracle.fft(z, inverse=True)), n
    for fb, n in ((b4, 4096), (b8, 8192), (b4, 4096), (b8, 8192)):
        z = cplx64(rng, 3, n)
        zd = torch.from_numpy(z.view(np.float32).copy()).to(dev)
        _batch_check(oracle, fb, zd, z, 3)
    for h in (f4, f8, b4, b8):
        h.close()
