"""GPU: the FIR at full size (4096 channels x 2^20 samples) with every sample of every channel checked.  Two-ends taps
(h[0] = 1, h[T-1] = s) make the whole output checkable on the device: y[n] = x[n] + s x[n-T+1], formed in float64 by torch
in channel chunks and held to the overlap-save limit of tests/edge_checks.py.  A second call through the same handle checks
the streamed history."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import edge_checks as ec  # noqa: E402

CH, N = 4096, 1 << 20
CHUNK = 128                                                  # channels per float64 pass: 1 GiB per temporary


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def worst_sample(x, prev, y, T, s):
    """max over every sample of |y - (x + s shift(x, T-1))| with `prev` [CH, T-1] (or zeros) in front of x: (err, channel,
    index, got, ref), and the mean square of x"""
    worst = (-1.0, 0, 0, 0.0, 0.0)
    sq = 0.0
    for c0 in range(0, CH, CHUNK):
        xc = x[c0:c0 + CHUNK].double()
        ref = xc.clone()
        ref[:, T - 1:] += s * xc[:, :N - T + 1]
        if prev is not None:
            ref[:, :T - 1] += s * prev[c0:c0 + CHUNK].double()
        sq += float((xc * xc).sum())
        err = (y[c0:c0 + CHUNK].double() - ref).abs_()
        flat = int(err.argmax())
        c, i = divmod(flat, N)
        e = float(err[c, i])
        if not np.isfinite(e) or e > worst[0]:
            worst = (e, c0 + c, i, float(y[c0 + c, i]), float(ref[c, i]))
        if not bool(torch.isfinite(err).all()):
            worst = (float("inf"),) + worst[1:]
        del xc, ref, err
    return worst, sq / (CH * float(N))


@pytest.mark.parametrize("T,s,nfft,overlap", [(257, 1, 1024, 256), (3073, -1, 8192, 3072), (6145, 1, 8192, 6144)])
def test_fir_full_size_every_sample(dev, T, s, nfft, overlap):
    """the default launcher on the headline batch: 257 taps (1024-point chain form), 3073 and 6145 taps (8192 points on pairs
    of waves); two calls through one handle; a failure names the worst sample's channel, index and place within the job"""
    f = filters.FirFilterMC(CH, N, ec.two_ends_taps(T, s))
    assert f.algo == {1024: filters.FIR_ALGO_OVERLAP_SAVE, 8192: filters.FIR_ALGO_OVERLAP_SAVE_8192}[nfft]
    job = 2 * (nfft - overlap)
    x = torch.empty(CH, N, dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    prev = None
    for call in range(2):
        filters.synth_f32(x, seed=100 + T + call)
        y.fill_(float("nan"))
        f.filter(x, y)
        torch.cuda.synchronize()
        (err, c, i, got, ref), msq = worst_sample(x, prev, y, T, s)
        limit = ec.ols_limit(nfft, np.sqrt(msq), np.sqrt(2.0))
        print(f"T={T} call {call}: worst |err| {err:.3g} (limit {limit:.3g}) at channel {c} index {i} (index mod {job} = {i % job})")
        assert err <= limit, (f"T={T} call {call}: |err| {err:.3g} > {limit:.3g} at channel {c} index {i} "
                              f"(index mod job length {job} = {i % job}): got {got:.9g} ref {ref:.9g}")
        prev = x[:, N - (T - 1):].clone()
    f.close()
