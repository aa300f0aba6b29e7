"""GPU: every float32 path of the batch resampler probed tap by tap.  The taps are designed inside the library and are
~1e-7 at the ends of the prototype, so white noise under an RMS gate leaves about a sixth of a tap matrix unchecked.  Here
unit impulses (tests/edge_checks.py), one at every residue modulo M and more than Q apart, put a single product into each
output: every non-zero entry of the tap matrix shows up alone and is compared with the oracle's to 4 units of float32
round-off.  The signal is split into calls so that some responses straddle a call boundary."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests import edge_checks as ec  # noqa: E402

# path of rsm_choose (llz_resample_host.c) -> the override that reaches it, and its shapes; the first shape also runs at
# gains 2.5 and 0.37 and under white noise at gain 2.5; the ratios with a common factor (repeated and empty phases in the phase
# maps floor(f M / L)) run whole periods here and ragged calls in test_resample_ragged_gpu.py
PATHS = {
    "fir_mfma_f32": ({}, [(1, 3), (1, 2), (1, 5)]),
    "resample_dec_f32": ({"rs_dec_valu": 1}, [(1, 3), (1, 2), (1, 5)]),
    "resample_mfma_f32 phase-tile waves": ({"rs_mfma_form": -1}, [(147, 160), (160, 147), (441, 320), (320, 441), (20, 147), (294, 320), (150, 160)]),
    "resample_mfma_f32 period-tile waves": ({"rs_mfma_form": 1}, [(147, 160), (160, 147), (441, 320), (320, 441), (20, 147), (294, 320), (150, 160)]),
    "resample_f32": ({}, [(2, 3), (3, 2), (5, 3), (8, 7), (4, 6), (6, 4), (40, 64)]),
    "resample_f32 rs_generic=1": ({"rs_generic": 1}, [(147, 160)]),
    "resample_f32 rs_generic=2": ({"rs_generic": 2}, [(147, 160)]),
}
WINS = (po.BLACKMAN, po.HAMMING, po.KAISER)
CASES = [(path, L, M, 1.0) for path, (_t, shapes) in PATHS.items() for (L, M) in shapes] + \
        [(path, shapes[0][0], shapes[0][1], g) for path, (_t, shapes) in PATHS.items() for g in (2.5, 0.37)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def run_calls(dev, tune, x, lens, L, M, gain, win, oracle):
    """x through one handle in calls of lens[] inputs, the override in force from init to the last call"""
    ch = x.shape[0]
    with capi.tuned(**tune):
        r = filters.ResampleMC(ch, L, M, gain, win, filters.PCM_F32)
        info = oracle.rs_info(2, L, M, gain, win)
        assert r.Q == info["cols"] and np.array_equal(r.matrix(), info["matrix"])
        outs, o = [], 0
        for n_in in lens:
            n_out = r.out_len(n_in)
            xd = torch.from_numpy(np.ascontiguousarray(x[:, o:o + n_in])).to(dev)
            yd = torch.full((ch, n_out), float("nan"), dtype=torch.float32, device=dev)
            assert r.process(xd, yd) == n_out
            outs.append(yd.cpu().numpy())
            o += n_in
        r.close()
    return np.concatenate(outs, axis=1), info


@pytest.mark.parametrize("path,L,M,gain", CASES, ids=[f"{c[0].replace(' ', '_')}-{c[1]}:{c[2]}-g{c[3]}" for c in CASES])
def test_resample_f32_probe_every_tap(dev, oracle, path, L, M, gain):
    tune = PATHS[path][0]
    win = WINS[(L + M) % 3]
    info = oracle.rs_info(2, L, M, gain, win)
    mat, Q = info["matrix"], info["cols"]
    x, positions = ec.rs_probe_signal(L, M, Q)
    lens = ec.rs_probe_cuts(positions, x.shape[1], M, Q)
    assert ec.rs_straddles(positions, lens, L, M, Q) >= 2, "no response straddles a call boundary"
    ref = oracle.rs_batch_f32(x, L, M, gain, win)
    hit = ec.rs_hits(positions, ref.shape[1], L, M, Q)
    assert hit[mat != 0].all(), f"{np.count_nonzero((mat != 0) & ~hit)} non-zero taps of {np.count_nonzero(mat)} not probed"
    got, _ = run_calls(dev, tune, x, lens, L, M, gain, win, oracle)
    ec.rs_probe_check(got, ref, f"{path} {L}:{M} gain {gain} calls {lens}")
    # and in one call: the same samples
    got1, _ = run_calls(dev, tune, x, [x.shape[1]], L, M, gain, win, oracle)
    ec.rs_probe_check(got1, ref, f"{path} {L}:{M} gain {gain} one call")


@pytest.mark.parametrize("path", list(PATHS))
def test_resample_f32_white_noise_with_gain(dev, oracle, path):
    """gain 2.5 (folded into the band table of the matrix-core path, a float factor elsewhere) under the RMS gate"""
    tune, shapes = PATHS[path]
    L, M = shapes[0]
    win = WINS[(L + M) % 3]
    lens = [200 * M, M, 1037 * M, 49 * M]
    x = oracle.synth_f32(3, sum(lens), seed=L + 2 * M)
    got, _ = run_calls(dev, tune, x, lens, L, M, 2.5, win, oracle)
    ref = oracle.rs_batch_f32(x, L, M, 2.5, win)
    assert got.shape == ref.shape
    ec.rms_check(got, ref, f"{path} {L}:{M} gain 2.5 white noise")
