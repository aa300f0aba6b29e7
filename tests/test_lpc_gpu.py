"""Linear prediction on the MI355X: the llz_lpc handle against the reference's own results (tests/golden/lpc.npz), and the
batch path llz_lpc_mc against llz_autocorr_mc and the Python restatement of llz_levinson, bit for bit."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests.test_lpc_host import levinson_py  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 1234.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    capi.build()
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def expected(r, n, p):
    """float32(restatement((double) r)) of one frame: acof, kcof, err, gain"""
    a, k, e = levinson_py(np.asarray(r, dtype=np.float32).astype(np.float64), p)
    r0 = float(np.float32(r[0]))
    gain = r0 / e if e > 0 else 0.0
    with np.errstate(all="ignore"):
        return (np.array(a, dtype=np.float32), np.array(k, dtype=np.float32), np.float32(np.float64(e) / n),
                np.float32(gain))


def run(x, p, win=None, host=False, outputs=("kcof", "err", "gain", "r")):
    """llz_lpc_mc with every output in a buffer followed by guard words; returns the outputs (guards checked)"""
    frames, n = x.shape
    sizes = {"acof": frames * (p + 1), "kcof": frames * p, "err": frames, "gain": frames, "r": frames * (p + 1)}
    bufs = {}
    for k, size in sizes.items():
        if k != "acof" and k not in outputs:
            continue
        full = np.full(size + 16, GUARD, dtype=np.float32)
        bufs[k] = full if host else torch.from_numpy(full).to(x.device if hasattr(x, "device") else "cuda:0")
    view = {k: b[:sizes[k]] for k, b in bufs.items()}
    filters.lpc_mc(x, view["acof"], kcof=view.get("kcof"), err=view.get("err"), gain=view.get("gain"), r=view.get("r"),
                   win=win, p=p)
    if not host:
        torch.cuda.synchronize()
    out = {}
    for k, b in bufs.items():
        h = b.cpu().numpy() if hasattr(b, "cpu") else b
        assert (h[sizes[k]:] == GUARD).all(), f"{k}: guard words overwritten"
        out[k] = h[:sizes[k]].copy()
    return out


def check_against_restatement(out, r, n, p, rows):
    acof = out["acof"].reshape(-1, p + 1)
    kcof = out["kcof"].reshape(len(acof), p) if "kcof" in out else None
    for f in rows:
        a, k, e, g = expected(r[f], n, p)
        assert np.array_equal(bits(acof[f]), bits(a)), f"frame {f}: acof"
        if kcof is not None:
            assert np.array_equal(bits(kcof[f]), bits(k)), f"frame {f}: kcof"
        if "err" in out:
            assert bits(out["err"][f]) == bits(e), f"frame {f}: err"
        if "gain" in out:
            assert bits(out["gain"][f]) == bits(g), f"frame {f}: gain"


FUSED = [(p, 300, 65) for p in (0, 1, 7, 8, 9, 10, 16, 17, 24, 25, 32)]
SPLIT = [(p, 700, 65) for p in (33, 48, 64)]
SHAPES = [(16, 37, 64), (10, 11, 63), (32, 33, 1), (9, 10, 65), (64, 65, 64), (48, 123, 1),
          (8, 1001, 70000), (17, 20, 70000), (25, 504, 64), (33, 40, 70000)]


@pytest.mark.parametrize("p,n,frames", FUSED + SPLIT + SHAPES)
def test_lpc_mc_bit_exact(dev, p, n, frames):
    rng = np.random.default_rng(1000 * p + n + frames)
    xh = (rng.standard_normal((frames, n)) * 0.3).astype(np.float32)
    x = torch.from_numpy(xh).to(dev)
    out = run(x, p)
    # r: llz_autocorr_mc's bits
    r_ref = torch.empty(frames, p + 1, dtype=torch.float32, device=dev)
    filters.autocorr_mc(x, r_ref, p)
    torch.cuda.synchronize()
    r = r_ref.cpu().numpy()
    assert np.array_equal(bits(out["r"]), bits(r.reshape(-1)))
    rows = range(frames) if frames <= 65 else sorted(set(rng.integers(0, frames, 300).tolist()) | {0, frames - 1, 63, 64})
    check_against_restatement(out, r, n, p, rows)
    # the other path gives the same bits (split vs fused; for p > 32 both calls take the split path)
    with capi.tuned(lpc_split=1):
        other = run(x, p)
    for k in out:
        assert np.array_equal(bits(out[k]), bits(other[k])), k
    if frames <= 65:
        host = run(xh, p, host=True)                  # host buffers: staged, same bits
        for k in out:
            assert np.array_equal(bits(out[k]), bits(host[k])), k
    only = run(x, p, outputs=())                       # NULL optional outputs
    assert np.array_equal(bits(only["acof"]), bits(out["acof"]))


def test_lpc_mc_window_is_x_times_win(dev):
    rng = np.random.default_rng(5)
    frames, n = 130, 500
    xh = rng.standard_normal((frames, n)).astype(np.float32)
    wh = (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n) / (n - 1))).astype(np.float32)
    x, w = torch.from_numpy(xh).to(dev), torch.from_numpy(wh).to(dev)
    pre = torch.from_numpy(xh * wh).to(dev)              # float32 products, one rounding each
    for p in (10, 16, 40):
        want = run(pre, p)
        got = run(x, p, win=w)
        for k in want:
            assert np.array_equal(bits(got[k]), bits(want[k])), (p, k)
        with capi.tuned(lpc_split=1):
            got = run(x, p, win=w)
        for k in want:
            assert np.array_equal(bits(got[k]), bits(want[k])), (p, k, "split")
        host = run(xh, p, win=wh, host=True)
        for k in want:
            assert np.array_equal(bits(host[k]), bits(want[k])), (p, k, "host")


@pytest.mark.parametrize("p", [10, 32, 64])
def test_lpc_mc_silent_frames(dev, p):
    rng = np.random.default_rng(p)
    frames, n = 200, 256
    xh = rng.standard_normal((frames, n)).astype(np.float32)
    silent = [0, 5, 63, 64, 127, 199]
    xh[silent] = 0
    out = run(torch.from_numpy(xh).to(dev), p)
    for k in out:
        assert not np.isnan(out[k]).any(), k
    acof, kcof = out["acof"].reshape(frames, p + 1), out["kcof"].reshape(frames, p)
    for f in silent:
        assert acof[f][0] == 1 and not acof[f][1:].any() and not kcof[f].any()
        assert out["err"][f] == 0 and out["gain"][f] == 0
    loud = [f for f in range(frames) if f not in silent]
    assert (out["gain"][loud] > 0).all()


def test_lpc_mc_against_double_oracle(dev, oracle):
    """end to end: float32 samples, float32 correlation, double recursion vs. the double correlation and the same recursion"""
    frames, n = 96, 1024
    x = torch.empty(frames, n, dtype=torch.float32, device=dev)
    filters.synth_f32(x, seed=11)
    xh = oracle.synth_f32(frames, n, 11)
    assert np.array_equal(x.cpu().numpy(), xh)
    worst_k, worst_e = 0.0, 0.0
    for p in (1, 8, 10, 16):
        out = run(x, p)
        kcof, err = out["kcof"].reshape(frames, p), out["err"]
        for f in range(frames):
            _, k, e = levinson_py(oracle.autocorr(xh[f].astype(np.float64), p), p)
            worst_k = max(worst_k, float(np.abs(kcof[f] - np.array(k)).max()))
            worst_e = max(worst_e, abs(float(err[f]) - e / n) / (e / n))
    print(f"worst |dk| {worst_k:.3g}, worst relative err difference {worst_e:.3g}")
    # observed on the MI355X: |dk| <= 1.7e-8, relative error difference <= 1.5e-7 (the float32 correlation's rounding)
    assert worst_k < 1e-6 and worst_e < 1e-6


def test_lpc_handle_matches_reference_sequences(dev):
    d = np.load(os.path.join(G, "lpc.npz"), allow_pickle=False)
    for s in "abcd":
        p = int(d[f"lpc_{s}_p"][0])
        h = filters.Lpc(p)
        for i in range(int(d[f"lpc_{s}_steps"][0])):
            k = f"lpc_{s}_{i}"
            acof, kcof, err, gain = h.run(d[k + "_x"])
            assert np.array_equal(acof, d[k + "_acof"]), k
            assert np.array_equal(kcof, d[k + "_kcof"]), k
            assert err == d[k + "_err"][0] and gain == d[k + "_gain"][0], k
        h.close()


def test_lpc_mc_bad_arguments(dev):
    x = torch.zeros(4, 32, device=dev)
    with pytest.raises(capi.LlzError, match="p 65"):
        filters.lpc_mc(x, torch.zeros(4, 66, device=dev), p=65)
    with pytest.raises(capi.LlzError, match="p 32"):
        filters.lpc_mc(x, torch.zeros(4, 33, device=dev), p=32)
    L = capi.lib()
    assert L.llz_lpc_mc(x.data_ptr(), None, None, None, None, None, None, 4, 32, 8, None) < 0
    assert "llz_lpc_mc" in capi.last_error()
    acof = torch.zeros(4, 9, device=dev)
    assert L.llz_lpc_mc(x.data_ptr(), None, acof.data_ptr(), None, None, None, None, 0, 32, 8, None) < 0
    assert "frames 0" in capi.last_error()
