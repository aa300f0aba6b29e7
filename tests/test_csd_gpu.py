"""The Welch cross-spectra on the MI355X (include/llz_spectral.h, filters.CsdMC; kernels/csd.hip) against the float64 reference
of tests/csd_checks.py: eight channels, fifteen pairs, K = 2 RUN + 3 frames, fft_len 64 .. 4096 with every hop at 256 and 1024,
each size under the fft_generic tune as well.

  1. the per-bin limit and the pooled gate on every pair (each case prints its worst ratios), the form plan() reports;
  2. exact ties in the raw sums: power-of-two copies, the conjugate pair, Sxy == Sxx with a zero imaginary part, exact zeros and
     NaN read-outs with the silent channel, the repeated pair;
  3. the read-outs within 2 float32 ulp of their formulas on the handle's own raw sums, y = -4 x, COHERENCE <= 1 + 4 u;
  4. call grouping: one call, single hops, (1 hop, rest), a split that ends mid-run -- the same bits, also over two and more walks
     of a capped scratch; reset; host pointers; a torch stream;
  5. guarded buffers (tests/buffer_checks.py) and the refusals.

Each coherence case prints the largest value read."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import csd_checks as cc  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG = -1
F32 = torch.float32
READS = ("psd_x", "psd_y", "csd", "coherence", "transfer")
CASE_IDS = [f"{N}-{hop}{'-generic' if g else ''}" for N, hop, g in cc.CASES]
GROUPING = [(64, 16, False), (128, 64, False), (256, 64, False), (512, 512, False), (1024, 512, False), (2048, 512, False),
            (4096, 2048, False), (256, 128, True), (1024, 256, True)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    capi.build()
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


_CACHE = {}


def cached(key, make):
    """inputs, references and device results of a case: computed once, shared by the tests that need them, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def data(N, hop):
    def make():
        x = cc.signals(N, hop)
        w32 = filters.window(cc.window_of(N), N).astype(np.float32)
        ref, lim, gate = cc.reference(x, w32, N, hop)
        return {"x": x, "w32": w32, "ref": ref, "lim": lim, "gate": gate, "u": float((w32.astype(np.float64) ** 2).sum())}
    return cached(("data", N, hop), make)


def tune_of(generic, **more):
    return capi.tuned(**dict({"fft_generic": 1} if generic else {}, **more))


def feed(dev, N, hop, generic, calls=None, xd=None, reads=False, **tune):
    """a fresh handle fed the case's stream in calls of `calls` hops (None: one call); returns what it read"""
    x = data(N, hop)["x"]
    xd = torch.from_numpy(x).to(dev) if xd is None else xd
    hops = x.shape[1] // hop
    calls = [hops] if calls is None else calls
    assert sum(calls) == hops
    out = {}
    with tune_of(generic, **tune):
        h = filters.CsdMC(cc.CHANNELS, cc.PAIRS, N, hop, cc.window_of(N))
        out["plan"] = h.plan(calls[0] * hop)
        at = 0
        for c in calls:
            part = xd[:, at * hop:(at + c) * hop]
            out["frames"] = h.update(part if len(calls) == 1 else part.contiguous())
            at += c
        out["raw"] = h.raw()
        if reads:
            for name in READS:
                out[name] = getattr(h, name)()
        assert h.frames() == out["frames"]
        h.close()
    return out


def result(dev, N, hop, generic):
    return cached(("run", N, hop, generic), lambda: feed(dev, N, hop, generic, reads=True))


def same_bits(a, b, what):
    assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32),
                                                 b.view(np.uint64 if a.dtype == np.float64 else np.uint32)), what


# ================================================================================================ 1. limits, gate, form
@pytest.mark.parametrize("N,hop,generic", cc.CASES, ids=CASE_IDS)
def test_limits_and_gate(dev, N, hop, generic):
    d, r = data(N, hop), result(dev, N, hop, generic)
    assert r["frames"] == cc.K_FRAMES
    want_form = 1 if N in cc.REGISTER_SIZES and not generic else 0
    assert r["plan"] == {"form": want_form, "run": cc.RUN, "runs_per_walk": 3, "walks": 1}, r["plan"]
    cc.check_raw(r["raw"], d["ref"], d["lim"], d["gate"],
                 f"CSD | fft_len {N} hop {hop} | {'register' if want_form else 'staged'}{' fft_generic' if generic else ''}")


# ================================================================================================ 2. exact ties
@pytest.mark.parametrize("N,hop,generic", cc.CASES, ids=CASE_IDS)
def test_exact_ties(dev, N, hop, generic):
    raw = result(dev, N, hop, generic)["raw"]
    for p, base, ex, ey in cc.SCALED:                                   # Sxx 2^2ex, Syy 2^2ey, Sxy 2^(ex + ey), bit for bit
        want = raw[base] * np.array([2.0 ** (2 * ex), 2.0 ** (2 * ey), 2.0 ** (ex + ey), 2.0 ** (ex + ey)])
        same_bits(raw[p], want, f"pair {p} is not pair {base} scaled")
        assert np.all(raw[p][:, :2] > 0)
    a, b = cc.CONJ_PAIRS
    same_bits(raw[b][:, [1, 0, 2]].copy(), raw[a][:, [0, 1, 2]].copy(), "(b, a) against (a, b)")
    assert np.array_equal(raw[b][:, 3], -raw[a][:, 3]) and np.any(raw[a][:, 3] != 0)
    for p in cc.AUTO_PAIRS:
        same_bits(raw[p][:, 2].copy(), raw[p][:, 0].copy(), "Sxy of (a, a) is not Sxx")
        same_bits(raw[p][:, 1].copy(), raw[p][:, 0].copy(), "Syy of (a, a) is not Sxx")
        assert not raw[p][:, 3].any()
    same_bits(raw[cc.REPEATED[1]], raw[cc.REPEATED[0]], "the repeated pair")
    for p, (cx, cy) in enumerate(cc.PAIRS):                             # the silent channel: exact zeros in its sums only
        silent = [k for k, c in ((0, cx), (1, cy)) if c == cc.E_ZERO]
        if silent:
            assert not raw[p][:, silent + [2, 3]].any(), p
        for k, c in ((0, cx), (1, cy)):
            if c != cc.E_ZERO:
                assert np.all(raw[p][:, k] > 0), (p, k)
    same_bits(raw[9][:, 0].copy(), raw[0][:, 0].copy(), "Sxx of (a, e) is not Sxx of (a, a)")


# ================================================================================================ 3. read-outs
@pytest.mark.parametrize("N,hop,generic", cc.CASES, ids=CASE_IDS)
def test_readouts_follow_their_formulas(dev, N, hop, generic):
    d, r = data(N, hop), result(dev, N, hop, generic)
    want = cc.readouts64(r["raw"], r["frames"], d["u"])
    for name in READS:
        assert r[name].dtype == np.float32 and r[name].shape == want[name].shape
        cc.within_ulps(r[name], want[name], 2, f"{name} {N}/{hop}")
    for p, (cx, cy) in enumerate(cc.PAIRS):
        assert np.isnan(r["coherence"][p]).all() == (cc.E_ZERO in (cx, cy)), p
        assert np.isnan(r["transfer"][p]).all() == (cx == cc.E_ZERO), p
        assert np.isnan(r["transfer"][p]).any() == (cx == cc.E_ZERO), p
    m4 = cc.MINUS4_PAIR                                                 # y = -4 x
    assert np.all(r["transfer"][m4][:, 0] == -4.0) and not r["transfer"][m4][:, 1].any()
    assert np.all(np.abs(r["coherence"][m4].astype(np.float64) - 1.0) <= 2 * 2.0 ** -23)


@pytest.mark.parametrize("N,hop,generic", cc.CASES, ids=CASE_IDS)
def test_coherence_never_above_one(dev, N, hop, generic):
    """COHERENCE <= 1 + 4 u at every bin of every pair.  The sine / cosine pairs are the hard case: two tones are coherent to
    within 1e-9 at their bins, Cauchy-Schwarz holds for the exact sums of the computed X_f and Y_f, and what the float32 sums of a
    run lose moves Sxx, Syy and Sxy independently.  With plain 32-term float32 sums the device read up to 1 + 12 u there (the
    plain model of tests/csd_checks.py 1 + 5 u to 1 + 14 u); the kernels' run sums are compensated (csd_add in kernels/csd.hip)."""
    coh = result(dev, N, hop, generic)["coherence"].astype(np.float64)
    over = np.nanmax(coh, axis=1) - 1.0
    worst = int(np.nanargmax(over))
    print(f"COHERENCE | fft_len {N} hop {hop}{' fft_generic' if generic else ''} | largest value 1 + {over[worst] / cc.U:.3g} u "
          f"(pair {worst} {cc.PAIRS[worst]})")
    assert over[worst] <= 4 * cc.U, (worst, over[worst] / cc.U)


# ================================================================================================ 4. call grouping
@pytest.mark.parametrize("N,hop,generic", GROUPING, ids=[f"{N}-{hop}{'-generic' if g else ''}" for N, hop, g in GROUPING])
def test_call_grouping_leaves_every_bit(dev, N, hop, generic):
    whole = result(dev, N, hop, generic)["raw"]
    xd = torch.from_numpy(data(N, hop)["x"]).to(dev)
    hops, lead = xd.shape[1] // hop, N // hop - 1
    mid = lead + cc.RUN + 8                                             # ends with 40 frames summed: inside the second run
    ways = {"single hops": [1] * hops, "1 hop, rest": [1, hops - 1], "mid-run": [mid, hops - mid],
            "mid-run thrice": [lead + 5, cc.RUN + 3, hops - lead - cc.RUN - 8]}
    for name, calls in ways.items():
        got = feed(dev, N, hop, generic, calls, xd)
        assert got["frames"] == cc.K_FRAMES
        same_bits(got["raw"], whole, f"{name} against one call")
    per_run = len(cc.PAIRS) * (N // 2 + 1) * 16
    kb = max(1, (per_run * 3 // 2) // 1024)                             # room for one run's partials and not for two
    for name, calls in (("one call", None), ("mid-run", ways["mid-run"])):
        got = feed(dev, N, hop, generic, calls, xd, csd_scratch_kb=kb)
        if calls is None:
            assert got["plan"]["walks"] == 3 and got["plan"]["runs_per_walk"] == 1, got["plan"]
        else:
            assert got["plan"]["walks"] >= 2, got["plan"]
        same_bits(got["raw"], whole, f"{name} over capped scratch against one call")


def test_reset_returns_to_a_fresh_handle(dev):
    N, hop = 256, 64
    d, whole = data(N, hop), result(dev, N, hop, False)
    xd = torch.from_numpy(d["x"]).to(dev)
    h = filters.CsdMC(cc.CHANNELS, cc.PAIRS, N, hop, cc.window_of(N))
    h.update(xd[:, :41 * hop].contiguous())                            # history, an open run and accumulators all in use
    assert h.frames() == 38
    h.reset()
    assert h.frames() == 0
    with pytest.raises(capi.LlzError, match="no frame yet"):
        h.raw()
    assert h.update(xd) == cc.K_FRAMES
    same_bits(h.raw(), whole["raw"], "after reset")
    for name in READS:
        same_bits(getattr(h, name)(), whole[name], name + " after reset")
    h.close()


def test_host_pointers_equal_device_pointers(dev):
    N, hop = 512, 256
    d = data(N, hop)
    whole = feed(dev, N, hop, False, reads=True)
    h = filters.CsdMC(cc.CHANNELS, cc.PAIRS, N, hop, cc.window_of(N))
    hops = d["x"].shape[1] // hop
    h.update(np.ascontiguousarray(d["x"][:, :9 * hop]))
    assert h.update(np.ascontiguousarray(d["x"][:, 9 * hop:])) == hops - 1
    same_bits(h.raw(), whole["raw"], "host x")
    for name in READS:                                                  # device outputs against host outputs
        out = torch.full(whole[name].shape, float("nan"), dtype=F32, device=dev)
        getattr(h, name)(out)
        same_bits(out.cpu().numpy(), whole[name], name)
    rawd = torch.zeros(whole["raw"].shape, dtype=torch.float64, device=dev)
    h.raw(rawd)
    same_bits(rawd.cpu().numpy(), whole["raw"], "raw into device memory")
    h.close()


def test_torch_stream(dev):
    N, hop = 1024, 256
    whole = feed(dev, N, hop, False)
    xd = torch.from_numpy(data(N, hop)["x"]).to(dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    h = filters.CsdMC(cc.CHANNELS, cc.PAIRS, N, hop, cc.window_of(N), stream=s)
    with torch.cuda.stream(s):
        h.update(xd[:, :7 * hop].contiguous())
        h.update(xd[:, 7 * hop:].contiguous())
        raw = h.raw()
    s.synchronize()
    same_bits(raw, whole["raw"], "on a torch stream")
    h.close()


# ================================================================================================ 5. buffers, refusals
@pytest.mark.parametrize("N,hop,offset", [(64, 16, 1), (256, 128, 3), (1024, 512, 5), (2048, 512, 7)])
def test_guarded_buffers(dev, N, hop, offset):
    """x at an odd element offset between NaN bands, every out between sentinel bands and pre-filled with the sentinel"""
    d = data(N, hop)
    whole = feed(dev, N, hop, False, reads=True)
    xin = bc.carve_input(dev, d["x"], offset)
    snap = bc.snapshot(xin)
    h = filters.CsdMC(cc.CHANNELS, cc.PAIRS, N, hop, cc.window_of(N))
    assert h.update(xin.shaped(*d["x"].shape)) == cc.K_FRAMES
    bc.check_untouched(xin, snap, "x")
    for name in READS:
        out = bc.carve(dev, F32, whole[name].size, offset)
        getattr(h, name)(out.shaped(*whole[name].shape))
        bc.check_bands(out, name)
        same_bits(bc.check_all_written(out, name).reshape(whole[name].shape), whole[name], name)
    raw = bc.carve(dev, F32, 2 * whole["raw"].size, 2 * offset)         # doubles at an 8-byte and no 16-byte boundary
    capi.check(h._L.llz_csd_mc_read_raw(h.handle, raw.view.data_ptr()), "llz_csd_mc_read_raw")
    bc.check_bands(raw, "raw")
    same_bits(bc.check_all_written(raw, "raw").view(np.float64).reshape(whole["raw"].shape), whole["raw"], "raw")
    h.close()


def test_refusals(dev):
    L = capi.lib()
    table = (C.c_int * 4)(0, 1, 1, 0)

    def refused(rc, *needles):
        assert rc == ERR_ARG or rc == capi.BAD_HANDLE, rc
        msg = capi.last_error()
        assert all(n in msg for n in needles), (needles, msg)

    refused(L.llz_csd_mc_init(2, 2, table, 256, 100, capi.HAMMING), "llz_csd_mc_init", "hop 100")
    refused(L.llz_csd_mc_init(2, 2, table, 384, 96, capi.HAMMING), "llz_csd_mc_init", "fft_len 384")
    refused(L.llz_csd_mc_init(2, 2, table, 8192, 4096, capi.HAMMING), "llz_csd_mc_init", "fft_len 8192")
    refused(L.llz_csd_mc_init(1, 2, table, 256, 64, capi.HAMMING), "llz_csd_mc_init", "channel 1")
    h = filters.CsdMC(2, [(0, 1), (1, 0)], 256, 64)
    x = torch.zeros(2, 256, dtype=F32, device=dev)
    out = torch.zeros(2, 129, 2, dtype=F32, device=dev)
    refused(L.llz_csd_mc_update(h.handle, x.data_ptr(), 65), "llz_csd_mc_update", "multiple of hop")
    refused(L.llz_csd_mc_update(h.handle, x.data_ptr(), 0), "llz_csd_mc_update")
    refused(L.llz_csd_mc_read(h.handle, capi.SPEC_PXX, out.data_ptr()), "llz_csd_mc_read", "no frame yet")
    assert h.update(x[:, :192].contiguous()) == 0                       # three hops: still no whole frame
    refused(L.llz_csd_mc_read(h.handle, capi.SPEC_TF, out.data_ptr()), "llz_csd_mc_read", "no frame yet")
    refused(L.llz_csd_mc_read_raw(h.handle, out.data_ptr()), "llz_csd_mc_read_raw", "no frame yet")
    assert h.update(x[:, :64].contiguous()) == 1
    refused(L.llz_csd_mc_read(h.handle, 7, out.data_ptr()), "llz_csd_mc_read", "what 7")
    assert np.isnan(h.coherence()).all() and np.isnan(h.transfer()).all() and not h.psd_x().any()   # silence: NaN, not a fault
    other = filters.StftMC(2, capi.OVERLAP_LOW, 128)
    for bad in (0, capi.BAD_HANDLE, other.handle):
        refused(L.llz_csd_mc_update(bad, x.data_ptr(), 64), "llz_csd_mc_update", "bad handle")
        refused(L.llz_csd_mc_read(bad, 0, out.data_ptr()), "llz_csd_mc_read", "bad handle")
        refused(L.llz_csd_mc_read_raw(bad, out.data_ptr()), "llz_csd_mc_read_raw", "bad handle")
        refused(L.llz_csd_mc_reset(bad), "llz_csd_mc_reset", "bad handle")
        refused(L.llz_csd_mc_frames(bad), "llz_csd_mc_frames", "bad handle")
    other.close()
    h.close()
