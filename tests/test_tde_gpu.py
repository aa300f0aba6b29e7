"""The time-delay estimator on the MI355X (include/llz_tde.h, filters.TdeMC; kernels/tde.hip) against the float64 model of
tests/tde_checks.py, over its case table.

  1. limits: the curve per lag, the peak, the delay and the state read-out of every frame within their derived limits, the
     integer lag equal to the model's (the margin condition holds on every (pair, frame)), the planted delays found;
  2. call grouping, reset, host pointers, peak = NULL, the pair count: the same bits;
  3. neighbours: a channel scaled by 2^20, zeroed or holding a NaN changes no bit of a pair without it; a NaN stays until reset;
  4. exact properties: the 2^7 scaling under LLZ_TDE_CC, Im S == 0 of (a, a), the swapped pair; set_forget mid-stream;
  5. guarded buffers (tests/buffer_checks.py), the refusals, a torch stream.

Each limits case prints its worst ratios."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import tde_checks as tk  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG = -1
F32 = torch.float32
SMALL = 0                       # CASES[0]: 64 / 16, PHAT, 37 pairs
GROUPING = [0, 1, 3, 4, 5, 6]


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


def data(ci):
    def make():
        case = tk.CASES[ci]
        N, hop = case[0], case[1]
        x = tk.signals(N, hop, case[7])
        w32 = filters.window(tk.window_of(N), N).astype(np.float32)
        return {"case": case, "x": x, "w32": w32, "ref": tk.model64(x, w32, case)}
    return cached(("data", ci), make)


def handle(case, pairs=None, stream=None, lam=None):
    N, hop, weight, L, band, table, lam0, _K = case
    return filters.TdeMC(tk.CHANNELS, table if pairs is None else pairs, N, hop, L, weight, lam0 if lam is None else lam,
                         tk.case_delta(case), band, tk.window_of(N), stream)


def feed(h, x, calls, reads=False, lams=None):
    """x [channels, n] (tensor or numpy) in calls of calls[i] hops each; returns {"delay", "peak": [pairs, K]} and with reads
    "curve", "state", "tau" per frame (a read behind every call that completed frames: use calls of one hop)"""
    hop, at, frame = h.hop, 0, 0
    delay, peak, curves, states = [], [], [], []
    for hops in calls:
        if lams and frame in lams:
            h.set_forget(lams[frame])
        part = x[:, at * hop:(at + hops) * hop]
        part = part.contiguous() if hasattr(part, "contiguous") else np.ascontiguousarray(part)
        d, p = h.process(part)
        assert d.shape == p.shape == (h.pairs, h.frames() - frame)
        at += hops
        frame = h.frames()
        delay.append(d)
        peak.append(p)
        if reads and d.shape[1]:
            assert d.shape[1] == 1
            curves.append(h.curve())
            states.append(h.state())
    out = {"delay": np.concatenate(delay, axis=1), "peak": np.concatenate(peak, axis=1)}
    if reads:
        out["curve"], out["state"] = np.stack(curves), np.stack(states)
        out["delay"], out["peak"] = out["delay"].T, out["peak"].T                       # [frames, pairs] as the model's
        out["tau"] = out["curve"].argmax(axis=2) - h.max_lag
    else:
        out["curve"], out["state"] = h.curve(), h.state()
    return out


def hops_of(case):
    return (case[7] - 1) + case[0] // case[1]


def whole(dev, ci):
    """one call over the whole input, device pointers"""
    def make():
        d = data(ci)
        h = handle(d["case"])
        out = feed(h, torch.from_numpy(d["x"]).to(dev), [hops_of(d["case"])])
        h.close()
        return out
    return cached(("whole", ci), make)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
    assert diff.size == 0, f"{what}: {diff.size} of {a.size} values differ in their bits, the first at {int(diff[0])}"


def same_run(a, b, what):
    for k in ("delay", "peak", "curve", "state"):
        same_bits(a[k], b[k], f"{what}: {k}")


# ================================================================================================ 1. limits
@pytest.mark.parametrize("ci", range(len(tk.CASES)), ids=tk.CASE_IDS)
def test_limits(dev, ci):
    d = data(ci)
    case, ref = d["case"], d["ref"]
    h = handle(case)
    got = feed(h, torch.from_numpy(d["x"]).to(dev), [1] * hops_of(case), reads=True)
    assert h.frames() == case[7]
    h.close()
    tk.check(got, ref, f"device {tk.CASE_IDS[ci]}")
    # the device's own delay belongs to the lag its curve peaks at
    assert np.all(np.abs(got["delay"] - got["tau"]) <= 0.5)
    pl = tk.planted(case[0])
    for p, (cx, cy) in enumerate(case[5]):
        if cx == tk.A and cy in pl and abs(pl[cy]) <= case[3]:
            assert np.all(got["tau"][:, p] == pl[cy]), (p, got["tau"][:, p])
    same_bits(got["delay"].T, whole(dev, ci)["delay"], "hop by hop against one call: delay")


# ================================================================================================ 2. the same bits
@pytest.mark.parametrize("ci", GROUPING, ids=[tk.CASE_IDS[i] for i in GROUPING])
def test_call_grouping(dev, ci):
    d = data(ci)
    case = d["case"]
    xd = torch.from_numpy(d["x"]).to(dev)
    total, lead = hops_of(case), case[0] // case[1] - 1
    one = whole(dev, ci)
    h = handle(case)
    same_run(feed(h, xd, [1] * total), one, "calls of one hop")
    h.close()
    if lead:
        # a ragged split whose first call ends before fft_len samples have arrived: 0 frames, nothing written
        h = handle(case)
        guard = bc.carve(dev, F32, h.pairs * 4, 1)
        snap = bc.snapshot(guard)
        dl, pk = h.process(xd[:, :lead * case[1]].contiguous(), delay=guard.shaped(h.pairs, 4))
        assert dl.shape == (h.pairs, 0) and pk.shape == (h.pairs, 0) and h.frames() == 0
        assert np.array_equal(bc.snapshot(guard), snap), "a call of 0 frames wrote to delay"
        rest = feed(h, xd[:, lead * case[1]:], [3, 1, total - lead - 4])
        h.close()
        same_run(rest, one, "a split that ends before the first frame")


def test_reset_gives_a_fresh_handle(dev):
    d = data(SMALL)
    xd = torch.from_numpy(d["x"]).to(dev)
    h = handle(d["case"])
    feed(h, xd, [7])
    h.reset()
    assert h.frames() == 0
    with pytest.raises(capi.LlzError, match="no frame yet"):
        h.curve()
    same_run(feed(h, xd, [hops_of(d["case"])]), whole(dev, SMALL), "behind reset")
    h.close()


@pytest.mark.parametrize("ci", [0, 4])
def test_host_pointers(dev, ci):
    d = data(ci)
    h = handle(d["case"])
    total = hops_of(d["case"])
    same_run(feed(h, d["x"], [5, total - 5]), whole(dev, ci), "host pointers")
    h.close()


def test_peak_null_leaves_delay(dev):
    d = data(SMALL)
    case = d["case"]
    L = capi.lib()
    h = handle(case)
    xd = torch.from_numpy(d["x"]).to(dev)
    out = torch.zeros(h.pairs, case[7], dtype=F32, device=dev)
    got = L.llz_tde_mc_process(h.handle, xd.data_ptr(), xd.shape[1], out.data_ptr(), None, case[7])
    assert got == case[7], capi.last_error()
    same_bits(out.cpu().numpy(), whole(dev, SMALL)["delay"], "delay with peak = NULL")
    h.close()


def test_pair_count(dev):
    d = data(SMALL)
    one = whole(dev, SMALL)
    xd = torch.from_numpy(d["x"]).to(dev)
    for p in (3, 36):
        h = handle(d["case"], pairs=[d["case"][5][p]])
        got = feed(h, xd, [hops_of(d["case"])])
        h.close()
        for k in ("delay", "peak", "curve", "state"):
            same_bits(got[k][0], one[k][p], f"pair {p} alone: {k}")


# ================================================================================================ 3. neighbours
@pytest.mark.parametrize("what", ["scaled", "zeroed", "nan"])
def test_neighbours(dev, what):
    d = data(SMALL)
    case = d["case"]
    N, hop = case[0], case[1]
    x = d["x"].copy()
    c = tk.D1
    t_nan = 5 * hop + 3
    if what == "scaled":
        x[c] *= np.float32(2.0 ** 20)
    elif what == "zeroed":
        x[c] = 0
    else:
        x[c, t_nan] = np.nan
    one = whole(dev, SMALL)
    h = handle(case)
    got = feed(h, torch.from_numpy(x).to(dev), [hops_of(case)])
    with_c = np.array([c in pair for pair in case[5]])
    assert with_c.any() and not with_c.all()
    for k in ("delay", "peak", "curve", "state"):
        same_bits(got[k][~with_c], one[k][~with_c], f"pairs without the {what} channel: {k}")
    if what == "nan":
        first = max(0, -(-(t_nan - N + 1) // hop))                       # the first frame that covers the sample
        assert 0 < first < case[7]
        same_bits(got["delay"][:, :first], one["delay"][:, :first], "in front of the NaN")
        assert np.isnan(got["delay"][with_c, first:]).all() and np.isnan(got["peak"][with_c, first:]).all()
        assert np.isnan(got["curve"][with_c]).all() and np.isnan(got["state"][with_c][:, :, :2]).all()
        h.reset()
        same_run(feed(h, torch.from_numpy(d["x"]).to(dev), [hops_of(case)]), one, "clean behind reset")
    else:
        assert np.isfinite(got["delay"]).all() and np.isfinite(got["peak"]).all()
    h.close()


# ================================================================================================ 4. exact properties
def test_cc_scales_by_a_power_of_two(dev):
    ci = 3
    d = data(ci)
    case = d["case"]
    x = d["x"].copy()
    ys = sorted({cy for _cx, cy in case[5]} - {cx for cx, _cy in case[5]})
    assert case[2] == tk.CC and ys
    x[ys] *= np.float32(128.0)
    one = whole(dev, ci)
    h = handle(case)
    got = feed(h, torch.from_numpy(x).to(dev), [hops_of(case)])
    h.close()
    scaled = np.array([cy in ys and cx not in ys for cx, cy in case[5]])
    assert scaled.any()
    same_bits(got["delay"][scaled], one["delay"][scaled], "delay under y 2^7")
    same_bits(got["peak"][scaled], one["peak"][scaled] * np.float32(128.0), "peak under y 2^7")
    same_bits(got["curve"][scaled], one["curve"][scaled] * np.float32(128.0), "curve under y 2^7")


@pytest.mark.parametrize("ci", [0, 6])
def test_auto_pair(dev, ci):
    d = data(ci)
    case, ref = d["case"], d["ref"]
    one = whole(dev, ci)
    autos = [p for p, (cx, cy) in enumerate(case[5]) if cx == cy]
    assert autos
    for p in autos:
        assert not one["state"][p][:, 1].any(), "Im S of (a, a)"
        same_bits(one["state"][p][:, 2], one["state"][p][:, 0], "Gx == Re S of (a, a)")
        assert np.all(np.abs(one["delay"][p]) <= ref["lim_d"][:, p]), (one["delay"][p], ref["lim_d"][:, p])
        assert int(one["curve"][p].argmax()) - case[3] == 0


def test_swapped_pair(dev):
    d = data(SMALL)
    ref = d["ref"]
    one = whole(dev, SMALL)
    a, b = tk.SWAP
    assert d["case"][5][a] == d["case"][5][b][::-1]
    err = np.abs(one["delay"][a] + one["delay"][b])
    assert np.all(err <= ref["lim_d"][:, a] + ref["lim_d"][:, b]), err
    a, b = tk.REPEATED
    for k in ("delay", "peak", "curve", "state"):
        same_bits(one[k][a], one[k][b], f"the repeated pair: {k}")


def test_set_forget_mid_stream(dev):
    ci = 6
    d = data(ci)
    case = d["case"]
    lams = {7: 0.5, 15: 0.0, 20: 0.95}
    ref = cached(("forget", ci), lambda: tk.model64(d["x"], d["w32"], case, lams=lams))
    N, hop = case[0], case[1]
    lead = N // hop - 1
    h = handle(case)
    x = torch.from_numpy(d["x"]).to(dev)
    # calls of one hop: frame f is completed by call f + lead, set_forget in front of it
    hop_lams = {f: v for f, v in lams.items()}
    got = {"delay": [], "peak": [], "curve": [], "state": []}
    for call in range(hops_of(case)):
        f = call - lead
        if f in hop_lams:
            h.set_forget(hop_lams[f])
        dl, pk = h.process(x[:, call * hop:(call + 1) * hop].contiguous())
        if dl.shape[1]:
            got["delay"].append(dl[:, 0]); got["peak"].append(pk[:, 0])
            got["curve"].append(h.curve()); got["state"].append(h.state())
    h.close()
    got = {k: np.stack(v) for k, v in got.items()}
    got["tau"] = got["curve"].argmax(axis=2) - case[3]
    tk.check(got, ref, "set_forget mid-stream")
    with pytest.raises(capi.LlzError, match="llz_tde_mc_set_forget.*lam 1"):
        handle(case).set_forget(1.0)


# ================================================================================================ 5. buffers, refusals, stream
@pytest.mark.parametrize("ci,offset", [(0, 1), (1, 3), (5, 5)])
def test_guarded_buffers(dev, ci, offset):
    d = data(ci)
    case = d["case"]
    one = whole(dev, ci)
    K, pitch = case[7], case[7] + 3
    xin = bc.carve_input(dev, d["x"], offset)
    snap = bc.snapshot(xin)
    h = handle(case)
    dl = bc.carve(dev, F32, h.pairs * pitch, offset)
    pk = bc.carve(dev, F32, h.pairs * pitch, offset + 2)
    got_d, got_p = h.process(xin.shaped(*d["x"].shape), delay=dl.shaped(h.pairs, pitch), peak=pk.shaped(h.pairs, pitch))
    torch.cuda.synchronize()
    bc.check_untouched(xin, snap, "x")
    for buf, got, name in ((dl, got_d, "delay"), (pk, got_p, "peak")):
        bc.check_bands(buf, name)
        assert got.shape == (h.pairs, K)
        same_bits(got.cpu().numpy(), one[name], name)
        tail = bc.bits(buf.shaped(h.pairs, pitch)[:, K:])
        assert np.all(tail == bc.SENTINEL32), f"{name}: the tail behind the frames written changed"
    out = bc.carve(dev, F32, h.pairs * (2 * case[3] + 1), offset)
    h.curve(out.shaped(h.pairs, 2 * case[3] + 1))
    bc.check_bands(out, "curve")
    same_bits(bc.check_all_written(out, "curve").reshape(h.pairs, -1), one["curve"], "curve into a device buffer")
    out = bc.carve(dev, F32, h.pairs * h.bins * 4, offset)
    h.state(out.shaped(h.pairs, h.bins, 4))
    bc.check_bands(out, "state")
    same_bits(bc.check_all_written(out, "state").reshape(h.pairs, h.bins, 4), one["state"], "state into a device buffer")
    # host outputs with a pitch: the tail stays as it was
    h.reset()
    hd = np.full((h.pairs, pitch), 7.0, dtype=np.float32)
    hp = np.full((h.pairs, pitch), 7.0, dtype=np.float32)
    got_d, got_p = h.process(d["x"], delay=hd, peak=hp)
    same_bits(got_d, one["delay"], "host delay with a pitch")
    same_bits(got_p, one["peak"], "host peak with a pitch")
    assert np.all(hd[:, K:] == 7.0) and np.all(hp[:, K:] == 7.0)
    h.close()


def test_refusals_leave_the_handle_unchanged(dev):
    d = data(SMALL)
    case = d["case"]
    N, hop, K = case[0], case[1], case[7]
    L = capi.lib()
    one = whole(dev, SMALL)
    xd = torch.from_numpy(d["x"]).to(dev)
    h = handle(case)
    first = 6
    part = xd[:, :first * hop].contiguous()
    h.process(part)
    before = h.frames()
    rest = xd[:, first * hop:].contiguous()
    n = rest.shape[1]
    frames = h.frames_for(n)
    assert frames == K - before
    out = torch.zeros(h.pairs * frames, dtype=F32, device=dev)
    pk = torch.zeros(h.pairs * frames, dtype=F32, device=dev)

    def refused(x_ptr, nn, d_ptr, p_ptr, pitch, *needles):
        L.llz_hip_tune(b"no_such_override", 0)
        assert L.llz_tde_mc_process(h.handle, x_ptr, nn, d_ptr, p_ptr, pitch) == ERR_ARG
        msg = capi.last_error()
        assert all(s in msg for s in ("llz_tde_mc_process",) + needles), msg
        assert h.frames() == before
    refused(rest.data_ptr(), n, out.data_ptr(), pk.data_ptr(), frames - 1, "out_pitch")
    refused(rest.data_ptr(), n + 1, out.data_ptr(), pk.data_ptr(), frames, "multiple of hop")
    refused(rest.data_ptr(), n, None, pk.data_ptr(), frames, "delay NULL")
    refused(None, n, out.data_ptr(), pk.data_ptr(), frames, "x NULL")
    flat = rest.view(-1)
    refused(rest.data_ptr(), n, flat[-4:].data_ptr(), pk.data_ptr(), frames, "delay may not overlap x")
    refused(rest.data_ptr(), n, out.data_ptr(), flat[8:].data_ptr(), frames, "peak may not overlap x")
    refused(rest.data_ptr(), n, out.data_ptr(), out[frames:].data_ptr(), frames, "peak may not overlap delay")
    assert not out.any() and not pk.any() and torch.equal(rest, xd[:, first * hop:])
    assert L.llz_tde_mc_read(h.handle, 2, out.data_ptr()) == ERR_ARG and "what 2" in capi.last_error()
    got = L.llz_tde_mc_process(h.handle, rest.data_ptr(), n, out.data_ptr(), pk.data_ptr(), frames)
    assert got == frames, capi.last_error()
    same_bits(out.view(h.pairs, frames).cpu().numpy(), one["delay"][:, before:], "behind the refused calls: delay")
    same_bits(pk.view(h.pairs, frames).cpu().numpy(), one["peak"][:, before:], "behind the refused calls: peak")
    same_bits(h.state(), one["state"], "behind the refused calls: state")
    h.close()


def test_torch_stream(dev):
    ci = 3
    d = data(ci)
    case = d["case"]
    one = whole(dev, ci)
    xd = torch.from_numpy(d["x"]).to(dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    h = handle(case, stream=s)
    total = hops_of(case)
    with torch.cuda.stream(s):
        got = feed(h, xd, [7, total - 7])
    s.synchronize()
    same_run(got, one, "on a torch stream")
    h.close()
