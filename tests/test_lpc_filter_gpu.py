"""The LPC filters on the MI355X (include/llz_lpc.h part 3): llz_lpc_residual_mc within the derived limit of the float64 sum and
llz_lpc_synth_mc bit for bit on the pinned double recursion (tests/lpc_filter_checks.py), at every order around the kernel's
template edges, frame lengths that are no multiple of the 16-sample block or of a 16-byte access, 1 .. 130 channels and 1 .. 7
frames; the same bits whatever the grouping of frames into calls, after reset, whatever the neighbouring channels hold, from
host or device pointers and at odd element offsets; guarded buffers and the overlap refusals; the round trip on static sets;
and llz_lpc_mc -> residual -> synth end to end on device tensors."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import lpc_filter_checks as lc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    capi.build()
    lib = capi.lib()
    assert hasattr(lib, "llz_lpc_residual_mc") and hasattr(lib, "llz_lpc_synth_mc"), "the library exports no LPC filters"
    capi.check(lib.llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(f, x, a, dev=None, direction="residual"):
    """one call of one direction on numpy inputs; dev None: host pointers.  Returns numpy"""
    fn = getattr(f, direction)
    if dev is None:
        out = np.full(x.shape, np.nan, dtype=np.float32)
        fn(np.ascontiguousarray(x), np.ascontiguousarray(a), out)
        return out
    out = torch.full(x.shape, float("nan"), dtype=torch.float32, device=dev)
    fn(to_dev(x, dev), to_dev(a, dev), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def both(f, x, a, dev):
    return run(f, x, a, dev, "residual"), run(f, x, a, dev, "synth")


def in_calls(channels, frame_len, p, x, a, plan, dev):
    """the frames of x in calls of plan[i] frames each on one handle: (e, y) of the whole stream"""
    f = filters.LpcFilterMC(channels, frame_len, p)
    es, ys, f0 = [], [], 0
    for n in plan:
        xs, asub = x[:, f0 * frame_len:(f0 + n) * frame_len], a[:, f0:f0 + n]
        e, y = both(f, xs, asub, dev)
        es.append(e), ys.append(y)
        f0 += n
    f.close()
    return np.concatenate(es, axis=1), np.concatenate(ys, axis=1)


@pytest.mark.parametrize("fam", lc.FAMILIES)
@pytest.mark.parametrize("channels,p,frame_len,frames", lc.CASES)
def test_parity(dev, channels, p, frame_len, frames, fam):
    d = lc.case_data(channels, p, frame_len, frames, fam)
    f = filters.LpcFilterMC(channels, frame_len, p)
    e, y = both(f, d["x"], d["a"], dev)
    f.close()
    what = f"{channels} ch p {p} frame_len {frame_len} x {frames} ({fam})"
    lc.check_residual(e, d, what)
    lc.check_synth(y, d, what)


@pytest.mark.parametrize("channels,p,frame_len,frames", lc.SPLIT_CASES)
def test_call_splitting_and_reset_leave_every_bit(dev, channels, p, frame_len, frames):
    """one call against 1 + 2 + rest on a second handle, both directions; then reset and the whole stream again on that
    handle: a fresh handle's bits"""
    d = lc.case_data(channels, p, frame_len, frames, "random")
    x, a = d["x"], d["a"]
    e1, y1 = in_calls(channels, frame_len, p, x, a, [frames], dev)
    lc.check_synth(y1, d, "one call")
    f = filters.LpcFilterMC(channels, frame_len, p)
    es, ys, f0 = [], [], 0
    for n in (1, 2, frames - 3):
        e, y = both(f, x[:, f0 * frame_len:(f0 + n) * frame_len], a[:, f0:f0 + n], dev)
        es.append(e), ys.append(y)
        f0 += n
    assert np.array_equal(lc.bits(np.concatenate(es, axis=1)), lc.bits(e1)), "residual: the grouping of frames changed bits"
    assert np.array_equal(lc.bits(np.concatenate(ys, axis=1)), lc.bits(y1)), "synthesis: the grouping of frames changed bits"
    f.reset()
    e3, y3 = both(f, x, a, dev)
    f.close()
    assert np.array_equal(lc.bits(e3), lc.bits(e1)) and np.array_equal(lc.bits(y3), lc.bits(y1)), "reset left state behind"


@pytest.mark.parametrize("p,frame_len", [(7, 50), (16, 160), (33, 1023), (64, 65)])
def test_neighbouring_channels_do_not_reach_a_channel(dev, p, frame_len):
    channels, frames, mid = 3, 3, 1
    d = lc.case_data(channels, p, frame_len, frames, "random")
    e0, y0 = in_calls(channels, frame_len, p, d["x"], d["a"], [1, 2], dev)
    for scale in (2.0 ** 20, 0.0):
        x, a = d["x"].copy(), d["a"].copy()
        for c in (0, 2):
            x[c] *= np.float32(scale)
            a[c, :, 1:] *= np.float32(1.0 if scale else 0.0)
        e, y = in_calls(channels, frame_len, p, x, a, [1, 2], dev)
        assert np.array_equal(lc.bits(e[mid]), lc.bits(e0[mid])) and np.array_equal(lc.bits(y[mid]), lc.bits(y0[mid])), scale


@pytest.mark.parametrize("channels,p,frame_len,frames", [(3, 9, 50, 5), (37, 16, 160, 7), (2, 64, 1023, 2), (5, 0, 1, 7)])
def test_host_pointers_and_odd_offsets_give_the_same_bits(dev, channels, p, frame_len, frames):
    d = lc.case_data(channels, p, frame_len, frames, "random")
    x, a = d["x"], d["a"]
    e0, y0 = in_calls(channels, frame_len, p, x, a, [frames], dev)
    eh, yh = in_calls(channels, frame_len, p, x, a, [frames], None)
    assert np.array_equal(lc.bits(eh), lc.bits(e0)) and np.array_equal(lc.bits(yh), lc.bits(y0)), "host pointers"
    for xo, ao, oo in ((1, 3, 0), (3, 1, 1), (2, 1, 3)):
        f = filters.LpcFilterMC(channels, frame_len, p)
        outs = []
        for direction in ("residual", "synth"):
            xi, ai = bc.carve_input(dev, x, xo, guard=64), bc.carve_input(dev, a, ao, guard=64)
            out = bc.carve(dev, torch.float32, x.size, oo, guard=64)
            getattr(f, direction)(xi.view, ai.view, out.view)
            torch.cuda.synchronize()
            outs.append(out.host().reshape(x.shape))
        f.close()
        assert np.array_equal(lc.bits(outs[0]), lc.bits(e0)) and np.array_equal(lc.bits(outs[1]), lc.bits(y0)), (xo, ao, oo)


@pytest.mark.parametrize("channels,p,frame_len,frames", [(3, 2, 3, 7), (3, 17, 50, 3), (37, 16, 160, 7), (130, 33, 1023, 2)])
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_guarded_buffers(dev, channels, p, frame_len, frames, offset):
    """outputs between sentinel bands at element offsets 0, 1 and 3: every element written, nothing outside; inputs between
    NaN bands: unchanged, and no NaN reaches an output"""
    d = lc.case_data(channels, p, frame_len, frames, "silent")
    x, a = d["x"], d["a"]
    f = filters.LpcFilterMC(channels, frame_len, p)
    for direction, check in (("residual", lc.check_residual), ("synth", lc.check_synth)):
        xi, ai = bc.carve_input(dev, x, (offset + 2) % 4), bc.carve_input(dev, a, (offset + 1) % 4)
        out = bc.carve(dev, torch.float32, x.size, offset)
        sx, sa = bc.snapshot(xi), bc.snapshot(ai)
        getattr(f, direction)(xi.view, ai.view, out.view)
        torch.cuda.synchronize()
        bc.check_bands(out, direction)
        bc.check_untouched(xi, sx, direction + " input")
        bc.check_untouched(ai, sa, direction + " acof")
        check(bc.check_all_written(out, direction).reshape(x.shape), d, f"{direction} at offset {offset}")
    f.close()


def test_overlapping_device_ranges_are_refused_with_nothing_written(dev):
    channels, p, frame_len, frames = 3, 7, 50, 4
    L = capi.lib()
    n, nc = channels * frames * frame_len, channels * frames * (p + 1)
    f = filters.LpcFilterMC(channels, frame_len, p)
    other_in = torch.zeros(n, dtype=torch.float32, device=dev)
    other_cof = torch.zeros(nc, dtype=torch.float32, device=dev)
    for name, in_name, out_name in (("llz_lpc_residual_mc", "x", "e"), ("llz_lpc_synth_mc", "e", "y")):
        fn = getattr(L, name)
        for which, numel in (("in", n), ("acof", nc)):
            for src, out in bc.overlap_cases(numel, n, device=dev):
                before = (bc.bits(src).copy(), bc.bits(out).copy())
                args = (src.data_ptr(), other_cof.data_ptr()) if which == "in" else (other_in.data_ptr(), src.data_ptr())
                rc = fn(f.handle, args[0], args[1], out.data_ptr(), frames)
                torch.cuda.synchronize()
                msg = capi.last_error()
                assert rc == -1 and name in msg and "may not overlap" in msg, (name, which, rc, msg)
                assert f"{out_name} may not overlap {in_name if which == 'in' else 'acof'}" in msg, msg
                assert np.array_equal(bc.bits(src), before[0]) and np.array_equal(bc.bits(out), before[1]), (name, which)
    # the refusals left the handle's state alone: a fresh handle's bits
    d = lc.case_data(channels, p, frame_len, frames, "random")
    e, y = both(f, d["x"], d["a"], dev)
    f.close()
    lc.check_residual(e, d, "after refusals")
    lc.check_synth(y, d, "after refusals")


@pytest.mark.parametrize("p", [2, 9, 16, 32, 64])
def test_round_trip_on_static_sets(dev, p):
    """family (iv): |synth(residual(x)) - x|[t] <= sum_j |g[j]| max_t (2 (p + 1) u S_t) + 1.01 u |x[t]|"""
    channels, frame_len, frames = 5, 160, 3
    x = lc.signal(channels, frames * frame_len, 50 + p)
    a = lc.family("static", channels, frames, p, 60 + p)
    g = lc.impulse_response(a[:, 0, :])
    f = filters.LpcFilterMC(channels, frame_len, p)
    e = run(f, x, a, dev, "residual")
    back = run(f, e, a, dev, "synth")
    f.close()
    lim = np.abs(g).sum(axis=1, keepdims=True) * lc.residual_limit(x, a, frame_len).max(axis=1, keepdims=True) \
        + 1.01 * lc.U * np.abs(x.astype(np.float64))
    err = np.abs(back.astype(np.float64) - x)
    print(f"round trip p {p}: worst |err| / limit = {float((err / lim).max()):.3g}")
    assert (err <= lim).all()


def test_end_to_end_from_llz_lpc_mc(dev):
    """family (ii): llz_lpc_mc -> residual -> synth on device tensors, p 16, frame_len 160, 37 channels x 7 frames of two tones
    plus noise with silent frames mixed in: the residual within its limit, the synthesis the model's bits, the residual's
    energy below the input's in every frame that is not silent, and synth(residual(x)) the model's bits on the device's e"""
    channels, p, frame_len, frames = 37, 16, 160, 7
    x = lc.signal(channels, frames * frame_len, 4242).reshape(channels, frames, frame_len).copy()
    silent = np.zeros((channels, frames), dtype=bool)
    silent[::5, 3] = silent[1::7, 0] = True
    x[silent] = 0.0
    x = x.reshape(channels, frames * frame_len)
    xd = to_dev(x, dev)
    acof = torch.empty(channels, frames, p + 1, dtype=torch.float32, device=dev)
    filters.lpc_mc(xd.view(channels * frames, frame_len), acof.view(channels * frames, p + 1), p=p)
    e, y, back = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)
    f = filters.LpcFilterMC(channels, frame_len, p)
    f.residual(xd, acof, e)
    f.synth(xd, acof, y)
    f.reset()
    f.synth(e, acof, back)
    torch.cuda.synchronize()
    f.close()
    a = acof.cpu().numpy()
    assert np.array_equal(a[silent], np.eye(1, p + 1, dtype=np.float32).repeat(int(silent.sum()), axis=0))
    d = {"x": x, "a": a, "e64": lc.residual64(x, a, frame_len), "lim": lc.residual_limit(x, a, frame_len),
         "y": lc.synth_model(x, a, frame_len).astype(np.float32)}
    eh = e.cpu().numpy()
    lc.check_residual(eh, d, "end to end")
    lc.check_synth(y.cpu().numpy(), d, "end to end")
    ex = (x.astype(np.float64) ** 2).reshape(channels, frames, frame_len).sum(axis=2)
    ee = (eh.astype(np.float64) ** 2).reshape(channels, frames, frame_len).sum(axis=2)
    assert (ee[~silent] < ex[~silent]).all() and (ee[silent] == 0).all(), "prediction gained nothing"
    bh = lc.synth_model(eh, a, frame_len).astype(np.float32)
    assert np.array_equal(lc.bits(back.cpu().numpy()), lc.bits(bh))
