"""The arbitrary-ratio resampler on the device (include/llz_asrc.h, llz_asrc_mc; kernels k_asrc_f32 / k_asrc_advance of asrc.hip)
against the float64 model of its definition (tests/asrc_checks.py, where the limit is stated):

  1. dense: 3 and 37 channels, steps 1/16 .. 16 spread over them, (T, phases) in {(4, 256), (32, 512), (128, 4096)} -- both table
     forms -- and (32, 512) under the override that forces the global form; calls of 257, 1 and 1000 samples of seeded noise;
     every sample within the limit, counts and times equal; and calls of 40000 to 150000 samples, where a workgroup walks 8 and 32
     tiles with the next span prefetched, or staged inside the walk at steps 3 and 16, in both table forms, also bit for bit
     against calls of 2500 samples;
  2. call grouping: the same stream in one call and cut elsewhere, one-sample and empty calls included: bit-equal outputs;
  3. glides of 1, 7 and 1000 outputs across call boundaries, one spanning three calls, a set_step inside a glide; afterwards a
     long run matches a fresh model started at that time with the target as its step;
  4. identity: cutoff 1, gain 1, step 1: row 0 of G is a unit impulse and y has the bits of x, NaN and Inf blocks included;
  5. neighbour independence: a channel's bits do not change when its neighbours are scaled by 2^20, zeroed or set to NaN;
  6. buffers: guarded buffers at odd offsets, overlapping device ranges and a too-small out_pitch refused with the next call
     unaffected, host pointers with the bits of device pointers;
  7. reset returns the handle to a fresh handle's outputs;
  8. end to end: a sine through a running glide against the analytic sine at the model's times.

test_asrc_host.py runs cases 1, 3 and 8 with the numpy float32 model in the device's place.  On the parent of this feature the
library exports no llz_asrc_mc and every test here fails."""
import numpy as np
import pytest
import torch

from llzlab_amd import capi, filters
from tests import asrc_checks as ac
from tests import buffer_checks as bc

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def as_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. dense
@pytest.mark.parametrize("T,phases,form", [s + (f,) for s, f in zip(ac.SHAPES, (0, 0, 1))])
@pytest.mark.parametrize("channels", ac.CHANNELS)
def test_dense_parity(dev, oracle, T, phases, form, channels):
    f = filters.AsrcMC(channels, 8, taps=T, phases=phases, cutoff=ac.CUTOFF)
    assert f.plan() == (T, phases, T - 1, form)
    assert np.array_equal(as_bits(f.table()), as_bits(ac.table(T, phases))), "get_table differs from the model's table"
    f.close()
    assert ac.check_against(ac.device(dev), oracle, channels, T, phases, what="dense") <= 1.0


@pytest.mark.parametrize("channels", ac.CHANNELS)
def test_dense_parity_global_form_forced(dev, oracle, channels):
    """(32, 512) once more with its table read from global memory: the same limit, and the LDS form's bits"""
    T, phases = 32, 512
    x = ac.noise(oracle, channels, sum(ac.CALLS), 11)
    lds, _, _, _ = ac.run_stream(ac.device(dev), channels, ac.CALLS, x, T, phases)
    with capi.tuned(asrc_table_global=1):
        f = filters.AsrcMC(channels, 8, taps=T, phases=phases, cutoff=ac.CUTOFF)
        assert f.plan() == (T, phases, T - 1, 1)
        f.close()
        assert ac.check_against(ac.device(dev), oracle, channels, T, phases, what="dense, global form forced") <= 1.0
        glb, _, _, _ = ac.run_stream(ac.device(dev), channels, ac.CALLS, x, T, phases)
    for c in range(channels):
        assert np.array_equal(as_bits(lds[c]), as_bits(glb[c])), c


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", sorted(ac.LONG))
def test_long_calls_walk_tiles(dev, oracle, name, form):
    """asrc_checks.LONG: calls long enough for workgroups that walk 8 and 32 tiles, with the next span prefetched into one and
    into both registers, and for spans that are staged inside the walk (steps 3 and 16), in both table forms: the limit, counts
    and times against the model, and the bits of the same stream in calls of 2500 samples"""
    with capi.tuned(asrc_table_global=form):
        f = filters.AsrcMC(2, 8)
        assert f.plan()[3] == form
        f.close()
        assert ac.check_long(ac.device(dev), oracle, name, what=f"long (table form {form})") <= 1.0


# ------------------------------------------------------------------------------------------------ 2. call grouping
def test_call_grouping_changes_no_bit(dev, oracle):
    channels, T, phases, n = 7, 32, 512, 1258
    x = ac.noise(oracle, channels, n, 11)
    script = {0: [(2, 1.0007, 900)]}                            # a glide under way while the calls are cut
    whole, _, counts, times = ac.run_stream(ac.device(dev), channels, (n,), x, T, phases, script=script)
    for cuts in ((257, 1, 1000), (1,) * 70 + (0, 1188), (0, 5, 0, 1253), (629, 629)):
        got, _, c2, t2 = ac.run_stream(ac.device(dev), channels, cuts, x, T, phases, script=script)
        assert np.array_equal(np.sum(c2, axis=0), np.sum(counts, axis=0)), cuts
        assert all(np.array_equal(a, b) for a, b in zip(t2[-1], times[-1])), cuts
        for c in range(channels):
            assert np.array_equal(as_bits(got[c]), as_bits(whole[c])), (cuts[:4], c)


# ------------------------------------------------------------------------------------------------ 3. glides
def test_glides_across_calls(dev, oracle):
    assert ac.check_glides(ac.device(dev), oracle) <= 1.0


def test_after_a_glide_the_step_is_the_target(dev, oracle):
    """behind the glides of case 3 every step equals its target exactly: 2000 more samples match a FRESH model that starts at
    the handle's next_time with the targets as its steps -- times to equality, samples to the limit"""
    channels, T, phases = 4, 32, 512
    calls, more = ac.GLIDE_CALLS + (1200,), 2000                # 1200 samples more: the last glide (600 outputs) is over
    x = ac.noise(oracle, channels, sum(calls) + more, 23)
    r = ac.Device(dev, channels, more, step=float(ac.GLIDE_STEPS[0]), taps=T, phases=phases)
    for c in range(1, channels):
        r.set_step(c, ac.GLIDE_STEPS[c], 0)
    pos = 0
    for i, n in enumerate(calls):
        for (first, st, ramp) in ac.GLIDE_SCRIPT.get(i, []):
            r.set_step(first, st, ramp)
        r.process(x[:, pos:pos + n])
        pos += n
    step, left = r.f.get_step()
    targets = [1.01, 1.25, 0.997, 1.5]
    assert np.array_equal(left, np.zeros(channels)) and np.array_equal(step * 2.0 ** 32, [ac.to_inc(s) for s in targets])
    whole, frac = r.next_time()
    fresh = ac.Model(channels, more, taps=T, phases=phases,
                     start=(x[:, :pos], [(int(w) << 32) | int(f) for w, f in zip(whole, frac)], [ac.to_inc(s) for s in targets]))
    y, _, _ = r.process(x[:, pos:pos + more])
    ym, A, _ = fresh.process(x[:, pos:pos + more])
    assert all(np.array_equal(a, b) for a, b in zip(r.next_time(), fresh.next_time()))
    worst = max(ac.ratio_to_limit(y[c], ym[c], A[c], T) for c in range(channels))
    print(f"asrc behind the glides: worst ratio to the limit {worst:.3g}")
    r.close()
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 4. identity
@pytest.mark.parametrize("T,phases", [(4, 256), (32, 512), (32, 1024), (6, 2048), (128, 4096)])
def test_identity_at_step_one(dev, oracle, T, phases):
    """cutoff 1, gain 1, step 1: y_j has the bits of x_j.  The sum still runs over the T samples around x_j with coefficients 0,
    so an output whose window holds a sample that is not finite away from its centre is NaN (0 x Inf), as is the output at a NaN;
    everywhere else, and at a lone Inf, the bits are the input's (noise holds no -0, which the sum from +0 would turn into +0)."""
    channels, n = 3, 1500
    x = np.array(ac.noise(oracle, channels, n, 5))
    x[0, 300:340] = np.nan
    x[1, 700:741] = np.inf
    x[1, 900] = -np.inf
    x[2, 1000] = np.nan
    x[2, 64] = np.float32(1e-42)                                # a subnormal keeps its bits
    f = filters.AsrcMC(channels, n, step=1.0, taps=T, phases=phases, cutoff=1.0)
    g = f.table()
    unit = np.zeros(T, np.float32)
    unit[T // 2] = 1.0
    assert np.array_equal(as_bits(g[0]), as_bits(unit)) and np.array_equal(as_bits(g), as_bits(ac.table(T, phases, cutoff=1.0)))
    out = torch.zeros(channels, n, dtype=F32, device=dev)
    counts = f.process(torch.from_numpy(x).to(dev), out)
    torch.cuda.synchronize()
    f.close()
    assert np.array_equal(counts, np.full(channels, n - T // 2))
    m = n - T // 2
    y, xs = out.cpu().numpy()[:, :m], x[:, :m]
    bad = ~np.isfinite(x)
    cum = np.concatenate([np.zeros((channels, T), int), np.cumsum(bad, axis=1)], axis=1)    # cum[:, T + i] = bad samples up to i
    j = np.arange(m)
    inside = cum[:, T + j + T // 2] - cum[:, T + j - T // 2]    # samples that are not finite in the window [j - T/2 + 1, j + T/2]
    same = (inside == 0) | ((inside == 1) & np.isinf(xs))       # a clean window, or a lone Inf at its centre
    assert np.array_equal(as_bits(y)[same], as_bits(xs)[same])
    assert np.all(np.isnan(y[~same]))
    assert same[1, 900] and y[1, 900] == -np.inf and not same[2, 1000] and same[2, 64] and np.count_nonzero(~same) > 80


# ------------------------------------------------------------------------------------------------ 5. neighbours
def test_neighbours_change_no_bit(dev, oracle):
    channels, T, phases, probe = 5, 32, 512, 2
    steps = np.array([1.0 / 16, 0.3337, 160.0 / 147, 16.0, 1.0])
    x = np.array(ac.noise(oracle, channels, sum(ac.CALLS), 17))
    script = {1: [(probe, 1.2, 300), (probe + 1, 3.0, 50)]}
    base, _, _, _ = ac.run_stream(ac.device(dev), channels, ac.CALLS, x, T, phases, steps=steps, script=script)
    for what, change in (("scaled by 2^20", lambda v: v * np.float32(2.0 ** 20)), ("zeroed", lambda v: v * 0),
                         ("NaN", lambda v: v * np.float32("nan"))):
        x2 = x.copy()
        for c in range(channels):
            if c != probe:
                x2[c] = change(x[c])
        got, _, _, _ = ac.run_stream(ac.device(dev), channels, ac.CALLS, x2, T, phases, steps=steps, script=script)
        assert np.array_equal(as_bits(got[probe]), as_bits(base[probe])), what
        assert len(base[probe]) > 1000


# ------------------------------------------------------------------------------------------------ 6. buffers
def plain_run(dev, x, steps, T, phases, frame_len):
    f = filters.AsrcMC(x.shape[0], frame_len, step=float(steps[0]), taps=T, phases=phases, cutoff=ac.CUTOFF)
    for c in range(1, x.shape[0]):
        f.set_step(c, steps[c])
    return f


@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 0), (0, 1), (1, 3)])
def test_guarded_buffers_at_odd_offsets(dev, oracle, off_in, off_out):
    """sentinel bands and out[c][count_c .. out_pitch) come back bit-unchanged, the input is not written, and the outputs have
    the bits of a run on plain tensors"""
    channels, T, phases, n = 6, 32, 512, 1000
    steps = ac.steps_for(channels)
    x = np.array(ac.noise(oracle, channels, n, 29))
    want, _, _, _ = ac.run_stream(ac.device(dev), channels, (n,), x, T, phases)
    f = plain_run(dev, x, steps, T, phases, n)
    counts = f.out_len(n)
    pitch = int(counts.max()) + 37
    xin = bc.carve_input(dev, x, off_in)
    out = bc.carve(dev, F32, channels * pitch, off_out)
    snap = bc.snapshot(xin)
    got = f.process(xin.shaped(channels, n), out.shaped(channels, pitch))
    torch.cuda.synchronize()
    f.close()
    assert np.array_equal(got, counts)
    bc.check_bands(out, "asrc out")
    bc.check_untouched(xin, snap, "asrc in")
    o = bc.bits(out.view).reshape(channels, pitch)
    for c in range(channels):
        assert np.array_equal(o[c, :counts[c]], as_bits(want[c])), c
        assert np.all(o[c, counts[c]:] == bc.SENTINEL32), f"channel {c}: written behind its count"


def test_overlap_and_small_pitch_are_refused_and_leave_the_handle_alone(dev, oracle):
    channels, T, phases, n = 3, 32, 512, 600
    steps = np.array([0.5, 1.0, 2.0])
    x = np.array(ac.noise(oracle, channels, 2 * n, 31))
    f = plain_run(dev, x, steps, T, phases, n)
    g = plain_run(dev, x, steps, T, phases, n)                  # the twin that sees no refused call
    xd = torch.from_numpy(x).to(dev)
    counts = f.out_len(n)
    pitch = int(counts.max())
    for a, b in bc.overlap_cases(channels * n, channels * pitch, device=dev):
        a.copy_(xd[:, :n].reshape(-1))
        before = (bc.bits(a).copy(), bc.bits(b).copy())
        with pytest.raises(capi.LlzError, match="may not overlap"):
            f.process(a.view(channels, n), b.view(channels, pitch))
        torch.cuda.synchronize()
        assert np.array_equal(bc.bits(a), before[0]) and np.array_equal(bc.bits(b), before[1])
    small = torch.zeros(channels, pitch - 1, dtype=F32, device=dev)
    t0 = f.next_time()
    with pytest.raises(capi.LlzError, match="out_pitch"):
        f.process(xd[:, :n].contiguous(), small)
    torch.cuda.synchronize()
    assert not small.any() and all(np.array_equal(u, v) for u, v in zip(t0, f.next_time()))
    for k in range(2):                                          # the same call with room, and the next one: the twin's bits
        o1 = torch.zeros(channels, 2 * n + 8, dtype=F32, device=dev)
        o2 = torch.zeros_like(o1)
        c1 = f.process(xd[:, k * n:(k + 1) * n].contiguous(), o1)
        c2 = g.process(xd[:, k * n:(k + 1) * n].contiguous(), o2)
        torch.cuda.synchronize()
        assert np.array_equal(c1, c2) and np.array_equal(bc.bits(o1), bc.bits(o2)) and c1.min() > 0
    f.close(), g.close()


def test_host_pointers_give_the_bits_of_device_pointers(dev, oracle):
    channels, T, phases = 6, 32, 512
    steps = ac.steps_for(channels)
    x = np.array(ac.noise(oracle, channels, sum(ac.CALLS), 37))
    want, _, _, _ = ac.run_stream(ac.device(dev), channels, ac.CALLS, x, T, phases)
    f = plain_run(dev, x, steps, T, phases, max(ac.CALLS))
    pos, got = 0, [[] for _ in range(channels)]
    for n in ac.CALLS:
        counts = f.out_len(n)
        pitch = int(counts.max()) + 5
        out = np.full((channels, pitch), -7.0, dtype=np.float32)
        assert np.array_equal(f.process(np.ascontiguousarray(x[:, pos:pos + n]), out), counts)
        pos += n
        for c in range(channels):
            got[c].append(out[c, :counts[c]])
            assert np.all(out[c, counts[c]:] == -7.0), "a host row was written behind its count"
    f.close()
    for c in range(channels):
        assert np.array_equal(as_bits(np.concatenate(got[c])), as_bits(want[c])), c


# ------------------------------------------------------------------------------------------------ 7. reset
def test_reset_gives_a_fresh_handle(dev, oracle):
    channels, T, phases = 6, 32, 512
    x = ac.noise(oracle, channels, sum(ac.CALLS), 41)
    want, _, counts_w, times_w = ac.run_stream(ac.device(dev), channels, ac.CALLS, x, T, phases)
    r = ac.Device(dev, channels, max(ac.CALLS), step=float(ac.STEPS[0]), taps=T, phases=phases)
    for c in range(1, channels):
        r.set_step(c, ac.STEPS[c], 0)
    r.set_step(4, 2.0, 100000)
    r.process(np.array(x[:, :700]) * 3)                         # some other stream, and a glide left running
    r.set_step(4, ac.STEPS[4], 100000)
    r.process(x[:, :5])
    r.reset()
    assert all(not v.any() for v in r.next_time())
    pos, got = 0, [[] for _ in range(channels)]
    for n in ac.CALLS:
        ys, _, _ = r.process(x[:, pos:pos + n])
        pos += n
        for c in range(channels):
            got[c].append(ys[c])
    assert all(np.array_equal(u, v) for u, v in zip(r.next_time(), times_w[-1]))
    r.close()
    for c in range(channels):
        assert np.array_equal(as_bits(np.concatenate(got[c])), as_bits(want[c])), c


# ------------------------------------------------------------------------------------------------ 8. end to end
def test_sine_through_a_running_glide(dev):
    err_m, worst = ac.check_sine(ac.device(dev))
    assert worst <= 1.0
