"""Shared pieces of the arbitrary-ratio resampler's tests (test_asrc_host.py, test_asrc_gpu.py; llz_asrc_mc, include/llz_asrc.h):
the MODEL of the definition -- time in Python integers by the recurrence t_(j+1) = t_j + inc_j, samples in float64 (the reference
everywhere) or in float32 with the device's order of operations (the device's stand-in on a machine without a GPU) --, the
cases, the two runners and the checks.  The model knows nothing of the kernel: no closed form, no tiles, no history buffer (it
keeps the whole input), no table padding.

The limit, per sample (none of it taken from the device's results): |y - y_model| <= 2 (T + 2) u A_j, u = 2^-24, A_j = sum_k
|x_k| (|G[p][k]| + |G[p+1][k]|).  First order: a coefficient costs at most 2 u (|G_p| + |G_(p+1)|) (one subtraction, one fma), an
fma chain of T terms T u sum |x c|: (T + 2) u A_j; the limit doubles that for the second-order terms.  Counts and times must
equal the integer model exactly, the table the model's bit for bit."""
import copy

import numpy as np

from llzlab_amd import filters

U = 2.0 ** -24
KAISER = filters.KAISER
# the steps of the issue, spread over the channels: channel c takes STEPS[c % 6]
STEPS = (1.0 / 16, 0.3337, 1.0, 1.0 + 2.0 ** -32, 160.0 / 147, 16.0)
CALLS = (257, 1, 1000)                      # the three calls of the dense case
SHAPES = ((4, 256), (32, 512), (128, 4096))            # (taps, phases): the LDS form twice, the global form
CHANNELS = (3, 37)
CUTOFF = 0.5
FAULTS = ("phase_row", "no_a", "sample_index", "no_quadratic", "short_history")
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def steps_for(channels):
    return np.array([STEPS[c % len(STEPS)] for c in range(channels)])


def to_inc(step):
    """llround(step 2^32): half away from zero, on the exact product (a power-of-two scaling of a double is exact)"""
    v = float(step) * 2.0 ** 32
    return int(np.floor(v + 0.5))


def table(T, phases, cutoff=CUTOFF, gain=1.0, win=KAISER):
    """G[p][k] = float32(gain phases h[k phases + p]), p <= phases, k < T, from the host design code"""
    def make():
        h = filters.fir_design("lpf", phases * T + 1, cutoff / phases, 0.0, win) * (gain * phases)
        g = np.empty((phases + 1, T), dtype=np.float32)
        g[:phases] = h[:phases * T].reshape(T, phases).T
        g[phases] = h[phases::phases][:T]
        g.setflags(write=False)
        return g
    return cached(("G", T, phases, cutoff, gain, win), make)


def noise(oracle, channels, n, seed):
    def make():
        x = oracle.synth_f32(channels, n, seed=seed)
        x.setflags(write=False)
        return x
    return cached(("x", channels, n, seed), make)


class Channel:
    """the integer state of one channel, straight from the definition"""

    def __init__(self, inc, t=0):
        self.t, self.inc, self.target, self.dinc, self.left = t, inc, inc, 0, 0

    def set_step(self, step, ramp, fault=None):
        self.target = to_inc(step)
        if ramp == 0:
            self.inc, self.dinc, self.left = self.target, 0, 0
        else:
            d = self.target - self.inc
            self.dinc = abs(d) // ramp * (1 if d >= 0 else -1)          # truncates toward zero
            self.left = ramp
        if fault == "no_quadratic":
            self.dinc = 0                                               # inc stays put through the glide, then jumps

    def reset(self):
        self.t, self.inc, self.dinc, self.left = 0, self.target, 0, 0

    def take(self, limit):
        """the times of the outputs with t >> 32 <= limit, by the recurrence; the state moves behind them"""
        times = []
        while self.t >> 32 <= limit:
            times.append(self.t)
            self.t += self.inc
            if self.left:
                self.left -= 1
                self.inc = self.inc + self.dinc if self.left else self.target
        return times


class Model:
    """channels x samples through the definition; prec 64: the reference, prec 32: float32 in the device's order of operations
    (d = G[p+1] - G[p]; c = fma(a, d, G[p]); y = fma(x, c, y), k ascending; an fma is the exact double product and sum rounded
    once more to float32, which differs from the true fma in rare double roundings only).  fault: one of FAULTS."""

    def __init__(self, channels, frame_len, step=1.0, taps=32, phases=512, cutoff=CUTOFF, gain=1.0, win=KAISER, prec=64, fault=None,
                 start=None):
        self.C, self.T, self.phases, self.prec, self.fault = channels, taps, phases, prec, fault
        self.G = table(taps, phases, cutoff, gain, win)
        self.logphi = phases.bit_length() - 1
        self.ch = [Channel(to_inc(step)) for _ in range(channels)]
        self.x = np.zeros((channels, 0), dtype=np.float32)
        self.call_start = 0
        if start is not None:                                           # a fresh model started at a time, after some input
            x, times, incs = start
            self.x = np.array(x, dtype=np.float32)
            self.call_start = self.x.shape[1]
            for c in range(channels):
                self.ch[c] = Channel(incs[c], times[c])

    def set_step(self, first, step, ramp=0):
        for i, s in enumerate(np.atleast_1d(step)):
            self.ch[first + i].set_step(float(s), ramp, self.fault)

    def reset(self):
        self.x = np.zeros((self.C, 0), dtype=np.float32)
        self.call_start = 0
        for ch in self.ch:
            ch.reset()

    def next_time(self):
        return (np.array([ch.t >> 32 for ch in self.ch], dtype=np.int64),
                np.array([ch.t & 0xFFFFFFFF for ch in self.ch], dtype=np.int64))

    def out_len(self, n_in):
        limit = self.x.shape[1] + n_in - 1 - self.T // 2
        return np.array([len(copy.copy(ch).take(limit)) for ch in self.ch], dtype=np.int64)

    def samples(self, c, times):
        """(y, A) of channel c at `times` (Python ints), from all the input received so far"""
        T, sh = self.T, 32 - self.logphi
        n = np.array([v >> 32 for v in times], dtype=np.int64)
        frac = np.array([v & 0xFFFFFFFF for v in times], dtype=np.int64)
        p = frac >> sh
        a = (frac & ((1 << sh) - 1)).astype(np.float64) * 2.0 ** -sh
        if self.fault == "phase_row":
            p = np.minimum(p + 1, self.phases - 1)
        if self.fault == "no_a":
            a = np.zeros_like(a)
        if self.fault == "sample_index":
            n = n + 1
        x = self.x[c].astype(np.float64)
        if self.fault == "short_history":                               # the oldest sample of the history reads as zero
            x = x.copy()
            x[:max(self.call_start - (T - 2), 0)] = 0.0
        xp = np.concatenate([np.zeros(T), x, np.zeros(1)])              # zeros before the stream (and one for the faulty index)
        idx = T + n[:, None] + T // 2 - np.arange(T)[None, :]
        w = xp[idx]                                                     # [outputs, T]: x[n + T/2 - k]
        g0, g1 = self.G[p].astype(np.float64), self.G[p + 1].astype(np.float64)
        A = np.sum(np.abs(w) * (np.abs(g0) + np.abs(g1)), axis=1)
        if self.prec == 64:
            y = np.sum(w * (g0 + a[:, None] * (g1 - g0)), axis=1)
        else:
            f32 = np.float32
            d = (g1.astype(f32) - g0.astype(f32)).astype(np.float64)
            cc = (a[:, None] * d + g0).astype(f32).astype(np.float64)
            y = np.zeros(len(n), dtype=np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                for k in range(T):
                    y = (w[:, k] * cc[:, k] + y).astype(f32).astype(np.float64)
        return y, A

    def process(self, x):
        """x: [channels, n_in] -> (outputs per channel: list of float64 arrays, A per channel, times per channel)"""
        x = np.asarray(x, dtype=np.float32).reshape(self.C, -1)
        self.call_start = self.x.shape[1]
        self.x = np.concatenate([self.x, x], axis=1)
        limit = self.x.shape[1] - 1 - self.T // 2
        ys, As, ts = [], [], []
        for c in range(self.C):
            times = self.ch[c].take(limit)
            if times:                                                   # (in pieces: a long call's windows stay small)
                parts = [self.samples(c, times[i:i + 32768]) for i in range(0, len(times), 32768)]
                y, A = np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
            else:
                y, A = np.zeros(0), np.zeros(0)
            ys.append(y), As.append(A), ts.append(times)
        return ys, As, ts

    def close(self):
        pass


def model64(*args, **kw):
    return Model(*args, prec=64, **kw)


def model32(*args, **kw):
    return Model(*args, prec=32, **kw)


class Device:
    """filters.AsrcMC behind the model's interface: device tensors in, lists of per-channel arrays out"""

    def __init__(self, dev, channels, frame_len, step=1.0, taps=32, phases=512, cutoff=CUTOFF, gain=1.0, win=KAISER):
        self.dev, self.C = dev, channels
        self.f = filters.AsrcMC(channels, frame_len, step=step, taps=taps, phases=phases, cutoff=cutoff, gain=gain, win=win)

    def set_step(self, first, step, ramp=0):
        self.f.set_step(first, step, ramp)

    def reset(self):
        self.f.reset()

    def next_time(self):
        return self.f.next_time()

    def out_len(self, n_in):
        return self.f.out_len(n_in)

    def process(self, x):
        import torch
        x = np.array(x, dtype=np.float32).reshape(self.C, -1)         # (a copy: the cached inputs are read-only)
        counts = self.f.out_len(x.shape[1])
        pitch = max(int(counts.max()), 1)
        xd = torch.from_numpy(x).to(self.dev)
        out = torch.full((self.C, pitch), float("nan"), dtype=torch.float32, device=self.dev)
        got = self.f.process(xd, out)
        torch.cuda.synchronize()
        assert np.array_equal(got, counts), "the call's counts differ from out_len's"
        o = out.cpu().numpy()
        return [o[c, :counts[c]].copy() for c in range(self.C)], None, None

    def close(self):
        self.f.close()


def device(dev):
    return lambda *args, **kw: Device(dev, *args, **kw)


# ------------------------------------------------------------------------------------------------ the checks
def ratio_to_limit(y, ym, A, T):
    """the worst |y - ym| / (2 (T + 2) u A); where A = 0 both must be zero"""
    y, ym = np.asarray(y, np.float64), np.asarray(ym, np.float64)
    assert y.shape == ym.shape, (y.shape, ym.shape)
    if y.size == 0:
        return 0.0
    lim = 2.0 * (T + 2) * U * A
    err = np.abs(y - ym)
    r = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def run_stream(make, channels, calls, x, T, phases, steps=None, script=None, **kw):
    """x cut into `calls` through a runner; script: {call index: [(first, steps, ramp), ...]} applied in front of that call;
    returns (per-channel concatenated outputs, counts per call, next_time after each call)"""
    steps = steps_for(channels) if steps is None else steps
    r = make(channels, max(max(calls), 1), step=float(steps[0]), taps=T, phases=phases, **kw)
    for c in range(1, channels):
        if steps[c] != steps[0]:
            r.set_step(c, steps[c], 0)
    outs, counts, times, pos = [[] for _ in range(channels)], [], [], 0
    extra = [[] for _ in range(channels)]
    for i, n in enumerate(calls):
        for (first, st, ramp) in (script or {}).get(i, []):
            r.set_step(first, st, ramp)
        ys, As, _ = r.process(x[:, pos:pos + n])
        pos += n
        counts.append([len(y) for y in ys])
        times.append(tuple(np.array(v) for v in r.next_time()))
        for c in range(channels):
            outs[c].append(ys[c])
            if As is not None:
                extra[c].append(As[c])
    r.close()
    cat = [np.concatenate(o) if o else np.zeros(0) for o in outs]
    A = [np.concatenate(e) for e in extra] if extra[0] else None
    return cat, A, counts, times


def reference(oracle, channels, T, phases, calls=CALLS, script=None, seed=11, **kw):
    """the float64 model's run of the noise case, computed once and shared"""
    key = ("ref", channels, T, phases, tuple(calls), repr(script), seed, repr(sorted(kw.items())))
    x = noise(oracle, channels, sum(calls), seed)
    return x, cached(key, lambda: run_stream(model64, channels, calls, x, T, phases, script=script, **kw))


def check_against(make, oracle, channels, T, phases, calls=CALLS, script=None, what="dense", seed=11, **kw):
    """a runner against the float64 model on seeded noise: counts and times equal, every sample within the limit; returns the
    worst ratio"""
    x, (ym, A, counts_m, times_m) = reference(oracle, channels, T, phases, calls, script, seed=seed, **kw)
    y, _, counts, times = run_stream(make, channels, calls, x, T, phases, script=script, **kw)
    assert counts == counts_m, f"{what}: counts differ from the integer model's"
    for (w, f), (wm, fm) in zip(times, times_m):
        assert np.array_equal(w, wm) and np.array_equal(f, fm), f"{what}: next_time differs from the integer model's"
    worst = max(ratio_to_limit(y[c], ym[c], A[c], T) for c in range(channels))
    print(f"asrc {what} T={T} phases={phases} channels={channels}: worst ratio to the limit {worst:.3g}")
    return worst


# the glide script of case 3 over calls of GLIDE_CALLS samples: R = 1, 7 and 1000 in front of call 1 (R = 1000 at steps near 1 runs
# through calls 1 to 4), a set_step inside that glide in front of call 3, and a downward glide of 300 outputs that spans three calls
GLIDE_CALLS = (300, 257, 1, 400, 1, 130, 130, 130, 700)
GLIDE_STEPS = np.array([1.0, 0.75, 1.0, 2.0])
GLIDE_SCRIPT = {1: [(0, 1.01, 1), (1, 1.25, 7), (2, 1.003, 1000)], 3: [(2, 0.997, 600)], 5: [(3, 1.5, 300)]}


# Calls long enough for the tile walks of a workgroup (asrc.hip walks 2 tiles of 1024 outputs per workgroup from 8 tiles of the
# largest count on, 8 from 32, 32 from 128, and keeps the next tile's span in two registers per lane while it fits 2048 samples):
#   walk     a call of 40000 samples (43 tiles at 147/160: walks of 8), then one of 140000 (137 to 149 tiles: walks of 32), at steps
#            1.000023 and 1.9 (spans of 1056 and 1977 samples: both registers in use) and 147/160 gliding to 0.95
#   restage  one call of 150000 samples at steps 3 and 16 (spans beyond 2048 samples, staged in the loop; 10 tiles at step 16)
#            next to 1.5 (prefetched), in walks of 8
# (steps, calls, script, the least largest count of each call); the same stream cut into calls of LONG_CUT samples must give the
# same bits
LONG_CUT = 2500
LONG = {
    "walk": (np.array([1.000023, 147.0 / 160, 1.9]), (40000, 140000), {1: [(1, 0.95, 100000)]}, (32 * 1024, 128 * 1024)),
    "restage": (np.array([3.0, 16.0, 1.5]), (150000,), None, (32 * 1024,)),
}


def check_long(make, oracle, name, grouping=True, what="long"):
    """a long-call case against the float64 model (the limit, counts and times) and, with `grouping`, bit for bit against the
    same stream through the same runner in calls of LONG_CUT samples; returns the worst ratio to the limit"""
    steps, calls, script, least = LONG[name]
    channels, T, phases = len(steps), 32, 512
    x, (ym, A, counts_m, _) = reference(oracle, channels, T, phases, calls, script, seed=43, steps=steps)
    assert all(max(c) >= m for c, m in zip(counts_m, least)), "the case no longer reaches the walk it is there for"
    if name == "restage":
        assert counts_m[0][1] > 9 * 1024
    worst = check_against(make, oracle, channels, T, phases, calls=calls, script=script, what=f"{what} {name}", seed=43, steps=steps)
    assert worst <= 1.0, f"{what} {name}: a sample misses the limit by a factor of {worst:.3g}"
    if grouping:
        whole, _, _, _ = run_stream(make, channels, calls, x, T, phases, steps=steps, script=script)
        edges = np.cumsum((0,) + calls)
        assert all(e % LONG_CUT == 0 for e in edges)
        cut_script = {int(edges[i]) // LONG_CUT: v for i, v in (script or {}).items()}
        cut, _, counts, _ = run_stream(make, channels, (LONG_CUT,) * (int(edges[-1]) // LONG_CUT), x, T, phases, steps=steps,
                                       script=cut_script)
        for c in range(channels):
            assert np.array_equal(np.asarray(cut[c], np.float32).view(np.uint32), np.asarray(whole[c], np.float32).view(np.uint32)), \
                f"{what} {name}: channel {c} differs between long calls and calls of {LONG_CUT}"
    return worst


def check_glides(make, oracle, what="glides"):
    return check_against(make, oracle, 4, 32, 512, calls=GLIDE_CALLS, script=GLIDE_SCRIPT, what=what, steps=GLIDE_STEPS)


def sine_case(make):
    """case 8: a unit sine at 0.3 of Nyquist through (32, 512, Kaiser, cutoff 0.9) at step 1 gliding to 1.000123; returns the
    runner's outputs, the float64 model's, the limit per sample and the analytic sine at the model's times (the first and last T
    outputs, whose windows reach in front of the stream, left out)"""
    T, phases, n = 32, 512, 6000
    calls = (1000, 2000, 3000)
    x = np.sin(np.pi * 0.3 * np.arange(n)).astype(np.float32)[None, :]
    kw = dict(cutoff=0.9)
    script = {0: [(0, 1.000123, 4000)]}
    steps = np.array([1.0])

    def ref():
        r = Model(1, max(calls), step=1.0, taps=T, phases=phases, prec=64, **kw)
        r.set_step(0, 1.000123, 4000)
        ys, As, ts, pos = [], [], [], 0
        for c in calls:
            y, A, t = r.process(x[:, pos:pos + c])
            pos += c
            ys.append(y[0]), As.append(A[0]), ts.extend(t[0])
        return np.concatenate(ys), np.concatenate(As), ts
    ym, A, ts = cached(("sine",), ref)
    tt = np.array([v / 2.0 ** 32 for v in ts])
    s = np.sin(np.pi * 0.3 * tt)
    y, _, _, _ = run_stream(make, 1, calls, x, T, phases, steps=steps, script=script, **kw)
    keep = slice(T, len(ym) - T)
    return y[0][keep], ym[keep], 2.0 * (T + 2) * U * A[keep], s[keep]


def check_sine(make, what="sine"):
    y, ym, lim, s = sine_case(make)
    err_m = float(np.max(np.abs(ym - s)))
    over = np.abs(y - s) - err_m
    worst = float(np.max(over / lim))
    print(f"asrc {what}: the float64 model's own error {err_m:.3g}; the runner's excess over it, worst ratio to the limit {worst:.3g}")
    assert err_m < 1e-3, "the model itself does not resample the sine"
    assert worst <= 1.0
    return err_m, worst
