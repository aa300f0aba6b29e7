"""Shared pieces of the per-band postfilter's tests (test_suppress_bands_host.py, test_suppress_bands_gpu.py;
llz_suppress_bands_mc, include/llz_suppress_bands.h): the MODEL of the definition in float64 (the reference everywhere) and in
float32 (the device's stand-in on a machine without a GPU), the definition as plain loops for one bin, the device runner, the
scene, the checks and the property case.  The model is written from the definition in llz_suppress_bands.h in plain numpy and knows
nothing of the kernel.  The generator of every signal is adapt_bands_checks.gaussian(oracle, ...).

The definition, per (channel, bin): seven state values S, Smin, Stmp, q, N, R, Z (0 at init but q = 1), per channel a floor gmin, a
leakage eta and a flag; constants omas = 1 - as, omaq = 1 - aq, omad = 1 - ad, omb = 1 - beta, kt = 1 / (t1 - t0) formed in float32
(the float64 model takes these float32 VALUES).  For frame n since init: pe = |e|^2, py = |y|^2 or 0; below W frames S and N are
running means (step c = 1 / (n + 1) until omas, omad are larger), Smin = Stmp = S; from W on S is smoothed by as, the two windows
of the minimum swap where n % W == 0, J = clamp((t1 Smin - S) / (Smin + delta) kt, 0, 1), q <- aq q + omaq J, step = omad q.  Then
N <- N + step (pe - N); R = max(eta py, rho R); Q = N + delta + R; prio = beta Z / Q + omb max(pe / Q - 1, 0);
G = clamp(prio / (1 + prio), gmin, 1); o = G e; Z = |o|^2.

Limits against the float64 model (none of them taken from the device's results), TOL = adapt_bands_checks.TOL = 1e-5:
  * o: per (channel, bin, run of 16 frames) rms(o - o_ref) <= TOL rms(e of that channel and bin over the case);
  * g: |g - g_ref| <= TOL;  q: |q - q_ref| <= TOL;
  * S, Smin, Stmp, N, R: |v - v_ref| <= TOL v_ref;
  * Z: |Z - Z_ref| <= 4 TOL |e|^2 of the last frame;
  * the zero bin of channel 0 (e = 0 throughout): o, S and N exactly 0 and g = gmin;
  * o bit-equal to float32(g) e everywhere.
The float32 model sits below half of every limit on every case; the five planted faults each miss a limit by more than 1e3.

The scene of a shape (bins, frames, W), one per channel count: unit-variance noise throughout; bursts 20 dB above it over W / 3
frames from frame 3 W / 2 in every 8th bin; a noise step of +10 dB from frame 9 W / 4 that is held to the end; from frame 3 W a
section where y is unit-variance Gaussian (zero before it) and, in the ECHO channels (every third, c % 3 == 2, which run at
eta = 0.01; the others at eta = 0), e is 0.1 |y| times Gaussian on noise 30 dB below unit variance; in channel 0 a bin with e = 0
throughout."""
import numpy as np

from tests import adapt_bands_checks as bc

TOL = bc.TOL
DEFAULTS = dict(window=128, as_=0.8, aq=0.2, ad=0.95, t0=2.0, t1=5.0, beta=0.98, rho=0.6, delta=1e-6)
GMIN, ETA = 0.1, 0.01
STATES = ("S", "Smin", "Stmp", "q", "N", "R", "Z")
# (bins, frames, W): bins of 5 and 33 put several channels into one wave, 129 and 65 straddle rows; every W is crossed, and every
# case sees at least three window swaps
SHAPES = [(5, 200, 16), (33, 300, 64), (129, 300, 64), (65, 700, 128)]
CHANNELS = (3, 37)
LONG = (2049, 64, 16, 3)        # bins, frames, W, channels: a row longer than any workgroup
ZERO_BIN = 1                    # the bin of channel 0 with e = 0 (no burst bin: those are 0, 8, 16, ..)
FAULTS = ("windows_never_swap", "step_from_speech_probability", "echo_without_hold", "z_from_input", "startup_skipped")
cached, cbits, split, ratio = bc.cached, bc.cbits, bc.split, bc.ratio


def constants(as_, aq, ad, beta, t0, t1):
    """(omas, omaq, omad, omb, kt) as the host layer forms them: float32 operations on float32 values"""
    one = np.float32(1)
    f = np.float32
    return f(one - f(as_)), f(one - f(aq)), f(one - f(ad)), f(one - f(beta)), f(one / f(f(t1) - f(t0)))


# ------------------------------------------------------------------------------------------------ the scene
def echo_channels(channels):
    return np.arange(channels) % 3 == 2


def scene(oracle, bins, frames, W, channels):
    """(e, y, eta): e, y [channels, frames, bins] complex64, eta [channels] float32"""
    def make():
        shape = (channels, frames, bins)
        noise, burst, ys, eg = (bc.gaussian(oracle, *shape, seed=s + 11 * bins + W).astype(np.complex128) for s in (301, 302, 303, 304))
        m = np.arange(frames)
        e = noise.copy()
        lo = 3 * W // 2
        e[:, lo:lo + W // 3, ::8] += 10.0 * burst[:, lo:lo + W // 3, ::8]                       # 20 dB above the noise
        e[:, 9 * W // 4:] *= np.sqrt(10.0)                                                      # +10 dB, held to the end
        sec = m >= 3 * W
        y = np.where(sec[None, :, None], ys, 0)
        echo = echo_channels(channels)
        quiet = 0.1 * np.abs(y) * eg + 10.0 ** (-30 / 20) * noise
        e[echo] = np.where(sec[None, :, None], quiet[echo], e[echo])
        assert bins > ZERO_BIN
        e[0, :, ZERO_BIN] = 0
        e, y = e.astype(np.complex64), y.astype(np.complex64)
        eta = np.where(echo, np.float32(ETA), np.float32(0)).astype(np.float32)
        for a in (e, y, eta):
            a.setflags(write=False)
        return e, y, eta
    return cached(("suppress scene", bins, frames, W, channels), make)


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """llz_suppress_bands_mc from the definition.  prec: 64 (the reference) or 32 (every operation rounded to float32, a fused
    multiply-add through one float64 product and sum).  fault: None or one of FAULTS, for the tests that show the limits are not
    slack."""

    def __init__(self, channels, bins, window=128, as_=0.8, aq=0.2, ad=0.95, t0=2.0, t1=5.0, beta=0.98, rho=0.6, delta=1e-6,
                 prec=64, fault=None):
        assert fault is None or fault in FAULTS
        self.rt = rt = np.float32 if prec == 32 else np.float64
        self.ct = np.complex64 if prec == 32 else np.complex128
        self.channels, self.bins, self.W, self.fault = channels, bins, int(window), fault
        self.omas, self.omaq, self.omad, self.omb, self.kt = (rt(v) for v in constants(as_, aq, ad, beta, t0, t1))
        self.aq, self.beta, self.rho, self.delta, self.t1 = (rt(np.float32(v)) for v in (aq, beta, rho, delta, t1))
        self.on = np.ones(channels, bool)
        self.gmin = np.full(channels, rt(np.float32(GMIN)), rt)
        self.eta = np.zeros(channels, rt)
        self.reset()

    def reset(self):
        z = lambda: np.zeros((self.channels, self.bins), self.rt)          # noqa: E731
        self.st = {name: z() for name in STATES}
        self.st["q"][:] = 1
        self.count = 0

    def set_floor(self, first, gmin):
        v = np.atleast_1d(np.asarray(gmin, np.float32))
        self.gmin[first:first + len(v)] = v

    def set_leak(self, first, eta):
        v = np.atleast_1d(np.asarray(eta, np.float32))
        self.eta[first:first + len(v)] = v

    def set_enable(self, first, on):
        on = np.atleast_1d(on) != 0
        self.on[first:first + len(on)] = on

    def get_state(self, which):
        which = STATES[which] if isinstance(which, int) else which
        return self.st[which].astype(np.float32)

    def frames(self):
        return self.count

    def fma(self, a, b, c):
        if self.rt is np.float32:
            return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
        return a * b + c

    def process(self, e, y=None, want_g=True):
        """e, y complex [channels, frames, bins] -> (o, g) in the model's precision"""
        rt, fma, W, fault = self.rt, self.fma, self.W, self.fault
        e = np.asarray(e).astype(self.ct)
        y = None if y is None else np.asarray(y).astype(self.ct)
        o, g = np.empty(e.shape, self.ct), np.empty(e.shape, rt)
        one, zero = rt(1), rt(0)
        gmin, eta, on = self.gmin[:, None], self.eta[:, None], self.on[:, None]
        for m in range(e.shape[1]):
            n = self.count + m
            er, ei = e[:, m].real.astype(rt), e[:, m].imag.astype(rt)
            S, Smin, Stmp, q, N, R, Z = (self.st[k] for k in STATES)
            pe = fma(ei, ei, er * er)
            py = np.zeros_like(pe) if y is None else fma(y[:, m].imag.astype(rt), y[:, m].imag.astype(rt),
                                                          y[:, m].real.astype(rt) * y[:, m].real.astype(rt))
            if n < W and fault != "startup_skipped":
                c = one / rt(n + 1)
                sa = c if c > self.omas else self.omas
                S = fma(sa, pe - S, S)
                Smin, Stmp = S, S
                step = c if c > self.omad else self.omad
            else:
                S = fma(self.omas, pe - S, S)
                if n % W == 0 and fault != "windows_never_swap":
                    Smin = np.where(S < Stmp, S, Stmp)
                    Stmp = S
                else:
                    Smin = np.where(S < Smin, S, Smin)
                    Stmp = np.where(S < Stmp, S, Stmp)
                rm = one / (Smin + self.delta)
                J = (fma(self.t1, Smin, -S) * rm) * self.kt
                J = np.where(J < 0, zero, J)
                J = np.where(J > 1, one, J)
                q = fma(self.aq, q, self.omaq * J)
                step = self.omad * ((one - q) if fault == "step_from_speech_probability" else q)
            N = fma(step, pe - N, N)
            a, b = eta * py, self.rho * R
            R = a if fault == "echo_without_hold" else np.where(a > b, a, b)
            Q = (N + self.delta) + R
            rq = one / Q
            ml = pe * rq - one
            ml = np.where(ml < 0, zero, ml)
            prio = fma(self.beta, Z * rq, self.omb * ml)
            rg = one / (one + prio)
            G = prio * rg
            G = np.where(G < gmin, gmin, G)
            G = np.where(G > 1, one, G).astype(rt)
            orr, oi = G * er, G * ei
            Z = pe if fault == "z_from_input" else fma(oi, oi, orr * orr)
            new = dict(zip(STATES, (S, Smin, Stmp, q, N, R, Z)))
            for k in STATES:
                self.st[k] = np.where(on, new[k], self.st[k]).astype(rt)
            o[:, m] = np.where(on, orr + 1j * oi, e[:, m])
            g[:, m] = np.where(on, G, one)
        self.count += e.shape[1]
        return o, g

    def close(self):
        pass


def model32(channels, bins, **kw):
    """the device's stand-in: the float32 model behind the runners' interface"""
    return Model(channels, bins, prec=32, **kw)


def definition_loops(e, y=None, gmin=GMIN, eta=0.0, window=128, as_=0.8, aq=0.2, ad=0.95, t0=2.0, t1=5.0, beta=0.98, rho=0.6,
                     delta=1e-6):
    """one (channel, bin) stream from the definition written out as plain loops over Python numbers: (o, g, state dict)"""
    omas, omaq, omad, omb, kt = (float(v) for v in constants(as_, aq, ad, beta, t0, t1))
    aq, beta, rho, delta, t1, gmin, eta = (float(np.float32(v)) for v in (aq, beta, rho, delta, t1, gmin, eta))
    S = Smin = Stmp = N = R = Z = 0.0
    q = 1.0
    o, g = [], []
    for n in range(len(e)):
        pe = abs(complex(e[n])) ** 2
        py = 0.0 if y is None else abs(complex(y[n])) ** 2
        if n < window:
            c = 1.0 / (n + 1)
            S += max(c, omas) * (pe - S)
            Smin = Stmp = S
            step = max(c, omad)
        else:
            S += omas * (pe - S)
            if n % window == 0:
                Smin, Stmp = min(S, Stmp), S
            else:
                Smin, Stmp = min(S, Smin), min(S, Stmp)
            J = min(max((t1 * Smin - S) / (Smin + delta) * kt, 0.0), 1.0)
            q = aq * q + omaq * J
            step = omad * q
        N += step * (pe - N)
        R = max(eta * py, rho * R)
        Q = N + delta + R
        prio = beta * Z / Q + omb * max(pe / Q - 1.0, 0.0)
        G = min(max(prio / (1.0 + prio), gmin), 1.0)
        o.append(G * complex(e[n]))
        g.append(G)
        Z = abs(o[-1]) ** 2
    return np.array(o), np.array(g), dict(S=S, Smin=Smin, Stmp=Stmp, q=q, N=N, R=R, Z=Z)


# ------------------------------------------------------------------------------------------------ the device
def sizes(calls, frames):
    """how `frames` are grouped into calls (None: all at once; a number: that many per call; a list: those counts in turn,
    repeated, 0 = an empty call)"""
    if calls is None:
        return [frames]
    steps = [calls] if isinstance(calls, int) else list(calls)
    out, k = [], 0
    while sum(out) < frames:
        out.append(min(steps[k % len(steps)], frames - sum(out)))
        k += 1
    return out


class Device:
    """filters.SuppressBandsMC behind the model's interface: complex numpy in and out through device tensors, outputs preset to
    NaN; calls: see sizes()"""

    def __init__(self, dev, channels, bins, calls=None, **kw):
        from llzlab_amd import filters
        self.dev, self.channels, self.bins, self.calls = dev, channels, bins, calls
        self.f = filters.SuppressBandsMC(channels, bins, **kw)
        assert self.f.plan() == (0, 64, -(-channels * bins // 64), 1), self.f.plan()

    def process(self, e, y=None, want_g=True):
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)           # noqa: E731
        new = lambda n: torch.full((self.channels, n, self.bins), float("nan"), dtype=torch.float32, device=self.dev)  # noqa: E731
        os, gs, at = [], [], 0
        for n in sizes(self.calls, e.shape[1]):
            ins = [up(a) for a in split(e[:, at:at + n])]
            ys = [None, None] if y is None else [up(a) for a in split(y[:, at:at + n])]
            ore, oim, g = new(n), new(n), (new(n) if want_g else None)
            self.f.process(*ins, ore, oim, *ys, g)
            if n:
                assert self.f.plan()[0] == (0 if y is None else 1)
            os.append(ore.cpu().numpy() + 1j * oim.cpu().numpy())
            gs.append(g.cpu().numpy() if want_g else None)
            at += n
        o = np.concatenate(os, axis=1).astype(np.complex64)
        return o, (np.concatenate(gs, axis=1) if want_g else None)

    def set_floor(self, first, gmin):
        self.f.set_floor(first, gmin)

    def set_leak(self, first, eta):
        self.f.set_leak(first, eta)

    def set_enable(self, first, on):
        self.f.set_enable(first, on)

    def get_state(self, which):
        return self.f.get_state(which)

    def reset(self):
        self.f.reset()

    def frames(self):
        return self.f.frames()

    def close(self):
        self.f.close()


def device(dev, calls=None):
    return lambda *a, **kw: Device(dev, *a, calls=calls, **kw)


def states(r):
    """all seven state arrays of a runner, float32 [7, channels, bins]"""
    return np.stack([r.get_state(k) for k in range(len(STATES))])


# ------------------------------------------------------------------------------------------------ the checks
def reference(oracle, bins, frames, W, channels, with_y=True):
    """the float64 model over the whole scene: (o, g, states [7, channels, bins] in float64), computed once"""
    def make():
        e, y, eta = scene(oracle, bins, frames, W, channels)
        m = Model(channels, bins, window=W, prec=64)
        m.set_leak(0, eta)
        o, g = m.process(e, y if with_y else None)
        return o, g, np.stack([m.st[k] for k in STATES])
    return cached(("suppress ref", bins, frames, W, channels, with_y), make)


def measure_parity(make, oracle, bins, frames, W, channels, with_y=True, want_g=True):
    """one scene through `make(channels, bins, window=W)` against the float64 model: 'o', 'g' and the seven states as ratios to
    their limits (the worst over the case), the zero bin and o = g e checked on the way"""
    e, y, eta = scene(oracle, bins, frames, W, channels)
    o_ref, g_ref, s_ref = reference(oracle, bins, frames, W, channels, with_y)
    what = f"suppress bins={bins} W={W} {channels}ch x {frames} frames{'' if with_y else ', no y'}{'' if want_g else ', no g'}"
    r = make(channels, bins, window=W)
    r.set_leak(0, eta)
    o, g = r.process(e, y if with_y else None, want_g=want_g)
    s = states(r)
    assert r.frames() == frames, f"{what}: frames() is {r.frames()}"
    r.close()
    assert o.shape == e.shape and s.shape == (len(STATES), channels, bins) and (g is None or g.shape == e.shape)
    e128 = e.astype(np.complex128)
    out = {}
    if g is not None:
        if g.dtype == np.float32:
            want = g[..., None] * np.stack(split(e), axis=-1)
            assert np.array_equal(np.stack(split(o), axis=-1).view(np.uint32), want.view(np.uint32)), f"{what}: o is not g e in float32"
        assert np.all(g[0, :, ZERO_BIN] == np.float32(GMIN)), f"{what}: g of the bin with e = 0 is not the floor"
        out["g"] = ratio(np.abs(g.astype(np.float64) - g_ref), TOL)
    assert not np.any(o[0, :, ZERO_BIN]) and s[0, 0, ZERO_BIN] == 0 and s[4, 0, ZERO_BIN] == 0, \
        f"{what}: the bin with e = 0 is not exactly zero"
    e_rms = np.sqrt(np.mean(np.abs(e128) ** 2, axis=1))                                        # [channels, bins]
    err = bc.run_rms(o.astype(np.complex128) - o_ref)
    out["o"] = ratio(err, TOL * np.broadcast_to(e_rms[:, None, :], err.shape))
    s = s.astype(np.float64)
    for k, name in enumerate(STATES):
        d = np.abs(s[k] - s_ref[k])
        if name == "q":
            out[name] = ratio(d, TOL)
        elif name == "Z":
            out[name] = ratio(d, 4 * TOL * np.abs(e128[:, -1]) ** 2)
        else:
            out[name] = ratio(d, TOL * s_ref[k])
    print(f"{what}: worst ratios to the limits: " + ", ".join(f"{k} {v:.3g}" for k, v in out.items()))
    return out


def check_parity(make, oracle, bins, frames, W, channels, share=1.0, **kw):
    """every figure within `share` of its limit (the float32 model is asked for half)"""
    m = measure_parity(make, oracle, bins, frames, W, channels, **kw)
    for name, v in m.items():
        assert v <= share, f"suppress bins={bins} W={W} {channels}ch: {name} at {v:.3g} of its limit (asked: {share})"
    return m


def worst_miss(make, oracle, bins, frames, W, channels):
    """the largest ratio of a figure to its limit (a run that ends in NaN or inf, or breaks an exact check, misses by inf)"""
    with np.errstate(all="ignore"):
        try:
            return max(measure_parity(make, oracle, bins, frames, W, channels).values())
        except AssertionError:
            return float("inf")


# ------------------------------------------------------------------------------------------------ the properties
# five channels of 33 bins at the defaults (W = 128), 700 frames, unit-variance noise behind the start-up in all but the last two:
#   0  noise only
#   1  a burst 20 dB up over frames 300..339 in every 8th bin
#   2  a noise step of +10 dB from frame 300
#   3  echo, eta = 0:     from frame 300 on y unit-variance Gaussian, e = 0.1 |y| Gaussian on noise 30 dB down (noise alone before)
#   4  echo, eta = 0.01:  the same signals
# the state is read behind the frames PROP_MARKS
PROP = dict(channels=5, bins=33, frames=700, at=300, burst=40)
PROP_MARKS = (300, 340, 360, 556, 700)


def prop_case(oracle):
    """(e, y, eta)"""
    def make():
        C, B, F, at = PROP["channels"], PROP["bins"], PROP["frames"], PROP["at"]
        noise, burst, ys, eg = (bc.gaussian(oracle, C, F, B, seed=s).astype(np.complex128) for s in (411, 412, 413, 414))
        e = noise.copy()
        e[1, at:at + PROP["burst"], ::8] += 10.0 * burst[1, at:at + PROP["burst"], ::8]
        e[2, at:] *= np.sqrt(10.0)
        y = np.zeros_like(e)
        y[3:, at:] = ys[3, at:]
        e[3:] = 10.0 ** (-30 / 20) * noise[3]
        e[3:, at:] += 0.1 * np.abs(y[3:, at:]) * eg[3, at:]
        eta = np.array([0, 0, 0, 0, ETA], np.float32)
        e, y = e.astype(np.complex64), y.astype(np.complex64)
        for a in (e, y, eta):
            a.setflags(write=False)
        return e, y, eta
    return cached(("suppress prop case",), make)


def db(x):
    return 10 * np.log10(x)


def prop_figures(r, oracle):
    """runner r (a model or a device, PROP's shape, defaults) over the case -> the figures of the header's properties"""
    e, y, eta = prop_case(oracle)
    r.set_leak(0, eta)
    os, gs, Ns, at = [], [], {}, 0
    for mark in PROP_MARKS:
        o, g = r.process(e[:, at:mark], y[:, at:mark])
        os.append(o)
        gs.append(g)
        Ns[mark] = r.get_state(STATES.index("N")).astype(np.float64)
        at = mark
    r.close()
    o, g = np.concatenate(os, axis=1).astype(np.complex128), np.concatenate(gs, axis=1).astype(np.float64)
    p = lambda a, c, lo, hi: np.mean(np.abs(a[c, lo:hi].astype(np.complex128)) ** 2)           # noqa: E731
    t, bl = PROP["at"], PROP["burst"]
    return {
        "noise_attenuation_db": float(db(p(e, 0, 300, 700) / p(o, 0, 300, 700))),
        "burst_gain": float(np.median(g[1, t + 4:t + bl, ::8])),
        "gain_behind_burst": float(np.median(g[1, t + bl + 20:t + bl + 40, ::8])),
        "burst_noise_rise": float(max(np.max(Ns[m][1, ::8] / Ns[300][1, ::8]) for m in (340, 360))),
        "step_noise_db": float(db(np.median(Ns[556][2]) / 10.0)),
        "echo_attenuation_db_eta0": float(db(p(e, 3, t, t + 128) / p(o, 3, t, t + 128))),      # the section's first W frames
        "echo_attenuation_db": float(db(p(e, 4, t, t + 128) / p(o, 4, t, t + 128))),
    }


def prop_float64(oracle):
    def make():
        return prop_figures(Model(PROP["channels"], PROP["bins"], prec=64), oracle)
    return cached(("suppress prop f64",), make)


def prop_check(f):
    """the properties with their margins: 1 dB on a level, 0.05 on a gain, against the float64 model's measured figures (the test
    files' docstrings and DESIGN.md K4m hold them)"""
    assert f["noise_attenuation_db"] >= PROP_FIGURES["noise_attenuation_db"] - 1, f
    assert f["noise_attenuation_db"] <= 20.0 + 1e-3, f                                          # the floor bounds it
    assert f["burst_gain"] >= PROP_FIGURES["burst_gain"] - 0.05, f
    assert f["gain_behind_burst"] <= GMIN + 0.05, f
    assert f["burst_noise_rise"] <= PROP_FIGURES["burst_noise_rise"] * 10 ** 0.1, f
    assert abs(f["step_noise_db"]) <= 1.0 + abs(PROP_FIGURES["step_noise_db"]), f
    assert f["echo_attenuation_db_eta0"] <= PROP_FIGURES["echo_attenuation_db_eta0"] + 1, f
    assert f["echo_attenuation_db"] >= PROP_FIGURES["echo_attenuation_db"] - 1, f


# the float64 model's figures on prop_case (measured once and written down; test_suppress_bands_host.py asserts the model still
# gives them)
PROP_FIGURES = {
    "noise_attenuation_db": 19.88,          # noise only, frames 300..699: output below input (the floor of 0.1 bounds it at 20)
    "burst_gain": 0.971,                    # median g in the burst's bins from its fifth frame on
    "gain_behind_burst": 0.100,             # median g there 20..39 frames behind the burst: the floor
    "burst_noise_rise": 3.09,               # N in the burst's bins behind the burst and 20 frames later / before it, the worst bin
    "step_noise_db": -1.05,                 # median N 2 W frames behind the +10 dB step, relative to the new level
    "echo_attenuation_db_eta0": 3.42,       # the echo section's first W frames at eta = 0
    "echo_attenuation_db": 19.97,           # ... at eta = 0.01
}


# ------------------------------------------------------------------------------------------------ end to end
def e2e_float64(oracle):
    """the float64 chain on kalman_bands_checks.e2e_case's signals: pfb_checks' float64 bank in TIME phase, the float64 Kalman
    model, the float64 postfilter on (e, y) at ETA, the float64 synthesis of o, of e and of d; returns (residual of o, residual of
    e) relative to d per channel over the last quarter (adapt_bands_checks.e2e_residual)"""
    def make():
        from tests import kalman_bands_checks as kc
        from tests import pfb_checks as pc
        x, d, w = kc.e2e_case(oracle)
        c, M, P, os = (kc.E2E[k] for k in ("channels", "M", "P", "os"))
        X, _ = pc.analysis(x, w, M, P, os, pc.TIME)
        D, _ = pc.analysis(d, w, M, P, os, pc.TIME)
        X, D = X.astype(np.complex64), D.astype(np.complex64)
        m = kc.Model(c, M // 2 + 1, kc.E2E["taps"], prec=64, **kc.e2e_params(X))
        e, y = m.process(X, D)
        s = Model(c, M // 2 + 1, prec=64, **e2e_params(D))
        s.set_leak(0, np.full(c, ETA, np.float32))
        o, _ = s.process(e.astype(np.complex64), y.astype(np.complex64))
        ot, _ = pc.synthesis(*split(o), w, M, P, os, pc.TIME)
        et, _ = pc.synthesis(*split(e), w, M, P, os, pc.TIME)
        dt, _ = pc.synthesis(*split(D), w, M, P, os, pc.TIME)
        return bc.e2e_residual(ot, dt), bc.e2e_residual(et, dt)
    return cached(("suppress e2e f64",), make)


def e2e_params(D):
    """delta for bands that are not of unit variance: 1e-6 of the microphone bands' mean power"""
    return dict(delta=float(1e-6 * np.mean(np.abs(D) ** 2)))
