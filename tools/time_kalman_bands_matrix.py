"""multi-reference per-band Kalman filter (llz_kalman_bands_matrix_mc) per call next to the multi-reference per-band NLMS filter
(llz_adapt_bands_matrix_mc) at the same shapes and, at one input, next to the single-reference Kalman filter
(llz_kalman_bands_mc), adapting and frozen, the forms alternated round by round in one process:
    python tools/time_kalman_bands_matrix.py [outputs ...] [bins=129] [shapes=1x4,1x32,2x4,2x16,4x8,8x4] [frames=64]
  kalman:        KalmanBandsMatrixMC, every output adapting
  kalman frozen: no output adapting (y and e written, the history moved on, no update)
  nlms:          AdaptBandsMatrixMC, every output at mu = 0.5
  nlms frozen:   AdaptBandsMatrixMC, every output at mu = 0
  single, single frozen (inputs = 1 only): KalmanBandsMC on as many channels as outputs, each with a copy of the reference
Default outputs: 8 1024; shapes are inputs x taps.  The method is tools/time_kalman_bands.py's: every form is warmed with WARM
calls, a probe sizes its calls per window so that a window lasts about WINDOW_MS, then it is timed in ROUNDS such windows between
events; time per call: median, min and max over the windows.  Counts per (output, bin) and frame, J = inputs x taps: 32 bytes of
d, e, y (re and im) and the 8 I bytes of x that the outputs share through the caches; per CALL the state in and out is 16 J for
NLMS and 24 J + 8 for the Kalman filter.  Arithmetic of an adapting frame: NLMS 10 J fused multiply-adds and two quotients;
Kalman 25 J operations and one quotient (tools/time_kalman_bands.py has the count per tap)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
outs = [int(a) for a in sys.argv[1:] if "=" not in a] or [8, 1024]
bins = int(opts.get("bins", "129"))
shapes = [tuple(int(v) for v in s.split("x")) for s in opts.get("shapes", "1x4,1x32,2x4,2x16,4x8,8x4").split(",")]
frames = int(opts.get("frames", "64"))
ROUNDS, WARM, PROBE, WINDOW_MS = 5, 3, 20, 100.0
L = capi.lib()
def window(fn, steps):
    t = L.llz_hip_timer_new(); L.llz_hip_timer_start(t, None)
    for _ in range(steps): fn()
    L.llz_hip_timer_stop(t, None); ms = L.llz_hip_timer_ms(t) / steps; L.llz_hip_timer_free(t)
    return ms
def alternated(forms):
    ms = {name: [] for name, _ in forms}
    steps = {}
    for name, fn in forms:
        for _ in range(WARM): fn()
        steps[name] = max(PROBE, int(np.ceil(WINDOW_MS / window(fn, PROBE))))
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in forms:
            ms[name].append(window(fn, steps[name]))
    return ms, steps
def noise(rows, seed):
    b = [torch.empty(rows, frames, bins, dtype=torch.float32, device=dev) for _ in range(2)]
    for k, t in enumerate(b):
        filters.synth_f32(t.view(rows, frames * bins), seed + k)
    return tuple(b)
print(f"{ROUNDS} windows of about {WINDOW_MS:.0f} ms per form after {WARM} warm-up calls and a probe of {PROBE}, forms alternated; "
      f"{frames} frames per call, {bins} bins", flush=True)
for O in outs:
    d, e, y = noise(O, 3), noise(O, 5), noise(O, 7)
    for I, K in shapes:
        x = noise(I, 1)
        rng = np.random.default_rng(K)
        h = (rng.standard_normal((O, I, K, bins)) + 1j * rng.standard_normal((O, I, K, bins))) * np.exp(-np.arange(K) / (K / 4 + 1))[None, None, :, None]
        h /= np.sqrt(np.sum(np.abs(h) ** 2, axis=(1, 2), keepdims=True))
        k, z = (filters.KalmanBandsMatrixMC(I, O, bins, K) for _ in range(2))
        n, m = (filters.AdaptBandsMatrixMC(I, O, bins, K, mu=mu) for mu in (0.5, 0.0))
        z.set_adapt(0, np.zeros(O))
        for f in (k, z, n, m): f.set_taps(0, h)
        made = [k, z, n, m]
        forms = [("kalman", lambda: k.process(x, d, e, y)), ("kalman frozen", lambda: z.process(x, d, e, y)),
                 ("nlms", lambda: n.process(x, d, e, y)), ("nlms frozen", lambda: m.process(x, d, e, y))]
        if I == 1:
            xs = tuple(t.expand(O, frames, bins).contiguous() for t in x)
            s, sz = (filters.KalmanBandsMC(O, bins, K) for _ in range(2))
            sz.set_adapt(0, np.zeros(O))
            for f in (s, sz): f.set_taps(0, h[:, 0])
            made += [s, sz]
            forms += [("single", lambda: s.process(*xs, *d, *e, *y)), ("single frozen", lambda: sz.process(*xs, *d, *e, *y))]
        inputs, ceiling, threads, groups, launches = k.plan()
        torch.cuda.synchronize()
        ms, steps = alternated(forms)
        med = {name: float(np.median(v)) for name, v in ms.items()}
        line = f"{O:5d} out x {bins} bins, {I} in x {K:2d} taps (ceiling {ceiling}, {groups} workgroups of {threads}):"
        for name, _ in forms:
            line += (f" {name} {1e3 * med[name]:9.2f} us/call (min {1e3 * min(ms[name]):.2f} max {1e3 * max(ms[name]):.2f}, "
                     f"{steps[name]} calls/window), {1e3 * med[name] / frames:.3f} us/frame |")
        line += (f" kalman / nlms = {med['kalman'] / med['nlms']:.3f}, frozen / nlms frozen = {med['kalman frozen'] / med['nlms frozen']:.3f},"
                 f" kalman / frozen = {med['kalman'] / med['kalman frozen']:.3f}")
        if I == 1:
            line += f", kalman / single = {med['kalman'] / med['single']:.3f}, frozen / single frozen = {med['kalman frozen'] / med['single frozen']:.3f}"
        print(line, flush=True)
        for f in made: f.close()
