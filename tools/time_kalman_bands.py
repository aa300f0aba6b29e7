"""per-band Kalman filter (llz_kalman_bands_mc) per call next to the per-band NLMS filter (llz_adapt_bands_mc) at the same shapes,
the forms alternated round by round in one process:
    python tools/time_kalman_bands.py [channels ...] [bins=129] [taps=4,8,16,32] [frames=64]
  kalman:        every channel adapting
  kalman frozen: no channel adapting (y and e written, no update)
  nlms:          AdaptBandsMC, every channel at mu = 0.5
Default channels: 8 1024.  The method is tools/time_adapt_bands.py's: every form is warmed with WARM calls, a probe sizes its calls
per window so that a window lasts about WINDOW_MS, then it is timed in ROUNDS such windows between events; time per call: median,
min and max over the windows.  Counts per (channel, bin) and frame, K = taps: 48 bytes for all three (x, d in, e, y out, re and
im); per CALL the state in and out is 16 K - 8 bytes for NLMS and 24 K - 4 for the Kalman filter.  Arithmetic of an adapting
frame: NLMS 10 K fused multiply-adds and two quotients; Kalman 4 K for y, then per tap 3 for u and 1 sum for s, and in the update
3 for u again, 2 for the gain, 4 for w, 3 for c with its clamp, 2 for |w|^2, 3 for P: 25 K operations and one quotient."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
chans = [int(a) for a in sys.argv[1:] if "=" not in a] or [8, 1024]
bins = int(opts.get("bins", "129"))
taps_list = [int(v) for v in opts.get("taps", "4,8,16,32").split(",")]
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
print(f"{ROUNDS} windows of about {WINDOW_MS:.0f} ms per form after {WARM} warm-up calls and a probe of {PROBE}, forms alternated; "
      f"{frames} frames per call, {bins} bins", flush=True)
for ch in chans:
    bufs = [torch.empty(ch, frames, bins, dtype=torch.float32, device=dev) for _ in range(8)]
    for k, b in enumerate(bufs[:4]):
        filters.synth_f32(b.view(ch, frames * bins), k + 1)
    torch.cuda.synchronize()
    for K in taps_list:
        rng = np.random.default_rng(K)
        h = (rng.standard_normal((ch, K, bins)) + 1j * rng.standard_normal((ch, K, bins))) * np.exp(-np.arange(K) / (K / 4 + 1))[None, :, None]
        h /= np.sqrt(np.sum(np.abs(h) ** 2, axis=1, keepdims=True))
        k = filters.KalmanBandsMC(ch, bins, K)
        z = filters.KalmanBandsMC(ch, bins, K)
        n = filters.AdaptBandsMC(ch, bins, K, mu=0.5)
        z.set_adapt(0, np.zeros(ch))
        for f in (k, z, n): f.set_taps(0, h)
        ceiling, threads, groups, launches = k.plan()
        names = ("kalman", "kalman frozen", "nlms")
        ms, steps = alternated(list(zip(names, (lambda: k.process(*bufs), lambda: z.process(*bufs), lambda: n.process(*bufs)))))
        med = {name: float(np.median(v)) for name, v in ms.items()}
        line = f"{ch:5d} ch x {bins} bins, {K:2d} taps (ceiling {ceiling}, {groups} workgroups of {threads}):"
        for name in names:
            line += (f" {name} {1e3 * med[name]:9.2f} us/call (min {1e3 * min(ms[name]):.2f} max {1e3 * max(ms[name]):.2f}, "
                     f"{steps[name]} calls/window), {1e3 * med[name] / frames:.3f} us/frame |")
        line += f" kalman / nlms = {med['kalman'] / med['nlms']:.3f}, kalman / frozen = {med['kalman'] / med['kalman frozen']:.3f}"
        print(line, flush=True)
        k.close(); z.close(); n.close()
