"""per-band postfilter (llz_suppress_bands_mc) per call in its four forms next to the per-band Kalman filter (llz_kalman_bands_mc)
at 4 taps with y on the same shape, the forms alternated round by round in one process:
    python tools/time_suppress_bands.py [channels ...] [bins=129] [frames=64] [window=128]
  y+g, y, g, plain: the postfilter with and without the echo estimate read and the gain stored, every channel enabled, eta = 0.01,
                    running form (the handle is walked past its start-up before it is timed)
  kalman:           KalmanBandsMC, 4 taps, every channel adapting, y stored
Default channels: 8 1024.  The method is tools/time_kalman_bands.py's: every form is warmed with WARM calls, a probe sizes its calls
per window so that a window lasts about WINDOW_MS, then it is timed in ROUNDS such windows between events; time per call: median,
min and max over the windows.  Bytes per (channel, bin) and frame: plain 16 (e in, o out, re and im), +8 with y, +4 with g; the
Kalman filter 48 (x, d in, e, y out).  Per CALL the state in and out is 56 bytes for the postfilter, 92 for the Kalman filter at 4
taps.  Arithmetic of a running frame: about 40 operations with 3 correctly rounded reciprocals (S, the two minima, J, q, N, R, Q,
the two ratios, G with its clamps, o, Z) against the Kalman filter's 25 K = 100 with one."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
chans = [int(a) for a in sys.argv[1:] if "=" not in a] or [8, 1024]
bins = int(opts.get("bins", "129"))
frames = int(opts.get("frames", "64"))
W = int(opts.get("window", "128"))
TAPS = 4
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
        for _ in range(max(WARM, -(-W // frames) + 1)): fn()
        steps[name] = max(PROBE, int(np.ceil(WINDOW_MS / window(fn, PROBE))))
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in forms:
            ms[name].append(window(fn, steps[name]))
    return ms, steps
print(f"{ROUNDS} windows of about {WINDOW_MS:.0f} ms per form after the start-up and a probe of {PROBE}, forms alternated; "
      f"{frames} frames per call, {bins} bins, W = {W}", flush=True)
for ch in chans:
    bufs = [torch.empty(ch, frames, bins, dtype=torch.float32, device=dev) for _ in range(8)]
    for k, b in enumerate(bufs[:4]):
        filters.synth_f32(b.view(ch, frames * bins), k + 1)
    torch.cuda.synchronize()
    er, ei, yr, yi, orr, oi, g, spare = bufs
    s = {name: filters.SuppressBandsMC(ch, bins, window=W) for name in ("y+g", "y", "g", "plain")}
    for f in s.values(): f.set_leak(0, np.full(ch, 0.01, np.float32))
    k = filters.KalmanBandsMC(ch, bins, TAPS)
    forms = [("y+g", lambda: s["y+g"].process(er, ei, orr, oi, yr, yi, g)), ("y", lambda: s["y"].process(er, ei, orr, oi, yr, yi)),
             ("g", lambda: s["g"].process(er, ei, orr, oi, g=g)), ("plain", lambda: s["plain"].process(er, ei, orr, oi)),
             ("kalman", lambda: k.process(er, ei, yr, yi, orr, oi, g, spare))]
    ms, steps = alternated(forms)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    _, threads, groups, _ = s["plain"].plan()
    line = f"{ch:5d} ch x {bins} bins ({groups} workgroups of {threads}):"
    for name, _ in forms:
        line += (f" {name} {1e3 * med[name]:9.2f} us/call (min {1e3 * min(ms[name]):.2f} max {1e3 * max(ms[name]):.2f}, "
                 f"{steps[name]} calls/window), {1e3 * med[name] / frames:.3f} us/frame |")
    line += f" y+g / kalman = {med['y+g'] / med['kalman']:.3f}, plain / kalman = {med['plain'] / med['kalman']:.3f}"
    print(line, flush=True)
    for f in list(s.values()) + [k]: f.close()
