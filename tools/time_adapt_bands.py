"""per-band adaptive filter (llz_adapt_bands_mc) per call, two forms alternated round by round in one process:
    python tools/time_adapt_bands.py [channels ...] [bins=129] [taps=4,8,16,32,64] [frames=64]
  adapting: every channel at mu = 0.5
  frozen:   every channel at mu = 0 (y and e written, no power, no update)
Default channels: 8 1024.  The method is tools/time_adapt.py's: every form is warmed with WARM calls, a probe sizes its calls per
window so that a window lasts about WINDOW_MS, then it is timed in ROUNDS such windows between events; time per call: median, min
and max over the windows.  Counts per (channel, bin) and frame, K = taps: 48 bytes (x, d in, e, y out, re and im), plus 16 K - 8
per CALL for the state in and out; fused multiply-adds: 4 K for y, 2 K for the power, 4 K for the update (adapting 10 K, frozen
4 K; the kernel sums the power in the filter's walk either way).  One launch per call, a lane per (channel, bin): channels x bins
/ 64 waves, each a recursion over the call's frames."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
chans = [int(a) for a in sys.argv[1:] if "=" not in a] or [8, 1024]
bins = int(opts.get("bins", "129"))
taps_list = [int(v) for v in opts.get("taps", "4,8,16,32,64").split(",")]
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
        a = filters.AdaptBandsMC(ch, bins, K, mu=0.5)
        z = filters.AdaptBandsMC(ch, bins, K, mu=0.0)
        a.set_taps(0, h); z.set_taps(0, h)
        ceiling, threads, groups, launches = a.plan()
        ms, steps = alternated([("frozen", lambda: z.process(*bufs)), ("adapting", lambda: a.process(*bufs))])
        med = {k: float(np.median(v)) for k, v in ms.items()}
        lanes = ch * bins
        nbytes = lanes * (48 * frames + 16 * K - 8)
        fma = {"frozen": 4 * K, "adapting": 10 * K}
        line = f"{ch:5d} ch x {bins} bins, {K:2d} taps (ceiling {ceiling}, {groups} workgroups of {threads}):"
        for k in ("frozen", "adapting"):
            line += (f" {k} {1e3 * med[k]:9.2f} us/call (min {1e3 * min(ms[k]):.2f} max {1e3 * max(ms[k]):.2f}, {steps[k]} calls/window), "
                     f"{1e3 * med[k] / frames:.3f} us/frame, {nbytes / (1e6 * med[k]):.1f} GB/s, "
                     f"{lanes * frames * fma[k] / (1e6 * med[k]):.1f} GFMA/s |")
        line += f" adapting / frozen = {med['adapting'] / med['frozen']:.3f}"
        print(line, flush=True)
        a.close(); z.close()
