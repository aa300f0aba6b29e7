"""adaptive filter (llz_adapt_mc) per call at k = 1, three forms alternated round by round in one process:
    python tools/time_adapt.py [channels ...] [blocks=128,512,2048] [taps=8193,25248] [ppw=1,2,4,8]
  adapting: every channel at mu = 0.5 (two launches per block: filter, update)
  frozen:   every channel at mu = 0 (the filter launch alone; y and e written)
  stream:   llz_fir_stream_mc with a tap row per channel at the same shape
With ppw=... the adapting form is timed instead under the adapt_ppw override, once per value (partitions per workgroup of the
weight update), the values alternated like the forms.  Default channels: 64 1024.  The method is tools/time_fir_stream.py's:
every form is warmed with WARM calls, a probe sizes its calls per window so that a window lasts about WINDOW_MS, then it is timed
in ROUNDS such windows between events; time per call: median, min and max over the windows.  Bytes by count per channel and block, B = block, P = partitions: the stream call reads
P B 16 (ring and spectra) and moves 2 B 4 of samples; the frozen call one more input row and one more output row (4 B 4); the
adapting call walks the ring twice and reads W in the filter, reads and writes W in the update: P B 40."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
chans = [int(a) for a in sys.argv[1:] if "=" not in a] or [64, 1024]
blocks = [int(v) for v in opts.get("blocks", "128,512,2048").split(",")]
taps_list = [int(v) for v in opts.get("taps", "8193,25248").split(",")]
ppws = [int(v) for v in opts["ppw"].split(",")] if "ppw" in opts else []
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
      f"frame_len = block", flush=True)
for ch in chans:
    for T in taps_list:
        h = np.random.default_rng(T).standard_normal((ch, T), dtype=np.float32) * np.exp(-np.arange(T) / (T / 4 + 1)).astype(np.float32)
        h /= np.sqrt(np.sum(h.astype(np.float64) ** 2, axis=1, keepdims=True)).astype(np.float32)
        for B in blocks:
            x = torch.empty(ch, B, dtype=torch.float32, device=dev)
            d = torch.empty_like(x); e = torch.empty_like(x); y = torch.empty_like(x)
            filters.synth_f32(x, 1); filters.synth_f32(d, 2)
            torch.cuda.synchronize()
            s = filters.FirStreamMC(ch, B, h)
            a = filters.AdaptMC(ch, B, T, mu=0.5)
            z = filters.AdaptMC(ch, B, T, mu=0.0)
            a.set_taps(0, h); z.set_taps(0, h)
            P = a.plan()[1]
            if ppws:
                def tuned(v):
                    return lambda: (L.llz_hip_tune(b"adapt_ppw", v), a.process(x, d, e, y))
                ms, steps = alternated([(f"ppw {v}", tuned(v)) for v in ppws])
                L.llz_hip_tune(b"adapt_ppw", -1)
                print(f"{ch:5d} ch {T:6d} taps block {B:4d} P={P:4d}: adapting us/call by partitions per update workgroup: " +
                      " | ".join(f"{v}: {1e3 * float(np.median(ms[f'ppw {v}'])):.2f} (min {1e3 * min(ms[f'ppw {v}']):.2f} max "
                                 f"{1e3 * max(ms[f'ppw {v}']):.2f})" for v in ppws), flush=True)
                s.close(); a.close(); z.close()
                continue
            ms, steps = alternated([("stream", lambda: s.filter(x, y)), ("frozen", lambda: z.process(x, d, e, y)),
                                    ("adapting", lambda: a.process(x, d, e, y))])
            med = {k: float(np.median(v)) for k, v in ms.items()}
            mb = {"stream": P * B * 16 + 8 * B, "frozen": P * B * 16 + 16 * B, "adapting": P * B * 40 + 16 * B}
            line = f"{ch:5d} ch {T:6d} taps block {B:4d} P={P:4d}:"
            for k in ("stream", "frozen", "adapting"):
                gbs = ch * mb[k] / (1e6 * med[k])
                line += (f" {k} {1e3 * med[k]:9.2f} us/call (min {1e3 * min(ms[k]):.2f} max {1e3 * max(ms[k]):.2f}, {steps[k]} calls/window, "
                         f"{ch * mb[k] / 2 ** 20:.1f} MiB by count, {gbs:.0f} GB/s) |")
            line += f" frozen / stream = {med['frozen'] / med['stream']:.3f} | adapting / frozen = {med['adapting'] / med['frozen']:.3f}"
            print(line, flush=True)
            s.close(); a.close(); z.close()
