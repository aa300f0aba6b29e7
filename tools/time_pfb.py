"""polyphase DFT filter bank (llz_pfb_mc) per call, next to llz_stft_mc at the same transform length and hop, forms alternated
round by round in one process:
    python tools/time_pfb.py [channels] [bands=1024] [frames=256]
  pfb analysis / synthesis at taps_per_band P in {1, 4, 8} and bands / hop in {1, 4}; the analysis in both forms where both are
      legal (the span of a workgroup's frames in LDS, and the samples read through the caches under the pfb_global override)
  stft analysis / synthesis: llz_stft_mc at fft_len = bands and the same hop (bands / hop = 4 only; it has no hop of fft_len)
Default: 1024 channels x 1024 bands x 256 frames.  The method is tools/time_asrc.py's: every form is warmed with WARM calls, a probe
sizes its calls per window so that a window lasts about WINDOW_MS, then it is timed in ROUNDS such windows between events; time per
call: median, min and max over the windows.  TB/s counts the algorithmic bytes, 4 D + 8 (M / 2 + 1) per frame and channel.  Every
call continues its handle's stream."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
ch = ([int(a) for a in sys.argv[1:] if "=" not in a] or [1024])[0]
M, frames = int(opts.get("bands", 1024)), int(opts.get("frames", 256))
ROUNDS, WARM, PROBE, WINDOW_MS = 5, 2, 3, 100.0
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
      f"{ch} channels x {M} bands x {frames} frames", flush=True)
bins = M // 2 + 1
re = torch.empty(ch, frames, bins, dtype=torch.float32, device=dev)
im = torch.empty(ch, frames, bins, dtype=torch.float32, device=dev)
filters.synth_f32(re.view(ch, -1), 2)
filters.synth_f32(im.view(ch, -1), 3)
im[:, :, 0] = 0
im[:, :, -1] = 0
forms, bytes_of, keep = [], {}, []
for os_ in (1, 4):
    D = M // os_
    x = torch.empty(ch, frames * D, dtype=torch.float32, device=dev)
    filters.synth_f32(x, 1)
    y = torch.empty_like(x)
    moved = ch * frames * (4 * D + 8 * bins)
    for P in (1, 4, 8):
        w = filters.pfb_prototype(M, P) if P > 1 else np.hanning(M + 1)[:M].astype(np.float32)
        for form, tune in (("lds", -1), ("global", 1)):
            L.llz_hip_tune(b"pfb_global", tune)
            f = filters.PfbMC(ch, M, D, P, w, None, filters.PFB_PHASE_TIME)
            took = f.plan(frames)[0]
            if took[0] != (1 if tune == 1 else 0):
                f.close()                                       # (the span does not fit LDS: only the global form is legal)
                continue
            name = f"pfb analysis P={P} M/D={os_} {form} ({took[1]} frames/wg)"
            def call(f=f, x=x, tune=tune):
                L.llz_hip_tune(b"pfb_global", tune)
                f.analysis(x, re, im)
            forms.append((name, call)); bytes_of[name] = moved; keep.append(f)
        L.llz_hip_tune(b"pfb_global", -1)
        f = filters.PfbMC(ch, M, D, P, w, None, filters.PFB_PHASE_TIME)
        name = f"pfb synthesis P={P} M/D={os_} ({f.plan(frames)[1][1]} frames/wg)"
        forms.append((name, (lambda f, y: lambda: f.synthesis(re, im, y))(f, y))); bytes_of[name] = moved; keep.append(f)
    if os_ == 4:
        s = filters.StftMC(ch, capi.OVERLAP_HIGH, D, capi.HAMMING)
        def stft_a(s=s, x=x):
            L.llz_hip_tune(b"pfb_global", -1)
            s.analysis(x, re, im)
        forms.append((f"stft analysis fft_len={M} hop={D}", stft_a))
        forms.append((f"stft synthesis fft_len={M} hop={D}", (lambda s, y: lambda: s.synthesis(re, im, y))(s, y)))
        bytes_of[forms[-2][0]] = bytes_of[forms[-1][0]] = moved; keep.append(s)
ms, steps = alternated(forms)
L.llz_hip_tune(b"pfb_global", -1)
for name, _ in forms:
    med = float(np.median(ms[name]))
    print(f"{name:48s} {med:9.3f} ms/call (min {min(ms[name]):.3f} max {max(ms[name]):.3f}, {steps[name]} calls/window) "
          f"{bytes_of[name] / (1e9 * med):7.3f} TB/s", flush=True)
