"""arbitrary-ratio resampler (llz_asrc_mc) per call, next to the rational resampler at the same ratio, forms alternated round by
round in one process:
    python tools/time_asrc.py [channels] [n=1048576] [taps=32] [phases=512]
  asrc lds / asrc global at step 1.000023 (a drifting clock) and at step 147/160 (44.1 -> 48 kHz): the table in LDS, and read
      from global memory under the asrc_table_global override
  resample 160:147: llz_resample_mc, float32, on its own choice of kernel, n rounded down to a multiple of 147
Default: 1024 channels x 2^20 samples.  The method is tools/time_adapt.py's: every form is warmed with WARM calls, a probe sizes
its calls per window so that a window lasts about WINDOW_MS, then it is timed in ROUNDS such windows between events; time per
call: median, min and max over the windows.  GS/s counts OUTPUT sample-channels; "of roof" is that rate over the 1000 GS/s at
which 8 B per sample-channel (one float read, one written) would move at 8 TB/s.  Every call continues its handle's stream."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
ch = ([int(a) for a in sys.argv[1:] if "=" not in a] or [1024])[0]
n, T, phases = int(opts.get("n", 1 << 20)), int(opts.get("taps", 32)), int(opts.get("phases", 512))
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
      f"{ch} channels x {n} samples, {T} taps x {phases} phases", flush=True)
x = torch.empty(ch, n, dtype=torch.float32, device=dev)
filters.synth_f32(x, 1)
n_rs = n - n % 147
x_rs = x[:, :n_rs].contiguous()
out = torch.empty(ch, int(n / (147.0 / 160.0)) + 64, dtype=torch.float32, device=dev)
torch.cuda.synchronize()
forms, outputs = [], {}
for label, step in (("1.000023", 1.000023), ("147/160", 147.0 / 160.0)):
    for form, tune in (("lds", -1), ("global", 1)):
        L.llz_hip_tune(b"asrc_table_global", tune)
        f = filters.AsrcMC(ch, n, step=step, taps=T, phases=phases)
        name = f"asrc {form} step {label}"
        assert f.plan()[3] == (1 if tune == 1 or (phases + 1) * 4 * (4 * (((T + 3) // 4) | 1)) > 80 * 1024 else 0)
        outputs[name] = float(np.mean(f.out_len(n)))
        forms.append((name, (lambda f: lambda: f.process(x, out))(f)))
L.llz_hip_tune(b"asrc_table_global", -1)
rs = filters.ResampleMC(ch, 160, 147, win=filters.KAISER)
out_rs = out.view(-1)[:ch * rs.out_len(n_rs)].view(ch, -1)
outputs["resample 160:147"] = float(rs.out_len(n_rs))
forms.append(("resample 160:147", lambda: rs.process(x_rs, out_rs)))
ms, steps = alternated(forms)
for name, _ in forms:
    med = float(np.median(ms[name]))
    gs = ch * outputs[name] / (1e6 * med)
    extra = f" ({rs.last_entry()}, {rs.Q} taps per phase)" if name.startswith("resample") else ""
    print(f"{name:28s} {med:9.3f} ms/call (min {min(ms[name]):.3f} max {max(ms[name]):.3f}, {steps[name]} calls/window) "
          f"{gs:8.1f} GS/s = {gs / 1000.0:.3f} of roof{extra}", flush=True)
