"""matrix convolver (llz_fir_matrix_mc: y_o = sum_i x_i * h[o][i], one delay line per input) against its emulation with the
stream convolver, the two forms alternated round by round in one process:
    python tools/time_fir_matrix.py [shapes=64x2,16x16,2x64,64x64] [blocks=128,512] [taps=8193,25248] [long=131073] [long_shapes=64x2,16x16]
  matrix:    FirMatrixMC(inputs, outputs, block, taps[O, I, T]), frame_len = block (k = 1)
  emulation: a FirStreamMC bank of inputs x outputs rows fed with every input replicated `outputs` times, then a torch sum over
             the input axis into [outputs, block].  The replication is done once, outside the timed calls.
Shapes are inputs x outputs; the `long` tap counts run for `long_shapes` only.  Every form is warmed, a probe window sizes its
calls per window so that a window lasts about WINDOW_MS, then it is timed in ROUNDS such windows between events; time per call:
median, min and max over the windows."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
def shape_list(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]
shapes = shape_list(opts.get("shapes", "64x2,16x16,2x64,64x64"))
long_shapes = shape_list(opts.get("long_shapes", "64x2,16x16"))
blocks = [int(v) for v in opts.get("blocks", "128,512").split(",")]
taps_list = [int(v) for v in opts.get("taps", "8193,25248").split(",") if v]
long_taps = [int(v) for v in opts.get("long", "131073").split(",") if v]
ROUNDS, WARM, PROBE, WINDOW_MS = 5, 3, 20, 100.0
L = capi.lib()
def window(fn, steps):
    t = L.llz_hip_timer_new(); L.llz_hip_timer_start(t, None)
    for _ in range(steps): fn()
    L.llz_hip_timer_stop(t, None); ms = L.llz_hip_timer_ms(t) / steps; L.llz_hip_timer_free(t)
    return ms
def alternated(forms):
    """forms: [(name, callable)]; every form warmed and probed for its calls per window, then ROUNDS rounds of one timed
    window per form: ({name: [ms per call]}, {name: calls per window})"""
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
      f"frame_len = block (k = 1)", flush=True)
for (I, O) in shapes:
    for T in taps_list + (long_taps if (I, O) in long_shapes else []):
        h = np.random.default_rng(T).standard_normal((O, I, T), dtype=np.float32)
        h /= np.float32(np.sqrt(I * T))
        for B in blocks:
            x = torch.empty(I, B, dtype=torch.float32, device=dev)
            filters.synth_f32(x, 1)
            xr = x.repeat(O, 1).contiguous()                                 # row o I + i = input i: the replication, not timed
            y = torch.empty(O, B, dtype=torch.float32, device=dev)
            yr = torch.empty(O * I, B, dtype=torch.float32, device=dev)
            ye = torch.empty(O, B, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter(); m = filters.FirMatrixMC(I, O, B, h); t1 = time.perf_counter()
            s = filters.FirStreamMC(O * I, B, h.reshape(O * I, T)); t2 = time.perf_counter()
            def emulation():
                s.filter(xr, yr)
                torch.sum(yr.view(O, I, B), dim=1, out=ye)
            mp = m.plan()
            ms, steps = alternated([("emulation", emulation), ("matrix", lambda: m.filter(x, y))])
            torch.cuda.synchronize()
            a, b = ms["matrix"], ms["emulation"]
            ma, mb = float(np.median(a)), float(np.median(b))
            read_mb = (I * mp[1] * B * 8 + O * I * mp[1] * B * 8) / 2 ** 20
            print(f"{I:3d} -> {O:3d} {T:6d} taps block {B:4d}: matrix P={mp[1]} G={mp[4]} ({read_mb:8.1f} MiB of distinct ring and H per call) "
                  f"{1e3 * ma:9.2f} us/call (min {1e3 * min(a):.2f} max {1e3 * max(a):.2f}, {steps['matrix']} calls/window) | emulation "
                  f"{O * I} rows {1e3 * mb:9.2f} us/call (min {1e3 * min(b):.2f} max {1e3 * max(b):.2f}, {steps['emulation']} "
                  f"calls/window) | matrix / emulation = {ma / mb:.3f} | {read_mb / 1024 / (ma * 1e-3):7.1f} GiB/s | "
                  f"init {1e3 * (t1 - t0):.0f} / {1e3 * (t2 - t1):.0f} ms", flush=True)
            m.close(); s.close()
