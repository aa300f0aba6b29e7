"""stream convolver (llz_fir_stream_mc: spectra kept between calls) against the partitioned overlap-save AT THE SAME frame_len,
the forms alternated round by round in one process:
    python tools/time_fir_stream.py shared [channels ...] [blocks=128,512,2048] [taps=8193,25248,131073]
    python tools/time_fir_stream.py rows   [channels ...] [blocks=...] [taps=...]
  shared: one tap set for all channels: FirStreamMC(1-D taps) against llz_fir_filter_mc with LLZ_FIR_ALGO_PARTITIONED
  rows:   a tap set per channel: FirStreamMC([channels, T]) against the partitioned bank (llz_fir_pbank_mc_init)
Default channels: 64 1024.  frame_len = block for both forms (k = 1).  Every form is warmed, a probe window sizes its calls per
window so that a window lasts about WINDOW_MS (a shorter one measures the clock and the scheduler as much as the kernel), then
it is timed in ROUNDS such windows between events; time per call: median, min and max over the windows.  The partitioned forms
are the yardstick:
they redo the whole history in every call, so their time hardly moves with the block."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
mode = sys.argv[1] if len(sys.argv) > 1 else "shared"
assert mode in ("shared", "rows"), mode
opts = dict(a.split("=", 1) for a in sys.argv[2:] if "=" in a)
chans = [int(a) for a in sys.argv[2:] if "=" not in a] or [64, 1024]
blocks = [int(v) for v in opts.get("blocks", "128,512,2048").split(",")]
taps_list = [int(v) for v in opts.get("taps", "8193,25248,131073").split(",")]
ROUNDS, WARM, PROBE, WINDOW_MS = 5, 3, 20, 100.0
PART = filters.FIR_ALGO_PARTITIONED
L = capi.lib()
def make_taps(ch, T):
    shape = (ch, T) if mode == "rows" else (T,)
    h = np.random.default_rng(T).standard_normal(shape, dtype=np.float32).astype(np.float64)
    return h / np.sqrt(np.sum(h * h, axis=-1, keepdims=True))
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
print(f"{mode}: {ROUNDS} windows of about {WINDOW_MS:.0f} ms per form after {WARM} warm-up calls and a probe of {PROBE}, forms "
      f"alternated; frame_len = block", flush=True)
for ch in chans:
    for T in taps_list:
        h = make_taps(ch, T)
        for B in blocks:
            x = torch.empty(ch, B, dtype=torch.float32, device=dev)
            y = torch.empty_like(x)
            filters.synth_f32(x, 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter(); s = filters.FirStreamMC(ch, B, h); t1 = time.perf_counter()
            part = filters.FirBankMC(ch, B, h, algo=PART) if mode == "rows" else filters.FirFilterMC(ch, B, h, algo=PART)
            t2 = time.perf_counter()
            sp, pp = s.plan(), part.partition_plan(B)
            ms, steps = alternated([("partitioned", lambda: part.filter(x, y)), ("stream", lambda: s.filter(x, y))])
            a, b = ms["stream"], ms["partitioned"]
            ma, mb = float(np.median(a)), float(np.median(b))
            ring_mb = sp[1] * B * 8 / 2 ** 20
            print(f"{ch:5d} ch {T:6d} taps block {B:4d}: stream P={sp[1]} R={sp[2]} ({ring_mb:.2f} MiB of ring read per channel) "
                  f"{1e3 * ma:9.2f} us/call (min {1e3 * min(a):.2f} max {1e3 * max(a):.2f}, {steps['stream']} calls/window) | partitioned N={pp[0]} P={pp[1]} "
                  f"{pp[2]} ch/pass x {pp[3]}: {1e3 * mb:9.1f} us/call (min {1e3 * min(b):.1f} max {1e3 * max(b):.1f}, "
                  f"{steps['partitioned']} calls/window) | "
                  f"stream / partitioned = {ma / mb:.3f} | init {1e3 * (t1 - t0):.0f} / {1e3 * (t2 - t1):.0f} ms", flush=True)
            s.close(); part.close()
