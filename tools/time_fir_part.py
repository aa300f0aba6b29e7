"""partitioned overlap-save (LLZ_FIR_ALGO_PARTITIONED) on the headline batch, 4096 ch x 2^20 float32, beside the best the other
algos offer for the same taps: python tools/time_fir_part.py [channels] [log2 n] [taps ...]
  * algo 7 at every tap count given (default 4097 6145 8193 16385 25248 65537 131073), with its plan and init time;
  * OVERLAP_SAVE_8192 up to 6145 taps on the same batch;
  * AUTO (time domain) from 6146 to 25248 taps on TD_CH = 256 channels of the same length, scaled to the batch by
    channels / 256 and marked so: a 4096-channel call there takes seconds.
Every form is warmed, then timed in ROUNDS windows of STEPS calls between events; median, min and max are printed."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
args = [int(v) for v in sys.argv[1:]]
ch = args[0] if len(args) > 0 else 4096
n = 1 << (args[1] if len(args) > 1 else 20)
taps_list = args[2:] or [4097, 6145, 8193, 16385, 25248, 65537, 131073]
TD_CH = min(256, ch)
ROUNDS, STEPS, WARM = 5, 3, 2
x = torch.empty(ch, n, dtype=torch.float32, device=dev)
y = torch.empty_like(x)
filters.synth_f32(x, 1)
L = capi.lib()
def window(fn, steps):
    t = L.llz_hip_timer_new(); L.llz_hip_timer_start(t, None)
    for _ in range(steps): fn()
    L.llz_hip_timer_stop(t, None); ms = L.llz_hip_timer_ms(t) / steps; L.llz_hip_timer_free(t)
    return ms
def timed(fn, rounds=ROUNDS, steps=STEPS, warm=WARM):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    v = [window(fn, steps) for _ in range(rounds)]
    return float(np.median(v)), min(v), max(v)
print(f"{ch} channels x {n} samples; {WARM} warm-up calls, {ROUNDS} windows of {STEPS} calls", flush=True)
for T in taps_list:
    h = np.random.default_rng(T).standard_normal(T)
    h /= np.sqrt(np.sum(h * h))
    torch.cuda.synchronize()
    t0 = time.perf_counter(); f = filters.FirFilterMC(ch, n, h, algo=filters.FIR_ALGO_PARTITIONED); t1 = time.perf_counter()
    plan = f.partition_plan(n)
    m, lo, hi = timed(lambda: f.filter(x, y))
    print(f"{T:6d} taps  partitioned N={plan[0]} P={plan[1]} {plan[2]} ch/pass x {plan[3]} passes: {m:8.2f} ms (min {lo:.2f} max {hi:.2f})  "
          f"{ch * n / m / 1e6:7.1f} GS/s  init {1e3 * (t1 - t0):.0f} ms", flush=True)
    f.close()
    if T <= 6145:
        g = filters.FirFilterMC(ch, n, h, algo=filters.FIR_ALGO_OVERLAP_SAVE_8192)
        m2, lo, hi = timed(lambda: g.filter(x, y))
        print(f"{T:6d} taps  OVERLAP_SAVE_8192: {m2:8.2f} ms (min {lo:.2f} max {hi:.2f})  partitioned / this = {m / m2:.2f}", flush=True)
        g.close()
    elif T <= 25248:
        g = filters.FirFilterMC(TD_CH, n, h, algo=filters.FIR_ALGO_AUTO)
        xs, ys = x[:TD_CH], y[:TD_CH]
        m2, lo, hi = timed(lambda: g.filter(xs, ys), rounds=2, steps=1, warm=1)
        print(f"{T:6d} taps  AUTO (algo {g.algo}) on {TD_CH} channels: {m2:8.2f} ms (min {lo:.2f} max {hi:.2f}); SCALED to {ch} channels: "
              f"{m2 * ch / TD_CH:9.1f} ms  partitioned / this = {m / (m2 * ch / TD_CH):.4f}", flush=True)
        g.close()
