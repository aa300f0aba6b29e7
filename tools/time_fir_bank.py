"""filter bank (llz_fir_bank_mc) on the headline shape, 4096 ch x 2^20 samples, against the shared-taps path (llz_fir_filter_mc)
in the same process, the forms alternated round by round: python tools/time_fir_bank.py [channels] [log2 n]
  1. 257 distinct tap sets, overlap-save: shared, bank (a spectrum image per half-wave in LDS), bank with the bank_global_h
     tune (every bin read from global memory per job); ms, TB/s at 8 B per sample, ratio to the shared form
  2. 9, 32, 33 and 63 taps, time domain and overlap-save, bank and shared: what the bank's AUTO crossover rests on
  3. init time for channels x 257 taps, set_taps time for 1 and for all channels"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
ch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
n = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 20)
ROUNDS, STEPS, WARM = 5, 10, 3
x = torch.empty(ch, n, dtype=torch.float32, device=dev)
y = torch.empty_like(x)
filters.synth_f32(x, 1)
L = capi.lib()
TIME, OLS = filters.FIR_ALGO_TIME, filters.FIR_ALGO_OVERLAP_SAVE
def bank_taps(T):
    h = np.random.default_rng(T).standard_normal((ch, T))
    return h / np.sqrt(np.sum(h * h, axis=1, keepdims=True))
def window(fn):
    t = L.llz_hip_timer_new(); L.llz_hip_timer_start(t, None)
    for _ in range(STEPS): fn()
    L.llz_hip_timer_stop(t, None); ms = L.llz_hip_timer_ms(t) / STEPS; L.llz_hip_timer_free(t)
    return ms
def alternated(forms):
    """forms: [(name, callable, tune)]; every form warmed, then ROUNDS rounds of one timed window of STEPS calls per form"""
    ms = {name: [] for name, _, _ in forms}
    for name, fn, tune in forms:
        with capi.tuned(**tune):
            for _ in range(WARM): fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn, tune in forms:
            with capi.tuned(**tune):
                ms[name].append(window(fn))
    return ms
def report(ms, base):
    b = float(np.median(ms[base]))
    for name, v in ms.items():
        m = float(np.median(v))
        print(f"  {name:34s} {m:7.3f} ms (min {min(v):.3f} max {max(v):.3f})  {8 * ch * n / m / 1e9:5.2f} TB/s  x{m / b:.3f} of {base}", flush=True)
def spot_check(bank_out, h, algo, chans):
    """the bank's output on a few channels against the shared form run on that channel alone with that channel's taps"""
    worst = 0.0
    for c in chans:
        f = filters.FirFilterMC(1, n, h[c], algo=algo)
        y1 = torch.empty(1, n, dtype=torch.float32, device=dev)
        f.filter(x[c:c + 1].contiguous(), y1)
        # (the timed handle has streamed: its first flt_len-1 outputs see the previous call, the fresh handle's see zeros)
        worst = max(worst, (y1[0, h.shape[1] - 1:] - bank_out[c, h.shape[1] - 1:]).abs().max().item())
        f.close()
    return worst

print(f"{ch} channels x {n} samples, {ROUNDS} rounds x {STEPS} calls per form after {WARM} warm-up calls, forms alternated", flush=True)
print("1. headline: 257 distinct tap sets, 1024-point overlap-save", flush=True)
h = bank_taps(257)
shared = filters.FirFilterMC(ch, n, h[0], algo=OLS)
bank = filters.FirBankMC(ch, n, h, algo=OLS)
forms = [("shared llz_fir_filter_mc", lambda: shared.filter(x, y), {}),
         ("bank, LDS half-spectrum images", lambda: bank.filter(x, y), {}),
         ("bank, bins from global memory", lambda: bank.filter(x, y), {"bank_global_h": 1})]
report(alternated(forms), "shared llz_fir_filter_mc")
chans = sorted({0, 1, 2, ch // 2, ch - 1})
for name, fn, tune in forms[1:]:
    with capi.tuned(**tune):
        fn()
    print(f"  {name}: max |bank - shared form with that channel's taps| on channels {chans}, samples {h.shape[1] - 1}..: {spot_check(y, h, OLS, chans):.3g}", flush=True)
shared.close(); bank.close()

print("2. the crossover: time domain and overlap-save at 9, 32, 33 and 63 taps", flush=True)
for T in (9, 32, 33, 63):
    h = bank_taps(T)
    hs = {a: filters.FirFilterMC(ch, n, h[0], algo=a) for a in (TIME, OLS)}
    hb = {a: filters.FirBankMC(ch, n, h, algo=a) for a in (TIME, OLS)}
    forms = [("shared time domain", lambda: hs[TIME].filter(x, y), {}), ("shared overlap-save", lambda: hs[OLS].filter(x, y), {}),
             ("bank time domain", lambda: hb[TIME].filter(x, y), {}), ("bank overlap-save", lambda: hb[OLS].filter(x, y), {})]
    print(f" {T} taps", flush=True)
    report(alternated(forms), "shared time domain")
    for f in list(hs.values()) + list(hb.values()): f.close()

print("3. init and set_taps, 257 taps, overlap-save (host time, the device idle before and synchronised after)", flush=True)
h = bank_taps(257)
torch.cuda.synchronize()
t0 = time.perf_counter(); bank = filters.FirBankMC(ch, n, h, algo=OLS); t1 = time.perf_counter()
print(f"  init {ch} x 257 taps: {1e3 * (t1 - t0):.1f} ms (FirBankMC(...): tap conversion, {ch} spectra in double, uploads, sync)", flush=True)
h32 = np.ascontiguousarray(h, dtype=np.float32)
for count in (1, ch):
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); bank.set_taps(0, h32[:count]); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    print(f"  set_taps {count} channel(s): median {1e3 * float(np.median(ts)):.3f} ms (min {1e3 * min(ts):.3f})", flush=True)
bank.close()
