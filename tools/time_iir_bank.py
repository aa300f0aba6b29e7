"""biquad bank (llz_iir_bank_mc) against the shared-coefficient handle (llz_iir_cascade_mc) of the same build, in one process,
the forms alternated round by round: python tools/time_iir_bank.py
  shapes        config 4 (1024 ch x 2^20 samples x 8 sections) and 4096 ch x 2^18
  coefficients  the config-4 set (8 x (0.44, 1.1): float32) and the 0.99-radius set (double)
  forms         the shared handle as it runs by default (the 32-sample wave form), a second shared handle BUILT under iir_unpacked = 2
                (the tune is read at init: its 16-sample wave form is the bank's counterpart) and the pipeline; a bank of equal rows
                and a bank of distinct rows, each on its default path (float32: the wave form; double: the pipeline) and on the
                pipeline (iir_pipe = 1)
  reported      ms, TB/s at 8 B per sample, ratio to the shared handle's default; each handle's plan; init time of the banks"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
ROUNDS, STEPS, WARM = 5, 10, 3
L = capi.lib()
def section(r, th):
    a1, a2 = -2 * r * np.cos(th), r * r
    g = (1 + a1 + a2) / 4
    return [g, 2 * g, g, 1.0, a1, a2]
def config4():
    return np.array([section(0.44, 1.1)] * 8)
def radius99():
    return np.array([section(0.99 - 0.004 * k, 0.25 + 0.31 * k) for k in range(8)])
def distinct(base, ch):
    """channel c: the base set with every pole angle moved by 1e-4 (c + 1) rad: no two channels equal, the same precision"""
    out = np.empty((ch,) + base.shape)
    for c in range(ch):
        for k, row in enumerate(base):
            r, th = np.sqrt(row[5]), np.arccos(-row[4] / (2 * np.sqrt(row[5])))
            out[c, k] = section(r, th + 1e-4 * (c + 1))
    return out
def window(fn):
    t = L.llz_hip_timer_new(); L.llz_hip_timer_start(t, None)
    for _ in range(STEPS): fn()
    L.llz_hip_timer_stop(t, None); ms = L.llz_hip_timer_ms(t) / STEPS; L.llz_hip_timer_free(t)
    return ms
def alternated(forms):
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
def report(ms, base, ch, n):
    b = float(np.median(ms[base]))
    for name, v in ms.items():
        m = float(np.median(v))
        print(f"  {name:38s} {m:7.3f} ms (min {min(v):.3f} max {max(v):.3f})  {8 * ch * n / m / 1e9:5.2f} TB/s  x{m / b:.3f} of {base}", flush=True)

print(f"{ROUNDS} rounds x {STEPS} calls per form after {WARM} warm-up calls, forms alternated", flush=True)
for ch, n in ((1024, 1 << 20), (4096, 1 << 18)):
    x = torch.empty(ch, n, dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    filters.synth_f32(x, 1)
    for cname, base in (("config-4 set, 8 x (0.44, 1.1)", config4()), ("0.99-radius set", radius99())):
        print(f"{ch} channels x {n} samples, {cname}", flush=True)
        shared = filters.IirCascadeMC(ch, base)
        with capi.tuned(iir_unpacked=2):
            shared16 = filters.IirCascadeMC(ch, base)
        t0 = time.perf_counter(); equal = filters.IirBankMC(ch, np.tile(base, (ch, 1, 1))); t1 = time.perf_counter()
        dist = filters.IirBankMC(ch, distinct(base, ch)); t2 = time.perf_counter()
        print(f"  init: bank of equal rows {t1 - t0:.2f} s, bank of distinct rows {t2 - t1:.2f} s (including {ch} sets built in numpy); "
              f"precision shared {shared.precision} equal {equal.precision} distinct {dist.precision}", flush=True)
        W16, PIPE = {"iir_unpacked": 2}, {"iir_pipe": 1}
        for name, h, tune in (("shared", shared, {}), ("shared wave16", shared16, W16), ("bank", dist, {}), ("bank pipeline", dist, PIPE)):
            with capi.tuned(**tune):
                print(f"  plan {name}: {h.plan(n)}", flush=True)
        forms = [("shared (default form)", lambda: shared.filter(x, y), {}),
                 ("shared, 16-sample wave form", lambda: shared16.filter(x, y), W16),
                 ("shared, pipeline", lambda: shared.filter(x, y), PIPE),
                 ("bank of equal rows, default path", lambda: equal.filter(x, y), {}),
                 ("bank of distinct rows, default path", lambda: dist.filter(x, y), {}),
                 ("bank of equal rows, pipeline", lambda: equal.filter(x, y), PIPE),
                 ("bank of distinct rows, pipeline", lambda: dist.filter(x, y), PIPE)]
        report(alternated(forms), "shared (default form)", ch, n)
        for h in (shared, shared16, equal, dist): h.close()
    del x, y
