"""partitioned bank (llz_fir_pbank_mc_init: LLZ_FIR_ALGO_PARTITIONED with a tap set per channel) against the shared-taps algo 7
and against the bank's time domain, the forms alternated round by round in one process:
    python tools/time_fir_bank_part.py shared [channels] [log2 n] [taps ...]    (default 64 20 4097 16385 65537 131073)
    python tools/time_fir_bank_part.py time   [channels] [log2 n] [taps ...]    (default 64 18 1025 4097 25248)
  shared: llz_fir_filter_mc algo 7 with row 0 and the bank with distinct rows: ms, ratio bank / shared, the plan, a spot check
          of the bank on a few channels against the shared form run on that channel alone with that channel's taps; then
          init time and set_taps time for one row and for all rows (host time, the device idle before, synchronised after)
  time:   the bank's LLZ_FIR_ALGO_TIME (k_fir_td_f32<true>) and the partitioned bank on the same distinct rows: the crossover"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
mode = sys.argv[1] if len(sys.argv) > 1 else "shared"
assert mode in ("shared", "time"), mode
args = [int(v) for v in sys.argv[2:]]
ch = args[0] if len(args) > 0 else 64
n = 1 << (args[1] if len(args) > 1 else (20 if mode == "shared" else 18))
taps_list = args[2:] or ([4097, 16385, 65537, 131073] if mode == "shared" else [1025, 4097, 25248])
ROUNDS, STEPS, WARM = 5, 10, 3
PART, TIME = filters.FIR_ALGO_PARTITIONED, filters.FIR_ALGO_TIME
x = torch.empty(ch, n, dtype=torch.float32, device=dev)
y = torch.empty_like(x)
filters.synth_f32(x, 1)
L = capi.lib()
def bank_taps(T):
    h = np.random.default_rng(T).standard_normal((ch, T), dtype=np.float32).astype(np.float64)
    return h / np.sqrt(np.sum(h * h, axis=1, keepdims=True))
def window(fn):
    t = L.llz_hip_timer_new(); L.llz_hip_timer_start(t, None)
    for _ in range(STEPS): fn()
    L.llz_hip_timer_stop(t, None); ms = L.llz_hip_timer_ms(t) / STEPS; L.llz_hip_timer_free(t)
    return ms
def alternated(forms):
    """forms: [(name, callable)]; every form warmed, then ROUNDS rounds of one timed window of STEPS calls per form"""
    ms = {name: [] for name, _ in forms}
    for name, fn in forms:
        for _ in range(WARM): fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in forms:
            ms[name].append(window(fn))
    return ms
def report(T, ms, base):
    b = float(np.median(ms[base]))
    for name, v in ms.items():
        m = float(np.median(v))
        print(f"  {T:6d} taps  {name:28s} {m:9.3f} ms (min {min(v):.3f} max {max(v):.3f})  {ch * n / m / 1e6:8.1f} GS/s  x{m / b:.3f} of {base}", flush=True)
def spot_check(bank_out, h, chans):
    """(the timed handle has streamed: its first flt_len-1 outputs see the previous call, the fresh handle's see zeros)"""
    T, worst = h.shape[1], 0.0
    if T > n:
        return float("nan")
    for c in chans:
        f = filters.FirFilterMC(1, n, h[c], algo=PART)
        y1 = torch.empty(1, n, dtype=torch.float32, device=dev)
        f.filter(x[c:c + 1].contiguous(), y1)
        worst = max(worst, (y1[0, T - 1:] - bank_out[c, T - 1:]).abs().max().item())
        f.close()
    return worst

print(f"{mode}: {ch} channels x {n} samples, {ROUNDS} rounds x {STEPS} calls per form after {WARM} warm-up calls, forms alternated", flush=True)
for T in taps_list:
    h = bank_taps(T)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); bank = filters.FirBankMC(ch, n, h, algo=PART); t1 = time.perf_counter()
    plan = bank.partition_plan(n)
    table_mb = ch * plan[1] * plan[0] * 8 / 2 ** 20
    if mode == "shared":
        other_name, other = "shared algo 7", filters.FirFilterMC(ch, n, h[0], algo=PART)
        assert other.partition_plan(n) == plan
    else:
        other_name, other = "bank time domain", filters.FirBankMC(ch, n, h, algo=TIME)
    print(f" {T} taps: N={plan[0]} P={plan[1]} {plan[2]} ch/pass x {plan[3]} passes, spectra table {table_mb:.1f} MiB, "
          f"init {1e3 * (t1 - t0):.0f} ms (tap conversion, {ch} x {plan[1]} spectra in double, uploads, sync)", flush=True)
    forms = [(other_name, lambda: other.filter(x, y)), ("partitioned bank", lambda: bank.filter(x, y))]
    report(T, alternated(forms), other_name)
    if mode == "shared":
        bank.filter(x, y)
        chans = sorted({0, 1, ch // 2, ch - 1})
        print(f"  {T:6d} taps  max |bank - shared form with that channel's taps| on channels {chans}, samples {T - 1}..: "
              f"{spot_check(y, h, chans):.3g}", flush=True)
        h32 = np.ascontiguousarray(h, dtype=np.float32)
        for count, reps in ((1, 5), (ch, 1)):
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); bank.set_taps(0, h32[:count]); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
            print(f"  {T:6d} taps  set_taps {count} row(s): median {1e3 * float(np.median(ts)):.3f} ms (min {1e3 * min(ts):.3f}, {reps} runs)", flush=True)
    other.close(); bank.close()
