"""multi-reference adaptive filter (llz_adapt_matrix_mc) per call at k = 1 against existing code, four forms alternated round by
round in one process:
    python tools/time_adapt_matrix.py [inputs:outputs ...] [blocks=128,512,2048] [taps=8193,25248]
  adapting: AdaptMatrixMC, every output at mu = 0.5 (forward and power per call; product, error, update per block)
  bank:     AdaptMC(channels = outputs x inputs) (outputs for inputs = 1) at mu = 0.5: the same weight bytes and update work,
            but a ring per channel where the matrix form keeps one per input
  frozen:   AdaptMatrixMC, every output at mu = 0 (forward, product, error; y and e written)
  matrix:   FirMatrixMC with a tap set per path at the same shape
Default shapes: 1:64 2:64 8:2 8:64.  The method is tools/time_adapt.py's: every form is warmed with WARM calls, a probe sizes
its calls per window so that a window lasts about WINDOW_MS, then it is timed in ROUNDS such windows between events; time per
call: median, min and max over the windows.  Bytes by count per block, B = block, P = partitions, I inputs, O outputs: the
update moves O I P B 24 (X read, W read and written), the product reads O I P B 8 of W and, per output, I P B 8 of rings, the
power I P B 8."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
shapes = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:] if "=" not in a] or [(1, 64), (2, 64), (8, 2), (8, 64)]
blocks = [int(v) for v in opts.get("blocks", "128,512,2048").split(",")]
taps_list = [int(v) for v in opts.get("taps", "8193,25248").split(",")]
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
for I, O in shapes:
    for T in taps_list:
        h = np.random.default_rng(T).standard_normal((O, I, T), dtype=np.float32) * np.exp(-np.arange(T) / (T / 4 + 1)).astype(np.float32)
        h /= np.sqrt(np.sum(h.astype(np.float64) ** 2, axis=(1, 2), keepdims=True)).astype(np.float32)
        for B in blocks:
            ch = O * I
            x = torch.empty(I, B, dtype=torch.float32, device=dev)
            d = torch.empty(O, B, dtype=torch.float32, device=dev); e = torch.empty_like(d); y = torch.empty_like(d)
            xb = torch.empty(ch, B, dtype=torch.float32, device=dev)
            db = torch.empty_like(xb); eb = torch.empty_like(xb); yb = torch.empty_like(xb)
            for k, t in enumerate((x, d, xb, db)): filters.synth_f32(t, k + 1)
            torch.cuda.synchronize()
            m = filters.FirMatrixMC(I, O, B, h)
            a = filters.AdaptMatrixMC(I, O, B, T, mu=0.5)
            z = filters.AdaptMatrixMC(I, O, B, T, mu=0.0)
            bank = filters.AdaptMC(ch, B, T, mu=0.5)
            P, G = a.plan()[1], a.plan()[4]
            ms, steps = alternated([("matrix", lambda: m.filter(x, y)), ("frozen", lambda: z.process(x, d, e, y)),
                                    ("bank", lambda: bank.process(xb, db, eb, yb)), ("adapting", lambda: a.process(x, d, e, y))])
            med = {k: float(np.median(v)) for k, v in ms.items()}
            line = f"{I:4d} -> {O:4d} {T:6d} taps block {B:4d} P={P:4d} G={G:2d}:"
            for k in ("matrix", "frozen", "bank", "adapting"):
                line += f" {k} {1e3 * med[k]:9.2f} us/call (min {1e3 * min(ms[k]):.2f} max {1e3 * max(ms[k]):.2f}, {steps[k]} calls/window) |"
            line += (f" update {ch * P * B * 24 / 2 ** 20:.1f} MiB by count | frozen / matrix = {med['frozen'] / med['matrix']:.3f} | "
                     f"adapting / bank = {med['adapting'] / med['bank']:.3f}")
            print(line, flush=True)
            m.close(); a.close(); z.close(); bank.close()
