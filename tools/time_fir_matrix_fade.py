"""matrix convolver (llz_fir_matrix_mc): a call while a fade between tap sets is in flight (llz_fir_xfade_matrix_mc, kernels of
fir_matrix_fade.hip) against the SAME handle's steady call (fir_matrix.hip), the two alternated round by round in one process:
    python tools/time_fir_matrix_fade.py column [shapes=64x2,16x16,2x64] [blocks=128,512,2048] [taps=8193,131073]
    python tools/time_fir_matrix_fade.py all    [shapes=...] [blocks=...] [taps=...]
  column: one input's paths fade (the last column, every output: a source that moves);  all: every path fades
Shapes are inputs x outputs.  frame_len = block (k = 1).  The method is tools/time_fir_stream_fade.py's: each form is warmed, a
probe window sizes its calls per window so that a window lasts about WINDOW_MS, then it is timed in ROUNDS such windows between
events; time per call: median, min and max over the windows.  A fade lasts 4096 blocks at the most, so a fading window holds at
most 4096 calls (the line says how long it was); a fresh fade of 4096 blocks is requested before every fading window, outside
the timed span, and the fade left over is dropped by a reset before the steady window, so that the steady calls run the three
untouched kernels."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
mode = sys.argv[1] if len(sys.argv) > 1 else "column"
assert mode in ("column", "all"), mode
opts = dict(a.split("=", 1) for a in sys.argv[2:] if "=" in a)
shapes = [tuple(int(v) for v in s.split("x")) for s in opts.get("shapes", "64x2,16x16,2x64").split(",") if s]
blocks = [int(v) for v in opts.get("blocks", "128,512,2048").split(",")]
taps_list = [int(v) for v in opts.get("taps", "8193,131073").split(",")]
ROUNDS, WARM, PROBE, WINDOW_MS, FADE = 5, 3, 20, 100.0, 4096
L = capi.lib()
def make_taps(O, I, T, seed):
    h = np.random.default_rng(seed).standard_normal((O, I, T), dtype=np.float32).astype(np.float64)
    return h / np.sqrt(np.sum(h * h, axis=(1, 2), keepdims=True))
def window(fn, steps):
    t = L.llz_hip_timer_new(); L.llz_hip_timer_start(t, None)
    for _ in range(steps): fn()
    L.llz_hip_timer_stop(t, None); ms = L.llz_hip_timer_ms(t) / steps; L.llz_hip_timer_free(t)
    return ms
print(f"{mode}: {ROUNDS} windows of about {WINDOW_MS:.0f} ms per form (a fading window: {FADE} calls at the most) after {WARM} "
      f"warm-up calls and a probe of {PROBE}, forms alternated; frame_len = block", flush=True)
for I, O in shapes:
    for T in taps_list:
        sets = [make_taps(O, I, T, T), make_taps(O, I, T, T + 7)]
        for B in blocks:
            x = torch.empty(I, B, dtype=torch.float32, device=dev)
            y = torch.empty(O, B, dtype=torch.float32, device=dev)
            filters.synth_f32(x, 1)
            s = filters.FirMatrixMC(I, O, B, sets[0])
            turn = [0]
            call = lambda: s.filter(x, y)
            def steady():
                if s.fade_left(): s.reset()                     # drops the fade: the untouched kernels from here on
                assert s.fade_left() == 0
            def fading():
                if s.fade_left(): s.reset()
                turn[0] ^= 1
                new = sets[turn[0]]
                if mode == "all": s.fade_taps(0, 0, new, FADE)
                else: s.fade_taps(0, I - 1, new[:, I - 1:], FADE)
                assert s.fade_left() == FADE
            steps = {}
            for name, prepare in (("steady", steady), ("fading", fading)):
                prepare()
                for _ in range(WARM): call()
                steps[name] = max(PROBE, int(np.ceil(WINDOW_MS / window(call, PROBE))))
            steps["fading"] = min(steps["fading"], FADE - WARM - PROBE)
            torch.cuda.synchronize()
            ms = {"steady": [], "fading": []}
            for _ in range(ROUNDS):
                for name, prepare in (("steady", steady), ("fading", fading)):
                    prepare()
                    torch.cuda.synchronize()
                    ms[name].append(window(call, steps[name]))
                    assert (s.fade_left() > 0) == (name == "fading")
            a, b = ms["fading"], ms["steady"]
            ma, mb = float(np.median(a)), float(np.median(b))
            plan = s.plan()
            print(f"{I:3d} -> {O:3d} {T:6d} taps block {B:4d} P={plan[1]} G={plan[4]}: fading {1e3 * ma:9.2f} us/call (min "
                  f"{1e3 * min(a):.2f} max {1e3 * max(a):.2f}, {steps['fading']} calls/window = {ma * steps['fading']:.0f} ms) | steady "
                  f"{1e3 * mb:9.2f} us/call (min {1e3 * min(b):.2f} max {1e3 * max(b):.2f}, {steps['steady']} calls/window) | fading / "
                  f"steady = {ma / mb:.3f}", flush=True)
            s.close()
