"""multi-reference per-band adaptive filter (llz_adapt_bands_matrix_mc) per call against its single-reference sibling with the
same regressor length, two forms alternated round by round in one process:
    python tools/time_adapt_bands_matrix.py [shapes=2x8x16,8x8x8,2x64x4] [bins=129,1025] [frames=64] [out=FILE]
  matrix:  AdaptBandsMatrixMC(I, O, bins, K), every output at mu = 0.5
  single:  AdaptBandsMC(O channels, bins, taps = I K), every channel at mu = 0.5
A shape is I x O x K.  The method is tools/time_adapt_bands.py's: every form is warmed with WARM calls, a probe sizes its calls per
window so that a window lasts about WINDOW_MS, then it is timed in ROUNDS such windows between events, the forms in turn; time per
call: median, min and max over the windows.  Both forms walk I K regressor entries per (output, bin) and frame with 10 I K fused
multiply-adds; the matrix form loads 2 I + 2 values per frame where the single one loads 4, that is 2 (I - 1) more, and stores the
same 4.  Counts per (output, bin) and frame: bytes 8 I (x, shared by the outputs: counted once per bin, 8 I / O per output) + 8
(d) + 16 (e, y).  One launch per call either way.  out=FILE appends the lines to FILE as well."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from llzlab_amd import capi, filters
dev = torch.device("cuda:0")
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
shapes = [tuple(int(v) for v in s.split("x")) for s in opts.get("shapes", "2x8x16,8x8x8,2x64x4").split(",")]
bins_list = [int(v) for v in opts.get("bins", "129,1025").split(",")]
frames = int(opts.get("frames", "64"))
out = open(opts["out"], "a") if "out" in opts else None
ROUNDS, WARM, PROBE, WINDOW_MS = 5, 3, 20, 100.0
L = capi.lib()
def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n"); out.flush()
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
say(f"{ROUNDS} windows of about {WINDOW_MS:.0f} ms per form after {WARM} warm-up calls and a probe of {PROBE}, forms alternated; "
    f"{frames} frames per call")
for bins in bins_list:
    for I, O, K in shapes:
        new = lambda rows: [torch.empty(rows, frames, bins, dtype=torch.float32, device=dev) for _ in range(2)]  # noqa: E731
        x, xs, d, e, y = new(I), new(O), new(O), new(O), new(O)
        for k, b in enumerate(x + xs + d):
            filters.synth_f32(b.view(b.shape[0], frames * bins), k + 1)
        torch.cuda.synchronize()
        m = filters.AdaptBandsMatrixMC(I, O, bins, K, mu=0.5)
        s = filters.AdaptBandsMC(O, bins, I * K, mu=0.5)
        inputs, ceiling, threads, groups, launches = m.plan()
        ms, steps = alternated([("single", lambda: s.process(*xs, *d, *e, *y)), ("matrix", lambda: m.process(x, d, e, y))])
        med = {k: float(np.median(v)) for k, v in ms.items()}
        lanes = O * bins
        line = (f"I={I} O={O} K={K} ({I * K} entries, instance <{inputs}, {ceiling}>, {groups} workgroups of {threads}, single ceiling "
                f"{s.plan()[0]}), {bins} bins:")
        for k in ("single", "matrix"):
            line += (f" {k} {1e3 * med[k]:9.2f} us/call (min {1e3 * min(ms[k]):.2f} max {1e3 * max(ms[k]):.2f}, {steps[k]} calls/window), "
                     f"{1e3 * med[k] / frames:.3f} us/frame, {lanes * frames * 10 * I * K / (1e6 * med[k]):.1f} GFMA/s |")
        line += f" matrix / single = {med['matrix'] / med['single']:.3f}"
        say(line)
        m.close(); s.close()
