#!/usr/bin/env python3
"""Event-timed DFT of any length on one GPU: filters.DftMC.forward and .rforward (kernels/dft.hip) at N = 480, 960, 1000, 2048 and
4800, at counts whose rows move at least 256 MB (16 N bytes a complex row in and out, 4 N + 8 (N / 2 + 1) a real one), in both
forms where both exist (the fused kernel, and the composed form forced by llz_dft_mc_configure), and
next to each filters.FftBatch.fft at the same M and count -- the library's own M-point transform in place, the yardstick: a fused
call is two of them and the product with the chirp's spectrum per row.  All handles of a size run in the same process,
alternating, median of the repeats.

    ms      the whole call between two events on the stream
    x fft   the call's time over llz_fft_batch's at M points and the same count
    of HBM  the algorithmic bytes over the time, as a share of 8 TB/s

    python tools/time_dft.py [--quick] [--out FILE]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from llzlab_amd import capi, filters  # noqa: E402

quick = "--quick" in sys.argv[1:]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
capi.check(capi.lib().llz_hip_set_device(0), "set_device")
stream = torch.cuda.current_stream()
lines = []
MOVE = 256e6
HBM = 8e12


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def size(N, repeats):
    forms = {"fused" if N <= 2048 else "composed": filters.DftMC(N, stream=stream)}
    if N <= 2048:
        forms["composed"] = filters.DftMC(N, stream=stream)
        forms["composed"].configure(composed=True)
    for op, row_bytes in (("forward", 16 * N), ("rforward", 4 * N + 8 * (N // 2 + 1))):
        count = int(-(-MOVE // row_bytes))
        real = op == "rforward"
        x = torch.randn(count, N if real else 2 * N, dtype=torch.float32, device=dev)
        out = torch.empty(count, 2 * (N // 2 + 1 if real else N), dtype=torch.float32, device=dev)
        plans = {name: h.plan(count) for name, h in forms.items()}
        M = next(iter(plans.values()))["m"]
        fft = filters.FftBatch(M, stream=stream)
        z = torch.randn(count, 2 * M, dtype=torch.float32, device=dev)
        calls = {name: (lambda h=h: getattr(h, op)(x, out=out)) for name, h in forms.items()}
        calls["fft"] = lambda: fft.fft(z, count)
        for fn in calls.values():
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(repeats):                                        # alternating
            for name, fn in calls.items():
                times[name].append(timed(fn))
        base = statistics.median(times["fft"])
        say(f"dft N={N} {op} count={count} M={M}: llz_fft_batch at M median {base:8.3f} ms (min {min(times['fft']):.3f} max "
            f"{max(times['fft']):.3f}, {repeats} repeats)")
        for name in forms:
            m = statistics.median(times[name])
            p = plans[name]
            say(f"    {name:8s} median {m:8.3f} ms (min {min(times[name]):.3f} max {max(times[name]):.3f}) = {m / base:5.2f} x fft, "
                f"{100 * count * row_bytes / (m * 1e-3) / HBM:5.1f} % of HBM peak by algorithmic bytes; plan tpw {p['tpw']} lds "
                f"{p['lds']} slabs {p['slabs']}")
        fft.close()
        del x, out, z
    for h in forms.values():
        h.close()


for N in (480, 960, 1000, 2048, 4800):
    size(N, 5 if quick else 9)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
