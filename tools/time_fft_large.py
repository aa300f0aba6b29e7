"""Timing of the FFT above 4096 points on one GPU.

Float32 batch (llz_fft_batch / llz_ifft_batch on a device buffer of at least 512 MiB): for N = 4096 (the register kernel,
for comparison) and 8192 .. 2^20, ms is the median of --steps calls timed with device events, TB/s counts 16 bytes per
point (one read and one write of a complex float, as DESIGN section 2 does), passes is the number of passes over device
memory the plan makes.  Single double transform (llz_fft / llz_ifft, host copies included): wall time at 2^16 and 2^20
beside the reference CPU library's llz_fft on the same host (oracle/_ref, when it was built).  Each configuration runs in
a fresh child process under a time limit.

    python tools/time_fft_large.py [--steps 20] [--mib 512] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = [1 << k for k in range(12, 21)]
SINGLE = [1 << 16, 1 << 20]


def passes(n):
    from llzlab_amd import capi
    if n <= 4096:
        return 1
    fn = capi.lib().llzs_fft_large_passes
    fn.argtypes, fn.restype = [C.c_int, C.c_int], C.c_int
    return fn(n, 1)


def child_batch(n, mib, steps, inverse):
    import torch
    from llzlab_amd import filters
    dev = torch.device("cuda:0")
    count = max(1, (mib << 20) // (8 * n))
    x = torch.rand(count * n * 2, dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    fb = filters.FftBatch(n)
    call = (lambda: fb.ifft(x, count)) if inverse else (lambda: fb.fft(x, count))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = sorted(times)[len(times) // 2]
    fb.close()
    return {"form": "batch_f32", "n": n, "count": count, "inverse": inverse, "ms": round(ms, 4),
            "TBs": round(count * n * 16 / ms / 1e9, 3), "passes": passes(n)}


def child_single(n, steps):
    import numpy as np
    from llzlab_amd import filters
    from oracle import pyoracle
    z = np.random.default_rng(n).standard_normal(n) + 1j * np.random.default_rng(n + 1).standard_normal(n)
    f = filters.Fft(n)
    f.fft(z)

    def med(fn):
        ts = []
        for _ in range(steps):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return round(sorted(ts)[len(ts) // 2], 3)
    row = {"form": "llz_fft", "n": n, "gpu_ms": med(lambda: f.fft(z)), "gpu_inv_ms": med(lambda: f.ifft(z))}
    f.close()
    if pyoracle.have_ref():
        ref = pyoracle.Ref()
        row["ref_cpu_ms"] = med(lambda: ref.fft(z))
        row["ref_cpu_inv_ms"] = med(lambda: ref.fft(z, inverse=True))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=512)
    ap.add_argument("--timeout", type=int, default=180)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=3)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, ROOT)
        form, n, inv = a.child[0], int(a.child[1]), int(a.child[2])
        row = child_batch(n, a.mib, a.steps, inv) if form == "batch" else child_single(n, max(3, a.steps // 4))
        print(json.dumps(row))
        return
    jobs = [("batch", n, inv) for n in BATCH for inv in (0, 1)] + [("single", n, 0) for n in SINGLE]
    rows = []
    for form, n, inv in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--mib", str(a.mib),
               "--child", form, str(n), str(inv)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if res.returncode != 0:
            print(f"{form} {n} inverse={inv}: exit {res.returncode}\n{res.stderr[-2000:]}", file=sys.stderr)
            sys.exit(1)                                 # nothing more on the GPU after a failure
        row = json.loads(res.stdout.strip().splitlines()[-1])
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
