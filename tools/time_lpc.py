"""Timing of batch LPC on one GPU: 2^18 frames x 1024 samples (float32, device buffers), for p in {10, 16, 32} llz_autocorr_mc
alone, the fused llz_lpc_mc and its split path (llz_hip_tune("lpc_split", 1)); for p in {48, 64} the split path (the only
one).  Each configuration runs in a fresh child process under a time limit; ms is the median of --steps timed calls, GB/s
counts the input read once.

    python tools/time_lpc.py [--frames 262144] [--n 1024] [--steps 20] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(p, form) for p in (10, 16, 32) for form in ("autocorr_mc", "lpc_fused", "lpc_split")] + \
          [(p, "lpc_split") for p in (48, 64)]


def child(frames, n, p, form, steps):
    sys.path.insert(0, ROOT)
    import torch
    from llzlab_amd import capi, filters
    dev = torch.device("cuda:0")
    x = torch.randn(frames, n, dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    acof = torch.empty(frames, p + 1, dtype=torch.float32, device=dev)
    kcof = torch.empty(frames, p, dtype=torch.float32, device=dev)
    err = torch.empty(frames, dtype=torch.float32, device=dev)
    gain = torch.empty_like(err)
    r = torch.empty(frames, p + 1, dtype=torch.float32, device=dev)
    if form == "lpc_split":
        capi.tune("lpc_split", 1)
    call = (lambda: filters.autocorr_mc(x, r, p)) if form == "autocorr_mc" else \
        (lambda: filters.lpc_mc(x, acof, kcof, err, gain, p=p))
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
    print(json.dumps({"p": p, "form": form, "frames": frames, "n": n, "ms": round(ms, 4),
                      "GBs": round(frames * n * 4 / ms / 1e6, 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 18)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        child(a.frames, a.n, int(a.child[0]), a.child[1], a.steps)
        return
    rows = []
    for p, form in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--frames", str(a.frames), "--n", str(a.n), "--steps", str(a.steps),
               "--child", str(p), form]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if res.returncode != 0:
            print(f"p={p} {form}: exit {res.returncode}\n{res.stderr[-2000:]}", file=sys.stderr)
            break                                       # nothing more on the GPU after a failure
        row = json.loads(res.stdout.strip().splitlines()[-1])
        rows.append(row)
        print(f"p={p:3d} {form:12s} {row['ms']:8.3f} ms {row['GBs']:8.1f} GB/s", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
