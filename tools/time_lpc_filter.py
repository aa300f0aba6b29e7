"""Timing of the LPC filters on one GPU: llz_lpc_residual_mc and llz_lpc_synth_mc over 2^28 samples (float32, device buffers)
for p in {10, 16, 32, 64}, frame_len in {160, 1024} and channels in {1024, 16384, 65536} (frames chosen to keep the total).
Each configuration runs in a fresh child process under a time limit; ms is the median of --steps timed calls, GB/s counts 8 B
per sample (one read, one write).  Next to the residual stands the device-to-device copy of the same bytes, timed in the same
run: the bound the residual is held against.  Next to the synthesis stands the same recursion on one host core: the numpy
model of the tests (tests/lpc_filter_checks.py synth_model) timed on 64 channels x 2048 samples and scaled to the total.

    python tools/time_lpc_filter.py [--log2-samples 28] [--steps 10] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(p, fl, ch) for fl in (160, 1024) for ch in (1024, 16384, 65536) for p in (10, 16, 32, 64)]


def median_ms(call, steps, torch):
    for _ in range(2):
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
    return sorted(times)[len(times) // 2]


def child(total, p, frame_len, channels, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from llzlab_amd import filters
    from tests import lpc_filter_checks as lc
    dev = torch.device("cuda:0")
    frames = max(1, total // (channels * frame_len))
    n = channels * frames * frame_len
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.rand(channels, frames * frame_len, dtype=torch.float32, device=dev, generator=gen) - 0.5
    # a few stable sets (|k_i| <= 0.5), spread over the (channel, frame) grid
    sets = torch.from_numpy(lc.step_up(np.random.RandomState(p).uniform(-0.5, 0.5, size=(257, p))).astype(np.float32)).to(dev)
    idx = (torch.arange(channels * frames, device=dev) * 7919) % 257
    acof = sets[idx].view(channels, frames, p + 1).contiguous()
    e, y = torch.empty_like(x), torch.empty_like(x)
    f = filters.LpcFilterMC(channels, frame_len, p)
    row = {"p": p, "frame_len": frame_len, "channels": channels, "frames": frames, "samples": n}
    gbs = lambda ms: round(n * 8 / ms / 1e6, 1)  # noqa: E731
    ms = median_ms(lambda: f.residual(x, acof, e), steps, torch)
    row.update(residual_ms=round(ms, 4), residual_GBs=gbs(ms))
    ms = median_ms(lambda: e.copy_(x), steps, torch)
    row.update(copy_ms=round(ms, 4), copy_GBs=gbs(ms))
    ms = median_ms(lambda: f.synth(e, acof, y), max(3, steps // 3), torch)
    row.update(synth_ms=round(ms, 4), synth_GBs=gbs(ms))
    f.close()
    hc, ht = 64, 2048
    he = np.random.RandomState(1).uniform(-0.5, 0.5, size=(hc, ht)).astype(np.float32)
    ha = acof[:hc, :max(1, ht // frame_len) + 1].cpu().numpy() if channels >= hc else None
    if ha is not None:
        t0 = time.perf_counter()
        lc.synth_model(he, ha, frame_len)
        row["host_synth_model_ms_scaled"] = round((time.perf_counter() - t0) * 1e3 * n / (hc * ht), 1)
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=28)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=3, type=int)
    a = ap.parse_args()
    if a.child:
        child(1 << a.log2_samples, a.child[0], a.child[1], a.child[2], a.steps)
        return
    rows = []
    for p, fl, ch in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--log2-samples", str(a.log2_samples), "--steps", str(a.steps),
               "--child", str(p), str(fl), str(ch)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"p={p} frame_len={fl} channels={ch}: over {a.timeout} s", file=sys.stderr)
            break                                       # nothing more on the GPU after a hang
        if res.returncode != 0:
            print(f"p={p} frame_len={fl} channels={ch}: exit {res.returncode}\n{res.stderr[-2000:]}", file=sys.stderr)
            break                                       # nothing more on the GPU after a failure
        row = json.loads(res.stdout.strip().splitlines()[-1])
        rows.append(row)
        print(f"p={p:3d} frame_len={fl:5d} channels={ch:6d}  residual {row['residual_ms']:8.3f} ms {row['residual_GBs']:7.1f} GB/s"
              f"  copy {row['copy_GBs']:7.1f} GB/s  synth {row['synth_ms']:9.3f} ms {row['synth_GBs']:7.1f} GB/s"
              f"  host {row.get('host_synth_model_ms_scaled', 0):.0f} ms", flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
    sys.exit(0 if len(rows) == len(CONFIGS) else 1)


if __name__ == "__main__":
    main()
