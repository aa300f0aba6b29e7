#!/usr/bin/env python3
"""Event-timed llz_stft_mc_* above 2048 points on one GPU: at fft_len 4096 the one-launch kernels (the library's choice)
against the composed form (the fft_generic tune) in the same run, then the composed form (the library's choice above 4096)
at 8192 and larger sizes.  The byte count is tools/time_paths.py's: 4 B per sample plus 8 B per bin.

    python tools/time_stft_large.py [--quick]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from llzlab_amd import capi, filters  # noqa: E402

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
L = capi.lib()
capi.check(L.llz_hip_set_device(0), "set_device")
stream = torch.cuda.current_stream()
sptr = stream.cuda_stream


def timeit(fn, steps):
    """tools/time_paths.py's timer: mean over >= `steps` calls and >= 30 ms, after >= 30 ms of warm-up calls"""
    def run(k):
        t = L.llz_hip_timer_new()
        L.llz_hip_timer_start(t, sptr)
        for _ in range(k):
            fn()
        L.llz_hip_timer_stop(t, sptr)
        ms = L.llz_hip_timer_ms(t) / k
        L.llz_hip_timer_free(t)
        return ms
    fn()
    torch.cuda.synchronize()
    once = max(run(1), 1e-3)
    reps = max(steps, min(2000, int(30.0 / once) + 1))
    run(reps)
    return run(reps)


def shape(hint, F, ch, frames, forms):
    n = F * frames
    x = torch.rand(ch, n, dtype=torch.float32, device=dev) * 2 - 1
    y = torch.empty_like(x)
    for name, generic in forms:
        with capi.tuned(fft_generic=generic):
            q = filters.StftMC(ch, hint, F, filters.BLACKMAN, stream=stream)
            re = torch.empty(ch, frames, q.bins, dtype=torch.float32, device=dev)
            im = torch.empty_like(re)
            ms_a = timeit(lambda: q.analysis(x, re, im), 5)
            ms_s = timeit(lambda: q.synthesis(re, im, y), 5)
            b = 4 * ch * n + 8 * ch * frames * q.bins
            print(f"stft {'3/4' if hint == 0 else '1/2'} overlap fft_len={F << (2 if hint == 0 else 1)} F={F} {ch}ch x "
                  f"{frames} frames [{name}]: analysis {ms_a:.3f} ms {b / ms_a / 1e9:.2f} TB/s, synthesis {ms_s:.3f} ms "
                  f"{b / ms_s / 1e9:.2f} TB/s", flush=True)
            q.close()
            del re, im
    del x, y


quick = "--quick" in sys.argv[1:]
for hint, F in ((0, 1024), (1, 2048)):                                     # fft_len 4096
    shape(hint, F, 1024, 128, (("one-launch", -1), ("composed", 1)))
for hint, F in ((0, 2048), (1, 4096)):                                     # fft_len 8192
    shape(hint, F, 1024, 128, (("composed", -1),))
if not quick:
    shape(0, 512, 1024, 128, (("fft_len 2048, for scale", -1),))
    for hint, F, ch, frames in ((0, 4096, 1024, 64), (1, 32768, 256, 32), (0, 262144, 16, 16), (1, 1 << 23, 2, 4)):
        shape(hint, F, ch, frames, (("composed", -1),))
