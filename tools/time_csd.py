#!/usr/bin/env python3
"""Event-timed Welch cross-spectra on one GPU: filters.CsdMC (update + the CSD read-out, the fused form of kernels/csd.hip)
against the composed path that needs nothing new -- StftMC.analysis on the x and on the y channels, then the product and the
mean over frames in torch -- in the same process, alternating, median of the repeats.  1024 pairs (i, 1024 + i) of 2048
channels x 2^18 samples at fft_len 1024 / hop 512 and at 256 / 128.

The composed path computes something else at its start (StftMC begins with a zero history, so its first frame is half zeros)
and sums in another order; the comparison is of time and traffic, and the two spectra are compared at 1e-3 of the mean.
Bytes: the least each form must move -- fused: every sample once and [pairs][bins][4] floats per run written, read by the
fold, plus the read-out; composed: every sample once, frames x bins x 8 B per channel written and read back, the product's
output written and read by the mean.

    python tools/time_csd.py [--quick] [--out FILE]
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


def shape(N, hop, pairs, n, repeats):
    assert N == 2 * hop, "the composed path is StftMC at 1/2 overlap: fft_len must be 2 hop"
    channels = 2 * pairs
    bins, frames = N // 2 + 1, (n - N) // hop + 1
    x = torch.rand(channels, n, dtype=torch.float32, device=dev) * 2 - 1
    x[pairs:] = 0.5 * x[:pairs].roll(3, dims=1) + 0.5 * x[pairs:]       # y: a delayed copy plus its own noise
    table = [(i, pairs + i) for i in range(pairs)]
    h = filters.CsdMC(channels, table, N, hop, filters.HAMMING, stream=stream)
    out = torch.empty(pairs, bins, 2, dtype=torch.float32, device=dev)
    sx = filters.StftMC(pairs, capi.OVERLAP_LOW, hop, filters.HAMMING, stream=stream)
    sy = filters.StftMC(pairs, capi.OVERLAP_LOW, hop, filters.HAMMING, stream=stream)
    sframes = n // hop
    re = [torch.empty(pairs, sframes, bins, dtype=torch.float32, device=dev) for _ in range(2)]
    im = [torch.empty_like(re[0]) for _ in range(2)]
    u = float((torch.from_numpy(filters.window(filters.HAMMING, N).astype("float32")).double() ** 2).sum())

    def fused():
        h.reset()
        h.update(x)
        h.csd(out)

    def composed():
        sx.analysis(x[:pairs], re[0], im[0])
        sy.analysis(x[pairs:], re[1], im[1])
        X, Y = torch.complex(re[0], im[0]), torch.complex(re[1], im[1])
        return (torch.conj(X) * Y).mean(dim=1) / u

    plan = h.plan(n)
    for _ in range(2):                                                  # warm-up of both, every shape the timed window uses
        fused()
        ref = composed()
    torch.cuda.synchronize()
    tf, tc_ = [], []
    for _ in range(repeats):                                            # alternating
        tf.append(timed(fused))
        tc_.append(timed(composed))
    got = torch.view_as_complex(out)
    # the composed path's first frame starts in a zero history and it has one frame more: compare loosely
    rel = float((got - ref).abs().mean() / ref.abs().mean())
    fused_bytes = 4 * channels * n + 2 * 16 * pairs * bins * ((frames + 31) // 32) + (32 + 8) * pairs * bins
    composed_bytes = 4 * channels * n + 2 * 8 * channels * sframes * bins + 2 * 8 * pairs * sframes * bins + 8 * pairs * bins
    mf, mc = statistics.median(tf), statistics.median(tc_)
    say(f"csd fft_len={N} hop={hop} {pairs} pairs of {channels} ch x {n} samples, {frames} frames, plan {plan}")
    say(f"  fused    CsdMC.update + csd : median {mf:8.3f} ms (min {min(tf):.3f} max {max(tf):.3f}, {repeats} repeats), "
        f"{fused_bytes / 1e9:.2f} GB -> {fused_bytes / mf / 1e9:.2f} TB/s")
    say(f"  composed 2 x StftMC + torch : median {mc:8.3f} ms (min {min(tc_):.3f} max {max(tc_):.3f}), "
        f"{composed_bytes / 1e9:.2f} GB -> {composed_bytes / mc / 1e9:.2f} TB/s")
    say(f"  fused / composed = {mf / mc:.3f}; mean |difference| of the two cross-spectra {rel:.2e} of the mean magnitude")
    h.close()
    sx.close()
    sy.close()


pairs, n = (64, 1 << 15) if quick else (1024, 1 << 18)
for N, hop in ((1024, 512), (256, 128)):
    shape(N, hop, pairs, n, 5 if quick else 9)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
