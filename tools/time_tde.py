#!/usr/bin/env python3
"""Event-timed time-delay estimator on one GPU: filters.TdeMC.process (kernels/tde.hip: one launch, a workgroup per pair, three
transforms per pair and frame) next to filters.CsdMC.update of the same shape forced to its staged form (fft_generic = 1:
k_csd_staged_f32, a workgroup per (pair, run of 32 frames), two of the three transforms) in the same process, alternating, median
of the repeats.  Pairs 8 and 1024 x fft_len 256, 1024, 4096 x hop fft_len / 2 x 1 and 64 frames per call, in the steady state
(both handles past their first frame; every call takes frames x hop new samples of 2 x pairs channels, pair i = (i, pairs + i)).

A call's time is the whole call between two events on the stream: the kernel and the history copy behind it.  There is no pass
mark; the ratio says what the serial walk of the frames and the third transform cost.

    python tools/time_tde.py [--quick] [--out FILE]
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


def shape(N, pairs, frames, repeats):
    hop, channels = N // 2, 2 * pairs
    n = frames * hop
    x = torch.rand(channels, n, dtype=torch.float32, device=dev) * 2 - 1
    x[pairs:] = x[:pairs].roll(3, dims=1) + 0.3 * x[pairs:]             # y: x delayed by 3 samples plus its own noise
    table = [(i, pairs + i) for i in range(pairs)]
    t = filters.TdeMC(channels, table, N, hop, min(64, N // 2 - 1), capi.TDE_PHAT, 0.9, 0.0, None, filters.HAMMING, stream=stream)
    c = filters.CsdMC(channels, table, N, hop, filters.HAMMING, stream=stream)
    delay = torch.empty(pairs, frames, dtype=torch.float32, device=dev)
    peak = torch.empty_like(delay)
    lead = x[:, :hop].contiguous()

    def tde():
        t.process(x, delay, peak)

    def csd():
        c.update(x)

    with capi.tuned(fft_generic=1):
        assert c.plan(n)["form"] == 0, "the yardstick is the staged form"
        t.process(lead, delay, peak)                                    # past the first frame: every call completes `frames`
        c.update(lead)
        for _ in range(2):
            tde()
            csd()
        torch.cuda.synchronize()
        tt, tc_ = [], []
        for _ in range(repeats):                                        # alternating
            tt.append(timed(tde))
            tc_.append(timed(csd))
    found = float((delay.round() == 3).float().mean())
    mt, mc = statistics.median(tt), statistics.median(tc_)
    say(f"tde fft_len={N} hop={hop} pairs={pairs} frames/call={frames}: process median {mt:8.3f} ms (min {min(tt):.3f} max "
        f"{max(tt):.3f}, {repeats} repeats) = {1e3 * mt / frames:8.2f} us/frame; csd staged update median {mc:8.3f} ms (min "
        f"{min(tc_):.3f} max {max(tc_):.3f}); tde / csd = {mt / mc:.2f}; planted delay found in {100 * found:.1f} % of the outputs")
    t.close()
    c.close()


for N in (256, 1024, 4096):
    for pairs in (8, 1024):
        for frames in (1, 64):
            shape(N, pairs, frames, 5 if quick else 9)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
