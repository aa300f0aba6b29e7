"""GPU checks of the polyphase DFT filter bank (include/llz_pfb.h, llz_pfb_mc; kernels/pfb.hip) against the float64 definition
and the derived limits of tests/pfb_checks.py: every shape on 3 and 37 channels in both phases over calls of 1, R - 1, R, R + 1
and 300 frames; bit for bit across call grouping, analysis forms, neighbours and pointer kinds; the TIME phase's steady phasor;
P = 1 against llz_stft_mc; the round trip; guarded buffers and refused overlaps.  Every case prints its worst ratio to its limit.
On the parent of this feature the library exports no llz_pfb_mc and every test here fails."""
import numpy as np
import pytest
import torch

from llzlab_amd import capi, filters
from tests import buffer_checks as bc
from tests import pfb_checks as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                     # (a copy: the shared references are read-only)


def run_analysis(f, x, calls, to=dev):
    """the stream x [channels, frames D] through handle f in calls of `calls` frames: complex64 [channels, frames, bins]"""
    outs, t, D = [], 0, f.hop
    for n in calls:
        xs = to(x[:, t * D:(t + n) * D])
        re, im = to(np.zeros((f.channels, n, f.bins), np.float32)), to(np.zeros((f.channels, n, f.bins), np.float32))
        f.analysis(xs, re, im)
        outs.append(np.asarray(re.cpu() if hasattr(re, "cpu") else re) + 1j * np.asarray(im.cpu() if hasattr(im, "cpu") else im))
        t += n
    return np.concatenate(outs, axis=1).astype(np.complex64)


def run_synthesis(f, re, im, calls, to=dev):
    outs, t = [], 0
    for n in calls:
        x = to(np.zeros((f.channels, n * f.hop), np.float32))
        f.synthesis(to(re[:, t:t + n]), to(im[:, t:t + n]), x)
        outs.append(np.asarray(x.cpu() if hasattr(x, "cpu") else x))
        t += n
    return np.concatenate(outs, axis=1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def bank(channels, M, P, os, phase=pc.FRAME):
    w, g = pc.windows(M, P)
    return filters.PfbMC(channels, M, M // os, P, w, g, phase)


@pytest.mark.parametrize("phase", pc.PHASES)
@pytest.mark.parametrize("channels", pc.CHANNELS)
@pytest.mark.parametrize("M,P,os", pc.SHAPES)
def test_shapes_hold_the_limits(M, P, os, channels, phase):
    """dense channels under the 1e-5 gate, every channel (the sparse ones one product per sum) within the per-value limits, both
    directions; the (4096, 8, 1) shape takes the analysis form that reads through the caches (and so does (1024, 8, 4), whose
    prototype alone fills most of the LDS budget), the other shapes the LDS form"""
    f = bank(channels, M, P, os, phase)
    (form, per_wg, wgs, lds), (sform, sper, swgs, slds) = f.plan(pc.LONG)
    assert form == {4096: 1, 1024: 1}.get(M, 0) and per_wg >= 1 and wgs >= channels and 0 < lds <= 64 * 1024
    assert sform == 1 and sper >= 1 and swgs >= 1 and 0 < slds <= 64 * 1024
    worst, dense = pc.check_analysis(lambda x, w, calls: run_analysis(f, x, calls), channels, M, P, os, phase, "MI355X")
    assert worst <= 1.0 and dense <= pc.GATE
    worst, dense = pc.check_synthesis(lambda re, im, g, calls: run_synthesis(f, re, im, calls), channels, M, P, os, phase, "MI355X")
    assert worst <= 1.0 and dense <= pc.GATE
    assert f.frames() == (sum(pc.call_frames(M, P, os)),) * 2
    f.close()


@pytest.mark.parametrize("M,P,os", [(16, 3, 4), (64, 4, 2), (1024, 8, 4), (8, 1, 1)])
def test_bits_do_not_depend_on_call_grouping(M, P, os):
    """all frames in one call, one frame per call, an uneven split with an empty call: equal bits in both directions, in both
    phases, and again behind a reset"""
    channels, R = 5, P * os
    total = 3 * R + 7
    rng = np.random.default_rng(11)
    x = rng.standard_normal((channels, total * (M // os))).astype(np.float32)
    re = rng.standard_normal((channels, total, M // 2 + 1)).astype(np.float32)
    im = rng.standard_normal((channels, total, M // 2 + 1)).astype(np.float32)
    im[:, :, 0] = im[:, :, -1] = 0
    uneven = [1, R - 1, 0, 5, R + 1, total - 2 * R - 6]
    assert sum(uneven) == total
    for phase in pc.PHASES:
        f = bank(channels, M, P, os, phase)
        X0, y0 = run_analysis(f, x, [total]), run_synthesis(f, re, im, [total])
        for calls in ([1] * total, uneven):
            f.reset()
            assert f.frames() == (0, 0)
            assert same_bits(run_analysis(f, x, calls).view(np.float32), X0.view(np.float32)), (phase, calls[:3])
            assert same_bits(run_synthesis(f, re, im, calls), y0), (phase, calls[:3])
        f.close()


@pytest.mark.parametrize("M,P,os,channels", [(64, 4, 2, 37), (1024, 2, 4, 37), (256, 16, 8, 3), (16, 3, 4, 3)])
def test_pfb_global_gives_the_bits_of_the_default_form(M, P, os, channels):
    """the fold through the caches and the fold from the LDS span, and with them other frames per workgroup: equal bits"""
    x = pc.case_x(channels, M, P, os, seed=5)[:, :(pc.LONG + 3) * (M // os)]
    calls = [3, pc.LONG]
    f = bank(channels, M, P, os, pc.TIME)
    plan0 = f.plan(pc.LONG)[0]
    X0 = run_analysis(f, x, calls)
    with capi.tuned(pfb_global=1):
        f.reset()
        plan1 = f.plan(pc.LONG)[0]
        X1 = run_analysis(f, x, calls)
    assert plan0[0] == 0 and plan1[0] == 1 and plan1[3] < plan0[3]
    assert same_bits(X0.view(np.float32), X1.view(np.float32))
    f.close()


@pytest.mark.parametrize("M,P,os", [(64, 4, 2), (1024, 8, 4), (4096, 8, 1)])
def test_neighbours_change_no_bit(M, P, os):
    """channel 1 of 3 next to neighbours scaled by 2^20, zeroed or NaN; and a NaN block reaches exactly the frames that cover it"""
    channels, R, D = 3, P * os, M // os
    total = 2 * R + 9
    rng = np.random.default_rng(13)
    x = rng.standard_normal((channels, total * D)).astype(np.float32)
    re = rng.standard_normal((channels, total, M // 2 + 1)).astype(np.float32)
    im = rng.standard_normal((channels, total, M // 2 + 1)).astype(np.float32)
    im[:, :, 0] = im[:, :, -1] = 0
    f = bank(channels, M, P, os, pc.TIME)
    X0, y0 = run_analysis(f, x, [total]), run_synthesis(f, re, im, [total])
    for scale in (2.0 ** 20, 0.0, np.nan):
        xs, res, ims = x.copy(), re.copy(), im.copy()
        for c in (0, 2):
            xs[c] = xs[c] * np.float32(scale)
            res[c] = res[c] * np.float32(scale)
            ims[c, :, 1:-1] = ims[c, :, 1:-1] * np.float32(scale)
        f.reset()
        X1, y1 = run_analysis(f, xs, [total]), run_synthesis(f, res, ims, [total])
        assert same_bits(X1[1].view(np.float32), X0[1].view(np.float32)), scale
        assert same_bits(y1[1], y0[1]), scale
    b = R + 2                                                        # a NaN hop / a NaN frame in channel 1
    xs, res = x.copy(), re.copy()
    xs[1, b * D:(b + 1) * D] = np.nan
    res[1, b, 1] = np.nan
    f.reset()
    X1, y1 = run_analysis(f, xs, [total]), run_synthesis(f, res, im, [total])
    hit = np.zeros(total, bool)
    hit[b:b + R] = True
    assert np.array_equal(np.isnan(X1[1]).all(axis=1), hit) and np.array_equal(np.isnan(X1[1]).any(axis=1), hit)
    yb = np.isnan(y1[1]).reshape(total, D)
    assert np.array_equal(yb.all(axis=1), hit) and np.array_equal(yb.any(axis=1), hit)
    for c in (0, 2):
        assert same_bits(X1[c].view(np.float32), X0[c].view(np.float32)) and same_bits(y1[c], y0[c])
    f.close()


@pytest.mark.parametrize("M,P", [(64, 4), (1024, 8)])
def test_time_phase_holds_a_tone_still(M, P):
    """cos(2 pi k0 t / M) under a raised-cosine prototype of L points (whose response at the image frequency 2 k0 / M is an exact
    zero): in TIME phase X_m[k0] is one phasor once the history is full, in FRAME phase it turns by e^{j 2 pi k0 (m + 1) D / M}
    (a quarter turn times k0 (m + 1) at M / D = 4), each within the sum of the two frames' limits"""
    os, k0 = 4, 5
    D, L, R = pc.geometry(M, P, os)
    frames = 2 * R + 11
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(L) / L)).astype(np.float32)
    t = np.arange(frames * D)
    x = np.tile(np.cos(2 * np.pi * k0 * t / M).astype(np.float32), (2, 1))
    for phase in pc.PHASES:
        f = filters.PfbMC(2, M, D, P, w, None, phase)
        X = run_analysis(f, x, [frames])[:, :, k0].astype(np.complex128)
        f.close()
        _, lim = pc.analysis(x, w, M, P, os, phase)
        if phase == pc.FRAME:
            X = X * (1j ** (-k0 * (np.arange(frames) + 1) % 4))[None, :]
        steady = X[:, R - 1:]
        worst = pc.ratio(np.abs(steady - steady[:, :1]), lim[:, R - 1:] + lim[:, R - 1:R])
        print(f"tone at bin {k0}, M={M} P={P} phase={phase}: |X_m - X_(R-1)| / (sum of limits) at most {worst:.3g}; |X| = {abs(steady[0, 0]):.6g}")
        assert worst <= 1.0 and abs(steady[0, 0]) > 0.2 * np.sum(w)


def test_time_and_frame_phase_agree_at_critical_sampling():
    M, P, os, channels = 64, 4, 1, 3
    x = pc.case_x(channels, M, P, os, seed=3)[:, :40 * M]
    re, im = pc.case_spectra(channels, M, P, os, seed=3)
    fa, fb = bank(channels, M, P, os, pc.FRAME), bank(channels, M, P, os, pc.TIME)
    assert same_bits(run_analysis(fa, x, [40]).view(np.float32), run_analysis(fb, x, [40]).view(np.float32))
    assert same_bits(run_synthesis(fa, re[:, :40], im[:, :40], [40]), run_synthesis(fb, re[:, :40], im[:, :40], [40]))
    fa.close()
    fb.close()


@pytest.mark.parametrize("hint,frame_len", [(capi.OVERLAP_HIGH, 64), (capi.OVERLAP_LOW, 512), (capi.OVERLAP_HIGH, 1024)])
def test_one_tap_per_band_is_the_stft(hint, frame_len):
    """P = 1 with llz_hamming's window against llz_stft_mc_analysis at the same fft_len and hop, within the sum of both limits"""
    channels, os = 3, 4 if hint == capi.OVERLAP_HIGH else 2
    M, frames = frame_len * os, 37
    L = capi.lib()
    wd = np.zeros(M)
    assert L.llz_hamming(wd.ctypes.data_as(filters._dp), M) >= 0
    w = wd.astype(np.float32)
    x = np.random.default_rng(17).standard_normal((channels, frames * frame_len)).astype(np.float32)
    f = filters.PfbMC(channels, M, frame_len, 1, w)
    X = run_analysis(f, x, [frames])
    f.close()
    s = filters.StftMC(channels, hint, frame_len, capi.HAMMING)
    re, im = torch.empty(channels, frames, s.bins, device=DEV), torch.empty(channels, frames, s.bins, device=DEV)
    s.analysis(dev(x), re, im)
    S = re.cpu().numpy() + 1j * im.cpu().numpy()
    s.close()
    Xref, lim = pc.analysis(x, w, M, 1, os, pc.FRAME)
    worst = pc.ratio(np.abs(X.astype(np.complex128) - S), 2 * lim[..., None])
    print(f"P = 1 against llz_stft_mc, fft_len {M} hop {frame_len}: |difference| / (sum of limits) at most {worst:.3g}; "
          f"against float64 {pc.ratio(np.abs(X - Xref), lim[..., None]):.3g}")
    assert worst <= 1.0


def test_round_trip():
    """P = 1, square-root Hann at D = M / 2 returns the input delayed by llz_pfb_mc_delay, within the synthesis limit of the
    spectra fed back; the reconstruction error of pfb_prototype at P = 8, M / D = 4 with w = g is printed, not asserted (it is
    the prototype's)"""
    channels, M, frames = 3, 256, 41
    w = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(M) / M)).astype(np.float32)
    x = np.random.default_rng(19).standard_normal((channels, frames * M // 2)).astype(np.float32)
    f = filters.PfbMC(channels, M, M // 2, 1, w)
    assert f.delay == M // 2 and f.bins == M // 2 + 1
    X = run_analysis(f, x, [frames])
    re, im = np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag)
    y = run_synthesis(f, re, im, [frames])
    f.close()
    _, lim = pc.synthesis(re, im, w, M, 1, 2, pc.FRAME)
    worst = pc.ratio(np.abs(y[:, f.delay:].astype(np.float64) - x[:, :-f.delay]), lim[:, f.delay:])
    print(f"round trip, square-root Hann, M={M} D={M // 2}: |y[t + delay] - x[t]| / limit at most {worst:.3g}")
    assert worst <= 1.0
    M, P, os = 256, 8, 4
    h = filters.pfb_prototype(M, P)
    assert h.dtype == np.float32 and h.shape == (M * P,)
    x = np.random.default_rng(23).standard_normal((channels, 200 * M // os)).astype(np.float32)
    f = filters.PfbMC(channels, M, M // os, P, h, None, pc.TIME)
    X = run_analysis(f, x, [200])
    y = run_synthesis(f, np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag), [200])
    e = y[:, f.delay:] - x[:, :-f.delay]
    print(f"pfb_prototype({M}, {P}), M/D = {os}, w = g: reconstruction error rms {np.sqrt(np.mean(e * e) / np.mean(x * x)):.3g} of the input's")
    f.close()


@pytest.mark.parametrize("M,P,os", [(64, 4, 2), (1024, 8, 4)])
def test_host_pointers_give_the_bits_of_device_pointers(M, P, os):
    channels = 3
    x = pc.case_x(channels, M, P, os, seed=7)[:, :50 * (M // os)]
    re, im = (a[:, :50] for a in pc.case_spectra(channels, M, P, os, seed=7))
    fd, fh = bank(channels, M, P, os, pc.TIME), bank(channels, M, P, os, pc.TIME)
    host = np.ascontiguousarray
    assert same_bits(run_analysis(fd, x, [7, 43]).view(np.float32), run_analysis(fh, x, [7, 43], to=host).view(np.float32))
    assert same_bits(run_synthesis(fd, re, im, [7, 43]), run_synthesis(fh, re, im, [7, 43], to=host))
    fd.close()
    fh.close()


@pytest.mark.parametrize("M,P,os,offset", [(64, 4, 2, 1), (1024, 8, 4, 3), (4096, 8, 1, 1)])
def test_guarded_buffers_at_odd_offsets(M, P, os, offset):
    """inputs between NaN bands, outputs between sentinel bands, every buffer `offset` elements past an aligned address: the
    bands come back unchanged, every output element is written, the inputs are not, and the values are those of plain buffers"""
    channels, frames, D = 3, 19, M // os
    x = pc.case_x(channels, M, P, os, seed=9)[:, :frames * D]
    re, im = (np.ascontiguousarray(a[:, :frames]) for a in pc.case_spectra(channels, M, P, os, seed=9))
    f = bank(channels, M, P, os, pc.TIME)
    X0, y0 = run_analysis(f, x, [frames]), run_synthesis(f, re, im, [frames])
    f.reset()
    bins = M // 2 + 1
    gx = bc.carve_input(DEV, x, offset)
    gre, gim = bc.carve(DEV, torch.float32, channels * frames * bins, offset), bc.carve(DEV, torch.float32, channels * frames * bins, offset + 2)
    snap = bc.snapshot(gx)
    f.analysis(gx.shaped(channels, frames * D), gre.shaped(channels, frames, bins), gim.shaped(channels, frames, bins))
    torch.cuda.synchronize()
    bc.check_untouched(gx, snap)
    for b in (gre, gim):
        bc.check_bands(b)
    X1 = bc.check_all_written(gre).reshape(channels, frames, bins) + 1j * bc.check_all_written(gim).reshape(channels, frames, bins)
    assert same_bits(X1.astype(np.complex64).view(np.float32), X0.view(np.float32))
    gre, gim = bc.carve_input(DEV, re, offset), bc.carve_input(DEV, im, offset + 2)
    gy = bc.carve(DEV, torch.float32, channels * frames * D, offset)
    snaps = bc.snapshot(gre), bc.snapshot(gim)
    f.synthesis(gre.shaped(channels, frames, bins), gim.shaped(channels, frames, bins), gy.shaped(channels, frames * D))
    torch.cuda.synchronize()
    bc.check_untouched(gre, snaps[0])
    bc.check_untouched(gim, snaps[1])
    bc.check_bands(gy)
    assert same_bits(bc.check_all_written(gy).reshape(channels, frames * D), y0)
    f.close()


def test_overlapping_device_ranges_are_refused_and_the_handle_continues():
    M, P, os, channels, frames = 64, 4, 2, 2, 9
    D, bins = M // os, M // 2 + 1
    x = pc.case_x(channels, M, P, os, seed=21)[:, :2 * frames * D]
    re, im = (np.ascontiguousarray(a[:, :2 * frames]) for a in pc.case_spectra(channels, M, P, os, seed=21))
    f, ref = bank(channels, M, P, os, pc.TIME), bank(channels, M, P, os, pc.TIME)
    X0, y0 = run_analysis(ref, x, [frames, frames]), run_synthesis(ref, re, im, [frames, frames])
    Xa, ya = run_analysis(f, x, [frames]), run_synthesis(f, re, im, [frames])
    nx, ns = channels * frames * D, channels * frames * bins
    other = torch.zeros(ns, device=DEV)
    for a, b in bc.overlap_cases(nx, ns, device=DEV):
        a.copy_(dev(x[:, frames * D:]).view(-1))
        before = bc.bits(a).copy(), bc.bits(b).copy()
        for args in ((a, b, other), (a, other, b)):
            with pytest.raises(capi.LlzError, match="may not overlap"):
                f.analysis(args[0].view(channels, -1), args[1].view(channels, frames, bins), args[2].view(channels, frames, bins))
        assert np.array_equal(bc.bits(a), before[0])
    for a, b in bc.overlap_cases(ns, nx, device=DEV):
        for args in ((a, other, b), (other, a, b)):
            with pytest.raises(capi.LlzError, match="may not overlap"):
                f.synthesis(args[0].view(channels, frames, bins), args[1].view(channels, frames, bins), args[2].view(channels, -1))
    assert f.frames() == (frames, frames)
    Xb = run_analysis(f, x[:, frames * D:], [frames])
    yb = run_synthesis(f, re[:, frames:], im[:, frames:], [frames])
    assert same_bits(np.concatenate([Xa, Xb], axis=1).view(np.float32), X0.view(np.float32))
    assert same_bits(np.concatenate([ya, yb], axis=1), y0)
    f.close()
    ref.close()
