"""The DFT of any length and the zoom transform on the MI355X (include/llz_dft.h, filters.DftMC / CztMC; kernels/dft.hip) against
the float64 definition of tests/dft_checks.py, over its case table.

  1. parity on both limits (per bin, and the RMS gate on the dense rows): every entry point on 3 and 37 rows of Gaussian rows,
     off-bin tones and impulses at n - 1; the fused form at every listed length, the composed form with a scratch cap under
     which one call walks two slabs, the composed form forced where the fused one would be taken, the zoom cases;
  2. identities: inverse(forward(x)), rforward against forward, the imaginary parts rinverse drops, the zoom that is the DFT,
     a window of 0.5, a Hann window;
  3. bit pins: a row's bits do not depend on count, position, neighbours (scaled, zeroed, NaN), host or device pointers, element
     offsets or in_pitch; a zero row gives zero; a row scaled by 2^k gives the output scaled;
  4. guarded buffers (tests/buffer_checks.py) and the refusals, with the handle alive behind each.

Each parity case prints its worst ratio to both limits.  Every test fails on the parent, which exports no such symbol."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402
from tests import dft_checks as dk  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG = -1
F32 = torch.float32
OPS = ("forward", "inverse", "rforward", "rinverse")
PIN_N = (17, 480, 2047)                 # 32, 2 and 1 rows per workgroup


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    capi.build()
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


_CACHE = {}


def cached(key, make):
    """inputs and references: computed once, shared by the tests that need them, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case_input(op, n, count):
    def make():
        x = dk.rows(n, count, real=op in ("rforward", "rzoom"))
        return x[:, :n // 2 + 1].copy() if op == "rinverse" else x
    return cached(("in", op, n, count), make)


def reference(op, n, count):
    return cached(("ref", op, n, count), lambda: dk.ref64(op, case_input(op, n, count), n))


def run(dev, h, op, x, **kw):
    """`op` of the handle on the rows of x (numpy, [count, row]) through device memory; the result on the host"""
    out = getattr(h, op)(torch.from_numpy(np.ascontiguousarray(x)).to(dev), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    va, vb = a.view(np.uint32), b.view(np.uint32)
    bad = np.flatnonzero(va.reshape(-1) != vb.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {va.size} words differ, the first at {int(bad[0])}"


def parity(dev, h, n, count, label):
    for op in OPS:
        x = case_input(op, n, count)
        got = run(dev, h, op, x)
        dk.check(got, reference(op, n, count), dk.bin_limit(op, x, n), dk.dense(count), f"{label} {op} n={n} rows={count}")


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("n", dk.FUSED_N)
def test_fused_parity(dev, n):
    h = filters.DftMC(n)
    for count in dk.ROWS:
        plan = h.plan(count)
        assert plan["form"] == capi.DFT_FUSED and plan["m"] == dk.m_of(n, n) and plan["tpw"] == dk.tpw_of(plan["m"], count)
        assert plan["slabs"] == 1 and 0 < plan["lds"] <= 65536
        parity(dev, h, n, count, "fused")
    h.close()


@pytest.mark.parametrize("n,mb", zip(dk.COMPOSED_N, (2, 4, 4)))
def test_composed_parity_over_two_slabs(dev, n, mb):
    h = filters.DftMC(n)
    counts = dk.ROWS if n < 65537 else dk.ROWS[:1]
    h.configure(scratch_mb=mb)
    plan = h.plan(counts[-1])
    assert plan["form"] == capi.DFT_COMPOSED and plan["m"] == dk.m_of(n, n) and plan["slabs"] == 2, plan
    for count in counts:
        parity(dev, h, n, count, f"composed, {h.plan(count)['slabs']} slab(s),")
    h.configure()
    assert h.plan(counts[-1])["slabs"] == 1
    h.close()


@pytest.mark.parametrize("n", dk.FORCED_N)
def test_forced_composed_parity_and_agreement_with_fused(dev, n):
    """configure(composed=True) on a handle the fused kernel would serve; the two forms agree within the limits, not bit for
    bit; configured back, the handle gives the fused form's bits again"""
    hc, hf = filters.DftMC(n), filters.DftMC(n)
    hc.configure(composed=True, scratch_mb=0)                   # a row per slab
    assert hc.plan(37)["form"] == capi.DFT_COMPOSED and hf.plan(37)["form"] == capi.DFT_FUSED
    assert hc.plan(37)["slabs"] == 37
    parity(dev, hc, n, 37, "forced composed, a row per slab,")
    hc.configure(composed=True)
    assert hc.plan(37)["slabs"] == 1
    parity(dev, hc, n, 3, "forced composed")
    for op in OPS:
        x = case_input(op, n, 37)
        a, b = run(dev, hf, op, x), run(dev, hc, op, x)
        lim = dk.bin_limit(op, x, n)
        worst = dk.worst_bin(a, b.astype(np.complex128), lim)
        print(f"fused against composed {op} n={n}: {worst:.3g} of the per-bin limit")
        assert worst <= 2.0
    hc.configure()
    assert hc.plan(37)["form"] == capi.DFT_FUSED
    x = case_input("forward", n, 37)
    same_bits(run(dev, hc, "forward", x), run(dev, hf, "forward", x), f"n={n}: configured back to the library's choice")
    hc.close()
    hf.close()


@pytest.mark.parametrize("n,k,f0,df", dk.ZOOMS)
def test_zoom_parity(dev, n, k, f0, df):
    h = filters.CztMC(n, k, f0, df)
    for count in dk.ROWS:
        plan = h.plan(count)
        assert plan["form"] == capi.DFT_FUSED and plan["m"] == dk.m_of(n, k) and plan["tpw"] == dk.tpw_of(plan["m"], count)
        for op, real in (("forward", False), ("rforward", True)):
            x = case_input("rzoom" if real else "forward", n, count)
            ref = cached(("zoom", n, k, real, count), lambda: dk.ref64("zoom", x, n, k, f0, df))
            got = run(dev, h, op, x)
            assert got.shape == (count, k)
            dk.check(got, ref, dk.bin_limit("zoom", x, n, k), dk.dense(count), f"zoom {op} n={n} k={k} rows={count}")
    h.close()


# ------------------------------------------------------------------------------------------------ 2. identities
@pytest.mark.parametrize("n", (441, 480, 2049))
def test_inverse_of_forward(dev, n):
    """forward's error is below its limit in every bin, so its inverse is below that limit in every sample; then the inverse's own"""
    h = filters.DftMC(n)
    x = case_input("forward", n, 37)
    X = run(dev, h, "forward", x)
    back = run(dev, h, "inverse", X)
    lim = dk.bin_limit("forward", x, n) + dk.bin_limit("inverse", X, n)
    worst = dk.worst_bin(back, x.astype(np.complex128), lim)
    print(f"inverse(forward) n={n}: {worst:.3g} of the sum of the two limits")
    assert worst <= 1.0
    xr = case_input("rforward", n, 37)
    Xr = run(dev, h, "rforward", xr)
    backr = run(dev, h, "rinverse", Xr)
    limr = dk.bin_limit("rforward", xr, n) + dk.bin_limit("rinverse", Xr, n)
    worst = dk.worst_bin(backr, xr.astype(np.float64), limr)
    print(f"rinverse(rforward) n={n}: {worst:.3g} of the sum of the two limits")
    assert backr.dtype == np.float32 and worst <= 1.0
    h.close()


@pytest.mark.parametrize("n", (441, 480, 2049))
def test_rforward_is_the_first_half_of_forward(dev, n):
    h = filters.DftMC(n)
    xr = case_input("rforward", n, 37)
    half = run(dev, h, "rforward", xr)
    full = run(dev, h, "forward", xr.astype(np.complex64))
    assert half.shape == (37, n // 2 + 1)
    lim = dk.bin_limit("rforward", xr, n)
    worst = dk.worst_bin(half, full[:, :n // 2 + 1].astype(np.complex128), lim)
    print(f"rforward against forward n={n}: {worst:.3g} of the per-bin limit")
    assert worst <= 2.0
    h.close()


@pytest.mark.parametrize("n", (441, 480, 2049, 4800))
def test_rinverse_drops_the_imaginary_parts_of_the_real_bins(dev, n):
    h = filters.DftMC(n)
    X = case_input("rinverse", n, 37).copy()
    X[:, 0] = X[:, 0].real
    if n % 2 == 0:
        X[:, n // 2] = X[:, n // 2].real
    clean = run(dev, h, "rinverse", X)
    planted = X.copy()
    planted[:, 0] += 1j * 1e6
    if n % 2 == 0:
        planted[:, n // 2] -= 1j * 3e5
    else:
        assert planted.shape[1] == (n + 1) // 2                 # odd n: no bin n / 2, the last bin keeps its imaginary part
    same_bits(run(dev, h, "rinverse", planted), clean, f"rinverse n={n} with planted imaginary parts")
    if n % 2:
        moved = X.copy()
        moved[:, -1] += 1j
        assert not np.array_equal(run(dev, h, "rinverse", moved), clean)
    h.close()


def test_zoom_on_the_dft_grid_is_the_dft(dev):
    n = 480
    h = filters.CztMC(n, n, 0.0, 1.0 / n)
    x = case_input("forward", n, 37)
    dk.check(run(dev, h, "forward", x), reference("forward", n, 37), dk.bin_limit("forward", x, n), dk.dense(37), "zoom as the DFT")
    h.close()


@pytest.mark.parametrize("n", (480, 2049))
def test_windows(dev, n):
    """a window of 0.5 scales every table entry exactly; a Hann window against the float64 definition and the float32 model"""
    h = filters.DftMC(n)
    plain = {op: run(dev, h, op, case_input(op, n, 3)) for op in OPS}
    h.set_window(np.full(n, 0.5, dtype=np.float32))
    for op in OPS:
        same_bits(run(dev, h, op, case_input(op, n, 3)), plain[op] * np.float32(0.5), f"{op} n={n} under a window of 0.5")
    w = np.hanning(n + 2)[1:-1].astype(np.float32)
    h.set_window(w)
    hann = {}
    for op in OPS:
        x = case_input(op, n, 3)
        got = run(dev, h, op, x)
        lim = dk.bin_limit(op, x, n, w=w)
        hann[op] = got
        dk.check(got, dk.ref64(op, x, n, w=w), lim, dk.dense(3), f"hann {op} n={n}")
        model = dk.model_f32(op, x, n, w=w)
        assert dk.worst_bin(got, model.astype(np.complex128), lim) <= 2.0
    # the window stays through a change of form and back
    h.configure(composed=True)
    for op in OPS:
        x = case_input(op, n, 3)
        dk.check(run(dev, h, op, x), dk.ref64(op, x, n, w=w), dk.bin_limit(op, x, n, w=w), dk.dense(3), f"hann composed {op} n={n}")
    h.configure()
    for op in OPS:
        same_bits(run(dev, h, op, case_input(op, n, 3)), hann[op], f"{op} n={n}: the window behind configure and back")
    h.set_window(None)
    for op in OPS:
        same_bits(run(dev, h, op, case_input(op, n, 3)), plain[op], f"{op} n={n} with the window taken off")
    h.close()
    hw = filters.DftMC(n, window=w)
    same_bits(run(dev, hw, "forward", case_input("forward", n, 3)), hann["forward"], "the window given at init")
    hw.close()


# ------------------------------------------------------------------------------------------------ 3. bit pins
def big(dev, n):
    """300 rows through one call, forward and rforward: what every pin compares with"""
    def make():
        h = filters.DftMC(n)
        x, xr = case_input("forward", n, 300), case_input("rforward", n, 300)
        out = {"x": x, "xr": xr, "forward": run(dev, h, "forward", x), "rforward": run(dev, h, "rforward", xr),
               "inverse": run(dev, h, "inverse", x)}
        h.close()
        return out
    return cached(("big", n), make)


@pytest.mark.parametrize("n", PIN_N + (2049,))
def test_bits_do_not_depend_on_count_or_position(dev, n):
    b = big(dev, n)
    h = filters.DftMC(n)
    for count in (1, 2, 3, 37, 299):
        same_bits(run(dev, h, "forward", b["x"][:count]), b["forward"][:count], f"forward n={n} count={count}")
    same_bits(run(dev, h, "inverse", b["x"][:37]), b["inverse"][:37], f"inverse n={n} count=37")
    moved = np.ascontiguousarray(b["x"][[7, 0, 299, 7, 150, 7, 36]])
    same_bits(run(dev, h, "forward", moved), b["forward"][[7, 0, 299, 7, 150, 7, 36]], f"forward n={n}, rows moved")
    h.close()


@pytest.mark.parametrize("what", ["scaled", "zeroed", "nan"])
@pytest.mark.parametrize("n", PIN_N + (2049,))
def test_neighbours(dev, n, what):
    """the rows around row 9 (and in its workgroup) scaled by 2^20, zeroed or NaN: no bit of row 9 moves; a NaN stays in its row"""
    b = big(dev, n)
    h = filters.DftMC(n)
    x = b["x"][:37].copy()
    keep = [9, 20]
    others = [r for r in range(37) if r not in keep]
    if what == "scaled":
        x[others] *= np.float32(2.0 ** 20)
    elif what == "zeroed":
        x[others] = 0
    else:
        x[8, n // 2] = np.nan
        x[10, 0] = complex(0, np.nan)
        others = [8, 10]
    got = run(dev, h, "forward", x)
    same_bits(got[keep], b["forward"][keep], f"n={n}: rows beside {what} neighbours")
    if what == "nan":
        rest = [r for r in range(37) if r not in (8, 10)]
        same_bits(got[rest], b["forward"][rest], f"n={n}: every row but the NaN rows")
        assert np.isnan(got[8]).any() and np.isnan(got[10]).any()
    if what == "zeroed":
        assert not got[others].any(), "a zero row gives exactly zero"
        zr = run(dev, h, "rinverse", np.zeros((3, n // 2 + 1), dtype=np.complex64))
        assert zr.shape == (3, n) and not zr.any()
    h.close()


@pytest.mark.parametrize("n", PIN_N + (2049,))
def test_power_of_two_scaling(dev, n):
    b = big(dev, n)
    h = filters.DftMC(n)
    for e in (7, -5):
        s = np.float32(2.0 ** e)
        same_bits(run(dev, h, "forward", b["x"][:5] * s), b["forward"][:5] * s, f"forward n={n} scaled by 2^{e}")
        same_bits(run(dev, h, "rforward", b["xr"][:5] * s), b["rforward"][:5] * s, f"rforward n={n} scaled by 2^{e}")
    h.close()


@pytest.mark.parametrize("n", PIN_N + (2049,))
def test_host_pointers_and_element_offsets(dev, n):
    b = big(dev, n)
    h = filters.DftMC(n)
    same_bits(h.forward(b["x"][:37].copy()), b["forward"][:37], f"forward n={n} on host memory")
    same_bits(h.rforward(b["xr"][:5].copy()), b["rforward"][:5], f"rforward n={n} on host memory")
    hosted = np.full((5, n + 3), 7.0 + 7.0j, dtype=np.complex64)
    h.forward(b["x"][:5].copy(), out=hosted.reshape(-1)[:4 * (n + 3) + n], out_pitch=n + 3)
    same_bits(hosted[:, :n], b["forward"][:5], "host output rows a pitch apart")
    assert np.all(hosted[:4, n:] == 7.0 + 7.0j), "the gaps between host output rows changed"
    # one complex element (8 bytes) and one float (4 bytes) past an aligned address
    xin = bc.carve_input(dev, b["x"][:5].view(np.float32), 2)
    out = bc.carve(dev, F32, 2 * 5 * n, 6)
    h.forward(xin.view, out=out.view)
    torch.cuda.synchronize()
    same_bits(bc.check_all_written(out, "forward").view(np.complex64).reshape(5, n), b["forward"][:5], "forward at element offsets")
    rin = bc.carve_input(dev, b["xr"][:5], 1)
    rout = bc.carve(dev, F32, 2 * 5 * (n // 2 + 1), 2)
    h.rforward(rin.view, out=rout.view)
    torch.cuda.synchronize()
    same_bits(bc.check_all_written(rout, "rforward").view(np.complex64).reshape(5, -1), b["rforward"][:5], "rforward at offsets")
    h.close()


@pytest.mark.parametrize("n", PIN_N + (2049,))
def test_overlapping_input_rows(dev, n):
    """rows a hop of 1 and of n / 4 apart in one signal against the same rows copied out: STFT analysis at any frame length"""
    h = filters.DftMC(n)
    rng = np.random.default_rng(n)
    for hop in (1, max(1, n // 4)):
        count = 37
        sig = rng.standard_normal((count - 1) * hop + n).astype(np.float32)
        frames = np.stack([sig[r * hop:r * hop + n] for r in range(count)])
        want = run(dev, h, "rforward", frames)
        got = h.rforward(torch.from_numpy(sig).to(dev), in_pitch=hop)
        torch.cuda.synchronize()
        same_bits(got.cpu().numpy(), want, f"rforward n={n} hop={hop}")
        csig = (sig + 1j * sig[::-1]).astype(np.complex64)
        cframes = np.stack([csig[r * hop:r * hop + n] for r in range(count)])
        cgot = h.forward(torch.from_numpy(csig).to(dev), in_pitch=hop)
        torch.cuda.synchronize()
        same_bits(cgot.cpu().numpy(), run(dev, h, "forward", cframes), f"forward n={n} hop={hop}")
    h.close()


# ------------------------------------------------------------------------------------------------ 4. buffers
ENTRY = {   # name: (zoom, input row, output row, floats per input element, floats per output element)
    "llz_dft_mc_forward": (False, lambda n, k: n, lambda n, k: n, 2, 2),
    "llz_dft_mc_inverse": (False, lambda n, k: n, lambda n, k: n, 2, 2),
    "llz_dft_mc_real_forward": (False, lambda n, k: n, lambda n, k: n // 2 + 1, 1, 2),
    "llz_dft_mc_real_inverse": (False, lambda n, k: n // 2 + 1, lambda n, k: n, 2, 1),
    "llz_czt_mc_forward": (True, lambda n, k: n, lambda n, k: k, 2, 2),
    "llz_czt_mc_real_forward": (True, lambda n, k: n, lambda n, k: k, 1, 2),
}


@pytest.mark.parametrize("name,n", [(name, n) for name in ENTRY for n in ((441,) if ENTRY[name][0] else (441, 2049))])
def test_guarded_buffers_and_refusals(dev, name, n):
    zoom, in_row, out_row, in_el, out_el = ENTRY[name]
    L = capi.lib()
    k, count = 100, 37
    h = filters.CztMC(n, k, 0.1, 1e-3) if zoom else filters.DftMC(n)
    fn = getattr(L, name)
    il, ol = in_row(n, k), out_row(n, k)
    in_pitch, out_pitch = il + 1, ol + 3
    rng = np.random.default_rng(5)
    data = rng.standard_normal(in_el * ((count - 1) * in_pitch + il)).astype(np.float32)
    xin = bc.carve_input(dev, data, in_el)                       # one element past an aligned address
    snap = bc.snapshot(xin)
    out = bc.carve(dev, F32, out_el * ((count - 1) * out_pitch + ol), 3 if out_el == 1 else 6)
    assert fn(h.handle, xin.view.data_ptr(), in_pitch, out.view.data_ptr(), out_pitch, count) == 0, capi.last_error()
    torch.cuda.synchronize()
    bc.check_untouched(xin, snap, "in")
    bc.check_bands(out, "out")
    got = np.zeros((count, out_el * out_pitch), dtype=np.uint32)
    got.reshape(-1)[:out.numel] = bc.bits(out.view)
    assert np.all(got[:-1, out_el * ol:] == bc.SENTINEL32), "the gap between output rows changed"
    assert not np.any(got[:, :out_el * ol] == bc.SENTINEL32), "an output element was never written"
    # the same rows, copied out and contiguous, give the same bits
    rows_in = np.stack([data[in_el * r * in_pitch:in_el * (r * in_pitch + il)] for r in range(count)])
    dense_in = torch.from_numpy(rows_in).to(dev)
    dense_out = torch.empty(count * ol * out_el, dtype=F32, device=dev)
    assert fn(h.handle, dense_in.data_ptr(), il, dense_out.data_ptr(), ol, count) == 0, capi.last_error()
    torch.cuda.synchronize()
    same_bits(got[:, :out_el * ol], dense_out.cpu().numpy().view(np.uint32).reshape(count, -1), f"{name} with pitches")

    def refused(in_ptr, ip, out_ptr, op, cnt, *needles):
        L.llz_hip_tune(b"no_such_override", 0)
        assert fn(h.handle, in_ptr, ip, out_ptr, op, cnt) == ERR_ARG
        msg = capi.last_error()
        assert all(s in msg for s in (name,) + needles), msg
        again = torch.empty_like(dense_out)
        assert fn(h.handle, xin.view.data_ptr(), in_pitch, again.data_ptr(), ol, count) == 0, capi.last_error()
        torch.cuda.synchronize()
        assert torch.equal(again.view(torch.int32), dense_out.view(torch.int32)), "the handle changed behind a refusal"

    keep = bc.snapshot(out)
    refused(xin.view.data_ptr(), in_pitch, out.view.data_ptr(), ol - 1, count, "out_pitch")
    refused(xin.view.data_ptr(), in_pitch, out.view.data_ptr(), out_pitch, 0, "count 0")
    refused(xin.view.data_ptr(), 0, out.view.data_ptr(), out_pitch, count, "in_pitch 0")
    other = "llz_dft_mc_forward" if zoom else "llz_czt_mc_forward"
    L.llz_hip_tune(b"no_such_override", 0)
    assert getattr(L, other)(h.handle, xin.view.data_ptr(), in_pitch, out.view.data_ptr(), out_pitch, count) == ERR_ARG
    assert other in capi.last_error() and "handle" in capi.last_error()
    # device input and output that overlap: exact alias, one element on, inside the last quarter
    span_in, span_out = xin.numel, out.numel
    for a, b_ in bc.overlap_cases(span_in, span_out, device=dev):
        a.copy_(xin.view)
        before = bc.bits(a).copy()
        refused(a.data_ptr(), in_pitch, b_.data_ptr(), out_pitch, count, "out may not overlap in")
        assert np.array_equal(bc.bits(a), before)
    assert np.array_equal(bc.snapshot(out), keep) and bc.untouched_report(xin, snap) is None
    h.close()


def test_torch_stream_and_window_ordering(dev):
    n = 480
    b = big(dev, n)
    xd = torch.from_numpy(b["x"][:37].copy()).to(dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    h = filters.DftMC(n, stream=s)
    with torch.cuda.stream(s):
        first = h.forward(xd)
        h.set_window(np.full(n, 0.5, dtype=np.float32))         # ordered on the stream behind the call in front of it
        second = h.forward(xd)
    s.synchronize()
    same_bits(first.cpu().numpy(), b["forward"][:37], "on a torch stream")
    same_bits(second.cpu().numpy(), b["forward"][:37] * np.float32(0.5), "behind set_window on the stream")
    h.close()
