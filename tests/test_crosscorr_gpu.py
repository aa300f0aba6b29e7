"""The batched cross-correlation on the MI355X: llz_crosscorr_mc (direct form, one- and two-sided), llz_corr_cof_mc and the FFT
form llz_crosscorr_fast_mc, against the oracle's llz_crosscorr / llz_corr_cof in double.  The reference row of a two-sided
call is ref[f, p+k] = crosscorr(x_f, y_f, p)[k], ref[f, p-k] = crosscorr(y_f, x_f, p)[k].

  1. exact: integer-valued rows in [-8, 8] -- every partial sum is an integer of magnitude <= 64 n <= 2^24, so float32 holds it in
     any order and the result equals the oracle's bit for bit; single +-1 rows put the one non-zero lag on both sides of every
     chunk edge (512 for the LDS window, 8 (64 - NL) for the register form);
  2. float parity under llz_autocorr_mc's gate, 1e-5 of sqrt(sum x^2 sum y^2), and the planted delay found in every frame;
  3. ties: the bits of llz_autocorr_mc for y = x, reversal, host / device / mixed pointers;
  4. llz_corr_cof_mc; 5. the FFT form; 6. the buffer contract with guarded buffers (tests/buffer_checks.py)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from llzlab_amd import capi, filters  # noqa: E402
from tests import buffer_checks as bc  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG = -1
F32 = torch.float32

# (frames, n, p): every path and edge of the autocorrelation's list (test_gpu_parity.py) -- the register form with 1..4
# neighbours, lengths that are no multiple of 8, shorter than a chunk, exactly one chunk, p = 0; the LDS window with 1..8 lag
# groups, 64 lags per launch (63 / 64 / 65), four launches (255), many chunks
SHAPES = [(9, 1021, 0), (300, 1000, 7), (33, 496, 8), (5, 497, 9), (1000, 480, 16), (4, 3001, 17),
          (6, 61, 24), (40, 2048, 25), (3, 10, 9), (2, 4096, 32),
          (7, 300, 40), (2, 64, 63), (3, 600, 64), (3, 600, 65), (3, 513, 128), (130, 512, 255), (5, 20000, 40)]
TUNES = [{}, {"acf_lds": 1}]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    capi.build()
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    return torch.device("cuda:0")


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def two_sided_ref(oracle, x, y, p):
    """[frames, 2p+1] in double from the float32 rows"""
    ref = np.zeros((x.shape[0], 2 * p + 1))
    for f in range(x.shape[0]):
        xf, yf = x[f].astype(np.float64), y[f].astype(np.float64)
        ref[f, p:] = oracle.crosscorr(xf, yf, p)
        ref[f, :p + 1] = oracle.crosscorr(yf, xf, p)[::-1]            # (lag 0 is the same sum either way)
    return ref


_CACHE = {}


def cached(key, make):
    """inputs and oracle rows of a case: computed once, shared by the tests that need them, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def run_direct(dev, x, y, p, two_sided, tune=None):
    frames = x.shape[0]
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    r = torch.full((frames, 2 * p + 1 if two_sided else p + 1), float("nan"), dtype=F32, device=dev)
    with capi.tuned(**(tune or {})):
        filters.crosscorr_mc(xd, yd, r, p, two_sided=two_sided)
    return r.cpu().numpy()


# ================================================================================================ 1. exact
def integer_case(oracle, frames, n, p):
    def make():
        rng = np.random.default_rng(7919 * frames + 31 * n + p)
        x = rng.integers(-8, 9, (frames, n)).astype(np.float32)
        y = rng.integers(-8, 9, (frames, n)).astype(np.float32)
        return x, y, two_sided_ref(oracle, x, y, p)
    return cached(("int", frames, n, p), make)


@pytest.mark.parametrize("frames,n,p", SHAPES)
def test_crosscorr_mc_exact_on_integers(dev, oracle, frames, n, p):
    assert 64 * n <= 1 << 24
    x, y, ref = integer_case(oracle, frames, n, p)
    want2 = ref.astype(np.float32)
    assert np.array_equal(want2.astype(np.float64), ref)                # the oracle's values are float32 numbers
    for tune in TUNES if p <= 32 else TUNES[:1]:
        got2 = run_direct(dev, x, y, p, True, tune)
        bad = np.argwhere(bits(got2) != bits(want2))
        assert bad.size == 0, f"two-sided {tune}: {len(bad)} differ, the first at frame {bad[0][0]} lag {bad[0][1] - p}"
        got1 = run_direct(dev, x, y, p, False, tune)
        bad = np.argwhere(bits(got1) != bits(want2[:, p:]))
        assert bad.size == 0, f"one-sided {tune}: {len(bad)} differ, the first at frame {bad[0][0]} lag {bad[0][1]}"


def impulse_rows(n, p):
    """rows (position in x, sign of x, lag k, sign of y): x is a single +-1 at `position`, y a single +-1 at position + k"""
    nl = (1 if p <= 8 else (p + 7) // 8) if p <= 32 else None
    spots = {0, n - 1, 511, 512}
    if nl:
        spots |= {8 * (64 - nl) - 1, 8 * (64 - nl)}
    lags = sorted({s * min(p, k) for k in (0, 1, 8, 9, 64, p // 2, p) for s in (1, -1)})
    rows = []
    for pos in sorted(s for s in spots if 0 <= s < n):
        for k in lags:
            if 0 <= pos + k < n:
                rows.append((pos, 1 if (pos + k) % 2 else -1, k, 1 if pos % 3 else -1))
    return rows


@pytest.mark.parametrize("n,p", sorted({(n, p) for _f, n, p in SHAPES}))
def test_crosscorr_mc_exact_on_single_impulses(dev, oracle, n, p):
    def make():
        rows = impulse_rows(n, p)
        x, y = np.zeros((len(rows), n), dtype=np.float32), np.zeros((len(rows), n), dtype=np.float32)
        for f, (pos, sx, k, sy) in enumerate(rows):
            x[f, pos], y[f, pos + k] = sx, sy
        return rows, x, y, two_sided_ref(oracle, x, y, p)
    rows, x, y, ref = cached(("imp", n, p), make)
    known = np.zeros_like(ref)
    for f, (pos, sx, k, sy) in enumerate(rows):
        known[f, p + k] = sx * sy
    assert np.array_equal(ref, known)                                   # the only non-zero lag is the known one
    for tune in TUNES if p <= 32 else TUNES[:1]:
        got = run_direct(dev, x, y, p, True, tune)
        bad = np.argwhere(bits(got) != bits(known))
        assert bad.size == 0, (f"{tune}: {len(bad)} differ, the first: x[{rows[bad[0][0]][0]}] against lag {rows[bad[0][0]][2]} "
                               f"shows {got[tuple(bad[0])]} at lag {bad[0][1] - p}")
        got1 = run_direct(dev, x, y, p, False, tune)
        assert np.array_equal(bits(got1), bits(known[:, p:])), tune


# ================================================================================================ 2. float parity
def delays(frames, n, p, rng):
    """a delay per frame in -p..p whose side differs from frame to frame.  A delay of d leaves n - |d| overlapping samples to
    the peak while every other lag sums about sqrt(n) products of independent samples, so |d| stays within n / 4 (which cuts
    only the shapes with p > n / 4): the peak is real in the reference itself, which the test asserts first."""
    cap = min(p, n // 4)
    d = rng.integers(0, cap + 1, frames)
    d[0] = cap                                                          # the largest delay on both sides
    if frames > 1:
        d[1] = cap
    return d * np.where(np.arange(frames) % 2 == 0, 1, -1)


def float_case(oracle, frames, n, p):
    def make():
        rng = np.random.default_rng(104729 * frames + 17 * n + p)
        x = oracle.synth_f32(frames, n, seed=n + p)
        noise = oracle.synth_f32(frames, n, seed=n + p + 100003)        # independent rows, a quarter of the amplitude
        d = delays(frames, n, p, rng)
        y = np.zeros_like(x)
        for f in range(frames):                                          # y[i] = x[i - d]: the peak of r sits at lag d
            if d[f] >= 0:
                y[f, d[f]:] = x[f, :n - d[f]]
            else:
                y[f, :n + d[f]] = x[f, -d[f]:]
        y = (y + np.float32(0.25) * noise).astype(np.float32)
        return x, y, d, two_sided_ref(oracle, x, y, p)
    return cached(("flt", frames, n, p), make)


def gate(x, y):
    """1e-5 of sqrt(sum x^2 sum y^2) per frame: llz_autocorr_mc's gate (1e-5 of the zero-lag energy), which this is for y = x"""
    x, y = x.astype(np.float64), y.astype(np.float64)
    return 1e-5 * np.sqrt((x * x).sum(axis=1) * (y * y).sum(axis=1))[:, None]


@pytest.mark.parametrize("frames,n,p", SHAPES)
def test_crosscorr_mc_float_parity_and_peak(dev, oracle, frames, n, p):
    x, y, d, ref = float_case(oracle, frames, n, p)
    assert np.array_equal(ref.argmax(axis=1) - p, d), "the planted delay is no peak of the reference: the test's data is wrong"
    lim = gate(x, y)
    for tune in TUNES if p <= 32 else TUNES[:1]:
        got2 = run_direct(dev, x, y, p, True, tune).astype(np.float64)
        got1 = run_direct(dev, x, y, p, False, tune).astype(np.float64)
        worst2, worst1 = np.max(np.abs(got2 - ref) / lim), np.max(np.abs(got1 - ref[:, p:]) / lim)
        print(f"crosscorr_mc {frames} x {n} p={p} {tune}: worst error / limit two-sided {worst2:.3g}, one-sided {worst1:.3g}")
        assert worst2 <= 1.0 and worst1 <= 1.0, (tune, worst2, worst1)
        assert np.array_equal(got2.argmax(axis=1) - p, d), tune
        assert np.array_equal(bits(got1), bits(got2[:, p:])), tune       # one kernel, two layouts


# ================================================================================================ 3. ties
@pytest.mark.parametrize("p", [0, 8, 16, 32, 40, 255])
def test_crosscorr_of_x_with_itself_is_autocorr_mc_bit_for_bit(dev, oracle, p):
    frames, n = 9, 1021
    x = oracle.synth_f32(frames, n, seed=5)
    xd = torch.from_numpy(x).to(dev)
    twin = xd.clone()                                                    # the same samples at another address: the two-row kernels
    for tune in TUNES:
        with capi.tuned(**tune):
            auto = torch.empty(frames, p + 1, dtype=F32, device=dev)
            filters.autocorr_mc(xd, auto, p)
            same = torch.full_like(auto, float("nan"))
            filters.crosscorr_mc(xd, xd, same, p)
            other = torch.full_like(auto, float("nan"))
            filters.crosscorr_mc(xd, twin, other, p)
            both = torch.full((frames, 2 * p + 1), float("nan"), dtype=F32, device=dev)
            filters.crosscorr_mc(xd, twin, both, p, two_sided=True)
        assert np.array_equal(bits(same), bits(auto)), (p, tune)
        assert np.array_equal(bits(other), bits(auto)), (p, tune, "x and a copy of x")
        assert np.array_equal(bits(both[:, p:]), bits(auto)), (p, tune)
        assert np.array_equal(bits(both[:, :p + 1].flip(1)), bits(auto)), (p, tune, "negative lags")


@pytest.mark.parametrize("frames,n,p", [(5, 497, 9), (4, 3001, 17), (2, 4096, 32), (3, 600, 65), (130, 512, 255)])
def test_crosscorr_mc_reversal_and_pointer_kinds(dev, oracle, frames, n, p):
    x, y, _d, _ref = float_case(oracle, frames, n, p)
    for tune in TUNES if p <= 32 else TUNES[:1]:
        xy = run_direct(dev, x, y, p, True, tune)
        yx = run_direct(dev, y, x, p, True, tune)
        assert np.array_equal(bits(xy), bits(yx[:, ::-1])), tune
    for two in (False, True):
        want = run_direct(dev, x, y, p, two)
        r = np.full_like(want, np.nan)
        filters.crosscorr_mc(x, y, r, p, two_sided=two)                  # host pointers
        assert np.array_equal(bits(r), bits(want)), two
        rd = torch.full(want.shape, float("nan"), dtype=F32, device=dev)
        filters.crosscorr_mc(x, torch.from_numpy(y).to(dev), rd, p, two_sided=two)       # x on the host, y and r on the device
        assert np.array_equal(bits(rd), bits(want)), two
        r = np.full_like(want, np.nan)
        filters.crosscorr_mc(torch.from_numpy(x).to(dev), y, r, p, two_sided=two)
        assert np.array_equal(bits(r), bits(want)), two


# ================================================================================================ 4. corr_cof_mc
COF_SHAPES = [(1, 1), (7, 300), (5, 497), (130, 512), (3, 20000)]


def run_cof(dev, a, b, host=False):
    if host:
        c = np.full(a.shape[0], 7.0, dtype=np.float32)
        return filters.corr_cof_mc(a, b, c)
    c = torch.full((a.shape[0],), 7.0, dtype=F32, device=dev)
    filters.corr_cof_mc(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), c)
    return c.cpu().numpy()


@pytest.mark.parametrize("kind", ["random", "same", "negated"])
@pytest.mark.parametrize("frames,n", COF_SHAPES)
def test_corr_cof_mc_integer_rows_within_one_ulp(dev, oracle, frames, n, kind):
    rng = np.random.default_rng(frames * 1000 + n)
    a = rng.integers(-8, 9, (frames, n)).astype(np.float32)
    a[:, 0] = np.where(np.abs(a).sum(axis=1) == 0, 1, a[:, 0])          # no silent row here
    b = {"same": a, "negated": -a}.get(kind)
    if b is None:
        b = rng.integers(-8, 9, (frames, n)).astype(np.float32)
        b[:, 0] = np.where(np.abs(b).sum(axis=1) == 0, 1, b[:, 0])
    b = np.ascontiguousarray(b)
    want = np.array([np.float32(oracle.corr_cof(a[f].astype(np.float64), b[f].astype(np.float64))) for f in range(frames)])
    if kind != "random":
        assert np.array_equal(want, np.full(frames, 1 if kind == "same" else -1, dtype=np.float32))
    got = run_cof(dev, a, b)
    ulps = np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64))
    print(f"corr_cof_mc {frames} x {n} {kind}: {'bit-equal' if ulps.max() == 0 else f'{ulps.max()} ulp off'}")
    assert ulps.max() <= 1, (got, want)
    assert np.array_equal(bits(run_cof(dev, a, b, host=True)), bits(got))


@pytest.mark.parametrize("frames,n", COF_SHAPES)
def test_corr_cof_mc_float_rows(dev, oracle, frames, n):
    a = oracle.synth_f32(frames, n, seed=n)
    b = (np.float32(0.5) * a + np.float32(0.5) * oracle.synth_f32(frames, n, seed=n + 77)).astype(np.float32)
    want = np.array([oracle.corr_cof(a[f].astype(np.float64), b[f].astype(np.float64)) for f in range(frames)])
    got = run_cof(dev, a, b).astype(np.float64)
    print(f"corr_cof_mc {frames} x {n}: worst error {np.max(np.abs(got - want)):.3g} (limit 3e-5)")
    assert np.max(np.abs(got - want)) <= 3e-5


def test_corr_cof_mc_silent_row_gives_nan_in_its_frame_only(dev, oracle):
    frames, n = 7, 300
    a = oracle.synth_f32(frames, n, seed=11)
    b = oracle.synth_f32(frames, n, seed=12)
    whole = run_cof(dev, a, b)
    assert np.isfinite(whole).all()
    for silent_in in ("a", "b"):
        a2, b2 = a.copy(), b.copy()
        (a2 if silent_in == "a" else b2)[3] = 0
        got = run_cof(dev, a2, b2)
        assert np.isnan(got[3]), got
        keep = np.arange(frames) != 3
        assert np.array_equal(bits(got[keep]), bits(whole[keep]))


# ================================================================================================ 5. the FFT form
FAST = [(4, 4, 3), (50, 64, 20), (9, 33, 32), (40, 200, 33), (7, 300, 299), (300, 256, 16),
        (3, 513, 200), (6, 1000, 999), (3, 1024, 32), (5, 1025, 16), (2, 2048, 2047), (4, 1500, 0),
        # 8200 frames of fft_len 4096 are 257 MiB of spectra: the 256 MiB scratch slab (8192 frames) is walked twice
        (8200, 1025, 16)]


def fast_case(oracle, frames, n, p):
    """rows as in 2 (a delayed copy plus noise), eight unique ones tiled where there are many"""
    def make():
        uniq = frames if frames <= 1000 else 8
        rng = np.random.default_rng(n + p)
        x = oracle.synth_f32(uniq, n, seed=n)
        y = np.stack([np.roll(x[f], int(rng.integers(-p, p + 1))) for f in range(uniq)])
        y = (y + np.float32(0.25) * oracle.synth_f32(uniq, n, seed=n + 9)).astype(np.float32)
        return x, y, two_sided_ref(oracle, x, y, p)
    return cached(("fast", frames if frames <= 1000 else 8, n, p), make)


@pytest.mark.parametrize("frames,n,p", FAST)
def test_crosscorr_fast_mc_vs_oracle(dev, oracle, frames, n, p):
    xu, yu, ref_u = fast_case(oracle, frames, n, p)
    reps = frames // len(xu)
    assert reps * len(xu) == frames
    x, y = np.tile(xu, (reps, 1)), np.tile(yu, (reps, 1))
    lim_u = gate(xu, yu)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    f = filters.CrosscorrFastMC(frames, n)
    for two in (True, False):
        ref = ref_u if two else ref_u[:, p:]
        r = torch.full((frames, ref.shape[1]), float("nan"), dtype=F32, device=dev)
        f.run(xd, yd, r, p, two_sided=two)
        got = r.cpu().numpy().astype(np.float64).reshape(reps, len(xu), -1)
        worst = np.max(np.abs(got - ref[None]) / lim_u[None])
        print(f"crosscorr_fast_mc {frames} x {n} p={p} two_sided={two}: worst error / limit {worst:.3g}")
        assert worst <= 1.0, (two, worst)
        if p <= 255 and frames <= 1000:                                   # the direct form agrees within twice the gate
            direct = run_direct(dev, x, y, p, two).astype(np.float64)
            assert np.max(np.abs(got[0] - direct) / lim_u) <= 2.0, two
        if frames <= 50:                                                  # host pointers: staged, the same bits
            rh = np.full((frames, ref.shape[1]), np.nan, dtype=np.float32)
            f.run(x, y, rh, p, two_sided=two)
            assert np.array_equal(bits(rh), bits(r)), two
    f.close()


def test_crosscorr_fast_mc_refuses_bad_p_and_foreign_handles(dev):
    L = capi.lib()
    frames, n = 4, 300
    x = torch.ones(frames, n, dtype=F32, device=dev)
    r = torch.full((frames, 2 * n + 1), 7.0, dtype=F32, device=dev)
    f = filters.CrosscorrFastMC(frames, n)
    for p, two in ((n, 0), (n + 1, 1), (-1, 0), (3, 2)):
        assert L.llz_crosscorr_fast_mc(f.handle, x.data_ptr(), x.data_ptr(), r.data_ptr(), p, two) == ERR_ARG
        assert "llz_crosscorr_fast_mc" in capi.last_error()
    g = filters.AutocorrFastMC(frames, n)
    assert L.llz_crosscorr_fast_mc(g.handle, x.data_ptr(), x.data_ptr(), r.data_ptr(), 3, 0) == ERR_ARG
    assert "llz_crosscorr_fast_mc" in capi.last_error()
    assert L.llz_autocorr_fast_mc(f.handle, x.data_ptr(), r.data_ptr(), 3) == ERR_ARG
    g.close()
    f.close()
    torch.cuda.synchronize()
    assert (r == 7.0).all()


# ================================================================================================ 6. buffer contract
OFFS = [(0, 0), (1, 1), (3, 3), (1, 3)]                                 # (inputs, output) element offsets from an aligned address
CONTRACT = [(7, 300, 16), (8, 512, 70), (7, 512, 16), (8, 300, 70)]     # a partial and a full last workgroup of 4 waves


class Io:
    """the guarded buffers of one call: inputs between NaN bands, the output and its bands holding the sentinel"""

    def __init__(self, dev, off):
        self.dev, self.off, self.ins, self.outs = dev, off, [], []

    def inp(self, data):
        buf = bc.carve_input(self.dev, data, self.off[0])
        self.ins.append((buf, bc.snapshot(buf)))
        return buf.shaped(*np.shape(data))

    def out(self, *shape):
        buf = bc.carve(self.dev, F32, int(np.prod(shape)), self.off[1])
        self.outs.append(buf)
        return buf.shaped(*shape)

    def verify(self, what):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                            # a faulted device serves no later test either: end the session here
            pytest.exit(f"{what}: the device reported an error, nothing more is run on it: {e}", returncode=3)
        for k, buf in enumerate(self.outs):
            bc.check_bands(buf, f"{what}: output {k}")
            bc.check_all_written(buf, f"{what}: output {k}")
        for k, (buf, snap) in enumerate(self.ins):
            bc.check_untouched(buf, snap, f"{what}: input {k}")


@pytest.mark.parametrize("off", OFFS, ids=lambda o: f"in{o[0]}-out{o[1]}")
@pytest.mark.parametrize("frames,n,p", CONTRACT)
def test_guarded_crosscorr_mc(dev, oracle, frames, n, p, off):
    x, y, ref = integer_case(oracle, frames, n, p)                       # exact: a NaN or a sample of the next frame would show
    for tune in TUNES if p <= 32 else TUNES[:1]:
        for two in (True, False):
            io = Io(dev, off)
            r = io.out(frames, 2 * p + 1 if two else p + 1)
            with capi.tuned(**tune):
                filters.crosscorr_mc(io.inp(x), io.inp(y), r, p, two_sided=two)
            io.verify(f"crosscorr_mc two_sided={two} {tune}")
            want = (ref if two else ref[:, p:]).astype(np.float32)
            assert np.array_equal(bits(r), bits(want)), (two, tune)


@pytest.mark.parametrize("off", OFFS, ids=lambda o: f"in{o[0]}-out{o[1]}")
@pytest.mark.parametrize("frames,n", [(7, 300), (8, 512)])
def test_guarded_corr_cof_mc(dev, oracle, frames, n, off):
    x, y, _ref = integer_case(oracle, frames, n, 16)
    want = np.array([np.float32(oracle.corr_cof(x[f].astype(np.float64), y[f].astype(np.float64))) for f in range(frames)])
    io = Io(dev, off)
    c = io.out(frames)
    filters.corr_cof_mc(io.inp(x), io.inp(y), c)
    io.verify("corr_cof_mc")
    assert np.max(np.abs(bits(c).astype(np.int64) - bits(want).astype(np.int64))) <= 1


@pytest.mark.parametrize("off", OFFS, ids=lambda o: f"in{o[0]}-out{o[1]}")
@pytest.mark.parametrize("frames,n,p", CONTRACT)
def test_guarded_crosscorr_fast_mc(dev, oracle, frames, n, p, off):
    x, y, _d, ref = float_case(oracle, frames, n, p)
    f = filters.CrosscorrFastMC(frames, n)
    for two in (True, False):
        io = Io(dev, off)
        r = io.out(frames, 2 * p + 1 if two else p + 1)
        f.run(io.inp(x), io.inp(y), r, p, two_sided=two)
        io.verify(f"crosscorr_fast_mc two_sided={two}")
        got = r.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - (ref if two else ref[:, p:])) <= gate(x, y)), two
    f.close()


def dptr(t):
    return C.c_void_p(t.data_ptr())


def refused(pairs, call, name, others=()):
    """every (in, out) pair of overlap_cases is refused by `call` with the overlap message, and in, out and the `others` buffers
    are bit-unchanged afterwards (nothing was staged or launched)"""
    for k, (a, b) in enumerate(pairs):
        before = [bc.bits(t).copy() for t in (a, b) + tuple(others)]
        rc, msg = call(a, b), capi.last_error()
        assert rc == ERR_ARG and name in msg and "may not overlap" in msg and "(device memory)" in msg, (k, rc, msg)
        torch.cuda.synchronize()
        for t, was in zip((a, b) + tuple(others), before):
            assert np.array_equal(bc.bits(t), was), f"{name}: case {k} changed a buffer it refused"


def test_output_overlapping_an_input_is_refused_and_x_overlapping_y_is_not(dev, oracle):
    L = capi.lib()
    frames, n, p = 7, 300, 16
    spare = bc.carve(dev, F32, frames * n, 0, guard=64).view
    fast = filters.CrosscorrFastMC(frames, n)
    for two in (0, 1):
        width = 2 * p + 1 if two else p + 1
        for name, call in (
                ("llz_crosscorr_mc", lambda xp, yp, rp: L.llz_crosscorr_mc(xp, yp, rp, frames, n, p, two, None)),
                ("llz_crosscorr_fast_mc", lambda xp, yp, rp: L.llz_crosscorr_fast_mc(fast.handle, xp, yp, rp, p, two))):
            refused(bc.overlap_cases(frames * n, frames * width, device=dev),
                    lambda a, b: call(dptr(a), dptr(spare), dptr(b)), name, (spare,))            # r over x
            refused(bc.overlap_cases(frames * n, frames * width, device=dev),
                    lambda a, b: call(dptr(spare), dptr(a), dptr(b)), name, (spare,))            # r over y
    fast.close()
    refused(bc.overlap_cases(frames * n, frames, device=dev),
            lambda a, b: L.llz_corr_cof_mc(dptr(a), dptr(spare), dptr(b), frames, n, None), "llz_corr_cof_mc", (spare,))
    refused(bc.overlap_cases(frames * n, frames, device=dev),
            lambda a, b: L.llz_corr_cof_mc(dptr(spare), dptr(a), dptr(b), frames, n, None), "llz_corr_cof_mc", (spare,))
    # x and y are both only read: rows that overlap (y starts one sample into x) are accepted and computed as what they hold
    rng = np.random.default_rng(3)
    flat = rng.integers(-8, 9, frames * n + 1).astype(np.float32)
    fd = torch.from_numpy(flat).to(dev)
    xd, yd = fd[:frames * n].view(frames, n), fd[1:].view(frames, n)
    r = torch.full((frames, 2 * p + 1), float("nan"), dtype=F32, device=dev)
    filters.crosscorr_mc(xd, yd, r, p, two_sided=True)
    want = two_sided_ref(oracle, flat[:-1].reshape(frames, n), flat[1:].reshape(frames, n), p).astype(np.float32)
    assert np.array_equal(bits(r), bits(want))
