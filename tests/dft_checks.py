"""Shared pieces of the DFT / zoom transform tests (test_dft_host.py, test_dft_gpu.py; include/llz_dft.h): the float64
definition, the host layer's table builder restated (tables), a float32 numpy model of the algorithm with the kernel's data
flow (model_f32: decimation-in-frequency forward passes, the product with V in image order, decimation-in-time inverse passes),
the two limits, the case table and the planted faults.  Plain numpy; nothing here opens a GPU.

Limits (u = 2^-24, |x| the 2-norm of the windowed input row):
  per bin   |X[k] - ref[k]| <= 8 u log2(M) sqrt(N + K) |x|   (inverse transforms: divided by N)
            The forward transform's error has norm <= c u log2 M sqrt(M) |a|, |V| = sqrt((N + K - 1) / M), and Cauchy-Schwarz
            over the product bounds every output of the unscaled inverse by their product; the second transform and the two chirp
            products add terms of the same order; 8 is the project's constant for transform limits.  For an inverse transform
            the input row is the spectrum (the Hermitian row of N bins for the real inverse: that is what is transformed), and
            a window, which multiplies the OUTPUT there, scales a sample's error by at most max |w|: the limit takes that factor.
  dense     |X - ref| / |ref| <= 1e-5 over a row, the project's gate, on the Gaussian rows (a tone seen through a zoom band
            that misses it has |ref| << |x|: its error is relative to |x|, which the per-bin limit holds).
"""
import ctypes as C
import ctypes.util
import math

import numpy as np

U = 2.0 ** -24
RMS_GATE = 1e-5
ROWS = (3, 37)

FUSED_N = (2, 3, 5, 7, 17, 127, 251, 441, 480, 960, 1000, 1023, 1024, 1025, 1920, 2047, 2048)
COMPOSED_N = (2049, 4800, 65537)            # 65537 on 3 rows only
FORCED_N = (7, 480, 2047)                   # the composed form forced by llz_dft_mc_configure
ZOOMS = ((1000, 64, 0.1, 1e-4), (2048, 2049, 0.0, 1.0 / 4096), (300, 3797, 0.25, 0.37 / 3797), (1, 1, 0.3, 0.1))
FAULTS = ("no_wrap", "short_m", "no_post", "natural_v", "fwd_chirp_inverse", "f32_phase")
FAULT_N = (7, 480, 2047)


def m_of(n, k):
    m = 8
    while m < n + k - 1:
        m *= 2
    return m


def tpw_of(m, count):
    return min(2048 // m if m < 2048 else 1, count)


# ------------------------------------------------------------------------------------------------ signals and the definition
def rows(n, count, seed=0, real=False):
    """row r: r % 3 == 0 Gaussian, 1 an off-bin tone, 2 an impulse at n - 1; [count, n] complex64 (float32 when real)"""
    rng = np.random.default_rng(1000 * n + count + seed)
    t = np.arange(n)
    x = np.zeros((count, n), dtype=np.complex128)
    for r in range(count):
        if r % 3 == 0:
            x[r] = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        elif r % 3 == 1:
            x[r] = (0.5 + r) * np.exp(2j * np.pi * ((n // 3) + 0.37 + 0.01 * r) * t / n)
        else:
            x[r, n - 1] = 1.0 + 0.5j * (r + 1)
    return x.real.astype(np.float32) if real else x.astype(np.complex64)


def dense(count):
    return [r for r in range(count) if r % 3 == 0]


def hermitian(bins, n):
    """the row of n bins the real inverse transforms: bins 0 .. n // 2 extended, the imaginary parts of the real bins dropped"""
    b = np.array(bins, dtype=np.complex128)
    b[..., 0] = b[..., 0].real
    if n % 2 == 0:
        b[..., n // 2] = b[..., n // 2].real
    tail = np.conj(b[..., 1:(n + 1) // 2][..., ::-1])
    return np.concatenate([b, tail], axis=-1)


def ref64(op, x, n, k=None, f0=0.0, df=0.0, w=None):
    """the float64 definition; op: forward, inverse, rforward, rinverse (numpy.fft in double), zoom (the explicit sum)"""
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    x = np.asarray(x, dtype=np.complex128 if np.iscomplexobj(x) else np.float64)
    if op == "forward":
        return np.fft.fft(x * w, axis=-1)
    if op == "rforward":
        return np.fft.fft(x * w, axis=-1)[..., :n // 2 + 1]
    if op == "inverse":
        return np.fft.ifft(x, axis=-1) * w
    if op == "rinverse":
        return np.fft.ifft(hermitian(x, n), axis=-1).real * w
    assert op == "zoom"
    t = np.arange(n, dtype=np.float64)
    ph = np.outer(f0 + np.arange(k, dtype=np.float64) * df, t)
    ph -= np.floor(ph)
    return (x * w) @ np.exp(-2j * np.pi * ph).T


# ------------------------------------------------------------------------------------------------ the tables, restated
def _turns(n, zoom, df, i):
    if not zoom:
        return float((i * i) % (2 * n)) / float(2 * n)
    t = df * float(i * i) / 2.0
    return t - math.floor(t)


_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
_libm.sincos.restype = None


def _cs(turns):
    """cos and sin of `turns` turns from libm's sincos, the call the host layer makes (its last bit is not always that of cos
    and sin called apart)"""
    s, c = C.c_double(), C.c_double()
    _libm.sincos(2 * math.pi * turns, C.byref(s), C.byref(c))
    return c.value, s.value


def _put(turns, conj, scale):
    c, s = _cs(turns)
    return np.float32(scale * c), np.float32(scale * (s if conj else -s))


def _cs_table(m):
    c = np.array([0.0 if i in (m // 4, 3 * m // 4) else math.cos(2.0 * math.pi * i / m) for i in range(m)])
    s = np.array([0.0 if i in (0, m // 2) else math.sin(2.0 * math.pi * i / m) for i in range(m)])
    return c, s


def bitrev(m):
    bits = m.bit_length() - 1
    e = np.arange(m)
    b = np.zeros(m, dtype=np.int64)
    for q in range(bits):
        b |= ((e >> q) & 1) << (bits - 1 - q)
    return b


def _dif64(zr, zi, m):
    """the host layer's double transform (llz_host_dif_f64), its products and sums in its order: entry e = bin bitrev(e)"""
    c, s = _cs_table(m)
    span = m
    while span >= 2:
        half, step = span // 2, m // span
        wr, wi = c[::step][:half], -s[::step][:half]
        ar, ai = zr.reshape(-1, span)[:, :half], zi.reshape(-1, span)[:, :half]
        br, bi = zr.reshape(-1, span)[:, half:], zi.reshape(-1, span)[:, half:]
        dr, di = ar - br, ai - bi
        ar += br
        ai += bi
        br[...] = dr * wr - di * wi
        bi[...] = dr * wi + di * wr
        span //= 2
    return zr, zi


def tables(n, k, zoom=False, f0=0.0, df=0.0, inverse=False, natural=False, w=None, m=None, wrap=True):
    """(pre [n], v [m], post [k]) complex64 as llz_host_dft_tables builds them, bit for bit: phases in turns from exact integer
    reduction (DFT) or the fractional part in double (zoom), libm's sincos, every entry rounded to float once.  m, wrap:
    for the planted faults only"""
    m = m_of(n, k) if m is None else m
    pre = np.zeros(n, dtype=np.complex64)
    post = np.zeros(k, dtype=np.complex64)
    for i in range(n):
        turns = _turns(n, zoom, df, i)
        if zoom:
            u = f0 * float(i)
            turns += u - math.floor(u)
            turns -= math.floor(turns)
        re, im = _put(turns, inverse, float(w[i]) if (w is not None and not inverse) else 1.0)
        pre[i] = complex(re, im)
    for j in range(k):
        scale = (float(w[j]) if w is not None else 1.0) / float(n) if inverse else 1.0
        re, im = _put(_turns(n, zoom, df, j), inverse, scale)
        post[j] = complex(re, im)
    zr, zi = np.zeros(m), np.zeros(m)
    for i in range(max(k, n)):
        c, s = _cs(_turns(n, zoom, df, i))
        s = -s if inverse else s
        if i < k:
            zr[i % m], zi[i % m] = c, s
        if wrap and 1 <= i < n:
            zr[(m - i) % m], zi[(m - i) % m] = c, s
    zr, zi = _dif64(zr, zi, m)
    v = np.zeros(m, dtype=np.complex64)
    if natural:
        b = bitrev(m)
        v.real[b] = zr.astype(np.float32)
        v.imag[b] = zi.astype(np.float32)
    else:
        v.real = (zr / m).astype(np.float32)
        v.imag = (zi / m).astype(np.float32)
    return pre, v, post


def tables_f32_phase(n):
    """the planted fault: phases from a float32 pi i^2 / n"""
    i = np.arange(n, dtype=np.float32)
    ang = (np.float32(np.pi) * (i * i) / np.float32(n)).astype(np.float64)
    c = (np.cos(ang) - 1j * np.sin(ang)).astype(np.complex64)
    m = m_of(n, n)
    z = np.zeros(m, dtype=np.complex128)
    z[:n] = np.conj(c)
    z[m - n + 1:] = np.conj(c[1:][::-1])
    v = (np.fft.fft(z) / m)[bitrev(m)].astype(np.complex64)
    return c, v, c


# ------------------------------------------------------------------------------------------------ the float32 model
def _tw32(m):
    ang = 2.0 * np.pi * np.arange(m // 2) / m
    return (np.cos(ang) - 1j * np.sin(ang)).astype(np.complex64)


def fft_dif32(a):
    """[rows, m] complex64, radix-2 decimation in frequency in float32: natural in, entry e = bin bitrev(e) out"""
    a = a.copy()
    m = a.shape[-1]
    tw = _tw32(m)
    span = m
    while span >= 2:
        half = span // 2
        z = a.reshape(a.shape[0], -1, span)
        lo, hi = z[..., :half].copy(), z[..., half:].copy()
        z[..., :half] = lo + hi
        z[..., half:] = (lo - hi) * tw[::m // span][:half]
        span //= 2
    return a


def ifft_dit32(a):
    """the unscaled inverse by decimation in time: entry e = bin bitrev(e) in, natural out"""
    a = a.copy()
    m = a.shape[-1]
    tw = np.conj(_tw32(m))
    span = 2
    while span <= m:
        half = span // 2
        z = a.reshape(a.shape[0], -1, span)
        lo, hi = z[..., :half].copy(), z[..., half:] * tw[::m // span][:half]
        z[..., :half] = lo + hi
        z[..., half:] = lo - hi
        span *= 2
    return a


def model_f32(op, x, n, k=None, f0=0.0, df=0.0, w=None, fault=None):
    """the algorithm in float32 with the kernel's data flow; x: [rows, n] (rinverse: [rows, n // 2 + 1])"""
    zoom = op == "zoom"
    inverse = op in ("inverse", "rinverse")
    k = n if not zoom else k
    m = m_of(n, k)
    if fault == "short_m":
        m = 8
        while m < n:
            m *= 2
    if fault == "f32_phase":
        pre, v, post = tables_f32_phase(n)
    else:
        pre, v, post = tables(n, k, zoom, f0, df, inverse and fault != "fwd_chirp_inverse", False, w, m, fault != "no_wrap")
        if fault == "natural_v":
            nat = np.empty_like(v)
            nat[bitrev(m)] = v
            v = nat
        if fault == "fwd_chirp_inverse":
            post = (post.astype(np.complex128) / n).astype(np.complex64)
    x = np.asarray(x)
    if op == "rinverse":
        x = hermitian(x, n)
    a = np.zeros((x.shape[0], m), dtype=np.complex64)
    a[:, :n] = x.astype(np.complex64) * pre
    big = fft_dif32(a) * v
    b = ifft_dit32(big)[:, :k]
    out = b if fault == "no_post" else b * post
    if op == "rforward":
        return out[:, :n // 2 + 1]
    return out.real.copy() if op == "rinverse" else out


# ------------------------------------------------------------------------------------------------ the limits
def input_norm(op, x, n, w=None):
    """|x| of the limit, per row"""
    x = np.asarray(x)
    if op == "rinverse":
        x = hermitian(x, n)
    x = x.astype(np.complex128)
    if op in ("inverse", "rinverse"):
        return np.linalg.norm(x, axis=-1) * (1.0 if w is None else float(np.max(np.abs(w))))
    return np.linalg.norm(x if w is None else x * np.asarray(w, dtype=np.float64), axis=-1)


def bin_limit(op, x, n, k=None, w=None):
    k = n if k is None else k
    lim = 8 * U * math.log2(m_of(n, k)) * math.sqrt(n + k) * input_norm(op, x, n, w)
    return lim / n if op in ("inverse", "rinverse") else lim


def worst_bin(got, ref, lim):
    """the worst |got - ref| over its row's limit; a zero row has the limit 0, which no error at all meets"""
    err = np.abs(np.asarray(got).astype(np.complex128) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(lim[:, None] > 0, err / lim[:, None], np.where(err > 0, np.inf, 0.0))))


def ratios(got, ref, lim, dense_rows):
    """(worst |got - ref| over its row's per-bin limit, worst relative RMS error of the dense rows over the gate)"""
    err = np.abs(np.asarray(got).astype(np.complex128) - ref)
    per_bin = worst_bin(got, ref, lim)
    rms = 0.0
    for r in dense_rows:
        rms = max(rms, float(np.linalg.norm(err[r]) / np.linalg.norm(ref[r])))
    return per_bin, rms / RMS_GATE


def check(got, ref, lim, dense_rows, label):
    per_bin, rms = ratios(got, ref, lim, dense_rows)
    print(f"{label}: worst bin at {per_bin:.3g} of its limit, dense rows at {rms:.3g} of the RMS gate")
    assert np.isfinite(np.asarray(got)).all(), label
    assert per_bin <= 1.0 and rms <= 1.0, (label, per_bin, rms)
    return per_bin, rms
