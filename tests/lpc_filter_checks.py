"""Shared pieces of the LPC filter tests (test_lpc_filter_host.py, test_lpc_filter_gpu.py): numpy models of the two filters of
include/llz_lpc.h part 3, the coefficient families, the cases and the limits.  Plain numpy: nothing here opens a GPU.

Models
  residual64   e[t] = x[t] + sum_k a_f[k] x[t-k], summed in float64 from the float32 inputs (the reference of the limit)
  S            S_t = |x[t]| + sum_k |a_f[k] x[t-k]|
  residual32   the same sum in float32, UNFUSED (a rounded product, then a rounded add; k = p .. 1): the device's place in
               the CPU suite
  synth_model  the pinned double recursion of llz_lpc_synth_mc: acc = (double) e[t]; k = p .. 1: acc = acc - a_f[k] * yd[t-k]
               as a separate `*` and `-` in float64; numpy reproduces it bit for bit.  Returns the unrounded doubles.

Limits (derived; u = 2^-24)
  residual     |e - residual64| <= 2 (p + 1) u S_t per sample.  The fused chain rounds p times, each by at most u times the
               partial sum's magnitude <= S_t (1 + u)^p: p u S_t to first order; the unfused model rounds 2 p times: 2 p u S_t;
               residual64's own error (2^-53 scale) is far below either.  2 (p + 1) covers both.  Where a_f[1..p] = 0 the bits
               are x's.
  synthesis    bits of float32(synth_model)
  round trip   synth(residual(x)) = x + g * d, d the residual's error, g the float64 impulse response of 1 / A:
               |.. - x|[t] <= sum_j |g[j]| max_t (2 (p + 1) u S_t) + 1.01 u |x[t]| (the store's rounding)
"""
import functools

import numpy as np

U = 2.0 ** -24
ORDER_MAX = 64
CHANNELS = (1, 3, 37, 130)
ORDERS = (0, 1, 2, 7, 8, 9, 16, 17, 32, 33, 64)


def frame_lens(p):
    """the least allowed, lengths that are no multiple of the 16-sample block, one that is no multiple of a 16-byte access"""
    return sorted({p + 1, 50, 160, 1023} - set(range(p + 1)))


def _cases():
    out = []
    for i, p in enumerate(ORDERS):
        for j, fl in enumerate(frame_lens(p)):
            out.append((CHANNELS[(i + j) % 4], p, fl, 1 + (3 * i + 2 * j) % 7))
    return out


CASES = _cases()                                  # (channels, p, frame_len, frames): every p with every kind of frame_len
SPLIT_CASES = [c for c in CASES if c[3] >= 4]     # 1 + 2 + rest needs a rest
FAMILIES = ("random", "silent")                   # (i) and (iii); (ii) is the device's own llz_lpc_mc output, (iv) `static`


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- signals, families
def signal(channels, T, seed):
    """two tones plus noise per channel, |x| < 1, float32; every channel differs from its neighbours"""
    rng = np.random.RandomState(seed)
    t = np.arange(T)
    f1 = 0.01 + 0.08 * rng.rand(channels, 1)
    f2 = 0.15 + 0.2 * rng.rand(channels, 1)
    ph = 2 * np.pi * rng.rand(channels, 2, 1)
    x = 0.45 * np.sin(2 * np.pi * f1 * t + ph[:, 0]) + 0.3 * np.sin(2 * np.pi * f2 * t + ph[:, 1])
    return (x + 0.1 * rng.uniform(-1, 1, size=(channels, T))).astype(np.float32)


def step_up(k):
    """reflection coefficients [..., p] -> a [..., p + 1] by llz_levinson's own update a[j] += k_i a_old[i - j], a[i] = k_i"""
    k = np.asarray(k, dtype=np.float64)
    p = k.shape[-1]
    a = np.zeros(k.shape[:-1] + (p + 1,))
    a[..., 0] = 1.0
    for i in range(1, p + 1):
        ki = k[..., i - 1:i]
        old = a[..., 1:i].copy()
        a[..., 1:i] = old + ki * old[..., ::-1]
        a[..., i] = ki[..., 0]
    return a


def family(name, channels, frames, p, seed):
    """acof [channels, frames, p + 1] float32, stable by construction (|k_i| <= 0.9), every frame unlike the one before it"""
    rng = np.random.RandomState(seed)
    if name == "static":
        return np.repeat(static_sets(channels, p, seed)[:, None, :], frames, axis=1)
    a = step_up(rng.uniform(-0.9, 0.9, size=(channels, frames, p))).astype(np.float32)
    if name == "silent":
        # llz_lpc_mc's answer to a silent frame, [1, 0, ...], on every other frame, the phase alternating with the channel
        for c in range(channels):
            a[c, (c % 2)::2, 1:] = 0.0
    else:
        assert name == "random", name
    return a


def static_sets(channels, p, seed):
    """(iv) one set per channel from poles of radius 0.5 .. 0.9, spread in angle (a clustered degree-64 polynomial does not
    survive its coefficients' rounding to float32), conjugate pairs and one real pole when p is odd"""
    rng = np.random.RandomState(seed)
    out = np.zeros((channels, p + 1))
    pairs = p // 2
    for c in range(channels):
        poles = []
        if pairs:
            ang = np.pi * (np.arange(pairs) + 0.5 + rng.uniform(-0.3, 0.3, size=pairs)) / pairs
            rad = rng.uniform(0.5, 0.9, size=pairs)
            poles = list(rad * np.exp(1j * ang)) + list(rad * np.exp(-1j * ang))
        if p % 2:
            poles.append(rng.uniform(-0.9, 0.9))
        out[c] = np.real(np.poly(poles)) if poles else [1.0]
    return out.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ models
def _frame_index(T, frame_len, p, late=False):
    """frame of sample t; late: the off-by-one-frame bug -- the first p samples of a frame still use the frame before it"""
    t = np.arange(T)
    f = t // frame_len
    if late:
        f = np.where((t % frame_len < p) & (f > 0), f - 1, f)
    return f


def _terms(x, a, frame_len, late, dtype):
    """(x[t] as dtype, generator of (a_f[k] as [C, T], x[t-k] as [C, T]) for k = p .. 1); zeros in front of the stream"""
    C, T = x.shape
    p = a.shape[2] - 1
    f = _frame_index(T, frame_len, p, late)
    xp = np.concatenate([np.zeros((C, p), dtype=dtype), x.astype(dtype)], axis=1)

    def gen():
        for k in range(p, 0, -1):
            yield a[:, f, k].astype(dtype), xp[:, p - k:p - k + T]
    return x.astype(dtype), gen()


def residual64(x, a, frame_len, late=False):
    acc, terms = _terms(x, a, frame_len, late, np.float64)
    acc = acc.copy()
    for ak, xk in terms:
        acc += ak * xk
    return acc


def S(x, a, frame_len):
    acc, terms = _terms(x, a, frame_len, False, np.float64)
    acc = np.abs(acc)
    for ak, xk in terms:
        acc += np.abs(ak * xk)
    return acc


def residual32(x, a, frame_len):
    acc, terms = _terms(x, a, frame_len, False, np.float32)
    acc = acc.copy()
    for ak, xk in terms:
        prod = ak * xk                       # float32: rounded
        acc = acc + prod                     # float32: rounded again
    assert acc.dtype == np.float32
    return acc


def residual_limit(x, a, frame_len):
    p = a.shape[2] - 1
    return 2 * (p + 1) * U * S(x, a, frame_len)


def synth_model(e, a, frame_len, state=None):
    """float64 [C, T]: the unrounded outputs; state: [C, p] doubles, [c][i] = y(-1 - i), zeros when None.  e float32 (or
    float64 for the models' own round trip)"""
    C, T = e.shape
    p = a.shape[2] - 1
    yd = np.zeros((C, p + T))
    if state is not None and p:
        yd[:, :p] = state[:, ::-1]
    ad = a.astype(np.float64)[:, :, :0:-1] if p else None                 # [C, F, p]: a[p], ..., a[1]
    ed = e.astype(np.float64)
    for t in range(T):
        acc = ed[:, t].copy()
        if p:
            prod = ad[:, t // frame_len, :] * yd[:, t:t + p]              # rounded products, lag p first
            for i in range(p):
                acc = acc - prod[:, i]                                    # rounded subtracts, one at a time
        yd[:, p + t] = acc
    return yd[:, p:]


def impulse_response(a_static, tol=1e-17, chunk=512, most=16384):
    """g [C, L] float64 of 1 / A per channel (a_static [C, p + 1]), run until every channel is below tol of its peak"""
    C, p1 = a_static.shape
    a = a_static[:, None, :]
    e = np.zeros((C, chunk))
    e[:, 0] = 1.0
    g = synth_model(e, a, chunk)
    while not (np.abs(g[:, -max(p1, 16):]).max(axis=1) < tol * np.abs(g).max(axis=1)).all():
        assert g.shape[1] < most, "an impulse response of family (iv) does not decay"
        g = np.concatenate([g, synth_model(np.zeros((C, chunk)), a, chunk, state=g[:, :-p1:-1] if p1 > 1 else None)], axis=1)
    return g


@functools.lru_cache(maxsize=None)
def case_data(channels, p, frame_len, frames, fam):
    """x, acof, residual64, limit, and float32(synth_model(x as the excitation)) for one case: computed once per session"""
    T = frames * frame_len
    seed = 1000 * p + frame_len + 7 * channels
    x = signal(channels, T, seed)
    a = family(fam, channels, frames, p, seed + 1)
    d = {"x": x, "a": a, "e64": residual64(x, a, frame_len), "lim": residual_limit(x, a, frame_len)}
    with np.errstate(all="ignore"):
        d["y"] = synth_model(x, a, frame_len).astype(np.float32)
    for v in d.values():
        v.setflags(write=False)
    return d


def check_residual(e, d, what):
    """e against the case's float64 sum under the derived limit, and bit for bit where the coefficients are [1, 0, ...]"""
    a, x = d["a"], d["x"]
    frames = a.shape[1]
    err = np.abs(e.astype(np.float64) - d["e64"])
    worst = float((err / np.maximum(d["lim"], 1e-300)).max())
    print(f"{what}: residual worst |err| / limit = {worst:.3g}")
    assert (err <= d["lim"]).all(), f"{what}: residual misses 2 (p + 1) u S_t: worst ratio {worst:.3g}"
    zero = ~a[:, :, 1:].any(axis=2) if a.shape[2] > 1 else np.ones(a.shape[:2], dtype=bool)
    ev, xv = bits(e).reshape(a.shape[0], frames, -1), bits(x).reshape(a.shape[0], frames, -1)
    assert np.array_equal(ev[zero], xv[zero]), f"{what}: a frame with a[1..p] = 0 does not return x's bits"


def check_synth(y, d, what):
    """y against float32(synth_model), bit for bit (no case here produces a zero of either sign from non-zero inputs, and the
    model runs the same operations in the same order, so bits are compared throughout)"""
    same = bits(y) == bits(d["y"])
    assert same.all(), (f"{what}: synthesis differs from the model in {int((~same).sum())} samples, the first at "
                        f"{tuple(int(i) for i in np.argwhere(~same)[0])}")
