"""CPU-side checks of the biquad bank llz_iir_bank_mc (include/llz_iir.h part 4): the seven symbols are declared and exported,
every refusal comes with a message that names its function, without a GPU a valid init fails loudly -- and the coefficient
families of tests/iir_bank_checks.py meet the conditions under which the limits of tests/iir_checks.py may be asked of a
kernel, and tell a wrong channel from the right one by a wide margin.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest

from llzlab_amd import capi, filters
from tests import iir_bank_checks as ib
from tests import iir_checks as ic

SYMBOLS = ["llz_iir_bank_mc_init", "llz_iir_bank_mc_uninit", "llz_iir_bank_mc", "llz_iir_bank_mc_set_coef",
           "llz_iir_bank_mc_set_stream", "llz_iir_bank_mc_precision", "llz_iir_bank_mc_plan"]
ERR_ARG = -1
N = 8192


@pytest.fixture(scope="module")
def L():
    capi.build()
    return capi.lib()


def test_bank_symbols_declared_and_exported(L):
    text = open(os.path.join(capi.INCLUDE_DIR, "llz_iir.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(llz_iir_bank_mc\w*)\s*\(", text))
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)
    assert all(n in capi.declared_symbols() for n in SYMBOLS)
    assert all(hasattr(L, n) for n in SYMBOLS)


def test_bank_init_refusals_carry_a_message(L):
    coef = np.ascontiguousarray(ib.family32(17, 4))
    p = coef.ctypes.data
    for what, args in (("channels 0", (0, 8, p)), ("channels -3", (-3, 8, p)), ("stages 0", (4, 0, p)), ("stages 17", (4, 17, p)),
                       ("NULL coef", (4, 8, None))):
        L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the init's
        assert L.llz_iir_bank_mc_init(*args) == capi.BAD_HANDLE, what
        assert "llz_iir_bank_mc_init" in capi.last_error(), (what, capi.last_error())
    with pytest.raises(capi.LlzError):
        filters.IirBankMC(4, ic.tiled(8, 0.5, 1.0))                 # 2-D coef: no quiet broadcast to the shared form
    with pytest.raises(capi.LlzError):
        filters.IirBankMC(4, ib.family32(8, 3))
    with pytest.raises(capi.LlzError):
        filters.IirBankMC(4, ib.family32(8, 4)[:, :, :5])


def test_bank_calls_refuse_a_bad_handle(L):
    import ctypes as C
    buf = np.zeros(64, dtype=np.float32)
    cf = np.ascontiguousarray(ib.family32(2, 1))
    out = (C.c_int * 5)()
    p = buf.ctypes.data
    for h in (0, capi.BAD_HANDLE):
        for name, call in (("llz_iir_bank_mc", lambda: L.llz_iir_bank_mc(h, p, p, 16)),
                           ("llz_iir_bank_mc_set_coef", lambda: L.llz_iir_bank_mc_set_coef(h, 0, 1, cf.ctypes.data)),
                           ("llz_iir_bank_mc_set_stream", lambda: L.llz_iir_bank_mc_set_stream(h, None)),
                           ("llz_iir_bank_mc_precision", lambda: L.llz_iir_bank_mc_precision(h)),
                           ("llz_iir_bank_mc_plan", lambda: L.llz_iir_bank_mc_plan(h, 4096, out))):
            L.llz_hip_tune(b"no_such_override", 0)
            assert call() == ERR_ARG and name in capi.last_error(), (name, capi.last_error())
        L.llz_iir_bank_mc_uninit(h)                              # harmless


def test_bank_init_fails_loudly_without_gpu(L):
    """a valid init on a machine without a GPU: BAD_HANDLE and a message, never a result computed elsewhere.  (What a live
    handle refuses -- a set_coef range outside the bank, the shared handle's entry points -- is in test_iir_bank_gpu.py.)"""
    coef = np.ascontiguousarray(ib.family32(3, 4))
    L.llz_hip_tune(b"no_such_override", 0)
    before = capi.last_error()
    h = L.llz_iir_bank_mc_init(4, 3, coef.ctypes.data)
    if L.llz_hip_device_count() > 0:
        assert h != capi.BAD_HANDLE, capi.last_error()
        L.llz_iir_bank_mc_uninit(h)
    else:
        assert h == capi.BAD_HANDLE
        assert capi.last_error() not in ("", before)
        with pytest.raises(capi.LlzError):
            filters.IirBankMC(4, coef)


def tone(coef_c, n=N):
    return (0.9 * np.sin(ic.pole_angle(coef_c) * np.arange(n, dtype=np.float64))).astype(np.float32)


@pytest.mark.parametrize("stages", [8, 5])
def test_float32_family_meets_the_float32_condition(oracle, stages):
    """plain sequential float32 stays at or below a quarter of both float32 limits on every (channel, signal) pair the GPU
    tests use: all 37 channels, every row of iir_checks.signals with tone_res at the channel's own pole angle, 8192 samples.
    Pairs over a quarter must be exactly those listed in iir_bank_checks.F32_DROPPED (none is widened)."""
    coef = ib.family32(stages)
    rows = ic.signals(N, 0.0, [], gap=3 * ic.CHUNK)
    names = list(rows)
    x = np.stack([rows[nm] if nm != "tone_res" else tone(coef[c]) for c in range(ib.CHANNELS) for nm in names])
    cf = np.stack([coef[c] for c in range(ib.CHANNELS) for _ in names])
    who = [(32, stages, c, nm) for c in range(ib.CHANNELS) for nm in names]
    got = ib.plain_f32_bank(x, cf)
    ref = np.stack([oracle.iir_cascade_batch_f32(x[i:i + 1], cf[i])[0] for i in range(len(x))])
    sample = ib.sample_ratio(got, ref, ic.f32_sample_limit(ref, x))
    chunk = ib.chunk_ratio(got, ref, x)
    print(f"float32 family, {stages} sections: plain float32 takes at most {chunk.max():.3g} of the chunk limit "
          f"({who[int(chunk.argmax())]}) and {sample.max():.3g} of the sample limit ({who[int(sample.argmax())]})")
    over = {w for w, s, k in zip(who, sample, chunk) if s > 0.25 or k > 0.25}
    assert over == {w for w in ib.F32_DROPPED if w[1] == stages}, sorted(over)


@pytest.mark.parametrize("stages", [8, 3])
def test_double_family_meets_the_double_condition(oracle, stages):
    """every channel's cascade: memory within the 64-chunk probe, residue after the warm-up <= 1e-11 per unit state and
    homogeneous peak <= 1e3, as the double limit's derivation assumes (iir_checks); and the memories differ between channels,
    so that the handle's warm-up is a real maximum"""
    probes = [ib.probe(oracle, cf) for cf in ib.family64(stages)]
    mems = [p[0] for p in probes]
    print(f"double family, {stages} sections: memory {min(mems)} .. {max(mems)} chunks, peak at most {max(p[1] for p in probes):.3g}, "
          f"residue at most {max(p[2] for p in probes):.3g}")
    assert all(1 <= m <= 64 for m in mems), mems
    assert all(p[1] <= 1e3 and p[2] <= 1e-11 for p in probes), probes
    assert len(set(mems)) > 1, mems


@pytest.mark.parametrize("precision", [32, 64])
def test_a_wrong_channel_is_seen(oracle, precision):
    """for every channel c: the oracle's output with channel c + 1's set instead of its own breaks the per-sample limit of
    the precision on the burst and the tone_res rows, by a factor of at least 10 (the smallest found is printed)"""
    coef = ib.family(precision, 8)
    gap = (ib.bank_warm(oracle, coef) + 1) * ic.CHUNK
    rows = ic.signals(N, 0.0, [], gap=gap)
    smallest = np.inf
    for name in ("burst", "tone_res"):
        for c in range(ib.CHANNELS):
            x = (rows[name] if name == "burst" else tone(coef[c]))[None, :]
            if precision == 64:
                ref, P = ic.section_peaks(oracle, x, coef[c])
                limit = ic.f64_sample_limit(ref, P)
            else:
                ref = oracle.iir_cascade_batch_f32(x, coef[c])
                limit = ic.f32_sample_limit(ref, x)
            wrong = oracle.iir_cascade_batch_f32(x, coef[(c + 1) % ib.CHANNELS])
            smallest = min(smallest, float(ib.sample_ratio(wrong, ref, limit)[0]))
    print(f"precision {precision}: a neighbour's coefficient set misses the sample limit by a factor of at least {smallest:.3g}")
    assert smallest >= 10


def test_carried_state_recursion_equals_the_oracle(oracle):
    """iir_bank_checks.df1_carried, run in two halves with the state handed over, against the oracle's one run"""
    coef = ib.family64(3, 5)
    x = oracle.synth_f32(5, 600, seed=3)
    a, st, Pa = ib.df1_carried(x[:, :250], coef)
    b, _, Pb = ib.df1_carried(x[:, 250:], coef, st)
    ref, P = ib.per_channel_ref(oracle, x, coef, 64)
    assert np.all(np.abs(np.concatenate([a, b], axis=1) - ref) <= 1e-12 * P[:, None])
    assert np.allclose(np.maximum(Pa, Pb), P, rtol=1e-12)
