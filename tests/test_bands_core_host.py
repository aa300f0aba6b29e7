"""The four per-band families (llz_adapt_bands_mc, llz_adapt_bands_matrix_mc, llz_kalman_bands_mc, llz_suppress_bands_mc) share
one host core (csrc/host/llz_bands_core.c), one kernel header and one Python base class; what they SAY must not have changed
with that.  Every refusal that is reachable without a device -- each init refusal the four test_init_refusals_carry_a_message
tests provoke, every call on a bad handle, and the classes' own errors for half a y and a wrong set_taps shape -- equals the
text in MESSAGES, which was printed by this file run as a script (python tests/test_bands_core_host.py) against a build of the
commit before the fold.  And the one fill of the device shim, llzs_fill_f32, is the only one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from llzlab_amd import capi, filters

NAN, INF = float("nan"), float("inf")
INITS = {
    "llz_adapt_bands_mc": ((2, 33, 8, 0.5, 1e-3), {
        0: (0, -1, 65536), 1: (0, -5, 4098), 2: (0, -1, 65), 3: (-0.5, 2.5, NAN), 4: (0.0, -1.0, INF, NAN)}),
    "llz_adapt_bands_matrix_mc": ((2, 3, 33, 8, 0.5, 1e-3), {
        0: (0, -1, 9), 1: (0, -1, 4097), 2: (0, -5, 4098), 3: (0, -1, 65), 4: (-0.5, 2.5, NAN), 5: (0.0, -1.0, INF, NAN)}),
    "llz_kalman_bands_mc": ((2, 33, 8, 0.999, 0.9, 1.0, 1e-3), {
        0: (0, -1, 65536), 1: (0, -5, 4098), 2: (0, -1, 65, 33, 64), 3: (0.0, -0.5, 1.5, NAN), 4: (-0.1, 1.0, NAN),
        5: (0.0, -1.0, INF, NAN), 6: (0.0, -1.0, INF, NAN)}),
}
MATRIX_ENTRIES = ((5, 13), (8, 9), (2, 33), (3, 22))
SUPPRESS = [("channels", v) for v in (0, -1, 65536)] + [("bins", v) for v in (0, -5, 4098)] + \
           [("window", v) for v in (1, 0, -3, 65536)] + \
           [(name, v) for name in ("as_", "aq", "ad", "beta", "rho") for v in (1.0, -0.1, 1.5, NAN)] + \
           [("t0 t1", t) for t in ((0.0, 5.0), (-1.0, 5.0), (5.0, 5.0), (6.0, 5.0), (NAN, 5.0), (2.0, NAN), (2.0, INF))] + \
           [("delta", v) for v in (0.0, -1.0, INF, NAN)]


def said(L, call, want):
    L.llz_hip_tune(b"no_such_override", 0)                      # leaves a message that is not the call's
    assert call() == want
    return capi.last_error()


def suppress_init(L, what, v):
    cfg = filters.SuppressCfg()
    L.llz_suppress_bands_mc_default_cfg(C.byref(cfg))
    channels, bins = 2, 33
    if what == "channels":
        channels = v
    elif what == "bins":
        bins = v
    elif what == "t0 t1":
        cfg.t0, cfg.t1 = v
    else:
        setattr(cfg, what, v)
    return L.llz_suppress_bands_mc_init(channels, bins, C.byref(cfg))


def bare(cls, **attrs):
    """an instance without a handle: the classes refuse half a y and a wrong shape before they touch the library"""
    f = object.__new__(cls)
    f.handle = 0
    for k, v in attrs.items():
        setattr(f, k, v)
    return f


def raised(call):
    with pytest.raises(capi.LlzError) as e:
        call()
    return str(e.value)


def collect(L):
    out = {}
    for p, (good, bad) in INITS.items():
        for index, values in bad.items():
            for v in values:
                args = list(good)
                args[index] = v
                out[f"{p}_init arg {index} = {v}"] = said(L, lambda: getattr(L, p + "_init")(*args), capi.BAD_HANDLE)
    for inputs, taps in MATRIX_ENTRIES:
        out[f"llz_adapt_bands_matrix_mc_init {inputs} x {taps}"] = said(
            L, lambda: L.llz_adapt_bands_matrix_mc_init(inputs, 3, 33, taps, 0.5, 1e-3), capi.BAD_HANDLE)
    for what, v in SUPPRESS:
        out[f"llz_suppress_bands_mc_init {what} = {v}"] = said(L, lambda: suppress_init(L, what, v), capi.BAD_HANDLE)
    f4, i5, n = (C.c_float * 64)(), (C.c_int * 5)(), C.c_longlong()
    for h in (0, capi.BAD_HANDLE):
        calls = {
            "llz_adapt_bands_mc": {"_plan": (i5,), "_reset": (1,), "_frames": (C.byref(n),), "_set_stream": (None,),
                                   "_set_step": (0, 1, f4), "_set_taps": (0, 1, f4, f4), "_get_taps": (0, 1, f4, f4),
                                   "": (f4, f4, f4, f4, f4, f4, None, None, 1)},
            "llz_adapt_bands_matrix_mc": {"_plan": (i5,), "_reset": (1,), "_frames": (C.byref(n),), "_set_stream": (None,),
                                          "_set_step": (0, 1, f4), "_set_taps": (0, 1, 0, 1, f4, f4),
                                          "_get_taps": (0, 1, 0, 1, f4, f4), "": (f4, f4, f4, f4, f4, f4, None, None, 1)},
            "llz_kalman_bands_mc": {"_plan": (i5,), "_reset": (1,), "_frames": (C.byref(n),), "_set_stream": (None,),
                                    "_set_adapt": (0, 1, i5), "_set_taps": (0, 1, f4, f4), "_get_taps": (0, 1, f4, f4),
                                    "_set_variance": (0, 1, f4), "_get_variance": (0, 1, f4), "_get_noise": (0, 1, f4),
                                    "": (f4, f4, f4, f4, f4, f4, None, None, 1)},
            "llz_suppress_bands_mc": {"_plan": (i5,), "_reset": (), "_frames": (C.byref(n),), "_set_stream": (None,),
                                      "_set_enable": (0, 1, i5), "_set_floor": (0, 1, f4), "_set_leak": (0, 1, f4),
                                      "_get_state": (0, 0, 1, f4), "": (f4, f4, None, None, f4, f4, None, 1)},
        }
        for p, names in calls.items():
            for name, args in names.items():
                out[f"{p}{name} on handle {h}"] = said(L, lambda: getattr(L, p + name)(h, *args), -1)
    z = np.zeros((2, 1, 33), dtype=np.float32)
    shapes = dict(channels=2, inputs=2, outputs=2, bins=33, taps=8)
    for cls in (filters.AdaptBandsMC, filters.KalmanBandsMC):
        f = bare(cls, **shapes)
        out[cls.__name__ + " half a y"] = raised(lambda: f.process(z, z, z, z, z, z, y_re=z))
        out[cls.__name__ + " set_taps [3, 7, 33]"] = raised(lambda: f.set_taps(0, np.zeros((3, 7, 33), dtype=np.complex64)))
        out[cls.__name__ + " set_taps [33]"] = raised(lambda: f.set_taps(0, np.zeros(33, dtype=np.complex64)))
    f = bare(filters.KalmanBandsMC, **shapes)
    out["KalmanBandsMC set_variance [8, 32]"] = raised(lambda: f.set_variance(0, np.zeros((8, 32), dtype=np.float32)))
    f = bare(filters.SuppressBandsMC, **shapes)
    out["SuppressBandsMC half a y"] = raised(lambda: f.process(z, z, z, z, y_im=z))
    f = bare(filters.AdaptBandsMatrixMC, **shapes)
    out["AdaptBandsMatrixMC x no pair"] = raised(lambda: f.process(z, (z, z), (z, z)))
    out["AdaptBandsMatrixMC set_taps [2, 8, 33]"] = raised(lambda: f.set_taps(0, np.zeros((2, 8, 33), dtype=np.complex64)))
    out["AdaptBandsMatrixMC set_taps [1, 2, 8, 32]"] = raised(lambda: f.set_taps(0, np.zeros((1, 2, 8, 32), dtype=np.complex64)))
    return out


MESSAGES = {
    'llz_adapt_bands_mc_init arg 0 = 0':
        'llz_adapt_bands_mc_init: channels 0 outside 1..65535',
    'llz_adapt_bands_mc_init arg 0 = -1':
        'llz_adapt_bands_mc_init: channels -1 outside 1..65535',
    'llz_adapt_bands_mc_init arg 0 = 65536':
        'llz_adapt_bands_mc_init: channels 65536 outside 1..65535',
    'llz_adapt_bands_mc_init arg 1 = 0':
        'llz_adapt_bands_mc_init: bins 0 outside 1..4097',
    'llz_adapt_bands_mc_init arg 1 = -5':
        'llz_adapt_bands_mc_init: bins -5 outside 1..4097',
    'llz_adapt_bands_mc_init arg 1 = 4098':
        'llz_adapt_bands_mc_init: bins 4098 outside 1..4097',
    'llz_adapt_bands_mc_init arg 2 = 0':
        'llz_adapt_bands_mc_init: taps 0 outside 1..64',
    'llz_adapt_bands_mc_init arg 2 = -1':
        'llz_adapt_bands_mc_init: taps -1 outside 1..64',
    'llz_adapt_bands_mc_init arg 2 = 65':
        'llz_adapt_bands_mc_init: taps 65 outside 1..64',
    'llz_adapt_bands_mc_init arg 3 = -0.5':
        'llz_adapt_bands_mc_init: mu -0.5 outside 0..2',
    'llz_adapt_bands_mc_init arg 3 = 2.5':
        'llz_adapt_bands_mc_init: mu 2.5 outside 0..2',
    'llz_adapt_bands_mc_init arg 3 = nan':
        'llz_adapt_bands_mc_init: mu nan outside 0..2',
    'llz_adapt_bands_mc_init arg 4 = 0.0':
        'llz_adapt_bands_mc_init: delta 0 is not a finite value above 0',
    'llz_adapt_bands_mc_init arg 4 = -1.0':
        'llz_adapt_bands_mc_init: delta -1 is not a finite value above 0',
    'llz_adapt_bands_mc_init arg 4 = inf':
        'llz_adapt_bands_mc_init: delta inf is not a finite value above 0',
    'llz_adapt_bands_mc_init arg 4 = nan':
        'llz_adapt_bands_mc_init: delta nan is not a finite value above 0',
    'llz_adapt_bands_matrix_mc_init arg 0 = 0':
        'llz_adapt_bands_matrix_mc_init: inputs 0 outside 1..8',
    'llz_adapt_bands_matrix_mc_init arg 0 = -1':
        'llz_adapt_bands_matrix_mc_init: inputs -1 outside 1..8',
    'llz_adapt_bands_matrix_mc_init arg 0 = 9':
        'llz_adapt_bands_matrix_mc_init: inputs 9 outside 1..8',
    'llz_adapt_bands_matrix_mc_init arg 1 = 0':
        'llz_adapt_bands_matrix_mc_init: outputs 0 outside 1..4096',
    'llz_adapt_bands_matrix_mc_init arg 1 = -1':
        'llz_adapt_bands_matrix_mc_init: outputs -1 outside 1..4096',
    'llz_adapt_bands_matrix_mc_init arg 1 = 4097':
        'llz_adapt_bands_matrix_mc_init: outputs 4097 outside 1..4096',
    'llz_adapt_bands_matrix_mc_init arg 2 = 0':
        'llz_adapt_bands_matrix_mc_init: bins 0 outside 1..4097',
    'llz_adapt_bands_matrix_mc_init arg 2 = -5':
        'llz_adapt_bands_matrix_mc_init: bins -5 outside 1..4097',
    'llz_adapt_bands_matrix_mc_init arg 2 = 4098':
        'llz_adapt_bands_matrix_mc_init: bins 4098 outside 1..4097',
    'llz_adapt_bands_matrix_mc_init arg 3 = 0':
        'llz_adapt_bands_matrix_mc_init: taps 0 outside 1..64',
    'llz_adapt_bands_matrix_mc_init arg 3 = -1':
        'llz_adapt_bands_matrix_mc_init: taps -1 outside 1..64',
    'llz_adapt_bands_matrix_mc_init arg 3 = 65':
        'llz_adapt_bands_matrix_mc_init: taps 65 outside 1..64',
    'llz_adapt_bands_matrix_mc_init arg 4 = -0.5':
        'llz_adapt_bands_matrix_mc_init: mu -0.5 outside 0..2',
    'llz_adapt_bands_matrix_mc_init arg 4 = 2.5':
        'llz_adapt_bands_matrix_mc_init: mu 2.5 outside 0..2',
    'llz_adapt_bands_matrix_mc_init arg 4 = nan':
        'llz_adapt_bands_matrix_mc_init: mu nan outside 0..2',
    'llz_adapt_bands_matrix_mc_init arg 5 = 0.0':
        'llz_adapt_bands_matrix_mc_init: delta 0 is not a finite value above 0',
    'llz_adapt_bands_matrix_mc_init arg 5 = -1.0':
        'llz_adapt_bands_matrix_mc_init: delta -1 is not a finite value above 0',
    'llz_adapt_bands_matrix_mc_init arg 5 = inf':
        'llz_adapt_bands_matrix_mc_init: delta inf is not a finite value above 0',
    'llz_adapt_bands_matrix_mc_init arg 5 = nan':
        'llz_adapt_bands_matrix_mc_init: delta nan is not a finite value above 0',
    'llz_kalman_bands_mc_init arg 0 = 0':
        'llz_kalman_bands_mc_init: channels 0 outside 1..65535',
    'llz_kalman_bands_mc_init arg 0 = -1':
        'llz_kalman_bands_mc_init: channels -1 outside 1..65535',
    'llz_kalman_bands_mc_init arg 0 = 65536':
        'llz_kalman_bands_mc_init: channels 65536 outside 1..65535',
    'llz_kalman_bands_mc_init arg 1 = 0':
        'llz_kalman_bands_mc_init: bins 0 outside 1..4097',
    'llz_kalman_bands_mc_init arg 1 = -5':
        'llz_kalman_bands_mc_init: bins -5 outside 1..4097',
    'llz_kalman_bands_mc_init arg 1 = 4098':
        'llz_kalman_bands_mc_init: bins 4098 outside 1..4097',
    'llz_kalman_bands_mc_init arg 2 = 0':
        'llz_kalman_bands_mc_init: taps 0 outside 1..32',
    'llz_kalman_bands_mc_init arg 2 = -1':
        'llz_kalman_bands_mc_init: taps -1 outside 1..32',
    'llz_kalman_bands_mc_init arg 2 = 65':
        'llz_kalman_bands_mc_init: taps 65 outside 1..32',
    'llz_kalman_bands_mc_init arg 2 = 33':
        "llz_kalman_bands_mc_init: taps 33: above 32 taps the weights, the history and the variances of a band no longer fit a lane's registers (llz_adapt_bands_mc takes up to 64)",
    'llz_kalman_bands_mc_init arg 2 = 64':
        "llz_kalman_bands_mc_init: taps 64: above 32 taps the weights, the history and the variances of a band no longer fit a lane's registers (llz_adapt_bands_mc takes up to 64)",
    'llz_kalman_bands_mc_init arg 3 = 0.0':
        'llz_kalman_bands_mc_init: a 0 is not above 0 and at most 1',
    'llz_kalman_bands_mc_init arg 3 = -0.5':
        'llz_kalman_bands_mc_init: a -0.5 is not above 0 and at most 1',
    'llz_kalman_bands_mc_init arg 3 = 1.5':
        'llz_kalman_bands_mc_init: a 1.5 is not above 0 and at most 1',
    'llz_kalman_bands_mc_init arg 3 = nan':
        'llz_kalman_bands_mc_init: a nan is not above 0 and at most 1',
    'llz_kalman_bands_mc_init arg 4 = -0.1':
        'llz_kalman_bands_mc_init: lam -0.1 is not at least 0 and below 1',
    'llz_kalman_bands_mc_init arg 4 = 1.0':
        'llz_kalman_bands_mc_init: lam 1 is not at least 0 and below 1',
    'llz_kalman_bands_mc_init arg 4 = nan':
        'llz_kalman_bands_mc_init: lam nan is not at least 0 and below 1',
    'llz_kalman_bands_mc_init arg 5 = 0.0':
        'llz_kalman_bands_mc_init: p0 0 is not a finite variance above 0',
    'llz_kalman_bands_mc_init arg 5 = -1.0':
        'llz_kalman_bands_mc_init: p0 -1 is not a finite variance above 0',
    'llz_kalman_bands_mc_init arg 5 = inf':
        'llz_kalman_bands_mc_init: p0 inf is not a finite variance above 0',
    'llz_kalman_bands_mc_init arg 5 = nan':
        'llz_kalman_bands_mc_init: p0 nan is not a finite variance above 0',
    'llz_kalman_bands_mc_init arg 6 = 0.0':
        'llz_kalman_bands_mc_init: delta 0 is not a finite value above 0',
    'llz_kalman_bands_mc_init arg 6 = -1.0':
        'llz_kalman_bands_mc_init: delta -1 is not a finite value above 0',
    'llz_kalman_bands_mc_init arg 6 = inf':
        'llz_kalman_bands_mc_init: delta inf is not a finite value above 0',
    'llz_kalman_bands_mc_init arg 6 = nan':
        'llz_kalman_bands_mc_init: delta nan is not a finite value above 0',
    'llz_adapt_bands_matrix_mc_init 5 x 13':
        'llz_adapt_bands_matrix_mc_init: inputs x taps = 5 x 13 = 65 regressor entries, above 64',
    'llz_adapt_bands_matrix_mc_init 8 x 9':
        'llz_adapt_bands_matrix_mc_init: inputs x taps = 8 x 9 = 72 regressor entries, above 64',
    'llz_adapt_bands_matrix_mc_init 2 x 33':
        'llz_adapt_bands_matrix_mc_init: inputs x taps = 2 x 33 = 66 regressor entries, above 64',
    'llz_adapt_bands_matrix_mc_init 3 x 22':
        'llz_adapt_bands_matrix_mc_init: inputs x taps = 3 x 22 = 66 regressor entries, above 64',
    'llz_suppress_bands_mc_init channels = 0':
        'llz_suppress_bands_mc_init: channels 0 outside 1..65535',
    'llz_suppress_bands_mc_init channels = -1':
        'llz_suppress_bands_mc_init: channels -1 outside 1..65535',
    'llz_suppress_bands_mc_init channels = 65536':
        'llz_suppress_bands_mc_init: channels 65536 outside 1..65535',
    'llz_suppress_bands_mc_init bins = 0':
        'llz_suppress_bands_mc_init: bins 0 outside 1..4097',
    'llz_suppress_bands_mc_init bins = -5':
        'llz_suppress_bands_mc_init: bins -5 outside 1..4097',
    'llz_suppress_bands_mc_init bins = 4098':
        'llz_suppress_bands_mc_init: bins 4098 outside 1..4097',
    'llz_suppress_bands_mc_init window = 1':
        'llz_suppress_bands_mc_init: window 1 outside 2..65535',
    'llz_suppress_bands_mc_init window = 0':
        'llz_suppress_bands_mc_init: window 0 outside 2..65535',
    'llz_suppress_bands_mc_init window = -3':
        'llz_suppress_bands_mc_init: window -3 outside 2..65535',
    'llz_suppress_bands_mc_init window = 65536':
        'llz_suppress_bands_mc_init: window 65536 outside 2..65535',
    'llz_suppress_bands_mc_init as_ = 1.0':
        'llz_suppress_bands_mc_init: as 1 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init as_ = -0.1':
        'llz_suppress_bands_mc_init: as -0.1 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init as_ = 1.5':
        'llz_suppress_bands_mc_init: as 1.5 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init as_ = nan':
        'llz_suppress_bands_mc_init: as nan is not at least 0 and below 1',
    'llz_suppress_bands_mc_init aq = 1.0':
        'llz_suppress_bands_mc_init: aq 1 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init aq = -0.1':
        'llz_suppress_bands_mc_init: aq -0.1 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init aq = 1.5':
        'llz_suppress_bands_mc_init: aq 1.5 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init aq = nan':
        'llz_suppress_bands_mc_init: aq nan is not at least 0 and below 1',
    'llz_suppress_bands_mc_init ad = 1.0':
        'llz_suppress_bands_mc_init: ad 1 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init ad = -0.1':
        'llz_suppress_bands_mc_init: ad -0.1 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init ad = 1.5':
        'llz_suppress_bands_mc_init: ad 1.5 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init ad = nan':
        'llz_suppress_bands_mc_init: ad nan is not at least 0 and below 1',
    'llz_suppress_bands_mc_init beta = 1.0':
        'llz_suppress_bands_mc_init: beta 1 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init beta = -0.1':
        'llz_suppress_bands_mc_init: beta -0.1 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init beta = 1.5':
        'llz_suppress_bands_mc_init: beta 1.5 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init beta = nan':
        'llz_suppress_bands_mc_init: beta nan is not at least 0 and below 1',
    'llz_suppress_bands_mc_init rho = 1.0':
        'llz_suppress_bands_mc_init: rho 1 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init rho = -0.1':
        'llz_suppress_bands_mc_init: rho -0.1 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init rho = 1.5':
        'llz_suppress_bands_mc_init: rho 1.5 is not at least 0 and below 1',
    'llz_suppress_bands_mc_init rho = nan':
        'llz_suppress_bands_mc_init: rho nan is not at least 0 and below 1',
    'llz_suppress_bands_mc_init t0 t1 = (0.0, 5.0)':
        'llz_suppress_bands_mc_init: thresholds t0 0, t1 5 are not finite with 0 < t0 < t1',
    'llz_suppress_bands_mc_init t0 t1 = (-1.0, 5.0)':
        'llz_suppress_bands_mc_init: thresholds t0 -1, t1 5 are not finite with 0 < t0 < t1',
    'llz_suppress_bands_mc_init t0 t1 = (5.0, 5.0)':
        'llz_suppress_bands_mc_init: thresholds t0 5, t1 5 are not finite with 0 < t0 < t1',
    'llz_suppress_bands_mc_init t0 t1 = (6.0, 5.0)':
        'llz_suppress_bands_mc_init: thresholds t0 6, t1 5 are not finite with 0 < t0 < t1',
    'llz_suppress_bands_mc_init t0 t1 = (nan, 5.0)':
        'llz_suppress_bands_mc_init: thresholds t0 nan, t1 5 are not finite with 0 < t0 < t1',
    'llz_suppress_bands_mc_init t0 t1 = (2.0, nan)':
        'llz_suppress_bands_mc_init: thresholds t0 2, t1 nan are not finite with 0 < t0 < t1',
    'llz_suppress_bands_mc_init t0 t1 = (2.0, inf)':
        'llz_suppress_bands_mc_init: thresholds t0 2, t1 inf are not finite with 0 < t0 < t1',
    'llz_suppress_bands_mc_init delta = 0.0':
        'llz_suppress_bands_mc_init: delta 0 is not a finite value above 0',
    'llz_suppress_bands_mc_init delta = -1.0':
        'llz_suppress_bands_mc_init: delta -1 is not a finite value above 0',
    'llz_suppress_bands_mc_init delta = inf':
        'llz_suppress_bands_mc_init: delta inf is not a finite value above 0',
    'llz_suppress_bands_mc_init delta = nan':
        'llz_suppress_bands_mc_init: delta nan is not a finite value above 0',
    'llz_adapt_bands_mc_plan on handle 0':
        'llz_adapt_bands_mc_plan: bad handle',
    'llz_adapt_bands_mc_reset on handle 0':
        'llz_adapt_bands_mc_reset: bad handle',
    'llz_adapt_bands_mc_frames on handle 0':
        'llz_adapt_bands_mc_frames: bad handle',
    'llz_adapt_bands_mc_set_stream on handle 0':
        'llz_adapt_bands_mc_set_stream: bad handle',
    'llz_adapt_bands_mc_set_step on handle 0':
        'llz_adapt_bands_mc_set_step: bad handle',
    'llz_adapt_bands_mc_set_taps on handle 0':
        'llz_adapt_bands_mc_set_taps: bad handle',
    'llz_adapt_bands_mc_get_taps on handle 0':
        'llz_adapt_bands_mc_get_taps: bad handle',
    'llz_adapt_bands_mc on handle 0':
        'llz_adapt_bands_mc: bad handle',
    'llz_adapt_bands_matrix_mc_plan on handle 0':
        'llz_adapt_bands_matrix_mc_plan: bad handle',
    'llz_adapt_bands_matrix_mc_reset on handle 0':
        'llz_adapt_bands_matrix_mc_reset: bad handle',
    'llz_adapt_bands_matrix_mc_frames on handle 0':
        'llz_adapt_bands_matrix_mc_frames: bad handle',
    'llz_adapt_bands_matrix_mc_set_stream on handle 0':
        'llz_adapt_bands_matrix_mc_set_stream: bad handle',
    'llz_adapt_bands_matrix_mc_set_step on handle 0':
        'llz_adapt_bands_matrix_mc_set_step: bad handle',
    'llz_adapt_bands_matrix_mc_set_taps on handle 0':
        'llz_adapt_bands_matrix_mc_set_taps: bad handle',
    'llz_adapt_bands_matrix_mc_get_taps on handle 0':
        'llz_adapt_bands_matrix_mc_get_taps: bad handle',
    'llz_adapt_bands_matrix_mc on handle 0':
        'llz_adapt_bands_matrix_mc: bad handle',
    'llz_kalman_bands_mc_plan on handle 0':
        'llz_kalman_bands_mc_plan: bad handle',
    'llz_kalman_bands_mc_reset on handle 0':
        'llz_kalman_bands_mc_reset: bad handle',
    'llz_kalman_bands_mc_frames on handle 0':
        'llz_kalman_bands_mc_frames: bad handle',
    'llz_kalman_bands_mc_set_stream on handle 0':
        'llz_kalman_bands_mc_set_stream: bad handle',
    'llz_kalman_bands_mc_set_adapt on handle 0':
        'llz_kalman_bands_mc_set_adapt: bad handle',
    'llz_kalman_bands_mc_set_taps on handle 0':
        'llz_kalman_bands_mc_set_taps: bad handle',
    'llz_kalman_bands_mc_get_taps on handle 0':
        'llz_kalman_bands_mc_get_taps: bad handle',
    'llz_kalman_bands_mc_set_variance on handle 0':
        'llz_kalman_bands_mc_set_variance: bad handle',
    'llz_kalman_bands_mc_get_variance on handle 0':
        'llz_kalman_bands_mc_get_variance: bad handle',
    'llz_kalman_bands_mc_get_noise on handle 0':
        'llz_kalman_bands_mc_get_noise: bad handle',
    'llz_kalman_bands_mc on handle 0':
        'llz_kalman_bands_mc: bad handle',
    'llz_suppress_bands_mc_plan on handle 0':
        'llz_suppress_bands_mc_plan: bad handle',
    'llz_suppress_bands_mc_reset on handle 0':
        'llz_suppress_bands_mc_reset: bad handle',
    'llz_suppress_bands_mc_frames on handle 0':
        'llz_suppress_bands_mc_frames: bad handle',
    'llz_suppress_bands_mc_set_stream on handle 0':
        'llz_suppress_bands_mc_set_stream: bad handle',
    'llz_suppress_bands_mc_set_enable on handle 0':
        'llz_suppress_bands_mc_set_enable: bad handle',
    'llz_suppress_bands_mc_set_floor on handle 0':
        'llz_suppress_bands_mc_set_floor: bad handle',
    'llz_suppress_bands_mc_set_leak on handle 0':
        'llz_suppress_bands_mc_set_leak: bad handle',
    'llz_suppress_bands_mc_get_state on handle 0':
        'llz_suppress_bands_mc_get_state: bad handle',
    'llz_suppress_bands_mc on handle 0':
        'llz_suppress_bands_mc: bad handle',
    'llz_adapt_bands_mc_plan on handle 18446744073709551615':
        'llz_adapt_bands_mc_plan: bad handle',
    'llz_adapt_bands_mc_reset on handle 18446744073709551615':
        'llz_adapt_bands_mc_reset: bad handle',
    'llz_adapt_bands_mc_frames on handle 18446744073709551615':
        'llz_adapt_bands_mc_frames: bad handle',
    'llz_adapt_bands_mc_set_stream on handle 18446744073709551615':
        'llz_adapt_bands_mc_set_stream: bad handle',
    'llz_adapt_bands_mc_set_step on handle 18446744073709551615':
        'llz_adapt_bands_mc_set_step: bad handle',
    'llz_adapt_bands_mc_set_taps on handle 18446744073709551615':
        'llz_adapt_bands_mc_set_taps: bad handle',
    'llz_adapt_bands_mc_get_taps on handle 18446744073709551615':
        'llz_adapt_bands_mc_get_taps: bad handle',
    'llz_adapt_bands_mc on handle 18446744073709551615':
        'llz_adapt_bands_mc: bad handle',
    'llz_adapt_bands_matrix_mc_plan on handle 18446744073709551615':
        'llz_adapt_bands_matrix_mc_plan: bad handle',
    'llz_adapt_bands_matrix_mc_reset on handle 18446744073709551615':
        'llz_adapt_bands_matrix_mc_reset: bad handle',
    'llz_adapt_bands_matrix_mc_frames on handle 18446744073709551615':
        'llz_adapt_bands_matrix_mc_frames: bad handle',
    'llz_adapt_bands_matrix_mc_set_stream on handle 18446744073709551615':
        'llz_adapt_bands_matrix_mc_set_stream: bad handle',
    'llz_adapt_bands_matrix_mc_set_step on handle 18446744073709551615':
        'llz_adapt_bands_matrix_mc_set_step: bad handle',
    'llz_adapt_bands_matrix_mc_set_taps on handle 18446744073709551615':
        'llz_adapt_bands_matrix_mc_set_taps: bad handle',
    'llz_adapt_bands_matrix_mc_get_taps on handle 18446744073709551615':
        'llz_adapt_bands_matrix_mc_get_taps: bad handle',
    'llz_adapt_bands_matrix_mc on handle 18446744073709551615':
        'llz_adapt_bands_matrix_mc: bad handle',
    'llz_kalman_bands_mc_plan on handle 18446744073709551615':
        'llz_kalman_bands_mc_plan: bad handle',
    'llz_kalman_bands_mc_reset on handle 18446744073709551615':
        'llz_kalman_bands_mc_reset: bad handle',
    'llz_kalman_bands_mc_frames on handle 18446744073709551615':
        'llz_kalman_bands_mc_frames: bad handle',
    'llz_kalman_bands_mc_set_stream on handle 18446744073709551615':
        'llz_kalman_bands_mc_set_stream: bad handle',
    'llz_kalman_bands_mc_set_adapt on handle 18446744073709551615':
        'llz_kalman_bands_mc_set_adapt: bad handle',
    'llz_kalman_bands_mc_set_taps on handle 18446744073709551615':
        'llz_kalman_bands_mc_set_taps: bad handle',
    'llz_kalman_bands_mc_get_taps on handle 18446744073709551615':
        'llz_kalman_bands_mc_get_taps: bad handle',
    'llz_kalman_bands_mc_set_variance on handle 18446744073709551615':
        'llz_kalman_bands_mc_set_variance: bad handle',
    'llz_kalman_bands_mc_get_variance on handle 18446744073709551615':
        'llz_kalman_bands_mc_get_variance: bad handle',
    'llz_kalman_bands_mc_get_noise on handle 18446744073709551615':
        'llz_kalman_bands_mc_get_noise: bad handle',
    'llz_kalman_bands_mc on handle 18446744073709551615':
        'llz_kalman_bands_mc: bad handle',
    'llz_suppress_bands_mc_plan on handle 18446744073709551615':
        'llz_suppress_bands_mc_plan: bad handle',
    'llz_suppress_bands_mc_reset on handle 18446744073709551615':
        'llz_suppress_bands_mc_reset: bad handle',
    'llz_suppress_bands_mc_frames on handle 18446744073709551615':
        'llz_suppress_bands_mc_frames: bad handle',
    'llz_suppress_bands_mc_set_stream on handle 18446744073709551615':
        'llz_suppress_bands_mc_set_stream: bad handle',
    'llz_suppress_bands_mc_set_enable on handle 18446744073709551615':
        'llz_suppress_bands_mc_set_enable: bad handle',
    'llz_suppress_bands_mc_set_floor on handle 18446744073709551615':
        'llz_suppress_bands_mc_set_floor: bad handle',
    'llz_suppress_bands_mc_set_leak on handle 18446744073709551615':
        'llz_suppress_bands_mc_set_leak: bad handle',
    'llz_suppress_bands_mc_get_state on handle 18446744073709551615':
        'llz_suppress_bands_mc_get_state: bad handle',
    'llz_suppress_bands_mc on handle 18446744073709551615':
        'llz_suppress_bands_mc: bad handle',
    'AdaptBandsMC half a y':
        'AdaptBandsMC.process: y_re and y_im must both be given or both be None',
    'AdaptBandsMC set_taps [3, 7, 33]':
        'AdaptBandsMC.set_taps: w must be [count, taps = 8, bins = 33], got (3, 7, 33)',
    'AdaptBandsMC set_taps [33]':
        'AdaptBandsMC.set_taps: w must be [count, taps = 8, bins = 33], got (33,)',
    'KalmanBandsMC half a y':
        'KalmanBandsMC.process: y_re and y_im must both be given or both be None',
    'KalmanBandsMC set_taps [3, 7, 33]':
        'KalmanBandsMC.set_taps: must be [count, taps = 8, bins = 33], got (3, 7, 33)',
    'KalmanBandsMC set_taps [33]':
        'KalmanBandsMC.set_taps: must be [count, taps = 8, bins = 33], got (33,)',
    'KalmanBandsMC set_variance [8, 32]':
        'KalmanBandsMC.set_variance: must be [count, taps = 8, bins = 33], got (1, 8, 32)',
    'SuppressBandsMC half a y':
        'SuppressBandsMC.process: y_re and y_im must both be given or both be None',
    'AdaptBandsMatrixMC x no pair':
        'AdaptBandsMatrixMC.process: x must be a pair (re, im)',
    'AdaptBandsMatrixMC set_taps [2, 8, 33]':
        'AdaptBandsMatrixMC.set_taps: w must be [out_count, in_count, taps = 8, bins = 33], got (2, 8, 33)',
    'AdaptBandsMatrixMC set_taps [1, 2, 8, 32]':
        'AdaptBandsMatrixMC.set_taps: w must be [out_count, in_count, taps = 8, bins = 33], got (1, 2, 8, 32)',
}


@pytest.fixture(scope="module")
def L():
    capi.build()
    return capi.lib()


def test_every_message_is_the_parents(L):
    got = collect(L)
    assert set(got) == set(MESSAGES) and len(got) > 150
    wrong = {k: (v, MESSAGES[k]) for k, v in got.items() if v != MESSAGES[k]}
    assert not wrong, wrong


def test_the_shared_messages_exist_once():
    """what went to llz_bands_core.c (and, for mu and delta, to llz_adapt_core.c) is there once, and no band handle keeps a copy
    of it or stages a buffer by itself"""
    from tests.test_host_sanitizers import CSRC
    host = os.path.join(CSRC, "host")
    core = open(os.path.join(host, "llz_bands_core.c")).read()
    moved = ("outside %d..%d", "frames x bins below 2^31", "must both be NULL or both be set", "NULL buffer", "no out",
             "outside the handle's", "no device memory to stage %d buffers of %zu B\"", "(x) and %zu B", "no host memory for %zu B of %s")
    for text in moved:
        assert core.count(text) == 1, text
    adapt = open(os.path.join(host, "llz_adapt_core.c")).read()
    assert adapt.count("mu %g outside 0..2") == 1 and adapt.count("is not a finite value above 0") == 1
    for fn in ("llz_adapt_bands_host.c", "llz_adapt_bands_matrix_host.c", "llz_kalman_bands_host.c", "llz_suppress_bands_host.c"):
        text = open(os.path.join(host, fn)).read()
        assert "llz_bands_begin(" in text and "llz_bands_end(" in text and "llz_bands_frames(" in text, fn
        for other in moved + ("outside 0..2", "is not a finite value", "llz_refuse_device_overlap", "llz_stage_in", "llz_stage_out",
                              "llzs_is_device_ptr"):
            assert other not in text, (fn, other)


def test_one_fill_in_the_shim():
    from tests.test_host_sanitizers import CSRC, gen_stub
    shim = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "llz_shim.h")).read(), flags=re.S)
    assert re.findall(r"\b(llzs_\w*fill\w*)\s*\(", shim) == ["llzs_fill_f32"]
    assert "int llzs_fill_f32(" in gen_stub()


if __name__ == "__main__":
    print("# library:", capi.LIB_PATH)
    print("MESSAGES = {")
    for k, v in collect(capi.lib()).items():
        print(f"    {k!r}:\n        {v!r},")
    print("}")
