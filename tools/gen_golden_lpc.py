"""Writes tests/golden/lpc.npz: the reference's own llz_levinson / llz_levinson1 / llz_atlvs / llz_lpc results (inputs and
outputs only).  Needs the reference tree (REFERENCE, default /root/reference): its llz_corr.c, llz_fft.c, llz_levinson.c
and llz_lpc.c are compiled where they lie, with oracle/Makefile's `ref` flags, into a temporary directory that is deleted
afterwards.  No test, smoke() or bench.py runs this.

    python tools/gen_golden_lpc.py [--reference DIR] [--out tests/golden/lpc.npz]
"""
import argparse
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = (1, 2, 8, 10, 16, 32, 64)
_dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


def build(reference, tmp):
    src = [os.path.join(reference, "libllzfilter", f) for f in ("llz_corr.c", "llz_fft.c", "llz_levinson.c", "llz_lpc.c")]
    so = os.path.join(tmp, "liblpcref.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-w", "-shared", "-o", so] + src + ["-lm"])
    L = C.CDLL(so)
    for name in ("llz_levinson", "llz_levinson1"):
        getattr(L, name).argtypes = [_dp, C.c_int, _dp, _dp, _dp]
        getattr(L, name).restype = None
    L.llz_atlvs.argtypes = [_dp, C.c_int, _dp, _dp, _dp, _dp]
    L.llz_atlvs.restype = C.c_int
    L.llz_autocorr.argtypes = [_dp, C.c_int, C.c_int, _dp]
    L.llz_lpc_init.argtypes = [C.c_int]
    L.llz_lpc_init.restype = C.c_ulong
    L.llz_lpc_uninit.argtypes = [C.c_ulong]
    L.llz_lpc.argtypes = [C.c_ulong, _dp, C.c_int, _dp, _dp, _dp]
    L.llz_lpc.restype = C.c_double
    return L


def toeplitz_cases(rng, p):
    """(name, r[0..p]): a well-conditioned autocorrelation and an ill-conditioned one (a narrow-band signal)"""
    n = 4 * p + 64
    t = np.arange(n)
    x_rand = rng.standard_normal(n)
    x_ill = np.sin(0.05 * t) + 0.5 * np.sin(0.11 * t + 1.0) + 1e-6 * rng.standard_normal(n)
    out = []
    for name, x in (("rand", x_rand), ("ill", x_ill)):
        r = np.array([np.dot(x[:n - k], x[k:]) for k in range(p + 1)])
        out.append((name, r))
    return out


def generate(L):
    rng = np.random.default_rng(20121117)
    d = {}
    for p in ORDERS:
        for name, r in toeplitz_cases(rng, p):
            key = f"{name}_{p}"
            d["r_" + key] = r
            for fn in ("llz_levinson", "llz_levinson1"):
                acof, kcof, err = np.zeros(p + 1), np.zeros(p + 1), np.zeros(1)
                getattr(L, fn)(_p(r), p, _p(acof), _p(kcof), _p(err))
                tag = "lev" if fn == "llz_levinson" else "lev1"
                d[f"{tag}_acof_{key}"], d[f"{tag}_kcof_{key}"], d[f"{tag}_err_{key}"] = acof, kcof, err
            b = rng.standard_normal(p)
            x, kcof, err = np.zeros(p), np.zeros(p), np.zeros(1)
            rc = L.llz_atlvs(_p(r), p, _p(b), _p(x), _p(kcof), _p(err))
            d[f"atl_b_{key}"], d[f"atl_x_{key}"], d[f"atl_kcof_{key}"] = b, x, kcof
            d[f"atl_err_{key}"], d[f"atl_rc_{key}"] = err, np.array([rc])
    # silent r for llz_levinson: acof[0] / kcof[0] untouched (the arrays start as zeros, as the binding's do)
    r = np.zeros(11)
    acof, kcof, err = np.full(11, 0.0), np.full(11, 0.0), np.zeros(1)
    L.llz_levinson(_p(r), 10, _p(acof), _p(kcof), _p(err))
    d["lev_silent_acof"], d["lev_silent_kcof"], d["lev_silent_err"] = acof, kcof, err
    # singular llz_atlvs cases: a constant r (the error vanishes after one step) and a negligible r[0]
    for name, r in (("const", np.ones(8)), ("tiny", np.array([1e-17, 0.5, 0.25, 0.1]))):
        n = len(r)
        b = np.arange(1.0, n + 1)
        x, kcof, err = np.zeros(n), np.zeros(n), np.zeros(1)
        rc = L.llz_atlvs(_p(r), n, _p(b), _p(x), _p(kcof), _p(err))
        d[f"sing_r_{name}"], d[f"sing_b_{name}"], d[f"sing_x_{name}"] = r, b, x
        d[f"sing_kcof_{name}"], d[f"sing_err_{name}"], d[f"sing_rc_{name}"] = kcof, err, np.array([rc])
    # llz_lpc call sequences on one handle: silent after normal, normal after silent, x_len below and above p
    seqs = {
        "a": (10, [("noise", 240), ("silent", 240), ("noise", 240), ("noise", 5)]),
        "b": (16, [("silent", 160), ("noise", 160), ("silent", 160), ("tone", 320)]),
        "c": (32, [("noise", 20), ("tone", 512), ("silent", 64)]),
        "d": (64, [("tone", 1024), ("silent", 100), ("noise", 1024)]),
    }
    for s, (p, steps) in seqs.items():
        h = L.llz_lpc_init(p)
        d[f"lpc_{s}_p"] = np.array([p])
        for i, (kind, n) in enumerate(steps):
            if kind == "silent":
                x = np.zeros(n)
            elif kind == "tone":
                x = np.sin(0.07 * np.arange(n)) + 0.01 * rng.standard_normal(n)
            else:
                x = rng.standard_normal(n)
            acof, kcof, err = np.zeros(p + 1), np.zeros(p + 1), np.zeros(1)
            gain = L.llz_lpc(h, _p(x), n, _p(acof), _p(kcof), _p(err))
            k = f"lpc_{s}_{i}"
            d[k + "_x"], d[k + "_acof"], d[k + "_kcof"] = x, acof, kcof
            d[k + "_err"], d[k + "_gain"] = err, np.array([gain])
        d[f"lpc_{s}_steps"] = np.array([len(steps)])
        L.llz_lpc_uninit(h)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lpc.npz"))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="lpcref_")
    try:
        d = generate(build(a.reference, tmp))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(a.out, **d)
    print(f"wrote {a.out}: {len(d)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
