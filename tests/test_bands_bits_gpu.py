"""The four per-band filters (AdaptBandsMC, AdaptBandsMatrixMC, KalmanBandsMC, SuppressBandsMC) keep their bits: every output
and every readable piece of state of a case, concatenated, has the SHA-256 written below.  The digests were printed by this file
run as a script against a build of the commit BEFORE the four families were folded onto kernels/bands_steps.hpp,
host/llz_bands_core.c and filters._BandsFilter (profiles/bands/refactor_bits.txt holds the printed lines), so a digest that
differs is a change of behaviour in a kernel, in the staged call or in the marshalling.

The inputs are an integer formula, ((7 i + 13 k) % 97 - 48) / 64 for element i of a case's k-th buffer: the bytes depend on
nothing but this file.  Every case runs as calls of 1 and 6 frames on one handle, so that state is carried between calls; the
forms with y take host (numpy) buffers, which are staged, the forms without take device tensors, which are used where they lie.
The shapes are the smallest at which these kernels can go wrong: 33 bins make a wave straddle channel rows, 64 do not; 1 tap has
no history, 5 is the first tap behind an instance's unguarded half, the others sit at or just above a ceiling; the matrix pairs
make 1, 6, 9, 32 and 64 entries, every ceiling and an I that is no power of two.

    python tests/test_bands_bits_gpu.py          prints "<case> <sha256>" per case"""
import hashlib

import numpy as np
import pytest
import torch

from llzlab_amd import capi, filters

pytestmark = pytest.mark.gpu
CALLS = (1, 6)
FRAMES = sum(CALLS)


def weights(*shape):
    """complex start weights, a quarter of the formula's buffers 4 and 5: a frozen row filters with them to the end"""
    return (formula(4, *shape) + 1j * formula(5, *shape)) / 4


def formula(k, *shape):
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    return (((i * 7 + k * 13) % 97 - 48) / 64).astype(np.float32).reshape(shape)


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.complex64), a.dtype
        h.update(a.tobytes())
    return h.hexdigest()


class Buffers:
    """host buffers (staged by the library) or device tensors (used where they lie) of one call"""

    def __init__(self, on_device):
        self.on_device = on_device

    def given(self, a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a).to("cuda:0") if self.on_device else a

    def empty(self, *shape):
        return self.given(np.full(shape, np.float32(-7.0)))

    @staticmethod
    def host(b):
        return b.cpu().numpy() if isinstance(b, torch.Tensor) else b


def frames_of(a, m0, n):
    return a[:, m0:m0 + n]


def run_pairs(f, rows_x, rows_d, bins, with_y, process):
    """the 1 + 6 frames of a filter with x / d / e / y: process(x pair, d pair, e pair, y pair or None); returns e and y of
    every call"""
    buf = Buffers(on_device=not with_y)
    x = [formula(k, rows_x, FRAMES, bins) for k in (0, 1)]
    d = [formula(k, rows_d, FRAMES, bins) for k in (2, 3)]
    out, m0 = [], 0
    for n in CALLS:
        xs = [buf.given(frames_of(a, m0, n)) for a in x]
        ds = [buf.given(frames_of(a, m0, n)) for a in d]
        e = [buf.empty(rows_d, n, bins) for _ in range(2)]
        y = [buf.empty(rows_d, n, bins) for _ in range(2)] if with_y else None
        process(xs, ds, e, y)
        out += [buf.host(b) for b in e + (y or [])]
        m0 += n
    return out


def nlms(bins, taps, with_y):
    f = filters.AdaptBandsMC(3, bins, taps)
    f.set_taps(0, weights(3, taps, bins))
    f.set_step(1, 0.0)                                                     # one channel frozen
    out = run_pairs(f, 3, 3, bins, with_y, lambda x, d, e, y: f.process(*x, *d, *e, *(y or ())))
    assert f.frames() == FRAMES
    out.append(f.get_taps())
    f.close()
    return out


def matrix(inputs, taps, with_y):
    f = filters.AdaptBandsMatrixMC(inputs, 2, 33, taps)
    f.set_taps(0, weights(2, inputs, taps, 33))
    f.set_step(1, 0.0)                                                     # one output frozen
    out = run_pairs(f, inputs, 2, 33, with_y, lambda x, d, e, y: f.process(tuple(x), tuple(d), tuple(e), tuple(y) if y else None))
    assert f.frames() == FRAMES
    out.append(f.get_taps())
    f.close()
    return out


def kalman(taps, with_y, then_reset=False):
    f = filters.KalmanBandsMC(3, 33, taps, p0=0.75)
    f.set_taps(0, weights(3, taps, 33))
    f.set_adapt(1, False)                                                  # one channel frozen
    out = run_pairs(f, 3, 3, 33, with_y, lambda x, d, e, y: f.process(*x, *d, *e, *(y or ())))
    assert f.frames() == FRAMES
    out += [f.get_taps(), f.get_variance(), f.get_noise()]
    if then_reset:                                                         # the variances back at p0: through the fill
        f.reset(True)
        out += [f.get_taps(), f.get_variance(), f.get_noise()]
    f.close()
    return out


def suppress(with_y, with_g):
    """two runs of 1 + 6 frames at a window of 4: the start-up and the swaps at frames 8 and 12"""
    f = filters.SuppressBandsMC(3, 33, window=4)
    f.set_enable(1, False)
    f.set_floor(0, [0.25, 0.5, 0.125])
    f.set_leak(0, [0.5, 1.0, 2.0])
    buf = Buffers(on_device=not with_y)
    e = [formula(k, 3, 2 * FRAMES, 33) for k in (0, 1)]
    y = [formula(k, 3, 2 * FRAMES, 33) for k in (2, 3)]
    out, m0 = [], 0
    for n in CALLS + CALLS:
        es = [buf.given(frames_of(a, m0, n)) for a in e]
        ys = [buf.given(frames_of(a, m0, n)) for a in y] if with_y else [None, None]
        o = [buf.empty(3, n, 33) for _ in range(2)]
        g = buf.empty(3, n, 33) if with_g else None
        f.process(*es, *o, *ys, g)
        out += [buf.host(b) for b in o + ([g] if with_g else [])]
        m0 += n
    assert f.frames() == 2 * FRAMES and f.plan()[0] == int(with_y)
    out += [f.get_state(s) for s in f.STATES]
    f.close()
    return out


CASES = {}
for _bins in (33, 64):
    for _taps in (1, 4, 5, 9, 17, 33, 64):
        for _y in (0, 1):
            CASES[f"nlms-bins{_bins}-taps{_taps}-y{_y}"] = (nlms, _bins, _taps, bool(_y))
for _inputs, _taps in ((1, 1), (3, 2), (3, 3), (2, 16), (8, 8)):
    for _y in (0, 1):
        CASES[f"matrix-inputs{_inputs}-taps{_taps}-y{_y}"] = (matrix, _inputs, _taps, bool(_y))
for _taps in (1, 4, 5, 9, 17, 32):
    for _y in (0, 1):
        CASES[f"kalman-taps{_taps}-y{_y}"] = (kalman, _taps, bool(_y))
CASES["kalman-taps5-y1-reset"] = (kalman, 5, True, True)
for _y in (0, 1):
    for _g in (0, 1):
        CASES[f"suppress-y{_y}-g{_g}"] = (suppress, bool(_y), bool(_g))

DIGESTS = {
    "nlms-bins33-taps1-y0": "ff2c57a7e59ec321e156c2f843ab0b05843a77ac403ede0b3e2607bd84a89a11",
    "nlms-bins33-taps1-y1": "b8f9f162f91649719a86e236fcf58346fc0b608dbd6d1801e3504f9c659f51af",
    "nlms-bins33-taps4-y0": "134cf6189a22933326fa1f711f4f41fc151b9e6accbc1bd686f06466cbf08f8f",
    "nlms-bins33-taps4-y1": "95969c8f7dfd028736d60d15781a85141b0017b4fd6fc9e9a0e12aaf0168edec",
    "nlms-bins33-taps5-y0": "806d0736a9960f3b1ea8da3a2383a12937c126e894a16951af82730abfe0c347",
    "nlms-bins33-taps5-y1": "cf7e0b1bd70c208b88c652c4433ecde29c7926de64fb48ea3f165c0394443aaa",
    "nlms-bins33-taps9-y0": "a11ba3d7c0d487d3d1950d5a70d979ce1a660a8a846a8ee661e4b900f8ad19c9",
    "nlms-bins33-taps9-y1": "8aa57aea5a36b43ced219809ae71fedf237fefcfbf5049ae551dea8a8a9a8037",
    "nlms-bins33-taps17-y0": "643976d7c6823889dedc59b61d44524f73e7b9fdac88076a84d139af114941e7",
    "nlms-bins33-taps17-y1": "e4a81c19103addf462e2552a44d6089b6312ccbf0aee0244bd0d9fe70bc64309",
    "nlms-bins33-taps33-y0": "a49bb04355bbc18a17160eacc8fbefdfdd84614549dc13a193edf0f4ae384787",
    "nlms-bins33-taps33-y1": "35ab476c65b62d54deabc23b754853d3649c5c927bc50af5c41b21b62276624a",
    "nlms-bins33-taps64-y0": "1e878c76a3a7af7bf10b3fcc9d9a5cd2dde80ebb353c59f5a3acad5e9878409a",
    "nlms-bins33-taps64-y1": "6aeb268961d2d310a649a1c4ade5d8ecbd89a97c7241c4347cc0cf6f9896f0f8",
    "nlms-bins64-taps1-y0": "ffb99b84231ba9b90335b90ef8fb0f37267c24d58b712dc7afffe97996bfb4a9",
    "nlms-bins64-taps1-y1": "501ec2a5824b08981443b137210e48be15fd7401348a7a7ef37a51f38c25b06d",
    "nlms-bins64-taps4-y0": "b337f0fb605eeb7cd411deb73fe4a36aee011620759d7a2786212c832a0a09f8",
    "nlms-bins64-taps4-y1": "74f09544956b6720c67313f55fc7c446a5a71aa51f66319e8f80ab011284b2d3",
    "nlms-bins64-taps5-y0": "3060fe6c625d84cd5bf1c782ac0adce8abe7167cedbe5790b6891e5fcb2d93fe",
    "nlms-bins64-taps5-y1": "127a50d4c3af6ef50870d80e51dd8f080da58b1e046d1e54eee780d4b246e150",
    "nlms-bins64-taps9-y0": "a2b0bbf468fe19bba80063993e1480cfa7cb24259594037128f49314f6f99728",
    "nlms-bins64-taps9-y1": "92ea4faea3e6ad9c86685b26e8fad1948d693935890c36659e4c182b26311e28",
    "nlms-bins64-taps17-y0": "c27d1b4d724d2f5a31869f5fd298968fa68eb7cda974d97b773b7145bb9a9274",
    "nlms-bins64-taps17-y1": "84aafb8cf4449a6f64ccdc7d0ad60adeeccba479b8b1d065da09c1ab593bbc40",
    "nlms-bins64-taps33-y0": "b3f9353ccc2a03a79245c0a068978db9193c5e2dad62bdf01e0b6a08b86c7750",
    "nlms-bins64-taps33-y1": "c7f91f51a89c9ac5b9646c9e2e60bfcc4130017b5c82161c88bdbd5ac1cdd9eb",
    "nlms-bins64-taps64-y0": "5aeb1436fb154cda8d8cfaf343ab2d711fe858419683d45af177c773f0a6cdd1",
    "nlms-bins64-taps64-y1": "058f558c2462c8d0a6ea7daecdc39e0d8a9d0b10682487e3637bb02965107c89",
    "matrix-inputs1-taps1-y0": "4690f8c40ee91d38156467bd20a3d8d98a55bc3b265a9b09405ba1a7e3b88f6e",
    "matrix-inputs1-taps1-y1": "b4c8f3c2e8ab8eecb5f842b303ef2d48141a48487402ad7b7fb7c303b2bf59c6",
    "matrix-inputs3-taps2-y0": "fcbc818efbaf60df222fbaef44d1ccf4f0b0caab2d224848d1a7a67e232739da",
    "matrix-inputs3-taps2-y1": "baf222d563cee45076768d300ae54df76eb22e248e2287a3d78fab7d3b9e44c8",
    "matrix-inputs3-taps3-y0": "d9dd9feb00c235002d67213fa330f1c739cf70b8df2fdc3a39abc6b2d145ba7d",
    "matrix-inputs3-taps3-y1": "01105006d2572d0b65a17557ac85bfd2642e16f88eef65b37a76ec3f91b80c03",
    "matrix-inputs2-taps16-y0": "a09edb01ffa129c8bf3f541dd56473ad1fdec68c7197c299c67c59b0be1d03fe",
    "matrix-inputs2-taps16-y1": "3c7c6458fce06de3504a31634acc368bd9cf4ed20853b22d708b92dc49fa510d",
    "matrix-inputs8-taps8-y0": "547132d270bdfbcb27ba99ce1aa347825613522bdd12647723ff050916a6bd6e",
    "matrix-inputs8-taps8-y1": "450958b4926449e4423983cb6499083f8adefc0f4a2383197c75f1d61395fff9",
    "kalman-taps1-y0": "f58c4254468571d5888098edc6dc85586107494ebda84e93e0fb12e30d0e9e57",
    "kalman-taps1-y1": "f510be00f2603ca91659cd9f36139fa89928f87141e897857c92c6f40945d1ad",
    "kalman-taps4-y0": "0812d69eb0cfd6cc1214384ecf93059f23afb4053c3fb93899c6eaa74c95aa05",
    "kalman-taps4-y1": "78870fbe961cc73071515985746a292743d75ecb90a74c4e4c5cdeb1adf0dfa6",
    "kalman-taps5-y0": "010c6c77096b67cfea073aae2938e56a14f6a1ee0bf7fca64abaddfab2855a5f",
    "kalman-taps5-y1": "ab06d3a72785992c7438fe9e85423608db39ab0987034170ddc71dfd02ecc58f",
    "kalman-taps9-y0": "92401573a93f1727994962da53bf9fd8bf3ac2d5ee2fde72e285d39b23ba7b80",
    "kalman-taps9-y1": "a8cd24f68e78d5613b8a49b903dcc37780db132237b816953bb11c11710cec04",
    "kalman-taps17-y0": "3141325e29ed1543a14198ca4e48b7d0990342441ca8366e4a0d1971318bba32",
    "kalman-taps17-y1": "06ec4c76f9d249d39b72d33c00cbd661f9af9c3f4c10f34b97785abff8ca91b5",
    "kalman-taps32-y0": "9f779a807da0f1a1574222565efc264cafbba63212259309e7fb22077d605b22",
    "kalman-taps32-y1": "eb2ddb480d04ae3fb5b748e654ab32b3170813ffd0f99b8a5797dfb11d4c5a34",
    "kalman-taps5-y1-reset": "3fed1692f04f518039a54d5f258cd637320d60e1f0fc8d3e121a55b85bfae8b4",
    "suppress-y0-g0": "69bf7c70398a026432b0fc5f3f3b7ee850b51d4f22b414c5c0053eb8a5b2191a",
    "suppress-y0-g1": "dade5530cb4a9703145c6c3f5da3d72d0cd84697e61ec3dbbb408aef92487b32",
    "suppress-y1-g0": "186a3ebe52a71ac772973b1053f165ae71a7f6d620adf69b06d5a6e165747e73",
    "suppress-y1-g1": "e2275d2a93cb029035f0c7a40abc7700042e412f00ec7d23b456994fc3596c20",
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert capi.lib().llz_hip_device_count() >= 1, capi.last_error()
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")


def test_every_case_has_a_digest():
    assert set(DIGESTS) == set(CASES) and len(CASES) == 28 + 10 + 13 + 4


@pytest.mark.parametrize("case", list(CASES))
def test_bits_are_the_parents(dev, case):
    fn, *args = CASES[case]
    got = digest(fn(*args))
    print(case, got)
    assert got == DIGESTS[case]


if __name__ == "__main__":
    torch.cuda.set_device(0)
    capi.check(capi.lib().llz_hip_set_device(0), "set_device")
    print("# library:", capi.LIB_PATH)
    for case, (fn, *args) in CASES.items():
        print(case, digest(fn(*args)), flush=True)
