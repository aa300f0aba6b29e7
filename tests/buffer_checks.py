"""Shared pieces of the buffer-contract tests (test_buffer_checks_host.py, test_buffer_contract_gpu.py): caller buffers carved
out of one flat allocation with a guard band on each side, at a chosen element offset from an allocator-aligned address, and
the checks that nothing outside a buffer was written and nothing inside an input was changed.  Plain numpy and torch; nothing
here opens a GPU by itself (a buffer lives wherever the `device` it is asked for says).

Why: a fresh torch tensor is 256-byte aligned, padded by the allocator and surrounded by memory nobody looks at, so a store a
few elements past a partial last tile, a read in front of a frame, or the unaligned side of a pointer-alignment branch all
pass a comparison of values.  Here

  * an OUTPUT buffer and both its bands hold a sentinel bit pattern: 0x7fc0dead for 4-byte types (a NaN with a payload, so a
    stray 0.0 or a plain NaN shows as a change), 0x5a5a for int16; every comparison is on the integer view, bit for bit;
  * an INPUT buffer holds its data between poisoned bands: a quiet NaN for floats (any use of it in a sum or a transform
    reaches the output), +max or -max-1 for integers (no NaN: such a case runs once with each, and the two results must be
    bit-identical);
  * GUARD = 16384 elements per band, the largest span a single workgroup here stores: two 8192-point blocks less the
    overlap per overlap-save job (13312 samples at most, fir_ols.hip), 8192 float32 of a 4096-point complex register
    transform (fft.hip), 4096 samples of PCM_TILE (pcm.hip).
"""
import numpy as np
import torch

GUARD = 16384
ALIGN = 256                      # bytes: what the device allocator gives a fresh tensor at the least
SENTINEL32 = 0x7FC0DEAD
SENTINEL16 = 0x5A5A
QNAN32 = 0x7FC00000              # numpy's / torch's default NaN

_INT_VIEW = {2: (torch.int16, np.uint16), 4: (torch.int32, np.uint32)}


def bits(t):
    """integer (numpy, unsigned) view of a tensor's elements, on the host"""
    tdt, ndt = _INT_VIEW[t.element_size()]
    return t.detach().contiguous().view(tdt).cpu().numpy().view(ndt)


def sentinel(dtype):
    size = torch.empty(0, dtype=dtype).element_size()
    if size not in _INT_VIEW:
        raise ValueError(f"no sentinel for {dtype}")
    return SENTINEL32 if size == 4 else SENTINEL16


def poison(dtype, which="nan"):
    """bit pattern of an input band: 'nan' (float types), 'max' or 'min' (integer types: +max, -max-1)"""
    if dtype.is_floating_point:
        assert which == "nan" and dtype == torch.float32, (dtype, which)
        return QNAN32
    assert which in ("max", "min"), (dtype, which)
    width = 8 * torch.empty(0, dtype=dtype).element_size()
    return (1 << (width - 1)) - 1 if which == "max" else 1 << (width - 1)


class Guarded:
    """`view`: the caller buffer ([numel], contiguous); `region`: front band, view, back band as one flat tensor;
    `band`: the bit pattern both bands were filled with"""

    def __init__(self, region, numel, guard, offset, band):
        self.region, self.numel, self.guard, self.offset, self.band = region, numel, guard, offset, band
        self.view = region[guard:guard + numel]

    def shaped(self, *shape):
        return self.view.view(*shape)

    def front(self):
        return self.region[:self.guard]

    def back(self):
        return self.region[self.guard + self.numel:]

    def host(self):
        """the view's elements on the host (a copy, numpy, in the buffer's own dtype)"""
        return self.view.detach().cpu().numpy().copy()


def _fill(t, pattern):
    tdt, _ = _INT_VIEW[t.element_size()]
    width = 8 * t.element_size()
    t.view(tdt).fill_(pattern - (1 << width) if pattern >= 1 << (width - 1) else pattern)


def carve(device, dtype, numel, offset, guard=GUARD):
    """An output buffer: one flat allocation, of which `view` is numel contiguous elements whose first element sits exactly
    `offset` elements past an ALIGN-byte aligned address, with `guard` elements on each side; bands and view hold the
    sentinel.  (Inputs: carve_input.)"""
    assert numel >= 1 and offset >= 0 and guard >= 1
    size = torch.empty(0, dtype=dtype).element_size()
    assert ALIGN % size == 0 and size in _INT_VIEW, dtype
    per = ALIGN // size
    flat = torch.empty(guard + numel + guard + offset + 2 * per, dtype=dtype, device=device)
    base = flat.data_ptr()
    assert base % size == 0
    # the smallest view start >= guard with (address of start - offset elements) on an ALIGN boundary
    first = (-(base // size) - guard + offset) % per + guard
    region = flat[first - guard:first + numel + guard]
    buf = Guarded(region, numel, guard, offset, sentinel(dtype))
    assert (buf.view.data_ptr() - offset * size) % ALIGN == 0 and buf.view.is_contiguous()
    _fill(region, buf.band)
    return buf


def carve_input(device, data, offset, guard=GUARD, which="nan"):
    """An input buffer holding `data` (numpy, any shape; flattened) between bands of poison(dtype, which)"""
    data = np.ascontiguousarray(data)
    src = torch.from_numpy(data.reshape(-1))
    buf = carve(device, src.dtype, src.numel(), offset, guard)
    buf.band = poison(src.dtype, which)
    _fill(buf.region, buf.band)
    buf.view.copy_(src)
    return buf


def _changed(side, got, want_bits, index_of):
    bad = np.flatnonzero(got != want_bits)
    if bad.size == 0:
        return None
    first = int(bad[0])
    return (f"{side}: {bad.size} element(s) changed, the first at index {index_of(first)} relative to the buffer "
            f"(now 0x{int(got[first]):x}, was 0x{int(np.broadcast_to(want_bits, got.shape)[first]):x})")


def band_report(buf):
    """None, or what changed in the bands: side, count, index of the first changed element relative to the view (negative
    in front of it, >= numel behind it)"""
    msgs = [_changed("front band", bits(buf.front()), buf.band, lambda i: i - buf.guard),
            _changed("back band", bits(buf.back()), buf.band, lambda i: buf.numel + i)]
    msgs = [m for m in msgs if m]
    return "; ".join(msgs) if msgs else None


def check_bands(buf, what="buffer"):
    """both bands still hold their fill, bit for bit"""
    msg = band_report(buf)
    assert msg is None, f"{what}: written outside the buffer: {msg}"


def snapshot(buf):
    """bits of the whole region (bands and view), for check_untouched after the call"""
    return bits(buf.region).copy()


def untouched_report(buf, snap):
    return _changed("input", bits(buf.region), snap, lambda i: i - buf.guard)


def check_untouched(buf, snap, what="input"):
    """for inputs: view and both bands bit-identical to the snapshot taken before the call"""
    msg = untouched_report(buf, snap)
    assert msg is None, f"{what}: an input buffer was written: {msg}"


def check_all_written(buf, what="output"):
    """no element of an output still holds the sentinel (every element was stored); returns the host copy"""
    left = np.flatnonzero(bits(buf.view) == buf.band)
    assert left.size == 0, f"{what}: {left.size} element(s) never written, the first at index {int(left[0])}"
    return buf.host()


def overlap_cases(numel, out_numel=None, device="cpu", dtype=torch.float32):
    """[(in, out)] x 3 over ONE allocation: exact alias, out one element after in, out starting inside the last quarter of
    in.  in has numel elements, out out_numel (default numel); the allocation holds the sentinel (compare bits(in) and
    bits(out) before and after a refused call)."""
    out_numel = numel if out_numel is None else out_numel
    assert numel >= 8
    inside = numel - max(1, numel // 8)
    assert numel - numel // 4 <= inside < numel
    whole = carve(device, dtype, numel + out_numel, 0, guard=64)
    return [(whole.view[:numel], whole.view[start:start + out_numel]) for start in (0, 1, inside)]
