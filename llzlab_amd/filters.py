"""Python mirror of the reference's handle interface (init / process / flush / uninit) over the C ABI.

Names and argument meaning follow reference libllzfilter/llz_{fir,iir,resample,fft,fft_fixed}.h; the *MC classes
are the multi-channel float32/int16 batch extension.  Device buffers are torch tensors (used for memory and
streams only: `tensor.data_ptr()` crosses the boundary as a plain pointer); numpy arrays are accepted as host
memory.  Nothing here computes: every sample goes through libllzfilter_hip.so.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import (BAD_HANDLE, BLACKMAN, FIR_ALGO_AUTO, FIR_ALGO_OVERLAP_SAVE, FIR_ALGO_OVERLAP_SAVE_2048, FIR_ALGO_OVERLAP_SAVE_4096, FIR_ALGO_OVERLAP_SAVE_8192, FIR_ALGO_PARTITIONED, FIR_ALGO_TIME,  # noqa: F401
                   FIR_ALGO_TIME_MFMA, HAMMING, KAISER,
                   PCM_F32, PCM_I16, PCM_I16_FAST, PFB_PHASE_FRAME, PFB_PHASE_TIME, LlzError, check, check_handle)


def _ptr(buf):
    """Plain address of a torch tensor (any device) or a numpy array; the library sorts host from device."""
    if isinstance(buf, np.ndarray):
        if not buf.flags["C_CONTIGUOUS"]:
            raise LlzError("numpy buffer must be C-contiguous")
        return buf.ctypes.data
    if hasattr(buf, "data_ptr"):
        if not buf.is_contiguous():
            raise LlzError("tensor must be contiguous")
        return buf.data_ptr()
    raise LlzError(f"unsupported buffer type {type(buf)}")


def _typed(buf, dtype, numel, what):
    """address of `buf` after checking that it holds exactly `numel` elements of `dtype` ("float32", "int16", ...): the C
    ABI takes plain pointers, so a wrong dtype or a short buffer would be read / written past its end"""
    name = str(buf.dtype).replace("torch.", "")
    size = buf.numel() if hasattr(buf, "numel") else buf.size
    if name != dtype or size != numel:
        raise LlzError(f"{what}: expected {numel} x {dtype}, got {size} x {name}")
    return _ptr(buf)


def _stream_ptr(stream):
    if stream is None:
        return None
    return getattr(stream, "cuda_stream", stream)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


_dp = C.POINTER(C.c_double)


# ------------------------------------------------------------------------------------------ design (host C)
def fir_design(kind, n, fc1, fc2=0.0, win=HAMMING):
    """kind: 'lpf' | 'hpf' | 'bandpass' | 'bandstop' -> float64 taps from llz_fir_*_cof (host C code)."""
    L = capi.lib()
    hp = _dp()
    if kind == "lpf":
        m = L.llz_fir_lpf_cof(C.byref(hp), n, fc1, win)
    elif kind == "hpf":
        m = L.llz_fir_hpf_cof(C.byref(hp), n, fc1, win)
    elif kind == "bandpass":
        m = L.llz_fir_bandpass_cof(C.byref(hp), n, fc1, fc2, win)
    elif kind == "bandstop":
        m = L.llz_fir_bandstop_cof(C.byref(hp), n, fc1, fc2, win)
    else:
        raise LlzError("unknown filter kind " + kind)
    if m < 1:
        raise LlzError("tap design failed")
    taps = np.ctypeslib.as_array(hp, shape=(m,)).copy()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(hp)                       # the caller owns *h (reference llz_fir.h:82-86)
    return taps


def window(win, n, beta=None):
    L = capi.lib()
    w = np.zeros(n)
    p = w.ctypes.data_as(_dp)
    if beta is not None:
        L.llz_kaiser_beta(p, n, beta)
    else:
        (L.llz_hamming, L.llz_blackman, L.llz_kaiser)[win](p, n)
    return w


# ------------------------------------------------------------------------------------------ FIR
class FirFilter:
    """Single channel, double, host buffers: llz_fir_filter_{lpf,hpf,bandpass,bandstop}_init & co."""

    def __init__(self, kind, frame_len, flt_len, fc1, fc2=0.0, win=HAMMING):
        L = self._L = capi.lib()
        if kind == "lpf":
            h = L.llz_fir_filter_lpf_init(frame_len, flt_len, fc1, win)
        elif kind == "hpf":
            h = L.llz_fir_filter_hpf_init(frame_len, flt_len, fc1, win)
        elif kind == "bandpass":
            h = L.llz_fir_filter_bandpass_init(frame_len, flt_len, fc1, fc2, win)
        elif kind == "bandstop":
            h = L.llz_fir_filter_bandstop_init(frame_len, flt_len, fc1, fc2, win)
        else:
            raise LlzError("unknown filter kind " + kind)
        self.handle = check_handle(h, "llz_fir_filter_*_init")
        self.frame_len = frame_len
        self.flt_len = flt_len if kind == "lpf" or flt_len & 1 else flt_len + 1

    def filter(self, x):
        x = _f64(x)
        y = np.zeros_like(x)
        check(self._L.llz_fir_filter(self.handle, x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), len(x)),
              "llz_fir_filter")
        return y

    def flush(self):
        y = np.zeros(max(self.flt_len - 1, 1))
        n = check(self._L.llz_fir_filter_flush(self.handle, y.ctypes.data_as(_dp)), "llz_fir_filter_flush")
        return y[:n]

    def close(self):
        if self.handle:
            self._L.llz_fir_filter_uninit(self.handle)
            self.handle = 0

    __del__ = close


class FirFilterMC:
    """channels x frame_len float32, planar; llz_fir_filter_mc_*."""

    def __init__(self, channels, frame_len, taps, algo=FIR_ALGO_AUTO, stream=None):
        self._L = capi.lib()
        taps = _f64(taps)
        self.handle = check_handle(
            self._L.llz_fir_filter_mc_init_f64taps(channels, frame_len, taps.ctypes.data, len(taps), algo),
            "llz_fir_filter_mc_init")
        self.channels, self.frame_len, self.flt_len = channels, frame_len, len(taps)
        self.algo = self._L.llz_fir_filter_mc_algo(self.handle)
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        check(self._L.llz_fir_filter_mc_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def partition_plan(self, n):
        """FIR_ALGO_PARTITIONED only: (transform points, partitions, channels per pass, passes) of a call of n samples under
        the tunes set now (llz_fir_filter_mc_partition_plan; nothing is launched)"""
        out = (C.c_int * 4)()
        check(self._L.llz_fir_filter_mc_partition_plan(self.handle, int(n), out), "llz_fir_filter_mc_partition_plan")
        return tuple(out)

    def real_rows(self):
        """FIR_ALGO_OVERLAP_SAVE: the K of the real spectrum product the next call takes under the tunes set now (taps symmetric
        about tap 32 K, K = 1..4), 0 for the complex product (llz_fir_filter_mc_real_rows; nothing is launched)"""
        return check(self._L.llz_fir_filter_mc_real_rows(self.handle), "llz_fir_filter_mc_real_rows")

    def filter(self, x, out):
        """x, out: [channels, frame_len] float32 (torch device tensors or numpy). Returns out."""
        count = self.channels * self.frame_len
        check(self._L.llz_fir_filter_mc(self.handle, _typed(x, "float32", count, "FirFilterMC.filter x"),
                                        _typed(out, "float32", count, "FirFilterMC.filter out"), self.frame_len),
              "llz_fir_filter_mc")
        return out

    def flush(self, out):
        check(self._L.llz_fir_filter_mc_flush(self.handle, _typed(out, "float32", self.channels * (self.flt_len - 1),
                                                                  "FirFilterMC.flush out")), "llz_fir_filter_mc_flush")
        return out

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_fir_filter_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class FirBankMC:
    """channels x frame_len float32, planar, one tap set per channel: llz_fir_bank_mc_*.  taps: [channels, flt_len].
    algo=FIR_ALGO_PARTITIONED is the partitioned bank (1..131073 taps, llz_fir_pbank_mc_init); every call but the init and
    partition_plan is the bank's."""

    def __init__(self, channels, frame_len, taps, algo=FIR_ALGO_AUTO, stream=None):
        self._L = capi.lib()
        taps = _f64(taps)
        if taps.ndim != 2 or taps.shape[0] != channels or taps.shape[1] < 1:
            raise LlzError(f"FirBankMC: taps must be [channels = {channels}, flt_len], got {taps.shape} "
                           "(one tap set for every channel is FirFilterMC)")
        if algo == FIR_ALGO_PARTITIONED:
            self.handle = check_handle(
                self._L.llz_fir_pbank_mc_init_f64taps(channels, frame_len, taps.ctypes.data, taps.shape[1]),
                "llz_fir_pbank_mc_init")
        else:
            self.handle = check_handle(
                self._L.llz_fir_bank_mc_init_f64taps(channels, frame_len, taps.ctypes.data, taps.shape[1], algo),
                "llz_fir_bank_mc_init")
        self.channels, self.frame_len, self.flt_len = channels, frame_len, taps.shape[1]
        self.algo = self._L.llz_fir_bank_mc_algo(self.handle)
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        check(self._L.llz_fir_bank_mc_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def partition_plan(self, n):
        """(transform points, partitions, channels per pass, passes) of a call of n samples on a partitioned bank under the
        tunes set now (llz_fir_pbank_mc_plan; nothing is launched)"""
        out = (C.c_int * 4)()
        check(self._L.llz_fir_pbank_mc_plan(self.handle, int(n), out), "llz_fir_pbank_mc_plan")
        return tuple(out)

    def set_taps(self, first, taps):
        """replace the taps of channels first .. first + len(taps) - 1; taps: [count, flt_len]"""
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        if taps.ndim != 2 or taps.shape[1] != self.flt_len:
            raise LlzError(f"FirBankMC.set_taps: taps must be [count, flt_len = {self.flt_len}], got {taps.shape}")
        check(self._L.llz_fir_bank_mc_set_taps(self.handle, first, taps.shape[0], taps.ctypes.data),
              "llz_fir_bank_mc_set_taps")

    def filter(self, x, out):
        """x, out: [channels, frame_len] float32 (torch device tensors or numpy). Returns out."""
        count = self.channels * self.frame_len
        check(self._L.llz_fir_bank_mc(self.handle, _typed(x, "float32", count, "FirBankMC.filter x"),
                                      _typed(out, "float32", count, "FirBankMC.filter out"), self.frame_len),
              "llz_fir_bank_mc")
        return out

    def flush(self, out):
        check(self._L.llz_fir_bank_mc_flush(self.handle, _typed(out, "float32", self.channels * (self.flt_len - 1),
                                                                "FirBankMC.flush out")), "llz_fir_bank_mc_flush")
        return out

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_fir_bank_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class FirStreamMC:
    """channels x frame_len float32, planar, frame_len = k x block: llz_fir_stream_mc_*, the block convolver that keeps the
    spectra of its input between calls (short blocks against long filters).  taps: 1-D (one tap set for all channels) or
    [channels, flt_len] (a tap set per channel).  frame_len defaults to block."""

    def __init__(self, channels, block, taps, frame_len=None, stream=None):
        self._L = capi.lib()
        taps = _f64(taps)
        if taps.ndim not in (1, 2) or taps.shape[-1] < 1 or (taps.ndim == 2 and taps.shape[0] != channels):
            raise LlzError(f"FirStreamMC: taps must be [flt_len] or [channels = {channels}, flt_len], got {taps.shape}")
        frame_len = block if frame_len is None else frame_len
        self.rows = 1 if taps.ndim == 1 else channels
        self.handle = check_handle(
            self._L.llz_fir_stream_mc_init_f64taps(channels, block, frame_len, taps.ctypes.data, self.rows, taps.shape[-1]),
            "llz_fir_stream_mc_init")
        self.channels, self.block, self.frame_len, self.flt_len = channels, block, frame_len, taps.shape[-1]
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        check(self._L.llz_fir_stream_mc_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def plan(self):
        """(N = 2 block, partitions P, ring slots R, blocks per call k)"""
        out = (C.c_int * 4)()
        check(self._L.llz_fir_stream_mc_plan(self.handle, out), "llz_fir_stream_mc_plan")
        return tuple(out)

    def set_taps(self, first, taps):
        """replace tap rows first .. first + count - 1; taps: [count, flt_len], or [flt_len] for one row"""
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        taps = taps[None, :] if taps.ndim == 1 else taps
        if taps.ndim != 2 or taps.shape[1] != self.flt_len:
            raise LlzError(f"FirStreamMC.set_taps: taps must be [count, flt_len = {self.flt_len}], got {taps.shape}")
        check(self._L.llz_fir_stream_mc_set_taps(self.handle, first, taps.shape[0], taps.ctypes.data),
              "llz_fir_stream_mc_set_taps")

    def fade_taps(self, first, taps, blocks):
        """fade tap rows first .. first + count - 1 to `taps` ([count, flt_len], or [flt_len] for one row) over the next
        `blocks` blocks, 1 .. 4096: a linear per-sample crossfade between the old and the new filter's outputs
        (llz_fir_xfade_stream_mc).  Until the first of those blocks has run, further calls with the same `blocks` add rows"""
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        taps = taps[None, :] if taps.ndim == 1 else taps
        if taps.ndim != 2 or taps.shape[1] != self.flt_len:
            raise LlzError(f"FirStreamMC.fade_taps: taps must be [count, flt_len = {self.flt_len}], got {taps.shape}")
        check(self._L.llz_fir_xfade_stream_mc(self.handle, first, taps.shape[0], taps.ctypes.data, blocks),
              "llz_fir_xfade_stream_mc")

    def fade_left(self):
        """blocks of the fade still to run; 0: none in flight"""
        return check(self._L.llz_fir_xfade_stream_mc_left(self.handle), "llz_fir_xfade_stream_mc_left")

    def filter(self, x, out):
        """x, out: [channels, frame_len] float32 (torch device tensors or numpy). Returns out."""
        count = self.channels * self.frame_len
        check(self._L.llz_fir_stream_mc(self.handle, _typed(x, "float32", count, "FirStreamMC.filter x"),
                                        _typed(out, "float32", count, "FirStreamMC.filter out"), self.frame_len),
              "llz_fir_stream_mc")
        return out

    def flush(self, out):
        """out: [channels, flt_len - 1]; the handle starts over afterwards.  With one tap there is nothing to emit: out is an
        empty buffer or None, and the call only resets the handle"""
        ptr = None
        if self.flt_len > 1 or out is not None:
            ptr = _typed(out, "float32", self.channels * (self.flt_len - 1), "FirStreamMC.flush out")
        check(self._L.llz_fir_stream_mc_flush(self.handle, ptr), "llz_fir_stream_mc_flush")
        return out

    def reset(self):
        check(self._L.llz_fir_stream_mc_reset(self.handle), "llz_fir_stream_mc_reset")

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_fir_stream_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class AdaptMC:
    """channels x frame_len float32, planar, frame_len = k x block: llz_adapt_mc_*, the partitioned frequency-domain NLMS
    adaptive filter (include/llz_adapt.h) -- the stream convolver's delay line with an error, a normalised gradient and a
    constrained weight update per block.  The weights start at zero; mu is every channel's step size (0 = frozen), delta the
    regularisation of the power (None: 1e-3 x block).  frame_len defaults to block and is the longest call."""

    def __init__(self, channels, block, flt_len, frame_len=None, mu=0.5, delta=None, stream=None):
        self._L = capi.lib()
        frame_len = block if frame_len is None else frame_len
        delta = 1e-3 * block if delta is None else delta
        self.handle = check_handle(self._L.llz_adapt_mc_init(channels, block, frame_len, flt_len, mu, delta), "llz_adapt_mc_init")
        self.channels, self.block, self.frame_len, self.flt_len = channels, block, frame_len, flt_len
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        check(self._L.llz_adapt_mc_set_stream(self.handle, _stream_ptr(stream)), "llz_adapt_mc_set_stream")

    def plan(self):
        """(N = 2 block, partitions P, ring slots R, blocks per call k)"""
        out = (C.c_int * 4)()
        check(self._L.llz_adapt_mc_plan(self.handle, out), "llz_adapt_mc_plan")
        return tuple(out)

    def process(self, x, d, e, y=None):
        """x (reference), d (desired), e (error, written), y (filter output, written when given): [channels, n] float32 with n
        a multiple of block up to frame_len (torch device tensors or numpy).  Returns e."""
        n = (x.numel() if hasattr(x, "numel") else x.size) // self.channels
        count = self.channels * n
        check(self._L.llz_adapt_mc(self.handle, _typed(x, "float32", count, "AdaptMC.process x"),
                                   _typed(d, "float32", count, "AdaptMC.process d"),
                                   _typed(e, "float32", count, "AdaptMC.process e"),
                                   None if y is None else _typed(y, "float32", count, "AdaptMC.process y"), n), "llz_adapt_mc")
        return e

    def set_step(self, first, mu):
        """step sizes of channels first .. first + count - 1: [count] values in [0, 2] (or one number), 0 = frozen"""
        mu = np.ascontiguousarray(np.atleast_1d(mu), dtype=np.float32)
        check(self._L.llz_adapt_mc_set_step(self.handle, first, mu.shape[0], mu.ctypes.data), "llz_adapt_mc_set_step")

    def set_taps(self, first, taps):
        """replace the weights of channels first .. first + count - 1; taps: [count, flt_len], or [flt_len] for one channel"""
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        taps = taps[None, :] if taps.ndim == 1 else taps
        if taps.ndim != 2 or taps.shape[1] != self.flt_len:
            raise LlzError(f"AdaptMC.set_taps: taps must be [count, flt_len = {self.flt_len}], got {taps.shape}")
        check(self._L.llz_adapt_mc_set_taps(self.handle, first, taps.shape[0], taps.ctypes.data), "llz_adapt_mc_set_taps")

    def get_taps(self, first=0, count=None):
        """the weights of channels first .. first + count - 1 (default: all from first) as [count, flt_len] float32"""
        count = self.channels - first if count is None else count
        taps = np.empty((max(count, 0), self.flt_len), dtype=np.float32)
        check(self._L.llz_adapt_mc_get_taps(self.handle, first, count, taps.ctypes.data), "llz_adapt_mc_get_taps")
        return taps

    def reset(self, clear_taps=False):
        check(self._L.llz_adapt_mc_reset(self.handle, 1 if clear_taps else 0), "llz_adapt_mc_reset")

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_adapt_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class FirMatrixMC:
    """[inputs, frame_len] -> [outputs, frame_len] float32, planar, frame_len = k x block: llz_fir_matrix_mc_*, the stream
    convolver with a filter per path, y_o = sum_i x_i * h[o, i].  taps: [outputs, inputs, flt_len]; a path whose taps are all
    zero is not connected (it costs nothing and passes nothing on).  frame_len defaults to block."""

    def __init__(self, inputs, outputs, block, taps, frame_len=None, stream=None):
        self._L = capi.lib()
        taps = _f64(taps)
        if taps.ndim != 3 or taps.shape[:2] != (outputs, inputs) or taps.shape[2] < 1:
            raise LlzError(f"FirMatrixMC: taps must be [outputs = {outputs}, inputs = {inputs}, flt_len], got {taps.shape}")
        frame_len = block if frame_len is None else frame_len
        self.handle = check_handle(
            self._L.llz_fir_matrix_mc_init_f64taps(inputs, outputs, block, frame_len, taps.ctypes.data, taps.shape[2]),
            "llz_fir_matrix_mc_init")
        self.inputs, self.outputs, self.block, self.frame_len, self.flt_len = inputs, outputs, block, frame_len, taps.shape[2]
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        check(self._L.llz_fir_matrix_mc_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def plan(self):
        """(N = 2 block, partitions P, ring slots R, blocks per call k, input groups G, connected paths)"""
        out = (C.c_int * 6)()
        check(self._L.llz_fir_matrix_mc_plan(self.handle, out), "llz_fir_matrix_mc_plan")
        return tuple(out)

    def set_taps(self, out_first, in_first, taps):
        """replace the paths [out_first, +out_count) x [in_first, +in_count); taps: [out_count, in_count, flt_len], or [flt_len]
        for one path"""
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        taps = taps[None, None, :] if taps.ndim == 1 else taps
        if taps.ndim != 3 or taps.shape[2] != self.flt_len:
            raise LlzError(f"FirMatrixMC.set_taps: taps must be [out_count, in_count, flt_len = {self.flt_len}], got {taps.shape}")
        check(self._L.llz_fir_matrix_mc_set_taps(self.handle, out_first, taps.shape[0], in_first, taps.shape[1], taps.ctypes.data),
              "llz_fir_matrix_mc_set_taps")

    def fade_taps(self, out_first, in_first, taps, blocks):
        """fade the paths [out_first, +out_count) x [in_first, +in_count) to `taps` ([out_count, in_count, flt_len], or [flt_len]
        for one path) over the next `blocks` blocks, 1 .. 4096: a linear per-sample crossfade between the old and the new
        matrix's outputs, per output after the sum over inputs (llz_fir_xfade_matrix_mc).  Until the first of those blocks has
        run, further calls with the same `blocks` add paths"""
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        taps = taps[None, None, :] if taps.ndim == 1 else taps
        if taps.ndim != 3 or taps.shape[2] != self.flt_len:
            raise LlzError(f"FirMatrixMC.fade_taps: taps must be [out_count, in_count, flt_len = {self.flt_len}], got {taps.shape}")
        check(self._L.llz_fir_xfade_matrix_mc(self.handle, out_first, taps.shape[0], in_first, taps.shape[1], taps.ctypes.data,
                                              blocks), "llz_fir_xfade_matrix_mc")

    def fade_left(self):
        """blocks of the fade still to run; 0: none in flight"""
        return check(self._L.llz_fir_xfade_matrix_mc_left(self.handle), "llz_fir_xfade_matrix_mc_left")

    def filter(self, x, out):
        """x: [inputs, frame_len], out: [outputs, frame_len] float32 (torch device tensors or numpy). Returns out."""
        check(self._L.llz_fir_matrix_mc(self.handle, _typed(x, "float32", self.inputs * self.frame_len, "FirMatrixMC.filter x"),
                                        _typed(out, "float32", self.outputs * self.frame_len, "FirMatrixMC.filter out"),
                                        self.frame_len), "llz_fir_matrix_mc")
        return out

    def flush(self, out):
        """out: [outputs, flt_len - 1]; the handle starts over afterwards.  With one tap there is nothing to emit: out is an
        empty buffer or None, and the call only resets the handle"""
        ptr = None
        if self.flt_len > 1 or out is not None:
            ptr = _typed(out, "float32", self.outputs * (self.flt_len - 1), "FirMatrixMC.flush out")
        check(self._L.llz_fir_matrix_mc_flush(self.handle, ptr), "llz_fir_matrix_mc_flush")
        return out

    def reset(self):
        check(self._L.llz_fir_matrix_mc_reset(self.handle), "llz_fir_matrix_mc_reset")

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_fir_matrix_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class AdaptMatrixMC:
    """x [inputs, n], d / e / y [outputs, n] float32, planar, n a multiple of block up to frame_len: llz_adapt_matrix_mc_*, the
    multi-reference frequency-domain NLMS adaptive filter (include/llz_adapt_matrix.h) -- the matrix convolver's delay lines with
    a weight set per path (o, i), the error of output o driving all of its paths, normalised by the joint power of all
    references.  The weights start at zero; mu is every output's step size (0 = frozen), delta the regularisation of the power
    (None: 1e-3 x block x inputs).  frame_len defaults to block and is the longest call."""

    def __init__(self, inputs, outputs, block, flt_len, frame_len=None, mu=0.5, delta=None, stream=None):
        self._L = capi.lib()
        frame_len = block if frame_len is None else frame_len
        delta = 1e-3 * block * inputs if delta is None else delta
        self.handle = check_handle(self._L.llz_adapt_matrix_mc_init(inputs, outputs, block, frame_len, flt_len, mu, delta),
                                   "llz_adapt_matrix_mc_init")
        self.inputs, self.outputs, self.block, self.frame_len, self.flt_len = inputs, outputs, block, frame_len, flt_len
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        check(self._L.llz_adapt_matrix_mc_set_stream(self.handle, _stream_ptr(stream)), "llz_adapt_matrix_mc_set_stream")

    def plan(self):
        """(N = 2 block, partitions P, ring slots R, blocks per call k, input groups G, inputs per group)"""
        out = (C.c_int * 6)()
        check(self._L.llz_adapt_matrix_mc_plan(self.handle, out), "llz_adapt_matrix_mc_plan")
        return tuple(out)

    def process(self, x, d, e, y=None):
        """x (references): [inputs, n]; d (desired), e (error, written), y (filter output, written when given): [outputs, n]
        float32 (torch device tensors or numpy).  Returns e."""
        n = (x.numel() if hasattr(x, "numel") else x.size) // self.inputs
        count = self.outputs * n
        check(self._L.llz_adapt_matrix_mc(self.handle, _typed(x, "float32", self.inputs * n, "AdaptMatrixMC.process x"),
                                          _typed(d, "float32", count, "AdaptMatrixMC.process d"),
                                          _typed(e, "float32", count, "AdaptMatrixMC.process e"),
                                          None if y is None else _typed(y, "float32", count, "AdaptMatrixMC.process y"), n),
              "llz_adapt_matrix_mc")
        return e

    def set_step(self, out_first, mu):
        """step sizes of outputs out_first .. out_first + count - 1: [count] values in [0, 2] (or one number), 0 = frozen"""
        mu = np.ascontiguousarray(np.atleast_1d(mu), dtype=np.float32)
        check(self._L.llz_adapt_matrix_mc_set_step(self.handle, out_first, mu.shape[0], mu.ctypes.data),
              "llz_adapt_matrix_mc_set_step")

    def set_taps(self, out_first, in_first, taps):
        """replace the weights of the paths [out_first, +out_count) x [in_first, +in_count); taps: [out_count, in_count,
        flt_len], or [flt_len] for one path"""
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        taps = taps[None, None, :] if taps.ndim == 1 else taps
        if taps.ndim != 3 or taps.shape[2] != self.flt_len:
            raise LlzError(f"AdaptMatrixMC.set_taps: taps must be [out_count, in_count, flt_len = {self.flt_len}], got {taps.shape}")
        check(self._L.llz_adapt_matrix_mc_set_taps(self.handle, out_first, taps.shape[0], in_first, taps.shape[1],
                                                   taps.ctypes.data), "llz_adapt_matrix_mc_set_taps")

    def get_taps(self, out_first=0, out_count=None, in_first=0, in_count=None):
        """the weights of the paths [out_first, +out_count) x [in_first, +in_count) (default: all from the firsts) as
        [out_count, in_count, flt_len] float32: what FirMatrixMC takes"""
        out_count = self.outputs - out_first if out_count is None else out_count
        in_count = self.inputs - in_first if in_count is None else in_count
        taps = np.empty((max(out_count, 0), max(in_count, 0), self.flt_len), dtype=np.float32)
        check(self._L.llz_adapt_matrix_mc_get_taps(self.handle, out_first, out_count, in_first, in_count, taps.ctypes.data),
              "llz_adapt_matrix_mc_get_taps")
        return taps

    def reset(self, clear_taps=False):
        check(self._L.llz_adapt_matrix_mc_reset(self.handle, 1 if clear_taps else 0), "llz_adapt_matrix_mc_reset")

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_adapt_matrix_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class _BandsFilter:
    """What the per-band classes share: the calls every llz_*_bands_*_mc family has (_P is its C prefix, _PLAN the length of
    its plan), the typed pointers of process and the complex [..., taps, bins] weights of set_taps / get_taps.  Messages carry
    the name of the class that was called."""
    _P = None
    _PLAN = 4

    def _call(self, name, *args):
        check(getattr(self._L, self._P + name)(self.handle, *args), self._P + name)

    def _open(self, stream, *args):
        self._L = capi.lib()
        self.handle = check_handle(getattr(self._L, self._P + "_init")(*args), self._P + "_init")
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        self._call("_set_stream", _stream_ptr(stream))

    def plan(self):
        """the launch of a call: what names the kernel instance (see the class), then threads per workgroup, workgroups and
        launches per call"""
        out = (C.c_int * self._PLAN)()
        self._call("_plan", out)
        return tuple(out)

    def frames(self):
        """frames taken since init or reset"""
        n = C.c_longlong()
        self._call("_frames", C.byref(n))
        return n.value

    def close(self):
        if getattr(self, "handle", 0):
            getattr(self._L, self._P + "_uninit")(self.handle)
            self.handle = 0

    __del__ = close

    def _frames_in(self, buf, rows):
        return (buf.numel() if hasattr(buf, "numel") else buf.size) // (rows * self.bins)

    def _process(self, frames, bufs):
        """the call itself; bufs: (name, buffer or None, rows) in the C call's order, each [rows, frames, bins] float32"""
        who = type(self).__name__ + ".process "
        ptrs = [None if b is None else _typed(b, "float32", rows * frames * self.bins, who + name) for name, b, rows in bufs]
        self._call("", *ptrs, frames)

    def _process_xdey(self, x_re, x_im, d_re, d_im, e_re, e_im, y_re, y_im):
        self._both_or_neither(y_re, y_im)
        rows = self.channels
        self._process(self._frames_in(x_re, rows), [("x_re", x_re, rows), ("x_im", x_im, rows), ("d_re", d_re, rows),
                                                    ("d_im", d_im, rows), ("e_re", e_re, rows), ("e_im", e_im, rows),
                                                    ("y_re", y_re, rows), ("y_im", y_im, rows)])
        return e_re, e_im

    def _process_pairs(self, x, d, e, y):
        """the call of the multi-reference classes: x [inputs, ...], d, e and an optional y [outputs, ...], each a pair (re, im)"""
        pairs = [("x", x, self.inputs), ("d", d, self.outputs), ("e", e, self.outputs)] + ([("y", y, self.outputs)] if y is not None else [])
        for name, p, _ in pairs:
            if not isinstance(p, (tuple, list)) or len(p) != 2:
                raise LlzError(f"{type(self).__name__}.process: {name} must be a pair (re, im)")
        bufs = [(f"{name}_{part}", b, rows) for name, p, rows in pairs for part, b in zip(("re", "im"), p)]
        self._process(self._frames_in(x[0], self.inputs), bufs + [("y", None, 0)] * (8 - len(bufs)))
        return e

    def _both_or_neither(self, y_re, y_im):
        if (y_re is None) != (y_im is None):
            raise LlzError(f"{type(self).__name__}.process: y_re and y_im must both be given or both be None")

    def _rows(self, a, what, must, lead=1):
        """a when it is [lead dimensions..., taps, bins]; else the error '<class>.<what>: <must>, taps = .., bins = ..], got ..'"""
        if a.ndim != lead + 2 or a.shape[lead:] != (self.taps, self.bins):
            raise LlzError(f"{type(self).__name__}.{what}: {must}, taps = {self.taps}, bins = {self.bins}], got {a.shape}")
        return a

    def _set_taps(self, w, *where):
        """complex weights up as a float32 re and im array; where: the C call's arguments between the handle and the arrays"""
        wre, wim = np.ascontiguousarray(w.real, dtype=np.float32), np.ascontiguousarray(w.imag, dtype=np.float32)
        self._call("_set_taps", *where, wre.ctypes.data, wim.ctypes.data)

    def _get_taps(self, lead, *where):
        """the weights [*lead, taps, bins] as complex64: the handle's own float32 values"""
        wre = np.empty(tuple(max(n, 0) for n in lead) + (self.taps, self.bins), dtype=np.float32)
        wim = np.empty_like(wre)
        self._call("_get_taps", *where, wre.ctypes.data, wim.ctypes.data)
        w = np.empty(wre.shape, dtype=np.complex64)
        w.real, w.imag = wre, wim
        return w

    def _get_rows(self, name, first, count, *tail):
        """float32 [count, *tail] of channels first .. first + count - 1 (count None: all from first) from the getter `name`"""
        count = self.channels - first if count is None else count
        out = np.empty((max(count, 0),) + tail, dtype=np.float32)
        self._call(name, first, count, out.ctypes.data)
        return out

    def _set_rows(self, name, first, values, dtype):
        v = np.ascontiguousarray(values, dtype=dtype)
        self._call(name, first, v.shape[0], v.ctypes.data)


class AdaptBandsMC(_BandsFilter):
    """band signals [channels, frames, bins] float32, re and im apart (StftMC's and PfbMC's layout): llz_adapt_bands_mc_*, a
    normalised LMS filter of `taps` complex taps for every (channel, bin), updated frame by frame (include/llz_adapt_bands.h) --
    the step between a bank's analysis of x and d and its synthesis of e in a subband echo canceller.  The weights start at zero;
    mu is every channel's step size (0 = frozen), delta the regularisation of the power (None: 1e-3 x taps).  plan() starts with
    the tap ceiling of the kernel instance."""
    _P = "llz_adapt_bands_mc"

    def __init__(self, channels, bins, taps, mu=0.5, delta=None, stream=None):
        self.channels, self.bins, self.taps = channels, bins, taps
        self._open(stream, channels, bins, taps, mu, 1e-3 * taps if delta is None else delta)

    def process(self, x_re, x_im, d_re, d_im, e_re, e_im, y_re=None, y_im=None):
        """x (reference), d (desired), e (error, written), y (filter output, written when both are given): [channels, frames,
        bins] float32 each (torch device tensors or numpy), any number of frames, none included.  Returns (e_re, e_im)."""
        return self._process_xdey(x_re, x_im, d_re, d_im, e_re, e_im, y_re, y_im)

    def set_step(self, first, mu):
        """step sizes of channels first .. first + count - 1: [count] values in [0, 2] (or one number), 0 = frozen"""
        self._set_rows("_set_step", first, np.atleast_1d(mu), np.float32)

    def set_taps(self, first, w):
        """replace the weights of channels first .. first + count - 1; w: complex [count, taps, bins] (row q the taps of age q),
        or [taps, bins] for one channel; the history is kept"""
        w = np.asarray(w)
        w = self._rows(w[None] if w.ndim == 2 else w, "set_taps", "w must be [count")
        self._set_taps(w, first, w.shape[0])

    def get_taps(self, first=0, count=None):
        """the weights of channels first .. first + count - 1 (default: all from first) as complex64 [count, taps, bins]: the
        handle's own float32 values"""
        count = self.channels - first if count is None else count
        return self._get_taps((count,), first, count)

    def reset(self, clear_taps=False):
        self._call("_reset", 1 if clear_taps else 0)


class AdaptBandsMatrixMC(_BandsFilter):
    """band signals, float32, re and im apart (StftMC's and PfbMC's layout): llz_adapt_bands_matrix_mc_*, a normalised LMS filter
    of `inputs` references x `taps` complex taps for every (output, bin), normalised by the joint power of the references and
    updated frame by frame (include/llz_adapt_bands_matrix.h) -- AdaptBandsMC for a microphone that hears several loudspeakers;
    frozen (mu = 0) with set_taps, a filter-and-sum beamformer with a weight per bin.  inputs 1..8, inputs x taps <= 64.  The
    weights start at zero; mu is every output's step size (0 = frozen), delta the regularisation of the power (None: 1e-3 x
    inputs x taps).  plan() starts with the inputs of the kernel instance and its entry ceiling."""
    _P = "llz_adapt_bands_matrix_mc"
    _PLAN = 5

    def __init__(self, inputs, outputs, bins, taps, mu=0.5, delta=None, stream=None):
        self.inputs, self.outputs, self.bins, self.taps = inputs, outputs, bins, taps
        self._open(stream, inputs, outputs, bins, taps, mu, 1e-3 * inputs * taps if delta is None else delta)

    def process(self, x, d, e, y=None):
        """x (references), d (desired), e (error, written), y (filter output, written when given): each a pair (re, im) of
        float32 buffers (torch device tensors or numpy, in any mix), x [inputs, frames, bins], the others [outputs, frames,
        bins]; any number of frames, none included.  Returns e."""
        return self._process_pairs(x, d, e, y)

    def set_step(self, out_first, mu):
        """step sizes of outputs out_first .. out_first + count - 1: [count] values in [0, 2] (or one number), 0 = frozen"""
        self._set_rows("_set_step", out_first, np.atleast_1d(mu), np.float32)

    def set_taps(self, out_first, w, in_first=0):
        """replace the weights of the paths (out_first .., in_first ..); w: complex [out_count, in_count, taps, bins] (row q the
        taps of age q); the history is kept"""
        w = self._rows(np.asarray(w), "set_taps", "w must be [out_count, in_count", lead=2)
        self._set_taps(w, out_first, w.shape[0], in_first, w.shape[1])

    def get_taps(self, out_first=0, out_count=None, in_first=0, in_count=None):
        """the weights of the paths (out_first .., in_first ..) (default: all from there) as complex64 [out_count, in_count, taps,
        bins]: the handle's own float32 values"""
        out_count = self.outputs - out_first if out_count is None else out_count
        in_count = self.inputs - in_first if in_count is None else in_count
        return self._get_taps((out_count, in_count), out_first, out_count, in_first, in_count)

    def reset(self, clear_taps=False):
        self._call("_reset", 1 if clear_taps else 0)


class KalmanBandsMC(_BandsFilter):
    """band signals [channels, frames, bins] float32, re and im apart (AdaptBandsMC's layout): llz_kalman_bands_mc_*, the diagonal
    Kalman adaptive filter of `taps` (1..32) complex taps for every (channel, bin) (include/llz_kalman_bands.h) -- AdaptBandsMC's
    place in a subband echo canceller, with the step controlled by a variance per tap and a tracked noise power, so that it
    survives double-talk unattended.  a: the state transition in (0, 1]; lam: the smoothing of the noise power in [0, 1); p0: the
    variances at init; delta: the regularisation.  Every channel adapts until set_adapt says otherwise.  plan() starts with the
    tap ceiling of the kernel instance."""
    _P = "llz_kalman_bands_mc"

    def __init__(self, channels, bins, taps, a=0.999, lam=0.9, p0=1.0, delta=1e-3, stream=None):
        self.channels, self.bins, self.taps = channels, bins, taps
        self._open(stream, channels, bins, taps, a, lam, p0, delta)

    def process(self, x_re, x_im, d_re, d_im, e_re, e_im, y_re=None, y_im=None):
        """x (reference), d (desired), e (error, written), y (filter output, written when both are given): [channels, frames,
        bins] float32 each (torch device tensors or numpy), any number of frames, none included.  Returns (e_re, e_im)."""
        return self._process_xdey(x_re, x_im, d_re, d_im, e_re, e_im, y_re, y_im)

    def set_adapt(self, first, on):
        """whether channels first .. first + count - 1 adapt: [count] truth values (or one), False = frozen"""
        self._set_rows("_set_adapt", first, np.atleast_1d(on) != 0, np.int32)

    def _rows3(self, a, what):
        return self._rows(a[None] if a.ndim == 2 else a, what, "must be [count")

    def set_taps(self, first, w):
        """replace the weights of channels first .. first + count - 1; w: complex [count, taps, bins] (row q the taps of age q),
        or [taps, bins] for one channel; history, variances and noise powers are kept"""
        w = self._rows3(np.asarray(w), "set_taps")
        self._set_taps(w, first, w.shape[0])

    def get_taps(self, first=0, count=None):
        """the weights of channels first .. first + count - 1 (default: all from first) as complex64 [count, taps, bins]"""
        count = self.channels - first if count is None else count
        return self._get_taps((count,), first, count)

    def set_variance(self, first, p):
        """replace the variances of channels first .. first + count - 1; p: real [count, taps, bins] or [taps, bins], finite and
        >= 0 -- raising them re-opens adaptation after a known path change"""
        self._set_rows("_set_variance", first, self._rows3(np.asarray(p), "set_variance"), np.float32)

    def get_variance(self, first=0, count=None):
        """the variances of channels first .. first + count - 1 as float32 [count, taps, bins]"""
        return self._get_rows("_get_variance", first, count, self.taps, self.bins)

    def get_noise(self, first=0, count=None):
        """the noise powers of channels first .. first + count - 1 as float32 [count, bins]"""
        return self._get_rows("_get_noise", first, count, self.bins)

    def reset(self, clear=False):
        self._call("_reset", 1 if clear else 0)


class KalmanBandsMatrixMC(_BandsFilter):
    """band signals, float32, re and im apart (AdaptBandsMatrixMC's layout): llz_kalman_bands_matrix_mc_*, the diagonal Kalman
    adaptive filter of `inputs` references x `taps` complex taps for every (output, bin) (include/llz_kalman_bands_matrix.h) --
    KalmanBandsMC for a microphone that hears several loudspeakers: a variance per path and tap and one tracked noise power per
    (output, bin), so that it survives double-talk unattended.  inputs 1..8, inputs x taps <= 32.  a, lam, p0 and delta are
    KalmanBandsMC's.  Every output adapts until set_adapt says otherwise.  plan() starts with the inputs of the kernel instance
    and its entry ceiling."""
    _P = "llz_kalman_bands_matrix_mc"
    _PLAN = 5

    def __init__(self, inputs, outputs, bins, taps, a=0.999, lam=0.9, p0=1.0, delta=1e-3, stream=None):
        self.inputs, self.outputs, self.bins, self.taps = inputs, outputs, bins, taps
        self._open(stream, inputs, outputs, bins, taps, a, lam, p0, delta)

    def process(self, x, d, e, y=None):
        """x (references), d (desired), e (error, written), y (filter output, written when given): each a pair (re, im) of
        float32 buffers (torch device tensors or numpy, in any mix), x [inputs, frames, bins], the others [outputs, frames,
        bins]; any number of frames, none included.  Returns e."""
        return self._process_pairs(x, d, e, y)

    def set_adapt(self, out_first, on):
        """whether outputs out_first .. out_first + count - 1 adapt: [count] truth values (or one), False = frozen"""
        self._set_rows("_set_adapt", out_first, np.atleast_1d(on) != 0, np.int32)

    def _counts(self, out_first, out_count, in_first, in_count):
        return (self.outputs - out_first if out_count is None else out_count,
                self.inputs - in_first if in_count is None else in_count)

    def set_taps(self, out_first, w, in_first=0):
        """replace the weights of the paths (out_first .., in_first ..); w: complex [out_count, in_count, taps, bins] (row q the
        taps of age q); history, variances and noise powers are kept"""
        w = self._rows(np.asarray(w), "set_taps", "w must be [out_count, in_count", lead=2)
        self._set_taps(w, out_first, w.shape[0], in_first, w.shape[1])

    def get_taps(self, out_first=0, out_count=None, in_first=0, in_count=None):
        """the weights of the paths (out_first .., in_first ..) (default: all from there) as complex64 [out_count, in_count, taps,
        bins]: the handle's own float32 values"""
        out_count, in_count = self._counts(out_first, out_count, in_first, in_count)
        return self._get_taps((out_count, in_count), out_first, out_count, in_first, in_count)

    def set_variance(self, out_first, p, in_first=0):
        """replace the variances of the paths (out_first .., in_first ..); p: real [out_count, in_count, taps, bins], finite and
        >= 0 -- raising them re-opens adaptation after a known path change"""
        p = self._rows(np.asarray(p), "set_variance", "p must be [out_count, in_count", lead=2)
        p = np.ascontiguousarray(p, dtype=np.float32)
        self._call("_set_variance", out_first, p.shape[0], in_first, p.shape[1], p.ctypes.data)

    def get_variance(self, out_first=0, out_count=None, in_first=0, in_count=None):
        """the variances of the paths (out_first .., in_first ..) as float32 [out_count, in_count, taps, bins]"""
        out_count, in_count = self._counts(out_first, out_count, in_first, in_count)
        p = np.empty((max(out_count, 0), max(in_count, 0), self.taps, self.bins), dtype=np.float32)
        self._call("_get_variance", out_first, out_count, in_first, in_count, p.ctypes.data)
        return p

    def get_noise(self, out_first=0, out_count=None):
        """the noise powers of outputs out_first .. out_first + count - 1 as float32 [count, bins]"""
        out_count = self.outputs - out_first if out_count is None else out_count
        psi = np.empty((max(out_count, 0), self.bins), dtype=np.float32)
        self._call("_get_noise", out_first, out_count, psi.ctypes.data)
        return psi

    def reset(self, clear=False):
        self._call("_reset", 1 if clear else 0)


class SuppressCfg(C.Structure):
    """llz_suppress_cfg of include/llz_suppress_bands.h"""
    _fields_ = [("window", C.c_int), ("as_", C.c_float), ("aq", C.c_float), ("ad", C.c_float), ("t0", C.c_float),
                ("t1", C.c_float), ("beta", C.c_float), ("rho", C.c_float), ("delta", C.c_float)]


class SuppressBandsMC(_BandsFilter):
    """band signals [channels, frames, bins] float32, re and im apart (KalmanBandsMC's layout): llz_suppress_bands_mc_*, the noise
    and residual-echo postfilter behind a subband echo canceller (include/llz_suppress_bands.h) -- a real gain per (channel, bin,
    frame) from a tracked noise power (MCRA), a decision-directed Wiener rule and a peak-hold residual-echo estimate eta |y|^2.
    It takes KalmanBandsMC's e and, on request, y; without y it is a noise suppressor for any band signal.  window: frames of
    the minimum search and of the start-up, which is taken as noise only; the other parameters are the header's.  Every channel
    is enabled, with a floor of 0.1 and no leakage, until the setters say otherwise.  plan() starts with 1 when the last call
    took y, else 0."""
    _P = "llz_suppress_bands_mc"
    STATES = ("S", "Smin", "Stmp", "q", "N", "R", "Z")

    def __init__(self, channels, bins, window=128, as_=0.8, aq=0.2, ad=0.95, t0=2.0, t1=5.0, beta=0.98, rho=0.6, delta=1e-6,
                 stream=None):
        cfg = SuppressCfg()
        capi.lib().llz_suppress_bands_mc_default_cfg(C.byref(cfg))
        cfg.window, cfg.as_, cfg.aq, cfg.ad, cfg.t0, cfg.t1, cfg.beta, cfg.rho, cfg.delta = window, as_, aq, ad, t0, t1, beta, rho, delta
        self.channels, self.bins, self.window = channels, bins, window
        self._open(stream, channels, bins, C.byref(cfg))

    def process(self, e_re, e_im, o_re, o_im, y_re=None, y_im=None, g=None):
        """e (the canceller's error), o (written), y (its echo estimate, read when both are given), g (the gain, written when
        given): [channels, frames, bins] float32 each (torch device tensors or numpy), any number of frames, none included.
        Returns (o_re, o_im)."""
        self._both_or_neither(y_re, y_im)
        bufs = [("e_re", e_re), ("e_im", e_im), ("y_re", y_re), ("y_im", y_im), ("o_re", o_re), ("o_im", o_im), ("g", g)]
        self._process(self._frames_in(e_re, self.channels), [(name, b, self.channels) for name, b in bufs])
        return o_re, o_im

    def set_floor(self, first, gmin):
        """the gain floors of channels first .. first + count - 1: [count] values (or one) in [0, 1]"""
        self._set_rows("_set_floor", first, np.atleast_1d(gmin), np.float32)

    def set_leak(self, first, eta):
        """the echo leakages of channels first .. first + count - 1: [count] values (or one), finite and >= 0"""
        self._set_rows("_set_leak", first, np.atleast_1d(eta), np.float32)

    def set_enable(self, first, on):
        """whether channels first .. first + count - 1 are processed: [count] truth values (or one), False = passed through"""
        self._set_rows("_set_enable", first, np.atleast_1d(on) != 0, np.int32)

    def get_state(self, which, first=0, count=None):
        """state value `which` (0..6 or one of STATES) of channels first .. first + count - 1 as float32 [count, bins]"""
        which = self.STATES.index(which) if isinstance(which, str) else which
        count = self.channels - first if count is None else count
        out = np.empty((max(count, 0), self.bins), dtype=np.float32)
        self._call("_get_state", which, first, count, out.ctypes.data)
        return out

    def reset(self):
        """state and frame count back to init; flags, floors and leakages are kept"""
        self._call("_reset")


# ------------------------------------------------------------------------------------------ IIR
class IirFilter:
    """Single channel direct form I, double, host buffers: llz_iir_filter_*."""

    def __init__(self, a, b):
        self._L = capi.lib()
        a = _f64(a)
        self.M = len(a) - 1
        if b is None:
            raise LlzError("pass b (zeros for the reference's NULL case)")
        b = _f64(b)
        self.N = len(b) - 1
        self.handle = check_handle(
            self._L.llz_iir_filter_init(self.M, a.ctypes.data_as(_dp), self.N, b.ctypes.data_as(_dp)),
            "llz_iir_filter_init")

    def filter(self, x):
        x = _f64(x)
        y = np.zeros_like(x)
        check(self._L.llz_iir_filter(self.handle, x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), len(x)),
              "llz_iir_filter")
        return y

    def flush(self):
        y = np.zeros(max(self.N, 1))
        n = check(self._L.llz_iir_filter_flush(self.handle, y.ctypes.data_as(_dp)), "llz_iir_filter_flush")
        return y[:n]

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_iir_filter_uninit(self.handle)
            self.handle = 0

    __del__ = close


IIR_FORMS = ("pipe", "wave16", "wave32")      # LLZ_IIR_FORM_* (include/llz_iir.h)


class IirCascadeMC:
    """channels x n float32 through a fused cascade of biquads; coef rows {b0,b1,b2,a0,a1,a2}."""

    def __init__(self, channels, coef, stream=None):
        self._L = capi.lib()
        coef = _f64(coef).reshape(-1, 6)
        self.stages = coef.shape[0]
        self.channels = channels
        self.handle = check_handle(self._L.llz_iir_cascade_mc_init(channels, self.stages, coef.ctypes.data),
                                   "llz_iir_cascade_mc_init")
        self.precision = self._L.llz_iir_cascade_mc_precision(self.handle)      # 32 or 64 (arithmetic of the fast kernel)
        if stream is not None:
            check(self._L.llz_iir_cascade_mc_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def filter(self, x, out):
        n = x.shape[-1]
        check(self._L.llz_iir_cascade_mc(self.handle, _typed(x, "float32", self.channels * n, "IirCascadeMC.filter x"),
                                         _typed(out, "float32", self.channels * n, "IirCascadeMC.filter out"), n),
              "llz_iir_cascade_mc")
        return out

    def plan(self, n):
        """what filter() would run a frame of n samples as, under the tunes set now (llz_iir_cascade_mc_plan; nothing is
        launched): dict of form ("pipe" / "wave16" / "wave32"), chunk (its chunk in samples), precision, segs, seg_chunks, warm"""
        out = (C.c_int * 5)()
        check(self._L.llz_iir_cascade_mc_plan(self.handle, int(n), out), "llz_iir_cascade_mc_plan")
        return {"form": IIR_FORMS[out[0]], "chunk": 2048 if out[0] == 2 else 1024, "precision": out[1], "segs": out[2],
                "seg_chunks": out[3], "warm": out[4]}

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_iir_cascade_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class IirBankMC:
    """channels x n float32 through a cascade of biquads PER CHANNEL: llz_iir_bank_mc_*.  coef: [channels, stages, 6], rows
    {b0,b1,b2,a0,a1,a2}; a channel with fewer sections pads with identity sections {1,0,0,1,0,0}."""

    def __init__(self, channels, coef, stream=None):
        self._L = capi.lib()
        coef = _f64(coef)
        if coef.ndim != 3 or coef.shape[0] != channels or coef.shape[1] < 1 or coef.shape[2] != 6:
            raise LlzError(f"IirBankMC: coef must be [channels = {channels}, stages, 6], got {coef.shape} "
                           "(one coefficient set for every channel is IirCascadeMC)")
        self.channels, self.stages = channels, coef.shape[1]
        self.handle = check_handle(self._L.llz_iir_bank_mc_init(channels, self.stages, coef.ctypes.data),
                                   "llz_iir_bank_mc_init")
        if stream is not None:
            check(self._L.llz_iir_bank_mc_set_stream(self.handle, _stream_ptr(stream)), "llz_iir_bank_mc_set_stream")

    @property
    def precision(self):
        """32 or 64: the arithmetic of the fast kernels, the handle's verdict over every channel's set (set_coef may change it)"""
        return check(self._L.llz_iir_bank_mc_precision(self.handle), "llz_iir_bank_mc_precision")

    def set_coef(self, first, coef):
        """replace the sets of channels first .. first + len(coef) - 1, state kept; coef: [count, stages, 6]"""
        coef = _f64(coef)
        if coef.ndim != 3 or coef.shape[1:] != (self.stages, 6):
            raise LlzError(f"IirBankMC.set_coef: coef must be [count, stages = {self.stages}, 6], got {coef.shape}")
        check(self._L.llz_iir_bank_mc_set_coef(self.handle, int(first), coef.shape[0], coef.ctypes.data),
              "llz_iir_bank_mc_set_coef")

    def filter(self, x, out):
        n = x.shape[-1]
        check(self._L.llz_iir_bank_mc(self.handle, _typed(x, "float32", self.channels * n, "IirBankMC.filter x"),
                                      _typed(out, "float32", self.channels * n, "IirBankMC.filter out"), n),
              "llz_iir_bank_mc")
        return out

    def plan(self, n):
        """as IirCascadeMC.plan (llz_iir_bank_mc_plan; nothing is launched); the bank has no "wave32" form"""
        out = (C.c_int * 5)()
        check(self._L.llz_iir_bank_mc_plan(self.handle, int(n), out), "llz_iir_bank_mc_plan")
        return {"form": IIR_FORMS[out[0]], "chunk": 2048 if out[0] == 2 else 1024, "precision": out[1], "segs": out[2],
                "seg_chunks": out[3], "warm": out[4]}

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_iir_bank_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


# ------------------------------------------------------------------------------------------ resample
class IirMC:
    """llz_iir_mc_* (include/llz_iir.h part 3): the general direct-form-I filter for many channels, float32 in / out."""

    def __init__(self, channels, a, b, stream=None):
        self._L = capi.lib()
        a, b = _f64(a), _f64(b)
        self.channels, self.M, self.N = channels, len(a) - 1, len(b) - 1
        self.handle = check_handle(self._L.llz_iir_mc_init(channels, self.M, a.ctypes.data_as(_dp), self.N, b.ctypes.data_as(_dp)),
                                   "llz_iir_mc_init")
        if stream is not None:
            check(self._L.llz_iir_mc_set_stream(self.handle, _stream_ptr(stream)), "llz_iir_mc_set_stream")

    def filter(self, x, out):
        n = int(x.shape[-1])
        check(self._L.llz_iir_mc(self.handle, _typed(x, "float32", self.channels * n, "x"), _typed(out, "float32", self.channels * n, "y"), n),
              "llz_iir_mc")
        return out

    def segments(self, n):
        """time segments per channel filter() would run a frame of n samples with (llz_iir_mc_segments; nothing is launched)"""
        return check(self._L.llz_iir_mc_segments(self.handle, int(n)), "llz_iir_mc_segments")

    def flush(self, out):
        """N more outputs per channel into out [channels][N] (N = 0: nothing to flush, out is not touched)"""
        if self.N == 0:
            return check(self._L.llz_iir_mc_flush(self.handle, _ptr(out)), "llz_iir_mc_flush")
        return check(self._L.llz_iir_mc_flush(self.handle, _typed(out, "float32", self.channels * self.N, "y")), "llz_iir_mc_flush")

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_iir_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class _Resample1:
    """int16 single channel, host buffers: llz_{decimate,interp,resample}."""
    _init = _run = _uninit = None

    def _open(self, h):
        self.handle = check_handle(h, type(self).__name__ + " init")
        self.bytes_in = self._L.llz_get_resample_framelen_bytes(self.handle)

    def process(self, pcm):
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        out = np.zeros(len(pcm) * 16 + 16, dtype=np.int16)
        ob = C.c_int(0)
        rc = self._run(self.handle, pcm.ctypes.data, 2 * len(pcm), out.ctypes.data, C.byref(ob))
        check(rc, type(self).__name__)
        return out[:ob.value // 2].copy()

    def close(self):
        if getattr(self, "handle", 0):
            self._uninit(self.handle)
            self.handle = 0

    __del__ = close


class Decimate(_Resample1):
    def __init__(self, M, gain=1.0, win=BLACKMAN):
        self._L = capi.lib()
        self._run, self._uninit = self._L.llz_decimate, self._L.llz_decimate_uninit
        self._open(self._L.llz_decimate_init(M, gain, win))


class Interp(_Resample1):
    def __init__(self, L_, gain=1.0, win=BLACKMAN):
        self._L = capi.lib()
        self._run, self._uninit = self._L.llz_interp, self._L.llz_interp_uninit
        self._open(self._L.llz_interp_init(L_, gain, win))


class Resample(_Resample1):
    def __init__(self, L_, M, gain=1.0, win=BLACKMAN):
        self._L = capi.lib()
        self._run, self._uninit = self._L.llz_resample, self._L.llz_resample_filter_uninit
        self._open(self._L.llz_resample_filter_init(L_, M, gain, win))


class ResampleMC:
    """channels x n_in -> channels x n_in*L/M; pcm_format PCM_F32 (float32), PCM_I16 (bit-exact int16) or PCM_I16_FAST
    (int16 within 1 LSB of the reference, matrix cores, decimators only)."""

    def __init__(self, channels, L_, M, gain=1.0, win=BLACKMAN, pcm_format=PCM_F32, stream=None):
        self._L = capi.lib()
        self.channels, self.L, self.M, self.fmt = channels, L_, M, pcm_format
        self.handle = check_handle(self._L.llz_resample_mc_init(channels, L_, M, gain, win, pcm_format),
                                   "llz_resample_mc_init")
        self.Q = self._L.llz_resample_mc_sub_len(self.handle)
        if stream is not None:
            check(self._L.llz_resample_mc_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def out_len(self, n_in):
        return check(self._L.llz_resample_mc_out_len(self.handle, n_in), "llz_resample_mc_out_len")

    def last_entry(self):
        """name of the shim entry that ran the last successful call ("" before the first)"""
        name = self._L.llz_resample_mc_last_entry(self.handle)
        if name is None:
            raise LlzError("llz_resample_mc_last_entry: bad handle")
        return name.decode()

    def matrix(self):
        m = np.zeros(self.L * self.Q)
        check(self._L.llz_resample_mc_get_matrix(self.handle, m.ctypes.data, m.size), "get_matrix")
        return m.reshape(self.L, self.Q)

    def set_matrix(self, m):
        m = _f64(m)
        check(self._L.llz_resample_mc_set_matrix(self.handle, m.ctypes.data, m.size), "set_matrix")

    def process(self, x, out):
        n_in = x.shape[-1]
        dt = "float32" if self.fmt == PCM_F32 else "int16"
        n_out = self.out_len(n_in)
        return check(self._L.llz_resample_mc(self.handle, _typed(x, dt, self.channels * n_in, "ResampleMC.process x"), n_in,
                                             _typed(out, dt, self.channels * n_out, "ResampleMC.process out")),
                     "llz_resample_mc")

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_resample_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class AsrcMC:
    """channels x n_in float32 -> a count of outputs per channel: llz_asrc_mc_*, the arbitrary-ratio resampler
    (include/llz_asrc.h) -- a polyphase windowed-sinc table with linear interpolation between phases, time in 64-bit fixed
    point, a step (input samples per output) per channel that may glide while the signals run.  frame_len is the longest
    n_in; cutoff=None means min(1, 1 / step), times 0.9 when that is below 1."""

    def __init__(self, channels, frame_len, step=1.0, taps=32, phases=512, cutoff=None, gain=1.0, win=KAISER, stream=None):
        self._L = capi.lib()
        if cutoff is None:
            cutoff = min(1.0, 1.0 / step) if step > 0 else 1.0
            cutoff = 0.9 * cutoff if cutoff < 1.0 else cutoff
        self.handle = check_handle(self._L.llz_asrc_mc_init(channels, frame_len, taps, phases, cutoff, gain, win, step),
                                   "llz_asrc_mc_init")
        self.channels, self.frame_len, self.taps, self.phases, self.cutoff = channels, frame_len, taps, phases, cutoff
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        check(self._L.llz_asrc_mc_set_stream(self.handle, _stream_ptr(stream)), "llz_asrc_mc_set_stream")

    def plan(self):
        """(taps, phases, history samples kept per channel, table form: 0 = in LDS, 1 = read from global memory)"""
        out = (C.c_int * 4)()
        check(self._L.llz_asrc_mc_plan(self.handle, out), "llz_asrc_mc_plan")
        return tuple(out)

    def out_len(self, n_in):
        """the counts [channels] the next call of n_in samples would deliver; the state does not move"""
        counts = (C.c_int * self.channels)()
        check(self._L.llz_asrc_mc_out_len(self.handle, n_in, counts), "llz_asrc_mc_out_len")
        return np.array(counts, dtype=np.int64)

    def process(self, x, out):
        """x: [channels, n_in] float32, n_in <= frame_len (n_in = 0: an empty array); out: [channels, out_pitch] float32, row c
        receives counts[c] outputs and is not written behind them (torch device tensors or numpy).  Returns counts."""
        n_in = (x.numel() if hasattr(x, "numel") else x.size) // self.channels
        out_pitch = (out.numel() if hasattr(out, "numel") else out.size) // self.channels
        counts = (C.c_int * self.channels)()
        check(self._L.llz_asrc_mc(self.handle, _typed(x, "float32", self.channels * n_in, "AsrcMC.process x") if n_in else None,
                                  n_in, _typed(out, "float32", self.channels * out_pitch, "AsrcMC.process out"), out_pitch,
                                  counts), "llz_asrc_mc")
        return np.array(counts, dtype=np.int64)

    def set_step(self, first, step, ramp=0):
        """steps of channels first .. first + count - 1: [count] values in [1/16, 16] (or one number), reached over `ramp`
        outputs (0: at once)"""
        step = _f64(np.atleast_1d(step))
        check(self._L.llz_asrc_mc_set_step(self.handle, first, step.shape[0], step.ctypes.data_as(_dp), ramp),
              "llz_asrc_mc_set_step")

    def get_step(self, first=0, count=None):
        """(the step behind each channel's next output, the outputs its glide has left) of channels first .. first + count - 1"""
        count = self.channels - first if count is None else count
        step, left = np.zeros(max(count, 1)), (C.c_long * max(count, 1))()
        check(self._L.llz_asrc_mc_get_step(self.handle, first, count, step.ctypes.data_as(_dp), left), "llz_asrc_mc_get_step")
        return step, np.array(left, dtype=np.int64)

    def next_time(self, first=0, count=None):
        """the time of each channel's next output as (whole input samples, fraction in units of 2^-32), two int arrays"""
        count = self.channels - first if count is None else count
        whole, frac = (C.c_longlong * max(count, 1))(), (C.c_uint * max(count, 1))()
        check(self._L.llz_asrc_mc_next_time(self.handle, first, count, whole, frac), "llz_asrc_mc_next_time")
        return np.array(whole, dtype=np.int64), np.array(frac, dtype=np.int64)

    def table(self):
        """G of the definition: [phases + 1, taps] float32"""
        g = np.empty((self.phases + 1, self.taps), dtype=np.float32)
        check(self._L.llz_asrc_mc_get_table(self.handle, g.ctypes.data, g.size), "llz_asrc_mc_get_table")
        return g

    def reset(self):
        check(self._L.llz_asrc_mc_reset(self.handle), "llz_asrc_mc_reset")

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_asrc_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


# ------------------------------------------------------------------------------------------ FFT
class Fft:
    """Reference API: complex128 host arrays, forward unscaled, inverse / N."""

    def __init__(self, size):
        self._L = capi.lib()
        self.size = size
        self.handle = check_handle(self._L.llz_fft_init(size), "llz_fft_init")

    def _run(self, fn, z):
        z = np.ascontiguousarray(z, dtype=np.complex128).copy()
        if len(z) != self.size:
            raise LlzError("length mismatch")
        fn(self.handle, z.view(np.float64).ctypes.data_as(_dp))
        return z

    def fft(self, z):
        return self._run(self._L.llz_fft, z)

    def ifft(self, z):
        return self._run(self._L.llz_ifft, z)

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_fft_uninit(self.handle)
            self.handle = 0

    __del__ = close


class FftBatch:
    """count x size complex64 transforms in place (device tensor of float32 pairs or numpy complex64)."""

    def __init__(self, size, stream=None):
        self._L = capi.lib()
        self.size = size
        self.handle = check_handle(self._L.llz_fft_batch_init(size), "llz_fft_batch_init")
        if stream is not None:
            check(self._L.llz_fft_batch_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def fft(self, data, count):
        check(self._L.llz_fft_batch(self.handle, _ptr(data), count), "llz_fft_batch")
        return data

    def ifft(self, data, count):
        check(self._L.llz_ifft_batch(self.handle, _ptr(data), count), "llz_ifft_batch")
        return data

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_fft_batch_uninit(self.handle)
            self.handle = 0

    __del__ = close


class FftFixed:
    """int32 interleaved data, Q15 twiddles, bit-exact; single (host) and batched (device or host)."""

    def __init__(self, size, stream=None):
        self._L = capi.lib()
        self.size = size
        self.handle = check_handle(self._L.llz_fft_fixed_init(size), "llz_fft_fixed_init")
        if stream is not None:
            check(self._L.llz_fft_fixed_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def fft(self, q):
        q = np.ascontiguousarray(q, dtype=np.int32).copy()
        self._L.llz_fft_fixed(self.handle, q.ctypes.data_as(C.POINTER(C.c_int)))
        return q

    def ifft(self, q):
        q = np.ascontiguousarray(q, dtype=np.int32).copy()
        self._L.llz_ifft_fixed(self.handle, q.ctypes.data_as(C.POINTER(C.c_int)))
        return q

    def fft_batch(self, data, count):
        check(self._L.llz_fft_fixed_batch(self.handle, _ptr(data), count), "llz_fft_fixed_batch")
        return data

    def ifft_batch(self, data, count):
        check(self._L.llz_ifft_fixed_batch(self.handle, _ptr(data), count), "llz_ifft_fixed_batch")
        return data

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_fft_fixed_uninit(self.handle)
            self.handle = 0

    __del__ = close


# ------------------------------------------------------------------------------------------ correlation
def autocorr(x, p):
    """llz_autocorr: host float64, exact."""
    x = _f64(x)
    r = np.zeros(p + 1)
    capi.lib().llz_autocorr(x.ctypes.data_as(_dp), len(x), p, r.ctypes.data_as(_dp))
    return r


def crosscorr(x, y, p):
    x, y = _f64(x), _f64(y)
    r = np.zeros(p + 1)
    capi.lib().llz_crosscorr(x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), len(x), p, r.ctypes.data_as(_dp))
    return r


def corr_cof(a, b):
    a, b = _f64(a), _f64(b)
    return capi.lib().llz_corr_cof(a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), len(a))


def autocorr_fast(x, p):
    """llz_autocorr_fast_{init,uninit} around one call: host float64, exact (the reference's definition)."""
    L = capi.lib()
    x = _f64(x)
    h = check_handle(L.llz_autocorr_fast_init(len(x)), "llz_autocorr_fast_init")
    r = np.zeros(p + 1)
    L.llz_autocorr_fast(h, x.ctypes.data_as(_dp), len(x), p, r.ctypes.data_as(_dp))
    L.llz_autocorr_fast_uninit(h)
    return r


def autocorr_mc(x, r, p, stream=None):
    """x: [frames, n] float32, r: [frames, p+1] float32 (device tensors or numpy)."""
    frames, n = x.shape
    check(capi.lib().llz_autocorr_mc(_ptr(x), _ptr(r), frames, n, p, _stream_ptr(stream)), "llz_autocorr_mc")
    return r


class AutocorrFastMC:
    def __init__(self, frames, n, stream=None):
        self._L = capi.lib()
        self.handle = check_handle(self._L.llz_autocorr_fast_mc_init(frames, n), "llz_autocorr_fast_mc_init")
        if stream is not None:
            check(self._L.llz_autocorr_fast_mc_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def run(self, x, r, p):
        check(self._L.llz_autocorr_fast_mc(self.handle, _ptr(x), _ptr(r), p), "llz_autocorr_fast_mc")
        return r

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_autocorr_fast_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


def _lags(p, two_sided):
    return 2 * p + 1 if two_sided else p + 1


def crosscorr_mc(x, y, r, p, two_sided=False, stream=None):
    """x, y: [frames, n] float32; r: [frames, p+1] float32 (lags 0..p) or, two_sided, [frames, 2p+1] with lag k at index p+k
    (device tensors or numpy, each on its own).  r[f][k] = sum_i x[f][i] * y[f][i+k]."""
    frames, n = x.shape
    check(capi.lib().llz_crosscorr_mc(_typed(x, "float32", frames * n, "x"), _typed(y, "float32", frames * n, "y"),
                                      _typed(r, "float32", frames * _lags(p, two_sided), "r"), frames, n, p,
                                      1 if two_sided else 0, _stream_ptr(stream)), "llz_crosscorr_mc")
    return r


def corr_cof_mc(a, b, c, stream=None):
    """a, b: [frames, n] float32; c: [frames] float32 = <a,b> / sqrt(<a,a><b,b>) per frame (NaN where a or b is silent)."""
    frames, n = a.shape
    check(capi.lib().llz_corr_cof_mc(_typed(a, "float32", frames * n, "a"), _typed(b, "float32", frames * n, "b"),
                                     _typed(c, "float32", frames, "c"), frames, n, _stream_ptr(stream)), "llz_corr_cof_mc")
    return c


class CrosscorrFastMC:
    """llz_crosscorr_fast_mc: the linear cross-correlation of frames x n float32 through the FFT, 4 <= n <= 2048, p <= n - 1."""

    def __init__(self, frames, n, stream=None):
        self._L = capi.lib()
        self.frames, self.n = frames, n
        self.handle = check_handle(self._L.llz_crosscorr_fast_mc_init(frames, n), "llz_crosscorr_fast_mc_init")
        if stream is not None:
            check(self._L.llz_crosscorr_fast_mc_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def run(self, x, y, r, p, two_sided=False):
        size = self.frames * self.n
        check(self._L.llz_crosscorr_fast_mc(self.handle, _typed(x, "float32", size, "x"), _typed(y, "float32", size, "y"),
                                            _typed(r, "float32", self.frames * _lags(max(p, 0), two_sided), "r"), p,
                                            1 if two_sided else 0), "llz_crosscorr_fast_mc")
        return r

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_crosscorr_fast_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


# ------------------------------------------------------------------------------------------ Welch cross-spectra
class CsdMC:
    """llz_csd_mc_*: the averaged cross-spectra of channel pairs (include/llz_spectral.h).  pairs_xy: [(x, y), ...] channel
    indices; update(x) takes planar [channels, n] float32 (n a multiple of hop; a device tensor or a numpy array) and returns
    the frames summed so far.  The read-outs fill `out` when given (device or host) or return a new numpy array: psd_x, psd_y,
    coherence [pairs, bins] float32; csd, transfer [pairs, bins, 2] float32 (re, im); raw [pairs, bins, 4] float64 (Sxx, Syy,
    Re Sxy, Im Sxy).  PSD and CSD are two-sided values over bins 0 .. fft_len / 2."""

    def __init__(self, channels, pairs_xy, fft_len, hop, win=HAMMING, stream=None):
        self._L = capi.lib()
        table = np.ascontiguousarray(pairs_xy, dtype=np.int32).reshape(-1, 2)
        self.channels, self.pairs, self.fft_len, self.hop = channels, len(table), fft_len, hop
        self.bins = fft_len // 2 + 1
        self.handle = check_handle(self._L.llz_csd_mc_init(channels, self.pairs, table.ctypes.data_as(C.POINTER(C.c_int)),
                                                           fft_len, hop, win), "llz_csd_mc_init")
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        check(self._L.llz_csd_mc_set_stream(self.handle, _stream_ptr(stream)), "llz_csd_mc_set_stream")

    def update(self, x):
        size = x.numel() if hasattr(x, "numel") else x.size
        n, rem = divmod(size, self.channels)
        if rem:
            raise LlzError(f"llz_csd_mc_update: {size} samples do not divide into {self.channels} channels")
        return check(self._L.llz_csd_mc_update(self.handle, _typed(x, "float32", size, "x"), n), "llz_csd_mc_update")

    def frames(self):
        return check(self._L.llz_csd_mc_frames(self.handle), "llz_csd_mc_frames")

    def _read(self, what, width, out):
        shape = (self.pairs, self.bins) + ((width,) if width > 1 else ())
        if out is None:
            out = np.empty(shape, dtype=np.float32)
        check(self._L.llz_csd_mc_read(self.handle, what, _typed(out, "float32", self.pairs * self.bins * width, "out")),
              "llz_csd_mc_read")
        return out

    def psd_x(self, out=None):
        return self._read(capi.SPEC_PXX, 1, out)

    def psd_y(self, out=None):
        return self._read(capi.SPEC_PYY, 1, out)

    def csd(self, out=None):
        return self._read(capi.SPEC_CSD, 2, out)

    def coherence(self, out=None):
        return self._read(capi.SPEC_COHERENCE, 1, out)

    def transfer(self, out=None):
        return self._read(capi.SPEC_TF, 2, out)

    def raw(self, out=None):
        if out is None:
            out = np.empty((self.pairs, self.bins, 4), dtype=np.float64)
        check(self._L.llz_csd_mc_read_raw(self.handle, _typed(out, "float64", self.pairs * self.bins * 4, "out")),
              "llz_csd_mc_read_raw")
        return out

    def reset(self):
        check(self._L.llz_csd_mc_reset(self.handle), "llz_csd_mc_reset")

    def plan(self, n):
        """what update() of n samples per channel would run now: {"form": 0 staged / 1 register, "run", "runs_per_walk", "walks"}"""
        out = (C.c_int * 4)()
        check(self._L.llz_csd_mc_plan(self.handle, n, out), "llz_csd_mc_plan")
        return dict(zip(("form", "run", "runs_per_walk", "walks"), (int(v) for v in out)))

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_csd_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class TdeMC:
    """llz_tde_mc_*: the delay between the two channels of each pair, per frame (include/llz_tde.h): generalised
    cross-correlation on recursively averaged cross-spectra, weight capi.TDE_CC / TDE_PHAT / TDE_SCOT over the bins `band` =
    (k_lo, k_hi) (None: 1 .. fft_len / 2 - 1).  pairs_xy: [(x, y), ...] channel indices; y[t] = x[t - D] reads a delay of +D.
    process(x) takes planar [channels, n] float32 (n a multiple of hop; a device tensor or a numpy array) and returns
    (delay, peak), each [pairs, frames written by the call]: new numpy arrays, or views of the `delay` / `peak` buffers when
    given ([pairs, out_pitch] float32, device or host, out_pitch >= the call's frames; what lies behind the frames written
    stays untouched).  curve(): [pairs, 2 max_lag + 1] of the last frame; state(): [pairs, bins, 4] = Re S, Im S, Gx, Gy."""

    def __init__(self, channels, pairs_xy, fft_len, hop, max_lag, weight=capi.TDE_PHAT, lam=0.9, delta=0.0, band=None,
                 win=HAMMING, stream=None):
        self._L = capi.lib()
        table = np.ascontiguousarray(pairs_xy, dtype=np.int32).reshape(-1, 2)
        k_lo, k_hi = (1, fft_len // 2 - 1) if band is None else band
        self.channels, self.pairs, self.fft_len, self.hop, self.max_lag = channels, len(table), fft_len, hop, max_lag
        self.bins = fft_len // 2 + 1
        self.handle = check_handle(self._L.llz_tde_mc_init(channels, self.pairs, table.ctypes.data_as(C.POINTER(C.c_int)),
                                                           fft_len, hop, win, max_lag, weight, k_lo, k_hi, lam, delta),
                                   "llz_tde_mc_init")
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        check(self._L.llz_tde_mc_set_stream(self.handle, _stream_ptr(stream)), "llz_tde_mc_set_stream")

    def frames_for(self, n):
        return check(self._L.llz_tde_mc_frames_for(self.handle, n), "llz_tde_mc_frames_for")

    def process(self, x, delay=None, peak=None):
        size = x.numel() if hasattr(x, "numel") else x.size
        n, rem = divmod(size, self.channels)
        if rem:
            raise LlzError(f"llz_tde_mc_process: {size} samples do not divide into {self.channels} channels")
        frames = self.frames_for(n)
        given = [buf.numel() if hasattr(buf, "numel") else buf.size for buf in (delay, peak) if buf is not None]
        if given and (len(set(given)) != 1 or given[0] % self.pairs):
            raise LlzError(f"llz_tde_mc_process: delay and peak are [pairs = {self.pairs}, out_pitch] with one out_pitch")
        pitch = given[0] // self.pairs if given else frames
        if delay is None:
            delay = np.empty((self.pairs, pitch), dtype=np.float32)
        if peak is None:
            peak = np.empty((self.pairs, pitch), dtype=np.float32)
        got = check(self._L.llz_tde_mc_process(self.handle, _typed(x, "float32", size, "x"), n,
                                               _typed(delay, "float32", self.pairs * pitch, "delay"),
                                               _typed(peak, "float32", self.pairs * pitch, "peak"), pitch),
                    "llz_tde_mc_process")
        return delay.reshape(self.pairs, pitch)[:, :got], peak.reshape(self.pairs, pitch)[:, :got]

    def frames(self):
        return check(self._L.llz_tde_mc_frames(self.handle), "llz_tde_mc_frames")

    def _read(self, what, shape, out):
        if out is None:
            out = np.empty(shape, dtype=np.float32)
        check(self._L.llz_tde_mc_read(self.handle, what, _typed(out, "float32", int(np.prod(shape)), "out")), "llz_tde_mc_read")
        return out

    def curve(self, out=None):
        return self._read(capi.TDE_CURVE, (self.pairs, 2 * self.max_lag + 1), out)

    def state(self, out=None):
        return self._read(capi.TDE_STATE, (self.pairs, self.bins, 4), out)

    def set_forget(self, lam):
        check(self._L.llz_tde_mc_set_forget(self.handle, lam), "llz_tde_mc_set_forget")

    def reset(self):
        check(self._L.llz_tde_mc_reset(self.handle), "llz_tde_mc_reset")

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_tde_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class _ChirpZ:
    """what DftMC and CztMC share (include/llz_dft.h): rows a pitch apart in device tensors or numpy arrays.  A complex buffer
    is complex64, or float32 pairs; pitches count elements of the buffer's own kind; `count` defaults to the rows a contiguous
    input holds, the pitches to the row lengths, `out` to a new buffer where the input lives ([count, row] complex64 or
    float32)."""

    def _open(self, handle, what, window, stream):
        self.handle = check_handle(handle, what)
        if stream is not None:
            self.set_stream(stream)
        if window is not None:
            self.set_window(window)

    def set_stream(self, stream):
        check(self._L.llz_dft_mc_set_stream(self.handle, _stream_ptr(stream)), "llz_dft_mc_set_stream")

    def set_window(self, window):
        """n float32 window values (host), None for all ones: folded into the tables, ordered on the stream"""
        w = None if window is None else np.ascontiguousarray(window, dtype=np.float32)
        if w is not None and w.size != self.n:
            raise LlzError(f"llz_dft_mc_set_window: expected {self.n} window values, got {w.size}")
        check(self._L.llz_dft_mc_set_window(self.handle, None if w is None else w.ctypes.data), "llz_dft_mc_set_window")

    def configure(self, composed=False, scratch_mb=None):
        """measurement and tests: the composed form even where the fused kernel would be taken, and the cap in MiB of the scratch
        it walks `count` under (None: the library's 256)"""
        check(self._L.llz_dft_mc_configure(self.handle, int(bool(composed)), -1 if scratch_mb is None else scratch_mb),
              "llz_dft_mc_configure")

    def plan(self, count):
        """{form, M, rows per workgroup, LDS bytes, slabs} of a call of `count` rows"""
        out = (C.c_int * 5)()
        check(self._L.llz_dft_mc_plan(self.handle, count, out), "llz_dft_mc_plan")
        return dict(zip(("form", "m", "tpw", "lds", "slabs"), (int(v) for v in out)))

    @staticmethod
    def _elems(buf, cplx, what):
        name = str(buf.dtype).replace("torch.", "")
        size = buf.numel() if hasattr(buf, "numel") else buf.size
        if cplx and name == "float32" and size % 2 == 0:
            return size // 2
        if name != ("complex64" if cplx else "float32"):
            raise LlzError(f"{what}: expected {'complex64 or pairs of float32' if cplx else 'float32'}, got {size} x {name}")
        return size

    def _run(self, name, x, out, count, in_pitch, out_pitch, in_len, out_len, in_cplx, out_cplx):
        have = self._elems(x, in_cplx, name)
        in_pitch = in_len if in_pitch is None else in_pitch
        out_pitch = out_len if out_pitch is None else out_pitch
        if count is None:
            count = have // in_len if in_pitch == in_len else (have - in_len) // in_pitch + 1
        if count < 1 or in_pitch < 1 or have != (count - 1) * in_pitch + in_len:
            raise LlzError(f"{name}: {have} input elements are not {count} rows of {in_len}, {in_pitch} apart")
        need = (count - 1) * max(out_pitch, 0) + out_len
        if out is None:
            if isinstance(x, np.ndarray):
                out = np.empty(need, dtype=np.complex64 if out_cplx else np.float32)
            else:
                import torch
                out = torch.empty(need, dtype=torch.complex64 if out_cplx else torch.float32, device=x.device)
            if out_pitch == out_len:
                out = out.reshape(count, out_len)
        elif self._elems(out, out_cplx, name) != need:
            raise LlzError(f"{name}: out holds {self._elems(out, out_cplx, name)} elements, {count} rows of {out_len}, "
                           f"{out_pitch} apart, take {need}")
        check(getattr(self._L, name)(self.handle, _ptr(x), in_pitch, _ptr(out), out_pitch, count), name)
        return out

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_dft_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class DftMC(_ChirpZ):
    """llz_dft_mc_*: batched DFT of any length n in 2 .. 1048576 by the chirp-z algorithm.  forward / inverse: rows of n
    complex; rforward: n real -> n // 2 + 1 bins; rinverse: n // 2 + 1 bins -> n real.  The window multiplies the time side
    (the input of forward transforms, the output of inverse ones)."""

    def __init__(self, n, window=None, stream=None):
        self._L = capi.lib()
        self.n, self.bins = n, n // 2 + 1
        self._open(self._L.llz_dft_mc_init(n), "llz_dft_mc_init", window, stream)

    def forward(self, x, out=None, count=None, in_pitch=None, out_pitch=None):
        return self._run("llz_dft_mc_forward", x, out, count, in_pitch, out_pitch, self.n, self.n, True, True)

    def inverse(self, x, out=None, count=None, in_pitch=None, out_pitch=None):
        return self._run("llz_dft_mc_inverse", x, out, count, in_pitch, out_pitch, self.n, self.n, True, True)

    def rforward(self, x, out=None, count=None, in_pitch=None, out_pitch=None):
        return self._run("llz_dft_mc_real_forward", x, out, count, in_pitch, out_pitch, self.n, self.bins, False, True)

    def rinverse(self, x, out=None, count=None, in_pitch=None, out_pitch=None):
        return self._run("llz_dft_mc_real_inverse", x, out, count, in_pitch, out_pitch, self.bins, self.n, True, False)


class CztMC(_ChirpZ):
    """llz_czt_mc_*: the zoom transform X[k] = sum_n w[n] x[n] exp(-2 pi i (f0 + k df) n), k < K, of rows of n complex
    (forward) or real (rforward) samples; f0, df in cycles per sample, n + k - 1 <= 4096."""

    def __init__(self, n, k, f0, df, window=None, stream=None):
        self._L = capi.lib()
        self.n, self.k = n, k
        self._open(self._L.llz_czt_mc_init(n, k, f0, df), "llz_czt_mc_init", window, stream)

    def forward(self, x, out=None, count=None, in_pitch=None, out_pitch=None):
        return self._run("llz_czt_mc_forward", x, out, count, in_pitch, out_pitch, self.n, self.k, True, True)

    def rforward(self, x, out=None, count=None, in_pitch=None, out_pitch=None):
        return self._run("llz_czt_mc_real_forward", x, out, count, in_pitch, out_pitch, self.n, self.k, False, True)


# ------------------------------------------------------------------------------------------ linear prediction
LEVINSON_ORDER_MAX = 64


def _order_ok(p, what, lo=0):
    if not lo <= p <= LEVINSON_ORDER_MAX:
        raise LlzError(f"{what}: order {p} outside {lo}..{LEVINSON_ORDER_MAX}")


def _levinson(fn, r, p):
    _order_ok(p, fn)
    r = _f64(r)
    if len(r) < p + 1:
        raise LlzError(f"{fn}: r needs p + 1 = {p + 1} entries")
    acof, kcof, err = np.zeros(p + 1), np.zeros(p + 1), np.zeros(1)
    getattr(capi.lib(), fn)(r.ctypes.data_as(_dp), p, acof.ctypes.data_as(_dp), kcof.ctypes.data_as(_dp),
                            err.ctypes.data_as(_dp))
    return acof, kcof, float(err[0])


def levinson(r, p):
    """llz_levinson: host float64, exact -> (acof[p+1], kcof[p+1] (kcof[0..p-1] used), err)."""
    return _levinson("llz_levinson", r, p)


def levinson1(r, p):
    """llz_levinson1 (negated coefficients): host float64, exact -> (acof[p+1], kcof[p+1], err)."""
    return _levinson("llz_levinson1", r, p)


def atlvs(r, b):
    """llz_atlvs: solves the Toeplitz system T(r[0..n-1]) x = b -> (x[n], kcof[n], err, rc); rc -1 = singular."""
    r, b = _f64(r), _f64(b)
    n = len(b)
    _order_ok(n, "llz_atlvs", 1)
    if len(r) < n:
        raise LlzError("llz_atlvs: r needs len(b) entries")
    x, kcof, err = np.zeros(n), np.zeros(n), np.zeros(1)
    rc = capi.lib().llz_atlvs(r.ctypes.data_as(_dp), n, b.ctypes.data_as(_dp), x.ctypes.data_as(_dp),
                              kcof.ctypes.data_as(_dp), err.ctypes.data_as(_dp))
    return x, kcof, float(err[0]), rc


class Lpc:
    """llz_lpc_{init,uninit} handle: run(x) -> (acof[p+1], kcof[p+1], err, gain), state kept between calls as in the
    reference."""

    def __init__(self, p):
        self._L = capi.lib()
        self.p = p
        self.handle = check_handle(self._L.llz_lpc_init(p), "llz_lpc_init")

    def run(self, x):
        x = _f64(x)
        if len(x) < 1:
            raise LlzError("llz_lpc: empty frame")
        acof, kcof, err = np.zeros(self.p + 1), np.zeros(self.p + 1), np.zeros(1)
        gain = self._L.llz_lpc(self.handle, x.ctypes.data_as(_dp), len(x), acof.ctypes.data_as(_dp),
                               kcof.ctypes.data_as(_dp), err.ctypes.data_as(_dp))
        return acof, kcof, float(err[0]), gain

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_lpc_uninit(self.handle)
            self.handle = 0

    __del__ = close


def lpc_mc(x, acof, kcof=None, err=None, gain=None, r=None, win=None, p=None, stream=None):
    """llz_lpc_mc: x [frames, n] float32 -> acof [frames, p+1] (kcof [frames, p], err / gain [frames], r [frames, p+1]
    when given); win None or [n].  p defaults to acof's width - 1.  Device tensors or numpy arrays."""
    frames, n = x.shape
    if p is None:
        p = acof.shape[1] - 1
    ptr = lambda b, numel, what: None if b is None else _typed(b, "float32", numel, what)  # noqa: E731
    check(capi.lib().llz_lpc_mc(ptr(x, frames * n, "x"), ptr(win, n, "win"), ptr(acof, frames * (p + 1), "acof"),
                                ptr(kcof, frames * p, "kcof"), ptr(err, frames, "err"), ptr(gain, frames, "gain"),
                                ptr(r, frames * (p + 1), "r"), frames, n, p, _stream_ptr(stream)), "llz_lpc_mc")
    return acof


class LpcFilterMC:
    """llz_lpc_filter_mc_*: the filters that apply lpc_mc's coefficients, a set per (channel, frame).  x, e, y:
    [channels, frames * frame_len] float32, planar; acof: [channels, frames, p + 1] float32 (lpc_mc's output on
    x.view(channels * frames, frame_len)).  residual and synth keep their own state in the handle, so consecutive calls
    continue the streams.  Device tensors or numpy arrays."""

    def __init__(self, channels, frame_len, p, stream=None):
        self._L = capi.lib()
        self.handle = check_handle(self._L.llz_lpc_filter_mc_init(channels, frame_len, p), "llz_lpc_filter_mc_init")
        self.channels, self.frame_len, self.p = channels, frame_len, p
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        check(self._L.llz_lpc_filter_mc_set_stream(self.handle, _stream_ptr(stream)), "llz_lpc_filter_mc_set_stream")

    def _run(self, fn, src, acof, dst, frames):
        if frames is None:
            frames = (src.numel() if hasattr(src, "numel") else src.size) // (self.channels * self.frame_len)
        count = self.channels * frames * self.frame_len
        check(getattr(self._L, fn)(self.handle, _typed(src, "float32", count, fn + " input"),
                                   _typed(acof, "float32", self.channels * frames * (self.p + 1), fn + " acof"),
                                   _typed(dst, "float32", count, fn + " output"), frames), fn)
        return dst

    def residual(self, x, acof, e, frames=None):
        """e[t] = x[t] + sum_k a_f[k] x[t-k] (float32 fma chain, k = p .. 1).  Returns e."""
        return self._run("llz_lpc_residual_mc", x, acof, e, frames)

    def synth(self, e, acof, y, frames=None):
        """y[t] = e[t] - sum_k a_f[k] y[t-k] (double, k = p .. 1, rounded to float32 on store).  Returns y."""
        return self._run("llz_lpc_synth_mc", e, acof, y, frames)

    def reset(self):
        check(self._L.llz_lpc_filter_mc_reset(self.handle), "llz_lpc_filter_mc_reset")

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_lpc_filter_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


# ------------------------------------------------------------------------------------------ windowed-FFT frames
class _FftFrames:
    """llz_analysis_fft_* / llz_synthesis_fft_* (llz_asmodel.h:36-42): one frame per call, host float64, exact."""
    _init = _uninit = None

    def __init__(self, overlap_hint, frame_len, win=HAMMING):
        self._L = capi.lib()
        self.handle = check_handle(getattr(self._L, self._init)(overlap_hint, frame_len, win), self._init)
        self.frame_len = frame_len
        self.fft_len = frame_len << (2 if overlap_hint == capi.OVERLAP_HIGH else 1)
        self.bins = self.fft_len // 2 + 1

    def close(self):
        if getattr(self, "handle", 0):
            getattr(self._L, self._uninit)(self.handle)
            self.handle = 0

    __del__ = close


class AnalysisFft(_FftFrames):
    _init, _uninit = "llz_analysis_fft_init", "llz_analysis_fft_uninit"

    def frame(self, x):
        x = _f64(x)
        re, im = np.zeros(self.bins), np.zeros(self.bins)
        self._L.llz_analysis_fft(self.handle, x.ctypes.data_as(_dp), re.ctypes.data_as(_dp), im.ctypes.data_as(_dp))
        return re, im


class SynthesisFft(_FftFrames):
    _init, _uninit = "llz_synthesis_fft_init", "llz_synthesis_fft_uninit"

    def frame(self, re, im):
        re, im = _f64(re), _f64(im)
        x = np.zeros(self.frame_len)
        self._L.llz_synthesis_fft(self.handle, re.ctypes.data_as(_dp), im.ctypes.data_as(_dp), x.ctypes.data_as(_dp))
        return x


class StftMC:
    """llz_stft_mc_*: many channels and frames per call, float32; x [channels, frames*frame_len],
    re/im [channels, frames, bins]; the handle carries both streams' state between calls."""

    def __init__(self, channels, overlap_hint, frame_len, win=HAMMING, stream=None):
        self._L = capi.lib()
        self.handle = check_handle(self._L.llz_stft_mc_init(channels, overlap_hint, frame_len, win), "llz_stft_mc_init")
        self.channels, self.frame_len = channels, frame_len
        self.bins = self._L.llz_stft_mc_bins(self.handle)
        if stream is not None:
            check(self._L.llz_stft_mc_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def analysis(self, x, re, im):
        frames = x.shape[1] // self.frame_len
        check(self._L.llz_stft_mc_analysis(self.handle, _ptr(x), _ptr(re), _ptr(im), frames), "llz_stft_mc_analysis")
        return re, im

    def synthesis(self, re, im, x):
        frames = re.shape[1]
        check(self._L.llz_stft_mc_synthesis(self.handle, _ptr(re), _ptr(im), _ptr(x), frames), "llz_stft_mc_synthesis")
        return x

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_stft_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


def pfb_prototype(bands, taps_per_band, win=KAISER):
    """A prototype for PfbMC: the windowed-sinc low-pass of llz_fir_lpf_cof with bands * taps_per_band taps and cutoff 1 / bands,
    as float32, scaled so that the squares of every bands / 4-th tap sum to about 1 (w = g at a hop of bands / 4 then returns the
    input at about unit gain).  A convenience: how well a prototype reconstructs is its own property."""
    h = fir_design("lpf", bands * taps_per_band, 1.0 / bands, win=win)
    return (h * np.sqrt((bands // 4) / np.sum(h * h))).astype(np.float32)


class PfbMC:
    """llz_pfb_mc_*: the uniform DFT polyphase filter bank (include/llz_pfb.h), many channels and frames per call, float32;
    x [channels, frames*hop], re/im [channels, frames, bins]; w (and g, default w): [taps_per_band * bands] float32 prototypes,
    index 0 on a frame's oldest sample.  The handle carries both streams' state between calls."""

    def __init__(self, channels, bands, hop, taps_per_band, w, g=None, phase=PFB_PHASE_FRAME, stream=None):
        self._L = capi.lib()
        n = bands * taps_per_band
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float32)
        g = None if g is None else np.ascontiguousarray(g, dtype=np.float32)
        for name, a in (("w", w), ("g", g)):
            if a is not None and n > 0 and a.size != n:
                raise LlzError(f"PfbMC: {name} holds {a.size} values, taps_per_band * bands = {n}")
        self.handle = check_handle(self._L.llz_pfb_mc_init(channels, bands, hop, taps_per_band,
                                                           None if w is None else w.ctypes.data,
                                                           None if g is None else g.ctypes.data, phase), "llz_pfb_mc_init")
        self.channels, self.bands, self.hop, self.taps_per_band, self.phase = channels, bands, hop, taps_per_band, phase
        self.bins = self._L.llz_pfb_mc_bins(self.handle)
        self.delay = self._L.llz_pfb_mc_delay(self.handle)
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        check(self._L.llz_pfb_mc_set_stream(self.handle, _stream_ptr(stream)), "llz_pfb_mc_set_stream")

    def _frames(self, x, re, im):
        frames = re.shape[1] if len(re.shape) == 3 else 0
        _typed(x, "float32", self.channels * frames * self.hop, "PfbMC x")
        _typed(re, "float32", self.channels * frames * self.bins, "PfbMC re")
        _typed(im, "float32", self.channels * frames * self.bins, "PfbMC im")
        return frames

    def analysis(self, x, re, im):
        frames = self._frames(x, re, im)
        check(self._L.llz_pfb_mc_analysis(self.handle, _ptr(x), _ptr(re), _ptr(im), frames), "llz_pfb_mc_analysis")
        return re, im

    def synthesis(self, re, im, x):
        frames = self._frames(x, re, im)
        check(self._L.llz_pfb_mc_synthesis(self.handle, _ptr(re), _ptr(im), _ptr(x), frames), "llz_pfb_mc_synthesis")
        return x

    def reset(self):
        check(self._L.llz_pfb_mc_reset(self.handle), "llz_pfb_mc_reset")

    def frames(self):
        """(analysis, synthesis) frames taken since init or reset"""
        a, s = C.c_longlong(), C.c_longlong()
        check(self._L.llz_pfb_mc_frames(self.handle, C.byref(a), C.byref(s)), "llz_pfb_mc_frames")
        return a.value, s.value

    def plan(self, frames):
        """what a call of `frames` frames launches, per direction: (form, frames per workgroup, workgroups, LDS bytes) of the
        analysis (form 0: a run's span staged in LDS, 1: samples read through the caches) and of the synthesis' inverse transforms"""
        out = (C.c_int * 8)()
        check(self._L.llz_pfb_mc_plan(self.handle, frames, out), "llz_pfb_mc_plan")
        return tuple(out[:4]), tuple(out[4:])

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_pfb_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


class MdctFramesMC:
    """llz_mdct_frames_mc_*: windowed 50 %-overlap MDCT frames (the batch form of llz_analysis_mdct / llz_synthesis_mdct);
    x [channels, frames*frame_len] float32, X [channels, frames, frame_len]; the handle carries both streams' state."""

    def __init__(self, channels, frame_len, win=capi.MDCT_SINE, stream=None):
        self._L = capi.lib()
        self.handle = check_handle(self._L.llz_mdct_frames_mc_init(channels, frame_len, win), "llz_mdct_frames_mc_init")
        self.channels, self.frame_len = channels, frame_len
        if stream is not None:
            check(self._L.llz_mdct_frames_mc_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def _frames(self, x, X):
        _typed(x, "float32", self.channels * X.shape[1] * self.frame_len, "x")
        _typed(X, "float32", self.channels * X.shape[1] * self.frame_len, "X")
        return X.shape[1]

    def analysis(self, x, X):
        check(self._L.llz_mdct_frames_mc_analysis(self.handle, _ptr(x), _ptr(X), self._frames(x, X)), "llz_mdct_frames_mc_analysis")
        return X

    def synthesis(self, X, x):
        check(self._L.llz_mdct_frames_mc_synthesis(self.handle, _ptr(X), _ptr(x), self._frames(x, X)), "llz_mdct_frames_mc_synthesis")
        return x

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_mdct_frames_mc_uninit(self.handle)
            self.handle = 0

    __del__ = close


# ------------------------------------------------------------------------------------------ MDCT
def mdct_window(win, n, alpha=6.0):
    w = np.zeros(n)
    if win == capi.MDCT_SINE:
        capi.lib().llz_mdct_sine(w.ctypes.data_as(_dp), n)
    else:
        capi.lib().llz_mdct_kbd(w.ctypes.data_as(_dp), n, alpha)
    return w


class Mdct:
    """llz_mdct_init / llz_mdct / llz_imdct (llz_mdct.h:37-41): one frame per call, host float64, exact."""

    def __init__(self, type_, length):
        self._L = capi.lib()
        self.handle = check_handle(self._L.llz_mdct_init(type_, length), "llz_mdct_init")
        self.length = length

    def forward(self, x):
        x = _f64(x)
        X = np.zeros(self.length // 2)
        self._L.llz_mdct(self.handle, x.ctypes.data_as(_dp), X.ctypes.data_as(_dp))
        return X

    def inverse(self, X):
        X = _f64(X)
        x = np.zeros(self.length)
        self._L.llz_imdct(self.handle, X.ctypes.data_as(_dp), x.ctypes.data_as(_dp))
        return x

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_mdct_uninit(self.handle)
            self.handle = 0

    __del__ = close


class MdctFixed:
    """llz_mdct_fixed_init / llz_mdct_fixed / llz_imdct_fixed (llz_mdct_fixed.h:24-28): host int32, bit-exact."""

    def __init__(self, type_, length):
        self._L = capi.lib()
        self.handle = check_handle(self._L.llz_mdct_fixed_init(type_, length), "llz_mdct_fixed_init")
        self.length = length

    def _run(self, fn, a, n_out):
        a = np.ascontiguousarray(a, dtype=np.int32)
        b = np.zeros(n_out, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        fn(self.handle, a.ctypes.data_as(ip), b.ctypes.data_as(ip))
        return b

    def forward(self, x):
        return self._run(self._L.llz_mdct_fixed, x, self.length // 2)

    def inverse(self, X):
        return self._run(self._L.llz_imdct_fixed, X, self.length)

    def _batch(self, fn, what, a, b, n_in, n_out):
        """a [count][n_in] -> b [count][n_out]: int32 numpy arrays (staged) or device tensors (in place, on the handle's stream)"""
        count = int(a.shape[0])
        assert tuple(a.shape) == (count, n_in) and tuple(b.shape) == (count, n_out)
        check(fn(self.handle, _ptr(a), _ptr(b), count), what)
        return b

    def forward_batch(self, x, X):
        return self._batch(self._L.llz_mdct_fixed_batch, "llz_mdct_fixed_batch", x, X, self.length, self.length // 2)

    def inverse_batch(self, X, x):
        return self._batch(self._L.llz_imdct_fixed_batch, "llz_imdct_fixed_batch", X, x, self.length // 2, self.length)

    def set_stream(self, stream):
        check(self._L.llz_mdct_fixed_set_stream(self.handle, C.c_void_p(stream.cuda_stream if stream is not None else 0)),
              "llz_mdct_fixed_set_stream")

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_mdct_fixed_uninit(self.handle)
            self.handle = 0

    __del__ = close


class _MdctFrames:
    _init = _uninit = _run = None

    def __init__(self, frame_len, win=0):
        self._L = capi.lib()
        self.handle = check_handle(getattr(self._L, self._init)(frame_len, win), self._init)
        self.frame_len = frame_len

    def frame(self, a):
        a = _f64(a)
        b = np.zeros(self.frame_len)
        getattr(self._L, self._run)(self.handle, a.ctypes.data_as(_dp), b.ctypes.data_as(_dp))
        return b

    def close(self):
        if getattr(self, "handle", 0):
            getattr(self._L, self._uninit)(self.handle)
            self.handle = 0

    __del__ = close


class AnalysisMdct(_MdctFrames):
    _init, _uninit, _run = "llz_analysis_mdct_init", "llz_analysis_mdct_uninit", "llz_analysis_mdct"


class SynthesisMdct(_MdctFrames):
    _init, _uninit, _run = "llz_synthesis_mdct_init", "llz_synthesis_mdct_uninit", "llz_synthesis_mdct"


class MdctBatch:
    """llz_mdct_batch_*: many float32 frames per call, N/4-point-FFT algorithm; x [count, len], X [count, len/2]."""

    def __init__(self, length, stream=None):
        self._L = capi.lib()
        self.handle = check_handle(self._L.llz_mdct_batch_init(length), "llz_mdct_batch_init")
        self.length = length
        if stream is not None:
            check(self._L.llz_mdct_batch_set_stream(self.handle, _stream_ptr(stream)), "set_stream")

    def forward(self, x, X):
        check(self._L.llz_mdct_batch(self.handle, _ptr(x), _ptr(X), x.shape[0]), "llz_mdct_batch")
        return X

    def inverse(self, X, x):
        check(self._L.llz_imdct_batch(self.handle, _ptr(X), _ptr(x), X.shape[0]), "llz_imdct_batch")
        return x

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_mdct_batch_uninit(self.handle)
            self.handle = 0

    __del__ = close


# ------------------------------------------------------------------------------------------ PCM ingest / egress
def pcm_deinterleave(ileaved, planar, scale=1.0 / 32768.0, stream=None):
    """ileaved: [n, channels] int16 -> planar: [channels, n] float32."""
    n, ch = ileaved.shape
    check(capi.lib().llz_pcm_deinterleave_i16_f32(_ptr(ileaved), _ptr(planar), ch, n, scale, _stream_ptr(stream)),
          "llz_pcm_deinterleave_i16_f32")
    return planar


def pcm_interleave(planar, ileaved, scale=32768.0, stream=None):
    """planar: [channels, n] float32 -> ileaved: [n, channels] int16 (clamp, truncate toward zero)."""
    ch, n = planar.shape
    check(capi.lib().llz_pcm_interleave_f32_i16(_ptr(planar), _ptr(ileaved), ch, n, scale, _stream_ptr(stream)),
          "llz_pcm_interleave_f32_i16")
    return ileaved


# ------------------------------------------------------------------------------------------ synthetic PCM
def synth_f32(dst, seed, chan0=0, stream=None):
    """Fill a [channels, n] float32 device tensor with the counter-hash PCM of SURVEY.md 8(d)."""
    ch, n = dst.shape
    check(capi.lib().llz_hip_synth_f32(_ptr(dst), ch, n, dst.stride(0), seed, chan0, _stream_ptr(stream)),
          "llz_hip_synth_f32")
    return dst


def synth_i16(dst, seed, chan0=0, stream=None):
    ch, n = dst.shape
    check(capi.lib().llz_hip_synth_i16(_ptr(dst), ch, n, dst.stride(0), seed, chan0, _stream_ptr(stream)),
          "llz_hip_synth_i16")
    return dst


# ------------------------------------------------------------------------------------------ sharded handles (llz_shard.h)
class _Sharded:
    """One batch handle over several GPUs of a node, single process (include/llz_shard.h): contiguous channel ranges, one
    stream per shard, tables broadcast from the first device at init.  Buffers are passed per shard (lists)."""

    def _finish_init(self, handle, what):
        self.handle = check_handle(handle, what)
        L = self._L
        self.n_shards = check(L.llz_sharded_count(self.handle), "llz_sharded_count")
        self.shards = []
        for s in range(self.n_shards):
            dev, c0, cnt = C.c_int(), C.c_int(), C.c_int()
            check(L.llz_sharded_shard(self.handle, s, C.byref(dev), C.byref(c0), C.byref(cnt)), "llz_sharded_shard")
            self.shards.append((dev.value, c0.value, cnt.value))

    def _ptrs(self, bufs):
        if len(bufs) != self.n_shards:
            raise LlzError(f"{len(bufs)} buffers for {self.n_shards} shards")
        return (C.c_void_p * self.n_shards)(*[_ptr(b) for b in bufs])

    def split(self, tensor):
        """views of a [channels, ...] tensor / array, one per shard.  Host arrays are staged by each shard; a DEVICE tensor can
        only serve shards that live on its own GPU (the library refuses a buffer of another device, it never enables peer
        access), so with shards on several GPUs allocate per shard instead: see alloc()."""
        if hasattr(tensor, "is_cuda") and tensor.is_cuda:
            other = sorted({d for (d, _c0, _cnt) in self.shards if d != tensor.device.index})
            if other:
                raise LlzError(f"split(): tensor is on cuda:{tensor.device.index}, shards also live on GPU(s) {other}")
        return [tensor[c0:c0 + cnt] for (_d, c0, cnt) in self.shards]

    def alloc(self, per_channel, dtype):
        """one torch tensor [count, per_channel] per shard, each on its shard's GPU"""
        import torch
        return [torch.empty(cnt, per_channel, dtype=dtype, device=torch.device("cuda", d)) for (d, _c0, cnt) in self.shards]

    @property
    def rccl_ranks(self):
        return check(self._L.llz_sharded_rccl_ranks(self.handle), "llz_sharded_rccl_ranks")

    def synchronize(self):
        check(self._L.llz_sharded_synchronize(self.handle), "llz_sharded_synchronize")

    def timer_start(self):
        check(self._L.llz_sharded_timer_start(self.handle), "llz_sharded_timer_start")

    def timer_stop(self):
        check(self._L.llz_sharded_timer_stop(self.handle), "llz_sharded_timer_stop")

    def timer_ms(self):
        per = np.zeros(self.n_shards)
        ms = self._L.llz_sharded_timer_ms(self.handle, per.ctypes.data_as(_dp))
        if ms < 0:
            raise LlzError("llz_sharded_timer_ms: " + capi.last_error())
        return ms, per

    def close(self):
        if getattr(self, "handle", 0):
            self._L.llz_sharded_uninit(self.handle)
            self.handle = 0

    __del__ = close


def _devlist(devices):
    return (C.c_int * len(devices))(*[int(d) for d in devices])


class FirFilterMCSharded(_Sharded):
    def __init__(self, channels, frame_len, taps, devices, algo=FIR_ALGO_AUTO):
        self._L = capi.lib()
        taps32 = np.ascontiguousarray(_f64(taps).astype(np.float32))
        self.frame_len, self.flt_len = frame_len, len(taps32)
        self._finish_init(self._L.llz_fir_filter_mc_sharded_init(channels, frame_len, taps32.ctypes.data, len(taps32), algo,
                                                                 _devlist(devices), len(devices)),
                          "llz_fir_filter_mc_sharded_init")

    def filter(self, xs, outs):
        check(self._L.llz_fir_filter_mc_sharded(self.handle, self._ptrs(xs), self._ptrs(outs), self.frame_len),
              "llz_fir_filter_mc_sharded")
        return outs

    def flush(self, outs):
        return check(self._L.llz_fir_filter_mc_sharded_flush(self.handle, self._ptrs(outs)), "llz_fir_filter_mc_sharded_flush")


class IirCascadeMCSharded(_Sharded):
    def __init__(self, channels, coef, devices):
        self._L = capi.lib()
        coef = _f64(coef).reshape(-1, 6)
        self._finish_init(self._L.llz_iir_cascade_mc_sharded_init(channels, coef.shape[0], coef.ctypes.data,
                                                                  _devlist(devices), len(devices)),
                          "llz_iir_cascade_mc_sharded_init")

    def filter(self, xs, outs):
        n = xs[0].shape[-1]
        check(self._L.llz_iir_cascade_mc_sharded(self.handle, self._ptrs(xs), self._ptrs(outs), n),
              "llz_iir_cascade_mc_sharded")
        return outs


class ResampleMCSharded(_Sharded):
    def __init__(self, channels, L, M, gain, win, fmt, devices):
        self._L = capi.lib()
        self.L, self.M = L, M
        self._finish_init(self._L.llz_resample_mc_sharded_init(channels, L, M, gain, win, fmt, _devlist(devices),
                                                               len(devices)), "llz_resample_mc_sharded_init")

    def process(self, xs, outs):
        n_in = xs[0].shape[-1]
        return check(self._L.llz_resample_mc_sharded(self.handle, self._ptrs(xs), n_in, self._ptrs(outs)),
                     "llz_resample_mc_sharded")
