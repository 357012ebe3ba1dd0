"""TimeStretch -- ctypes mirror of the reference wrapper class (python/audioflux/mir/time_stretch.py) over
libaudioflux_mi355x.so: same constructor arguments and defaults, `cal_data_capacity`, `time_stretch` (leading axes are
clips, one call each as in the reference).  Extra: `time_stretch_batch_device` on torch
tensors and `set_scratch_limit`."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util
from .types import WindowType


class TimeStretch:
    """STFT without padding, phase vocoder, weighted-overlap-add inverse (include/mir/timeStretch_algorithm.h).
    rate > 1 shortens the signal, rate < 1 lengthens it."""

    def __init__(self, radix2_exp=12, slide_length=1024, window_type=WindowType.HANN):
        self.radix2_exp, self.slide_length, self.window_type = radix2_exp, slide_length, window_type
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        fn = self._lib.timeStretchObj_new
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), POINTER(c_int), POINTER(c_int), POINTER(c_int)]
        st = fn(ctypes.byref(self._obj), _util.opt_int(radix2_exp), _util.opt_int(slide_length), _util.opt_int(int(window_type)))
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"timeStretchObj_new failed with status {st}: {_lib.last_error()}")
        self.fft_length = 1 << (radix2_exp if radix2_exp is not None and 1 <= radix2_exp <= 30 else 12)
        self._lib.timeStretchObj_calDataCapacity.restype = c_int
        self._lib.timeStretchObj_calDataCapacity.argtypes = [c_void_p, c_float, c_int]

    def cal_data_capacity(self, rate, data_length):
        """ceilf(data_length / rate) + fft_length in float32: the samples per row `time_stretch` returns"""
        return int(self._lib.timeStretchObj_calDataCapacity(self._obj, c_float(rate), int(data_length)))

    def set_scratch_limit(self, nbytes):
        """device scratch the batched call may hold (one clip is always taken); 0: the default of 4 GiB"""
        fn = self._lib.timeStretchObj_setScratchLimit
        fn.restype, fn.argtypes = None, [c_void_p, c_longlong]
        fn(self._obj, int(nbytes))

    def time_stretch(self, data_arr, rate):
        """data_arr (..., n) -> (..., cal_data_capacity(rate, n)) float32: the inverse transform's samples, zeros behind them
        (the rows of the reference's wrapper); roundf(n / rate) of them count as the stretched signal"""
        x = _util.as_f32(data_arr)
        if x.ndim < 1 or x.shape[-1] < 1:
            raise ValueError("data_arr must have at least one sample")
        n = x.shape[-1]
        cap = self.cal_data_capacity(rate, n)
        if cap <= 0:
            raise ValueError(f"rate={rate} must be a positive finite number")
        clips, lead = _util.flatten_leading(x, 1)
        clips = np.ascontiguousarray(clips)
        out = np.zeros((clips.shape[0], cap), np.float32)
        fn = self._lib.timeStretchObj_timeStretch
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_float, _util.c_float_p, c_int, _util.c_float_p]
        for c in range(clips.shape[0]):
            st = fn(self._obj, c_float(rate), _util.fptr(clips[c]), n, _util.fptr(out[c]))
            if st <= 0:
                raise RuntimeError(f"timeStretchObj_timeStretch failed with status {st}: {_lib.last_error()}")
        return out[0] if x.ndim == 1 else _util.restore_leading(out, lead)

    # -- additive: device-resident batches ----------------------------------
    def time_stretch_batch_device(self, x, rate, out=None, stream=None):
        """x: CUDA/HIP torch.float32 (clips, n), rows contiguous -> torch (clips, roundf(n / rate)): every clip stretched on
        its own, the words both calls write bit for bit those of `time_stretch`.  `out`: a tensor to write into, (clips, >=
        that length) with contiguous rows; its first columns are returned.  Asynchronous on `stream` or torch's current
        stream; the batch is worked through in chunks under the scratch limit."""
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        b, n = x.shape
        fn = self._lib.timeStretchObj_timeStretchBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_float, c_void_p, c_int, c_int, c_longlong, c_void_p, c_longlong, c_void_p]
        m = _return_length(self._lib, self.radix2_exp, self.slide_length, rate, n)
        if out is None:
            out = torch.empty((b, m), dtype=torch.float32, device=x.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == b and out.shape[1] >= m
        assert out.stride(1) == 1 or out.shape[1] <= 1
        if b:
            st = fn(self._obj, c_float(rate), x.data_ptr(), b, n, x.stride(0) if b > 1 else n, out.data_ptr(),
                    out.stride(0) if b > 1 else m, s.cuda_stream)
            if st != m:
                raise RuntimeError(f"timeStretchObj_timeStretchBatchDevice failed with status {st}: {_lib.last_error()}")
        return out[:, :m]

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.timeStretchObj_free
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)


class _Plan(ctypes.Structure):
    """AfxTimeStretchPlan"""
    _fields_ = [("fftLength", c_int), ("slideLength", c_int), ("T1", c_int), ("T2", c_int), ("istftLength", c_int),
                ("returnLength", c_int), ("capacity", c_int), ("scratchBytes", c_longlong), ("clipsPerChunk", c_int)]


def _return_length(lib, radix2_exp, slide_length, rate, n):
    """roundf(n / rate) as the library decides it; ValueError for a rate or a length a call refuses"""
    fn = lib.afx_timestretch_plan
    fn.restype = c_int
    fn.argtypes = [c_int, c_int, c_float, c_int, c_int, c_longlong, POINTER(_Plan), c_void_p, c_void_p]
    p = _Plan()
    st = fn(int(radix2_exp), int(slide_length), c_float(rate), int(n), 1, 0, ctypes.byref(p), None, None)
    if st != 0:
        raise ValueError(f"time stretch of {n} samples at rate {rate}: status {st}: {_lib.last_error()}")
    return int(p.returnLength)
