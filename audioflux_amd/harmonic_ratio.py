"""HarmonicRatio -- ctypes mirror of the reference wrapper class (python/audioflux/mir/harmonic_ratio.py:14-148) over
libaudioflux_mi355x.so (include/mir/harmonicRatio_algorithm.h): same constructor arguments and defaults, `cal_time_length`,
`harmonic_ratio`.  All leading axes of the input go through ONE batched call where the reference loops over channels; each
channel is a call of its own there, and a clip of its own here.  Extra: device-resident calls on torch tensors."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util
from .types import WindowType

_C1 = 440.0 * 2.0 ** ((24 - 69) / 12.0)  # note_to_hz('C1') = 32.703...: the reference wrapper's default low_fre


class HarmonicRatio:
    """samplate, low_fre, radix2_exp (window length 2**radix2_exp, transforms of twice that), window_type (kept for the
    signature: the object always uses the Hamming window, as the reference does), slide_length."""

    def __init__(self, samplate=32000, low_fre=_C1, radix2_exp=12, window_type=WindowType.HAMM, slide_length=1024):
        self.samplate, self.low_fre, self.radix2_exp = samplate, low_fre, radix2_exp
        self.window_type, self.slide_length = window_type, slide_length
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        fn = self._lib.harmonicRatioObj_new
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), POINTER(c_int), POINTER(c_float), POINTER(c_int), POINTER(c_int), POINTER(c_int)]
        st = fn(ctypes.byref(self._obj), _util.opt_int(samplate), _util.opt_float(low_fre), _util.opt_int(radix2_exp),
                _util.opt_int(window_type), _util.opt_int(slide_length))
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"harmonicRatioObj_new failed with status {st}: {_lib.last_error()}")
        self._lib.harmonicRatioObj_calTimeLength.restype = c_int
        self._lib.harmonicRatioObj_calTimeLength.argtypes = [c_void_p, c_int]
        for g in ("maxLength", "windowLength"):
            f = getattr(self._lib, f"harmonicRatioObj_{g}")
            f.restype, f.argtypes = c_int, [c_void_p]
        self.max_length = int(self._lib.harmonicRatioObj_maxLength(self._obj))
        self.window_length = int(self._lib.harmonicRatioObj_windowLength(self._obj))
        self.fft_length = 2 * self.window_length

    def cal_time_length(self, data_length):
        return int(self._lib.harmonicRatioObj_calTimeLength(self._obj, int(data_length)))

    def harmonic_ratio(self, data_arr):
        """data_arr (..., n) -> (..., time) float32"""
        x = _util.as_f32(data_arr)
        if x.ndim < 1 or x.shape[-1] < 1:
            raise ValueError("data_arr must have at least one sample")
        n = x.shape[-1]
        t = self.cal_time_length(n)
        if x.ndim == 1:
            out = np.zeros(t, np.float32)
            fn = _lib.checked(self._lib.harmonicRatioObj_harmonicRatio)
            fn.restype = None
            fn.argtypes = [c_void_p, _util.c_float_p, c_int, _util.c_float_p]
            fn(self._obj, _util.fptr(x), n, _util.fptr(out))
            return out
        import torch
        clips, lead = _util.flatten_leading(x, 1)
        value, _, _ = self.harmonic_ratio_batch_device(torch.from_numpy(np.ascontiguousarray(clips)).to("cuda"))
        torch.cuda.current_stream().synchronize()
        return _util.restore_leading(value.cpu().numpy(), lead)

    # -- additive: device-resident batches ----------------------------------
    def _args(self, x, stream):
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        return x.shape[0], x.shape[1], self.cal_time_length(x.shape[1]), s

    def harmonic_ratio_batch_device(self, x, stream=None):
        """x: CUDA/HIP torch.float32 (clips, n) -> (value float32, lag int32, first int32) torch (clips, time): the value, the
        lag of the chosen maximum (-1: the range was empty) and the minIndex the frame used.  Every clip is one reference call.
        Asynchronous on `stream` or torch's current stream."""
        import torch
        b, n, t, s = self._args(x, stream)
        value = torch.empty((b, t), dtype=torch.float32, device=x.device)
        lag, first = (torch.empty((b, t), dtype=torch.int32, device=x.device) for _ in range(2))
        if t:  # (0: fewer samples than a window)
            fn = self._lib.harmonicRatioObj_harmonicRatioBatchDevice
            fn.restype = c_int
            fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_void_p, c_void_p, c_longlong, c_void_p]
            _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), value.data_ptr(), lag.data_ptr(), first.data_ptr(), t,
                          s.cuda_stream), "harmonicRatioObj_harmonicRatioBatchDevice")
        return value, lag, first

    def curve_batch_device(self, x, stream=None):
        """x: torch (clips, n) -> g, torch (clips, time, max_length); column j is lag j, zeros at and below the frame's minIndex"""
        import torch
        b, n, t, s = self._args(x, stream)
        out = torch.empty((b, t, self.max_length), dtype=torch.float32, device=x.device)
        if t:
            fn = self._lib.harmonicRatioObj_curveBatchDevice
            fn.restype = c_int
            fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_void_p]
            _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), out.data_ptr(), s.cuda_stream), "harmonicRatioObj_curveBatchDevice")
        return out

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.harmonicRatioObj_free
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)
