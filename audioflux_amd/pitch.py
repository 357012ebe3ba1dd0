"""PitchYIN, PitchHPS, PitchLHS, PitchPEF -- ctypes mirrors of the reference wrapper classes.  PitchYIN: ctypes mirror of the reference wrapper class (python/audioflux/mir/pitch_yin.py:10-150) over
libaudioflux_mi355x.so: same constructor arguments and defaults, `set_thresh`, `cal_time_length`, `pitch` ->
(fre_arr, value1_arr, value2_arr).  All leading axes of the input go through ONE batched call where the reference loops over
channels.  Extra: device-resident calls on torch tensors (`pitch_device`, `troughs_device`, `curve_device`)."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util
from .types import WindowType


class PitchYIN:
    def __init__(self, samplate=32000, low_fre=27.0, high_fre=2000.0, radix2_exp=12, slide_length=1024, auto_length=2048):
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        self.samplate, self.low_fre, self.high_fre = samplate, low_fre, high_fre
        self.radix2_exp, self.slide_length, self.auto_length = radix2_exp, slide_length, auto_length
        self.fft_length = 1 << radix2_exp
        self.is_continue = False
        fn = self._lib.pitchYINObj_new
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_int), POINTER(c_int),
                       POINTER(c_int), POINTER(c_int)]
        st = fn(ctypes.byref(self._obj), _util.opt_int(samplate), _util.opt_float(low_fre), _util.opt_float(high_fre),
                _util.opt_int(radix2_exp), _util.opt_int(slide_length), _util.opt_int(auto_length), _util.opt_int(0))
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"pitchYINObj_new failed with status {st}: {_lib.last_error()}")
        for name in ("pitchYINObj_yinLength", "pitchYINObj_minIndex", "pitchYINObj_calTimeLength"):
            getattr(self._lib, name).restype = c_int
        self._lib.pitchYINObj_yinLength.argtypes = self._lib.pitchYINObj_minIndex.argtypes = [c_void_p]
        self._lib.pitchYINObj_calTimeLength.argtypes = [c_void_p, c_int]
        self.yin_length = int(self._lib.pitchYINObj_yinLength(self._obj))
        self.min_index = int(self._lib.pitchYINObj_minIndex(self._obj))

    def set_thresh(self, thresh):
        """default 0.1; values <= 0 are ignored, as in the reference"""
        fn = self._lib.pitchYINObj_setThresh
        fn.restype, fn.argtypes = None, [c_void_p, c_float]
        fn(self._obj, c_float(thresh))

    def cal_time_length(self, data_length):
        return int(self._lib.pitchYINObj_calTimeLength(self._obj, int(data_length)))

    def pitch(self, data_arr):
        """data_arr (..., n) -> fre_arr, value1_arr, value2_arr (..., time) float32: frequency of the first trough of the YIN
        curve below the threshold (0 where there is none), the curve's value there, and the curve's minimum"""
        x = _util.as_f32(data_arr)
        if x.ndim < 1 or x.shape[-1] < 1:
            raise ValueError("data_arr must have at least one sample")
        n = x.shape[-1]
        t = self.cal_time_length(n)
        if x.ndim == 1:
            fre, v1, v2 = (np.zeros(t, np.float32) for _ in range(3))
            fn = _lib.checked(self._lib.pitchYINObj_pitch)
            fn.restype = None
            fn.argtypes = [c_void_p, _util.c_float_p, c_int, _util.c_float_p, _util.c_float_p, _util.c_float_p]
            fn(self._obj, _util.fptr(x), n, _util.fptr(fre), _util.fptr(v1), _util.fptr(v2))
            return fre, v1, v2
        import torch
        clips, lead = _util.flatten_leading(x, 1)
        out = self.pitch_device(torch.from_numpy(np.ascontiguousarray(clips)).to("cuda"))
        torch.cuda.current_stream().synchronize()
        return tuple(_util.restore_leading(o.cpu().numpy(), lead) for o in out)

    # -- additive: device-resident batches ----------------------------------
    def _args(self, x, stream):
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        return x.shape[0], x.shape[1], self.cal_time_length(x.shape[1]), s

    def pitch_device(self, x, stream=None):
        """x: CUDA/HIP torch.float32 (clips, n) -> (fre, value1, value2) torch (clips, time).  Every frame is written: fre and
        value1 are 0 where no trough qualifies.  One launch, asynchronous on `stream` or torch's current stream."""
        import torch
        b, n, t, s = self._args(x, stream)
        fre, v1, v2 = (torch.empty((b, t), dtype=torch.float32, device=x.device) for _ in range(3))
        if t == 0:  # fewer samples than a frame
            return fre, v1, v2
        fn = self._lib.pitchYINObj_pitchBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_void_p, c_void_p, c_longlong, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), fre.data_ptr(), v1.data_ptr(), v2.data_ptr(), max(t, 1),
                      s.cuda_stream), "pitchYINObj_pitchBatchDevice")
        return fre, v1, v2

    def troughs_device(self, x, max_troughs=4, stream=None):
        """x: torch (clips, n) -> (fre, value, count): the first max_troughs troughs below the threshold per frame in lag order,
        torch (clips, time, max_troughs) -- entries behind a frame's count are 0 --, and the count of ALL of them (clips, time) int32"""
        import torch
        b, n, t, s = self._args(x, stream)
        with torch.cuda.stream(s):
            fre = torch.zeros((b, t, max_troughs), dtype=torch.float32, device=x.device)
            val = torch.zeros_like(fre)
        cnt = torch.empty((b, t), dtype=torch.int32, device=x.device)
        if t == 0:
            return fre, val, cnt
        fn = self._lib.pitchYINObj_troughsBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_void_p, c_void_p, c_int, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), fre.data_ptr(), val.data_ptr(), cnt.data_ptr(), int(max_troughs),
                      s.cuda_stream), "pitchYINObj_troughsBatchDevice")
        return fre, val, cnt

    def curve_device(self, x, stream=None):
        """x: torch (clips, n) -> the cumulative-mean-normalised difference curve, torch (clips, time, yin_length); column k is
        lag min_index + k"""
        import torch
        b, n, t, s = self._args(x, stream)
        out = torch.empty((b, t, self.yin_length), dtype=torch.float32, device=x.device)
        if t == 0:
            return out
        fn = self._lib.pitchYINObj_curveBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), out.data_ptr(), s.cuda_stream), "pitchYINObj_curveBatchDevice")
        return out

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.pitchYINObj_free
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)


class _PitchHS:
    """What PitchHPS and PitchLHS share (python/audioflux/mir/pitch_hps.py:14-172, pitch_lhs.py): same constructor arguments
    and defaults, `cal_time_length`, `pitch` -> fre_arr.  Extra: `pitch_batch_device` / `curve_batch_device` on torch
    tensors.  `_name` selects the exported names."""
    _name = None

    def __init__(self, samplate=32000, low_fre=32.0, high_fre=2000.0, radix2_exp=12, slide_length=1024, window_type=WindowType.HAMM,
                 harmonic_count=5):
        if low_fre >= high_fre:
            raise ValueError("`low_fre` must be smaller than `high_fre`")
        if harmonic_count <= 0:
            raise ValueError("`harmonic_count` must be greater than 0.")
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        self.samplate, self.low_fre, self.high_fre = samplate, low_fre, high_fre
        self.radix2_exp, self.slide_length, self.window_type = radix2_exp, slide_length, window_type
        self.fft_length = 1 << radix2_exp
        self.is_continue = False
        fn = self._fn("new")
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_int), POINTER(c_int),
                       POINTER(c_int), POINTER(c_int), POINTER(c_int)]
        st = fn(ctypes.byref(self._obj), _util.opt_int(samplate), _util.opt_float(low_fre), _util.opt_float(high_fre),
                _util.opt_int(radix2_exp), _util.opt_int(slide_length), _util.opt_int(window_type), _util.opt_int(harmonic_count),
                _util.opt_int(0))
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"pitch{self._name}Obj_new failed with status {st}: {_lib.last_error()}")
        for name in ("minIndex", "maxIndex", "harmonicCount", "interpLength"):
            g = self._fn(name)
            g.restype, g.argtypes = c_int, [c_void_p]
        self._fn("calTimeLength").restype = c_int
        self._fn("calTimeLength").argtypes = [c_void_p, c_int]
        self.min_index = int(self._fn("minIndex")(self._obj))
        self.max_index = int(self._fn("maxIndex")(self._obj))
        self.harmonic_count = int(self._fn("harmonicCount")(self._obj))  # as the object uses it (mir/_pitch_hps.h)
        self.interp_length = int(self._fn("interpLength")(self._obj))

    def _fn(self, what):
        return getattr(self._lib, f"pitch{self._name}Obj_{what}")

    def cal_time_length(self, data_length):
        return int(self._fn("calTimeLength")(self._obj, int(data_length)))

    def pitch(self, data_arr):
        """data_arr (..., n) -> fre_arr (..., time) float32: (index + 1) * samplate / interp_length of the first maximum of the
        harmonic curve over min_index ... max_index"""
        x = _util.as_f32(data_arr)
        if x.ndim < 1 or x.shape[-1] < 1:
            raise ValueError("data_arr must have at least one sample")
        n = x.shape[-1]
        t = self.cal_time_length(n)
        if x.ndim == 1:
            fre = np.zeros(t, np.float32)
            fn = _lib.checked(self._fn("pitch"))
            fn.restype = None
            fn.argtypes = [c_void_p, _util.c_float_p, c_int, _util.c_float_p]
            fn(self._obj, _util.fptr(x), n, _util.fptr(fre))
            return fre
        import torch
        clips, lead = _util.flatten_leading(x, 1)
        fre, _ = self.pitch_batch_device(torch.from_numpy(np.ascontiguousarray(clips)).to("cuda"))
        torch.cuda.current_stream().synchronize()
        return _util.restore_leading(fre.cpu().numpy(), lead)

    # -- additive: device-resident batches ----------------------------------
    def _args(self, x, stream):
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        return x.shape[0], x.shape[1], self.cal_time_length(x.shape[1]), s

    def pitch_batch_device(self, x, stream=None):
        """x: CUDA/HIP torch.float32 (clips, n) -> (fre, value) torch (clips, time): the frequency and the curve's value at the
        chosen index.  One launch, asynchronous on `stream` or torch's current stream."""
        import torch
        b, n, t, s = self._args(x, stream)
        fre, val = (torch.empty((b, t), dtype=torch.float32, device=x.device) for _ in range(2))
        if t == 0:  # fewer samples than a frame
            return fre, val
        fn = self._fn("pitchBatchDevice")
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_void_p, c_longlong, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), fre.data_ptr(), val.data_ptr(), max(t, 1), s.cuda_stream),
                   f"pitch{self._name}Obj_pitchBatchDevice")
        return fre, val

    def curve_batch_device(self, x, stream=None):
        """x: torch (clips, n) -> the harmonic curve, torch (clips, time, max_index + 1); column j is candidate bin j (the
        entries below min_index included)"""
        import torch
        b, n, t, s = self._args(x, stream)
        out = torch.empty((b, t, self.max_index + 1), dtype=torch.float32, device=x.device)
        if t == 0:
            return out
        fn = self._fn("curveBatchDevice")
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), out.data_ptr(), s.cuda_stream),
                   f"pitch{self._name}Obj_curveBatchDevice")
        return out

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._fn("free")
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)


class PitchHPS(_PitchHS):
    """Harmonic product spectrum (include/mir/_pitch_hps.h): curve[j] = prod_k |X[j (k + 1)]|.  A window type above HAMM falls
    back to HAMM and harmonic_count is used as given, as in the reference."""
    _name = "HPS"


class PitchLHS(_PitchHS):
    """Log-harmonic sum (include/mir/_pitch_lhs.h): curve[j] = sum_k log |X[j (k + 1)]|.  Every window type is taken as given and
    harmonic_count is clamped to samplate // (max_index + 1), as in the reference."""
    _name = "LHS"


class PitchPEF:
    """Mirrors audioflux.PitchPEF (python/audioflux/mir/pitch_pef.py:14-227; include/mir/_pitch_pef.h): same constructor
    arguments, defaults and ValueErrors, `cal_time_length`, `set_filter_params`, `pitch` -> fre_arr.  Extra:
    `pitch_batch_device` / `curve_batch_device` on torch tensors."""

    def __init__(self, samplate=32000, low_fre=32.0, high_fre=2000.0, cut_fre=4000.0, radix2_exp=12, slide_length=1024,
                 window_type=WindowType.HAMM, alpha=10.0, beta=0.5, gamma=1.8):
        if low_fre >= high_fre:
            raise ValueError("`low_fre` must be smaller than `high_fre`")
        if high_fre >= cut_fre:
            raise ValueError("`high_fre` must be smaller than `cut_fre`")
        self._check_filter(alpha, beta, gamma)
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        self.samplate, self.low_fre, self.high_fre, self.cut_fre = samplate, low_fre, high_fre, cut_fre
        self.radix2_exp, self.slide_length, self.window_type = radix2_exp, slide_length, window_type
        self.alpha, self.beta, self.gamma = alpha, beta, gamma
        self.fft_length = 1 << radix2_exp
        self.is_continue = False
        fn = self._lib.pitchPEFObj_new
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_int),
                       POINTER(c_int), POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_int)]
        st = fn(ctypes.byref(self._obj), _util.opt_int(samplate), _util.opt_float(low_fre), _util.opt_float(high_fre),
                _util.opt_float(cut_fre), _util.opt_int(radix2_exp), _util.opt_int(slide_length), _util.opt_int(window_type),
                _util.opt_float(alpha), _util.opt_float(beta), _util.opt_float(gamma), _util.opt_int(0))
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"pitchPEFObj_new failed with status {st}: {_lib.last_error()}")
        for name in ("minIndex", "maxIndex", "filterPadNum", "logLength"):
            g = getattr(self._lib, f"pitchPEFObj_{name}")
            g.restype, g.argtypes = c_int, [c_void_p]
        self._lib.pitchPEFObj_calTimeLength.restype = c_int
        self._lib.pitchPEFObj_calTimeLength.argtypes = [c_void_p, c_int]
        self.min_index = int(self._lib.pitchPEFObj_minIndex(self._obj))
        self.max_index = int(self._lib.pitchPEFObj_maxIndex(self._obj))
        self.filter_pad_num = int(self._lib.pitchPEFObj_filterPadNum(self._obj))
        self.log_length = int(self._lib.pitchPEFObj_logLength(self._obj))

    @staticmethod
    def _check_filter(alpha, beta, gamma):
        if alpha <= 0:
            raise ValueError("`alpha` must be greater than 0.")
        if beta < 0 or beta > 1:
            raise ValueError("`beta` must be between 0 and 1.")
        if gamma <= 1:
            raise ValueError("`gamma` must be greater than 1.")

    def cal_time_length(self, data_length):
        return int(self._lib.pitchPEFObj_calTimeLength(self._obj, int(data_length)))

    def set_filter_params(self, alpha, beta, gamma):
        """As in the reference: the arguments are validated and remembered here; the object's filter stays the
        constructor's (include/mir/_pitch_pef.h, the deviations)"""
        self._check_filter(alpha, beta, gamma)
        fn = _lib.checked(self._lib.pitchPEFObj_setFilterParams)
        fn.restype = None
        fn.argtypes = [c_void_p, c_float, c_float, c_float]
        fn(self._obj, alpha, beta, gamma)
        self.alpha, self.beta, self.gamma = alpha, beta, gamma

    def pitch(self, data_arr):
        """data_arr (..., n) -> fre_arr (..., time) float32: the log frequency at the first maximum of the filter's
        correlation with the log spectrum over min_index ... max_index"""
        x = _util.as_f32(data_arr)
        if x.ndim < 1 or x.shape[-1] < 1:
            raise ValueError("data_arr must have at least one sample")
        n = x.shape[-1]
        t = self.cal_time_length(n)
        if x.ndim == 1:
            fre = np.zeros(t, np.float32)
            fn = _lib.checked(self._lib.pitchPEFObj_pitch)
            fn.restype = None
            fn.argtypes = [c_void_p, _util.c_float_p, c_int, _util.c_float_p]
            fn(self._obj, _util.fptr(x), n, _util.fptr(fre))
            return fre
        import torch
        clips, lead = _util.flatten_leading(x, 1)
        fre, _ = self.pitch_batch_device(torch.from_numpy(np.ascontiguousarray(clips)).to("cuda"))
        torch.cuda.current_stream().synchronize()
        return _util.restore_leading(fre.cpu().numpy(), lead)

    # -- additive: device-resident batches ----------------------------------
    def _args(self, x, stream):
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        return x.shape[0], x.shape[1], self.cal_time_length(x.shape[1]), s

    def pitch_batch_device(self, x, stream=None):
        """x: CUDA/HIP torch.float32 (clips, n) -> (fre, value) torch (clips, time): the frequency and the correlation at the
        chosen index.  One launch, asynchronous on `stream` or torch's current stream."""
        import torch
        b, n, t, s = self._args(x, stream)
        fre, val = (torch.empty((b, t), dtype=torch.float32, device=x.device) for _ in range(2))
        if t == 0:  # fewer samples than a frame
            return fre, val
        fn = self._lib.pitchPEFObj_pitchBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_void_p, c_longlong, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), fre.data_ptr(), val.data_ptr(), max(t, 1), s.cuda_stream),
                   "pitchPEFObj_pitchBatchDevice")
        return fre, val

    def curve_batch_device(self, x, stream=None):
        """x: torch (clips, n) -> the correlation curve, torch (clips, time, max_index + 1); column k is lag k (the entries
        below min_index included)"""
        import torch
        b, n, t, s = self._args(x, stream)
        out = torch.empty((b, t, self.max_index + 1), dtype=torch.float32, device=x.device)
        if t == 0:
            return out
        fn = self._lib.pitchPEFObj_curveBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), out.data_ptr(), s.cuda_stream), "pitchPEFObj_curveBatchDevice")
        return out

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.pitchPEFObj_free
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)
