"""HPSS -- ctypes mirror of the reference wrapper class (python/audioflux/mir/hpss.py:14-200) over
libaudioflux_mi355x.so: same constructor arguments and defaults, `cal_data_length`, `hpss` -> (h_arr, p_arr).  All leading
axes of the input go through ONE batched call where the reference loops over channels.  Extra: device-resident calls on
torch tensors (`hpss_device`, `spectra_device`) and the sliding median on its own (`median_filter_device`)."""
import ctypes
from ctypes import POINTER, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util
from .types import WindowType


class HPSS:
    def __init__(self, radix2_exp=12, window_type=WindowType.HAMM, slide_length=1024, h_order=21, p_order=31):
        """slide_length is accepted and ignored, as in the reference: the hop is always fft_length // 4"""
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        self.radix2_exp, self.window_type, self.slide_length = radix2_exp, window_type, slide_length
        self.h_order, self.p_order = h_order, p_order
        self.fft_length = 1 << radix2_exp
        fn = self._lib.hpssObj_new
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)]
        st = fn(ctypes.byref(self._obj), radix2_exp, _util.opt_int(int(window_type)), _util.opt_int(slide_length),
                _util.opt_int(h_order), _util.opt_int(p_order))
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"hpssObj_new failed with status {st}: {_lib.last_error()}")

    def cal_data_length(self, data_length):
        fn = self._lib.hpssObj_calDataLength
        fn.restype, fn.argtypes = c_int, [c_void_p, c_int]
        return int(fn(self._obj, int(data_length)))

    def cal_time_length(self, data_length):
        """frames of one clip (0 below fft_length samples)"""
        n, hop = self.fft_length, self.fft_length // 4
        return 0 if data_length < n else (int(data_length) - n) // hop + 1

    def hpss(self, data_arr):
        """data_arr (..., n) -> h_arr, p_arr (..., cal_data_length(n)) float32"""
        x = _util.as_f32(data_arr)
        if x.ndim < 1 or x.shape[-1] < 1:
            raise ValueError("data_arr must have at least one sample")
        n = x.shape[-1]
        m = self.cal_data_length(n)
        if x.ndim == 1:
            h, p = np.zeros(m, np.float32), np.zeros(m, np.float32)
            fn = self._lib.hpssObj_hpss
            fn = _lib.checked(fn)
            fn.restype = None
            fn.argtypes = [c_void_p, _util.c_float_p, c_int, _util.c_float_p, _util.c_float_p]
            fn(self._obj, _util.fptr(x), n, _util.fptr(h), _util.fptr(p))
            return h, p
        import torch
        clips, lead = _util.flatten_leading(x, 1)
        h, p = self.hpss_device(torch.from_numpy(np.ascontiguousarray(clips)).to("cuda"))
        torch.cuda.current_stream().synchronize()
        return _util.restore_leading(h.cpu().numpy(), lead), _util.restore_leading(p.cpu().numpy(), lead)

    # -- additive: device-resident batches ----------------------------------
    def hpss_device(self, x, stream=None, harmonic=True, percussive=True):
        """x: CUDA/HIP torch.float32 (clips, n) -> (h, p) torch (clips, cal_data_length(n)); an output that is switched off is
        None and costs nothing.  Asynchronous on `stream` or torch's current stream."""
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        assert harmonic or percussive
        b, n = x.shape
        m = self.cal_data_length(n)
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        with torch.cuda.stream(s):  # the zero fill is ordered before the kernels that add onto it
            h = torch.zeros((b, m), dtype=torch.float32, device=x.device) if harmonic else None
            p = torch.zeros((b, m), dtype=torch.float32, device=x.device) if percussive else None
        fn = self._lib.hpssObj_hpssBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_void_p, c_longlong, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), h.data_ptr() if harmonic else None,
                      p.data_ptr() if percussive else None, m, s.cuda_stream), "hpssObj_hpssBatchDevice")
        return h, p

    def spectra_device(self, x, stream=None):
        """x: torch (clips, n) -> (h_mag, p_mag) torch (clips, time, fft_length // 2 + 1): the masked magnitudes, no inverse"""
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        b, n = x.shape
        t = self.cal_time_length(n)
        h = torch.empty((b, t, self.fft_length // 2 + 1), dtype=torch.float32, device=x.device)
        p = torch.empty_like(h)
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        fn = self._lib.hpssObj_spectraBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_void_p, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), h.data_ptr(), p.data_ptr(), s.cuda_stream),
                   "hpssObj_spectraBatchDevice")
        return h, p

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.hpssObj_free
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)


def median_filter_device(x, order, axis=0, frames_per_clip=0, stream=None):
    """x: CUDA/HIP torch.float32 (rows, cols), contiguous -> the 1-D median of odd `order` (1 ... 255) along `axis`, zeros outside
    the plane; along axis 0 never across a clip of frames_per_clip rows (0: one clip).  Exact selection."""
    import torch
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    out = torch.empty_like(x)
    s = stream if stream is not None else torch.cuda.current_stream(x.device)
    fn = _lib.get_lib().afx_medianFilterDevice
    fn.restype = c_int
    fn.argtypes = [c_void_p, c_longlong, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    _lib.check(fn(x.data_ptr(), x.shape[0], x.shape[1], int(frames_per_clip), int(axis), int(order), out.data_ptr(), s.cuda_stream),
               "afx_medianFilterDevice")
    return out
