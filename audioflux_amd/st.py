"""ST -- ctypes mirror of python/audioflux/st.py:15-241 over libaudioflux_mi355x.so: the S-transform (one FFT of the chunk,
per bin an inverse transform of the rotated spectrum under a Gaussian window as wide as the bin is high).  Result
(..., num, 2**radix2_exp) complex64, num = max_index - min_index + 1 or the length of the last accepted use_bin_arr."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util


class ST:
    def __init__(self, radix2_exp=12, min_index=1, max_index=None, samplate=32000, factor=1., norm=1.):
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        fft_length = 1 << radix2_exp
        if max_index is None:
            max_index = (fft_length // 2) - 1
        if min_index < 1:
            raise ValueError(f'min_index={min_index} must be a positive integer.')
        if max_index >= (fft_length / 2):
            raise ValueError(f'max_index={max_index} must be less than or equal to fft_length/2={fft_length / 2}')
        if min_index >= max_index:
            raise ValueError(f'min_index={min_index} must be less than max_index={max_index}')
        self.radix2_exp, self.min_index, self.max_index, self.samplate = radix2_exp, min_index, max_index, samplate
        self.factor, self.norm = factor, norm
        self.fft_length = fft_length
        self.num = self.max_index - self.min_index + 1
        self._bins = np.arange(min_index, max_index + 1, dtype=np.int32)
        fn = self._lib.stObj_new
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), c_int, c_int, c_int, POINTER(c_float), POINTER(c_float)]
        st = fn(ctypes.byref(self._obj), radix2_exp, min_index, max_index, ctypes.byref(c_float(factor)),
                ctypes.byref(c_float(norm)))
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"stObj_new failed with status {st}: {_lib.last_error()}")

    def _bin_length(self):
        fn = self._lib.stObj_getBinLength
        fn.argtypes, fn.restype = [c_void_p], c_int
        return fn(self._obj)

    def use_bin_arr(self, bin_arr):
        """the rows from now on: bins in 0 ... fft_length/2, any order, repeats allowed (handed over as int32: the reference
        wrapper hands float32 words to the library's `int *`).  A list with an entry outside that range is ignored, as
        the library does; an empty or over-long one raises."""
        bin_arr = np.ascontiguousarray(bin_arr, dtype=np.int32)
        if bin_arr.ndim != 1:
            raise ValueError('bin_arr is only defined for 1D arrays')
        fn = _lib.checked(self._lib.stObj_useBinArr)
        fn.restype = None
        fn.argtypes = [c_void_p, c_void_p, c_int]
        fn(self._obj, bin_arr.ctypes.data, bin_arr.shape[0])
        if bin_arr.min() >= 0 and bin_arr.max() <= self.fft_length // 2:
            self._bins = bin_arr.copy()
        self.num = self._bin_length()

    def set_value(self, factor, norm):
        fn = _lib.checked(self._lib.stObj_setValue)
        fn.restype = None
        fn.argtypes = [c_void_p, c_float, c_float]
        fn(self._obj, factor, norm)
        self.factor, self.norm = factor, norm

    def get_fre_band_arr(self):
        return self._bins.astype(np.float32) * self.samplate / self.fft_length

    def _fit(self, x):
        n = self.fft_length  # truncate / zero-pad like utils/util.py:98-111
        if x.shape[-1] >= n:
            return np.ascontiguousarray(x[..., :n])
        out = np.zeros(x.shape[:-1] + (n,), np.float32)
        out[..., : x.shape[-1]] = x
        return out

    def st(self, data_arr):
        """data_arr (..., 2**radix2_exp) -> complex64 (..., num, 2**radix2_exp)"""
        x = self._fit(_util.as_f32(data_arr))
        clips, lead = _util.flatten_leading(x, 1)
        re = np.zeros((clips.shape[0], self.num, self.fft_length), np.float32)
        im = np.zeros_like(re)
        fn = _lib.checked(self._lib.stObj_st)
        fn.restype = None
        fn.argtypes = [c_void_p, _util.c_float_p, _util.c_float_p, _util.c_float_p]
        for i in range(clips.shape[0]):
            fn(self._obj, _util.fptr(clips[i]), _util.fptr(re[i]), _util.fptr(im[i]))
        out = np.empty(re.shape, np.complex64)
        out.real, out.imag = re, im
        return _util.restore_leading(out, lead)

    def y_coords(self):
        fre_band_arr = self.get_fre_band_arr()
        return np.insert(fre_band_arr, 0, fre_band_arr[0])

    def x_coords(self):
        return np.linspace(0, self.fft_length / self.samplate, self.fft_length + 1)

    def st_device(self, x, out_real=None, out_imag=None, stream=None):
        """Additive (include/st_algorithm.h: stObj_stBatchDevice): x HIP torch.float32 (chunks, 2**radix2_exp) with
        contiguous rows -> (real, imag) torch (chunks, num, 2**radix2_exp).  Asynchronous on `stream`."""
        import torch
        n = self.fft_length
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == n
        c = x.shape[0]
        if out_real is None:
            out_real = torch.empty((c, self.num, n), dtype=torch.float32, device=x.device)
        if out_imag is None:
            out_imag = torch.empty_like(out_real)
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        fn = self._lib.stObj_stBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_longlong, c_void_p, c_void_p, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), c, x.stride(0), out_real.data_ptr(), out_imag.data_ptr(), s.cuda_stream),
                   "stObj_stBatchDevice")
        return out_real, out_imag

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.stObj_free
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)
