"""FST -- ctypes mirror of python/audioflux/fst.py:15-195 over libaudioflux_mi355x.so: the fast S-transform (one FFT of the
chunk, per dyadic band of the shifted spectrum an inverse transform of the band's own length, then a sample-and-hold of
every band onto the 2**radix2_exp column grid).  Result (..., max_index - min_index + 1, 2**radix2_exp) complex64."""
import ctypes
from ctypes import POINTER, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util


class FST:
    def __init__(self, radix2_exp=12, min_index=1, max_index=None, samplate=32000):
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
        self.fft_length = fft_length
        self.num = self.max_index - self.min_index + 1
        fn = self._lib.fstObj_new
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), c_int]
        st = fn(ctypes.byref(self._obj), radix2_exp)
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"fstObj_new failed with status {st}: {_lib.last_error()}")

    def get_fre_band_arr(self):
        return np.arange(self.min_index, self.max_index + 1, dtype=np.float32) * self.samplate / self.fft_length

    def get_cell_length(self):
        fn = self._lib.fstObj_getCellLength
        fn.argtypes, fn.restype = [c_void_p], c_int
        return fn(self._obj)

    def _fit(self, x):
        n = self.fft_length  # truncate / zero-pad like utils/util.py:98-111
        if x.shape[-1] >= n:
            return np.ascontiguousarray(x[..., :n])
        out = np.zeros(x.shape[:-1] + (n,), np.float32)
        out[..., : x.shape[-1]] = x
        return out

    def fst(self, data_arr):
        """data_arr (..., 2**radix2_exp) -> complex64 (..., num, 2**radix2_exp)"""
        x = self._fit(_util.as_f32(data_arr))
        clips, lead = _util.flatten_leading(x, 1)
        re = np.zeros((clips.shape[0], self.num, self.fft_length), np.float32)
        im = np.zeros_like(re)
        fn = self._lib.fstObj_fst
        fn = _lib.checked(fn)
        fn.restype = None
        fn.argtypes = [c_void_p, _util.c_float_p, c_int, c_int, _util.c_float_p, _util.c_float_p]
        for i in range(clips.shape[0]):
            fn(self._obj, _util.fptr(clips[i]), self.min_index, self.max_index, _util.fptr(re[i]), _util.fptr(im[i]))
        out = np.empty(re.shape, np.complex64)
        out.real, out.imag = re, im
        return _util.restore_leading(out, lead)

    def y_coords(self):
        fre_band_arr = self.get_fre_band_arr()
        return np.insert(fre_band_arr, 0, fre_band_arr[0])

    def x_coords(self):
        return np.linspace(0, self.fft_length / self.samplate, self.fft_length + 1)

    def fst_device(self, x, out_real=None, out_imag=None, cells=False, stream=None):
        """Additive (include/fst_algorithm.h: fstObj_fstBatchDevice): x HIP torch.float32 (chunks, 2**radix2_exp) with
        contiguous rows -> (real, imag) torch (chunks, num, 2**radix2_exp); with cells=True also the cell planes
        (chunks, 2**radix2_exp / 2 + 1): (real, imag, cell_real, cell_imag).  Asynchronous on `stream`."""
        import torch
        n = self.fft_length
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == n
        c = x.shape[0]
        if out_real is None:
            out_real = torch.empty((c, self.num, n), dtype=torch.float32, device=x.device)
        if out_imag is None:
            out_imag = torch.empty_like(out_real)
        cre = cim = None
        if cells:
            cre = torch.empty((c, self.get_cell_length()), dtype=torch.float32, device=x.device)
            cim = torch.empty_like(cre)
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        fn = self._lib.fstObj_fstBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_longlong, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), c, x.stride(0), self.min_index, self.max_index, out_real.data_ptr(),
                      out_imag.data_ptr(), cre.data_ptr() if cells else None, cim.data_ptr() if cells else None,
                      s.cuda_stream), "fstObj_fstBatchDevice")
        return (out_real, out_imag, cre, cim) if cells else (out_real, out_imag)

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.fstObj_free
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)
