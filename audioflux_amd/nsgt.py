"""NSGT -- ctypes mirror of python/audioflux/nsgt.py:123-367 over libaudioflux_mi355x.so: the non-stationary Gabor
transform (one FFT of the chunk, per band a window on a spectrum slice and an inverse DFT of the band's own length, then
a sample-and-hold of every band onto the longest band's time grid).  Result (..., num, max_time_length) complex64."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util
from .types import (NSGTFilterBankType, SpectralFilterBankNormalType, SpectralFilterBankScaleType,
                    SpectralFilterBankStyleType)


class NSGT:
    def __init__(self, num=84, radix2_exp=12, samplate=32000, low_fre=None, high_fre=None, bin_per_octave=12, min_len=3,
                 nsgt_filter_bank_type=NSGTFilterBankType.EFFICIENT, scale_type=SpectralFilterBankScaleType.OCTAVE,
                 style_type=SpectralFilterBankStyleType.SLANEY, normal_type=SpectralFilterBankNormalType.BAND_WIDTH):
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        self.fft_length = 1 << radix2_exp
        if num > self.fft_length // 2 + 1:
            raise ValueError(f"num={num} is too large")
        if scale_type == SpectralFilterBankScaleType.OCTAVE and bin_per_octave < 1:
            raise ValueError(f"bin_per_octave={bin_per_octave} must be a positive integer")
        if style_type == SpectralFilterBankStyleType.GAMMATONE:
            raise ValueError(f"style_type={style_type.name} is unsupported")
        if normal_type not in (SpectralFilterBankNormalType.NONE, SpectralFilterBankNormalType.BAND_WIDTH):
            raise ValueError(f"normal_type={normal_type.name} is unsupported")
        octave_like = scale_type in (SpectralFilterBankScaleType.OCTAVE, SpectralFilterBankScaleType.LOG)
        if low_fre is None:
            low_fre = 32.703195662574764 if octave_like else 0.0
        if high_fre is None:
            high_fre = samplate / 2
        if octave_like and low_fre < 32.703:
            raise ValueError(f"{scale_type.name} low_fre={low_fre} must be greater than or equal to 32.703")
        if low_fre < 0:
            raise ValueError(f"{scale_type.name} low_fre={low_fre} must be a non-negative number")
        self.num, self.radix2_exp, self.samplate = num, radix2_exp, samplate
        self.low_fre, self.high_fre, self.bin_per_octave, self.min_len = low_fre, high_fre, bin_per_octave, min_len
        self.nsgt_filter_bank_type, self.scale_type = nsgt_filter_bank_type, scale_type
        self.style_type, self.normal_type = style_type, normal_type
        fn = self._lib.nsgtObj_new
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), c_int, c_int, POINTER(c_int), POINTER(c_float), POINTER(c_float)] + \
                      [POINTER(c_int)] * 6
        st = fn(ctypes.byref(self._obj), num, radix2_exp, _util.opt_int(samplate), _util.opt_float(low_fre),
                _util.opt_float(high_fre), _util.opt_int(bin_per_octave), _util.opt_int(min_len),
                _util.opt_int(int(nsgt_filter_bank_type)), _util.opt_int(int(scale_type)), _util.opt_int(int(style_type)),
                _util.opt_int(int(normal_type)))
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"nsgtObj_new failed with status {st}: {_lib.last_error()}")

    def _int(self, name):
        fn = getattr(self._lib, name)
        fn.argtypes, fn.restype = [c_void_p], c_int
        return fn(self._obj)

    def _arr(self, name, ctype):
        fn = getattr(self._lib, name)
        fn.argtypes, fn.restype = [c_void_p], POINTER(ctype)
        return np.ctypeslib.as_array(fn(self._obj), (self.num,)).copy()

    def get_max_time_length(self):
        return self._int("nsgtObj_getMaxTimeLength")

    def get_total_time_length(self):
        return self._int("nsgtObj_getTotalTimeLength")

    def get_time_length_arr(self):
        return self._arr("nsgtObj_getTimeLengthArr", c_int)

    def get_fre_band_arr(self):
        return self._arr("nsgtObj_getFreBandArr", c_float)

    def get_bin_band_arr(self):
        return self._arr("nsgtObj_getBinBandArr", c_int)

    def set_min_length(self, min_length=3):
        """rebuilds the whole plan, the time map included; a plan the library refuses (a band longer than the chunk)
        raises and leaves the object as it was"""
        if min_length < 1:
            raise ValueError(f"min_length={min_length} cannot be less than 1")
        fn = self._lib.nsgtObj_setMinLength
        fn = _lib.checked(fn)
        fn.restype = None
        fn.argtypes = [c_void_p, c_int]
        fn(self._obj, int(min_length))
        self.min_len = min_length

    def _fit(self, x):
        n = self.fft_length  # truncate / zero-pad like utils/util.py:98-111
        if x.shape[-1] >= n:
            return np.ascontiguousarray(x[..., :n])
        out = np.zeros(x.shape[:-1] + (n,), np.float32)
        out[..., : x.shape[-1]] = x
        return out

    def nsgt(self, data_arr):
        """data_arr (..., 2**radix2_exp) -> complex64 (..., num, max_time_length)"""
        x = self._fit(_util.as_f32(data_arr))
        clips, lead = _util.flatten_leading(x, 1)
        re = np.zeros((clips.shape[0], self.num, self.get_max_time_length()), np.float32)
        im = np.zeros_like(re)
        fn = self._lib.nsgtObj_nsgt
        fn = _lib.checked(fn)
        fn.restype = None
        fn.argtypes = [c_void_p, _util.c_float_p, _util.c_float_p, _util.c_float_p]
        for i in range(clips.shape[0]):
            fn(self._obj, _util.fptr(clips[i]), _util.fptr(re[i]), _util.fptr(im[i]))
        return _util.restore_leading((re + 1j * im).astype(np.complex64), lead)

    def get_cell_data(self):
        """the cells of the last nsgt() chunk: a list of complex64 arrays, one per band, of that band's own length"""
        fn = self._lib.nsgtObj_getCellData
        fn = _lib.checked(fn)
        fn.restype = None
        fn.argtypes = [c_void_p, POINTER(_util.c_float_p), POINTER(_util.c_float_p)]
        re, im = _util.c_float_p(), _util.c_float_p()
        fn(self._obj, ctypes.byref(re), ctypes.byref(im))
        total = self.get_total_time_length()
        flat = (np.ctypeslib.as_array(re, (total,)) + 1j * np.ctypeslib.as_array(im, (total,))).astype(np.complex64)
        return np.split(flat, np.cumsum(self.get_time_length_arr())[:-1])

    def y_coords(self):
        return np.insert(self.get_fre_band_arr(), 0, self.low_fre)

    def x_coords(self, data_length):
        return np.linspace(0, data_length * 1. / self.samplate, self.get_max_time_length() + 1)

    def nsgt_device(self, x, out_real=None, out_imag=None, cells=False, stream=None):
        """Additive (include/nsgt_algorithm.h: nsgtObj_nsgtBatchDevice): x HIP torch.float32 (chunks, 2**radix2_exp) with
        contiguous rows -> (real, imag) torch (chunks, num, max_time_length); with cells=True also the cell planes
        (chunks, total_time_length): (real, imag, cell_real, cell_imag).  Asynchronous on `stream`."""
        import torch
        n = self.fft_length
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == n
        c = x.shape[0]
        if out_real is None:
            out_real = torch.empty((c, self.num, self.get_max_time_length()), dtype=torch.float32, device=x.device)
        if out_imag is None:
            out_imag = torch.empty_like(out_real)
        cre = cim = None
        if cells:
            cre = torch.empty((c, self.get_total_time_length()), dtype=torch.float32, device=x.device)
            cim = torch.empty_like(cre)
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        fn = self._lib.nsgtObj_nsgtBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_longlong, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), c, x.stride(0), out_real.data_ptr(), out_imag.data_ptr(),
                      cre.data_ptr() if cells else None, cim.data_ptr() if cells else None, s.cuda_stream),
                   "nsgtObj_nsgtBatchDevice")
        return (out_real, out_imag, cre, cim) if cells else (out_real, out_imag)

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.nsgtObj_free
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)
