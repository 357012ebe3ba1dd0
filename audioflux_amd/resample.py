"""Resample, WindowResample -- ctypes mirrors of the reference wrapper classes (python/audioflux/dsp/resample.py:31-213) over
libaudioflux_mi355x.so: same constructor arguments and defaults, `set_samplate`, `cal_data_length`, `resample`.  All leading
axes of the input go through ONE batched call where the reference loops over channels.  Extra: `set_samplate_ratio`, and
`resample_batch_device` on torch tensors."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util
from .types import ResampleQualityType, WindowType

_QUALITY = {pre + name: q for name, q in (("best", ResampleQualityType.BEST), ("mid", ResampleQualityType.MID),
                                          ("fast", ResampleQualityType.FAST)) for pre in ("", "af_", "audio_")}


def _quality(tp):
    """python/audioflux/dsp/resample.py:14-28: the enum, or 'best' / 'af_best' / 'audio_best' and so on"""
    if isinstance(tp, ResampleQualityType):
        return tp
    if isinstance(tp, str) and tp in _QUALITY:
        return _QUALITY[tp]
    raise ValueError(f"ResampleQualityType[{tp}] not supported")


class _ResampleBase:
    """What the two classes share; a subclass supplies its constructor call."""

    def _new(self, name, argtypes, *args):
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        fn = getattr(self._lib, name)
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), *argtypes]
        st = fn(ctypes.byref(self._obj), *args)
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"{name} failed with status {st}: {_lib.last_error()}")
        self.source_rate = None
        self.target_rate = None
        self._lib.resampleObj_calDataLength.restype = c_int
        self._lib.resampleObj_calDataLength.argtypes = [c_void_p, c_int]

    def set_samplate(self, source_rate, target_rate):
        """equal or non-positive rates are ignored, as in the reference"""
        fn = _lib.checked(self._lib.resampleObj_setSamplate)
        fn.restype = None
        fn.argtypes = [c_void_p, c_int, c_int]
        fn(self._obj, int(source_rate), int(target_rate))
        self.source_rate = source_rate
        self.target_rate = target_rate

    def set_samplate_ratio(self, ratio):
        """target rate / source rate directly; negative values are ignored"""
        fn = _lib.checked(self._lib.resampleObj_setSamplateRatio)
        fn.restype = None
        fn.argtypes = [c_void_p, c_float]
        fn(self._obj, c_float(ratio))

    def cal_data_length(self, data_length):
        """samples `resample` returns for data_length samples: floorf(data_length * ratio) in float32"""
        return int(self._lib.resampleObj_calDataLength(self._obj, int(data_length)))

    def resample(self, data_arr):
        """data_arr (..., n) -> (..., cal_data_length(n)) float32"""
        x = _util.as_f32(data_arr)
        if x.ndim < 1 or x.shape[-1] < 1:
            raise ValueError("data_arr must have at least one sample")
        n = x.shape[-1]
        if x.ndim == 1:
            out = np.zeros(self.cal_data_length(n), np.float32)
            fn = self._lib.resampleObj_resample
            fn.restype = c_int
            fn.argtypes = [c_void_p, _util.c_float_p, c_int, _util.c_float_p]
            st = fn(self._obj, _util.fptr(x), n, _util.fptr(out))
            if st < 0:
                raise RuntimeError(f"resampleObj_resample failed with status {st}: {_lib.last_error()}")
            return out[:st]
        import torch
        clips, lead = _util.flatten_leading(x, 1)
        out = self.resample_batch_device(torch.from_numpy(np.ascontiguousarray(clips)).to("cuda"))
        torch.cuda.current_stream().synchronize()
        return _util.restore_leading(out.cpu().numpy(), lead)

    # -- additive: device-resident batches ----------------------------------
    def resample_batch_device(self, x, out=None, stream=None):
        """x: CUDA/HIP torch.float32 (clips, n), rows contiguous -> torch (clips, cal_data_length(n)): every clip resampled on
        its own, bit for bit what `resample` gives for it.  `out`: a tensor to write into, (clips, >= that length) with
        contiguous rows; its first columns are returned.  One launch, asynchronous on `stream` or torch's current stream."""
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        b, n = x.shape
        m = self.cal_data_length(n)
        if out is None:
            out = torch.empty((b, m), dtype=torch.float32, device=x.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == b and out.shape[1] >= m
        assert out.stride(1) == 1 or out.shape[1] <= 1
        if b and m:
            fn = self._lib.resampleObj_resampleBatchDevice
            fn.restype = c_int
            fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong, c_void_p, c_longlong, c_void_p]
            st = fn(self._obj, x.data_ptr(), b, n, x.stride(0) if b > 1 else n, out.data_ptr(), out.stride(0) if b > 1 else m,
                    s.cuda_stream)
            if st != m:
                raise RuntimeError(f"resampleObj_resampleBatchDevice failed with status {st}: {_lib.last_error()}")
        return out[:, :m]

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.resampleObj_free
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)


class Resample(_ResampleBase):
    """Mirrors the reference wrapper class (python/audioflux/dsp/resample.py:118-157): one of three Kaiser-windowed sinc
    tables (BEST / MID / FAST: 64 / 32 / 16 zero crossings).  The object starts at 32000 -> 16000."""

    def __init__(self, qual_type=ResampleQualityType.BEST, is_scale=False):
        self.qual_type = _quality(qual_type)
        self.is_scale = is_scale
        self.is_continue = False
        self._new("resampleObj_new", [POINTER(c_int), POINTER(c_int), POINTER(c_int)], _util.opt_int(self.qual_type.value),
                  _util.opt_int(bool(is_scale)), _util.opt_int(0))


class WindowResample(_ResampleBase):
    """Mirrors the reference wrapper class (python/audioflux/dsp/resample.py:160-213): a sinc table of zero_num zero crossings
    with 2^nbit entries each under any WindowType; `value` is the Kaiser beta, the Gauss alpha or the Tukey alpha."""

    def __init__(self, zero_num=64, nbit=9, win_type=WindowType.HANN, value=None, roll_off=0.945, is_scale=False):
        self.zero_num, self.nbit, self.win_type = zero_num, nbit, win_type
        self.value, self.roll_off, self.is_scale = value, roll_off, is_scale
        self.is_continue = False
        self._new("resampleObj_newWithWindow",
                  [POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_int), POINTER(c_int)],
                  _util.opt_int(zero_num), _util.opt_int(nbit), _util.opt_int(int(win_type)), _util.opt_float(value),
                  _util.opt_float(roll_off), _util.opt_int(bool(is_scale)), _util.opt_int(0))
