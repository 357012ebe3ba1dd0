"""PitchShift -- ctypes mirror of the reference wrapper class (python/audioflux/mir/pitch_shift.py) over
libaudioflux_mi355x.so: same constructor arguments and defaults, `pitch_shift` (leading axes are clips, one call each as in
the reference).  Extra: `pitch_shift_batch_device` on torch tensors and
`set_scratch_limit`."""
import ctypes
from ctypes import POINTER, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util
from .types import WindowType


class PitchShift:
    """A time stretch by 2^(-n_semitone / 12) and the Fast resampler back to the input's length
    (include/mir/pitchShift_algorithm.h)."""

    def __init__(self, radix2_exp=12, slide_length=1024, window_type=WindowType.HANN):
        self.radix2_exp, self.slide_length, self.window_type = radix2_exp, slide_length, window_type
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        fn = self._lib.pitchShiftObj_new
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), POINTER(c_int), POINTER(c_int), POINTER(c_int)]
        st = fn(ctypes.byref(self._obj), _util.opt_int(radix2_exp), _util.opt_int(slide_length), _util.opt_int(int(window_type)))
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"pitchShiftObj_new failed with status {st}: {_lib.last_error()}")

    def set_scratch_limit(self, nbytes):
        """device scratch the batched call may hold.  The limit applies twice: to the owned time-stretch object and to this
        object's own rows (stretched and resampled clips), so up to 2 x nbytes in all; 0: the default of 4 GiB each, 8 GiB in all"""
        fn = self._lib.pitchShiftObj_setScratchLimit
        fn.restype, fn.argtypes = None, [c_void_p, c_longlong]
        fn(self._obj, int(nbytes))

    @staticmethod
    def _check(n_semitone):
        if n_semitone < -12 or n_semitone > 12:
            raise ValueError(f"n_semitone={n_semitone} must be in range [-12, 12]")

    def pitch_shift(self, data_arr, n_semitone, samplate=32000):
        """data_arr (..., n) -> (..., n) float32; a sample the resampled signal does not reach stays 0, as in the
        reference's wrapper.  samplate has no effect on the result."""
        self._check(n_semitone)
        x = _util.as_f32(data_arr)
        if x.ndim < 1 or x.shape[-1] < 1:
            raise ValueError("data_arr must have at least one sample")
        n = x.shape[-1]
        clips, lead = _util.flatten_leading(x, 1)
        clips = np.ascontiguousarray(clips)
        out = np.zeros((clips.shape[0], n), np.float32)
        fn = _lib.checked(self._lib.pitchShiftObj_pitchShift)
        fn.restype = None
        fn.argtypes = [c_void_p, c_int, c_int, _util.c_float_p, c_int, _util.c_float_p]
        for c in range(clips.shape[0]):
            fn(self._obj, int(samplate), int(n_semitone), _util.fptr(clips[c]), n, _util.fptr(out[c]))
        return out[0] if x.ndim == 1 else _util.restore_leading(out, lead)

    # -- additive: device-resident batches ----------------------------------
    def pitch_shift_batch_device(self, x, n_semitone, out=None, stream=None):
        """x: CUDA/HIP torch.float32 (clips, n), rows contiguous -> torch (clips, m), m = min(n, resampled length): every clip
        shifted on its own, bit for bit what `pitch_shift` writes.  `out`: a tensor to write into, (clips, >= n) with
        contiguous rows; its first m columns are returned.  Asynchronous on `stream` or torch's current stream; only a
        call whose rate differs from the previous call's waits for the resampler table's readers and uploads the table."""
        import torch
        self._check(n_semitone)
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        b, n = x.shape
        if out is None:
            out = torch.empty((b, n), dtype=torch.float32, device=x.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == b and out.shape[1] >= n
        assert out.stride(1) == 1 or out.shape[1] <= 1
        m = 0
        if b:
            fn = self._lib.pitchShiftObj_pitchShiftBatchDevice
            fn.restype = c_int
            fn.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_longlong, c_void_p, c_longlong, c_void_p]
            m = fn(self._obj, int(n_semitone), x.data_ptr(), b, n, x.stride(0) if b > 1 else n, out.data_ptr(),
                   out.stride(0) if b > 1 else n, s.cuda_stream)
            if m <= 0:
                raise RuntimeError(f"pitchShiftObj_pitchShiftBatchDevice failed with status {m}: {_lib.last_error()}")
        return out[:, :m]

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.pitchShiftObj__free
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)
