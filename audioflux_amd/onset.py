"""Onset, NoveltyParam, power_to_db -- ctypes mirrors of the reference wrapper (python/audioflux/mir/onset.py:14-221,
python/audioflux/utils/convert.py:26-72) over libaudioflux_mi355x.so: same constructor arguments and defaults, `onset` ->
(point_arr, evn_arr, time_arr, value_arr).  All leading axes of the input go through ONE batched call where the reference
loops over channels.  Extra: device-resident calls on torch tensors (`Onset.onset_device`, `power_to_db_device`,
`max_filter_device`, `peak_pick_device`)."""
import ctypes
from ctypes import POINTER, Structure, c_float, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util
from .types import NoveltyType


class NoveltyParam(Structure):
    """the parameters of the novelty function, positional as in the reference: step, p, isPostive, isExp, type, threshold,
    isNorm, gamma (include/mir/onset_algorithm.h; isNorm and gamma are unused)"""
    _fields_ = [("step", c_int), ("p", c_float), ("isPostive", c_int), ("isExp", c_int), ("type", c_int),
                ("threshold", c_float), ("isNorm", c_int), ("gamma", c_float)]


def _default_param():  # python/audioflux/mir/onset.py:157-158 (not the C default: type 1, the mean)
    return NoveltyParam(1, 1.0, 1, 0, 1, 0.0, 1, 1.0)


def _index(index_arr):
    if index_arr is None:
        return None, None, 0
    idx = np.ascontiguousarray(np.asarray(index_arr).astype(np.int32))
    return idx, idx.ctypes.data_as(_util.c_int_p), len(idx)


class Onset:
    def __init__(self, time_length, fre_length, slide_length, samplate=32000, filter_order=1, novelty_type=NoveltyType.FLUX):
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        self.time_length, self.fre_length = int(time_length), int(fre_length)
        self.samplate, self.slide_length = samplate, slide_length
        self.filter_order, self.novelty_type = filter_order, novelty_type
        fn = self._lib.onsetObj_new
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int)]
        st = fn(ctypes.byref(self._obj), self.time_length, self.fre_length, int(slide_length), _util.opt_int(samplate),
                _util.opt_int(filter_order), _util.opt_int(int(getattr(novelty_type, "value", novelty_type))))
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"onsetObj_new failed with status {st}: {_lib.last_error()}")

    def onset(self, m_data_arr1, m_data_arr2=None, novelty_param=None, index_arr=None):
        """m_data_arr1 (..., fre, time) (and m_data_arr2, the phase, for PD / WPD / NWPD / CD / RCD) -> point_arr (..., points)
        int32, evn_arr (..., time) float32, time_arr = point_arr * slide_length / samplate, value_arr = evn_arr at the points.
        With leading axes the point axis is as long as the longest channel's list; shorter lists end in zeros."""
        a = np.ascontiguousarray(np.swapaxes(np.asarray(m_data_arr1, dtype=np.float32), -1, -2))
        b = None
        if m_data_arr2 is not None:
            b = np.ascontiguousarray(np.swapaxes(np.asarray(m_data_arr2, dtype=np.float32), -1, -2))
            if a.shape != b.shape:
                raise ValueError("m_data_arr1 and m_data_arr2 must be the same shape")
        if a.ndim < 2 or a.shape[-2:] != (self.time_length, self.fre_length):
            raise ValueError(f"m_data_arr1 must be (..., {self.fre_length}, {self.time_length})")
        if novelty_param is None:
            novelty_param = _default_param()
        elif not isinstance(novelty_param, NoveltyParam):
            raise ValueError("novelty_param must be type of NoveltyParam")
        n = self.time_length
        if a.ndim == 2:
            idx, idx_p, idx_n = _index(index_arr)
            evn, point = np.zeros(n, np.float32), np.zeros(n, np.int32)
            fn = self._lib.onsetObj_onset
            fn.restype = c_int
            fn.argtypes = [c_void_p, _util.c_float_p, _util.c_float_p, POINTER(NoveltyParam), _util.c_int_p, c_int,
                           _util.c_float_p, _util.c_int_p]
            count = fn(self._obj, _util.fptr(a), None if b is None else _util.fptr(b), ctypes.byref(novelty_param), idx_p, idx_n,
                       _util.fptr(evn), point.ctypes.data_as(_util.c_int_p))
            if count < 0:
                raise RuntimeError(f"onsetObj_onset failed with status {count}: {_lib.last_error()}")
            point = point[:count]
            value = evn[point]
        else:
            import torch
            clips, lead = _util.flatten_leading(a, 2)
            ph = None if b is None else torch.from_numpy(_util.flatten_leading(b, 2)[0]).to("cuda")
            evn, point, count = self.onset_device(torch.from_numpy(clips).to("cuda"), ph, novelty_param, index_arr)
            torch.cuda.current_stream().synchronize()
            evn, point, count = evn.cpu().numpy(), point.cpu().numpy(), count.cpu().numpy()
            longest = int(count.max()) if len(count) else 0
            point = point[:, :longest]
            value = np.zeros(point.shape, np.float32)
            for c in range(len(count)):
                value[c, :count[c]] = evn[c, point[c, :count[c]]]
            evn, point, value = (_util.restore_leading(v, lead) for v in (evn, point, value))
        time = 1.0 * point * self.slide_length / self.samplate
        return point, evn, time, value

    # -- additive: device-resident batches ----------------------------------
    def onset_device(self, spec, phase=None, novelty_param=None, index_arr=None, max_points=None, stream=None):
        """spec (and phase): CUDA/HIP torch.float32 (clips, time, fre), contiguous -- rows of frames, the layout the
        spectrogram kernels write -> (evn (clips, time) float32, points (clips, max_points) int32, count (clips,) int32).
        count holds ALL points of a clip; points beyond min(count, max_points) are 0.  max_points None: time.  novelty_param
        None: the C default (step 1, p 1, rectified, sum).  Asynchronous on `stream` or torch's current stream."""
        import torch
        for t in (spec,) + (() if phase is None else (phase,)):
            assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous()
            assert tuple(t.shape[1:]) == (self.time_length, self.fre_length), tuple(t.shape)
        assert phase is None or phase.shape == spec.shape
        if novelty_param is not None and not isinstance(novelty_param, NoveltyParam):
            raise ValueError("novelty_param must be type of NoveltyParam")
        b, n = spec.shape[0], self.time_length
        cap = n if max_points is None else int(max_points)
        s = stream if stream is not None else torch.cuda.current_stream(spec.device)
        evn = torch.empty((b, n), dtype=torch.float32, device=spec.device)
        with torch.cuda.stream(s):  # the zero fill is ordered before the kernel that writes the points
            point = torch.zeros((b, cap), dtype=torch.int32, device=spec.device)
        count = torch.empty((b,), dtype=torch.int32, device=spec.device)
        if b == 0:
            return evn, point, count
        idx, idx_p, idx_n = _index(index_arr)
        fn = self._lib.onsetObj_onsetBatchDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_void_p, c_int, POINTER(NoveltyParam), _util.c_int_p, c_int, c_void_p, c_void_p,
                       c_void_p, c_longlong, c_longlong, c_void_p]
        _lib.check(fn(self._obj, spec.data_ptr(), None if phase is None else phase.data_ptr(), b,
                      None if novelty_param is None else ctypes.byref(novelty_param), idx_p, idx_n, evn.data_ptr(),
                      point.data_ptr() if cap > 0 else None, count.data_ptr(), n, cap, s.cuda_stream), "onsetObj_onsetBatchDevice")
        return evn, point, count

    def debug(self):
        fn = self._lib.onsetObj_debug
        fn.argtypes = [c_void_p]
        fn(self._obj)

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.onsetObj_free
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)


def power_to_db_device(x, min_db=-80.0, out=None, stream=None):
    """x: CUDA/HIP torch.float32 (clips, ...), contiguous -> 10 log10(x / max of the clip) clamped at min_db (>= 0: -80), one
    maximum per entry of the first axis; out may be x itself.  Asynchronous on `stream` or torch's current stream."""
    import torch
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() >= 1 and x.is_contiguous()
    out = torch.empty_like(x) if out is None else out
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous()
    if x.numel() == 0:
        return out
    b, length = x.shape[0], x.numel() // x.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(x.device)
    fn = _lib.get_lib().afx_powerToDbDevice
    fn.restype = c_int
    fn.argtypes = [c_void_p, c_int, c_longlong, c_longlong, c_float, c_void_p, c_void_p]
    _lib.check(fn(x.data_ptr(), b, length, length, float(min_db), out.data_ptr(), s.cuda_stream), "afx_powerToDbDevice")
    return out


def power_to_db(X, min_db=-80):
    """python/audioflux/utils/convert.py:26-72: X (..., fre, time) power -> relative dB, one maximum per (fre, time) plane;
    a resident torch tensor goes to power_to_db_device with its leading axes as the clips"""
    if _util.is_torch(X):
        if X.dim() < 2:
            raise ValueError("The dimension should be greater than equal to 2")
        flat = X.contiguous().reshape((-1, X.shape[-2] * X.shape[-1]))
        return power_to_db_device(flat, min_db).reshape(X.shape)
    x = _util.as_f32(X)
    if x.ndim < 2:
        raise ValueError("The dimension should be greater than equal to 2")
    if x.ndim == 2:
        out = np.zeros(x.shape, np.float32)
        fn = _lib.checked(_lib.get_lib().util_powerToDB)
        fn.restype = None
        fn.argtypes = [_util.c_float_p, c_int, c_float, _util.c_float_p]
        fn(_util.fptr(x), x.size, float(min_db), _util.fptr(out))
        return out
    import torch
    planes, lead = _util.flatten_leading(x, 2)
    out = power_to_db_device(torch.from_numpy(planes.reshape(len(planes), -1)).to("cuda"), min_db)
    torch.cuda.current_stream().synchronize()
    return out.cpu().numpy().reshape(x.shape)


def max_filter_device(x, order, stream=None):
    """x: CUDA/HIP torch.float32 (rows, cols), contiguous -> the running maximum of `order` bins along the columns, the window
    of bin j being j - order // 2 ... j - 1 + order - order // 2 cut at the row's ends.  Exact."""
    import torch
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    s = stream if stream is not None else torch.cuda.current_stream(x.device)
    fn = _lib.get_lib().afx_maxFilterDevice
    fn.restype = c_int
    fn.argtypes = [c_void_p, c_longlong, c_int, c_int, c_void_p, c_void_p]
    _lib.check(fn(x.data_ptr(), x.shape[0], x.shape[1], int(order), out.data_ptr(), s.cuda_stream), "afx_maxFilterDevice")
    return out


def peak_pick_device(evn, pre_max, post_max, pre_avg, post_avg, wait, delta, max_points=None, stream=None):
    """evn: CUDA/HIP torch.float32 (clips, time), rows contiguous -> (points (clips, max_points) int32, count (clips,) int32)
    by the rule of include/afx_batch.h (afx_peakPickDevice); points beyond min(count, max_points) are 0"""
    import torch
    assert evn.is_cuda and evn.dtype == torch.float32 and evn.dim() == 2 and evn.stride(1) == 1
    b, n = evn.shape
    cap = n if max_points is None else int(max_points)
    s = stream if stream is not None else torch.cuda.current_stream(evn.device)
    with torch.cuda.stream(s):
        point = torch.zeros((b, cap), dtype=torch.int32, device=evn.device)
    count = torch.empty((b,), dtype=torch.int32, device=evn.device)
    if b == 0 or n == 0:
        return point, count
    fn = _lib.get_lib().afx_peakPickDevice
    fn.restype = c_int
    fn.argtypes = [c_void_p, c_int, c_int, c_longlong, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_longlong,
                   c_void_p]
    _lib.check(fn(evn.data_ptr(), b, n, evn.stride(0) if b > 1 else n, int(pre_max), int(post_max), int(pre_avg), int(post_avg), int(wait),
                  float(delta), point.data_ptr() if cap > 0 else None, count.data_ptr(), cap, s.cuda_stream), "afx_peakPickDevice")
    return point, count
