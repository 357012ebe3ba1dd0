"""PitchYIN, PitchHPS, PitchLHS, PitchPEF, PitchNCF, PitchCEP -- ctypes mirrors of the reference wrapper classes over libaudioflux_mi355x.so: same
constructor arguments and defaults, `cal_time_length`, `pitch`.  All leading axes of the input go through ONE batched call
where the reference loops over channels.  Extra: device-resident calls on torch tensors.  `_Pitch` holds what every tracker
shares; a new one supplies its constructor and, where its results differ from (fre, value) + curve, its own calls."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util
from .types import WindowType


class _Pitch:
    """What the trackers share.  `_name` selects the exported names pitch<_name>Obj_*."""
    _name = None

    def _fn(self, what):
        return getattr(self._lib, f"pitch{self._name}Obj_{what}")

    def _new(self, argtypes, *args):
        """the constructor call: the object, or RuntimeError with the library's message"""
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        fn = self._fn("new")
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), *argtypes]
        st = fn(ctypes.byref(self._obj), *args)
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"pitch{self._name}Obj_new failed with status {st}: {_lib.last_error()}")
        self._fn("calTimeLength").restype = c_int
        self._fn("calTimeLength").argtypes = [c_void_p, c_int]

    def _get(self, what):
        """an int getter of the object"""
        g = self._fn(what)
        g.restype, g.argtypes = c_int, [c_void_p]
        return int(g(self._obj))

    def cal_time_length(self, data_length):
        return int(self._fn("calTimeLength")(self._obj, int(data_length)))

    # -- additive: device-resident batches ----------------------------------
    def _args(self, x, stream):
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        return x.shape[0], x.shape[1], self.cal_time_length(x.shape[1]), s

    def _batch(self, what, x, b, n, outs, tail, s):
        """<what>BatchDevice on the clips x into the tensors `outs`; `tail`: the (ctype, value) arguments between the outputs
        and the stream"""
        fn = self._fn(what)
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_longlong] + [c_void_p] * len(outs) + [t for t, _ in tail] + [c_void_p]
        _lib.check(fn(self._obj, x.data_ptr(), b, n, x.stride(0), *(o.data_ptr() for o in outs), *(v for _, v in tail),
                      s.cuda_stream), f"pitch{self._name}Obj_{what}")

    def _curve(self, x, width, stream):
        import torch
        b, n, t, s = self._args(x, stream)
        out = torch.empty((b, t, width), dtype=torch.float32, device=x.device)
        if t:
            self._batch("curveBatchDevice", x, b, n, [out], [], s)
        return out

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._fn("free")
            fn.argtypes, fn.restype = [c_void_p], None
            fn(self._obj)
            self._obj = c_void_p(None)


class PitchYIN(_Pitch):
    """Mirrors the reference wrapper class (python/audioflux/mir/pitch_yin.py:10-150): `set_thresh`, `pitch` -> (fre_arr,
    value1_arr, value2_arr).  Extra: `pitch_device`, `troughs_device`, `curve_device` on torch tensors."""
    _name = "YIN"

    def __init__(self, samplate=32000, low_fre=27.0, high_fre=2000.0, radix2_exp=12, slide_length=1024, auto_length=2048):
        self.samplate, self.low_fre, self.high_fre = samplate, low_fre, high_fre
        self.radix2_exp, self.slide_length, self.auto_length = radix2_exp, slide_length, auto_length
        self.fft_length = 1 << radix2_exp
        self.is_continue = False
        self._new([POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)],
                  _util.opt_int(samplate), _util.opt_float(low_fre), _util.opt_float(high_fre), _util.opt_int(radix2_exp),
                  _util.opt_int(slide_length), _util.opt_int(auto_length), _util.opt_int(0))
        self.yin_length = self._get("yinLength")
        self.min_index = self._get("minIndex")

    def set_thresh(self, thresh):
        """default 0.1; values <= 0 are ignored, as in the reference"""
        fn = self._lib.pitchYINObj_setThresh
        fn.restype, fn.argtypes = None, [c_void_p, c_float]
        fn(self._obj, c_float(thresh))

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

    def pitch_device(self, x, stream=None):
        """x: CUDA/HIP torch.float32 (clips, n) -> (fre, value1, value2) torch (clips, time).  Every frame is written: fre and
        value1 are 0 where no trough qualifies.  One launch, asynchronous on `stream` or torch's current stream."""
        import torch
        b, n, t, s = self._args(x, stream)
        fre, v1, v2 = (torch.empty((b, t), dtype=torch.float32, device=x.device) for _ in range(3))
        if t:  # (0: fewer samples than a frame)
            self._batch("pitchBatchDevice", x, b, n, [fre, v1, v2], [(c_longlong, t)], s)
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
        if t:
            self._batch("troughsBatchDevice", x, b, n, [fre, val, cnt], [(c_int, int(max_troughs))], s)
        return fre, val, cnt

    def curve_device(self, x, stream=None):
        """x: torch (clips, n) -> the cumulative-mean-normalised difference curve, torch (clips, time, yin_length); column k is
        lag min_index + k"""
        return self._curve(x, self.yin_length, stream)


class _PitchFre(_Pitch):
    """The trackers whose `pitch` returns a frequency per frame from the first maximum of a curve over min_index ...
    max_index (which the constructor sets); the class docstring says which curve and which frequency."""

    def pitch(self, data_arr):
        """data_arr (..., n) -> fre_arr (..., time) float32: the frequency at the first maximum of the tracker's curve over
        min_index ... max_index"""
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

    def pitch_batch_device(self, x, stream=None):
        """x: CUDA/HIP torch.float32 (clips, n) -> (fre, value) torch (clips, time): the frequency and the curve's value at the
        chosen index.  One launch, asynchronous on `stream` or torch's current stream."""
        import torch
        b, n, t, s = self._args(x, stream)
        fre, val = (torch.empty((b, t), dtype=torch.float32, device=x.device) for _ in range(2))
        if t:  # (0: fewer samples than a frame)
            self._batch("pitchBatchDevice", x, b, n, [fre, val], [(c_longlong, t)], s)
        return fre, val

    def curve_batch_device(self, x, stream=None):
        """x: torch (clips, n) -> the tracker's curve, torch (clips, time, max_index + 1); column j is candidate index j (the
        entries below min_index included)"""
        return self._curve(x, self.max_index + 1, stream)


class _PitchHS(_PitchFre):
    """What PitchHPS and PitchLHS share (python/audioflux/mir/pitch_hps.py:14-172, pitch_lhs.py): `pitch` -> fre_arr, (index +
    1) * samplate / interp_length of the first maximum of the harmonic curve; column j of the curve is candidate bin j."""

    def __init__(self, samplate=32000, low_fre=32.0, high_fre=2000.0, radix2_exp=12, slide_length=1024, window_type=WindowType.HAMM,
                 harmonic_count=5):
        if low_fre >= high_fre:
            raise ValueError("`low_fre` must be smaller than `high_fre`")
        if harmonic_count <= 0:
            raise ValueError("`harmonic_count` must be greater than 0.")
        self.samplate, self.low_fre, self.high_fre = samplate, low_fre, high_fre
        self.radix2_exp, self.slide_length, self.window_type = radix2_exp, slide_length, window_type
        self.fft_length = 1 << radix2_exp
        self.is_continue = False
        self._new([POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int),
                   POINTER(c_int)],
                  _util.opt_int(samplate), _util.opt_float(low_fre), _util.opt_float(high_fre), _util.opt_int(radix2_exp),
                  _util.opt_int(slide_length), _util.opt_int(window_type), _util.opt_int(harmonic_count), _util.opt_int(0))
        self.min_index = self._get("minIndex")
        self.max_index = self._get("maxIndex")
        self.harmonic_count = self._get("harmonicCount")  # as the object uses it (mir/_pitch_hps.h)
        self.interp_length = self._get("interpLength")


class PitchHPS(_PitchHS):
    """Harmonic product spectrum (include/mir/_pitch_hps.h): curve[j] = prod_k |X[j (k + 1)]|.  A window type above HAMM falls
    back to HAMM and harmonic_count is used as given, as in the reference."""
    _name = "HPS"


class PitchLHS(_PitchHS):
    """Log-harmonic sum (include/mir/_pitch_lhs.h): curve[j] = sum_k log |X[j (k + 1)]|.  Every window type is taken as given and
    harmonic_count is clamped to samplate // (max_index + 1), as in the reference."""
    _name = "LHS"


class PitchPEF(_PitchFre):
    """Mirrors audioflux.PitchPEF (python/audioflux/mir/pitch_pef.py:14-227; include/mir/_pitch_pef.h): same constructor
    arguments, defaults and ValueErrors, `set_filter_params`, `pitch` -> fre_arr: the log frequency at the first maximum of
    the filter's correlation with the log spectrum; column k of the curve is lag k."""
    _name = "PEF"

    def __init__(self, samplate=32000, low_fre=32.0, high_fre=2000.0, cut_fre=4000.0, radix2_exp=12, slide_length=1024,
                 window_type=WindowType.HAMM, alpha=10.0, beta=0.5, gamma=1.8):
        if low_fre >= high_fre:
            raise ValueError("`low_fre` must be smaller than `high_fre`")
        if high_fre >= cut_fre:
            raise ValueError("`high_fre` must be smaller than `cut_fre`")
        self._check_filter(alpha, beta, gamma)
        self.samplate, self.low_fre, self.high_fre, self.cut_fre = samplate, low_fre, high_fre, cut_fre
        self.radix2_exp, self.slide_length, self.window_type = radix2_exp, slide_length, window_type
        self.alpha, self.beta, self.gamma = alpha, beta, gamma
        self.fft_length = 1 << radix2_exp
        self.is_continue = False
        self._new([POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_int), POINTER(c_int), POINTER(c_int),
                   POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_int)],
                  _util.opt_int(samplate), _util.opt_float(low_fre), _util.opt_float(high_fre), _util.opt_float(cut_fre),
                  _util.opt_int(radix2_exp), _util.opt_int(slide_length), _util.opt_int(window_type), _util.opt_float(alpha),
                  _util.opt_float(beta), _util.opt_float(gamma), _util.opt_int(0))
        self.min_index = self._get("minIndex")
        self.max_index = self._get("maxIndex")
        self.filter_pad_num = self._get("filterPadNum")
        self.log_length = self._get("logLength")

    @staticmethod
    def _check_filter(alpha, beta, gamma):
        if alpha <= 0:
            raise ValueError("`alpha` must be greater than 0.")
        if beta < 0 or beta > 1:
            raise ValueError("`beta` must be between 0 and 1.")
        if gamma <= 1:
            raise ValueError("`gamma` must be greater than 1.")

    def set_filter_params(self, alpha, beta, gamma):
        """As in the reference: the arguments are validated and remembered here; the object's filter stays the
        constructor's (include/mir/_pitch_pef.h, the deviations)"""
        self._check_filter(alpha, beta, gamma)
        fn = _lib.checked(self._lib.pitchPEFObj_setFilterParams)
        fn.restype = None
        fn.argtypes = [c_void_p, c_float, c_float, c_float]
        fn(self._obj, alpha, beta, gamma)
        self.alpha, self.beta, self.gamma = alpha, beta, gamma


class _PitchLag(_PitchFre):
    """What PitchNCF and PitchCEP share (python/audioflux/mir/pitch_ncf.py:10-160, pitch_cep.py): `pitch` -> fre_arr,
    samplate / (index + 1) of the first maximum of the lag-domain curve; column j of the curve is candidate index j."""

    def __init__(self, samplate, low_fre, high_fre, radix2_exp, slide_length, window_type):
        self.samplate, self.low_fre, self.high_fre = samplate, low_fre, high_fre
        self.radix2_exp, self.slide_length, self.window_type = radix2_exp, slide_length, window_type
        self.fft_length = 1 << radix2_exp
        self.is_continue = False
        self._new([POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)],
                  _util.opt_int(samplate), _util.opt_float(low_fre), _util.opt_float(high_fre), _util.opt_int(radix2_exp),
                  _util.opt_int(slide_length), _util.opt_int(window_type), _util.opt_int(0))
        self.min_index = self._get("minIndex")
        self.max_index = self._get("maxIndex")


class PitchNCF(_PitchLag):
    """Normalised autocorrelation (include/mir/_pitch_ncf.h): curve[j] = (2N)^(-1/4) r[j + 1] / sqrt(r[0]) over min_index - 1
    ... max_index - 1, r the inverse transform of the zero-padded frame's power spectrum.  Every window type is taken."""
    _name = "NCF"

    def __init__(self, samplate=32000, low_fre=32.0, high_fre=2000.0, radix2_exp=12, slide_length=1024, window_type=WindowType.RECT):
        super().__init__(samplate, low_fre, high_fre, radix2_exp, slide_length, window_type)


class PitchCEP(_PitchLag):
    """Cepstrum (include/mir/_pitch_cep.h): curve[j] is the real cepstrum of the zero-padded frame at quefrency j.  A window
    type above HAMM falls back to HAMM, as in the reference."""
    _name = "CEP"

    def __init__(self, samplate=32000, low_fre=32.0, high_fre=2000.0, radix2_exp=12, slide_length=1024, window_type=WindowType.HAMM):
        if low_fre >= high_fre:  # (python/audioflux/mir/pitch_cep.py:72; pitch_ncf.py has no such check)
            raise ValueError("`low_fre` must be smaller than `high_fre`")
        super().__init__(samplate, low_fre, high_fre, radix2_exp, slide_length, window_type)
