"""Spectral -- ctypes mirror of python/audioflux/feature/spectral.py over libaudioflux_mi355x.so: the spectral descriptors
of a (..., fre, time) magnitude / power spectrogram.  Same method names, defaults and orientation as the reference wrapper;
unlike it, a failure raises and the time length is set from the input.  compute_device is additive: any list of
descriptors of rows that already live on the device, in one pass, without host copies."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_longlong, c_void_p

import numpy as np

from . import _lib, _util
from .types import SpectralNoveltyDataType, SpectralNoveltyMethodType

KINDS = ("flatness", "flux", "rolloff", "centroid", "spread", "skewness", "kurtosis", "entropy", "crest", "slope", "decrease",
         "bandwidth", "rms", "energy", "hfc", "sd", "sf", "mkl", "pd", "wpd", "nwpd", "cd", "rcd", "broadband", "novelty",
         "eef", "eer", "max", "mean", "var")
_TWO = ("max", "mean", "var")
_PHASE = ("pd", "wpd", "nwpd", "cd", "rcd")


class SpectralRequest(ctypes.Structure):
    """AfxSpectralRequest (include/afx_batch.h)"""
    _fields_ = [("kind", c_int), ("iarg", c_int * 4), ("farg", c_float * 2)]


def request(kind, iarg=(), farg=()):
    """kind: a name of KINDS or its number; iarg / farg: the descriptor's parameters in the order of its C prototype"""
    r = SpectralRequest()
    r.kind = KINDS.index(kind) if isinstance(kind, str) else int(kind)
    for k, v in enumerate(iarg):
        r.iarg[k] = int(v)
    for k, v in enumerate(farg):
        r.farg[k] = float(v)
    return r


def calloc_index_arr(lib_c, index_arr):
    """setEdgeArr takes ownership of a calloc'ed array (and frees it): allocate it with the C library's calloc"""
    lib_c.calloc.restype = c_void_p
    lib_c.calloc.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    p = ctypes.cast(lib_c.calloc(max(len(index_arr), 1), 4), POINTER(c_int))
    for k, v in enumerate(index_arr):
        p[k] = int(v)
    return p


class DescriptorMixin:
    """the descriptor methods over `self._obj` / `self._lib`, C functions `<self._prefix>_<name>` (spectralObj /
    spectrogramObj share prototypes behind the object pointer)"""
    _prefix = "spectralObj"

    def _before(self, time_length):
        pass

    def _run(self, name, m_data_arr, c_types, c_args, m_phase_arr=None, two=False):
        m = np.asarray(m_data_arr)
        if np.iscomplexobj(m):
            m = np.abs(m)
        m = _util.as_f32(np.swapaxes(m, -1, -2))  # (..., time, fre)
        if m.shape[-1] != self.num:
            raise ValueError(f"m_data_arr must have {self.num} rows of frequencies, not {m.shape[-1]}")
        frames, lead = _util.flatten_leading(m, 2)
        phases = None
        if m_phase_arr is not None:
            ph = _util.as_f32(np.swapaxes(np.asarray(m_phase_arr), -1, -2))
            if ph.shape != m.shape:
                raise ValueError("m_phase_arr must have the shape of m_spec_arr")
            phases, _ = _util.flatten_leading(ph, 2)
        t = m.shape[-2]
        outs = [np.zeros((frames.shape[0], t), np.float32) for _ in range(2 if two else 1)]
        fn = getattr(self._lib, f"{self._prefix}_{name}")
        fn = _lib.checked(fn)
        fn.restype = None
        n_in = 2 if phases is not None else 1
        fn.argtypes = [c_void_p] + [_util.c_float_p] * n_in + list(c_types) + [_util.c_float_p] * len(outs)
        self._before(t)
        for i in range(frames.shape[0]):
            ins = [_util.fptr(frames[i])] + ([_util.fptr(phases[i])] if phases is not None else [])
            fn(self._obj, *ins, *c_args, *[_util.fptr(o[i]) for o in outs])
        outs = [_util.restore_leading(o, lead) for o in outs]
        return tuple(outs) if two else outs[0]

    def set_edge(self, start, end):
        if not 0 <= start < end <= self.num - 1:
            raise ValueError(f"start={start} and end={end} must be in range [0, {self.num - 1}] and start < end")
        fn = getattr(self._lib, f"{self._prefix}_setEdge")
        fn.argtypes = [c_void_p, c_int, c_int]
        fn = _lib.checked(fn)
        fn.restype = None
        fn(self._obj, int(start), int(end))

    def set_edge_arr(self, index_arr):
        idx = [int(v) for v in np.asarray(index_arr).ravel()]
        if not idx or min(idx) < 0 or max(idx) > self.num - 1:
            raise ValueError(f"index_arr must be a non-empty list of indices in range [0, {self.num - 1}]")
        fn = getattr(self._lib, f"{self._prefix}_setEdgeArr")
        fn.argtypes = [c_void_p, POINTER(c_int), c_int]
        fn = _lib.checked(fn)
        fn.restype = None
        fn(self._obj, calloc_index_arr(ctypes.CDLL(None), idx), len(idx))

    def flatness(self, m_data_arr):
        return self._run("flatness", m_data_arr, [], [])

    def flux(self, m_data_arr, step=1, p=2, is_positive=False, is_exp=False, tp=0):
        return self._run("flux", m_data_arr, [c_int, c_float, c_int, POINTER(c_int), POINTER(c_int)],
                         [int(step), float(p), int(is_positive), _util.opt_int(int(is_exp)), _util.opt_int(int(tp))])

    def rolloff(self, m_data_arr, threshold=0.95):
        return self._run("rolloff", m_data_arr, [c_float], [float(threshold)])

    def centroid(self, m_data_arr):
        return self._run("centroid", m_data_arr, [], [])

    def spread(self, m_data_arr):
        return self._run("spread", m_data_arr, [], [])

    def skewness(self, m_data_arr):
        return self._run("skewness", m_data_arr, [], [])

    def kurtosis(self, m_data_arr):
        return self._run("kurtosis", m_data_arr, [], [])

    def entropy(self, m_data_arr, is_norm=False):
        return self._run("entropy", m_data_arr, [c_int], [int(is_norm)])

    def crest(self, m_data_arr):
        return self._run("crest", m_data_arr, [], [])

    def slope(self, m_data_arr):
        return self._run("slope", m_data_arr, [], [])

    def decrease(self, m_data_arr):
        return self._run("decrease", m_data_arr, [], [])

    def band_width(self, m_data_arr, p=2):
        return self._run("bandWidth", m_data_arr, [c_float], [float(p)])

    def rms(self, m_data_arr):
        return self._run("rms", m_data_arr, [], [])

    def energy(self, m_data_arr, is_log=False, gamma=10.):
        return self._run("energy", m_data_arr, [c_int, c_float], [int(is_log), float(gamma)])

    def hfc(self, m_data_arr):
        return self._run("hfc", m_data_arr, [], [])

    def sd(self, m_data_arr, step=1, is_positive=False):
        return self._run("sd", m_data_arr, [c_int, c_int], [int(step), int(is_positive)])

    def sf(self, m_data_arr, step=1, is_positive=False):
        return self._run("sf", m_data_arr, [c_int, c_int], [int(step), int(is_positive)])

    def mkl(self, m_data_arr, tp=0):
        return self._run("mkl", m_data_arr, [c_int], [int(tp)])

    def pd(self, m_data_arr, m_phase_arr):
        return self._run("pd", m_data_arr, [], [], m_phase_arr)

    def wpd(self, m_data_arr, m_phase_arr):
        return self._run("wpd", m_data_arr, [], [], m_phase_arr)

    def nwpd(self, m_data_arr, m_phase_arr):
        return self._run("nwpd", m_data_arr, [], [], m_phase_arr)

    def cd(self, m_data_arr, m_phase_arr):
        return self._run("cd", m_data_arr, [], [], m_phase_arr)

    def rcd(self, m_data_arr, m_phase_arr):
        return self._run("rcd", m_data_arr, [], [], m_phase_arr)

    def broadband(self, m_data_arr, threshold=0):
        return self._run("broadband", m_data_arr, [c_float], [float(threshold)])

    def novelty(self, m_data_arr, step=1, threshold=0., method_type=SpectralNoveltyMethodType.SUB,
                data_type=SpectralNoveltyDataType.VALUE):
        return self._run("novelty", m_data_arr, [c_int, c_float, POINTER(c_int), POINTER(c_int)],
                         [int(step), float(threshold), _util.opt_int(int(method_type)), _util.opt_int(int(data_type))])

    def eef(self, m_data_arr, is_norm=False):
        return self._run("eef", m_data_arr, [c_int], [int(is_norm)])

    def eer(self, m_data_arr, is_norm=False, gamma=1.):
        return self._run("eer", m_data_arr, [c_int, c_float], [int(is_norm), float(gamma)])

    def max(self, m_data_arr):
        return self._run("max", m_data_arr, [], [], two=True)

    def mean(self, m_data_arr):
        return self._run("mean", m_data_arr, [], [], two=True)

    def var(self, m_data_arr):
        return self._run("var", m_data_arr, [], [], two=True)


class Spectral(DescriptorMixin):
    def __init__(self, num, fre_band_arr):
        self._lib = _lib.get_lib()
        self._obj = c_void_p(None)
        fre = _util.as_f32(fre_band_arr).ravel()
        if num < 2 or fre.size != num:
            raise ValueError(f"num={num} must be >= 2 and the length of fre_band_arr ({fre.size})")
        self.num = int(num)
        self.fre_band_arr = fre
        self.time_length = 0
        fn = self._lib.spectralObj_new
        fn.restype = c_int
        fn.argtypes = [POINTER(c_void_p), c_int, _util.c_float_p]
        st = fn(ctypes.byref(self._obj), self.num, _util.fptr(fre))
        if st != 0 or not self._obj:
            self._obj = c_void_p(None)
            raise RuntimeError(f"spectralObj_new failed with status {st}: {_lib.last_error()}")

    def set_time_length(self, time_length):
        fn = self._lib.spectralObj_setTimeLength
        fn.argtypes = [c_void_p, c_int]
        fn = _lib.checked(fn)
        fn.restype = None
        fn(self._obj, int(time_length))
        self.time_length = int(time_length)

    def _before(self, time_length):
        self.set_time_length(time_length)

    def compute_device(self, spec, requests, phase=None, frames_per_clip=0, out=None, stream=None):
        """Additive: spec (and phase) are CUDA/HIP torch.float32 tensors (..., num) of frames, requests a list of
        request(...) entries; returns a [slots, rows] tensor on the device (max / mean / var take two slots)."""
        import torch
        assert spec.is_cuda and spec.dtype == torch.float32 and spec.is_contiguous() and spec.shape[-1] == self.num
        if phase is not None:
            assert phase.is_cuda and phase.dtype == torch.float32 and phase.is_contiguous() and phase.shape == spec.shape
        rows = spec.numel() // self.num
        arr = (SpectralRequest * len(requests))(*requests)
        fn_slots = self._lib.afx_spectralSlots
        fn_slots.restype = c_int
        fn_slots.argtypes = [POINTER(SpectralRequest), c_int]
        slots = fn_slots(arr, len(requests))
        if slots < 0:
            raise ValueError("requests must be a non-empty list of known descriptor kinds")
        if out is None:
            out = torch.empty((slots, rows), dtype=torch.float32, device=spec.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (slots, rows)
        s = stream if stream is not None else torch.cuda.current_stream(spec.device)
        fn = self._lib.spectralObj_computeDevice
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_void_p, c_longlong, c_int, POINTER(SpectralRequest), c_int, c_void_p, c_longlong,
                       c_void_p]
        _lib.check(fn(self._obj, spec.data_ptr(), phase.data_ptr() if phase is not None else None, rows, int(frames_per_clip),
                      arr, len(requests), out.data_ptr(), rows, s.cuda_stream), "spectralObj_computeDevice")
        return out

    def __del__(self):
        if getattr(self, "_obj", None):
            fn = self._lib.spectralObj_free
            fn.argtypes = [c_void_p]
            fn.restype = None
            fn(self._obj)
            self._obj = c_void_p(None)
