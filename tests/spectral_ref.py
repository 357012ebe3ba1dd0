"""ctypes prototypes of the reference's SpectralObj (src/feature/spectral_algorithm.h) in the compiled reference library
(oracle.ref.lib()), and one call per descriptor in the request form of tests/spectral_cases.py.  Used by the fixture
generator and by the GPU tests that compare fresh inputs against the reference."""
import ctypes as C

import numpy as np

from tests.spectral_cases import KINDS, TWO_SLOT, PHASE_KINDS

fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int)

# name -> C argument types between the data pointer(s) and the output pointer(s)
EXTRA = {"flux": [C.c_int, C.c_float, C.c_int, ip, ip], "rolloff": [C.c_float], "entropy": [C.c_int], "bandWidth": [C.c_float],
         "energy": [C.c_int, C.c_float], "sd": [C.c_int, C.c_int], "sf": [C.c_int, C.c_int], "mkl": [C.c_int],
         "broadband": [C.c_float], "novelty": [C.c_int, C.c_float, ip, ip], "eef": [C.c_int], "eer": [C.c_int, C.c_float]}


def c_name(kind):
    return "bandWidth" if kind == "bandwidth" else kind


def bind(lib, prefix="spectralObj"):
    """sets argtypes / restype of every descriptor function `prefix`_<name> of `lib`"""
    for kind in KINDS:
        fn = getattr(lib, f"{prefix}_{c_name(kind)}")
        fn.restype = None
        n_in = 2 if kind in PHASE_KINDS else 1
        n_out = 2 if kind in TWO_SLOT else 1
        fn.argtypes = [C.c_void_p] + [fp] * n_in + EXTRA.get(c_name(kind), []) + [fp] * n_out
    if prefix == "spectralObj":
        lib.spectralObj_new.restype = C.c_int
        lib.spectralObj_new.argtypes = [C.POINTER(C.c_void_p), C.c_int, fp]
        lib.spectralObj_setTimeLength.restype = None
        lib.spectralObj_setTimeLength.argtypes = [C.c_void_p, C.c_int]
        lib.spectralObj_free.restype = None
        lib.spectralObj_free.argtypes = [C.c_void_p]
    getattr(lib, f"{prefix}_setEdge").restype = None
    getattr(lib, f"{prefix}_setEdge").argtypes = [C.c_void_p, C.c_int, C.c_int]
    getattr(lib, f"{prefix}_setEdgeArr").restype = None
    getattr(lib, f"{prefix}_setEdgeArr").argtypes = [C.c_void_p, ip, C.c_int]


def call_args(kind, iarg, farg):
    """the C arguments of a request, in the order of the prototype; returns (args, keep-alive list)"""
    i, f = list(iarg) + [0] * 4, list(farg) + [0.0] * 2
    keep = []

    def ref(v):
        keep.append(C.c_int(int(v)))
        return C.byref(keep[-1])
    if kind == "flux":
        return [i[0], C.c_float(f[0]), i[1], ref(i[2]), ref(i[3])], keep
    if kind in ("rolloff", "bandwidth", "broadband"):
        return [C.c_float(f[0])], keep
    if kind in ("entropy", "eef", "mkl"):
        return [i[0]], keep
    if kind in ("energy", "eer"):
        return [i[0], C.c_float(f[0])], keep
    if kind in ("sd", "sf"):
        return [i[0], i[1]], keep
    if kind == "novelty":
        return [i[0], C.c_float(f[0]), ref(i[1]), ref(i[2])], keep
    return [], keep


def calloc_ints(values):
    """an int array from the C library's calloc: setEdgeArr takes ownership and frees it"""
    libc = C.CDLL(None)
    libc.calloc.restype = C.c_void_p
    libc.calloc.argtypes = [C.c_size_t, C.c_size_t]
    p = C.cast(libc.calloc(len(values), 4), ip)
    for k, v in enumerate(values):
        p[k] = int(v)
    return p


class RefSpectral:
    """the reference object over one input; a fresh object per call keeps its caches out of the way"""

    def __init__(self, lib, num, fre, edge):
        self.lib, self.num, self.edge = lib, num, edge
        self.fre = np.ascontiguousarray(fre, np.float32)
        bind(lib)

    def run(self, kind, iarg, farg, spec, phase=None):
        lib = self.lib
        spec = np.ascontiguousarray(spec, np.float32)
        T = spec.shape[0]
        obj = C.c_void_p()
        assert lib.spectralObj_new(C.byref(obj), self.num, self.fre.ctypes.data_as(fp)) == 0
        lib.spectralObj_setTimeLength(obj, T)
        if isinstance(self.edge, tuple):
            lib.spectralObj_setEdge(obj, *self.edge)
        elif self.edge is not None:
            lib.spectralObj_setEdgeArr(obj, calloc_ints(self.edge), len(self.edge))
        outs = [np.zeros(T, np.float32) for _ in range(2 if kind in TWO_SLOT else 1)]
        ins = [spec.ctypes.data_as(fp)]
        if kind in PHASE_KINDS:
            phase = np.ascontiguousarray(phase, np.float32)
            ins.append(phase.ctypes.data_as(fp))
        args, keep = call_args(kind, iarg, farg)
        getattr(lib, f"spectralObj_{c_name(kind)}")(obj, *ins, *args, *[o.ctypes.data_as(fp) for o in outs])
        lib.spectralObj_free(obj)
        return outs
