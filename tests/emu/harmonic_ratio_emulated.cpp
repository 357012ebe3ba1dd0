// the DEVICE code of audioflux_amd/csrc/hip/afx_harmonic_ratio.hip (k_harmonic_ratio<7 ... 13, first run / listed
// frames>, k_harmonic_ratio_resolve) compiled for the host against tests/emu/hip/hip_runtime.h; exports afxk_harmonic_ratio.
// Everything else of the device layer is the generated stand-in.
#include "hip/hip_runtime.h"

// the one atomic of the resolve kernel: workgroups run one after the other here, the lanes of a wave as threads
static inline int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

namespace {
alignas(16) unsigned char smem_raw[160 * 1024];
}
#include "../../audioflux_amd/csrc/hip/afx_harmonic_ratio.hip"
