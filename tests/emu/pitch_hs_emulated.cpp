// the DEVICE code of audioflux_amd/csrc/hip/afx_pitch_hs.hip (k_pitch_hs<6 ... 13, product | log-sum>) compiled for the host
// against tests/emu/hip/hip_runtime.h; exports afxk_pitch_hs.  Everything else of the device layer is the generated stand-in.
#include "hip/hip_runtime.h"

namespace {
alignas(16) unsigned char smem_raw[160 * 1024];
}
#include "../../audioflux_amd/csrc/hip/afx_pitch_hs.hip"
