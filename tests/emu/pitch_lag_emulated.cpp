// the DEVICE code of audioflux_amd/csrc/hip/afx_pitch_lag.hip (k_pitch_lag<7 ... 13, NCF / CEP>) compiled for the host
// against tests/emu/hip/hip_runtime.h; exports afxk_pitch_lag.  Everything else of the device layer is the generated stand-in.
#include "hip/hip_runtime.h"

namespace {
alignas(16) unsigned char smem_raw[160 * 1024];
}
#include "../../audioflux_amd/csrc/hip/afx_pitch_lag.hip"
