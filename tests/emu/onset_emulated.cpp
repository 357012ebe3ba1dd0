// the DEVICE code of audioflux_amd/csrc/hip/afx_onset.hip (k_max_filter, k_onset_pick<LDS | global>, k_db_max, k_db_map)
// compiled for the host against tests/emu/hip/hip_runtime.h; exports afxk_max_filter / afxk_onset_pick / afxk_power_to_db.
// The novelty is the emulated device code of tests/emu/descriptors_emulated.cpp; everything else of the device layer is the
// generated stand-in.
#include "hip/hip_runtime.h"

namespace {
alignas(16) unsigned char smem_raw[64 * 1024];
}
#include "../../audioflux_amd/csrc/hip/afx_onset.hip"
