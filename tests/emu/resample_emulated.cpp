// the DEVICE code of audioflux_amd/csrc/hip/afx_resample.hip (k_resample<table in LDS / global, 1 / 2 / 4 clips>) compiled
// for the host against tests/emu/hip/hip_runtime.h; exports afxk_resample.  Everything else of the device layer is the
// generated stand-in.
#include "hip/hip_runtime.h"

namespace {
alignas(16) unsigned char smem_raw[160 * 1024];
}
#include "../../audioflux_amd/csrc/hip/afx_resample.hip"
