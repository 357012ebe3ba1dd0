// the DEVICE code of audioflux_amd/csrc/hip/afx_descriptors.hip (k_desc_rows / _wide / _long, k_desc_frames, k_desc_preprocess)
// compiled for the host against tests/emu/hip/hip_runtime.h; exports afxk_descriptors / afxk_desc_preprocess
#include "hip/hip_runtime.h"
#include "../../audioflux_amd/csrc/hip/afx_descriptors.hip"
