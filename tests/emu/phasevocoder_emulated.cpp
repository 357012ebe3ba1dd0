// the DEVICE code of audioflux_amd/csrc/hip/afx_phasevocoder.hip (k_pv_polar, k_pv_phase, k_pv_synthesis, k_rows_fit) compiled
// for the host against tests/emu/hip/hip_runtime.h; exports afxk_phase_vocoder and afxk_rows_fit.  Everything else of the
// device layer is the generated stand-in.
#include "hip/hip_runtime.h"

#include "../../audioflux_amd/csrc/hip/afx_phasevocoder.hip"
