// wf_windgen.h — what the two translation units of the wind generator extension (include/wfwindgen.h) share: the arguments of
// the two generating kernels and their launcher (wf_windgen_kernels.hip), called from the C boundary (wf_windgen_abi.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfwindgen.h"

struct WfWindgenArgs {
  int B, T;
  unsigned long long seed;
  double ws_revert, ws_sigma, wd_revert, wd_sigma, wd_ramp;
  double ws_lo, ws_hi;  // the distribution's speed bounds: the stored speed's clip
  double *ws, *wd;      // [T][B] tick-major; row 0 holds tick 0 already, the kernel writes rows 1 .. T - 1
};

// tiled != 0: wf_windgen_tiled_kernel, else wf_windgen_kernel — the same bits
extern "C" hipError_t wfk_launch_windgen(const WfWindgenArgs* a, int tiled, hipStream_t s);
extern "C" hipError_t wfk_windgen_func_attributes(int kernel, hipFuncAttributes* a);
