// wf_probe.h — what the two translation units of the probe extension (include/wfprobe.h) share: the arguments of the two
// kernels of wf_probe_kernels.hip and their launchers, called by wf_probe_abi.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../wf_resolve.h"

// Per-source state record the float64 farm solve leaves for the sampler: [farm slot][sorted turbine][WF_PROBE_REC] doubles.
// The record holds the source's constants already DERIVED (near-wake lengths, initial widths, the deflection's far-wake
// prefactor ...) instead of the dozen raw state values (Ct, induction, yaw, TI): a sampler block of a 16-point set would
// otherwise redo 80 sources' square roots and tangents for 16 points.  The sampler stages the whole record in LDS.
#define WF_PROBE_REC 20
enum {
  PR_X = 0, PR_Y, PR_GT, PR_GB, PR_GW,                       // sorted x', y'; circulations / (2 pi): top, bottom, wake rotation [A.3-4]
  PR_X0D, PR_KYD, PR_D0, PR_PFAR, PR_X0V, PR_KYV,            // of the centre column's TI: deflection (before mixing), deficit (after) [A.3-3, A.3-6]
  PR_SY0D, PR_SZ0D, PR_IS0D, PR_SM, PR_LNAB, PR_SY0V, PR_SZ0V, PR_SNW, PR_KDEF  // independent of TI
};
static_assert(PR_KDEF + 1 == WF_PROBE_REC, "the record is exactly what the sampler reads");
// Per-farm header: [farm slot][WF_PROBE_HDR] doubles — wind speed, cos / sin of the rotation angle (the sampler rotates a
// point with the very numbers the farm was rotated with)
#define WF_PROBE_HDR 3

struct WfProbeConsts {
  WfResolveConsts r;
  double shear, kappa, lm_c;  // lm = kappa z / (1 + kappa z / lm_c), lm_c = D / 8 [A.3-4]
  double dudz_c;              // shear (1 / HH)^shear: dU/dz = ws dudz_c z^(shear - 1) [A.2]
  double inv_HH;
  double xc, yc;              // centre of rotation [A.1-1]
};

struct WfProbeStateArgs {
  const double* tab64;     // [3][WF_TABLE_PAD] wind speed, Ct, power (the handle's float64 tables)
  const double *lx, *ly;   // [N] layout, caller's order
  const double *ws, *wd;   // the handle's wind
  int wind_stride;         // 0 shared, 1 per farm
  const float* yaw;        // [B][N] absolute yaw, caller's order
  const int* farms;        // [n_farms] farm of each slot, or null: slot == farm
  double* rec;             // [n_farms][N][WF_PROBE_REC]
  double* hdr;             // [n_farms][WF_PROBE_HDR]
};

struct WfProbeSampleArgs {
  const double* rec;
  const double* hdr;
  const int* farms;        // as above
  const double* xyz;       // [n_sets][P][3]
  int per_farm;            // 1: the set of farm b is xyz + b P 3
  int P;
  float* uvw;              // [n_farms][P][3]
};

extern "C" hipError_t wfk_launch_probe_state(const WfProbeConsts* c, const WfProbeStateArgs* a, int n_farms, hipStream_t s);
extern "C" hipError_t wfk_launch_probe_sample(const WfProbeConsts* c, const WfProbeSampleArgs* a, int n_farms, hipStream_t s);
extern "C" hipError_t wfk_probe_func_attributes(int which, hipFuncAttributes* a);
