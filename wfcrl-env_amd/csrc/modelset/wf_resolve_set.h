// wf_resolve_set.h — the members of WfResolveConsts (../wf_resolve.h) that a wake-model parameter set OWNS, built on the device:
// a restatement of those lines of fill_resolve_consts (../wf_model.hip), to be read beside it — the same expressions in the
// same order of operations, every one rounded once (-ffp-contract=off).  It lives here and not next to wf_resolve.h because
// the directory above is the recorded source set of the fuzz campaign (profiles/fuzz_head.json).
//
// What a set owns:  amb; shearf[3], uinf1, nu1[3], vel_top, vel_bot (shear); alpha .. dm and defl_*; ch_constant, ch_ai,
// ch_amb_pow, ch_down; cos_veer, cos2_veer, sin2_veer, sin_2veer.  Everything else of an entry — N, the switches, D, HH, TSR, the
// vortex tables, near_c, the GCH internals, the density terms — is the model's and is READ here from the entry itself, which
// the host code has filled (modelset/wf_modelset.hip: modelset_upload); kappa is no member and comes as an argument.
//
// NOT BIT-IDENTICAL to the host-built table: pow, cos and sin are wf_f64_math.h's general-range routines (pow_any: 3 + 2 |y ln x|
// ulp; sincos_any: 3.3e-16 absolute — tests/test_f64_math_gpu.py) where the host calls glibc's.  The constants differ by a few
// ulp; what is held is the oracle tolerance of the solve (tests/test_calib_gpu.py), not bits against wf_set_model_sets.
// Exact all the same: x^0 = 1, 1^y = 1 (the hub row's shear factor), veer 0 -> cos 1, sin 0.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfmodelset.h"
#include "../wf_f64_math.h"
#include "../wf_resolve.h"

// what wf_set_model_sets asks of a set beyond finiteness, with its roundings (modelset/wf_modelset.hip: modelset_validate)
__device__ __forceinline__ bool wf_model_set_valid(const wf_model_set& s) {
  return s.ambient_ti > 0.0 && s.alpha > 0.0 && s.defl_alpha > 0.0 && s.ka * s.ambient_ti + s.kb > 0.0 &&
         s.defl_ka * s.ambient_ti + s.defl_kb > 0.0 && s.ch_constant > 0.0;
}

// The set-owned members of *out from s, one thread per entry, in two parts: a caller that loops over entries runs each part in a
// loop of its own — the compiler keeps a loop's float64 literals in scalar registers, and the polynomials of pow and of sin / cos
// together take more of them than there are.
// ... part 1: everything but the veer terms (pow)
__device__ __forceinline__ void wf_resolve_set_flow(const wf_model_set& s, double kappa, WfResolveConsts* __restrict__ out) {
  WfResolveConsts& r = *out;
  const double D = r.D, HH = r.HH, R = D / 2;
  r.amb = s.ambient_ti;
  double uinf1 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double off = k == 0 ? -D / 4 : (k == 1 ? 0.0 : D / 4);
    const double shearf = pow_any((HH + off) / HH, s.shear);
    r.shearf[k] = shearf;
    uinf1 += shearf;
    const double z = HH + off;
    const double dudz1 = s.shear * pow_any(1.0 / HH, s.shear) * pow_any(z, s.shear - 1.0);
    const double lm = kappa * z / (1.0 + kappa * z / (D / 8.0));
    r.nu1[k] = lm * lm * fabs(dudz1);
  }
  r.uinf1 = uinf1 / 3.0;
  r.vel_top = pow_any((HH + R) / HH, s.shear);
  r.vel_bot = pow_any((HH - R) / HH, s.shear);
  r.alpha = s.alpha; r.beta = s.beta; r.ka = s.ka; r.kb = s.kb; r.ad = s.ad; r.bd = s.bd; r.dm = s.dm;
  r.defl_alpha = s.defl_alpha; r.defl_beta = s.defl_beta; r.defl_ka = s.defl_ka; r.defl_kb = s.defl_kb;
  r.ch_constant = s.ch_constant; r.ch_ai = s.ch_ai; r.ch_amb_pow = pow_any(s.ambient_ti, s.ch_initial); r.ch_down = s.ch_downstream;
}
// ... part 2: the four veer terms (sin, cos)
__device__ __forceinline__ void wf_resolve_set_veer(double veer, WfResolveConsts* __restrict__ out) {
  WfResolveConsts& r = *out;
  const double vr = veer * 3.14159265358979323846 / 180.0;
  double sv, cv, s2, c2;
  sincos_any(vr, sv, cv);
  sincos_any(2.0 * vr, s2, c2);
  r.cos_veer = cv; r.cos2_veer = cv * cv; r.sin2_veer = sv * sv;
  r.sin_2veer = s2;
}
