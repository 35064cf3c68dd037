// wf_deviate.h — the unit-variance deviate of the device code, shared by the planner's candidates (plan/wf_plan_kernels.hip)
// and the synthetic wind process (windgen/wf_windgen_kernels.hip): the sum of the four words of one Philox block (wf_philox.h)
// is an Irwin-Hall sum of four uniforms — mean 2, variance 1/3 in units of 2^32 —, so
//   z = (sum * 2^-32 - 2) * sqrt 3
// has mean 0, variance 1 and |z| <= 2 sqrt 3.  The sum is an integer below 2^34 and the scaling a power of two: z is exact up
// to the last product (tests/plan_ref.py: deviate restates it in NumPy).  The counter is (farm << 32) | index.
#pragma once
#include "../wf_philox.h"

// the deviate of one Philox block's four words
__device__ __forceinline__ double wf_deviate_of(const unsigned r[4]) {
  const unsigned long long S = (unsigned long long)r[0] + r[1] + r[2] + r[3];
  return ((double)S * (1.0 / 4294967296.0) - 2.0) * 1.7320508075688772;
}
// ... and of the block (seed, counter, stream)
__device__ __forceinline__ double wf_deviate(unsigned long long seed, unsigned long long counter, unsigned stream) {
  unsigned r[4];
  philox4x32_10(seed, counter, stream, r);
  return wf_deviate_of(r);
}
