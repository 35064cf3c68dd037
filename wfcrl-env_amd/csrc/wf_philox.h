// wf_philox.h — the counter-based generator of the device code: Philox4x32-10 (Salmon et al., SC'11), keyed by a 64-bit seed,
// counted by a 64-bit counter and a 32-bit stream.  One definition for the wind process (wf_kernels.hip: reset sampling,
// series starts) and the planner's candidates (plan/wf_plan_kernels.hip): a draw depends on (seed, counter, stream) alone,
// never on the launch, the batch or the order of the threads.  (seed 0, counter 0, stream 0) is Random123's zero-key,
// zero-counter vector 6627e8d5 e169c58d bc57ac4c 9b00dbd8 (tests/plan_ref.py restates the arithmetic in NumPy).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void philox_round(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0,
                                             unsigned k1) {
  const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
  const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
  const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
  const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
  c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}
__device__ __forceinline__ void philox4x32_10(unsigned long long seed, unsigned long long ctr, unsigned stream,
                                              unsigned out[4]) {
  unsigned c0 = (unsigned)ctr, c1 = (unsigned)(ctr >> 32), c2 = stream, c3 = 0;
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ double u01(unsigned hi, unsigned lo) {  // (0, 1), 53 bits
  const unsigned long long v = (((unsigned long long)hi << 32) | lo) >> 11;
  return ((double)v + 0.5) * (1.0 / 9007199254740992.0);
}
