// wf_math_check.hip — TEST HOOK, its own library (libwfcheck.so, never linked into libwfstep.so): one entry point that
// evaluates a routine of wf_f64_math.h, or the device library's counterpart, on arrays of arguments.  The header lives in an
// anonymous namespace and has no entry point of its own; this unit includes it under the product's $(FLAGS), so
// tests/test_f64_math_gpu.py measures the arithmetic that ships.  The ids below are mirrored in tests/f64_math_cases.py.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../wf_f64_math.h"

enum WfCheckFn : int {
  // the header's routines: one id each
  WFC_RCP64 = 0, WFC_SQRT_POS, WFC_SQRT_NN, WFC_EXP_LEAN, WFC_LOG_LEAN, WFC_LOG_ANY, WFC_POW_LEAN, WFC_POW_ANY,
  WFC_SINCOS_SMALL, WFC_SINCOS_ANY, WFC_TAN_SMALL, WFC_TAN_ANY, WFC_ASIN_SMALL, WFC_ASIN_ANY, WFC_ATAN_SMALL, WFC_ATAN_01,
  WFC_ATAN2_ANY, WFC_CBRT_POS, WFC_CBRT_ANY,
  // the device library on the same arguments: a yardstick, nothing is asserted on it
  WFC_LIB_RCP = 100, WFC_LIB_SQRT, WFC_LIB_EXP, WFC_LIB_LOG, WFC_LIB_POW, WFC_LIB_SINCOS, WFC_LIB_TAN, WFC_LIB_ASIN,
  WFC_LIB_ATAN, WFC_LIB_ATAN2, WFC_LIB_CBRT
};

// out0[i] = f(in0[i] [, in1[i]]); sincos: out0 = sin, out1 = cos.  The id is a kernel argument: the switch is wave-uniform.
__global__ void wf_math_check_kernel(int fn, const double* __restrict__ in0, const double* __restrict__ in1,
                                     double* __restrict__ out0, double* __restrict__ out1, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a = in0[i];
  const double b = in1 ? in1[i] : 0.0;
  double r = 0.0, r1 = 0.0;
  switch (fn) {
    case WFC_RCP64: r = rcp64(a); break;
    case WFC_SQRT_POS: r = sqrt_pos(a); break;
    case WFC_SQRT_NN: r = sqrt_nn(a); break;
    case WFC_EXP_LEAN: r = exp_lean(a); break;
    case WFC_LOG_LEAN: r = log_lean(a); break;
    case WFC_LOG_ANY: r = log_any(a); break;
    case WFC_POW_LEAN: r = pow_lean(a, b); break;
    case WFC_POW_ANY: r = pow_any(a, b); break;
    case WFC_SINCOS_SMALL: sincos_small(a, r, r1); break;
    case WFC_SINCOS_ANY: sincos_any(a, r, r1); break;
    case WFC_TAN_SMALL: r = tan_small(a); break;
    case WFC_TAN_ANY: r = tan_any(a); break;
    case WFC_ASIN_SMALL: r = asin_small(a); break;
    case WFC_ASIN_ANY: r = asin_any(a); break;
    case WFC_ATAN_SMALL: r = atan_small(a); break;
    case WFC_ATAN_01: r = atan_01(a); break;
    case WFC_ATAN2_ANY: r = atan2_any(a, b); break;
    case WFC_CBRT_POS: r = cbrt_pos(a); break;
    case WFC_CBRT_ANY: r = cbrt_any(a); break;
    case WFC_LIB_RCP: r = 1.0 / a; break;
    case WFC_LIB_SQRT: r = sqrt(a); break;
    case WFC_LIB_EXP: r = exp(a); break;
    case WFC_LIB_LOG: r = log(a); break;
    case WFC_LIB_POW: r = pow(a, b); break;
    case WFC_LIB_SINCOS: r = sin(a); r1 = cos(a); break;
    case WFC_LIB_TAN: r = tan(a); break;
    case WFC_LIB_ASIN: r = asin(a); break;
    case WFC_LIB_ATAN: r = atan(a); break;
    case WFC_LIB_ATAN2: r = atan2(a, b); break;
    case WFC_LIB_CBRT: r = cbrt(a); break;
    default: r = __builtin_nan(""); r1 = r; break;
  }
  out0[i] = r;
  if (out1) out1[i] = r1;
}

// fn: a WfCheckFn; in0, out0: n doubles on the device; in1 (two-argument routines) and out1 (sincos) may be null.
// Returns 0, -1 for an argument it refuses, or the hipError_t of the launch.
extern "C" int wf_math_check(int fn, const double* in0, const double* in1, double* out0, double* out1, long long n,
                             hipStream_t stream) {
  if (!in0 || !out0 || n < 0) return -1;
  const bool two_in = fn == WFC_POW_LEAN || fn == WFC_POW_ANY || fn == WFC_ATAN2_ANY || fn == WFC_LIB_POW || fn == WFC_LIB_ATAN2;
  if (two_in && !in1) return -1;
  if (n == 0) return 0;
  const long long blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(wf_math_check_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, fn, in0, in1, out0, out1, n);
  return (int)hipGetLastError();
}
