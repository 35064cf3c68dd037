// wf_lookahead_kernels.hip — the kernels around the step kernel that make multi-step look-ahead returns run on the device
// (include/wflookahead.h).  The farm solve is the existing wf_step on the object's evaluator handle; these two kernels are the
// glue, so that a whole run is enqueued without a host read:
//
//   wf_lookahead_layout_kernel  once per chunk, ONE WORKGROUP PER SLOT.  Thread (k, t), t fastest, keeps the yaw, the
//                               accumulator and the move counter of turbine t in registers and walks sequence k's steps
//                               h = 0 .. H - 1 with the env's transition (wf_env_transition, ext/wf_ext_kernels.h): it reads
//                               actions[((slot K + k) H + h) N + t] and writes yaw[(slot R + k H + h) N + t] — consecutive
//                               lanes on consecutive floats on both sides — and final_yaw after the last step.  Every row's
//                               wind: the caller's wind of step h, or the parent's device wind held.
//   wf_lookahead_reduce_kernel  once per chunk, after the step, ONE WORKGROUP PER SLOT.  The slot's R = K H rows go by in
//                               LDS tiles (wf_staged_row_rewards, ext/wf_ext_kernels.h: the tile of wf_credit_reduce_kernel —
//                               odd row strides, float64 sums in the stated orders); the thread of a tile's row leaves the
//                               row's reward in LDS ([K][Hs] doubles, Hs = H | 1 where that fits: no bank conflict when
//                               thread k walks sequence k) and writes rewards / farm_power, consecutive threads on consecutive
//                               doubles.  After the last tile's barrier thread k forms sequence k's discounted return in
//                               ascending h; the argmax is a fixed-order reduction: every thread over its own k ascending,
//                               then a tree over the threads in LDS, the larger return and among equal ones the lower index.
//
// The row normalisers: step 0's is the parent's (the pending prev-wind speed, else the current speed), step h >= 1's the
// speed of row (k, h - 1), read from the evaluator's wind block.  LDS per block stays below 64 KiB (36 KiB of rewards at
// most, 24 KiB of tile, 3 KiB of argmax).  Trip counts are run-time values: no private segment, no spill
// (tests/test_lookahead.py reads the metadata); every barrier sits in block-uniform control flow.  The library is built with
// -ffp-contract=off: the transition's float32 sums and the return's product and sum stay single roundings, as in the step
// kernels and the NumPy restatement.
#include <hip/hip_runtime.h>

#include "wf_lookahead.h"

__global__ __launch_bounds__(256) void wf_lookahead_layout_kernel(const WfLookaheadLayoutArgs a) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = a.N, K = a.K, H = a.H, R = K * H;
  const int slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  const bool writes = slot < a.sl.n_slots;
  const size_t in = writes ? slot : 0;  // the slot's input block
  const size_t st0 = (size_t)b * N;     // ... and its farm's env state
  const double ws0 = a.ws[(size_t)b * a.wind_stride], wd0 = a.wd[(size_t)b * a.wind_stride];
  const double* __restrict__ wind = a.wind ? a.wind + in * H * 2 : nullptr;
  for (int r = tid; r < R; r += nth) {
    const int h = r % H;
    a.ews[(size_t)slot * R + r] = wind ? wind[2 * h] : ws0;
    a.ewd[(size_t)slot * R + r] = wind ? wind[2 * h + 1] : wd0;
  }
  const int moves0 = a.env.moves[b];
  const float* __restrict__ act = a.actions + in * R * N;
  float* __restrict__ out = a.yaw + (size_t)slot * R * N;
  const int n_traj = K * N;
  for (int q = tid; q < n_traj; q += nth) {
    const int k = q / N, t = q - k * N;
    float y = a.env.yaw[st0 + t], acc = a.env.acc[st0 + t];
    size_t o = (size_t)k * H * N + t;
    for (int h = 0; h < H; ++h, o += N) {
      float da;
      y = wf_env_transition(a.env, y, act[o], acc, moves0 + 1 + h, da);
      acc += fabsf(da);
      out[o] = y;
    }
    if (writes && a.final_yaw) a.final_yaw[in * n_traj + q] = y;
  }
}

__global__ __launch_bounds__(256) void wf_lookahead_reduce_kernel(const WfLookaheadReduceArgs a, int T, int sp, int sl, int Hs) {
  extern __shared__ double la_red[];
  wf_sequence_returns(a, T, sp, sl, Hs, la_red);
}

extern "C" hipError_t wfk_launch_lookahead_layout(const WfLookaheadLayoutArgs* a, hipStream_t s) {
  const int threads = a->K * a->N <= 64 ? 64 : 256;  // a few short sequences of a small farm: one wave
  hipLaunchKernelGGL(wf_lookahead_layout_kernel, dim3(a->sl.C), dim3(threads), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_lookahead_reduce(const WfLookaheadReduceArgs* a, hipStream_t s) {
  const WfReturnsLaunch l = wf_returns_launch(a->N, a->K, a->H);
  hipLaunchKernelGGL(wf_lookahead_reduce_kernel, dim3(a->sl.n_slots), dim3(l.threads), l.lds_bytes, s, *a, l.t.T, l.t.sp, l.t.sl, l.Hs);
  return hipGetLastError();
}
extern "C" hipError_t wfk_lookahead_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[WF_LOOKAHEAD_KERNELS] = {(const void*)wf_lookahead_layout_kernel, (const void*)wf_lookahead_reduce_kernel};
  if (kernel < 0 || kernel >= WF_LOOKAHEAD_KERNELS) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, fn[kernel]);
}
