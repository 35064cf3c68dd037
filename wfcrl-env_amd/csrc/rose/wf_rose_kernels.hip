// wf_rose_kernels.hip — the kernels around the step kernel that make an expected-power evaluation over a wind rose, and a
// yaw look-up-table controller, run on the device (include/wfrose.h).  The farm solve is the existing wf_step on the rose
// object's evaluator handle; these kernels are the glue, so that a whole evaluation is enqueued without a host read:
//
//   wf_rose_layout_kernel      once per chunk: each row's wind (ws, wd) and its yaw row — zeros, a copy of a fixed row, or the
//                              table look-up of include/wfrose.h in float64.  ONE WAVE PER ROW, lanes over turbines in a loop
//                              (N can exceed 64): a row's N floats are contiguous, so every store is a whole line.
//   wf_rose_rowsum_kernel      once per chunk: the farm power of every row — its N float32 powers added in caller order in
//                              float64 — masked by cut-in / cut-out, to the partial-sum input and to condition_power: the
//                              staged row sum of ext/wf_ext_kernels.h (wf_staged_rowsum), shared with the robust search.
//   wf_rose_accumulate_kernel  once per chunk: the frequency-weighted sums.  ONE THREAD PER SUM (case x turbine, and case x
//                              farm) walks this chunk's conditions in (d, s) index order in float64, starting from the partial
//                              the previous chunk left in the device buffer: a fixed order whatever the scheduling and
//                              whatever the chunk size — no floating-point atomics.  Neighbouring threads read neighbouring
//                              turbines of a row: coalesced; eight conditions' loads are in flight at a time.
//   wf_rose_policy_kernel      the controller: one wave per farm of the PARENT — the same look-up device function at the
//                              farm's current wind (read on the device), clipped to the env's bounds, and the action that
//                              tracks it from the env's yaw state.
//
// The look-up itself (rose_bracket, rose_lookup, ROSE_PICK) is wf_rose_lookup.h's, shared with the rollout extension.
// Trip counts are run-time values and the table slot is picked by comparison, not by indexing the by-value argument: no
// private segment, no spilled register, no out-of-line call (tests/test_rose.py reads the metadata; wf_probe_kernels.hip
// states what a private segment costs per launch on this device).  The library is built with -ffp-contract=off: a product
// and a sum stay two roundings, as in the NumPy restatement.
#include <hip/hip_runtime.h>

#include "../ext/wf_ext_kernels.h"
#include "wf_rose.h"
#include "wf_rose_lookup.h"

namespace {

__device__ __forceinline__ bool rose_masked(double ws, double cut_in, double cut_out) {
  return ws < cut_in || (cut_out > 0.0 && ws > cut_out);
}

}  // namespace

__global__ __launch_bounds__(256) void wf_rose_layout_kernel(const WfRoseLayoutArgs a) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= a.sh.E) return;
  const int N = a.sh.N, C = a.sh.C, S = a.sh.S;
  const int g = a.sh.row0 + (e < a.sh.n_rows ? e : 0);
  const int s = g % S, dc = g / S;
  const int c = dc % C, d = dc / C;
  const double ws = a.ws[s], wd = a.wd[d];
  if (lane == 0) {
    a.ews[e] = ws;
    a.ewd[e] = wd;
  }
  const int kind = a.cases[c], arg = a.cases[C + c];
  float* __restrict__ row = a.yaw + (size_t)e * N;
  if (kind == WF_ROSE_CASE_TABLE) {
    const WfRoseTable tb = ROSE_PICK(a.tab, arg);
    const RoseBracket b = rose_bracket(tb, ws, wd);
    for (int t = lane; t < N; t += 64) row[t] = rose_lookup(tb, b, t, N);
  } else if (kind == WF_ROSE_CASE_FIXED) {
    const float* __restrict__ src = a.fixed_yaw + (size_t)arg * N;
    for (int t = lane; t < N; t += 64) row[t] = src[t];
  } else {
    for (int t = lane; t < N; t += 64) row[t] = 0.0f;
  }
}

__global__ __launch_bounds__(64) void wf_rose_rowsum_kernel(const WfRoseReduceArgs a, int rows_per_block, int stride) {
  extern __shared__ float rs_pw[];
  const int lane = threadIdx.x;
  const int N = a.sh.N, C = a.sh.C, S = a.sh.S, D = a.sh.D;
  const int e0 = blockIdx.x * rows_per_block;
  int nr = a.sh.n_rows - e0;
  nr = nr > rows_per_block ? rows_per_block : nr;
  double sum = wf_staged_rowsum(a.power + (size_t)e0 * N, nr, N, stride, rs_pw, lane);
  if (lane < nr) {
    const int e = e0 + lane, g = a.sh.row0 + e;
    const int s = g % S, dc = g / S;
    const int c = dc % C, d = dc / C;
    if (rose_masked(a.ws[s], a.cut_in, a.cut_out)) sum = 0.0;
    a.rowsum[e] = sum;
    if (a.condition_power) a.condition_power[((size_t)c * D + d) * S + s] = (float)sum;
  }
}

// One weighted sum: the conditions k = d S + s of the directions this chunk touches, in index order, eight at a time — the
// loads of a batch are issued together (registers, fully unrolled; selects, no branch per condition), the adds stay in index
// order.  A condition outside the chunk, or a masked one, adds 0 x v = 0, which leaves the sum's bits alone: the bits do not
// depend on the chunking.  FARM: the rows' float64 farm powers; otherwise turbine t of the rows' float32 powers.
template <bool FARM>
__device__ __forceinline__ double rose_weighted_sum(const WfRoseReduceArgs& a, int c, int t, double acc) {
  const int N = a.sh.N, C = a.sh.C, S = a.sh.S;
  const int r0 = a.sh.row0, r1 = a.sh.row0 + a.sh.n_rows;  // this chunk's rows
  const int d_lo = r0 / (C * S), d_hi = (r1 - 1) / (C * S);
  const float* __restrict__ pw = a.power;
  const double* __restrict__ rsum = a.rowsum;
  const double* __restrict__ freq = a.freq;
  const double* __restrict__ ws = a.ws;
  const int k_hi = (d_hi + 1) * S;
  for (int k0 = d_lo * S; k0 < k_hi; k0 += 8) {
    double v[8], f[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + u < k_hi ? k0 + u : k_hi - 1;
      const int d = k / S, sp = k - d * S;
      const int g = (d * C + c) * S + sp;
      const bool in = k0 + u < k_hi && g >= r0 && g < r1;
      const int e = in ? g - r0 : 0;
      if constexpr (FARM) v[u] = rsum[e];
      else v[u] = (double)pw[(size_t)e * N + t];
      const double fk = freq[k];
      f[u] = (!in || rose_masked(ws[sp], a.cut_in, a.cut_out)) ? 0.0 : fk;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += f[u] * v[u];
  }
  return acc;
}

// blocks [0, turbine_blocks): a thread per (case, turbine); the blocks behind them: a thread per case (the farm sums) — so
// that a wave takes one of the two paths as a whole
__global__ __launch_bounds__(256) void wf_rose_accumulate_kernel(const WfRoseReduceArgs a, int turbine_blocks) {
  const int N = a.sh.N, C = a.sh.C;
  if ((int)blockIdx.x < turbine_blocks) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= C * N) return;
    const int c = idx / N, t = idx - c * N;
    a.acc_turbine[idx] = rose_weighted_sum<false>(a, c, t, a.first ? 0.0 : a.acc_turbine[idx]);
  } else {
    const int c = ((int)blockIdx.x - turbine_blocks) * 256 + threadIdx.x;
    if (c >= C) return;
    a.acc_farm[c] = rose_weighted_sum<true>(a, c, 0, a.first ? 0.0 : a.acc_farm[c]);
  }
}

__global__ __launch_bounds__(256) void wf_rose_policy_kernel(const WfRosePolicyArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const int N = a.N;
  const double ws = a.ws[(size_t)b * a.wind_stride], wd = a.wd[(size_t)b * a.wind_stride];
  const RoseBracket br = rose_bracket(a.tab, ws, wd);
  const size_t row0 = (size_t)b * N;
  const float half = 0.5f * a.step;
  for (int t = lane; t < N; t += 64) {
    float tg = rose_lookup(a.tab, br, t, N);
    tg = fminf(fmaxf(tg, a.lo), a.hi);
    if (a.target) a.target[row0 + t] = tg;
    if (a.action) {
      const float dy = tg - a.yaw_state[row0 + t];
      float act;
      if (a.discrete) act = dy >= half ? 2.0f : (dy <= -half ? 0.0f : 1.0f);
      else act = fminf(fmaxf(dy, -a.step), a.step);
      a.action[row0 + t] = act;
    }
  }
}

extern "C" hipError_t wfk_launch_rose_layout(const WfRoseLayoutArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(wf_rose_layout_kernel, dim3((a->sh.E + 3) / 4), dim3(256), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_rose_rowsum(const WfRoseReduceArgs* a, hipStream_t s) {
  const WfRowsumLaunch l = wf_rowsum_launch(a->sh.n_rows, a->sh.N);
  hipLaunchKernelGGL(wf_rose_rowsum_kernel, dim3(l.blocks), dim3(64), l.lds_bytes, s, *a, l.rows_per_block, l.stride);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_rose_accumulate(const WfRoseReduceArgs* a, hipStream_t s) {
  const int tb = (a->sh.C * a->sh.N + 255) / 256, fb = (a->sh.C + 255) / 256;
  hipLaunchKernelGGL(wf_rose_accumulate_kernel, dim3(tb + fb), dim3(256), 0, s, *a, tb);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_rose_policy(const WfRosePolicyArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(wf_rose_policy_kernel, dim3((a->B + 3) / 4), dim3(256), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_rose_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[WF_ROSE_KERNELS] = {(const void*)wf_rose_layout_kernel, (const void*)wf_rose_rowsum_kernel,
                                     (const void*)wf_rose_accumulate_kernel, (const void*)wf_rose_policy_kernel};
  if (kernel < 0 || kernel >= WF_ROSE_KERNELS) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, fn[kernel]);
}
