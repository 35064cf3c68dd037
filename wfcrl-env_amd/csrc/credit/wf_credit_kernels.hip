// wf_credit_kernels.hip — the kernels around the step kernel that make per-agent counterfactual rewards run on the device
// (include/wfcredit.h).  The farm solve is the existing wf_step on the object's evaluator handle; these two kernels are the
// glue, so that a whole run is enqueued without a host read:
//
//   wf_credit_layout_kernel  once per chunk, ONE WORKGROUP PER SLOT.  Phase 1: the slot's base yaw and its N K alternative
//                            yaws -> LDS [N][K + 1] (entry 0 the base), the env's transition applied ONCE per (slot, turbine,
//                            alternative) where the value is an action; consecutive threads read consecutive inputs.  A
//                            barrier.  Phase 2: the slot's [R][N] yaw block in one pass, consecutive threads on consecutive
//                            floats: every store is a whole line; element (row, t) is the base entry unless t is the row's own
//                            turbine.  Every row's wind from the parent's device wind, or from the
//                            chunk's override rows (the series-ahead mode, include/wfseries.h).
//   wf_credit_reduce_kernel  once per chunk, after the step, ONE WORKGROUP PER SLOT.  The slot's R rows go by in TILES of T
//                            rows: a tile's [T][N] powers and [T][4 N] load values are contiguous in the evaluator's outputs
//                            and are staged in LDS with coalesced loads, two arrays of odd row stride (the pattern of
//                            wf_staged_rowsum, ext/wf_ext_kernels.h: no bank conflict when a lane walks a row).  Then thread
//                            k < T adds row k in float64 — the powers in caller order, the absolute load values in memory
//                            order — and leaves the row's reward and farm power in LDS ([R] doubles each, R <= 2049).  After
//                            the last tile's barrier ALL threads write reward, farm_power and difference, consecutive threads
//                            on consecutive doubles; a row whose alternative has the bits of the base entry (read back from the
//                            evaluator's yaw block) gets row 0's values and a difference of exactly 0.0.
//
// The transition and the tile loop are wf_env_transition and wf_staged_row_rewards (ext/wf_ext_kernels.h), shared with lookahead/.
// T is what 24 KiB of LDS holds (15 rows at N = 80, 4 at N = 256, every row of a farm of 7 with K = 3); with the two [R]
// arrays a block stays below 57 KiB.  Trip counts are run-time values: no private segment, no spill (tests/test_credit.py
// reads the metadata); every barrier sits in block-uniform control flow.  The library is built with -ffp-contract=off: the
// transition's float32 sum and the reward's products stay single roundings, as in the step kernels and the NumPy restatement.
#include <hip/hip_runtime.h>

#include "wf_credit.h"

__global__ __launch_bounds__(256) void wf_credit_layout_kernel(const WfCreditLayoutArgs a) {
  extern __shared__ float cr_lay[];  // [N][K + 1]: the base yaw, then the K alternatives, of every turbine
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = a.N, K = a.K, K1 = K + 1, R = 1 + N * K;
  const int slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  const size_t in0 = (size_t)(slot < a.sl.n_slots ? slot : 0) * N;  // the slot's input rows
  const size_t st0 = (size_t)b * N;                                 // ... and its farm's env state
  const int moves_new = a.env.moves ? a.env.moves[b] + 1 : 1;
  const size_t in_slot = slot < a.sl.n_slots ? slot : 0;
  const double ws = a.wind ? a.wind[2 * in_slot] : a.ws[(size_t)b * a.wind_stride];
  const double wd = a.wind ? a.wind[2 * in_slot + 1] : a.wd[(size_t)b * a.wind_stride];
  for (int r = tid; r < R; r += nth) {
    a.ews[(size_t)slot * R + r] = ws;
    a.ewd[(size_t)slot * R + r] = wd;
  }
  const int n_val = N * K1;
  for (int q = tid; q < n_val; q += nth) {
    const int t = q / K1, k = q - t * K1;
    int kind;
    float v;
    if (k == 0) {
      kind = a.base ? a.base_kind : WF_CREDIT_YAW;
      v = a.base ? a.base[in0 + t] : a.env.yaw[st0 + t];
    } else {
      kind = a.alt_kind;
      v = a.alt ? a.alt[(in0 + t) * K + (k - 1)] : (kind == WF_CREDIT_ACTION && a.env.discrete ? 1.0f : 0.0f);  // hold / zero yaw
    }
    float da;  // (the accumulator is not carried: one step)
    if (kind == WF_CREDIT_ACTION) v = wf_env_transition(a.env, a.env.yaw[st0 + t], v, a.env.acc[st0 + t], moves_new, da);
    cr_lay[q] = v;
  }
  __syncthreads();
  float* __restrict__ out = a.yaw + (size_t)slot * R * N;
  const int n_out = R * N;
  for (int q = tid; q < n_out; q += nth) {
    const int row = q / N, t = q - row * N;
    int src = t * K1;
    if (row > 0) {
      const int i = (row - 1) / K;
      if (t == i) src += row - i * K;  // 1 + k, k = row - 1 - i K
    }
    out[q] = cr_lay[src];
  }
}

__global__ __launch_bounds__(256) void wf_credit_reduce_kernel(const WfCreditReduceArgs a, int T, int sp, int sl) {
  extern __shared__ double cr_red[];
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = a.N, K = a.K, R = 1 + N * K;
  double* rw = cr_red;                                // [R] row rewards
  double* ps = cr_red + R;                            // [R] row farm powers
  float* pw = reinterpret_cast<float*>(cr_red + 2 * R);  // [T][sp] a tile's powers
  float* ld = pw + T * sp;                            // [T][sl] ... and load values
  const int slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  const double wr = a.ws_prev ? a.ws_prev[b] : a.ws[(size_t)b * a.wind_stride];
  const float* __restrict__ pblk = a.power_ev + (size_t)slot * R * N;
  const float* __restrict__ lblk = a.load_ev + (size_t)slot * R * 4 * N;
  wf_staged_row_rewards(pblk, lblk, R, N, T, sp, sl, a.load_coef, pw, ld, [wr](int) { return wr; },
                        [rw, ps](int row, double r, double psum) { rw[row] = r; ps[row] = psum; });
  const float* __restrict__ yblk = a.yaw_ev + (size_t)slot * R * N;
  const size_t o_row = (size_t)slot * R, o_dif = (size_t)slot * N * K;
  const double r_base = rw[0], p_base = ps[0];
  for (int q = tid; q < R; q += nth) {
    bool same = false;  // the alternative's float32 yaw has the bits of the base entry
    if (q > 0) {
      const int i = (q - 1) / K;
      same = __float_as_uint(yblk[(size_t)q * N + i]) == __float_as_uint(yblk[i]);
    }
    if (a.reward) a.reward[o_row + q] = same ? r_base : rw[q];
    if (a.farm_power) a.farm_power[o_row + q] = same ? p_base : ps[q];
    if (a.difference && q > 0) a.difference[o_dif + q - 1] = same ? 0.0 : r_base - rw[q];
  }
}

extern "C" hipError_t wfk_launch_credit_layout(const WfCreditLayoutArgs* a, hipStream_t s) {
  const int N = a->N, K = a->K, R = 1 + N * K;
  const int threads = R * N <= 512 ? 64 : 256;  // a small farm's block is a few hundred floats: one wave
  const size_t lds = sizeof(float) * (size_t)N * (K + 1);
  hipLaunchKernelGGL(wf_credit_layout_kernel, dim3(a->sl.C), dim3(threads), lds, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_credit_reduce(const WfCreditReduceArgs* a, hipStream_t s) {
  const int N = a->N, R = 1 + N * a->K;
  const int threads = R * N <= 512 ? 64 : 256;
  const WfRewardTile t = wf_reward_tile(R, N, threads);
  const size_t lds = sizeof(double) * 2 * (size_t)R + t.lds_bytes;
  hipLaunchKernelGGL(wf_credit_reduce_kernel, dim3(a->sl.n_slots), dim3(threads), lds, s, *a, t.T, t.sp, t.sl);
  return hipGetLastError();
}
extern "C" hipError_t wfk_credit_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[WF_CREDIT_KERNELS] = {(const void*)wf_credit_layout_kernel, (const void*)wf_credit_reduce_kernel};
  if (kernel < 0 || kernel >= WF_CREDIT_KERNELS) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, fn[kernel]);
}
