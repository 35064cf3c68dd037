// wf_scenario_kernels.hip — the kernels around the step kernel that make scenario look-ahead run on the device
// (include/wfscenario.h).  The farm solve is the existing wf_step on the object's evaluator handle; these two kernels are the
// glue, so that a whole run — the ensemble's draws included — is enqueued without a host read:
//
//   wf_scenario_layout_kernel  once per chunk, ONE WORKGROUP PER SLOT.  The M member paths of the slot's farm, every row's
//                              evaluator wind and wind_paths are the ensemble's tiled body (ensemble/wf_ensemble.h:
//                              wf_ensemble_tiles), in tiles of 2048 / M ticks.  Then thread (k, t), t fastest, keeps the yaw
//                              and the accumulator of turbine t in registers and walks sequence k's steps with the env's
//                              transition (wf_env_transition, ext/wf_ext_kernels.h), as wf_lookahead_layout_kernel does, and
//                              stores each yaw to the M member rows of that step: consecutive lanes write consecutive floats.
//   wf_scenario_reduce_kernel  once per chunk, after the step, ONE WORKGROUP PER SLOT: row rewards, member returns, the statistics
//                              and the choice — the body of wf_scenario_reduce.h (wf_scenario_statistics), which the
//                              scenario-rollout extension instantiates too.
//
// The row normalisers: step 0's is the farm's CURRENT speed (a pending prev-wind speed is not read), step h >= 1's the speed
// of row (k, m, h - 1), read from the evaluator's wind block.  LDS per block stays below 64 KiB: the lay-out's tile is at most
// 2 x (2048 + 64) doubles (33 KiB); the reduce kernel's is laid out as wf_lookahead_reduce_kernel's with K M sequences (36 KiB
// of rewards at most, 3 KiB — 12 KiB with 1024 threads — for the passes and the argmax) and its tile takes the rest of 63 KiB,
// 24 KiB at the least.  Trip counts are run-time values: no private segment,
// no spill (tests/test_scenario.py reads the metadata); every barrier sits in block-uniform control flow.  The library is
// built with -ffp-contract=off: every product and sum of the paths and the statistics is one rounding, in the header's order.
#include <hip/hip_runtime.h>

#include "wf_scenario.h"
#include "wf_scenario_reduce.h"

__global__ __launch_bounds__(256) void wf_scenario_layout_kernel(const WfScenarioLayoutArgs a, int Ht, int Hs) {
  extern __shared__ double sc_tile[];
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = a.N, K = a.K, M = a.ens.M, H = a.ens.H, MH = M * H, R = K * MH;
  const int slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  wf_ensemble_tiles(a.ens, a.sl, K, Ht, Hs, sc_tile, a.ews, a.ewd, a.wind_paths);
  // the trajectories: what addresses them is formed HERE, from the slot and the farm in vector registers — formed at the top
  // and held in scalar registers across the draws it would not fit (spilled scalar registers)
  int slot_v = slot, b_v = b;
  WF_IN_VGPR(slot_v); WF_IN_VGPR(b_v);
  const bool writes_v = slot_v < a.sl.n_slots;
  const size_t in_v = writes_v ? slot_v : 0, st0 = (size_t)b_v * N;
  const int moves0 = a.env.moves[b_v];
  const float* __restrict__ act = a.actions + in_v * K * H * N;
  float* __restrict__ out = a.yaw + (size_t)slot_v * R * N;
  const int n_traj = K * N;
  const size_t member = (size_t)H * N;  // floats from a member's row of step h to the next member's
  for (int q = tid; q < n_traj; q += nth) {
    const int k = q / N, t = q - k * N;
    float yw = a.env.yaw[st0 + t], acc = a.env.acc[st0 + t];
    size_t i = (size_t)k * H * N + t;   // the action of step h
    size_t o = (size_t)k * MH * N + t;  // row (k, 0, h)
    for (int h = 0; h < H; ++h, i += N, o += N) {
      float da;
      yw = wf_env_transition(a.env, yw, act[i], acc, moves0 + 1 + h, da);
      acc += fabsf(da);
      size_t om = o;
      for (int m = 0; m < M; ++m, om += member) out[om] = yw;
    }
    if (writes_v && a.final_yaw) a.final_yaw[in_v * n_traj + q] = yw;
  }
}

__global__ __launch_bounds__(1024) void wf_scenario_reduce_kernel(const WfScenarioReduceArgs a, int T, int sp, int sl, int Hs) {
  extern __shared__ double sc_red[];
  wf_scenario_statistics(a, T, sp, sl, Hs, sc_red);
}

extern "C" hipError_t wfk_launch_scenario_layout(const WfScenarioLayoutArgs* a, hipStream_t s) {
  const int R = a->K * a->ens.M * a->ens.H;
  const int threads = (R <= 128 && a->K * a->N <= 64) ? 64 : 256;  // a few short sequences of a small farm: one wave
  const WfEnsembleTile t = wf_ensemble_tile(a->ens.M, a->ens.H);
  const size_t lds = sizeof(double) * 2 * (size_t)a->ens.M * t.Hs;
  hipLaunchKernelGGL(wf_scenario_layout_kernel, dim3(a->sl.C), dim3(threads), lds, s, *a, t.Ht, t.Hs);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_scenario_reduce(const WfScenarioReduceArgs* a, hipStream_t s) {
  const WfScenarioReduceLaunch l = wf_scenario_reduce_launch(a->N, a->K, a->M, a->H);
  hipLaunchKernelGGL(wf_scenario_reduce_kernel, dim3(a->sl.n_slots), dim3(l.threads), l.lds_bytes, s, *a, l.t.T, l.t.sp, l.t.sl, l.Hs);
  return hipGetLastError();
}
extern "C" hipError_t wfk_scenario_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[WF_SCENARIO_KERNELS] = {(const void*)wf_scenario_layout_kernel, (const void*)wf_scenario_reduce_kernel};
  if (kernel < 0 || kernel >= WF_SCENARIO_KERNELS) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, fn[kernel]);
}
