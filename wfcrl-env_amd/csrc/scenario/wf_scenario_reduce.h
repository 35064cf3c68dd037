// wf_scenario_reduce.h — the reduce of K M H rows in the scenario order, row = (k M + m) H + h, to row rewards, member returns,
// mean, tail mean, score and a choice (include/wfscenario.h: ROW REWARD, MEMBER RETURN, STATISTICS): the ONE body the reduce
// kernels of the scenario extension (wf_scenario_kernels.hip: K action sequences) and of the scenario-rollout extension
// (rollscen/wf_rollscen_kernels.hip: K controllers) instantiate, and its launch choice.
//
// ONE WORKGROUP PER SLOT.  The slot's R = K M H rows go by in the shared reward tile (wf_staged_row_rewards); the thread of a
// tile's row leaves the row's reward in LDS ([K M][Hs] doubles) and writes rewards.  Thread (k, m) forms its discounted return
// in ascending h, as wf_sequence_returns does, and leaves it in its row's first entry.  The statistics and the choice are the ensemble's
// (ensemble/wf_ensemble.h: wf_member_statistics over the returns at stride Hs, which emits to the three output arrays, then
// wf_argmax_tree).
//
// The row normalisers: step 0's is the farm's CURRENT speed (a pending prev-wind speed is not read), step h >= 1's the speed
// of row (k, m, h - 1), read from the evaluator's wind block.  LDS is laid out as wf_lookahead_reduce_kernel's with K M
// sequences (36 KiB of rewards at most, 3 KiB — 12 KiB with 1024 threads — for the passes and the argmax) and the tile takes
// the rest of 63 KiB, 24 KiB at the least.  Trip counts are run-time values: no private segment, no spill; every barrier sits
// in block-uniform control flow.
#pragma once
#include <hip/hip_runtime.h>

#include "wf_scenario.h"

#define WF_SCENARIO_WIDE 8192  // floats of power per slot (R N) from which the reduce kernel runs 1024 threads

// `sc_red` is the block's dynamic LDS: [K M][Hs] + [nth] doubles (bv), [nth] ints (bi), then the tile's [T][sp] + [T][sl] floats
__device__ __forceinline__ void wf_scenario_statistics(const WfScenarioReduceArgs& a, int T, int sp, int sl, int Hs, double* sc_red) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = a.N, K = a.K, M = a.M, H = a.H, KM = K * M, R = KM * H;
  double* rw = sc_red;                              // [K M][Hs] row rewards; entry 0 of a row becomes the member return
  float* pw = reinterpret_cast<float*>(reinterpret_cast<int*>(rw + KM * Hs + nth) + nth);  // [T][sp] a tile's powers
  float* ld = pw + T * sp;                                                                  // [T][sl] ... and load values
  const int slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  double wr0 = a.ws[(size_t)b * a.wind_stride];
  WF_IN_VGPR(wr0);  // (as the lay-out's parameters: no spilled scalar register)
  const double* __restrict__ ews = a.ews + (size_t)slot * R;
  const float* __restrict__ pblk = a.power_ev + (size_t)slot * R * N;
  const float* __restrict__ lblk = a.load_ev + (size_t)slot * R * 4 * N;
  double* const rewards = a.rewards ? a.rewards + (size_t)slot * R : nullptr;
  wf_staged_row_rewards(
      pblk, lblk, R, N, T, sp, sl, a.load_coef, pw, ld,
      [H, wr0, ews](int row) { return row % H == 0 ? wr0 : ews[row - 1]; },  // the speed BEFORE the step, of the row's member
      [H, Hs, rw, rewards](int row, double r, double) {
        const int km = row / H, h = row - km * H;
        rw[km * Hs + h] = r;
        if (rewards) rewards[row] = r;
      });
  int after = KM * Hs;  // (formed again, in a vector register, and not held in scalar ones across the tiles)
  WF_IN_VGPR(after);
  double* bv = rw + after;                     // [nth] a pass's sorted returns, then the argmax tree: scores ...
  int* bi = reinterpret_cast<int*>(bv + nth);  // [nth] ... and their sequences
  double gamma = a.gamma;
  WF_IN_VGPR(gamma);
  for (int km = tid; km < KM; km += nth) {
    double* r = rw + km * Hs;
    double g = 1.0, ret = 0.0;
    for (int h = 0; h < H; ++h) {
      ret += g * r[h];
      g = g * gamma;
    }
    r[0] = ret;
    if (a.member_returns) a.member_returns[(size_t)slot * KM + km] = ret;
  }
  __syncthreads();
  const size_t o0 = (size_t)slot * K;
  const WfBest best = wf_member_statistics(rw, Hs, K, M, a.q, a.lam, bv, [&a, o0](int k, double mean, double cvar, double score) {
    if (a.expected) a.expected[o0 + k] = mean;
    if (a.cvar) a.cvar[o0 + k] = cvar;
    if (a.score) a.score[o0 + k] = score;
  });
  wf_argmax_tree(best, bv, bi);
  if (tid == 0 && a.best) a.best[slot] = wf_argmax_winner(bi);
}

// Its launch: wf_returns_launch's choices with K M sequences — one wave for a few short rows, the odd stride where it fits in
// 36 KiB — with two differences, both because a slot has up to 4096 rows here and one workgroup takes them all.  A slot of
// many floats (R N >= WF_SCENARIO_WIDE) gets 1024 threads where that leaves the tile its 24 KiB: staging a tile is a chain of
// global loads per thread, and its time goes with their number.  And the tile takes what the rewards leave of 63 KiB, 24 KiB at
// the least: a tile's rows are added by a thread each, one dependent chain of 5 N additions, so that part goes with the NUMBER
// of tiles.  A kernel that instantiates the body is declared with __launch_bounds__(1024).
struct WfScenarioReduceLaunch {
  int threads, Hs;
  WfRewardTile t;
  size_t lds_bytes;
};
inline WfScenarioReduceLaunch wf_scenario_reduce_launch(int N, int K, int M, int H) {
  const int KM = K * M, R = KM * H;
  const int Hs = KM * (H | 1) <= 4608 ? (H | 1) : H;
  const auto head_of = [&](int threads) { return sizeof(double) * ((size_t)KM * Hs + threads) + sizeof(int) * threads; };
  const size_t room = 63 * 1024, least = 24 * 1024;
  int threads = R * N <= 512 ? 64 : 256;
  if (R * N >= WF_SCENARIO_WIDE && head_of(1024) + least <= room) threads = 1024;
  const size_t head = head_of(threads);
  const WfRewardTile t = wf_reward_tile(R, N, threads, (int)((room - head) / sizeof(float)));
  return WfScenarioReduceLaunch{threads, Hs, t, head + t.lds_bytes};
}
