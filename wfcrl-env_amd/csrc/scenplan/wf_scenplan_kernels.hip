// wf_scenplan_kernels.hip — the kernels around the step kernel that make the scenario planner run on the device
// (include/wfscenplan.h: the cross-entropy method over action sequences, every candidate scored over an ensemble of wind
// futures).  The farm solve is the existing wf_step on the object's evaluator handle; these kernels are the glue, so that a
// whole run — the ensemble's draws included — is enqueued without a host read:
//
//   wf_scenplan_paths_kernel    once per chunk, ONE WORKGROUP PER SLOT.  The M member paths of the slot's farm, every row's
//     evaluator wind and wind_paths: the ensemble's tiled body (ensemble/wf_ensemble.h: wf_ensemble_tiles) with ONE tile of
//     H ticks, Hs = H | 1 — K >= 3 and K M H <= 4096 leave M H <= 1365, and the launcher refuses M H > 2048.  The rows' wind
//     is the same in every iteration: it is written here and nowhere else.
//   wf_scenplan_advance_kernel  I + 1 launches per chunk, ONE WORKGROUP PER SLOT.  Launch v
//     REDUCES iteration v - 1 (v > 0).  The slot's R = K M H rows go by in LDS tiles (wf_staged_row_rewards,
//       ext/wf_ext_kernels.h) and leave their rewards in LDS ([K M][Hs] doubles); thread (k, m) forms its member return in
//       ascending h and leaves it in its row's first double.  The statistics and the choice are the ensemble's
//       (wf_member_statistics over the returns at stride Hs, then wf_argmax_tree); what they emit here is (mean, tail mean) in
//       the last launch, and the score into the candidate's FIRST entry (member 0's return has been added by then: no [K]
//       array of its own, K reaches 4096 when M = H = 1).  Then wf_plan_advance_kernel's update over the K scores: thread k counts rank_k (a broadcast read per
//       j) and flags the elites; thread e of the [H][N] elements adds the elites' actions in ascending k in float64, divides
//       once by E and stores the mean, and copies the winner's action where the winner is not candidate 0.  In the LAST
//       launch the member returns and every candidate's (mean, tail mean) also go to the slot's blocks in global memory: the
//       outputs read the winner's.
//     LAYS OUT iteration v (v < I).  Thread (k, t), t fastest, keeps the yaw and the accumulator of turbine t in registers and
//       walks candidate k's H steps: the action is the best sequence's (k = 0), the mean's (k = 1) or the mean plus sigma
//       times a deviate of its own Philox counter (k >= 2); it goes to the candidates' buffer and through the env's
//       transition, the yaw to the M member rows of step h: consecutive lanes on consecutive floats.  Launch 0 seeds mean
//       and best sequence first.
//     WRITES THE OUTPUTS instead (v = I), thread e on element e; final_yaw by a walk of the plan.
//
// LDS per block stays below 64 KiB: 36 KiB of rewards at most ([K M][H | 1] where that fits, else [K M][H]), 3 KiB — 12 KiB with
// 1024 threads — for the passes and the argmax, and the tile and the K elite flags (a byte each, 4 KiB at most) share what is
// left of 63 KiB, 24 KiB at the least.  A slot of R N >= 8192 floats of power runs 1024 threads where that leaves the tile its
// 24 KiB, as wf_scenario_reduce_kernel: measured on HornsRev1 x 256, K = 16, M = 8, H = 8, I = 3, the glue is 12.1 ms with 256
// threads and a 24 KiB tile, 9.8 ms with the larger tile and 5.0 ms with 1024 threads too.  Trip counts are
// run-time values: no private segment, no spill (tests/test_scenplan.py reads the metadata); every barrier sits in
// block-uniform control flow — the branches around them test kernel arguments only.  The library is built with
// -ffp-contract=off: every product and sum is one rounding.
//
// KNOWN SECOND COPY: the candidate draw and the update restate plan/wf_plan_kernels.hip's; that file is left as
// it was.
#include <hip/hip_runtime.h>

#include "../ext/wf_deviate.h"
#include "../wf_philox.h"
#include "wf_scenplan.h"

#define WF_SCENPLAN_WIDE 8192  // floats of power per slot (R N) from which the advance kernel runs 1024 threads

__global__ __launch_bounds__(256) void wf_scenplan_paths_kernel(const WfScenPlanPathsArgs a, int Hs) {
  extern __shared__ double sp_tile[];
  wf_ensemble_tiles(a.ens, a.sl, a.K, a.ens.H, Hs, sp_tile, a.ews, a.ewd, a.wind_paths);  // (one tile: Ht = H)
}

// The phases below read the run's block (WfScenPlanRun, device memory) and name the slot's blocks themselves, where they use
// them: what a phase holds in scalar registers dies with it (the staged row rewards take nearly all of them).

// reduce iteration v - 1: rw [K M][Hs], bv / bi [nth], pw / ld the tile, el [K]; leaves the winner's score in bv[0], the winner in bi[0]
__device__ __forceinline__ void wf_scenplan_reduce(const WfScenPlanRun& a, const WfSlots& sl_, int v, bool last, int T, int sp, int sl, int Hs,
                                                   double* rw, double* bv, int* bi, float* pw, float* ld, unsigned char* el) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  const int N = a.N, K = a.K, M = a.M, H = a.H, KM = K * M, R = KM * H;
  {
    const int b = wf_slot_farm(sl_, slot);
    const double wr0 = a.ws[(size_t)b * a.wind_stride];  // the CURRENT speed: a pending prev-wind speed is not read
    const double* __restrict__ ews = a.ews + (size_t)slot * R;
    wf_staged_row_rewards(
        a.power_ev + (size_t)slot * R * N, a.load_ev + (size_t)slot * R * 4 * N, R, N, T, sp, sl, a.load_coef, pw, ld,
        [H, wr0, ews](int row) { return row % H == 0 ? wr0 : ews[row - 1]; },  // the speed BEFORE the step, of the row's member
        [H, Hs, rw](int row, double r, double) {
          const int km = row / H, h = row - km * H;
          rw[km * Hs + h] = r;
        });
  }
  {
    double gamma = a.gamma;
    WF_IN_VGPR(gamma);
    double* const mret = last ? a.mret + (size_t)slot * KM : nullptr;
    for (int km = tid; km < KM; km += nth) {
      double* r = rw + km * Hs;
      double g = 1.0, ret = 0.0;
      for (int h = 0; h < H; ++h) {
        ret += g * r[h];
        g = g * gamma;
      }
      r[0] = ret;  // (the row is this thread's own)
      if (mret) mret[km] = ret;
    }
  }
  __syncthreads();
  const int Ks = M * Hs;  // doubles from a candidate's first entry to the next candidate's
  double* const stat = last ? a.stat + (size_t)slot * K * 2 : nullptr;
  const WfBest top = wf_member_statistics(rw, Hs, K, M, a.q, a.lam, bv, [rw, Ks, stat](int k, double mean, double cvar, double score) {
    if (stat) { stat[2 * k] = mean; stat[2 * k + 1] = cvar; }
    rw[(size_t)k * Ks] = score;  // (the candidate's first entry is its score from here on)
  });
  wf_argmax_tree(top, bv, bi);
  const int E = a.E;
  for (int k = tid; k < K; k += nth) {
    const double rk = rw[(size_t)k * Ks];
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const double rj = rw[(size_t)j * Ks];
      rank += (rj > rk) || (rj == rk && j < k);
    }
    el[k] = rank < E;
  }
  __syncthreads();
  const int w = wf_argmax_winner(bi);
  const int HN = H * N;
  const float* cand = a.cand + (size_t)slot * K * HN;
  float* const best = a.best + (size_t)slot * HN;
  float* const mu = a.mu + (size_t)slot * HN;
  const double n_el = (double)E;
  for (int e = tid; e < HN; e += nth) {
    double s = 0.0;
    for (int k = 0; k < K; ++k)
      if (el[k]) s += (double)cand[(size_t)k * HN + e];
    mu[e] = (float)(s / n_el);
    if (w) best[e] = cand[(size_t)w * HN + e];
  }
  if (tid == 0 && v == 1 && a.hold_score && (unsigned)slot < (unsigned)sl_.n_slots) a.hold_score[sl_.base + slot] = rw[0];
}

// launch 0: the mean, and the hold as the best sequence so far
__device__ __forceinline__ void wf_scenplan_seed(const WfScenPlanRun& a, const WfSlots& sl_) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  const int HN = a.H * a.N;
  const size_t in = sl_.base + (slot < sl_.n_slots ? slot : 0);  // the slot's rows of the caller's arrays
  float* const best = a.best + (size_t)slot * HN;
  float* const mu = a.mu + (size_t)slot * HN;
  for (int e = tid; e < HN; e += nth) {
    mu[e] = a.mean0 ? a.mean0[in * HN + e] : 0.0f;
    best[e] = 0.0f;
  }
}

// lay out iteration v: candidates, trajectories, the M member rows of every step
__device__ __forceinline__ void wf_scenplan_layout(const WfScenPlanRun& a, const WfSlots& sl_, int v, double sigma) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  const int N = a.N, K = a.K, M = a.M, H = a.H, HN = H * N;
  const int b = wf_slot_farm(sl_, slot);
  const size_t st0 = (size_t)b * N;  // the farm's env state
  const int moves0 = a.env.moves[b];
  const float* const best = a.best + (size_t)slot * HN;
  const float* const mu = a.mu + (size_t)slot * HN;
  float* __restrict__ cand = a.cand + (size_t)slot * K * HN;
  float* __restrict__ out = a.yaw + (size_t)slot * K * M * HN;
  const double lim = (double)a.env.step;
  const unsigned long long hi = (unsigned long long)(unsigned)b << 32;
  const int n_traj = K * N;
  for (int q = tid; q < n_traj; q += nth) {
    const int k = q / N, t = q - k * N;
    float y = a.env.yaw[st0 + t], acc = a.env.acc[st0 + t];
    size_t o = (size_t)k * HN + t;         // the candidate's element of step h: the draw's counter
    size_t orow = (size_t)k * M * HN + t;  // row (k, 0, h)
    for (int h = 0, e = t; h < H; ++h, e += N, o += N, orow += N) {
      float act;
      if (k == 0) {
        act = best[e];
      } else {
        act = mu[e];
        if (k >= 2) {
          unsigned r[4];
          philox4x32_10(a.seed, hi | (unsigned)o, (unsigned)v, r);
          const double z = wf_deviate_of(r);
          double c = (double)act + sigma * z;
          c = c < -lim ? -lim : c;
          c = c > lim ? lim : c;
          act = (float)c;
        }
      }
      cand[o] = act;
      float da;
      y = wf_env_transition(a.env, y, act, acc, moves0 + 1 + h, da);
      acc += fabsf(da);
      size_t om = orow;
      for (int m = 0; m < M; ++m, om += HN) out[om] = y;
    }
  }
}

// the last launch: the outputs; the winner of the last iteration is candidate w, its score plan_score
__device__ __forceinline__ void wf_scenplan_outputs(const WfScenPlanRun& a, const WfSlots& sl_, double plan_score, int w) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  if (slot >= sl_.n_slots) return;
  const int N = a.N, H = a.H, M = a.M, HN = H * N;
  const size_t in = sl_.base + slot;  // the slot's rows of the caller's arrays
  const float* const best = a.best + (size_t)slot * HN;
  const float* const mu = a.mu + (size_t)slot * HN;
  for (int e = tid; e < HN; e += nth) {
    const float bs = best[e];
    if (a.plan) a.plan[in * HN + e] = bs;
    if (a.mean) a.mean[in * HN + e] = mu[e];
    if (a.first_action && e < N) a.first_action[in * N + e] = bs;
  }
  if (tid == 0) {
    const double* st = a.stat + ((size_t)slot * a.K + w) * 2;
    if (a.plan_score) a.plan_score[in] = plan_score;
    if (a.plan_expected) a.plan_expected[in] = st[0];
    if (a.plan_cvar) a.plan_cvar[in] = st[1];
  }
  if (a.plan_member_returns) {
    const double* mr = a.mret + ((size_t)slot * a.K + w) * M;
    for (int m = tid; m < M; m += nth) a.plan_member_returns[in * M + m] = mr[m];
  }
  if (a.final_yaw) {  // the yaw after walking the plan
    const int b = wf_slot_farm(sl_, slot);
    const size_t st0 = (size_t)b * N;
    const int moves0 = a.env.moves[b];
    for (int t = tid; t < N; t += nth) {
      float y = a.env.yaw[st0 + t], acc = a.env.acc[st0 + t];
      for (int h = 0; h < H; ++h) {
        float da;
        y = wf_env_transition(a.env, y, best[h * N + t], acc, moves0 + 1 + h, da);
        acc += fabsf(da);
      }
      a.final_yaw[in * N + t] = y;
    }
  }
}

// the block's LDS, carved by the launcher (byte offsets: kernel arguments, not values the kernel computes and then holds)
struct WfScenPlanLds {
  int Hs;             // rw [K M][Hs] doubles at 0: row rewards; [k m][0] becomes the member return, [k 0][0] then candidate k's score
  int bv, bi;         // [threads] doubles, [threads] ints: a pass's sorted returns, then the argmax tree's scores and their candidates
  int T, sp, sl;      // the tile (wf_reward_tile) ...
  int pw, ld;         // ... [T][sp] powers and [T][sl] load values
  int el;             // [K] bytes, 1 = elite
};

__global__ __launch_bounds__(1024) void wf_scenplan_advance_kernel(const WfScenPlanRun* __restrict__ run, const WfSlots sl_, int v, int I,
                                                                  double sigma, const WfScenPlanLds L) {
  extern __shared__ double spl_lds[];
  char* const lds = reinterpret_cast<char*>(spl_lds);
  // what only the phases after the tiles use is held in vector registers: in scalar ones, across the staged row rewards, it
  // does not fit (a spilled scalar register; tests/test_scenplan.py reads the metadata).  Block-uniform all the same
  int vv = v, Iv = I, o_bv = L.bv, o_bi = L.bi, o_el = L.el;
  double sg = sigma;
  WF_IN_VGPR(vv); WF_IN_VGPR(Iv); WF_IN_VGPR(sg);
  WF_IN_VGPR(o_bv); WF_IN_VGPR(o_bi); WF_IN_VGPR(o_el);
  double* const bv = reinterpret_cast<double*>(lds + o_bv);
  int* const bi = reinterpret_cast<int*>(lds + o_bi);
  if (v > 0)  // (block-uniform)
    wf_scenplan_reduce(*run, sl_, vv, vv == Iv, L.T, L.sp, L.sl, L.Hs, spl_lds, bv, bi, reinterpret_cast<float*>(lds + L.pw),
                       reinterpret_cast<float*>(lds + L.ld), reinterpret_cast<unsigned char*>(lds + o_el));
  else
    wf_scenplan_seed(*run, sl_);
  __syncthreads();  // (mean and best sequence in global memory: other threads of the block read them below)
  if (vv < Iv) wf_scenplan_layout(*run, sl_, vv, sg);  // (no barrier below this line)
  else wf_scenplan_outputs(*run, sl_, bv[0], wf_argmax_winner(bi));
}

extern "C" hipError_t wfk_launch_scenplan_paths(const WfScenPlanPathsArgs* a, hipStream_t s) {
  const int MH = a->ens.M * a->ens.H;
  if (MH > WF_ENSEMBLE_TILE) return hipErrorInvalidValue;  // (one tile: K >= 3 keeps M H <= 1365)
  const int threads = a->K * MH <= 128 ? 64 : 256;
  const int Hs = a->ens.H | 1;
  hipLaunchKernelGGL(wf_scenplan_paths_kernel, dim3(a->sl.C), dim3(threads), sizeof(double) * 2 * (size_t)a->ens.M * Hs, s, *a, Hs);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_scenplan_advance(const WfScenPlanRun* host, const WfScenPlanRun* dev, const WfSlots* sl, int v, double sigma,
                                                  hipStream_t s) {
  // wf_scenario_reduce_kernel's choices: one wave for a few short rows; a slot of many floats (R N >= WF_SCENPLAN_WIDE) gets 1024
  // threads where that leaves the tile its 24 KiB; the tile and the K elite flags take what the rewards leave of 63 KiB
  const int N = host->N, K = host->K, KM = K * host->M, H = host->H, R = KM * H;
  const int Hs = KM * (H | 1) <= 4608 ? (H | 1) : H;  // the odd stride where [K M][H | 1] doubles fit in 36 KiB
  const auto head_of = [&](int threads) { return sizeof(double) * ((size_t)KM * Hs + threads) + sizeof(int) * threads; };
  const size_t room = 63 * 1024, least = 24 * 1024;
  int threads = R * N <= 512 ? 64 : 256;
  if (R * N >= WF_SCENPLAN_WIDE && head_of(1024) + least <= room) threads = 1024;
  const size_t head = head_of(threads);
  const int flags = (K + 15) & ~15;  // the elite flags come out of the tile's share
  const WfRewardTile t = wf_reward_tile(R, N, threads, (int)((room - head - flags) / sizeof(float)));
  WfScenPlanLds L{};
  L.Hs = Hs;
  L.T = t.T; L.sp = t.sp; L.sl = t.sl;
  L.bv = (int)sizeof(double) * KM * L.Hs;
  L.bi = L.bv + (int)sizeof(double) * threads;
  L.pw = L.bi + (int)sizeof(int) * threads;
  L.ld = L.pw + (int)sizeof(float) * t.T * t.sp;
  L.el = L.pw + (int)t.lds_bytes;
  hipLaunchKernelGGL(wf_scenplan_advance_kernel, dim3(sl->C), dim3(threads), (size_t)(L.el + flags), s, dev, *sl, v, host->I, sigma, L);
  return hipGetLastError();
}
extern "C" hipError_t wfk_scenplan_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[WF_SCENPLAN_KERNELS] = {(const void*)wf_scenplan_paths_kernel, (const void*)wf_scenplan_advance_kernel};
  if (kernel < 0 || kernel >= WF_SCENPLAN_KERNELS) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, fn[kernel]);
}
