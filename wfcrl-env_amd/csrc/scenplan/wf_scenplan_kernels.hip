// wf_scenplan_kernels.hip — the kernels around the step kernel that make the scenario planner run on the device
// (include/wfscenplan.h: the cross-entropy method over action sequences, every candidate scored over an ensemble of wind
// futures).  The farm solve is the existing wf_step on the object's evaluator handle; these kernels are the glue, so that a
// whole run — the ensemble's draws included — is enqueued without a host read:
//
//   wf_scenplan_paths_kernel    once per chunk, ONE WORKGROUP PER SLOT.  The M member paths of the slot's farm, two [M][Hs]
//     arrays of doubles in LDS, Hs = H | 1, in ONE tile: K >= 3 and K M H <= 4096 leave M H <= 1365 (the scenario lay-out's
//     several-tiles branch, M H > 2048, cannot be reached here).  Every thread draws the deviates of its (member, tick) pairs,
//     streams 17 and 18; thread m < M draws its ramp rate, stream 16, and walks member m's recursion in place; after the
//     barrier the threads fill every row's evaluator wind, thread r on row r, and wind_paths, consecutive lanes on consecutive
//     (speed, direction) pairs.  The rows' wind is the same in every iteration: it is written here and nowhere else.
//   wf_scenplan_advance_kernel  I + 1 launches per chunk, ONE WORKGROUP PER SLOT.  Launch v
//     REDUCES iteration v - 1 (v > 0).  The slot's R = K M H rows go by in LDS tiles (wf_staged_row_rewards,
//       ext/wf_ext_kernels.h) and leave their rewards in LDS ([K M][Hs] doubles); thread (k, m) forms its member return in
//       ascending h and leaves it in its row's first double.  The statistics run in PASSES of nth / M whole candidates, as
//       wf_scenario_reduce_kernel's: thread (k, m) counts its rank over the M members of its candidate — (return, m)
//       ascending — and scatters its return to sorted[k][rank] (a pass's [nth] doubles); thread k adds the mean in ascending m
//       and the tail in ascending rank, forms the score, leaves it in the candidate's FIRST entry (member 0's return has been
//       added by then: no [K] array of its own, K reaches 4096 when M = H = 1) and keeps its argmax.  A fixed-order tree over the
//       threads follows.  Then wf_plan_advance_kernel's update over the K scores: thread k counts rank_k (a broadcast read per
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
// KNOWN SECOND COPIES: the path walk and the member statistics restate scenario/wf_scenario_kernels.hip's, the
// candidate draw and the update plan/wf_plan_kernels.hip's; those files are left as they were.
#include <hip/hip_runtime.h>

#include <climits>

#include "../ext/wf_deviate.h"
#include "../wf_philox.h"
#include "wf_scenplan.h"

#define WF_SCENPLAN_WIDE 8192  // floats of power per slot (R N) from which the advance kernel runs 1024 threads
#define WF_SCENPLAN_IN_VGPR(v) asm volatile("" : "+v"(v))  // the value is held in a vector register from here on

__global__ __launch_bounds__(256) void wf_scenplan_paths_kernel(const WfScenPlanPathsArgs a, int Hs) {
  extern __shared__ double sp_tile[];
  const int tid = threadIdx.x, nth = blockDim.x;
  const int M = a.M, H = a.H, MH = M * H, R = a.K * MH;
  double* sp = sp_tile;      // [M][Hs] deviates of stream 17, then the stored speeds
  double* dr = sp + M * Hs;  // [M][Hs] ... of stream 18, then the stored directions
  const int slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  const bool writes = slot < a.sl.n_slots;
  const size_t in = writes ? slot : 0;  // the slot's input block
  double Sc = a.ws[(size_t)b * a.wind_stride], Dc = a.wd[(size_t)b * a.wind_stride];
  WF_SCENPLAN_IN_VGPR(Sc); WF_SCENPLAN_IN_VGPR(Dc);
  double Sa = a.anchor ? a.anchor[in * 2] : Sc, Da = a.anchor ? a.anchor[in * 2 + 1] : Dc;
  // the walk's parameters live in vector registers, as wf_scenario_layout_kernel's: block-uniform values held in scalar ones
  // across the Philox rounds of the draws would not fit
  double ws_revert = a.ws_revert, ws_sigma = a.ws_sigma, wd_revert = a.wd_revert, wd_sigma = a.wd_sigma;
  double ws_lo = a.ws_lo, ws_hi = a.ws_hi;
  WF_SCENPLAN_IN_VGPR(Sa); WF_SCENPLAN_IN_VGPR(Da);
  WF_SCENPLAN_IN_VGPR(ws_revert); WF_SCENPLAN_IN_VGPR(ws_sigma); WF_SCENPLAN_IN_VGPR(wd_revert); WF_SCENPLAN_IN_VGPR(wd_sigma);
  WF_SCENPLAN_IN_VGPR(ws_lo); WF_SCENPLAN_IN_VGPR(ws_hi);
  const unsigned long long hi = (unsigned long long)b << 32;
  for (int i = tid; i < MH; i += nth) {
    const int m = i / H, j = i - m * H;
    const unsigned long long ctr = hi | (unsigned)(m * 64 + j);
    sp[m * Hs + j] = wf_deviate(a.seed, ctr, 17u);
    dr[m * Hs + j] = wf_deviate(a.seed, ctr, 18u);
  }
  __syncthreads();
  for (int m = tid; m < M; m += nth) {  // the walkers: thread m keeps member m's state (M <= 64 <= nth: one trip)
    unsigned r[4];
    philox4x32_10(a.seed, hi | (unsigned)m, 16u, r);
    const double rate = a.wd_ramp * (2.0 * u01(r[0], r[1]) - 1.0);
    double x = Sc, y = Dc;
    double* s = sp + m * Hs;
    double* d = dr + m * Hs;
    for (int j = 0; j < H; ++j) {
      x = (x + ws_revert * (Sa - x)) + ws_sigma * s[j];
      const double mu = Da + rate * (double)(j + 1);
      y = (y + wd_revert * (mu - y)) + wd_sigma * d[j];
      double w = fmod(y, 360.0);
      if (w < 0.0) w += 360.0;
      s[j] = fmin(fmax(x, ws_lo), ws_hi);
      d[j] = w;
    }
  }
  __syncthreads();
  double* __restrict__ ews = a.ews + (size_t)slot * R;
  double* __restrict__ ewd = a.ewd + (size_t)slot * R;
  for (int r = tid; r < R; r += nth) {
    const int km = r / H, h = r - km * H, m = km % M;
    ews[r] = sp[m * Hs + h];
    ewd[r] = dr[m * Hs + h];
  }
  if (writes && a.wind_paths) {
    double* __restrict__ paths = a.wind_paths + in * MH * 2;
    for (int i = tid; i < MH; i += nth) {
      const int m = i / H, j = i - m * H;
      paths[2 * i] = sp[m * Hs + j];
      paths[2 * i + 1] = dr[m * Hs + j];
    }
  }
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
    WF_SCENPLAN_IN_VGPR(gamma);
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
  {
    const int spp = nth / M;  // whole candidates per pass (M <= 64 <= nth)
    const int kk = tid / M, m = tid - kk * M;
    const int q = a.q;
    double lam = a.lam;
    WF_SCENPLAN_IN_VGPR(lam);
    double* const stat = last ? a.stat + (size_t)slot * K * 2 : nullptr;
    double best_v = -HUGE_VAL;
    int best_k = INT_MAX;
    for (int k0 = 0; k0 < K; k0 += spp) {  // (block-uniform)
      const bool member = kk < spp && k0 + kk < K;
      double rv = 0.0;
      int rank = 0;
      if (member) {
        const double* s = rw + (size_t)(k0 + kk) * Ks;
        rv = s[m * Hs];
        for (int j = 0; j < M; ++j) {
          const double vj = s[j * Hs];
          rank += (vj < rv) || (vj == rv && j < m);
        }
      }
      __syncthreads();  // (the previous pass's tails have been added)
      if (member) bv[kk * M + rank] = rv;
      __syncthreads();
      if (tid < spp && k0 + tid < K) {
        const int k = k0 + tid;
        double* s = rw + (size_t)k * Ks;
        double sum = 0.0, tail = 0.0;
        for (int j = 0; j < M; ++j) sum += s[j * Hs];
        for (int j = 0; j < q; ++j) tail += bv[tid * M + j];
        const double mean = sum / (double)M, cvar = tail / (double)q;
        const double score = ((1.0 - lam) * mean) + (lam * cvar);
        if (stat) { stat[2 * k] = mean; stat[2 * k + 1] = cvar; }
        s[0] = score;  // (member 0's return has been added, and ranked before the barriers: the entry is the candidate's score from here on)
        if (score > best_v || (score == best_v && k < best_k)) { best_v = score; best_k = k; }
      }
    }
    __syncthreads();  // (the last pass's tails have been added: bv becomes the tree)
    bv[tid] = best_v;
    bi[tid] = best_k;
  }
  __syncthreads();
  for (int s = nth >> 1; s > 0; s >>= 1) {  // (block-uniform)
    if (tid < s) {
      const double x = bv[tid + s];
      const int k = bi[tid + s];
      if (x > bv[tid] || (x == bv[tid] && k < bi[tid])) { bv[tid] = x; bi[tid] = k; }
    }
    __syncthreads();
  }
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
  const int w = bi[0] == INT_MAX ? 0 : bi[0];
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
  WF_SCENPLAN_IN_VGPR(vv); WF_SCENPLAN_IN_VGPR(Iv); WF_SCENPLAN_IN_VGPR(sg);
  WF_SCENPLAN_IN_VGPR(o_bv); WF_SCENPLAN_IN_VGPR(o_bi); WF_SCENPLAN_IN_VGPR(o_el);
  double* const bv = reinterpret_cast<double*>(lds + o_bv);
  int* const bi = reinterpret_cast<int*>(lds + o_bi);
  if (v > 0)  // (block-uniform)
    wf_scenplan_reduce(*run, sl_, vv, vv == Iv, L.T, L.sp, L.sl, L.Hs, spl_lds, bv, bi, reinterpret_cast<float*>(lds + L.pw),
                       reinterpret_cast<float*>(lds + L.ld), reinterpret_cast<unsigned char*>(lds + o_el));
  else
    wf_scenplan_seed(*run, sl_);
  __syncthreads();  // (mean and best sequence in global memory: other threads of the block read them below)
  if (vv < Iv) wf_scenplan_layout(*run, sl_, vv, sg);  // (no barrier below this line)
  else wf_scenplan_outputs(*run, sl_, bv[0], bi[0] == INT_MAX ? 0 : bi[0]);
}

extern "C" hipError_t wfk_launch_scenplan_paths(const WfScenPlanPathsArgs* a, hipStream_t s) {
  const int MH = a->M * a->H;
  if (MH > 2048) return hipErrorInvalidValue;  // (one tile: K >= 3 keeps M H <= 1365)
  const int threads = a->K * MH <= 128 ? 64 : 256;
  const int Hs = a->H | 1;
  hipLaunchKernelGGL(wf_scenplan_paths_kernel, dim3(a->sl.C), dim3(threads), sizeof(double) * 2 * (size_t)a->M * Hs, s, *a, Hs);
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
