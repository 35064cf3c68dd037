// wf_plan_kernels.hip — the one kernel around the step kernel that makes the receding-horizon planner run on the device
// (include/wfplan.h: the cross-entropy method over action sequences).  The farm solve is the existing wf_step on the object's
// evaluator handle; this kernel is the glue between two steps, so that a whole run is enqueued without a host read:
//
//   wf_plan_advance_kernel  I + 1 launches per chunk, ONE WORKGROUP PER SLOT.  Launch v
//     REDUCES iteration v - 1 (v > 0).  The slot's R = K H rows go by in LDS tiles (wf_staged_row_rewards, ext/wf_ext_kernels.h)
//       and leave their rewards in LDS ([K][Hs] doubles, the lookahead reduce's stride); thread k forms candidate k's
//       discounted return in ascending h and leaves it in its row's first double; the winner is the lookahead reduce's
//       fixed-order argmax: every thread over its own k ascending, then a tree over the threads in LDS; thread k counts
//       rank_k over the K returns in LDS (a broadcast read per j) and flags the elites; thread e of the [H][N] elements adds
//       the elites' actions in ascending k in float64, divides once by E and stores the mean, and copies the winner's
//       action where the winner is not candidate 0 — mean and best sequence live in global memory from launch to launch.
//     LAYS OUT iteration v (v < I).  Thread (k, t), t fastest, keeps the yaw and the accumulator of turbine t in registers and
//       walks candidate k's H steps: the action is the best sequence's (k = 0), the mean's (k = 1) or the mean plus sigma
//       times a deviate of its own Philox counter (k >= 2, wf_philox.h); it goes to the candidates' buffer and through the
//       env's transition (wf_env_transition), the yaw to row (k, h) — consecutive lanes on consecutive floats on every side.
//       Launch 0 seeds mean and best sequence first, and writes every row's wind: it is the same in every iteration.
//     WRITES THE OUTPUTS instead (v = I), thread e on element e: whole lines; final_yaw by a walk of the plan.
//
// LDS per block stays below 64 KiB with the lookahead reduce's accounting: 36 KiB of rewards at most, 3 KiB of argmax, and
// 24 KiB shared by the tile and the K elite flags (a byte each, 4 KiB at most: the tile is given that much less).  Trip counts
// are run-time values: no private segment, no spill (tests/test_plan.py reads the metadata); every barrier sits in
// block-uniform control flow — the branches around them test kernel arguments only.  The library is built with
// -ffp-contract=off: the candidate's product and sum, the transition's float32 sums and the return's product and sum stay
// single roundings, as in the NumPy restatement.
#include <hip/hip_runtime.h>

#include <climits>

#include "../ext/wf_deviate.h"
#include "../wf_philox.h"
#include "wf_plan.h"

// The phases below read the run's block (WfPlanRun, device memory) and name the slot's blocks themselves, where they use
// them: what a phase holds in scalar registers dies with it (the staged row rewards take nearly all of them).

// reduce iteration v - 1: rw [K][Hs], bv / bi [nth], pw / ld the tile, el [K]; leaves the winner's return in bv[0]
__device__ __forceinline__ void wf_plan_reduce(const WfPlanRun& a, const WfSlots& sl_, int v, int T, int sp, int sl, int Hs, double* rw,
                                               double* bv, int* bi, float* pw, float* ld, unsigned char* el) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  const int N = a.N, K = a.K, H = a.H, R = K * H;
  {
    const int b = wf_slot_farm(sl_, slot);
    const double wr0 = a.ws_prev ? a.ws_prev[b] : a.ws[(size_t)b * a.wind_stride];
    const double* __restrict__ ews = a.ews + (size_t)slot * R;
    wf_staged_row_rewards(
        a.power_ev + (size_t)slot * R * N, a.load_ev + (size_t)slot * R * 4 * N, R, N, T, sp, sl, a.load_coef, pw, ld,
        [H, wr0, ews](int row) { return row % H == 0 ? wr0 : ews[row - 1]; },  // the speed BEFORE the step
        [H, Hs, rw](int row, double r, double) {
          const int k = row / H, h = row - k * H;
          rw[k * Hs + h] = r;
        });
  }
  const double gamma = a.gamma;
  double best_v = -HUGE_VAL;
  int best_k = INT_MAX;
  for (int k = tid; k < K; k += nth) {
    double* r = rw + k * Hs;
    double g = 1.0, ret = 0.0;
    for (int h = 0; h < H; ++h) {
      ret += g * r[h];
      g = g * gamma;
    }
    r[0] = ret;  // (the row is this thread's own)
    if (ret > best_v || (ret == best_v && k < best_k)) { best_v = ret; best_k = k; }
  }
  bv[tid] = best_v;
  bi[tid] = best_k;
  __syncthreads();
  for (int s = nth >> 1; s > 0; s >>= 1) {  // (block-uniform)
    if (tid < s) {
      const double v = bv[tid + s];
      const int k = bi[tid + s];
      if (v > bv[tid] || (v == bv[tid] && k < bi[tid])) { bv[tid] = v; bi[tid] = k; }
    }
    __syncthreads();
  }
  const int E = a.E;
  for (int k = tid; k < K; k += nth) {
    const double rk = rw[k * Hs];
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const double rj = rw[j * Hs];
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
  // (an unsigned comparison of its own: the mask wf_slot_farm compared for above would be held across the tiles, in two spilled SGPRs)
  if (tid == 0 && v == 1 && a.hold_return && (unsigned)slot < (unsigned)sl_.n_slots) a.hold_return[sl_.base + slot] = rw[0];
}

// launch 0: the mean, the hold as the best sequence so far, and every row's wind
__device__ __forceinline__ void wf_plan_seed(const WfPlanRun& a, const WfSlots& sl_) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  const int N = a.N, H = a.H, R = a.K * H, HN = H * N;
  const int b = wf_slot_farm(sl_, slot);
  const size_t in = sl_.base + (slot < sl_.n_slots ? slot : 0);  // the slot's rows of the caller's arrays
  float* const best = a.best + (size_t)slot * HN;
  float* const mu = a.mu + (size_t)slot * HN;
  for (int e = tid; e < HN; e += nth) {
    mu[e] = a.mean0 ? a.mean0[in * HN + e] : 0.0f;
    best[e] = 0.0f;
  }
  const double ws0 = a.ws[(size_t)b * a.wind_stride], wd0 = a.wd[(size_t)b * a.wind_stride];
  const double* __restrict__ wind = a.wind ? a.wind + in * H * 2 : nullptr;
  for (int r = tid; r < R; r += nth) {
    const int h = r % H;
    a.ews[(size_t)slot * R + r] = wind ? wind[2 * h] : ws0;
    a.ewd[(size_t)slot * R + r] = wind ? wind[2 * h + 1] : wd0;
  }
}

// lay out iteration v: candidates, trajectories, yaw rows
__device__ __forceinline__ void wf_plan_layout(const WfPlanRun& a, const WfSlots& sl_, int v, double sigma) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  const int N = a.N, K = a.K, H = a.H, HN = H * N;
  const int b = wf_slot_farm(sl_, slot);
  const size_t st0 = (size_t)b * N;  // the farm's env state
  const int moves0 = a.env.moves[b];
  const float* const best = a.best + (size_t)slot * HN;
  const float* const mu = a.mu + (size_t)slot * HN;
  float* __restrict__ cand = a.cand + (size_t)slot * K * HN;
  float* __restrict__ out = a.yaw + (size_t)slot * K * HN;
  const double lim = (double)a.env.step;
  const unsigned long long hi = (unsigned long long)(unsigned)b << 32;
  const int n_traj = K * N;
  for (int q = tid; q < n_traj; q += nth) {
    const int k = q / N, t = q - k * N;
    float y = a.env.yaw[st0 + t], acc = a.env.acc[st0 + t];
    size_t o = (size_t)k * HN + t;
    for (int h = 0, e = t; h < H; ++h, e += N, o += N) {
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
      out[o] = y;
    }
  }
}

// the last launch: the outputs, in whole lines; plan_return is the last winner's return
__device__ __forceinline__ void wf_plan_outputs(const WfPlanRun& a, const WfSlots& sl_, double plan_return) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  if (slot >= sl_.n_slots) return;
  const int N = a.N, H = a.H, HN = H * N;
  const size_t in = sl_.base + slot;  // the slot's rows of the caller's arrays
  const float* const best = a.best + (size_t)slot * HN;
  const float* const mu = a.mu + (size_t)slot * HN;
  for (int e = tid; e < HN; e += nth) {
    const float bs = best[e];
    if (a.plan) a.plan[in * HN + e] = bs;
    if (a.mean) a.mean[in * HN + e] = mu[e];
    if (a.first_action && e < N) a.first_action[in * N + e] = bs;
  }
  if (tid == 0 && a.plan_return) a.plan_return[in] = plan_return;
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
struct WfPlanLds {
  int Hs;             // rw [K][Hs] doubles at 0: row rewards; [k][0] becomes candidate k's return
  int bv, bi;         // [threads] doubles, [threads] ints: the argmax tree's returns and their candidates
  int T, sp, sl;      // the tile (wf_reward_tile) ...
  int pw, ld;         // ... [T][sp] powers and [T][sl] load values
  int el;             // [K] bytes, 1 = elite
};

__global__ __launch_bounds__(256) void wf_plan_advance_kernel(const WfPlanRun* __restrict__ run, const WfSlots sl_, int v, int I, double sigma,
                                                              const WfPlanLds L) {
  extern __shared__ double pl_lds[];
  char* const lds = reinterpret_cast<char*>(pl_lds);
  double* const bv = reinterpret_cast<double*>(lds + L.bv);
  if (v > 0)  // (block-uniform)
    wf_plan_reduce(*run, sl_, v, L.T, L.sp, L.sl, L.Hs, pl_lds, bv, reinterpret_cast<int*>(lds + L.bi), reinterpret_cast<float*>(lds + L.pw),
                   reinterpret_cast<float*>(lds + L.ld), reinterpret_cast<unsigned char*>(lds + L.el));
  else
    wf_plan_seed(*run, sl_);
  __syncthreads();  // (mean and best sequence in global memory: other threads of the block read them below)
  if (v < I) wf_plan_layout(*run, sl_, v, sigma);
  else wf_plan_outputs(*run, sl_, bv[0]);
}

extern "C" hipError_t wfk_launch_plan_advance(const WfPlanRun* host, const WfPlanRun* dev, const WfSlots* sl, int v, double sigma,
                                              hipStream_t s) {
  const int N = host->N, K = host->K, H = host->H, R = K * H;
  const int threads = R * N <= 512 ? 64 : 256;
  const int flags = (K + 15) & ~15;  // the elite flags come out of the tile's 24 KiB
  const WfRewardTile t = wf_reward_tile(R, N, threads, 6144 - flags / 4);
  WfPlanLds L{};
  L.Hs = K * (H | 1) <= 4608 ? (H | 1) : H;  // the odd stride where [K][H | 1] doubles fit in 36 KiB
  L.T = t.T; L.sp = t.sp; L.sl = t.sl;
  L.bv = (int)sizeof(double) * K * L.Hs;
  L.bi = L.bv + (int)sizeof(double) * threads;
  L.pw = L.bi + (int)sizeof(int) * threads;
  L.ld = L.pw + (int)sizeof(float) * t.T * t.sp;
  L.el = L.pw + (int)t.lds_bytes;
  hipLaunchKernelGGL(wf_plan_advance_kernel, dim3(sl->C), dim3(threads), (size_t)(L.el + flags), s, dev, *sl, v, host->I, sigma, L);
  return hipGetLastError();
}
extern "C" hipError_t wfk_plan_func_attributes(int kernel, hipFuncAttributes* a) {
  if (kernel != 0) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, (const void*)wf_plan_advance_kernel);
}
