// wf_ext_kernels.h — the device side the extensions share (yawopt/, robust/, rose/, grad/, credit/, lookahead/, plan/, rollout/, retgrad/): which farm a
// chunk's slot works on, a visit's candidate grid, the visit order of a slot's turbines, the phases the two searches' advance
// kernels have in common, the fused env's transition, the staged row rewards of credit, lookahead, rollout and retgrad, the returns of K sequences
// (lookahead, rollout), and the staged row sum of the rose and the robust search.  The per-extension headers build their kernels'
// argument structs from these; wf_ext.h is the host side.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "../wf_f64_math.h"

// The value is held in a vector register from here on.  For block-uniform values that, held in scalar registers across a
// register-hungry stretch (the Philox rounds of a draw, the staged row rewards), would not fit: spilled scalar registers.
#define WF_IN_VGPR(v) asm volatile("" : "+v"(v))

// which farm a slot works on: farms[base + s] (or base + s without a list), s = slot for the chunk's own slots, 0 beyond
struct WfSlots {
  const int* farms;  // device copy of the caller's list, or null
  int base;          // first entry of the chunk in the list
  int n_slots;       // farms of this chunk (<= C)
  int C;             // slots of the evaluator
};

// One visit's candidate grid: value of candidate j (0-based) around the incumbent `inc` (include/wfyawopt.h)
//   mode 0 (pass 0)   a + j b                 a = lo, b = h_0
//   mode 1 (refine)   (inc - a) + (j + 1) b   a = h_{p-1}, b = 2 h_{p-1} / (K_p + 1)
// clipped to [lo, hi] in float64, rounded once to float32.
struct WfGrid {
  int s;     // position in the visit order, -1 = no such visit
  int mode, K;
  double a, b;
};

// the order kernels' arguments (WfYawoptOrderArgs and WfRobustOrderArgs derive from it: the kernels keep their names)
struct WfOrderArgs {
  WfSlots sl;
  const double *lx, *ly;  // [N] layout, caller's order
  double xc, yc;          // centre of rotation [A.1-1]
  const double* wd;       // the parent's wind directions (the nominal ones)
  int wind_stride;        // 0 shared, 1 per farm
  int N;
  int* order;             // [C][N]: caller index of the s-th turbine a slot visits
};

#define WF_ORDER_MAX_N 256

// the limits of a search (include/wfyawopt.h and include/wfrobust.h name them once each; their *_abi.hip assert they agree)
#define WF_SEARCH_MAX_PASSES 4
#define WF_SEARCH_MAX_K0 31
#define WF_SEARCH_MAX_K 15
#define WF_SEARCH_ROWS_MAX 32  // K_0 <= 31 candidates + the incumbent

// What the two advance kernels share (WfYawoptAdvanceArgs and WfRobustAdvanceArgs derive from it): the host driver
// (wf_ext.h: run_search) fills it per chunk and per visit, the extension adds where the previous visit's powers are.
struct WfAdvanceArgs {
  WfSlots sl;
  int N, R;
  double lo, hi;
  WfGrid prev, next;  // the visit whose powers are in (prev.s < 0: none, initialise from yaw0) / the one to lay out
  int first;                // prev is the run's first visit: its incumbent's power is power_init
  const int* order;         // [C][N]
  float* yaw;               // the evaluator's input for next: [C][R][N], or [C][R][M][N] under M members
  float* best;              // [C][N] best (nominal) yaw so far
  const float* yaw0;        // [n_slots][N] rows of this chunk, or null = zeros
  float *out_yaw, *out_power, *out_init;  // rows of this chunk: [n_slots][N], [n_slots], [n_slots]; written when next.s < 0 / first
};

__device__ __forceinline__ int wf_slot_farm(const WfSlots& sl, int slot) {
  const int s = sl.base + (slot < sl.n_slots ? slot : 0);
  return sl.farms ? sl.farms[s] : s;
}

// candidate j of a visit's grid around `inc`.  The library is built with -ffp-contract=off: a product and a sum stay two
// roundings, as in the NumPy restatement.
__device__ __forceinline__ float wf_grid_candidate(const WfGrid& g, double inc, int j, double lo, double hi) {
  double c = g.mode == 0 ? g.a + (double)j * g.b : (inc - g.a) + (double)(j + 1) * g.b;
  c = c < lo ? lo : c;
  c = c > hi ? hi : c;
  return (float)c;
}

// Each slot's visit order, upstream to downstream: the float64 rotation and stable rank sort of wf_geometry_kernel /
// wf_probe_state_kernel.  One workgroup per slot, one thread per turbine; sx is the block's __shared__ double[WF_ORDER_MAX_N].
__device__ __forceinline__ void wf_visit_order(const WfOrderArgs& a, double* sx) {
  const int N = a.N, t = threadIdx.x, slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  // wd % 360, rotation about the bounding-box centre [A.1]: the arithmetic of wf_geometry_kernel
  double wdm = fmod(a.wd[(size_t)b * a.wind_stride], 360.0);
  if (wdm < 0.0) wdm += 360.0;
  double dev = fmod(wdm - 270.0, 360.0);
  if (dev < 0.0) dev += 360.0;
  dev = fmod(dev + 360.0, 360.0);
  double ca, sa;
  sincos_any(dev * (M_PI / 180.0), sa, ca);
  double xr = 0.0;
  if (t < N) {
    const double xo = a.lx[t] - a.xc, yo = a.ly[t] - a.yc;
    xr = xo * ca - yo * sa + a.xc;
    sx[t] = xr;
  }
  __syncthreads();
  if (t < N) {
    int rank = 0;
    for (int u = 0; u < N; ++u) {
      const double xu = sx[u];
      rank += (xu < xr) || (xu == xr && u < t);
    }
    a.order[(size_t)slot * N + rank] = t;
  }
}

// ---- the phases of an advance kernel (wf_yawopt_advance_kernel, wf_robust_advance_kernel): ONE WAVE PER SLOT, `lane` its
// lane; sums[WF_SEARCH_ROWS_MAX], cnd[WF_SEARCH_ROWS_MAX] and brow[N] are the wave's own LDS.  `live` (the slot exists) is
// wave-uniform and is tested INSIDE the phases that hold a barrier: every wave of the block calls them. ----

// the slot's best yaw -> brow: seeded from yaw0 (or zeros) and stored before the first visit, loaded afterwards.  No barrier.
__device__ __forceinline__ void wf_advance_load_best(const WfAdvanceArgs& a, int slot, int lane, float* brow) {
  const int N = a.N;
  const size_t row0 = (size_t)slot * N;
  if (a.prev.s < 0) {
    const size_t src = (size_t)(slot < a.sl.n_slots ? slot : 0) * N;
    for (int t = lane; t < N; t += 64) {
      const float v = a.yaw0 ? a.yaw0[src + t] : 0.0f;
      brow[t] = v;
      a.best[row0 + t] = v;
    }
  } else {
    for (int t = lane; t < N; t += 64) brow[t] = a.best[row0 + t];
  }
}

// The winner of the previous visit from sums[0 .. prev.K] (every lane finds it: K + 1 LDS broadcasts), the writes of best /
// out_init / out_power, and the hand-over of the winner into brow between two barriers.  The caller's barrier after sums[]
// comes first.
__device__ __forceinline__ void wf_advance_pick(const WfAdvanceArgs& a, int slot, int lane, bool live, const double* sums, float* brow) {
  const bool has_prev = a.prev.s >= 0, writes = live && slot < a.sl.n_slots;
  const size_t row0 = (size_t)slot * a.N;
  int tp = 0;
  float newval = 0.0f;
  if (live && has_prev) {
    tp = a.order[row0 + a.prev.s];
    const double p_inc = sums[0];
    double p_best = p_inc;
    int w = 0;
    for (int k = 1; k <= a.prev.K; ++k) {
      const double pk = sums[k];
      if (pk > p_best) { p_best = pk; w = k; }  // strictly greater: the incumbent, then the lowest index, keep a tie
    }
    const float inc = brow[tp];
    newval = w ? wf_grid_candidate(a.prev, (double)inc, w - 1, a.lo, a.hi) : inc;
    if (lane == 0) {
      if (w) a.best[row0 + tp] = newval;
      if (writes && a.first) a.out_init[slot] = (float)p_inc;
      if (writes && a.next.s < 0) a.out_power[slot] = (float)p_best;
    }
  }
  __syncthreads();  // (every lane has read brow[tp])
  if (live && has_prev && lane == 0) brow[tp] = newval;
  __syncthreads();
}

// the next visit's candidates -> cnd; returns the turbine they replace.  The caller's barrier follows.
__device__ __forceinline__ int wf_advance_candidates(const WfAdvanceArgs& a, int slot, int lane, bool live, const float* brow, float* cnd) {
  if (!live || a.next.s < 0) return 0;
  const int tn = a.order[(size_t)slot * a.N + a.next.s];
  if (lane < a.next.K) cnd[lane] = wf_grid_candidate(a.next, (double)brow[tn], lane, a.lo, a.hi);
  return tn;
}

// after the last visit: the slot's best yaw is the answer
__device__ __forceinline__ void wf_advance_write_best(const WfAdvanceArgs& a, int slot, int lane, const float* brow) {
  for (int t = lane; t < a.N; t += 64) a.out_yaw[(size_t)slot * a.N + t] = brow[t];
}

// ---- the fused env as the kernels of credit/ and lookahead/ see it: parameters by value, state by (read-only) pointer ----
struct WfEnvView {
  const float *yaw, *acc;  // [B][N], or null: no env state
  const int* moves;        // [B]
  float lo, hi, step, rate, dt, budget;
  int discrete;
};

// The fused env step's transition (wf_kernels.hip: "fused MDP transition"), the same float32 operations in the same order;
// nothing is written back.  Returns the new yaw; `da` is the increment the accumulator grows by (|da|).
// the budget gate of that transition: closed when the accumulated actuation per move and second has reached the budget
__device__ __forceinline__ bool wf_env_gate_closed(const WfEnvView& e, float acc, int moves_new) {
  const float frac = __fdiv_rn(__fdiv_rn(__fdiv_rn(acc, e.rate), (float)moves_new), e.dt);
  return frac >= e.budget;
}
__device__ __forceinline__ float wf_env_transition(const WfEnvView& e, float y, float a, float acc, int moves_new, float& da) {
  if (wf_env_gate_closed(e, acc, moves_new)) a = 0.0f;  // the gate zeroes the RAW action: "down" in the discrete encoding (the reference's quirk)
  if (e.discrete) a = (a - 1.0f) * e.step;
  if (!e.discrete) a = fminf(fmaxf(a, -e.step), e.step);
  da = a;
  return fminf(fmaxf(y + a, e.lo), e.hi);
}

// ---- the staged row rewards (wf_credit_reduce_kernel, wf_lookahead_reduce_kernel): ONE WORKGROUP PER SLOT, every thread of
// the block calls it.  The slot's R rows go by in TILES of T rows: a tile's [T][N] powers and [T][4 N] load values are
// contiguous at pblk / lblk and are staged in pw [T][sp] / ld [T][sl] with coalesced loads (odd row strides: no bank conflict
// when a lane walks a row, as wf_staged_rowsum below).  Then thread k < T adds row k in float64 — the powers in caller order,
// the absolute load values in memory order — and hands the row's reward and farm power to keep(row, reward, psum), which
// leaves them in the kernel's [R] doubles in LDS (or, consecutive threads being on consecutive rows, in the caller's array).
// wr_of(row) is the speed the row's reward is normalised by.  After the last tile's barrier what `keep` stored is visible
// to the block.  Every barrier sits in block-uniform control flow. ----
template <class WR, class KEEP>
__device__ __forceinline__ void wf_staged_row_rewards(const float* __restrict__ pblk, const float* __restrict__ lblk, int R, int N, int T,
                                                      int sp, int sl, float load_coef, float* pw, float* ld, WR wr_of, KEEP keep) {
  const int tid = threadIdx.x, nth = blockDim.x, N4 = 4 * N;
  for (int r0 = 0; r0 < R; r0 += T) {  // (block-uniform)
    int nt = R - r0;
    nt = nt > T ? T : nt;
    const float* __restrict__ psrc = pblk + (size_t)r0 * N;
    const int n_p = nt * N;
    for (int q = tid; q < n_p; q += nth) {
      const int r = q / N, t = q - r * N;
      pw[r * sp + t] = psrc[q];
    }
    const float* __restrict__ lsrc = lblk + (size_t)r0 * N4;
    const int n_l = nt * N4;
    for (int q = tid; q < n_l; q += nth) {
      const int r = q / N4, t = q - r * N4;
      ld[r * sl + t] = lsrc[q];
    }
    __syncthreads();
    if (tid < nt) {
      const float* prow = pw + tid * sp;
      const float* lrow = ld + tid * sl;
      double psum = 0.0, lsum = 0.0;
      for (int t = 0; t < N; ++t) psum += (double)prow[t];
      for (int t = 0; t < N4; ++t) lsum += fabs((double)lrow[t]);
      const double wr = wr_of(r0 + tid);
      // wf_resolve.hip: res_outputs — psum / n / 1e6 * 1e3 / wr^3 - load_coef lsum / (4 n)
      keep(r0 + tid, psum / N / 1.0e6 * 1.0e3 / (wr * wr * wr) - (double)load_coef * lsum / (4.0 * N), psum);
    }
    __syncthreads();  // (the next tile overwrites pw / ld; after the last one what `keep` left in LDS is complete)
  }
}

// its launch: the odd row strides and T, the rows per tile — [T][sp] + [T][sl] floats in 24 KiB of LDS, at most a row per
// thread —, and the tile's LDS bytes (the kernel's [R] arrays of doubles come first and are the kernel's to add).  A kernel
// that keeps more in LDS beside the tile gives it fewer `floats` (wf_plan_advance_kernel: its elite flags come out of these)
struct WfRewardTile {
  int T, sp, sl;
  size_t lds_bytes;
};
inline WfRewardTile wf_reward_tile(int R, int N, int threads, int floats = 6144) {
  const int sp = N | 1, sl = (4 * N) | 1;
  int T = floats / (sp + sl);
  T = T < 1 ? 1 : T;
  T = T > R ? R : T;
  T = T > threads ? threads : T;
  return WfRewardTile{T, sp, sl, sizeof(float) * (size_t)T * (sp + sl)};
}

// ---- the returns of K sequences of H rows (wf_lookahead_reduce_kernel, wf_rollout_reduce_kernel: both are this body, and
// WfLookaheadReduceArgs / WfRolloutReduceArgs derive from these arguments): ONE WORKGROUP PER SLOT.  The slot's R = K H rows
// go by in the tiles above; the thread of a tile's row leaves the row's reward in LDS ([K][Hs] doubles, Hs = H | 1 where that
// fits: no bank conflict when thread k walks sequence k) and writes rewards / farm_power, consecutive threads on consecutive
// doubles.  After the last tile's barrier thread k forms sequence k's discounted return in ascending h; the argmax is a
// fixed-order reduction: every thread over its own k ascending, then a tree over the threads in LDS, the larger return and
// among equal ones the lower index.  The row normalisers: step 0's is the parent's (the pending prev-wind speed, else the
// current speed), step h >= 1's the speed of row (k, h - 1), read from the evaluator's wind block. ----
struct WfReturnsReduceArgs {
  WfSlots sl;
  int N, K, H;
  const double* ws;       // the parent's wind speed ...
  int wind_stride;
  const double* ws_prev;  // ... or [B] the speed the next env step normalises by (null: the current one): step 0's
  const double* ews;      // [C R] every row's wind speed: row (k, h - 1)'s normalises step h >= 1
  float load_coef;
  double gamma;
  const float* power_ev;  // [C][R][N] the evaluator's outputs
  const float* load_ev;   // [C][R][N][4]
  double* returns;        // rows of this chunk [n_slots][K], or null
  double* rewards;        // [n_slots][R], or null
  double* farm_power;     // [n_slots][R], or null
  int* best;              // [n_slots], or null
};

// `red` is the block's dynamic LDS: [K][Hs] + [nth] doubles, [nth] ints, then the tile's [T][sp] + [T][sl] floats
__device__ __forceinline__ void wf_sequence_returns(const WfReturnsReduceArgs& a, int T, int sp, int sl, int Hs, double* red) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = a.N, K = a.K, H = a.H, R = K * H;
  double* rw = red;                                 // [K][Hs] row rewards
  double* bv = rw + K * Hs;                         // [nth] the argmax tree: returns ...
  int* bi = reinterpret_cast<int*>(bv + nth);       // [nth] ... and their sequences
  float* pw = reinterpret_cast<float*>(bi + nth);   // [T][sp] a tile's powers
  float* ld = pw + T * sp;                          // [T][sl] ... and load values
  const int slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  const double wr0 = a.ws_prev ? a.ws_prev[b] : a.ws[(size_t)b * a.wind_stride];
  const double* __restrict__ ews = a.ews + (size_t)slot * R;
  const float* __restrict__ pblk = a.power_ev + (size_t)slot * R * N;
  const float* __restrict__ lblk = a.load_ev + (size_t)slot * R * 4 * N;
  double* const rewards = a.rewards ? a.rewards + (size_t)slot * R : nullptr;
  double* const farm_power = a.farm_power ? a.farm_power + (size_t)slot * R : nullptr;
  wf_staged_row_rewards(
      pblk, lblk, R, N, T, sp, sl, a.load_coef, pw, ld,
      [H, wr0, ews](int row) { return row % H == 0 ? wr0 : ews[row - 1]; },  // the speed BEFORE the step
      [H, Hs, rw, rewards, farm_power](int row, double r, double psum) {
        const int k = row / H, h = row - k * H;
        rw[k * Hs + h] = r;
        if (rewards) rewards[row] = r;
        if (farm_power) farm_power[row] = psum;
      });
  const double gamma = a.gamma;
  double best_v = -HUGE_VAL;
  int best_k = INT_MAX;
  for (int k = tid; k < K; k += nth) {
    const double* r = rw + k * Hs;
    double g = 1.0, ret = 0.0;
    for (int h = 0; h < H; ++h) {
      ret += g * r[h];
      g = g * gamma;
    }
    if (a.returns) a.returns[(size_t)slot * K + k] = ret;
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
  if (tid == 0 && a.best) a.best[slot] = bi[0] == INT_MAX ? 0 : bi[0];
}

// its launch: one wave for a few short rows, the odd stride where [K][H | 1] doubles fit in 36 KiB, the tile, the LDS bytes
struct WfReturnsLaunch {
  int threads, Hs;
  WfRewardTile t;
  size_t lds_bytes;
};
inline WfReturnsLaunch wf_returns_launch(int N, int K, int H) {
  const int R = K * H;
  const int threads = R * N <= 512 ? 64 : 256;
  const int Hs = K * (H | 1) <= 4608 ? (H | 1) : H;
  const WfRewardTile t = wf_reward_tile(R, N, threads);
  return WfReturnsLaunch{threads, Hs, t, sizeof(double) * ((size_t)K * Hs + threads) + sizeof(int) * threads + t.lds_bytes};
}

// ---- the staged row sum (wf_rose_rowsum_kernel, wf_robust_rowsum_kernel): a block of ONE wave stages the N float32 powers of
// its `nr` rows (<= 64, contiguous at src) in LDS with coalesced loads — consecutive lanes on consecutive floats; odd row
// stride: no bank conflict — then lane k adds row k in turbine order in float64.  Returns lane k's sum (0 for k >= nr). ----
__device__ __forceinline__ double wf_staged_rowsum(const float* __restrict__ src, int nr, int N, int stride, float* pw, int lane) {
  const int n_load = nr * N;
  for (int i = lane; i < n_load; i += 64) {
    const int r = i / N, t = i - r * N;
    pw[r * stride + t] = src[i];
  }
  __syncthreads();
  double sum = 0.0;
  if (lane < nr) {
    const float* row = pw + lane * stride;
    for (int t = 0; t < N; ++t) sum += (double)row[t];
  }
  return sum;
}

// its launch: rows per block — what fits in 32 KiB of LDS, at most a row per lane —, the odd row stride and the LDS bytes
struct WfRowsumLaunch {
  int rows_per_block, stride, blocks;
  size_t lds_bytes;
};
inline WfRowsumLaunch wf_rowsum_launch(int n_rows, int N) {
  const int stride = N | 1;
  int rpb = 32768 / (4 * stride);
  rpb = rpb < 1 ? 1 : (rpb > 64 ? 64 : rpb);
  return WfRowsumLaunch{rpb, stride, (n_rows + rpb - 1) / rpb, sizeof(float) * rpb * stride};
}
