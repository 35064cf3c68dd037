// wf_retgrad_kernels.hip — the kernels around the step kernel that make the gradient of look-ahead returns with respect to
// the action sequences run on the device (include/wfretgrad.h).  The farm solve is the existing wf_step on the object's
// evaluator handle; these three kernels are the glue, so that a whole run is enqueued without a host read:
//
//   wf_retgrad_layout_kernel  once per chunk, ONE WORKGROUP PER SLOT.  Thread (k, i), i fastest, keeps the yaw, the
//                             accumulator and the move counter of turbine i in registers and walks sequence k's steps
//                             h = 0 .. H - 1 with the env's transition (wf_env_transition, ext/wf_ext_kernels.h), as
//                             wf_lookahead_layout_kernel does.  Per step it forms the two pass flags and the perturbed yaws
//                             y+ / y- (include/wfgrad.h's arithmetic: float64, rounded once, one-sided at a bound), writes the
//                             divisor, the flags and the trajectory — consecutive lanes on consecutive entries — and then the
//                             step's W = 2 N + 1 rows in a loop over the rows: row j of the step gets y at entry i, except
//                             y+ in row 2 i + 1 and y- in row 2 i + 2, so every store of the loop is coalesced along the
//                             turbine index and no entry is written twice.  Every row's wind: the caller's wind of step h,
//                             or the parent's device wind held.
//   wf_retgrad_reduce_kernel  once per chunk, after the step, ONE WORKGROUP PER (SLOT, SEQUENCE), at least a thread per
//                             turbine.  It steps through h DESCENDING; a step's W rows go by in LDS tiles
//                             (wf_staged_row_rewards, ext/wf_ext_kernels.h, unchanged: odd row strides, float64 sums in the
//                             stated orders) and leave their W rewards in LDS — one step's only, never H W —; the base row's
//                             reward and farm power stay in 2 [H] doubles beside the [H] discounts and the [H] normalisers.  Thread i then forms q, lam (a register)
//                             and the two gradient entries, consecutive threads on consecutive doubles.  After the sweep
//                             thread 0 forms the return in ascending h, as wf_sequence_returns does.
//   wf_retgrad_best_kernel    once per chunk when `best` is asked for: a thread per slot walks the farm's K returns in
//                             ascending k — the larger return, among equal ones the lower index.  A third kernel rather
//                             than a last-block pass in the reduce kernel: no counter, no fence, no order to argue about.
//
// The row normalisers: step 0's is the parent's (the pending prev-wind speed, else the current speed), step h >= 1's the
// speed of base row (k, h - 1), read from the evaluator's wind block; the +- rows of a step take the base row's.  LDS per
// block: (W + 4 H) doubles and the tile, 60 KiB together at most.  Trip counts are run-time values: no private segment, no spill
// (tests/test_retgrad.py reads the metadata); every barrier sits in block-uniform control flow.  The library is built with
// -ffp-contract=off: the transition's float32 sums, the sweep's product and sum and the return's stay single roundings, as in
// the step kernels and the NumPy restatement.
#include <hip/hip_runtime.h>

#include "wf_retgrad.h"

__global__ __launch_bounds__(256) void wf_retgrad_layout_kernel(const WfRetgradLayoutArgs a) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = a.N, K = a.K, H = a.H, W = 2 * N + 1, R = K * H * W;
  const int slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  const bool writes = slot < a.sl.n_slots;
  const size_t in = writes ? slot : 0;  // the slot's input block
  const size_t st0 = (size_t)b * N;     // ... and its farm's env state
  const double ws0 = a.ws[(size_t)b * a.wind_stride], wd0 = a.wd[(size_t)b * a.wind_stride];
  const double* __restrict__ wind = a.wind ? a.wind + in * H * 2 : nullptr;
  for (int r = tid; r < R; r += nth) {
    const int h = (r / W) % H;
    a.ews[(size_t)slot * R + r] = wind ? wind[2 * h] : ws0;
    a.ewd[(size_t)slot * R + r] = wind ? wind[2 * h + 1] : wd0;
  }
  const int moves0 = a.env.moves[b];
  const size_t seq = (size_t)K * H * N;  // entries of a slot's [K][H][N] blocks
  const float* __restrict__ act = a.actions + in * seq;
  float* __restrict__ out = a.yaw + (size_t)slot * R * N;
  double* __restrict__ div = a.div + (size_t)slot * seq;
  unsigned char* __restrict__ flags = a.flags + (size_t)slot * seq;
  float* const traj = writes && a.traj ? a.traj + in * seq : nullptr;
  unsigned char* const pass_mask = writes && a.pass_mask ? a.pass_mask + in * seq : nullptr;
  const double lo = (double)a.env.lo, hi = (double)a.env.hi, delta = a.delta;
  const int n_traj = K * N;
  for (int q = tid; q < n_traj; q += nth) {
    const int k = q / N, i = q - k * N;
    float y = a.env.yaw[st0 + i], acc = a.env.acc[st0 + i];
    size_t o = (size_t)k * H * N + i;
    for (int h = 0; h < H; ++h, o += N) {
      const float raw = act[o];
      const bool open = !wf_env_gate_closed(a.env, acc, moves0 + 1 + h);
      float da;
      const float yn = wf_env_transition(a.env, y, raw, acc, moves0 + 1 + h, da);
      const bool t = yn == y + da;         // the clip to [lo, hi] returned its input
      const bool s = open && da == raw && t;  // ... and so did the gate and the clip to +-step
      acc += fabsf(da);
      y = yn;
      // include/wfgrad.h's perturbation
      const double yd = (double)y;
      const float yp = (float)fmin(yd + delta, hi), ym = (float)fmax(yd - delta, lo);
      div[o] = (double)yp - (double)ym;
      const unsigned char f = (unsigned char)((s ? 1 : 0) | (t ? 2 : 0));
      flags[o] = f;
      if (traj) traj[o] = y;
      if (pass_mask) pass_mask[o] = f;
      float* __restrict__ row = out + (size_t)(k * H + h) * W * N + i;
      const int jp = 2 * i + 1;
      for (int j = 0; j < W; ++j, row += N) *row = j == jp ? yp : (j == jp + 1 ? ym : y);
    }
    if (writes && a.final_yaw) a.final_yaw[in * n_traj + q] = y;
  }
}

// `T`, `sp`, `sl`: the tile of wf_staged_row_rewards.  Dynamic LDS: [W] + 4 [H] doubles, then the tile's floats.
__global__ __launch_bounds__(1024) void wf_retgrad_reduce_kernel(const WfRetgradReduceArgs a, int T, int sp, int sl) {
  extern __shared__ double rg_red[];
  const int tid = threadIdx.x;
  const int N = a.N, K = a.K, H = a.H, W = 2 * N + 1, R = K * H * W;
  double* rr = rg_red;                           // [W] one step's row rewards
  double* rb = rr + W;                           // [H] the base rows' rewards ...
  double* fp = rb + H;                           // [H] ... and farm powers
  double* g = fp + H;                            // [H] the discounts
  double* wn = g + H;                            // [H] the steps' normalising speeds
  float* pw = reinterpret_cast<float*>(wn + H);  // [T][sp] a tile's powers
  float* ld = pw + T * sp;                       // [T][sl] ... and load values
  const int slot = blockIdx.x / K, k = blockIdx.x - slot * K;
  const size_t sk = (size_t)slot * K + k;  // the sequence within the chunk
  const bool mine = tid < N;
  double lam = mine && a.terminal ? a.terminal[sk * N + tid] : 0.0;
  {
    const int b = wf_slot_farm(a.sl, slot);
    const double wr0 = a.ws_prev ? a.ws_prev[b] : a.ws[(size_t)b * a.wind_stride];
    const double* __restrict__ ews = a.ews + (size_t)slot * R;
    // the speed BEFORE step h, for all W rows of the step: step 0's is the parent's, step h's base row (k, h - 1)'s
    for (int h = tid; h < H; h += blockDim.x) wn[h] = h == 0 ? wr0 : ews[(k * H + h - 1) * W];
    if (tid == 0) {
      const double gamma = a.gamma;
      double v = 1.0;
#pragma unroll 1
      for (int h = 0; h < H; ++h) {
        g[h] = v;
        v = v * gamma;
      }
    }
  }
  __syncthreads();
  const float* __restrict__ pblk = a.power_ev + (size_t)slot * R * N;
  const float* __restrict__ lblk = a.load_ev + (size_t)slot * R * 4 * N;
  // thread i's entries of step H - 1 in the [C][K][H][N] blocks: per-thread pointers that step back by N
  const size_t o_last = (sk * H + (H - 1)) * N + (mine ? tid : 0);
  const double* divp = a.div + o_last;
  const unsigned char* flagp = a.flags + o_last;
  double* rgp = a.reward_gradient ? a.reward_gradient + o_last : nullptr;
  double* agp = a.action_gradient ? a.action_gradient + o_last : nullptr;
  // ... and where the thread writes after the sweep: its state-gradient entry, entry `tid` of the sequence's rewards and
  // farm powers, thread 0 the return (per-thread pointers: nothing of these waits in scalar registers through the sweep)
  double* const sgp = a.state_gradient ? a.state_gradient + sk * N + tid : nullptr;
  double* const rwp = a.rewards ? a.rewards + sk * H + tid : nullptr;
  double* const fpp = a.farm_power ? a.farm_power + sk * H + tid : nullptr;
  double* const revp = a.returns_ev + sk + tid;
  double* const retp = a.returns ? a.returns + sk + tid : nullptr;
  for (int h = H - 1; h >= 0; --h) {  // (block-uniform)
    const int row0 = (k * H + h) * W;
    const double wr = wn[h];
    wf_staged_row_rewards(
        pblk + (size_t)row0 * N, lblk + (size_t)row0 * 4 * N, W, N, T, sp, sl, a.load_coef, pw, ld, [wr](int) { return wr; },
        [h, rr, rb, fp](int row, double r, double psum) {
          rr[row] = r;
          if (row == 0) {
            rb[h] = r;
            fp[h] = psum;
          }
        });
    // (the call's last barrier has passed: rr is complete; the next step's rows reach rr only after its first barrier)
    if (mine) {
      const double d = *divp;
      const double q = d > 0.0 ? (rr[2 * tid + 1] - rr[2 * tid + 2]) / d : 0.0;
      const unsigned f = *flagp;
      lam = g[h] * q + lam;
      if (rgp) *rgp = q;
      if (agp) *agp = (f & 1u) ? lam : 0.0;
      lam = (f & 2u) ? lam : 0.0;
      divp -= N; flagp -= N;
      if (rgp) rgp -= N;
      if (agp) agp -= N;
    }
  }
  // (rb, fp: written by thread 0 — row 0 of a step is the first tile's first row — before the last step's last barrier)
  int t2 = tid;
  asm volatile("" : "+v"(t2));  // (the conditions below are formed here, not kept as lane masks in scalar registers through the sweep)
  if (t2 < N && sgp) *sgp = lam;
  if (t2 < H) {  // (H <= 64 <= the block's threads)
    if (rwp) *rwp = rb[t2];
    if (fpp) *fpp = fp[t2];
  }
  if (t2 == 0) {
    double ret = 0.0;
    int h = 0;
#pragma unroll 1
    do ret += g[h] * rb[h];  // (H >= 1)
    while (++h < H);
    *revp = ret;
    if (retp) *retp = ret;
  }
}

__global__ __launch_bounds__(64) void wf_retgrad_best_kernel(const WfRetgradBestArgs a) {
  const int slot = blockIdx.x * 64 + threadIdx.x;
  if (slot >= a.n_slots) return;
  const double* __restrict__ r = a.returns_ev + (size_t)slot * a.K;
  double best_v = -HUGE_VAL;
  int best_k = INT_MAX;
  for (int k = 0; k < a.K; ++k) {
    const double v = r[k];
    if (v > best_v || (v == best_v && k < best_k)) { best_v = v; best_k = k; }
  }
  a.best[slot] = best_k == INT_MAX ? 0 : best_k;
}

extern "C" hipError_t wfk_launch_retgrad_layout(const WfRetgradLayoutArgs* a, hipStream_t s) {
  const int threads = a->K * a->N <= 64 ? 64 : 256;  // a few short sequences of a small farm: one wave
  hipLaunchKernelGGL(wf_retgrad_layout_kernel, dim3(a->sl.C), dim3(threads), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_retgrad_reduce(const WfRetgradReduceArgs* a, hipStream_t s) {
  const int N = a->N, W = 2 * N + 1;
  // a thread per turbine at the least (lam is a register); one wave where a step's rows are few and short, sixteen where a
  // step's powers and loads are 128 KiB and more: staging them is a chain of global loads per thread, shorter with more threads
  const int threads = W * N <= 512 ? 64 : (5 * W * N >= 32768 ? 1024 : (N <= 256 ? 256 : (N + 63) / 64 * 64));
  // the block's LDS stays below 60 KiB: the [W] + 4 [H] doubles, the rest the tile (a row per summing thread: the larger the
  // tile, the more rows of a step are summed at once)
  const size_t own = sizeof(double) * ((size_t)W + 4 * (size_t)a->H);
  const WfRewardTile t = wf_reward_tile(W, N, threads, (int)((61440 - own) / sizeof(float)));
  const size_t lds = own + t.lds_bytes;
  hipLaunchKernelGGL(wf_retgrad_reduce_kernel, dim3(a->sl.n_slots * a->K), dim3(threads), lds, s, *a, t.T, t.sp, t.sl);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_retgrad_best(const WfRetgradBestArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(wf_retgrad_best_kernel, dim3((a->n_slots + 63) / 64), dim3(64), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_retgrad_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[WF_RETGRAD_KERNELS] = {(const void*)wf_retgrad_layout_kernel, (const void*)wf_retgrad_reduce_kernel,
                                        (const void*)wf_retgrad_best_kernel};
  if (kernel < 0 || kernel >= WF_RETGRAD_KERNELS) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, fn[kernel]);
}
