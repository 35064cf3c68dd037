// wf_policy_kernels.hip — the kernels around the step kernel that make closed-loop rollouts of MLP policies run on the device
// (include/wfpolicy.h).  The farm solve is the existing wf_step on the object's evaluator handle, one batched step per env
// step; these kernels are the glue, so that a whole run is enqueued without a host read:
//
//   wf_policy_transpose_kernel  once per call: params [K][P] -> wt [K][P] with every weight block [out][in] turned to
//                               [in][out], so that the lanes of the advance kernel — consecutive output neurons — read
//                               consecutive floats.
//   wf_policy_begin_kernel      once per chunk, a thread per (row, turbine): the round-0 rows (the farm's current yaw), their
//                               wind, and the per-row state: accumulators, return 0, discount 1, gate count 0.
//   wf_policy_advance_kernel    H times per chunk, between two steps.  A WORKGROUP SERVES A TILE OF T SLOTS OF ONE POLICY
//                               (rows k C + s0 .. + T - 1: contiguous blocks), in order:
//                               1. from round 2 on: the reward of the step before from its power and load rows — the tile of
//                                  wf_staged_row_rewards (ext/wf_ext_kernels.h), the sums and the formula of the lookahead
//                                  extension's reduce —, added to the row's return, ret += g r, g = g gamma;
//                               2. the rows' observation — yaw, local wind speed, local wind direction, the wind they were solved
//                                  under — staged in LDS (odd row stride) with coalesced loads and written to `observations`;
//                               3. the network, activations in LDS as doubles: a pass holds MB instances (central: the tile's
//                                  rows; shared: turbines of the tile's rows, pass after pass).  A thread owns one output
//                                  neuron o of FOUR instances (g, g + G, g + 2 G, g + 3 G: G groups, so that the lanes of one
//                                  o-range read LDS rows an odd stride apart): it reads weight wt[i][o] once per input i,
//                                  ascending, and feeds four accumulators, z = z + w x, product and sum rounded separately.
//                                  Consecutive lanes read consecutive floats of wt; a policy's weights are streamed once per
//                                  workgroup pass, not once per row;
//                               4. the action of every (row, turbine) -> LDS, then the env's transition (wf_env_transition);
//                               5. the next yaw row, `actions`, the accumulators: consecutive lanes on consecutive floats
//                                  along the turbine index; under a wind per step the rows' next wind.
//   wf_policy_reduce_kernel     once per chunk, after the last step, a workgroup per tile of T slots, policy after policy:
//                               the last reward (the same tile), returns, final_yaw, gated; then thread s takes the argmax of
//                               slot s over k ascending from the returns kept in LDS: strictly greater wins, so the lowest
//                               index among equal maxima.
//
// UNDER AN ENSEMBLE of M wind futures (include/wfpolscen.h; polscen/ launches the transpose, begin and advance kernels of THIS
// file, so the five phases exist once) a policy has M C rows, row j = m C + slot, each solved under its member's path
// (WfPolicyRun: M, paths); wf_policy_run sets M = 1 and no paths: then j is the slot and every index below is what it was.
//
// No floating-point atomics (the gate count is an integer sum in LDS), no order that depends on scheduling.  Trip counts are
// run-time values and nothing is indexed by a run-time value in registers: no private segment at any N (tests/test_policy.py
// reads the metadata); every barrier sits in block-uniform control flow.  The library is built with -ffp-contract=off: the
// network's products and sums, the transition's float32 sums and the return's product and sum stay single roundings, as in the
// NumPy restatement (tests/policy_ref.py).
#include <hip/hip_runtime.h>

#include "wf_policy.h"

namespace {

__device__ __forceinline__ double policy_act(int kind, double z) {
  if (kind == WF_POLICY_RELU) return z > 0.0 ? z : 0.0;
  if (kind == WF_POLICY_SOFTSIGN) return z / (1.0 + fabs(z));
  if (kind == WF_POLICY_TANH) {
    const double c = fmin(fmax(z, -20.0), 20.0);
    return 1.0 - 2.0 / (exp_lean(2.0 * c) + 1.0);
  }
  return z;
}

// the speed step h >= 0 is solved under / the direction
__device__ __forceinline__ double wind_of(const double* wind, int h, int c, double held) { return wind ? wind[2 * h + c] : held; }

// the (speed, direction) rows [H][2] row (m, slot) is solved under: its member path of the chunk (an ensemble), else the
// caller's wind of the slot's block `in`, else null = the parent's wind held
__device__ __forceinline__ const double* policy_row_wind(const WfPolicyRun& a, size_t in, int slot, int m) {
  if (a.paths) return a.paths + ((size_t)slot * a.M + m) * a.H * 2;
  return a.wind ? a.wind + in * a.H * 2 : nullptr;
}

// The reward of step hp of a tile's nt rows (evaluator rows e0 .., rows s0 .. of their policy — slots, where M = 1): thread r leaves the speed row r is normalised
// by in wrl[r] — step 0's is the parent's (the pending prev-wind speed, else the current speed), step hp >= 1's the speed of
// wind hp - 1 —, then the tile of wf_staged_row_rewards; its hooks touch LDS only (what a hook holds in scalar registers stays
// live across the staged sums, which take nearly all of them).  Afterwards thread r < nt finds row r's reward in rwl[r] and its
// farm power in psl[r].  Every thread of the block calls it.
__device__ __forceinline__ void policy_tile_rewards(const WfPolicyRun& a, const WfSlots& sl_, size_t e0, int s0, int nt, int hp, int sp,
                                                    int sl, double* wrl, double* rwl, double* psl, float* pw, float* ld) {
  const int tid = threadIdx.x, N = a.N;
  if (tid < nt) {
    const int j = s0 + tid, m = j / sl_.C, slot = j - m * sl_.C, b = wf_slot_farm(sl_, slot);  // (M = 1: m = 0, slot = j)
    const size_t in = (size_t)sl_.base + (slot < sl_.n_slots ? slot : 0);
    const double held = a.ws[(size_t)b * a.wind_stride];
    double wr;
    if (hp == 0) wr = a.ws_prev ? a.ws_prev[b] : held;
    else wr = wind_of(policy_row_wind(a, in, slot, m), hp - 1, 0, held);
    wrl[tid] = wr;
  }
  wf_staged_row_rewards(
      a.power_ev + e0 * N, a.load_ev + e0 * 4 * N, nt, N, nt, sp, sl, a.load_coef, pw, ld, [wrl](int r) { return wrl[r]; },
      [rwl, psl](int r, double rew, double psum) {
        rwl[r] = rew;
        psl[r] = psum;
      });
}

}  // namespace

__global__ __launch_bounds__(256) void wf_policy_transpose_kernel(const WfPolicyRun* __restrict__ run) {
  const WfPolicyRun& a = *run;
  const int P = a.net.P;
  const size_t n = (size_t)a.K * P;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(q / P), j = (int)(q - (size_t)k * P);  // j: position in the TRANSPOSED vector
    int src = j;
    for (int l = 0; l < a.net.L; ++l) {
      const int nin = a.net.width[l], nout = a.net.width[l + 1], w0 = a.net.woff[l];
      if (j >= w0 && j < w0 + nin * nout) {
        const int i = (j - w0) / nout, o = (j - w0) - i * nout;
        src = w0 + o * nin + i;
      }
    }
    a.wt[q] = a.params[(size_t)k * P + src];
  }
}

__global__ __launch_bounds__(256) void wf_policy_begin_kernel(const WfPolicyRun* __restrict__ run, const WfSlots sl_) {
  const WfPolicyRun& a = *run;
  const int N = a.N, C = sl_.C;
  const size_t E = (size_t)a.K * a.M * C, n = E * N;  // (e = (k M + m) C + slot: e % C is the slot under an ensemble too)
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q / N;
    const int t = (int)(q - e * N), slot = (int)(e % C);
    const int b = wf_slot_farm(sl_, slot);
    a.yaw[q] = a.env.yaw[(size_t)b * N + t];
    a.st.acc[q] = a.env.acc[(size_t)b * N + t];
    if (t == 0) {
      a.ews[e] = a.ws[(size_t)b * a.wind_stride];
      a.ewd[e] = a.wd[(size_t)b * a.wind_stride];
      a.st.ret[e] = 0.0;
      a.st.disc[e] = 1.0;
      a.st.gated[e] = 0;
    }
  }
}

// (the run block is NOT declared __restrict__ in the two kernels below: a phase's stores then end the life of what an earlier
// phase read from it, where otherwise every field is fetched on entry and held in scalar registers across the staged sums)
__global__ __launch_bounds__(256) void wf_policy_advance_kernel(const WfPolicyRun* run, const WfSlots sl_, const int round) {
  extern __shared__ double po_lds[];
  const WfPolicyRun& a = *run;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int C = sl_.C, T = a.pl.T, R = a.M * C;          // R: the rows of one policy (M = 1: its slots)
  const int k = blockIdx.y, s0 = blockIdx.x * T;
  int nt = R - s0;
  nt = nt > T ? T : nt;                                  // rows of this tile (block-uniform)
  const size_t e0 = (size_t)k * R + s0;                  // its first evaluator row
  const int h = round - 1;                               // the step whose action this launch issues
  // the LDS: the reward tile first, so that phase 1 needs nothing of what the later phases hold
  double* const wrl = po_lds;                            // [T] the rows' normalisers, ...
  double* const rwl = wrl + T;                           // [T] ... rewards ...
  double* const psl = rwl + T;                           // [T] ... and farm powers of the step before
  float* const pw = reinterpret_cast<float*>(psl + T);   // [T][sp] the reward tile: powers ...

  // ---- 1. the reward of step h - 1, the row solved last ----
  if (h >= 1) {  // (block-uniform)
    const int sp = a.pl.sp, sl = a.pl.sl;
    policy_tile_rewards(a, sl_, e0, s0, nt, h - 1, sp, sl, wrl, rwl, psl, pw, pw + (size_t)T * sp);  // (... and load values [T][sl])
    if (tid < nt) {
      const size_t e = e0 + tid;
      const int j = s0 + tid, m = j / C, slot = j - m * C;
      const double g = a.st.disc[e];
      a.st.ret[e] = a.st.ret[e] + g * rwl[tid];
      a.st.disc[e] = g * a.gamma;
      if (slot < sl_.n_slots) {
        const size_t o = (((size_t)(sl_.base + slot) * a.K + k) * a.M + m) * a.H + (h - 1);
        if (a.rewards) a.rewards[o] = rwl[tid];
        if (a.farm_power) a.farm_power[o] = psl[tid];
      }
    }
  }

  // ---- 2. observation h of the tile's rows -> LDS and `observations` ----
  const int N = a.N, K = a.K, H = a.H, MB = a.pl.MB, xs = a.pl.xs, as = a.pl.as, ds = a.pl.ds;
  const int D0 = 3 * N + 2;
  double* const x0 = reinterpret_cast<double*>(pw + (((size_t)T * (a.pl.sp + a.pl.sl) + 1) & ~(size_t)1));  // [MB][xs] a pass's normalised inputs
  double* const bufA = x0 + (size_t)MB * xs;             // [MB][as] activations ...
  double* const bufB = bufA + (size_t)MB * as;           // [MB][as] ... of alternate layers
  float* const obs = reinterpret_cast<float*>(bufB + (size_t)MB * as);  // [T][ds] the rows' observations, un-normalised
  float* const actf = obs + (size_t)T * ds;              // [T][N] the rows' raw actions
  int* const ng = reinterpret_cast<int*>(actf + (size_t)T * N);  // [T] closed gates of this step
  if (tid < T) ng[tid] = 0;
  for (int q = tid; q < nt * D0; q += nth) {
    const int r = q / D0, i = q - r * D0;
    const size_t e = e0 + r;
    float v;
    if (i < N) v = a.yaw[e * N + i];
    else if (i < 2 * N) v = a.lws[e * N + (i - N)];
    else if (i < 3 * N) v = a.lwd[e * N + (i - 2 * N)];
    else v = (float)(i == 3 * N ? a.ews[e] : a.ewd[e]);
    obs[r * ds + i] = v;
    const int j = s0 + r, m = j / C, slot = j - m * C;
    if (a.observations && slot < sl_.n_slots)
      a.observations[((((size_t)(sl_.base + slot) * K + k) * a.M + m) * H + h) * D0 + i] = v;
  }
  __syncthreads();

  // ---- 3. the network, pass after pass of MB instances ----
  const int D = a.net.width[0], L = a.net.L;
  const bool shared = a.net.kind == WF_POLICY_SHARED;
  const int n_inst = shared ? nt * N : nt;
  const float* __restrict__ wt = a.wt + (size_t)k * a.net.P;
  for (int b0 = 0; b0 < n_inst; b0 += MB) {  // (block-uniform)
    int cnt = n_inst - b0;
    cnt = cnt > MB ? MB : cnt;
    for (int q = tid; q < cnt * D; q += nth) {
      const int inst = q / D, i = q - inst * D;
      float raw;
      if (shared) {
        const int gi = b0 + inst, r = gi / N, t = gi - r * N;
        raw = i < 3 ? obs[r * ds + i * N + t] : obs[r * ds + 3 * N + (i - 3)];
      } else {
        raw = obs[(b0 + inst) * ds + i];
      }
      x0[inst * xs + i] = ((double)raw - a.shift[i]) * a.scale[i];
    }
    __syncthreads();
    const double* in = x0;
    int ins = xs;
    const int G = (cnt + 3) >> 2;  // groups of four instances
    for (int l = 0; l < L; ++l) {  // (block-uniform)
      const int nin = a.net.width[l], nout = a.net.width[l + 1];
      const float* __restrict__ W = wt + a.net.woff[l];
      const float* __restrict__ bias = wt + a.net.boff[l];
      double* outp = (l & 1) ? bufB : bufA;
      const int hidden = l < L - 1 ? a.net.act : a.net.fin;
      for (int q = tid; q < nout * G; q += nth) {
        const int g = q / nout, o = q - g * nout;
        const int i1 = g + G, i2 = g + 2 * G, i3 = g + 3 * G;
        const bool v1 = i1 < cnt, v2 = i2 < cnt, v3 = i3 < cnt;
        const double* xa = in + (size_t)g * ins;
        const double* xb = in + (size_t)(v1 ? i1 : g) * ins;
        const double* xc = in + (size_t)(v2 ? i2 : g) * ins;
        const double* xd = in + (size_t)(v3 ? i3 : g) * ins;
        const double bz = (double)bias[o];
        double za = bz, zb = bz, zc = bz, zd = bz;
        for (int i = 0; i < nin; ++i) {
          const double w = (double)W[(size_t)i * nout + o];
          za = za + w * xa[i];
          zb = zb + w * xb[i];
          zc = zc + w * xc[i];
          zd = zd + w * xd[i];
        }
        outp[(size_t)g * as + o] = policy_act(hidden, za);
        if (v1) outp[(size_t)i1 * as + o] = policy_act(hidden, zb);
        if (v2) outp[(size_t)i2 * as + o] = policy_act(hidden, zc);
        if (v3) outp[(size_t)i3 * as + o] = policy_act(hidden, zd);
      }
      __syncthreads();
      in = outp;
      ins = as;
    }
    // the pass's raw actions: `in` holds f(z) of the last layer
    const int per = shared ? 1 : N;  // turbines an instance decides
    for (int q = tid; q < cnt * per; q += nth) {
      const int inst = q / per, tt = q - inst * per;
      const double* z = in + (size_t)inst * ins + (a.net.discrete ? 3 * tt : tt);
      float act;
      if (a.net.discrete) {
        int best = 0;
        double zb = z[0];
        if (z[1] > zb) { zb = z[1]; best = 1; }
        if (z[2] > zb) { best = 2; }
        act = (float)best;
      } else {
        act = (float)(a.net.out_scale * z[0]);
      }
      const int gi = b0 + inst;
      actf[shared ? gi : gi * N + tt] = act;  // (shared: gi = r N + t; central: gi = r)
    }
    __syncthreads();  // (the next pass overwrites x0 and the activations; the actions are visible)
  }

  // ---- 4. / 5. the transition and the next rows ----
  const int moves_new_base = 1 + h;
  for (int q = tid; q < nt * N; q += nth) {
    const int r = q / N, t = q - r * N;
    const size_t e = e0 + r;
    const int j = s0 + r, m = j / C, slot = j - m * C, b = wf_slot_farm(sl_, slot);
    const int moves_new = a.env.moves[b] + moves_new_base;
    const float raw = actf[q], y = obs[r * ds + t], acc = a.st.acc[e * N + t];
    if (wf_env_gate_closed(a.env, acc, moves_new)) atomicAdd(&ng[r], 1);  // (an integer sum in LDS: any order gives the same value)
    float da;
    const float yn = wf_env_transition(a.env, y, raw, acc, moves_new, da);
    a.st.acc[e * N + t] = acc + fabsf(da);
    a.yaw[e * N + t] = yn;
    if (slot < sl_.n_slots) {
      const size_t f = (size_t)(sl_.base + slot) * K + k;
      if (a.actions) a.actions[((f * a.M + m) * H + h) * N + t] = raw;
      if (a.first_action && h == 0 && m == 0) a.first_action[f * N + t] = raw;  // (observation 0 is the same for every member)
    }
  }
  __syncthreads();
  if (tid < nt) {
    const size_t e = e0 + tid;
    a.st.gated[e] += ng[tid];
    if (a.wind || a.paths) {  // the wind step h is solved under
      const int j = s0 + tid, m = j / C, slot = j - m * C;
      const double* w = policy_row_wind(a, (size_t)sl_.base + (slot < sl_.n_slots ? slot : 0), slot, m);
      a.ews[e] = w[2 * h];
      a.ewd[e] = w[2 * h + 1];
    }
  }
}

__global__ __launch_bounds__(256) void wf_policy_reduce_kernel(const WfPolicyRun* run, const WfSlots sl_, const int T, const int sp, const int sl) {
  extern __shared__ double pr_lds[];
  const WfPolicyRun& a = *run;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = a.N, K = a.K, H = a.H, C = sl_.C;
  double* rets = pr_lds;                                  // [K][T] the tile's returns
  double* wrl = rets + (size_t)K * T;                     // [T] normalisers, rewards and farm powers of the last step
  double* rwl = wrl + T;
  double* psl = rwl + T;
  float* pw = reinterpret_cast<float*>(psl + T);          // [T][sp]
  float* ld = pw + (size_t)T * sp;                        // [T][sl]
  const int s0 = blockIdx.x * T;
  int nt = C - s0;
  nt = nt > T ? T : nt;
  const int hp = H - 1;
  for (int k = 0; k < K; ++k) {  // (block-uniform)
    const size_t e0 = (size_t)k * C + s0;
    policy_tile_rewards(a, sl_, e0, s0, nt, hp, sp, sl, wrl, rwl, psl, pw, ld);
    if (tid < nt) {
      const size_t e = e0 + tid;
      const int slot = s0 + tid;
      const double total = a.st.ret[e] + a.st.disc[e] * rwl[tid];
      rets[k * T + tid] = total;
      if (slot < sl_.n_slots) {
        const size_t f = (size_t)(sl_.base + slot) * K + k;
        if (a.returns) a.returns[f] = total;
        if (a.rewards) a.rewards[f * H + hp] = rwl[tid];
        if (a.farm_power) a.farm_power[f * H + hp] = psl[tid];
        if (a.gated) a.gated[f] = a.st.gated[e];
      }
    }
    for (int q = tid; q < nt * N; q += nth) {
      const int r = q / N, t = q - r * N, slot = s0 + r;
      if (a.final_yaw && slot < sl_.n_slots) a.final_yaw[((size_t)(sl_.base + slot) * K + k) * N + t] = a.yaw[(e0 + r) * N + t];
    }
  }
  __syncthreads();
  // (thread s reads the returns it wrote itself)
  if (tid < nt && a.best && s0 + tid < sl_.n_slots) {
    double bv = rets[tid];
    int bk = 0;
    for (int k = 1; k < K; ++k) {
      const double v = rets[k * T + tid];
      if (v > bv) { bv = v; bk = k; }
    }
    a.best[sl_.base + s0 + tid] = bk;
  }
}

// The tile: the rows a workgroup serves, from the LDS a row needs beside the pass buffers; at most 16, at most the chunk.
WfPolicyPlan wf_policy_plan(const WfPolicyNet& net, int N, int C) {
  WfPolicyPlan p{};
  const size_t budget = 56 * 1024;
  int wmax = 1;
  for (int l = 1; l <= net.L; ++l) wmax = net.width[l] > wmax ? net.width[l] : wmax;
  p.xs = net.width[0] | 1;
  p.as = wmax | 1;
  p.ds = (3 * N + 2) | 1;
  p.sp = N | 1;
  p.sl = (4 * N) | 1;
  p.threads = 256;
  const size_t per_inst = sizeof(double) * ((size_t)p.xs + 2 * (size_t)p.as);
  const size_t per_row = sizeof(float) * ((size_t)p.ds + N + p.sp + p.sl) + sizeof(int) + 3 * sizeof(double);
  int T;
  if (net.kind == WF_POLICY_SHARED) {
    // half of the budget to the rows, the rest to a pass of instances
    T = (int)((budget / 2) / per_row);
    T = T < 1 ? 1 : (T > 16 ? 16 : T);
    T = T > C ? C : T;
    size_t left = budget - (size_t)T * per_row;
    int MB = (int)(left / per_inst);
    MB = MB < 1 ? 1 : MB;
    MB = MB > T * N ? T * N : MB;
    p.MB = MB;
  } else {
    T = (int)(budget / (per_row + per_inst));
    T = T < 1 ? 1 : (T > 16 ? 16 : T);
    T = T > C ? C : T;
    p.MB = T;
  }
  p.T = T;
  p.lds_bytes = (size_t)p.MB * per_inst + (size_t)T * per_row + 16;
  return p;
}

extern "C" hipError_t wfk_launch_policy_transpose(const WfPolicyRun* host, const WfPolicyRun* dev, hipStream_t s) {
  const size_t n = (size_t)host->K * host->net.P;
  const int blocks = (int)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256);
  hipLaunchKernelGGL(wf_policy_transpose_kernel, dim3(blocks), dim3(256), 0, s, dev);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_policy_begin(const WfPolicyRun* host, const WfPolicyRun* dev, const WfSlots* sl, hipStream_t s) {
  const size_t n = (size_t)host->K * host->M * sl->C * host->N;
  const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
  hipLaunchKernelGGL(wf_policy_begin_kernel, dim3(blocks), dim3(256), 0, s, dev, *sl);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_policy_advance(const WfPolicyRun* host, const WfPolicyRun* dev, const WfSlots* sl, int round, hipStream_t s) {
  const int tiles = (host->M * sl->C + host->pl.T - 1) / host->pl.T;
  hipLaunchKernelGGL(wf_policy_advance_kernel, dim3(tiles, host->K), dim3(host->pl.threads), host->pl.lds_bytes, s, dev, *sl, round);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_policy_reduce(const WfPolicyRun* host, const WfPolicyRun* dev, const WfSlots* sl, hipStream_t s) {
  // the tile: [K][T] doubles of returns and the reward tile's [T][sp] + [T][sl] floats in 48 KiB, at most a slot per thread
  const int sp = host->N | 1, sll = (4 * host->N) | 1;
  const size_t per = sizeof(double) * ((size_t)host->K + 3) + sizeof(float) * ((size_t)sp + sll);
  int T = (int)(48 * 1024 / per);
  T = T < 1 ? 1 : (T > 64 ? 64 : T);
  T = T > sl->C ? sl->C : T;
  const int tiles = (sl->C + T - 1) / T;
  hipLaunchKernelGGL(wf_policy_reduce_kernel, dim3(tiles), dim3(T * host->N <= 64 ? 64 : 256), per * T, s, dev, *sl, T, sp, sll);
  return hipGetLastError();
}
extern "C" hipError_t wfk_policy_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[WF_POLICY_KERNELS] = {(const void*)wf_policy_transpose_kernel, (const void*)wf_policy_begin_kernel,
                                       (const void*)wf_policy_advance_kernel, (const void*)wf_policy_reduce_kernel};
  if (kernel < 0 || kernel >= WF_POLICY_KERNELS) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, fn[kernel]);
}
