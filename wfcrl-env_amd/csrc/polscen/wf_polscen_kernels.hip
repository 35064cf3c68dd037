// wf_polscen_kernels.hip — the kernels that, with the policy extension's, make policy rollouts over a wind ensemble run on the
// device (include/wfpolscen.h).  The farm solve is the existing wf_step on the object's evaluator handle, one batched step per
// env step; the closed loop between two steps — reward, observation, network, action and transition, stores — is the policy
// extension's advance kernel (policy/wf_policy_kernels.hip), launched here with M members and the chunk's path buffer, and the
// round-0 rows and the transposed parameters are its begin and transpose kernels': none of that exists twice.  What this file
// adds, per chunk of C slots, evaluator farm e = (k M + m) C + slot:
//
//   wf_polscen_paths_kernel    once, before the begin kernel, A THREAD PER (slot, member): it draws the member's ramp rate
//                              and walks its H ticks, two deviates per tick, with the ensemble's scalar pieces
//                              (ensemble/wf_ensemble.h: wf_ensemble_rate, wf_ensemble_deviates, wf_ensemble_tick), and stores (speed,
//                              direction) of tick h + 1 to the chunk's path buffer [C][M][H][2] and to wind_paths.  No LDS:
//                              M H reaches 4096 pairs of doubles per slot.  A thread's stores are H pairs apart from its
//                              neighbour's; the kernel runs once per chunk against H + 1 steps.
//   wf_polscen_returns_kernel  once, after the last step, A WORKGROUP PER TILE of T consecutive rows of one policy (the advance
//                              kernel's rows: j = m C + slot): the last reward through the extensions' reward tile
//                              (wf_staged_row_rewards), normalised by the member's speed of step H - 2 (H = 1: the farm's
//                              current speed), the member return ret + g r as the policy extension's reduce forms it, kept per
//                              row for the statistics; rewards and farm_power of the last step, member_returns, gated,
//                              final_yaw.
//   wf_polscen_stats_kernel    once, A WORKGROUP PER SLOT: the slot's K M member returns -> LDS; then the ensemble's
//                              statistics (wf_member_statistics over the returns at stride 1), which emit to the outputs and
//                              leave the score in LDS; thread 0 takes the argmax over k ascending, strictly greater wins: the
//                              lowest index among equal maxima.
//
// No floating-point atomics, no order that depends on scheduling.  Trip counts are run-time values and nothing is indexed by a
// run-time value in registers: no private segment at any N (tests/test_polscen.py reads the metadata); every barrier sits in
// block-uniform control flow.  The library is built with -ffp-contract=off: every product and sum of the paths, the return and
// the statistics is one rounding, as in tests/scenario_ref.py.
#include <hip/hip_runtime.h>

#include "wf_polscen.h"

__global__ __launch_bounds__(256) void wf_polscen_paths_kernel(const WfPolscenPathsArgs a) {
  const int M = a.ens.M, H = a.ens.H;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.sl.C * M) return;
  const int slot = q / M, m = q - slot * M;
  const int b = wf_slot_farm(a.sl, slot);
  const bool writes = slot < a.sl.n_slots;
  const size_t in = writes ? slot : 0;  // the slot's input block
  const WfEnsembleWalk w = wf_ensemble_walk<false>(a.ens, b, in);  // (a thread per member: nothing to pin)
  const double rate = wf_ensemble_rate(a.ens, b, m);
  double x = w.Sc, y = w.Dc;
  double* __restrict__ buf = a.paths + (size_t)q * H * 2;
  double* __restrict__ out = (writes && a.wind_paths) ? a.wind_paths + (in * M + m) * H * 2 : nullptr;
  for (int j = 0; j < H; ++j) {
    double z17, z18, s, d;
    wf_ensemble_deviates(a.ens, b, m, j, z17, z18);
    wf_ensemble_tick(w, rate, j, z17, z18, x, y, s, d);
    buf[2 * j] = s;
    buf[2 * j + 1] = d;
    if (out) {
      out[2 * j] = s;
      out[2 * j + 1] = d;
    }
  }
}

// (the run block is not declared __restrict__ and is read where a phase needs a field: policy/wf_policy.h says why)
__global__ __launch_bounds__(256) void wf_polscen_returns_kernel(const WfPolicyRun* run, const WfSlots sl_, const WfPolscenReduceArgs x,
                                                                 const int T, const int sp, const int sl) {
  extern __shared__ double pn_lds[];
  const WfPolicyRun& a = *run;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int C = sl_.C, R = a.M * C;                        // R: the rows of one policy
  double* const wrl = pn_lds;                              // [T] the rows' normalisers, ...
  double* const rwl = wrl + T;                             // [T] ... rewards ...
  double* const psl = rwl + T;                             // [T] ... and farm powers of the last step
  float* const pw = reinterpret_cast<float*>(psl + T);     // [T][sp] the reward tile: powers ...
  float* const ld = pw + (size_t)T * sp;                   // [T][sl] ... and load values
  const int k = blockIdx.y, s0 = blockIdx.x * T;
  int nt = R - s0;
  nt = nt > T ? T : nt;                                    // rows of this tile (block-uniform)
  const size_t e0 = (size_t)k * R + s0;
  const int hp = a.H - 1;
  if (tid < nt) {
    const int j = s0 + tid, m = j / C, slot = j - m * C, b = wf_slot_farm(sl_, slot);
    // step 0: the farm's CURRENT speed (a pending prev-wind speed is not read); step hp >= 1: the member's speed of step hp - 1
    wrl[tid] = hp == 0 ? a.ws[(size_t)b * a.wind_stride] : a.paths[(((size_t)slot * a.M + m) * a.H + (hp - 1)) * 2];
  }
  wf_staged_row_rewards(
      a.power_ev + e0 * a.N, a.load_ev + e0 * 4 * a.N, nt, a.N, nt, sp, sl, a.load_coef, pw, ld, [wrl](int r) { return wrl[r]; },
      [rwl, psl](int r, double rew, double psum) {
        rwl[r] = rew;
        psl[r] = psum;
      });
  const int N = a.N, K = a.K, M = a.M, H = a.H;
  if (tid < nt) {
    const size_t e = e0 + tid;
    const int j = s0 + tid, m = j / C, slot = j - m * C;
    const double total = a.st.ret[e] + a.st.disc[e] * rwl[tid];
    x.mret[e] = total;
    if (slot < sl_.n_slots) {
      const size_t f = ((size_t)(sl_.base + slot) * K + k) * M + m;
      if (x.member_returns) x.member_returns[f] = total;
      if (a.rewards) a.rewards[f * H + hp] = rwl[tid];
      if (a.farm_power) a.farm_power[f * H + hp] = psl[tid];
      if (a.gated) a.gated[f] = a.st.gated[e];
    }
  }
  if (a.final_yaw) {
    for (int q = tid; q < nt * N; q += nth) {
      const int r = q / N, t = q - r * N, j = s0 + r, m = j / C, slot = j - m * C;
      if (slot < sl_.n_slots) a.final_yaw[(((size_t)(sl_.base + slot) * K + k) * M + m) * N + t] = a.yaw[(e0 + r) * N + t];
    }
  }
}

__global__ __launch_bounds__(256) void wf_polscen_stats_kernel(const WfPolicyRun* run, const WfSlots sl_, const WfPolscenReduceArgs x) {
  extern __shared__ double ps_lds[];
  const WfPolicyRun& a = *run;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int K = a.K, M = a.M, KM = K * M, C = sl_.C;
  double* const rets = ps_lds;     // [K][M] the slot's member returns
  double* const srt = rets + KM;   // [nth] a pass's returns in ascending rank
  double* const sc = srt + nth;    // [K] the scores
  const int slot = blockIdx.x;     // (< n_slots: the launch has a workgroup per farm of the chunk)
  for (int i = tid; i < KM; i += nth) rets[i] = x.mret[(size_t)i * C + slot];  // (row (k, m) is evaluator farm (k M + m) C + slot)
  __syncthreads();
  const size_t o0 = (size_t)(sl_.base + slot) * K;
  wf_member_statistics(rets, 1, K, M, x.q, x.lam, srt, [&x, o0, sc](int k, double mean, double cvar, double score) {
    if (x.expected) x.expected[o0 + k] = mean;
    if (x.cvar) x.cvar[o0 + k] = cvar;
    if (x.score) x.score[o0 + k] = score;
    sc[k] = score;
  });
  __syncthreads();
  if (tid == 0 && x.best) {
    double bv = sc[0];
    int bk = 0;
    for (int k = 1; k < K; ++k) {
      const double v = sc[k];
      if (v > bv) { bv = v; bk = k; }
    }
    x.best[sl_.base + slot] = bk;
  }
}

// The returns kernel's tile: three [T] doubles and the reward tile's [T][sp] + [T][sl] floats in 48 KiB, at most 64 rows, at
// most the policy's rows.
WfPolscenTile wf_polscen_tile(int N, int rows) {
  WfPolscenTile t{};
  t.sp = N | 1;
  t.sl = (4 * N) | 1;
  const size_t per = 3 * sizeof(double) + sizeof(float) * ((size_t)t.sp + t.sl);
  int T = (int)(48 * 1024 / per);
  T = T < 1 ? 1 : (T > 64 ? 64 : T);
  t.T = T > rows ? rows : T;
  t.threads = t.T * N <= 64 ? 64 : 256;
  t.lds_bytes = per * t.T;
  return t;
}

extern "C" hipError_t wfk_launch_polscen_paths(const WfPolscenPathsArgs* a, hipStream_t s) {
  const int n = a->sl.C * a->ens.M;
  hipLaunchKernelGGL(wf_polscen_paths_kernel, dim3((n + 63) / 64), dim3(64), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_polscen_returns(const WfPolicyRun* host, const WfPolicyRun* dev, const WfSlots* sl, const WfPolscenReduceArgs* x,
                                                 hipStream_t s) {
  const int rows = host->M * sl->C;
  const WfPolscenTile t = wf_polscen_tile(host->N, rows);
  hipLaunchKernelGGL(wf_polscen_returns_kernel, dim3((rows + t.T - 1) / t.T, host->K), dim3(t.threads), t.lds_bytes, s, dev, *sl, *x, t.T, t.sp,
                     t.sl);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_polscen_stats(const WfPolicyRun* host, const WfPolicyRun* dev, const WfSlots* sl, const WfPolscenReduceArgs* x,
                                               hipStream_t s) {
  const int threads = 256;
  const size_t lds = sizeof(double) * ((size_t)host->K * host->M + threads + host->K);
  hipLaunchKernelGGL(wf_polscen_stats_kernel, dim3(sl->n_slots), dim3(threads), lds, s, dev, *sl, *x);
  return hipGetLastError();
}
extern "C" hipError_t wfk_polscen_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[3] = {(const void*)wf_polscen_paths_kernel, (const void*)wf_polscen_returns_kernel, (const void*)wf_polscen_stats_kernel};
  if (kernel < 0 || kernel >= WF_POLSCEN_KERNELS) return hipErrorInvalidValue;
  if (kernel >= 3) return wfk_policy_func_attributes(kernel - 3, a);  // transpose, begin, advance
  return hipFuncGetAttributes(a, fn[kernel]);
}
