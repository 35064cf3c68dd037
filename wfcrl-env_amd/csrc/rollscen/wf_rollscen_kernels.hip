// wf_rollscen_kernels.hip — the kernels around the step kernel that make scenario rollouts of yaw-table controllers run on the
// device (include/wfrollscen.h).  The farm solve is the existing wf_step on the object's evaluator handle; these kernels are
// the glue, so that a whole run — the ensemble's draws included — is enqueued without a host read:
//
//   wf_rollscen_layout_kernel  once per chunk, ONE WORKGROUP PER SLOT, three phases.
//                              PHASE 1 — the member paths, every row's evaluator wind and wind_paths: the ensemble's tiled body
//                              (ensemble/wf_ensemble.h: wf_ensemble_tiles), in tiles of 2048 / M ticks.  The observations of
//                              phase 2 are the wind of rows (0, m, .) — what this block has just written, behind a block barrier.
//                              PHASE 2 — filter and bracket depend on (k, m, h), not on the turbine: thread (k, m) walks
//                              h = 0 .. H - 1 ONCE — observation obs[min(h + lead, H)], the float64 filter, then steps 1-3 of
//                              the table look-up (rose/wf_rose_lookup.h: rose_bracket, the rose extension's own device
//                              function) — and leaves a record of 32 bytes per step.  The records of a slot lie in LDS, over
//                              the tile that is no longer needed, up to WF_ROLLSCEN_LDS_RECORDS rows; above they go through the
//                              slot's scratch block in global memory, read by the block that wrote them (block barrier:
//                              workgroup-scope release / acquire).  The two are two INSTANCES of the kernel, picked at launch.
//                              PHASE 3 — thread (k, m, t), t fastest, keeps the yaw and the accumulator of turbine t in
//                              registers and walks the horizon as the rollout lay-out does: the record every lane of its
//                              (k, m) shares (a broadcast), the table entries T[.][.][t] — consecutive lanes on consecutive
//                              floats —, the target, the raw action and the env's transition (wf_env_gate_closed,
//                              wf_env_transition: ext/wf_ext_kernels.h), and writes actions[(((slot K + k) M + m) H + h) N + t]
//                              and yaw[(slot R + (k M + m) H + h) N + t]: consecutive floats per wave, whole lines along the
//                              turbine index.  final_yaw after the last step, first_action from member 0's step 0.  `gated`
//                              is a sum of ints: every thread adds its count to its (k, m)'s LDS word (integer adds in any
//                              order give one value), then one store per (k, m).
//   wf_rollscen_reduce_kernel  once per chunk, after the step, ONE WORKGROUP PER SLOT: the rows are in the scenario order, and
//                              this is the scenario extension's reduce, the same body instantiated here
//                              (scenario/wf_scenario_reduce.h: wf_scenario_statistics) with K controllers.
//
// A block has 64 threads for a few short rollouts of a small farm, 1024 from WF_ROLLSCEN_WIDE trajectories per slot on, else 256.
// LDS per block stays below 64 KiB: the tile is at most 2 x (2048 + 64) doubles (33 KiB), the records at most 32 KiB in the
// same bytes, the K M counts of `gated` at most 16 KiB behind them.  Trip counts are run-time values, the table slot is picked
// by comparison (ROSE_PICK), a thread holds ONE turbine: nothing is indexed by a run-time value in registers, so there is no
// private segment at any N and no spill (tests/test_rollscen.py reads the metadata); every barrier sits in block-uniform
// control flow.  The library is built with -ffp-contract=off: every product and sum of the paths, the filter, the transition
// and the statistics is one rounding, in the headers' order.
#include <hip/hip_runtime.h>

#include "../rose/wf_rose_lookup.h"
#include "../scenario/wf_scenario_reduce.h"
#include "wf_rollscen.h"

#define WF_ROLLSCEN_WIDE 1024  // trajectories per slot (K M N) from which the lay-out kernel runs 1024 threads

static_assert(sizeof(WfRollscenBracket) == 32 && sizeof(RoseBracket) == sizeof(WfRollscenBracket), "a bracket is 32 bytes");
static_assert(WF_ROLLSCEN_LDS_RECORDS * sizeof(WfRollscenBracket) <= 32 * 1024, "the records in LDS take at most 32 KiB");

// `rs_lds` is the block's dynamic LDS: A8 doubles — the tile's [2][M][Hs], then (SPILL == false) the [R] records in the same
// bytes —, then the [K M] ints of `gated`
template <bool SPILL>
__global__ __launch_bounds__(1024) void wf_rollscen_layout_kernel(const WfRollscenLayoutArgs a, int Ht, int Hs, int A8) {
  extern __shared__ double rs_lds[];
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = a.N, K = a.K, M = a.ens.M, H = a.ens.H, R = K * M * H;
  const int slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  // ---- phase 1: the member paths ----
  wf_ensemble_tiles(a.ens, a.sl, K, Ht, Hs, rs_lds, a.ews, a.ewd, a.wind_paths);
  // what addresses the rest is formed HERE, from the slot and the farm in vector registers — formed at the top and held in
  // scalar registers across the draws it would not fit (spilled scalar registers)
  int slot_v = slot, b_v = b;
  WF_IN_VGPR(slot_v); WF_IN_VGPR(b_v);
  const bool writes_v = slot_v < a.sl.n_slots;
  const size_t in_v = writes_v ? slot_v : 0, st0 = (size_t)b_v * N;
  const int KM = K * M;
  int* n_gated = reinterpret_cast<int*>(rs_lds + A8);  // [K M]
  WfRollscenBracket* rec = SPILL ? a.brk + (size_t)slot_v * R : reinterpret_cast<WfRollscenBracket*>(rs_lds);  // [R]
  // ---- phase 2: the filter and the bracket of every (k, m, h), once per (controller, member): a recurrence over h ----
  {
    const double ws0 = a.ens.ws[(size_t)b_v * a.ens.wind_stride], wd0 = a.ens.wd[(size_t)b_v * a.ens.wind_stride];
    const double* ews0 = a.ews + (size_t)slot_v * R;  // rows (0, m, .): member m's winds, written in phase 1 by this block
    const double* ewd0 = a.ewd + (size_t)slot_v * R;
    for (int km = tid; km < KM; km += nth) {
      n_gated[km] = 0;
      const int k = km / M, m = km - k * M;
      const int lead = a.c_lead[k], cs = a.c_slot[k];
      const double alpha = a.c_alpha[k];
      const WfRoseTable tb = ROSE_PICK(a.tab, cs);
      const double* __restrict__ f0 = a.filter0 ? a.filter0 + (in_v * K + k) * 2 : nullptr;
      double fs = f0 ? f0[0] : ws0, fd = f0 ? f0[1] : wd0;
      const double* os_m = ews0 + (size_t)m * H;
      const double* od_m = ewd0 + (size_t)m * H;
      WfRollscenBracket* out = rec + (size_t)km * H;
      for (int h = 0; h < H; ++h) {
        int j = h + lead;
        j = j < H ? j : H;  // obs[0] the parent's wind, obs[j] member m's tick j: the wind of step j - 1
        const double os = j > 0 ? os_m[j - 1] : ws0, od = j > 0 ? od_m[j - 1] : wd0;
        if (alpha == 1.0) {
          fs = os; fd = od;
        } else {
          fs = fs + alpha * (os - fs);
          const double d = od - fd;
          fd = fd + alpha * (d - 360.0 * rint(d / 360.0));
        }
        const RoseBracket rb = rose_bracket(tb, fs, fd);
        WfRollscenBracket w;
        w.k = rb.k; w.k1 = rb.k1; w.j = rb.j; w.j1 = rb.j1; w.fd = rb.fd; w.fs = rb.fs;
        out[h] = w;
      }
    }
  }
  __syncthreads();  // (the records, and the zeroed counts, are visible to the block)
  // ---- phase 3: the trajectories, one thread per (controller, member, turbine) ----
  const int moves0 = a.env.moves[b_v];
  const float half = 0.5f * a.env.step;
  float* __restrict__ act = (writes_v && a.actions) ? a.actions + in_v * R * N : nullptr;
  float* __restrict__ first = (writes_v && a.first_action) ? a.first_action + in_v * K * N : nullptr;
  float* __restrict__ yaw = a.yaw + (size_t)slot_v * R * N;
  const int n_traj = KM * N;
  for (int q = tid; q < n_traj; q += nth) {
    const int km = q / N, t = q - km * N;
    const int k = km / M, m = km - k * M;
    const int cs = a.c_slot[k];
    const float band = a.c_deadband[k];
    const WfRoseTable tb = ROSE_PICK(a.tab, cs);
    float y = a.env.yaw[st0 + t], acc = a.env.acc[st0 + t];
    int closed = 0;
    size_t o = (size_t)km * H * N + t;  // row (k, m, 0)
    const WfRollscenBracket* w_h = rec + (size_t)km * H;
    for (int h = 0; h < H; ++h, o += N) {
      const WfRollscenBracket w = w_h[h];
      RoseBracket rb;
      rb.k = w.k; rb.k1 = w.k1; rb.j = w.j; rb.j1 = w.j1; rb.fd = w.fd; rb.fs = w.fs;
      float tg = rose_lookup(tb, rb, t, N);
      tg = fminf(fmaxf(tg, a.env.lo), a.env.hi);
      const float e = tg - y;
      float raw;
      if (a.env.discrete) raw = fabsf(e) <= band ? 1.0f : (e >= half ? 2.0f : (e <= -half ? 0.0f : 1.0f));
      else raw = fabsf(e) <= band ? 0.0f : fminf(fmaxf(e, -a.env.step), a.env.step);
      closed += wf_env_gate_closed(a.env, acc, moves0 + 1 + h) ? 1 : 0;
      float da;
      y = wf_env_transition(a.env, y, raw, acc, moves0 + 1 + h, da);
      acc += fabsf(da);
      if (act) act[o] = raw;
      if (first && h == 0 && m == 0) first[(size_t)k * N + t] = raw;
      yaw[o] = y;
    }
    if (writes_v && a.final_yaw) a.final_yaw[in_v * n_traj + q] = y;
    atomicAdd(&n_gated[km], closed);  // (an integer sum in LDS: any order gives the same value)
  }
  __syncthreads();
  if (writes_v && a.gated)
    for (int km = tid; km < KM; km += nth) a.gated[in_v * KM + km] = n_gated[km];
}

__global__ __launch_bounds__(1024) void wf_rollscen_reduce_kernel(const WfRollscenReduceArgs a, int T, int sp, int sl, int Hs) {
  extern __shared__ double rs_red[];
  wf_scenario_statistics(a, T, sp, sl, Hs, rs_red);
}

extern "C" hipError_t wfk_launch_rollscen_layout(const WfRollscenLayoutArgs* a, hipStream_t s) {
  const int KM = a->K * a->ens.M, R = KM * a->ens.H;
  // a few short rollouts of a small farm: one wave.  From WF_ROLLSCEN_WIDE trajectories per slot on, 1024 threads: a trajectory
  // is a chain of dependent loads (record, table entries) and float32 steps, H long, and a slot has one workgroup to hide them
  const int threads = (R <= 128 && KM * a->N <= 64) ? 64 : (KM * a->N >= WF_ROLLSCEN_WIDE ? 1024 : 256);
  const WfEnsembleTile t = wf_ensemble_tile(a->ens.M, a->ens.H);
  const int Ht = t.Ht, Hs = t.Hs;
  const int tile8 = 2 * a->ens.M * Hs, rec8 = a->spill ? 0 : 4 * R;  // doubles: the tile, the records that follow it in the same bytes
  const int A8 = tile8 > rec8 ? tile8 : rec8;
  const size_t lds = sizeof(double) * (size_t)A8 + sizeof(int) * (size_t)KM;
  if (a->spill) hipLaunchKernelGGL(wf_rollscen_layout_kernel<true>, dim3(a->sl.C), dim3(threads), lds, s, *a, Ht, Hs, A8);
  else hipLaunchKernelGGL(wf_rollscen_layout_kernel<false>, dim3(a->sl.C), dim3(threads), lds, s, *a, Ht, Hs, A8);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_rollscen_reduce(const WfRollscenReduceArgs* a, hipStream_t s) {
  const WfScenarioReduceLaunch l = wf_scenario_reduce_launch(a->N, a->K, a->M, a->H);
  hipLaunchKernelGGL(wf_rollscen_reduce_kernel, dim3(a->sl.n_slots), dim3(l.threads), l.lds_bytes, s, *a, l.t.T, l.t.sp, l.t.sl, l.Hs);
  return hipGetLastError();
}
extern "C" hipError_t wfk_rollscen_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[WF_ROLLSCEN_KERNELS] = {(const void*)wf_rollscen_layout_kernel<false>, (const void*)wf_rollscen_layout_kernel<true>,
                                         (const void*)wf_rollscen_reduce_kernel};
  if (kernel < 0 || kernel >= WF_ROLLSCEN_KERNELS) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, fn[kernel]);
}
