// wf_rollout_kernels.hip — the kernels around the step kernel that make closed-loop rollouts of yaw-table controllers run on
// the device (include/wfrollout.h).  The farm solve is the existing wf_step on the object's evaluator handle; these two
// kernels are the glue, so that a whole run is enqueued without a host read:
//
//   wf_rollout_layout_kernel  once per chunk, ONE WORKGROUP PER SLOT, two phases.
//                             PHASE A — the filter is a recurrence over h, and filter and bracket depend on (k, h) only, not on
//                             the turbine.  A1: thread k < K walks h = 0 .. H - 1 once — observation obs[min(h + lead, H)],
//                             the float64 filter — and leaves the filtered wind of (k, h) in the slot's scratch block [K][H]
//                             in global memory (records of 32 bytes: K H of them exceed LDS at the limits), and
//                             filter_final; the other threads write every row's wind meanwhile.  Block barrier.  A2: the
//                             block's threads take the (k, h) pairs in turn and replace the filtered wind by its bracket —
//                             steps 1-3 of the table look-up (rose/wf_rose_lookup.h: the rose extension's own device
//                             function), whose two binary searches are chains of dependent loads: they run side by side
//                             here, not one after the other inside the serial walk of A1.  Block barrier (workgroup-scope
//                             release / acquire: the records are read by the block that wrote them).
//                             PHASE B — thread (k, t), t fastest, keeps the yaw and the accumulator of turbine t in registers
//                             and walks controller k's steps as the lookahead lay-out does: it reads the bracket every lane of
//                             its k shares (one line, broadcast), the table entries T[.][.][t] — consecutive lanes on
//                             consecutive floats —, forms the target, the raw action and the env's transition
//                             (wf_env_transition, ext/wf_ext_kernels.h) and writes actions[((slot K + k) H + h) N + t] and
//                             yaw[(slot R + k H + h) N + t]: both stores consecutive floats per wave.  final_yaw after the
//                             last step.  `gated` is a sum of ints: every thread adds its count to its k's LDS word (integer
//                             adds in any order give one value), then one store per k.
//   wf_rollout_reduce_kernel  once per chunk, after the step, ONE WORKGROUP PER SLOT: the lookahead extension's reduce, the
//                             same body instantiated here (ext/wf_ext_kernels.h: wf_sequence_returns over
//                             wf_staged_row_rewards) — row rewards, returns in ascending h, fixed-order argmax.
//
// Trip counts are run-time values, the table slot is picked by comparison (ROSE_PICK), nothing is indexed by a run-time value
// in registers: no private segment, no spill (tests/test_rollout.py reads the metadata); every barrier sits in block-uniform
// control flow.  The library is built with -ffp-contract=off: the filter's products and sums, the transition's float32 sums
// and the return's product and sum stay single roundings, as in the NumPy restatement (tests/rollout_ref.py).
#include <hip/hip_runtime.h>

#include "../rose/wf_rose_lookup.h"
#include "wf_rollout.h"

static_assert(sizeof(WfRolloutBracket) == 32 && sizeof(RoseBracket) == sizeof(WfRolloutBracket), "a bracket is 32 bytes");

__global__ __launch_bounds__(256) void wf_rollout_layout_kernel(const WfRolloutLayoutArgs a) {
  __shared__ int n_gated[WF_ROLLOUT_MAX_K];
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = a.N, K = a.K, H = a.H, R = K * H;
  const int slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  const bool writes = slot < a.sl.n_slots;
  const size_t in = writes ? slot : 0;  // the slot's input block
  const size_t st0 = (size_t)b * N;     // ... and its farm's env state
  const double ws0 = a.ws[(size_t)b * a.wind_stride], wd0 = a.wd[(size_t)b * a.wind_stride];
  const double* __restrict__ wind = a.wind ? a.wind + in * H * 2 : nullptr;
  WfRolloutBracket* brk = a.brk + (size_t)slot * R;
  if (tid < WF_ROLLOUT_MAX_K) n_gated[tid] = 0;  // (blocks have at least 64 threads)
  // ---- phase A1: the filter of every (k, h), once per controller: a recurrence over h ----
  if (tid < K) {
    const int k = tid, lead = a.c_lead[k];
    const double alpha = a.c_alpha[k];
    const double* __restrict__ f0 = a.filter0 ? a.filter0 + (in * K + k) * 2 : nullptr;
    double fs = f0 ? f0[0] : ws0, fd = f0 ? f0[1] : wd0;
    for (int h = 0; h < H; ++h) {
      int j = h + lead;
      j = j < H ? j : H;  // obs[0] the parent's wind, obs[j] the wind of step j - 1
      const double os = (j > 0 && wind) ? wind[2 * (j - 1)] : ws0, od = (j > 0 && wind) ? wind[2 * (j - 1) + 1] : wd0;
      if (alpha == 1.0) {
        fs = os; fd = od;
      } else {
        fs = fs + alpha * (os - fs);
        const double d = od - fd;
        fd = fd + alpha * (d - 360.0 * rint(d / 360.0));
      }
      brk[(size_t)k * H + h].fs = fs;  // (the filtered wind waits in the record's two doubles for phase A2)
      brk[(size_t)k * H + h].fd = fd;
    }
    if (writes && a.filter_final) {
      a.filter_final[(in * K + k) * 2] = fs;
      a.filter_final[(in * K + k) * 2 + 1] = fd;
    }
  }
  for (int r = tid; r < R; r += nth) {
    const int h = r % H;
    a.ews[(size_t)slot * R + r] = wind ? wind[2 * h] : ws0;
    a.ewd[(size_t)slot * R + r] = wind ? wind[2 * h + 1] : wd0;
  }
  __syncthreads();  // (the filtered winds, and the zeroed counts, are visible to the block)
  // ---- phase A2: the bracket of every (k, h) — the look-up's steps 1-3, two binary searches — once per (k, h), all threads ----
  for (int r = tid; r < R; r += nth) {
    const int cs = a.c_slot[r / H];
    const WfRoseTable tb = ROSE_PICK(a.tab, cs);
    const RoseBracket rb = rose_bracket(tb, brk[r].fs, brk[r].fd);
    WfRolloutBracket w;
    w.k = rb.k; w.k1 = rb.k1; w.j = rb.j; w.j1 = rb.j1; w.fd = rb.fd; w.fs = rb.fs;
    brk[r] = w;  // (the thread that read the record overwrites it)
  }
  __syncthreads();  // (the brackets are visible to the block)
  // ---- phase B: the trajectories, one thread per (controller, turbine) ----
  const int moves0 = a.env.moves[b];
  const float half = 0.5f * a.env.step;
  float* __restrict__ act = a.actions ? a.actions + in * R * N : nullptr;
  float* __restrict__ out = a.yaw + (size_t)slot * R * N;
  const int n_traj = K * N;
  for (int q = tid; q < n_traj; q += nth) {
    const int k = q / N, t = q - k * N;
    const int cs = a.c_slot[k];
    const float band = a.c_deadband[k];
    const WfRoseTable tb = ROSE_PICK(a.tab, cs);
    float y = a.env.yaw[st0 + t], acc = a.env.acc[st0 + t];
    int closed = 0;
    size_t o = (size_t)k * H * N + t;
    for (int h = 0; h < H; ++h, o += N) {
      const WfRolloutBracket w = brk[(size_t)k * H + h];
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
      if (writes && act) act[o] = raw;
      out[o] = y;
    }
    if (writes && a.final_yaw) a.final_yaw[in * n_traj + q] = y;
    atomicAdd(&n_gated[k], closed);  // (an integer sum in LDS: any order gives the same value)
  }
  __syncthreads();
  if (tid < K && writes && a.gated) a.gated[in * K + tid] = n_gated[tid];
}

__global__ __launch_bounds__(256) void wf_rollout_reduce_kernel(const WfRolloutReduceArgs a, int T, int sp, int sl, int Hs) {
  extern __shared__ double ro_red[];
  wf_sequence_returns(a, T, sp, sl, Hs, ro_red);
}

extern "C" hipError_t wfk_launch_rollout_layout(const WfRolloutLayoutArgs* a, hipStream_t s) {
  const int threads = a->K * a->N <= 64 ? 64 : 256;  // a few controllers of a small farm: one wave (K <= 64 threads walk phase A)
  hipLaunchKernelGGL(wf_rollout_layout_kernel, dim3(a->sl.C), dim3(threads), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_rollout_reduce(const WfRolloutReduceArgs* a, hipStream_t s) {
  const WfReturnsLaunch l = wf_returns_launch(a->N, a->K, a->H);
  hipLaunchKernelGGL(wf_rollout_reduce_kernel, dim3(a->sl.n_slots), dim3(l.threads), l.lds_bytes, s, *a, l.t.T, l.t.sp, l.t.sl, l.Hs);
  return hipGetLastError();
}
extern "C" hipError_t wfk_rollout_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[WF_ROLLOUT_KERNELS] = {(const void*)wf_rollout_layout_kernel, (const void*)wf_rollout_reduce_kernel};
  if (kernel < 0 || kernel >= WF_ROLLOUT_KERNELS) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, fn[kernel]);
}
