// wf_calib_kernels.hip — the one kernel around the step kernel that makes wake-model calibration run on the device
// (include/wfcalib.h: candidate parameter sets scored against measured powers, and the cross-entropy fit over the eighteen
// fields).  The farm solve is the existing wf_step on the object's evaluator handle, which holds a table of WfResolveConsts per
// (slot, candidate); this kernel is the glue between two steps, so that a whole run is enqueued without a host read:
//
//   wf_calib_advance_kernel  I + 1 launches per chunk, ONE WORKGROUP PER SLOT, 1024 threads.  Launch v
//     REDUCES iteration v - 1 (v > 0).  Thread r of the slot's R = S C rows adds its row's weighted squared residuals in
//       ascending t and leaves the sum in the slot's row losses (global: R may be 65 536); thread s adds candidate s's C row
//       losses in ascending c — +inf for an invalid candidate — and leaves the loss in LDS; the winner is the planner's
//       fixed-order tree, for the lowest loss: every thread over its own s ascending, then a tree over the threads in LDS;
//       thread s counts rank_s over the S losses in LDS and flags the elites; thread f of the eighteen fields adds the elites'
//       field in ascending s, divides once by E and stores the mean, and copies the winner's field where the winner is not
//       candidate 0; the winner's C N powers go to the slot's best rows, whole lines.
//     LAYS OUT iteration v (v < I).  Thread (s, f), f fastest, writes field f of candidate s: the best set's (s = 0), the mean's
//       (s = 1) or the mean plus the width times a deviate of its own Philox counter (s >= 2, ext/wf_deviate.h), clipped; for a
//       score the caller's set.  Then thread s judges candidate s and writes the set-owned members of entry slot S + s of the
//       evaluator's table (modelset/wf_resolve_set.h) — the starting set's for an invalid candidate.  Launch 0 seeds the
//       slot's state first and writes every row's wind and yaw: they are the observations' in every iteration.
//     WRITES THE OUTPUTS instead (v = I), whole lines.
//
// The entries of the table are 500-odd bytes apart and a thread writes the forty doubles a set owns into its own: the stores of
// a wave do not share lines.  They are S 320 bytes per slot and launch against the S C N 4 bytes the step then writes; staging
// them through LDS would not be seen (tools/calib_timing.py measures the glue).
// LDS is static: 8 KiB of losses, 12 KiB of the tree, 1 KiB of elite flags.  Trip counts are run-time values and a set is held in
// named registers: no private segment (tests/test_calib.py reads the metadata); every barrier sits in block-uniform control
// flow — the branches around them test kernel arguments and the run's block only.  The library is built with
// -ffp-contract=off: the residual's division, square, weight and sum, and the candidate's two products and sum, stay single
// roundings, as in the NumPy restatement (tests/calib_ref.py).
#include <hip/hip_runtime.h>

#include <climits>

#include "../ext/wf_deviate.h"
#include "../modelset/wf_resolve_set.h"
#include "wf_calib.h"

#define WF_CALIB_THREADS 1024  // (one workgroup per slot may be the whole grid, G = 1: sixteen waves hide the rows' load latency)

__device__ __forceinline__ double* wf_fields(wf_model_set* s) { return reinterpret_cast<double*>(s); }
__device__ __forceinline__ const double* wf_fields(const wf_model_set* s) { return reinterpret_cast<const double*>(s); }

// The phases below read the run's block (WfCalibRun, device memory) and name the slot's problem themselves, where they use
// it: what a phase holds in scalar registers dies with it.
// the slot's problem — its block of the caller's arrays: base + slot for the chunk's own slots, the chunk's first beyond
__device__ __forceinline__ int wf_calib_problem(const WfSlots& sl, int slot) { return sl.base + (slot < sl.n_slots ? slot : 0); }

// launch 0: the slot's state, and every row's wind and yaw
__device__ __forceinline__ void wf_calib_seed(const WfCalibRun& a, const WfSlots& sl) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  const int g = wf_calib_problem(sl, slot);
  const int N = a.N, C = a.C, R = a.S * C;
  WfCalibSlot& st = a.state[slot];
  if (a.fit) {
    const double* init = wf_fields(a.sets + (size_t)g * a.sets_stride);
    if (tid < WF_CALIB_FIELDS) {
      const double x = init[tid];
      wf_fields(&st.mu)[tid] = x; wf_fields(&st.best)[tid] = x; wf_fields(&st.init)[tid] = x;
    }
  }
  if (tid == 0) { st.best_loss = HUGE_VAL; st.init_loss = HUGE_VAL; st.n_invalid = 0; }
  const double* __restrict__ ws = a.ws + (size_t)g * C;
  const double* __restrict__ wd = a.wd + (size_t)g * C;
  for (int r = tid; r < R; r += nth) {
    const int c = r % C;
    a.ews[(size_t)slot * R + r] = ws[c];
    a.ewd[(size_t)slot * R + r] = wd[c];
  }
  const float* __restrict__ yaw = a.yaw + (size_t)g * C * N;
  float* __restrict__ out = a.yaw_ev + (size_t)slot * R * N;
  const int CN = C * N;
  for (size_t e = tid; e < (size_t)R * N; e += nth) out[e] = yaw[e % CN];
}

// reduce iteration v - 1: loss [S] (LDS), bv / bi [threads], el [S]; leaves the winner's loss in bv[0], its index in bi[0]
__device__ __forceinline__ void wf_calib_reduce(const WfCalibRun& a, const WfSlots& sl, int v, double* loss, double* bv, int* bi,
                                                unsigned char* el) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  const int g = wf_calib_problem(sl, slot);
  const int N = a.N, S = a.S, C = a.C, R = S * C;
  const double scale = a.scale;
  double* const row_loss = a.row_loss + (size_t)slot * R;
  {
    const float* __restrict__ pw = a.power_ev + (size_t)slot * R * N;
    const double* __restrict__ obs = a.power + (size_t)g * C * N;
    const double* __restrict__ wgt = a.weight ? a.weight + (size_t)g * C * N : nullptr;
    for (int r = tid; r < R; r += nth) {
      const int c = r % C;
      const float* __restrict__ p = pw + (size_t)r * N;
      double acc = 0.0;
#pragma unroll 8  // (the loads of eight turbines in flight: the sum is a dependent chain, and the block is alone on its CU)
      for (int t = 0; t < N; ++t) {
        const double q = ((double)p[t] - obs[c * N + t]) / scale;
        const double w = wgt ? wgt[c * N + t] : 1.0;
        acc += w == 0.0 ? 0.0 : w * (q * q);  // (a masked entry adds +0 whatever stands there — a NaN power too)
      }
      row_loss[r] = acc;
    }
  }
  __syncthreads();  // (row losses in global memory: other threads of the block read them below)
  const wf_model_set* cand = a.cand + (size_t)slot * S;
  double best_v = HUGE_VAL;
  int best_s = INT_MAX;
  for (int s = tid; s < S; s += nth) {
    double L = 0.0;
    for (int c = 0; c < C; ++c) L += row_loss[s * C + c];
    // (+inf for an invalid candidate, and for a loss that is not finite — a NaN observation under a positive weight, a solve
    // that left the model's domain: a NaN compares false with everything, would rank FIRST and would leave the tree without a winner)
    if (!wf_model_set_valid(cand[s]) || !(fabs(L) < HUGE_VAL)) L = HUGE_VAL;
    loss[s] = L;
    if (L < best_v || (L == best_v && s < best_s)) { best_v = L; best_s = s; }
  }
  bv[tid] = best_v;
  bi[tid] = best_s;
  __syncthreads();
  for (int h = nth >> 1; h > 0; h >>= 1) {  // (block-uniform)
    if (tid < h) {
      const double x = bv[tid + h];
      const int s = bi[tid + h];
      if (x < bv[tid] || (x == bv[tid] && s < bi[tid])) { bv[tid] = x; bi[tid] = s; }
    }
    __syncthreads();
  }
  if (!a.fit) return;  // (block-uniform: a score has no update)
  const int E = a.E;
  for (int s = tid; s < S; s += nth) {
    const double ls = loss[s];
    int rank = 0;
    for (int j = 0; j < S; ++j) {
      const double lj = loss[j];
      rank += (lj < ls) || (lj == ls && j < s);
    }
    el[s] = rank < E;
  }
  __syncthreads();
  const int w = bi[0] == INT_MAX ? 0 : bi[0];  // (every loss is a number by now, +inf at worst, and candidate 0 wins among equals: never taken)
  const bool take = w != 0 || v == 1;  // (iteration 0's winner founds the best rows, candidate 0 included)
  WfCalibSlot& st = a.state[slot];
  if (tid < WF_CALIB_FIELDS) {
    double sum = 0.0;
    for (int s = 0; s < S; ++s)
      if (el[s]) sum += wf_fields(cand + s)[tid];
    wf_fields(&st.mu)[tid] = sum / (double)E;
    if (w != 0) wf_fields(&st.best)[tid] = wf_fields(cand + w)[tid];
  }
  if (tid == 0) {
    if (v == 1) st.init_loss = loss[0];
    if (take) st.best_loss = bv[0];
    if ((unsigned)slot < (unsigned)sl.n_slots && a.history) a.history[(size_t)g * a.I + (v - 1)] = bv[0];
  }
  if (take) {
    const int CN = C * N;
    const float* __restrict__ src = a.power_ev + ((size_t)slot * R + (size_t)w * C) * N;
    float* __restrict__ dst = a.fit_rows + (size_t)slot * CN;
    for (int e = tid; e < CN; e += nth) dst[e] = src[e];
  }
}

// lay out iteration v: candidates, validity, the table's entries; bi [threads] serves the count of invalid candidates
__device__ __forceinline__ void wf_calib_layout(const WfCalibRun& a, const WfSlots& sl, int v, double sigma, int* bi) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  const int g = wf_calib_problem(sl, slot);
  const int S = a.S;
  WfCalibSlot& st = a.state[slot];
  wf_model_set* const cand = a.cand + (size_t)slot * S;
  if (a.fit) {
    const unsigned long long hi32 = (unsigned long long)(unsigned)g << 32;
    for (int q = tid; q < S * WF_CALIB_FIELDS; q += nth) {
      const int s = q / WF_CALIB_FIELDS, f = q - s * WF_CALIB_FIELDS;
      double x;
      if (s == 0) {
        x = wf_fields(&st.best)[f];
      } else {
        x = wf_fields(&st.mu)[f];
        if (s >= 2) {
          const double lo = a.lo[f], hi = a.hi[f];
          const double z = wf_deviate(a.seed, hi32 | (unsigned)q, (unsigned)v);
          x = x + (sigma * (hi - lo)) * z;
          x = x < lo ? lo : x;
          x = x > hi ? hi : x;
          x = lo == hi ? lo : x;
        }
      }
      wf_fields(cand)[q] = x;
    }
  } else {
    const double* __restrict__ src = wf_fields(a.sets + (size_t)g * a.sets_stride);
    for (int q = tid; q < S * WF_CALIB_FIELDS; q += nth) wf_fields(cand)[q] = src[q];
  }
  __syncthreads();  // (the candidates in global memory: thread s reads the eighteen fields other threads wrote)
  int bad = 0;
  for (int s = tid; s < S; s += nth) {
    wf_model_set c = cand[s];
    if (!wf_model_set_valid(c)) {  // (a score's sets are validated on the host: never taken there)
      ++bad;
      c = st.init;
    }
    wf_resolve_set_flow(c, a.kappa, a.tab + (size_t)slot * S + s);
  }
  for (int s = tid; s < S; s += nth) {  // (a loop of its own: modelset/wf_resolve_set.h says why)
    const double veer = wf_model_set_valid(cand[s]) ? cand[s].veer : st.init.veer;
    wf_resolve_set_veer(veer, a.tab + (size_t)slot * S + s);
  }
  bi[tid] = bad;
  __syncthreads();
  for (int h = nth >> 1; h > 0; h >>= 1) {  // (block-uniform; integers: any order gives the same count)
    if (tid < h) bi[tid] += bi[tid + h];
    __syncthreads();
  }
  if (tid == 0) st.n_invalid += bi[0];
}

// the last launch: the outputs, in whole lines
__device__ __forceinline__ void wf_calib_outputs(const WfCalibRun& a, const WfSlots& sl, const double* loss, double best_v, int best_s) {
  const int tid = threadIdx.x, nth = blockDim.x, slot = blockIdx.x;
  if (slot >= sl.n_slots) return;
  const int g = sl.base + slot;
  const int N = a.N, S = a.S, C = a.C, CN = C * N;
  if (!a.fit) {
    if (a.loss)
      for (int s = tid; s < S; s += nth) a.loss[(size_t)g * S + s] = loss[s];
    if (tid == 0 && a.best) a.best[g] = best_s == INT_MAX ? 0 : best_s;
    if (a.row_power) {
      const size_t n = (size_t)S * CN;
      const float* __restrict__ src = a.power_ev + (size_t)slot * n;
      float* __restrict__ dst = a.row_power + (size_t)g * n;
      for (size_t e = tid; e < n; e += nth) dst[e] = src[e];
    }
    return;
  }
  const WfCalibSlot& st = a.state[slot];
  if (tid < WF_CALIB_FIELDS) {
    if (a.best_set) wf_fields(a.best_set + g)[tid] = wf_fields(&st.best)[tid];
    if (a.mean) wf_fields(a.mean + g)[tid] = wf_fields(&st.mu)[tid];
  }
  if (tid == 0) {
    if (a.best_loss) a.best_loss[g] = st.best_loss;
    if (a.init_loss) a.init_loss[g] = st.init_loss;
    if (a.n_invalid) a.n_invalid[g] = st.n_invalid;
  }
  if (a.fit_power) {
    const float* __restrict__ src = a.fit_rows + (size_t)slot * CN;
    float* __restrict__ dst = a.fit_power + (size_t)g * CN;
    for (int e = tid; e < CN; e += nth) dst[e] = src[e];
  }
}

__global__ __launch_bounds__(WF_CALIB_THREADS) void wf_calib_advance_kernel(const WfCalibRun* __restrict__ run, const WfSlots sl, int v, int I,
                                                                             double sigma) {
  __shared__ double loss[WF_CALIB_MAX_S];
  __shared__ double bv[WF_CALIB_THREADS];
  __shared__ int bi[WF_CALIB_THREADS];
  __shared__ unsigned char el[WF_CALIB_MAX_S];
  if (v > 0) wf_calib_reduce(*run, sl, v, loss, bv, bi, el);  // (block-uniform)
  else wf_calib_seed(*run, sl);
  __syncthreads();  // (the slot's state in global memory: other threads of the block read it below)
  if (v < I) wf_calib_layout(*run, sl, v, sigma, bi);
  else wf_calib_outputs(*run, sl, loss, bv[0], bi[0]);
}

extern "C" hipError_t wfk_launch_calib_advance(const WfCalibRun* host, const WfCalibRun* dev, const WfSlots* sl, int v, double sigma,
                                               hipStream_t s) {
  hipLaunchKernelGGL(wf_calib_advance_kernel, dim3(sl->C), dim3(WF_CALIB_THREADS), 0, s, dev, *sl, v, host->I, sigma);
  return hipGetLastError();
}
extern "C" hipError_t wfk_calib_func_attributes(int kernel, hipFuncAttributes* a) {
  if (kernel != 0) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, (const void*)wf_calib_advance_kernel);
}
