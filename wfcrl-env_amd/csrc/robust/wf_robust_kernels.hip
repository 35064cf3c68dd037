// wf_robust_kernels.hip — the kernels around the step kernel that make expected power under wind-direction uncertainty, and
// the coordinate search that maximises it, run on the device (include/wfrobust.h).  The farm solve is the existing wf_step
// on the object's evaluator handles; these kernels are the glue, so that a whole search is enqueued without a host read:
//
//   wf_robust_order_kernel    once per chunk: each slot's visit order under its NOMINAL direction (ext/wf_ext_kernels.h:
//                             wf_visit_order, shared with the yaw optimiser); one workgroup per slot, one thread per turbine.
//   wf_robust_layout_kernel   once per chunk: the wind of every evaluator row (slot, candidate, member): ws and
//                             wd + delta[m] from the parent's device wind; for wf_robust_evaluate also the row's yaw (the
//                             farm's row, with the FIXED-frame offset).  ONE WAVE PER ROW, lanes over turbines in a loop: a
//                             row's N floats are contiguous, so every store is a whole line.
//   wf_robust_rowsum_kernel   once per visit: the farm power of every row — its N float32 powers added in caller order in
//                             float64: the staged row sum of ext/wf_ext_kernels.h (wf_staged_rowsum), shared with the rose.
//   wf_robust_advance_kernel  once per visit, select and expand fused: per slot, E of the previous visit's K + 1 candidates
//                             from the [R][M] row sums in member order, the winner (strictly greater than the incumbent;
//                             lowest index among equals), the slot's best yaw, and the next visit's [R][M][N] yaw block —
//                             the best yaw with one entry replaced per candidate row, plus delta[m] in the FIXED frame.
//   wf_robust_expect_kernel   wf_robust_evaluate's outputs: per farm E, the per-turbine expectation and the member powers.
//
// Lane layout of the advance kernel: ONE WAVE PER SLOT.  A slot's power block is M times that of the yaw optimiser — 32
// rows x 9 members x 80 turbines are 92 KB — so it is never staged: the row sums have their own pass and this kernel reads
// doubles only, (K + 1) M of them per slot.  Its one large stream, the slot's contiguous [R][M][N] yaw block, is written
// with lane = consecutive float: a full 256-byte line per wave instruction.  There is no size-dependent second path.
// Trip counts are run-time values (no unrolled register arrays): no private segment, no spill, no out-of-line call
// (tests/test_robust.py reads the metadata).  The library is built with -ffp-contract=off: a product and a sum stay two
// roundings, as in the NumPy restatement.
#include <hip/hip_runtime.h>

#include "wf_robust.h"

namespace {

// the yaw member m is stepped with (include/wfrobust.h: FRAME)
__device__ __forceinline__ float rb_member_yaw(float yaw, int frame, double delta) {
  return frame == WF_ROBUST_FIXED ? (float)((double)yaw + delta) : yaw;
}

}  // namespace

__global__ __launch_bounds__(WF_ORDER_MAX_N) void wf_robust_order_kernel(const WfRobustOrderArgs a) {
  __shared__ double sx[WF_ORDER_MAX_N];
  wf_visit_order(a, sx);
}

__global__ __launch_bounds__(256) void wf_robust_layout_kernel(const WfRobustLayoutArgs a) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int M = a.mb.M, RM = a.R * M;
  if (e >= a.sl.C * RM) return;
  const int slot = e / RM, m = e % M;
  const int b = wf_slot_farm(a.sl, slot);
  const double dm = a.mb.delta[m];
  if (lane == 0) {
    a.ews[e] = a.ws[(size_t)b * a.wind_stride];
    a.ewd[e] = a.wd[(size_t)b * a.wind_stride] + dm;
  }
  if (!a.write_yaw) return;
  const int N = a.N;
  const float* __restrict__ src = a.yaw_in ? a.yaw_in + (size_t)(slot < a.sl.n_slots ? slot : 0) * N : nullptr;
  float* __restrict__ row = a.yaw + (size_t)e * N;
  for (int t = lane; t < N; t += 64) row[t] = rb_member_yaw(src ? src[t] : 0.0f, a.mb.frame, dm);
}

__global__ __launch_bounds__(64) void wf_robust_rowsum_kernel(const WfRobustRowsumArgs a, int rows_per_block, int stride) {
  extern __shared__ float rb_pw[];
  const int lane = threadIdx.x;
  const int e0 = blockIdx.x * rows_per_block;
  int nr = a.n_rows - e0;
  nr = nr > rows_per_block ? rows_per_block : nr;
  const double sum = wf_staged_rowsum(a.power + (size_t)e0 * a.N, nr, a.N, stride, rb_pw, lane);
  if (lane < nr) a.rowsum[e0 + lane] = sum;
}

// Dynamic LDS per wave: 32 doubles (the candidates' E), 32 floats (the next candidates), N floats (the slot's best yaw); the
// launcher sizes the region (a multiple of 16 bytes).  The phases shared with the yaw optimiser (best yaw, winner,
// candidates) are ext/wf_ext_kernels.h's.
#define RB_HDR_BYTES (WF_ROBUST_ROWS_MAX * 8 + WF_ROBUST_ROWS_MAX * 4)

__global__ __launch_bounds__(256) void wf_robust_advance_kernel(const WfRobustAdvanceArgs a, int region_bytes) {
  extern __shared__ double rb_dyn[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int slot = blockIdx.x * 4 + wv;
  const bool live = slot < a.sl.C;  // (wave-uniform; the barriers below, and those of the phases, are reached by every wave)
  char* region = (char*)rb_dyn + (size_t)wv * region_bytes;
  double* sums = (double*)region;
  float* cnd = (float*)(region + WF_ROBUST_ROWS_MAX * 8);
  float* brow = (float*)(region + RB_HDR_BYTES);
  const int N = a.N, M = a.mb.M, RM = a.R * M;
  const bool has_prev = a.prev.s >= 0, has_next = a.next.s >= 0;

  // ---- the slot's best yaw -> LDS; E of each candidate of the previous visit: lane k, members in index order, float64 ----
  if (live) {
    wf_advance_load_best(a, slot, lane, brow);
    if (has_prev && lane <= a.prev.K) {
      const double* __restrict__ rs = a.rowsum + ((size_t)slot * a.R + lane) * M;
      double e = 0.0;
      for (int m = 0; m < M; ++m) e += a.mb.w[m] * rs[m];
      sums[lane] = e;
    }
  }
  __syncthreads();
  wf_advance_pick(a, slot, lane, live, sums, brow);
  // ---- the next visit's candidates, then its yaw block: per (row, member) the best yaw, one entry replaced per candidate row ----
  const int tn = wf_advance_candidates(a, slot, lane, live, brow, cnd);
  __syncthreads();
  if (live && has_next) {
    float* __restrict__ blk = a.yaw + (size_t)slot * RM * N;
    const int n_store = RM * N;
    for (int i = lane; i < n_store; i += 64) {
      const int km = i / N, t = i - km * N;
      const int k = km / M, m = km - k * M;
      float v = brow[t];
      if (t == tn && k >= 1 && k <= a.next.K) v = cnd[k - 1];
      blk[i] = rb_member_yaw(v, a.mb.frame, a.mb.delta[m]);
    }
  } else if (live && slot < a.sl.n_slots) {
    wf_advance_write_best(a, slot, lane, brow);
  }
}

__global__ __launch_bounds__(256) void wf_robust_expect_kernel(const WfRobustExpectArgs a) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= a.sl.n_slots) return;
  const int N = a.N, M = a.mb.M;
  const double* __restrict__ w = a.mb.w;
  const double* __restrict__ rs = a.rowsum + (size_t)slot * M;
  if (a.turbine) {
    const float* __restrict__ pw = a.power + (size_t)slot * M * N;
    for (int t = lane; t < N; t += 64) {
      double e = 0.0;
      for (int m = 0; m < M; ++m) e += w[m] * (double)pw[(size_t)m * N + t];
      a.turbine[(size_t)slot * N + t] = e;
    }
  }
  if (a.member)
    for (int m = lane; m < M; m += 64) a.member[(size_t)slot * M + m] = (float)rs[m];
  if (a.expected && lane == 0) {
    double e = 0.0;
    for (int m = 0; m < M; ++m) e += w[m] * rs[m];
    a.expected[slot] = e;
  }
}

extern "C" hipError_t wfk_launch_robust_order(const WfRobustOrderArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(wf_robust_order_kernel, dim3(a->sl.C), dim3(((a->N + 63) / 64) * 64), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_robust_layout(const WfRobustLayoutArgs* a, hipStream_t s) {
  const int n = a->sl.C * a->R * a->mb.M;
  hipLaunchKernelGGL(wf_robust_layout_kernel, dim3((n + 3) / 4), dim3(256), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_robust_rowsum(const WfRobustRowsumArgs* a, hipStream_t s) {
  const WfRowsumLaunch l = wf_rowsum_launch(a->n_rows, a->N);
  hipLaunchKernelGGL(wf_robust_rowsum_kernel, dim3(l.blocks), dim3(64), l.lds_bytes, s, *a, l.rows_per_block, l.stride);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_robust_advance(const WfRobustAdvanceArgs* a, hipStream_t s) {
  const int region = (RB_HDR_BYTES + 4 * a->N + 15) & ~15;  // (N <= 256: at most 1408 bytes a wave)
  hipLaunchKernelGGL(wf_robust_advance_kernel, dim3((a->sl.C + 3) / 4), dim3(256), (size_t)region * 4, s, *a, region);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_robust_expect(const WfRobustExpectArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(wf_robust_expect_kernel, dim3((a->sl.n_slots + 3) / 4), dim3(256), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_robust_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[WF_ROBUST_KERNELS] = {(const void*)wf_robust_order_kernel, (const void*)wf_robust_layout_kernel,
                                       (const void*)wf_robust_rowsum_kernel, (const void*)wf_robust_advance_kernel,
                                       (const void*)wf_robust_expect_kernel};
  if (kernel < 0 || kernel >= WF_ROBUST_KERNELS) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, fn[kernel]);
}
