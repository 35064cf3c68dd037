// wf_yawopt_kernels.hip — the loop around the step kernel that makes a coordinate search over yaw run on the device
// (include/wfyawopt.h).  Candidate evaluation is the existing wf_step on the optimiser's evaluator handle; these kernels are
// the glue, so that a whole optimisation is enqueued without a host round trip:
//
//   wf_yawopt_order_kernel    once per chunk: each slot's visit order (ext/wf_ext_kernels.h: wf_visit_order, shared with
//                             the robust search); one workgroup per slot, one thread per turbine.
//   wf_yawopt_wind_kernel     once per chunk, only for a parent with a wind per farm: each farm's wind repeated over its
//                             candidate rows (device to device), what wf_set_wind on the evaluator then takes.
//   wf_yawopt_advance_kernel  once per visit, select and expand fused: per slot, sum the power of the previous visit's K + 1
//                             candidates (caller's turbine order, float64), pick the winner (strictly greater than the
//                             incumbent; lowest index among equals), update the slot's best yaw, and write the next visit's
//                             [R][N] yaw block — the best yaw with one entry replaced per row.
//
// Lane layout of the advance kernel: ONE WAVE PER SLOT.  A slot's yaw block and power block are contiguous [R][N] floats
// (wf_yawopt.h), so the wave walks them with lane = consecutive float: every global load and store of the only traffic that
// scales as B K N is a full 256-byte line per wave instruction.  The power block is staged in LDS first, because the sums
// must run in a FIXED order (turbine 0, 1, ... in float64): lane k then adds row k from LDS — a stride-N walk that would
// touch a cache line per lane in global memory.  Trip counts are run-time values (no unrolled register arrays): no private
// segment, no spill (tests/test_yawopt.py reads the metadata).
#include <hip/hip_runtime.h>

#include "wf_yawopt.h"

__global__ __launch_bounds__(WF_ORDER_MAX_N) void wf_yawopt_order_kernel(const WfYawoptOrderArgs a) {
  __shared__ double sx[WF_ORDER_MAX_N];
  wf_visit_order(a, sx);
}

__global__ __launch_bounds__(256) void wf_yawopt_wind_kernel(const WfYawoptWindArgs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.sl.C * a.R) return;
  const int b = wf_slot_farm(a.sl, e / a.R);
  a.ews[e] = a.ws[b];
  a.ewd[e] = a.wd[b];
}

// Dynamic LDS per wave: 32 doubles (the candidates' power sums), 32 floats (the next candidates), N floats (the slot's best
// yaw), R N floats (the power block); the launcher sizes the region (a multiple of 16 bytes) and the waves per block.
// The phases shared with the robust search (best yaw, winner, candidates) are ext/wf_ext_kernels.h's.
#define YO_HDR_BYTES (WF_YAWOPT_ROWS_MAX * 8 + WF_YAWOPT_ROWS_MAX * 4)

__global__ __launch_bounds__(256) void wf_yawopt_advance_kernel(const WfYawoptAdvanceArgs a, int region_bytes) {
  extern __shared__ double yo_dyn[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int slot = blockIdx.x * (blockDim.x >> 6) + wv;
  const bool live = slot < a.sl.C;  // (wave-uniform; the barriers below, and those of the phases, are reached by every wave)
  char* region = (char*)yo_dyn + (size_t)wv * region_bytes;
  double* sums = (double*)region;
  float* cnd = (float*)(region + WF_YAWOPT_ROWS_MAX * 8);
  float* brow = (float*)(region + YO_HDR_BYTES);
  const int N = a.N, RN = a.R * a.N;
  float* pw = brow + N;
  const bool has_prev = a.prev.s >= 0, has_next = a.next.s >= 0;
  const size_t blk0 = (size_t)slot * RN;

  // ---- the slot's best yaw and the previous visit's power block -> LDS (coalesced) ----
  if (live) {
    wf_advance_load_best(a, slot, lane, brow);
    if (has_prev) {
      const int n_load = (a.prev.K + 1) * N;
      for (int i = lane; i < n_load; i += 64) pw[i] = a.power[blk0 + i];
    }
  }
  __syncthreads();
  // ---- farm power of each candidate: lane k sums row k, caller's turbine order, float64 ----
  if (live && has_prev && lane <= a.prev.K) {
    const float* row = pw + lane * N;
    double s = 0.0;
    for (int t = 0; t < N; ++t) s += (double)row[t];
    sums[lane] = s;
  }
  __syncthreads();
  wf_advance_pick(a, slot, lane, live, sums, brow);
  // ---- the next visit's candidates, then its yaw block: the best yaw, one entry replaced per candidate row ----
  const int tn = wf_advance_candidates(a, slot, lane, live, brow, cnd);
  __syncthreads();
  if (live && has_next) {
    for (int i = lane; i < RN; i += 64) {
      const int k = i / N, t = i - k * N;
      float v = brow[t];
      if (t == tn && k >= 1 && k <= a.next.K) v = cnd[k - 1];
      a.yaw[blk0 + i] = v;
    }
  } else if (live && slot < a.sl.n_slots) {
    wf_advance_write_best(a, slot, lane, brow);
  }
}

extern "C" hipError_t wfk_launch_yawopt_order(const WfYawoptOrderArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(wf_yawopt_order_kernel, dim3(a->sl.C), dim3(((a->N + 63) / 64) * 64), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_yawopt_wind(const WfYawoptWindArgs* a, hipStream_t s) {
  const int n = a->sl.C * a->R;
  hipLaunchKernelGGL(wf_yawopt_wind_kernel, dim3((n + 255) / 256), dim3(256), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_yawopt_advance(const WfYawoptAdvanceArgs* a, hipStream_t s) {
  const int region = (YO_HDR_BYTES + 4 * a->N * (a->R + 1) + 15) & ~15;
  int wpb = 49152 / region;  // waves (= slots) per block: what fits in 48 KiB of LDS, at most 4
  wpb = wpb < 1 ? 1 : (wpb > 4 ? 4 : wpb);
  hipLaunchKernelGGL(wf_yawopt_advance_kernel, dim3((a->sl.C + wpb - 1) / wpb), dim3(64 * wpb), (size_t)region * wpb, s, *a, region);
  return hipGetLastError();
}
