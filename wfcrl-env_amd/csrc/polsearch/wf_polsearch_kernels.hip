// wf_polsearch_kernels.hip — the device side of the policy-search extension (include/wfpolsearch.h has the definition,
// polsearch/wf_polsearch.h the buffers).  Two kernels stand between two runs of the scorer:
//   wf_polsearch_tiles_kernel    a workgroup per tile of 256 list positions.  The tile's [256][K] scores are contiguous: the
//       workgroup reads them 32 positions at a time, every lane consecutive doubles, into LDS (and copies them to
//       farm_scores[i]); thread k < K then adds its column in ascending position.  At one step of that walk the K threads read
//       K CONSECUTIVE doubles of one LDS row: a row read, free of bank conflicts at any K, so the rows carry no padding.
//   wf_polsearch_advance_kernel  launch v = 0 .. I, a grid of (passes along p) x (slices of WF_POLSEARCH_ROWS candidate rows).
//       Every workgroup first adds the tile sums in ascending tile and divides (thread k < K: T K doubles, a few KiB at most,
//       cheaper than a launch of its own), ranks the K fitnesses by counting in LDS and finds the winner, as the planner's kernel
//       does; workgroup (0, 0) writes fitness[v - 1] and winner[v - 1].  Then a thread per p — consecutive lanes consecutive p,
//       every load and store a whole line of floats — walks the K candidates of iteration v - 1 for the elite mean and width,
//       ONCE for the rows of its slice, and writes their elements of iteration v: row 0 the winner's bits, row 1 the mean, row
//       k >= 2 one Philox block each.  Launch 0 seeds from mean0 and sigma0; launch I is slice 0 alone and writes best_params,
//       mean and sigma.
// Wave64-aware only in that nothing depends on the wave width: no cross-lane operation, no floating-point atomics.  Compiled
// under -fno-fast-math -ffp-contract=off: every product and sum is rounded separately, sqrt(double) is the device library's
// correctly rounded one.
#include "../ext/wf_deviate.h"
#include "../ext/wf_ext_kernels.h"
#include "wf_polsearch.h"

__global__ __launch_bounds__(WF_POLSEARCH_THREADS) void wf_polsearch_tiles_kernel(const WfPolSearchRun r, int i) {
  extern __shared__ double ps_tile[];  // [WF_POLSEARCH_SUB][K]
  const int K = r.K, tid = threadIdx.x;
  const int first = blockIdx.x * WF_POLSEARCH_TILE;
  const int count = r.n - first < WF_POLSEARCH_TILE ? r.n - first : WF_POLSEARCH_TILE;
  double* const copy = r.farm_scores ? r.farm_scores + (size_t)i * r.n * K : nullptr;
  double acc = 0.0;
  for (int sub = 0; sub < count; sub += WF_POLSEARCH_SUB) {  // (block-uniform bounds)
    const int rows = count - sub < WF_POLSEARCH_SUB ? count - sub : WF_POLSEARCH_SUB;
    const size_t base = (size_t)(first + sub) * K;
    for (int e = tid; e < rows * K; e += WF_POLSEARCH_THREADS) {
      const double v = r.scores[base + e];
      ps_tile[e] = v;
      if (copy) copy[base + e] = v;
    }
    __syncthreads();
    if (tid < K)
      for (int q = 0; q < rows; ++q) acc = acc + ps_tile[q * K + tid];
    __syncthreads();
  }
  if (tid < K) r.tile[(size_t)blockIdx.x * K + tid] = acc;
}

__global__ __launch_bounds__(WF_POLSEARCH_THREADS) void wf_polsearch_advance_kernel(const WfPolSearchRun r, int v) {
  extern __shared__ double ps_fit[];  // [K] doubles: the fitness; then [K] ints: 1 = elite; then the winner
  const int K = r.K, P = r.P, tid = threadIdx.x, slice = blockIdx.y;
  int* const elite = reinterpret_cast<int*>(ps_fit + K);
  int* const win = elite + K;
  if (v > 0) {  // (block-uniform)
    if (tid < K) {
      double f = 0.0;
      for (int t = 0; t < r.T; ++t) f = f + r.tile[(size_t)t * K + tid];
      ps_fit[tid] = f / (double)r.n;
    }
    __syncthreads();
    if (tid < K) {
      const double ninf = -__builtin_huge_val();
      const double fk = ps_fit[tid], gk = __builtin_isfinite(fk) ? fk : ninf;
      int rank = 0;
      for (int j = 0; j < K; ++j) {  // (a broadcast read per j)
        const double fj = ps_fit[j], gj = __builtin_isfinite(fj) ? fj : ninf;
        rank += (gj > gk) || (gj == gk && j < tid);
      }
      elite[tid] = rank < r.E;
      if (rank == 0) *win = tid;
    }
    __syncthreads();
    if (blockIdx.x == 0 && slice == 0) {
      if (tid < K && r.fitness) r.fitness[(size_t)(v - 1) * K + tid] = ps_fit[tid];
      if (tid == 0) {
        if (r.winner) r.winner[v - 1] = *win;
        if (v == 1 && r.init_fitness) *r.init_fitness = ps_fit[0];
        if (v == r.I && r.best_fitness) *r.best_fitness = ps_fit[*win];
      }
    }
  }
  const float* const prev = r.cand + (size_t)((v - 1) & 1) * K * P;  // (read only when v > 0)
  float* const cur = r.cand + (size_t)(v & 1) * K * P;
  const int w = v > 0 ? *win : 0;
  const double dE = (double)r.E;
  // this workgroup's candidate rows k0 .. k1 - 1 (block-uniform); slice 0 holds rows 0 and 1, and is the only one of launch I
  const int k0 = slice * WF_POLSEARCH_ROWS;
  const int k1 = v == r.I ? 2 : (k0 + WF_POLSEARCH_ROWS < K ? k0 + WF_POLSEARCH_ROWS : K);
  for (int p = blockIdx.x * WF_POLSEARCH_THREADS + tid; p < P; p += gridDim.x * WF_POLSEARCH_THREADS) {
    float mu, sg;  // the mean and the width iteration v draws with: once per element, for all the rows of the slice
    if (v == 0) {
      mu = r.mean0[p];
      sg = r.sigma0[p];
    } else {
      double s = 0.0;
      for (int j = 0; j < K; ++j) {  // (every row is loaded, the elites' are added: loads that do not wait for a branch)
        const double x = (double)prev[(size_t)j * P + p];
        s = elite[j] ? s + x : s;
      }
      const double m = s / dE;
      double q = 0.0;
      for (int j = 0; j < K; ++j) {
        const double d = (double)prev[(size_t)j * P + p] - m;
        q = elite[j] ? q + d * d : q;
      }
      mu = (float)m;
      sg = (float)(sqrt(q / dE) + r.sigma_min);
    }
    const float inc = k0 > 0 ? 0.0f : (v > 0 ? prev[(size_t)w * P + p] : mu);  // (row 0's: slice 0 only)
    if (v == r.I) {
      if (r.best_params) r.best_params[p] = inc;
      if (r.mean) r.mean[p] = mu;
      if (r.sigma) r.sigma[p] = sg;
      continue;
    }
    if (k0 == 0 && r.sigma_history) r.sigma_history[(size_t)v * P + p] = sg;
    for (int k = k0; k < k1; ++k) {
      float val = k == 0 ? inc : mu;
      if (k >= 2) {
        unsigned long long seed = r.seed;  // (block-uniform: held in vector registers across the Philox rounds, ext/wf_ext_kernels.h)
        unsigned row = (unsigned)k, stream = (unsigned)v;
        WF_IN_VGPR(seed); WF_IN_VGPR(row); WF_IN_VGPR(stream);
        const double z = wf_deviate(seed, ((unsigned long long)row << 32) | (unsigned)p, stream);
        const double prod = (double)sg * z;
        val = (float)((double)mu + prod);
      }
      cur[(size_t)k * P + p] = val;
      if (r.candidates) r.candidates[((size_t)v * K + k) * P + p] = val;
    }
  }
}

extern "C" hipError_t wfk_launch_polsearch_tiles(const WfPolSearchRun* r, int i, hipStream_t s) {
  const size_t lds = sizeof(double) * WF_POLSEARCH_SUB * r->K;
  hipLaunchKernelGGL(wf_polsearch_tiles_kernel, dim3(r->T), dim3(WF_POLSEARCH_THREADS), lds, s, *r, i);
  return hipGetLastError();
}

extern "C" hipError_t wfk_launch_polsearch_advance(const WfPolSearchRun* r, int v, hipStream_t s) {
  int gx = (r->P + WF_POLSEARCH_THREADS - 1) / WF_POLSEARCH_THREADS;
  if (gx > WF_POLSEARCH_PASS_BLOCKS) gx = WF_POLSEARCH_PASS_BLOCKS;
  const size_t lds = sizeof(double) * r->K + sizeof(int) * (r->K + 1);
  hipLaunchKernelGGL(wf_polsearch_advance_kernel, dim3(gx, v < r->I ? (r->K + WF_POLSEARCH_ROWS - 1) / WF_POLSEARCH_ROWS : 1), dim3(WF_POLSEARCH_THREADS), lds, s, *r, v);
  return hipGetLastError();
}

extern "C" hipError_t wfk_polsearch_func_attributes(int kernel, hipFuncAttributes* a) {
  switch (kernel) {
    case 0: return hipFuncGetAttributes(a, (const void*)wf_polsearch_tiles_kernel);
    case 1: return hipFuncGetAttributes(a, (const void*)wf_polsearch_advance_kernel);
    default: return hipErrorInvalidValue;
  }
}
