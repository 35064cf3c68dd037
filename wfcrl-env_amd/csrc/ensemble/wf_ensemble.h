// wf_ensemble.h — the wind ensemble of include/wfscenario.h on the device, ONCE: what the four extensions that score something
// over M wind futures (scenario/, scenplan/, rollscen/, polscen/) share.  The path definition — the ramp rate from Philox
// stream 16, the recursion over ticks with the deviates of streams 17 and 18, clip and wrap — is the three scalar pieces
// below and nothing else; the workgroup-per-slot draw -> walk -> fill sequence is wf_ensemble_tiles; the rank / mean / tail
// mean / score passes are wf_member_statistics, and the choice wf_argmax_tree.  The kernels' argument structs embed
// WfEnsemble; ensemble/wf_ensemble_host.h fills and checks it.  The library is built with -ffp-contract=off: every product
// and sum below is one rounding, in the header's order (tests/scenario_ref.py restates it in NumPy).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "../ext/wf_deviate.h"
#include "../ext/wf_ext_kernels.h"
#include "../wf_philox.h"

#define WF_ENSEMBLE_TILE 2048  // (member, tick) pairs of a tile of wf_ensemble_tiles: two [M][Hs] arrays of doubles, 33 KiB at most

// what defines the paths of a chunk's slots
struct WfEnsemble {
  unsigned long long seed;
  double ws_revert, ws_sigma, wd_revert, wd_sigma, wd_ramp;
  double ws_lo, ws_hi;
  const double* anchor;   // [n_slots][2] (speed, direction) of this chunk, or null = the farm's current wind
  const double *ws, *wd;  // the parent's wind: (S_c, D_c)
  int wind_stride;        // 0 shared, 1 per farm
  int M, H;
};

// ---- the scalar pieces ----

// what a walk of farm b's members holds: where the latents start, what they revert to, the process and the bounds
struct WfEnsembleWalk {
  double Sc, Dc, Sa, Da;
  double ws_revert, ws_sigma, wd_revert, wd_sigma, ws_lo, ws_hi;
};
// `in` is the slot's input block (0 for a slot beyond the chunk's farms).  PIN: the values live in vector registers — for a
// workgroup per slot they are block-uniform, and held in scalar registers across the Philox rounds of the draws they would
// not fit (spilled scalar registers; the tests of the four extensions read the metadata).  The current wind is pinned
// before the anchor's select reads it
template <bool PIN>
__device__ __forceinline__ WfEnsembleWalk wf_ensemble_walk(const WfEnsemble& e, int b, size_t in) {
  WfEnsembleWalk w;
  w.Sc = e.ws[(size_t)b * e.wind_stride]; w.Dc = e.wd[(size_t)b * e.wind_stride];
  if (PIN) { WF_IN_VGPR(w.Sc); WF_IN_VGPR(w.Dc); }
  w.Sa = e.anchor ? e.anchor[in * 2] : w.Sc; w.Da = e.anchor ? e.anchor[in * 2 + 1] : w.Dc;
  w.ws_revert = e.ws_revert; w.ws_sigma = e.ws_sigma; w.wd_revert = e.wd_revert; w.wd_sigma = e.wd_sigma;
  w.ws_lo = e.ws_lo; w.ws_hi = e.ws_hi;
  if (PIN) {
    WF_IN_VGPR(w.Sa); WF_IN_VGPR(w.Da);
    WF_IN_VGPR(w.ws_revert); WF_IN_VGPR(w.ws_sigma); WF_IN_VGPR(w.wd_revert); WF_IN_VGPR(w.wd_sigma);
    WF_IN_VGPR(w.ws_lo); WF_IN_VGPR(w.ws_hi);
  }
  return w;
}

// member m's ramp rate: stream 16, counter (b << 32) | m
__device__ __forceinline__ double wf_ensemble_rate(const WfEnsemble& e, int b, int m) {
  unsigned r[4];
  philox4x32_10(e.seed, ((unsigned long long)b << 32) | (unsigned)m, 16u, r);
  return e.wd_ramp * (2.0 * u01(r[0], r[1]) - 1.0);
}

// the two deviates of (m, tick): streams 17 (speed) and 18 (direction), counter (b << 32) | (m * 64 + tick)
__device__ __forceinline__ void wf_ensemble_deviates(const WfEnsemble& e, int b, int m, int tick, double& z17, double& z18) {
  const unsigned long long ctr = ((unsigned long long)b << 32) | (unsigned)(m * 64 + tick);
  z17 = wf_deviate(e.seed, ctr, 17u);
  z18 = wf_deviate(e.seed, ctr, 18u);
}

// one tick of the recursion: the latents (x, y) advance to tick u + 1; the stored speed is clipped, the stored direction wrapped
__device__ __forceinline__ void wf_ensemble_tick(const WfEnsembleWalk& w, double rate, int u, double z17, double z18, double& x, double& y,
                                                 double& speed, double& dir) {
  x = (x + w.ws_revert * (w.Sa - x)) + w.ws_sigma * z17;
  const double mu = w.Da + rate * (double)(u + 1);
  y = (y + w.wd_revert * (mu - y)) + w.wd_sigma * z18;
  double d = fmod(y, 360.0);
  if (d < 0.0) d += 360.0;
  speed = fmin(fmax(x, w.ws_lo), w.ws_hi);
  dir = d;
}

// ---- the tiled body: ONE WORKGROUP PER SLOT, every thread of the block calls it.  The M member paths of the slot's farm go
// by in TILES of Ht ticks, two [M][Hs] arrays of doubles in `tile`, Hs = Ht | 1: (1) every thread draws the deviates of its
// (member, tick) pairs into the tile — the draws are not serial, the recursion is —; (2) thread m < M (M <= 64 <= nth), which
// keeps member m's latents and ramp rate in registers across the tiles, walks the tile's ticks and leaves the stored speed
// and direction in place; (3) after the barrier the threads fill the wind of the slot's K M H rows, row = (k M + m) H + h,
// thread r on row r — consecutive lanes read consecutive doubles of a member's LDS row and write consecutive doubles —, and
// wind_paths ([n_slots][M][H][2] of this chunk, or null), consecutive lanes on consecutive (speed, direction) pairs.  After
// its last barrier the tile is free and the rows' wind is visible to the block.  Every barrier sits in block-uniform control
// flow. ----
__device__ __forceinline__ void wf_ensemble_tiles(const WfEnsemble& e, const WfSlots& sl, int K, int Ht, int Hs, double* tile,
                                                  double* ews_chunk, double* ewd_chunk, double* wind_paths) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int M = e.M, H = e.H, MH = M * H, R = K * MH;
  double* sp = tile;         // [M][Hs] deviates of stream 17, then the stored speeds
  double* dr = sp + M * Hs;  // [M][Hs] ... of stream 18, then the stored directions
  const int slot = blockIdx.x;
  const int b = wf_slot_farm(sl, slot);
  const bool writes = slot < sl.n_slots;
  const size_t in = writes ? slot : 0;  // the slot's input block
  const WfEnsembleWalk w = wf_ensemble_walk<true>(e, b, in);  // (the walk's parameters in vector registers)
  const bool walker = tid < M;  // thread m keeps member m's state
  double x = w.Sc, y = w.Dc, rate = 0.0;
  if (walker) rate = wf_ensemble_rate(e, b, tid);
  double* __restrict__ ews = ews_chunk + (size_t)slot * R;
  double* __restrict__ ewd = ewd_chunk + (size_t)slot * R;
  double* __restrict__ paths = (writes && wind_paths) ? wind_paths + in * MH * 2 : nullptr;
  for (int h0 = 0; h0 < H; h0 += Ht) {  // (block-uniform)
    const int nt = H - h0 < Ht ? H - h0 : Ht;
    const int n = M * nt;
    for (int i = tid; i < n; i += nth) {
      const int m = i / nt, j = i - m * nt;
      wf_ensemble_deviates(e, b, m, h0 + j, sp[m * Hs + j], dr[m * Hs + j]);
    }
    __syncthreads();
    if (walker) {
      double* s = sp + tid * Hs;
      double* d = dr + tid * Hs;
      for (int j = 0; j < nt; ++j) wf_ensemble_tick(w, rate, h0 + j, s[j], d[j], x, y, s[j], d[j]);
    }
    __syncthreads();
    for (int r = tid; r < R; r += nth) {
      const int km = r / H, h = r - km * H, j = h - h0;
      if (j >= 0 && j < nt) {
        const int m = km % M;
        ews[r] = sp[m * Hs + j];
        ewd[r] = dr[m * Hs + j];
      }
    }
    if (paths) {
      for (int i = tid; i < n; i += nth) {
        const int m = i / nt, j = i - m * nt;
        const size_t o = ((size_t)m * H + h0 + j) * 2;
        paths[o] = sp[m * Hs + j];
        paths[o + 1] = dr[m * Hs + j];
      }
    }
    __syncthreads();  // (the next tile's draws, or what the caller keeps there, overwrite the tile; the rows' wind is visible to the block)
  }
}

// its launch: the ticks of a tile and the odd row stride; the tile takes sizeof(double) * 2 * M * Hs bytes
struct WfEnsembleTile {
  int Ht, Hs;
};
inline WfEnsembleTile wf_ensemble_tile(int M, int H) {
  int Ht = WF_ENSEMBLE_TILE / M;
  Ht = Ht > H ? H : Ht;
  return WfEnsembleTile{Ht, Ht | 1};
}

// ---- the member statistics (include/wfscenario.h: STATISTICS): every thread of the block calls it, behind the barrier that
// makes the K M member returns visible — member (k, m)'s at rets[(k M + m) stride] in LDS.  PASSES of nth / M whole
// candidates: thread (k, m) counts its rank over the M members of its candidate — (return, m) ascending, a count — and
// scatters its return to srt[k][rank] (a pass's [nth] doubles in LDS); thread k adds the mean in ascending m and the tail in
// ascending rank, forms the score, hands them to emit(k, mean, cvar, score) — which may overwrite candidate k's first return:
// it has been added, and ranked before the barriers — and keeps its argmax over ascending k.  Returns the thread's running
// best: (-inf, INT_MAX) where it had no candidate.  Every barrier sits in block-uniform control flow. ----
struct WfBest {
  double v;
  int k;
};
template <class EMIT>
__device__ __forceinline__ WfBest wf_member_statistics(const double* rets, int stride, int K, int M, int q, double lam, double* srt, EMIT emit) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int spp = nth / M;  // whole candidates per pass (M <= 64 <= nth)
  const int kk = tid / M, m = tid - kk * M;
  WF_IN_VGPR(lam);  // (as the walk's parameters: no spilled scalar register)
  WfBest best{-HUGE_VAL, INT_MAX};
  for (int k0 = 0; k0 < K; k0 += spp) {  // (block-uniform)
    const bool member = kk < spp && k0 + kk < K;
    double v = 0.0;
    int rank = 0;
    if (member) {
      const double* s = rets + (size_t)(k0 + kk) * M * stride;
      v = s[m * stride];
      for (int j = 0; j < M; ++j) {
        const double vj = s[j * stride];
        rank += (vj < v) || (vj == v && j < m);
      }
    }
    __syncthreads();  // (the previous pass's tails have been added)
    if (member) srt[kk * M + rank] = v;
    __syncthreads();
    if (tid < spp && k0 + tid < K) {
      const int k = k0 + tid;
      const double* s = rets + (size_t)k * M * stride;
      double sum = 0.0, tail = 0.0;
      for (int j = 0; j < M; ++j) sum += s[j * stride];
      for (int j = 0; j < q; ++j) tail += srt[tid * M + j];
      const double mean = sum / (double)M, cvar = tail / (double)q;
      const double score = ((1.0 - lam) * mean) + (lam * cvar);
      emit(k, mean, cvar, score);
      if (score > best.v || (score == best.v && k < best.k)) { best.v = score; best.k = k; }
    }
  }
  return best;
}

// ---- the choice: a fixed-order tree over the threads' running bests in bv / bi ([nth] doubles and ints in LDS; bv may be the
// statistics' srt: the leading barrier lets the last pass's tails be added first) — the larger score and among equal ones the
// lower index.  Leaves the winner's score in bv[0] and the winner in bi[0], visible to the block; wf_argmax_winner reads it
// where a thread needs it: 0 where no thread had a candidate. ----
__device__ __forceinline__ int wf_argmax_winner(const int* bi) { return bi[0] == INT_MAX ? 0 : bi[0]; }
__device__ __forceinline__ void wf_argmax_tree(WfBest best, double* bv, int* bi) {
  const int tid = threadIdx.x, nth = blockDim.x;
  __syncthreads();
  bv[tid] = best.v;
  bi[tid] = best.k;
  __syncthreads();
  for (int s = nth >> 1; s > 0; s >>= 1) {  // (block-uniform)
    if (tid < s) {
      const double v = bv[tid + s];
      const int k = bi[tid + s];
      if (v > bv[tid] || (v == bv[tid] && k < bi[tid])) { bv[tid] = v; bi[tid] = k; }
    }
    __syncthreads();
  }
}
