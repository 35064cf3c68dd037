// wf_probe_kernels.hip — flow sampling at arbitrary points (include/wfprobe.h), float64 on the device.
//
//   wf_probe_state_kernel   one farm per workgroup: rotation and stable rank sort as wf_geometry_kernel does them, then the
//                           full sequential Gauss-Curl-Hybrid solve [A.3-1 .. A.3-9] following oracle/floris_gch_numpy.py
//                           step by step.  One thread per (sorted) turbine owns that target's 9-point wake^2 / V / W (a column
//                           of LDS) and its 3-column TI (registers); the thread of source i publishes the source's record
//                           through LDS, two barriers per source.  Leaves a per-source state record (wf_probe.h) in global memory.
//                           Latency-shaped, not the hot path.
//   wf_probe_sample_kernel  the hot path: a block stages its farm's records in LDS (160 bytes per turbine), one lane per
//                           point: rotate the point, walk the sources in sorted order (wave-uniform LDS reads: broadcasts),
//                           stop at the first source downstream of the point, accumulate wake^2, v, w in registers.
//
// Both kernels share the per-point arithmetic below, so a probe that sits on a rotor-grid point of a turbine goes through
// the same instructions as that grid point in the farm solve.  No function call, no spill, no private segment (the reason
// is the one csrc/wf_resolve.hip states: a kernel with a private segment pays ~20 us per launch on this chip).
#include <hip/hip_runtime.h>

#include "../wf_device.h"
#include "../wf_f64_math.h"
#include "wf_probe.h"

namespace {

// ---- a height above ground: what the transverse terms [A.3-4] need of it --------------------------------------------
struct PrHeight {
  double zc[6];   // vertical offsets to the three vortices (top, bottom, wake rotation) and their ground mirrors, num_eps included
  double ez[6];   // exp(-zc^2 / eps^2): the z part of the vortex core factor
  double dec_a;   // 4 nu / Uinf: decay = eps^2 / (dec_a dx + eps^2)
};

__device__ __forceinline__ void pr_height(const WfProbeConsts& c, double z, double nu1, PrHeight& h) {
  const double R = 0.5 * c.r.D, HH = c.r.HH, ne = c.r.num_eps;
  const double hs[3] = {HH + R, HH - R, HH};
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    h.zc[v] = z - hs[v] + ne;
    h.zc[3 + v] = z + hs[v] + ne;
  }
#pragma unroll
  for (int v = 0; v < 6; ++v) h.ez[v] = exp_lean(-(h.zc[v] * h.zc[v]) * c.r.inv_eps2);
  h.dec_a = 4.0 * nu1 * rcp64(c.r.uinf1);  // (nu and Uinf are both proportional to the wind speed)
}
// eddy viscosity per unit wind speed at height z: lm^2 |dU/dz| / ws [A.3-4]
__device__ __forceinline__ double pr_nu1(const WfProbeConsts& c, double z) {
  const double dudz1 = c.dudz_c * pow_any(z, c.shear - 1.0);
  const double lm = c.kappa * z * rcp64(1.0 + c.kappa * z * rcp64(c.lm_c));
  return lm * lm * fabs(dudz1);
}

// ---- 4. transverse velocities of ONE source at one point [A.3-4]: lateral offset yL (num_eps included), the point's
// height terms, dx >= 0.  Three vortices and their mirrors (both signs flip); the per-source w < 0 -> 0 clamp ----
__device__ __forceinline__ void pr_transverse(const WfProbeConsts& c, const PrHeight& h, double dx, double yL, double Gt, double Gb,
                                              double Gw, double& v, double& w) {
  const double yL2 = yL * yL;
  const double Ey = exp_lean(-yL2 * c.r.inv_eps2);
  const double G[3] = {Gt, Gb, Gw};
  double A = 0.0, Bw = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double zr = h.zc[k], zm = h.zc[3 + k];
    const double tr = (1.0 - Ey * h.ez[k]) * rcp64(yL2 + zr * zr);      // core / r of the real vortex
    const double tm = (1.0 - Ey * h.ez[3 + k]) * rcp64(yL2 + zm * zm);  // ... of its mirror
    A += G[k] * (zr * tr - zm * tm);
    Bw += G[k] * (tr - tm);
  }
  const double dec = c.r.eps2 * rcp64(fma(h.dec_a, dx, c.r.eps2));
  v = A * dec;
  const double ww = -yL * Bw * dec;
  w = (ww < 0.0) ? 0.0 : ww;  // quirk (5) [A.6]
}

// ---- what a source leaves for the deflection / deficit at points behind it ------------------------------------------
struct PrCol {  // the part that depends on the TI of a rotor-grid column [A.3-3, A.3-6]
  double x0d, kyd, d0, pfar, x0v, kyv;
};
struct PrCommon {
  double sy0d, sz0d, is0d, sM, lnAB, sy0v, sz0v, snw, kdef;
};

__device__ __forceinline__ void pr_column(const WfProbeConsts& pc, const PrCommon& s, double cgd, double s_cc, double s_c, double cgv,
                                          double th0, double tan_th0, double E0, double M0, double TIpre, double TIpost, PrCol& o) {
  const WfResolveConsts& c = pc.r;
  o.x0d = c.D * cgd * (1.0 + s_cc) * rcp64(c.sqrt2 * (4.0 * c.defl_alpha * TIpre + 2.0 * c.defl_beta * (1.0 - s_c)));
  o.kyd = c.defl_ka * TIpre + c.defl_kb;
  o.d0 = tan_th0 * o.x0d;
  o.pfar = th0 * E0 * (1.0 / 5.2) * sqrt_pos(s.sy0d * s.sz0d * rcp64(o.kyd * o.kyd * M0));
  o.x0v = c.D * cgv * (1.0 + s_c) * rcp64(c.sqrt2 * (4.0 * c.alpha * TIpost + 2.0 * c.beta * (1.0 - s_c)));
  o.kyv = c.ka * TIpost + c.kb;
}

// ---- 3 + 6: deflection and the deficit's amplitude / widths at downstream position x_t (x_t >= x_i) of one source;
// the masks as FLORIS takes them on the coordinates ----
__device__ __forceinline__ void pr_wake_shape(const WfProbeConsts& pc, const PrCommon& s, const PrCol& k, double x_i, double x_t,
                                              double& delta, double& amp, double& isy2, double& isz2) {
  const WfResolveConsts& c = pc.r;
  const double dx = x_t - x_i;
  const double lin = c.ad + c.bd * dx;
  const double x0d = k.x0d + x_i, x0v = k.x0v + x_i;
  double d_near = (dx * rcp64(k.x0d)) * k.d0 + lin;
  if (!(x_t <= x0d)) d_near = 0.0;
  double d_far = 0.0;
  if (x_t > x0d) {
    const double sy = k.kyd * (x_t - x0d) + s.sy0d, sz = k.kyd * (x_t - x0d) + s.sz0d;
    const double sg = sqrt_pos(sy * sz * s.is0d);
    const double ln_arg = s.lnAB * (1.6 * sg - s.sM) * rcp64(1.6 * sg + s.sM);
    d_far = k.d0 + k.pfar * log_any(ln_arg) + lin;
  }
  delta = d_near + d_far;
  amp = 0.0; isy2 = 0.0; isz2 = 0.0;
  double sy = 0.0, sz = 0.0;
  bool on = false;
  if (x_t > x_i + 0.1 && x_t < x0v) {
    const double ix0v = rcp64(k.x0v);
    const double up = dx * ix0v, dn = (x0v - x_t) * ix0v;
    sy = dn * s.snw + up * s.sy0v;
    sz = dn * s.snw + up * s.sz0v;
    on = true;
  } else if (x_t >= x0v) {
    sy = k.kyv * (x_t - x0v) + s.sy0v;
    sz = k.kyv * (x_t - x0v) + s.sz0v;
    on = true;
  }
  if (on) {
    const double isy = rcp64(sy), isz = rcp64(sz);
    double dd = 1.0 - s.kdef * isy * isz;
    dd = fmin(fmax(dd, 0.0), 1.0);
    amp = 1.0 - sqrt_nn(dd);
    isy2 = 0.5 * isy * isy;
    isz2 = 0.5 * isz * isz;
  }
}
// the Gaussian at lateral offset yy (deflection taken off) and vertical offset zz from the hub; veer: FLORIS rCalt [gauss.py]
__device__ __forceinline__ double pr_gauss(const WfProbeConsts& pc, bool veer_on, double amp, double isy2, double isz2, double yy, double zz) {
  const WfResolveConsts& c = pc.r;
  if (!veer_on) return amp * exp_lean(-((yy * yy) * isy2 + (zz * zz) * isz2));
  const double ca = c.cos2_veer * isy2 + c.sin2_veer * isz2;
  const double cb = 0.5 * c.sin_2veer * (isz2 - isy2);
  const double cc = c.sin2_veer * isy2 + c.cos2_veer * isz2;
  return amp * exp_lean(-(ca * yy * yy - 2.0 * cb * yy * zz + cc * zz * zz));
}

// scipy interp1d(linear, bounds_error=False, fill_value=(lo, hi)) on the LDS copy of a table column; sl: the segment slopes
__device__ __forceinline__ double pr_interp_fill(double xq, int n, const double* xs, const double* ys, const double* sl, double lo, double hi) {
  if (xq < xs[0]) return lo;
  if (xq > xs[n - 1]) return hi;
  if (xq == xs[n - 1]) return ys[n - 1];
  int j = 0;  // last knot <= xq, at most n - 2
  for (int step = 32; step >= 1; step >>= 1) {
    const int k = j + step;
    if (k <= n - 2 && xq >= xs[k]) j = k;
  }
  return sl[j] * (xq - xs[j]) + ys[j];
}

struct PrSource {  // what the thread of source i publishes through LDS (two copies, by the parity of i)
  double x, y, Gt, Gb, Gw;  // written before the first barrier of the stage
  PrCommon s;               // written before the second
  PrCol col[3];
  double ch_pref;
};

}  // namespace

#define PROBE_MAX_N 256

// ---------------------------------------------------------------------------------------------------------------------
// The farm solve: one workgroup per farm slot, one thread per sorted turbine
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PROBE_MAX_N) void wf_probe_state_kernel(const WfProbeConsts c_arg, const WfProbeStateArgs a) {
  // the targets' wake^2 (q = 0..8), V (9..17), W (18..26) as [q][thread]: a quantity of consecutive turbines lies in consecutive
  // banks, and the three rotor-grid columns are walked by a real loop (in registers all 9 x 6 reciprocal chains of the
  // transverse terms were in flight at once and the kernel spilled); the 3-column TI stays in registers
  __shared__ double st[27][PROBE_MAX_N];
  __shared__ WfProbeConsts c;  // (read from LDS: held in scalar registers the constants spilled)
  double *sx = st[0], *s_xs = st[1], *s_ys = st[2], *s_yaw = st[3];  // the sort's scratch lies in rows the state takes over afterwards
  __shared__ double tws[WF_TABLE_PAD], tct[WF_TABLE_PAD], tcs[WF_TABLE_PAD];
  __shared__ PrHeight hz[3];
  __shared__ PrSource S[2];
  const WfResolveConsts& r = c.r;
  const int N = c_arg.r.N, t = threadIdx.x, slot = blockIdx.x;
  if (t == 0) c = c_arg;
  __syncthreads();
  const int b = a.farms ? a.farms[slot] : slot;
  const bool veer_on = r.sin2_veer != 0.0;

  // ---- geometry [A.1]: wd % 360, rotation about the bounding-box centre, stable ascending rank sort — the arithmetic of
  // wf_geometry_kernel ----
  const double ws = a.ws[(size_t)b * a.wind_stride];
  double wdm = fmod(a.wd[(size_t)b * a.wind_stride], 360.0);
  if (wdm < 0.0) wdm += 360.0;
  double dev = fmod(wdm - 270.0, 360.0);
  if (dev < 0.0) dev += 360.0;
  dev = fmod(dev + 360.0, 360.0);
  double ca, sa;
  sincos_any(dev * (M_PI / 180.0), sa, ca);
  double xr = 0.0, yr = 0.0;
  if (t < N) {
    const double xo = a.lx[t] - c.xc, yo = a.ly[t] - c.yc;
    xr = xo * ca - yo * sa + c.xc;
    yr = xo * sa + yo * ca + c.yc;
    sx[t] = xr;
  }
  for (int k = t; k < r.n_table; k += blockDim.x) {  // thrust table and its segment slopes
    tws[k] = a.tab64[k];
    tct[k] = a.tab64[WF_TABLE_PAD + k];
    if (k + 1 < r.n_table) tcs[k] = (a.tab64[WF_TABLE_PAD + k + 1] - a.tab64[WF_TABLE_PAD + k]) / (a.tab64[k + 1] - a.tab64[k]);
  }
  if (t < 3) pr_height(c, r.HH + r.off[t], r.nu1[t], hz[t]);
  if (t == 0) {
    double* hd = a.hdr + (size_t)slot * WF_PROBE_HDR;
    hd[0] = ws; hd[1] = ca; hd[2] = sa;
  }
  __syncthreads();
  if (t < N) {
    int rank = 0;
    for (int u = 0; u < N; ++u) {
      const double xu = sx[u];
      rank += (xu < xr) || (xu == xr && u < t);
    }
    s_xs[rank] = xr;
    s_ys[rank] = yr;
    s_yaw[rank] = (double)a.yaw[(size_t)b * N + t];
  }
  __syncthreads();

  // ---- this thread's target: sorted turbine t ----
  const bool live = t < N;
  const double x_t = live ? s_xs[t] : 0.0, y_t = live ? s_ys[t] : 0.0;
  const double g = live ? s_yaw[t] : 0.0;
  __syncthreads();  // (every thread has its target: the rows become state)
  double sg, cg;
  if (fabs(g) > 45.0) sincos_any(g * kDeg, sg, cg);  // (never an admissible yaw command)
  else sincos_small(g * kDeg, sg, cg);
  double TI[3];  // per lateral column j; the 9-point quantities are indexed [j * 3 + k], k vertical
#pragma unroll 1
  for (int q = 0; q < 27; ++q) st[q][t] = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) TI[j] = r.amb;
  double Uinit[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) Uinit[k] = ws * r.shearf[k];
  const double Uinf = ws * r.uinf1;
  double* rec = a.rec + ((size_t)slot * N + (live ? t : 0)) * WF_PROBE_REC;

  double ct = 0.0, ai = 0.0, ubar = 0.0, val = 0.0;  // the source's own state, carried from the stage's first part to its second
  for (int i = 0; i < N; ++i) {
    PrSource& P = S[i & 1];
    if (t == i) {  // 1. Ct / induction [A.3-1], the circulations [A.3-4], the steering ratio [A.3-2]
      double m3 = 0.0, vs = 0.0;
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const double u = Uinit[q % 3] - sqrt_nn(st[q][t]);
        m3 += u * u * u;
        vs += st[9 + q][t];
      }
      const double m3m = m3 * (1.0 / 9.0);
      ubar = (m3m > 1.0e-6) ? cbrt_pos(m3m) : cbrt_any(m3m);
      double ct_tab = pr_interp_fill(ubar, r.n_table, tws, tct, tcs, 0.0001, 0.9999);
      ct_tab = fmin(fmax(ct_tab, 0.0001), 0.9999);
      ct = ct_tab * cg;
      ai = 0.5 * rcp64(cg) * (1.0 - sqrt_nn(1.0 - ct * cg));
      const double G_wr = (0.25 * kTwoPi) * r.D * (ai - ai * ai) * ubar * r.inv_TSR;
      const double gam_top = (kTwoPi / 16.0) * r.D * r.vel_top * Uinf * ct;
      const double gam_bot = (kTwoPi / 16.0) * r.D * r.vel_bot * Uinf * ct;
      const double sc = sg * cg;
      P.x = x_t; P.y = y_t;
      P.Gt = sc * gam_top * (1.0 / kTwoPi); P.Gb = -sc * gam_bot * (1.0 / kTwoPi); P.Gw = G_wr * (1.0 / kTwoPi);
      const double v_top = gam_top * r.k_top, v_bot = -gam_bot * r.k_bot, v_core = G_wr * r.k_core;
      val = 2.0 * (vs * (1.0 / 9.0) - v_core) * rcp64(v_top + v_bot);
    }
    __syncthreads();
    const double x_i = P.x, y_i = P.y;
    if (live && r.sw_tv && !(x_t - x_i < 0.0)) {  // 4. transverse velocities on every turbine at or downstream of the source, itself and ties included
      const double Gt = P.Gt, Gb = P.Gb, Gw = P.Gw, dx = x_t - x_i;
#pragma unroll 1
      for (int j = 0; j < 3; ++j) {
        const double yL = (y_t + r.off[j] - y_i) + r.num_eps;
#pragma unroll 1
        for (int k = 0; k < 3; ++k) {
          double v, w;
          pr_transverse(c, hz[k], dx, yL, Gt, Gb, Gw, v, w);
          st[9 + j * 3 + k][t] += v;
          st[18 + j * 3 + k][t] += w;
        }
      }
    }
    if (t == i) {  // 2, 5 and the source-only part of 3 + 6 + 8
      val = fmin(fmax(val, -1.0), 1.0);
      const double asv = (fabs(val) > 0.3) ? asin_any(val) : asin_small(val);
      const double g_off = r.sw_steer ? 0.5 * asv : 0.0;  // radians added to the commanded yaw [A.3-2]
      double dTI = 0.0;
      {  // 5. yaw-added recovery [A.3-5] (the source's own transverse contribution is in V / W now)
        double vsum = 0.0, wsum = 0.0;
#pragma unroll
        for (int q = 0; q < 9; ++q) { vsum += st[9 + q][t]; wsum += st[18 + q][t]; }
        const double I = TI[0];
        const double k_tke = (ubar * I) * (ubar * I) * 1.5;
        const double vbar = vsum * (1.0 / 9.0), wbar = wsum * (1.0 / 9.0);
        const double I_tot = sqrt_nn((2.0 / 3.0) * 0.5 * (2.0 * k_tke + vbar * vbar + wbar * wbar)) * rcp64(ubar);
        if (r.sw_yar) dTI = r.gch_gain * (I_tot - I);
      }
      const double c2d = sqrt_nn(fmax(1.0 - val * val, 0.0)), cd = sqrt_pos(0.5 * (1.0 + c2d)), sd = 0.5 * val * rcp64(cd);
      const double cgd = r.sw_steer ? cg * cd - sg * sd : cg;  // cosd(-g_eff) = cos(g + asin(val) / 2)
      const double gd_rad = -(g * kDeg + g_off);
      const double s_cc = sqrt_nn(1.0 - ct * cgd), s_c = sqrt_nn(1.0 - ct);
      const double th0 = r.dm * (0.3 * gd_rad * rcp64(cgd)) * (1.0 - s_cc);
      const double tan_th0 = (fabs(th0) > 0.5) ? tan_any(th0) : tan_small(th0);
      const double C0 = 1.0 - s_c;
      const double M0 = C0 * (2.0 - C0);
      const double E0 = C0 * C0 - r.e0c1 * C0 + r.e0c2;
      const double i1sc = rcp64(1.0 + s_c);
      PrCommon s;
      s.sz0d = r.D * 0.5 * sqrt_pos((ct * cgd * rcp64(2.0 * (1.0 - s_cc))) * i1sc);
      s.sy0d = s.sz0d * cgd * r.cos_veer;
      s.is0d = rcp64(s.sy0d * s.sz0d);
      s.sM = sqrt_pos(M0);
      s.lnAB = (1.6 + s.sM) * rcp64(1.6 - s.sM);
      s.sz0v = r.D * 0.5 * sqrt_pos((ct * rcp64(2.0 * (1.0 - s_c))) * i1sc);
      s.sy0v = s.sz0v * cg * r.cos_veer;
      s.snw = r.near_c * sqrt_pos(ct * 0.5);
      s.kdef = ct * cg * r.D * r.D * 0.125;
      P.s = s;
      P.ch_pref = r.ch_constant * pow_any(ai, r.ch_ai) * r.ch_amb_pow;
#pragma unroll
      for (int j = 0; j < 3; ++j) pr_column(c, s, cgd, s_cc, s_c, cg, th0, tan_th0, E0, M0, TI[j], TI[j] + dTI, P.col[j]);
      // the sampler's record: the source's CENTRE column (include/wfprobe.h)
      rec[PR_X] = x_t; rec[PR_Y] = y_t; rec[PR_GT] = r.sw_tv ? P.Gt : 0.0; rec[PR_GB] = r.sw_tv ? P.Gb : 0.0; rec[PR_GW] = r.sw_tv ? P.Gw : 0.0;
      rec[PR_X0D] = P.col[1].x0d; rec[PR_KYD] = P.col[1].kyd; rec[PR_D0] = P.col[1].d0; rec[PR_PFAR] = P.col[1].pfar;
      rec[PR_X0V] = P.col[1].x0v; rec[PR_KYV] = P.col[1].kyv;
      rec[PR_SY0D] = s.sy0d; rec[PR_SZ0D] = s.sz0d; rec[PR_IS0D] = s.is0d; rec[PR_SM] = s.sM; rec[PR_LNAB] = s.lnAB;
      rec[PR_SY0V] = s.sy0v; rec[PR_SZ0V] = s.sz0v; rec[PR_SNW] = s.snw; rec[PR_KDEF] = s.kdef;
      // (stored: max(ambient, TI + dTI) — FLORIS' maximum(sqrt(ti_added^2 + ambient^2), TI) over all turbines at the end of
      // the source step lifts a TI that a negative rotor-mean speed drove below ambient; the deficit goes on with TI + dTI)
#pragma unroll
      for (int j = 0; j < 3; ++j) TI[j] = fmax(TI[j] + dTI, r.amb);
    }
    __syncthreads();
    if (live && t > i) {  // 3 + 6 + 7 + 8 on the turbines behind the source
      const PrCommon s = P.s;
      const double dx = x_t - x_i;
      int cnt = 0;
#pragma unroll 1
      for (int j = 0; j < 3; ++j) {
        const PrCol k = P.col[j];
        double delta, amp, isy2, isz2;
        pr_wake_shape(c, s, k, x_i, x_t, delta, amp, isy2, isz2);
        const double yy = (y_t + r.off[j]) - y_i - delta;
#pragma unroll
        for (int kz = 0; kz < 3; ++kz) {
          const double dU = pr_gauss(c, veer_on, amp, isy2, isz2, yy, r.off[kz]) * Uinit[kz];
          if (dU > r.overlap_thr) ++cnt;  // the comparison as FLORIS takes it [A.3-8]
          st[j * 3 + kz][t] = fma(dU, dU, st[j * 3 + kz][t]);  // 7. SOSFS [A.3-7]: the sum of squares, root taken where needed
        }
      }
      // 8. Crespo-Hernandez + overlap gating [A.3-8]
      const bool reach = (x_t > x_i) && (x_t <= x_i + 15.0 * r.D);
      if (reach) {
        const double dxp = (dx <= 0.1) ? dx + 1.0 : dx;
        double ti = P.ch_pref * pow_any(dxp * r.inv_D, r.ch_down);
        if (isnan(ti) || (isinf(ti) && ti > 0)) ti = 0.0;
        const double ti_added = ((double)cnt * (1.0 / 9.0)) * ti;
        const double cand = sqrt_pos(ti_added * ti_added + r.amb * r.amb);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if ((fabs(y_i - (y_t + r.off[j])) < 2.0 * r.D) && cand > TI[j]) TI[j] = cand;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The sampler: grid (n_farms, ceil(P / 256)) — the farm in x, whose limit is 2^31 (a batch may exceed the 65 535 of y)
// ---------------------------------------------------------------------------------------------------------------------
extern __shared__ double probe_dyn[];  // [N][WF_PROBE_REC]

__global__ __launch_bounds__(256) void wf_probe_sample_kernel(const WfProbeConsts c, const WfProbeSampleArgs a) {
  const WfResolveConsts& r = c.r;
  const int N = r.N, slot = blockIdx.x, tid = threadIdx.x;
  const int b = a.farms ? a.farms[slot] : slot;
  {
    const double* rec = a.rec + (size_t)slot * N * WF_PROBE_REC;
    for (int k = tid; k < N * WF_PROBE_REC; k += 256) probe_dyn[k] = rec[k];
  }
  __syncthreads();
  const int p = blockIdx.y * 256 + tid;
  if (p >= a.P) return;
  const double* hd = a.hdr + (size_t)slot * WF_PROBE_HDR;
  const double ws = hd[0], ca = hd[1], sa = hd[2];
  const double* pt = a.xyz + ((size_t)(a.per_farm ? b : 0) * a.P + p) * 3;
  const double z = pt[2];
  const double xo = pt[0] - c.xc, yo = pt[1] - c.yc;
  const double x_t = xo * ca - yo * sa + c.xc;
  const double y_t = xo * sa + yo * ca + c.yc;
  const double Uinit = ws * pow_any(z * c.inv_HH, c.shear);  // [A.2]
  const double zz = z - r.HH;
  const bool veer_on = r.sin2_veer != 0.0;
  PrHeight h;
  pr_height(c, z, pr_nu1(c, z), h);
  double wake2 = 0.0, v = 0.0, w = 0.0;
  for (int i = 0; i < N; ++i) {
    const double* s = probe_dyn + i * WF_PROBE_REC;
    const double x_i = s[PR_X];
    if (x_i > x_t) break;  // sorted: this source and every later one lie downstream of the point (dx < 0: no term applies)
    const double y_i = s[PR_Y];
    {
      double vi, wi;
      pr_transverse(c, h, x_t - x_i, (y_t - y_i) + r.num_eps, s[PR_GT], s[PR_GB], s[PR_GW], vi, wi);
      v += vi;
      w += wi;
    }
    PrCommon cm;
    cm.sy0d = s[PR_SY0D]; cm.sz0d = s[PR_SZ0D]; cm.is0d = s[PR_IS0D]; cm.sM = s[PR_SM]; cm.lnAB = s[PR_LNAB];
    cm.sy0v = s[PR_SY0V]; cm.sz0v = s[PR_SZ0V]; cm.snw = s[PR_SNW]; cm.kdef = s[PR_KDEF];
    PrCol k;
    k.x0d = s[PR_X0D]; k.kyd = s[PR_KYD]; k.d0 = s[PR_D0]; k.pfar = s[PR_PFAR]; k.x0v = s[PR_X0V]; k.kyv = s[PR_KYV];
    double delta, amp, isy2, isz2;
    pr_wake_shape(c, cm, k, x_i, x_t, delta, amp, isy2, isz2);
    const double dU = pr_gauss(c, veer_on, amp, isy2, isz2, y_t - y_i - delta, zz) * Uinit;
    wake2 = fma(dU, dU, wake2);
  }
  float* o = a.uvw + ((size_t)slot * a.P + p) * 3;
  o[0] = (float)(Uinit - sqrt_nn(wake2));
  o[1] = (float)v;
  o[2] = (float)w;
}

extern "C" hipError_t wfk_launch_probe_state(const WfProbeConsts* c, const WfProbeStateArgs* a, int n_farms, hipStream_t s) {
  const int threads = ((c->r.N + 63) / 64) * 64;
  hipLaunchKernelGGL(wf_probe_state_kernel, dim3(n_farms), dim3(threads), 0, s, *c, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_probe_sample(const WfProbeConsts* c, const WfProbeSampleArgs* a, int n_farms, hipStream_t s) {
  const size_t lds = sizeof(double) * WF_PROBE_REC * (size_t)c->r.N;
  hipLaunchKernelGGL(wf_probe_sample_kernel, dim3(n_farms, (a->P + 255) / 256), dim3(256), lds, s, *c, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_probe_func_attributes(int which, hipFuncAttributes* attr) {
  return hipFuncGetAttributes(attr, which == 0 ? (const void*)wf_probe_state_kernel : (const void*)wf_probe_sample_kernel);
}
