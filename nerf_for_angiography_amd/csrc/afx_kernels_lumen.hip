// afx_kernels_lumen.hip - lumen cross-sections along a centreline (afx_lumen_profile); the definition stands in include/afx.h.  At every
// centreline point a fan of R rays in the plane normal to the centreline is marched through the trilinearly interpolated volume until it
// crosses the iso level; the crossing radii give the area, the diameters and the mean radius.  One lane per ray; a wavefront holds
// 64 / R points (R = 64: one).  The reductions are xor-butterflies inside the R lanes of a point: no LDS, no atomics, nothing allocated.
// NOTHING CAN HANG: no lane waits for a value that another lane or wave writes, and the march runs at most max_steps times, a count the
// lane holds before it enters the loop.  Every load is made after the index test of the definition passed; the window ends are clamped
// into [0, P - 1] before a point is read.
#include "afx_internal.h"
#include "afx_geom.h"
#include <cmath>

// every fp64 product and sum below is rounded on its own (the definition is stated operation by operation); plain operators under this
// pragma, as in afx_kernels_graph.hip
#pragma clang fp contract(off)

namespace {

constexpr int LM_BLOCK = 256;                         // 4 waves
constexpr int LM_WAVES = LM_BLOCK / 64;
constexpr int LM_MAX_RAYS = 64;
constexpr int LM_MAX_STEPS = 4096;
enum { LM_NO_TANGENT = 1, LM_CENTRE_OUTSIDE = 2 };

// by value in the kernel arguments (1.2 KiB): no copy is issued for the ray table
struct LumenArgs {
  double W[12];
  double cs[2 * LM_MAX_RAYS];                         // cos, sin of ray j at [2 j], [2 j + 1]
  double area_coef, iso, ds;
  int64_t P;
  int32_t n0, n1, n2, h, R, M;
  int32_t ppw;                                        // points per wave: 64 / R, or 1 (lanes >= R idle)
};

// step 4 of the definition: afx::lattice_lookup, 0.0 outside
template <typename T>
__device__ __forceinline__ double lm_lookup(const LumenArgs& a, const T* __restrict__ vol, double x0, double x1, double x2) {
  return afx::lattice_lookup(a, vol, x0, x1, x2, 0.0);
}

template <typename T>
__global__ void __launch_bounds__(LM_BLOCK) k_lumen_profile(const LumenArgs a, const T* __restrict__ vol, const double* __restrict__ points,
                                                            const int32_t* __restrict__ seg_first, const int32_t* __restrict__ seg_last,
                                                            double* __restrict__ profile, int32_t* __restrict__ flags, double* __restrict__ radii) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int R = a.R, j = lane & (R - 1), sub = lane / R;
  const int64_t k = ((int64_t)blockIdx.x * LM_WAVES + wave) * a.ppw + sub;
  const bool mine = sub < a.ppw && k < a.P;           // this lane has a ray of a point; every lane stays for the shuffles below
  int flag = 0;
  double f_c = 0.0, cx = 0.0, cy = 0.0, cz = 0.0, dx = 0.0, dy = 0.0, dz = 0.0;
  if (mine) {
    // 1. the tangent over the window, cut at the ends of the point's polyline
    int64_t ia = k - a.h, ib = k + a.h;
    const int64_t sf = seg_first[k], sl = seg_last[k];
    ia = ia > sf ? ia : sf;
    ib = ib < sl ? ib : sl;
    ia = ia < 0 ? 0 : (ia > a.P - 1 ? a.P - 1 : ia);
    ib = ib < 0 ? 0 : (ib > a.P - 1 ? a.P - 1 : ib);
    double t0 = points[3 * ib] - points[3 * ia], t1 = points[3 * ib + 1] - points[3 * ia + 1], t2 = points[3 * ib + 2] - points[3 * ia + 2];
    const double nn = (t0 * t0 + t1 * t1) + t2 * t2;
    if (ib <= ia || nn == 0.0) flag |= LM_NO_TANGENT;
    cx = points[3 * k], cy = points[3 * k + 1], cz = points[3 * k + 2];
    // 5. the centre
    f_c = lm_lookup(a, vol, cx, cy, cz);
    if (!(f_c >= a.iso)) flag |= LM_CENTRE_OUTSIDE;
    if (!flag) {
      const double nt = sqrt(nn);
      t0 = t0 / nt, t1 = t1 / nt, t2 = t2 / nt;
      // 2. the frame: e = the axis of the first smallest |t_a|, u = t x e normalised, v = t x u
      const double m0 = fabs(t0), m1 = fabs(t1), m2 = fabs(t2);
      int ax = 0;
      double best = m0;
      if (m1 < best) ax = 1, best = m1;
      if (m2 < best) ax = 2;
      const double e0 = ax == 0 ? 1.0 : 0.0, e1 = ax == 1 ? 1.0 : 0.0, e2 = ax == 2 ? 1.0 : 0.0;
      double u0 = t1 * e2 - t2 * e1, u1 = t2 * e0 - t0 * e2, u2 = t0 * e1 - t1 * e0;
      const double nu = sqrt((u0 * u0 + u1 * u1) + u2 * u2);
      u0 = u0 / nu, u1 = u1 / nu, u2 = u2 / nu;
      const double v0 = t1 * u2 - t2 * u1, v1 = t2 * u0 - t0 * u2, v2 = t0 * u1 - t1 * u0;
      // 3. this lane's direction
      const double cs = a.cs[2 * j], sn = a.cs[2 * j + 1];
      dx = cs * u0 + sn * v0, dy = cs * u1 + sn * v1, dz = cs * u2 + sn * v2;
    }
  }
  // 6. the march: at most M steps, M fixed before entry (0 for a lane without a ray)
  const bool go = mine && !flag;
  const int steps = go ? a.M : 0;
  double r = go ? (double)a.M * a.ds : 0.0;
  int open = go ? 1 : 0;
  double f_prev = f_c;
#pragma unroll 1
  for (int m = 1; m <= steps; ++m) {
    const double s = (double)m * a.ds;
    const double f_m = lm_lookup(a, vol, cx + s * dx, cy + s * dy, cz + s * dz);
    if (f_m < a.iso) {
      r = a.ds * ((double)(m - 1) + (f_prev - a.iso) / (f_prev - f_m));
      open = 0;
      break;
    }
    f_prev = f_m;
  }
  // 7. the reductions, inside the R lanes of the point (lane distances below R never leave them)
  const int base = lane & ~(R - 1);
  const double r_next = __shfl(r, base | ((j + 1) & (R - 1)));
  const double r_opp = __shfl_xor(r, R >> 1);
  double s_area = r * r_next, s_r = r, lo = r, hi = r;
  const double dia = r + r_opp;
  double d_lo = dia, d_hi = dia;
  int n_open = open;
  for (int d = 1; d < R; d <<= 1) {
    s_area = s_area + __shfl_xor(s_area, d);
    s_r = s_r + __shfl_xor(s_r, d);
    const double o_lo = __shfl_xor(lo, d), o_hi = __shfl_xor(hi, d), o_dlo = __shfl_xor(d_lo, d), o_dhi = __shfl_xor(d_hi, d);
    lo = o_lo < lo ? o_lo : lo;
    hi = o_hi > hi ? o_hi : hi;
    d_lo = o_dlo < d_lo ? o_dlo : d_lo;
    d_hi = o_dhi > d_hi ? o_dhi : d_hi;
    n_open += __shfl_xor(n_open, d);
  }
  // 8. the outputs
  if (!mine) return;
  if (radii) radii[k * R + j] = r;
  if (j == 0) {
    double* row = profile + 8 * k;
    row[0] = go ? a.area_coef * s_area : 0.0;
    row[1] = go ? s_r / (double)R : 0.0;
    row[2] = lo;
    row[3] = hi;
    row[4] = d_lo;
    row[5] = d_hi;
    row[6] = f_c;
    row[7] = 0.0;
    flags[k] = flag | (n_open << 8);
  }
}

}  // namespace

extern "C" int afx_lumen_profile(const void* vol, int32_t vol_is_f64, int32_t n0, int32_t n1, int32_t n2, const double* world_to_index,
                                 const double* points, const int32_t* seg_first, const int32_t* seg_last, int64_t n_points,
                                 int32_t half_window, int32_t n_rays, const double* ray_cs, double area_coef, double iso, double step,
                                 int32_t max_steps, double* profile, int32_t* flags, double* radii, void* stream) {
  const char* who = "afx_lumen_profile";
  if (!vol) return afx::set_error(AFX_E_INVALID, who, "null vol");
  if (!world_to_index) return afx::set_error(AFX_E_INVALID, who, "null world_to_index");
  if (!ray_cs) return afx::set_error(AFX_E_INVALID, who, "null ray_cs");
  if (n0 < 2 || n1 < 2 || n2 < 2) return afx::set_error(AFX_E_INVALID, who, "n0, n1, n2: need at least 2 voxels along each axis");
  if (int rc = afx::check_lattice_size(n0, n1, n2, who)) return rc;
  if (n_points < 0 || n_points > 0x7fffffff) return afx::set_error(AFX_E_INVALID, who, "n_points must lie in 0..2^31 - 1");
  if (n_rays != 8 && n_rays != 16 && n_rays != 32 && n_rays != 64) return afx::set_error(AFX_E_INVALID, who, "n_rays must be 8, 16, 32 or 64");
  if (half_window < 1) return afx::set_error(AFX_E_INVALID, who, "half_window must be at least 1");
  if (!std::isfinite(iso)) return afx::set_error(AFX_E_INVALID, who, "iso must be finite");
  if (!afx::all_finite(world_to_index, 12)) return afx::set_error(AFX_E_INVALID, who, "world_to_index must be finite");
  if (!afx::all_finite(ray_cs, 2 * n_rays)) return afx::set_error(AFX_E_INVALID, who, "ray_cs must be finite");
  if (!std::isfinite(area_coef)) return afx::set_error(AFX_E_INVALID, who, "area_coef must be finite");
  if (!(step > 0.0) || !std::isfinite(step)) return afx::set_error(AFX_E_INVALID, who, "step must be finite and > 0");
  if (max_steps < 1 || max_steps > LM_MAX_STEPS) return afx::set_error(AFX_E_INVALID, who, "max_steps must lie in 1..4096");
  if (n_points == 0) return AFX_OK;                   // nothing to launch
  if (!points) return afx::set_error(AFX_E_INVALID, who, "null points");
  if (!seg_first || !seg_last) return afx::set_error(AFX_E_INVALID, who, "null seg_first or seg_last");
  if (!profile) return afx::set_error(AFX_E_INVALID, who, "null profile");
  if (!flags) return afx::set_error(AFX_E_INVALID, who, "null flags");
  if (int rc = afx::check_device(vol, "the volume", who)) return rc;
  if (int rc = afx::check_device(profile, "profile", who)) return rc;
  LumenArgs a;
  for (int i = 0; i < 12; ++i) a.W[i] = world_to_index[i];
  for (int i = 0; i < 2 * LM_MAX_RAYS; ++i) a.cs[i] = i < 2 * n_rays ? ray_cs[i] : 0.0;
  a.area_coef = area_coef, a.iso = iso, a.ds = step, a.P = n_points;
  a.n0 = n0, a.n1 = n1, a.n2 = n2, a.h = half_window, a.R = n_rays, a.M = max_steps;
#ifdef AFX_LUMEN_IDLE_LANES
  a.ppw = 1;                                          // measurement build: one point per wave at every R
#else
  a.ppw = 64 / n_rays;
#endif
  const int64_t per_block = (int64_t)LM_WAVES * a.ppw;
  const unsigned blocks = (unsigned)((n_points + per_block - 1) / per_block);
  hipStream_t st = (hipStream_t)stream;
  if (vol_is_f64)
    hipLaunchKernelGGL(k_lumen_profile<double>, dim3(blocks), dim3(LM_BLOCK), 0, st, a, (const double*)vol, points, seg_first, seg_last, profile,
                       flags, radii);
  else
    hipLaunchKernelGGL(k_lumen_profile<float>, dim3(blocks), dim3(LM_BLOCK), 0, st, a, (const float*)vol, points, seg_first, seg_last, profile,
                       flags, radii);
  return afx::launched(who);
}
