// afx_geom.h - the geometry that the projective and lattice-sampling analysis units share (afx_kernels_hull.hip, afx_kernels_sirt.hip,
// afx_kernels_viewmap.hip, afx_kernels_pose.hip, afx_kernels_lumen.hip, afx_kernels_reformat.hip): the view record, the 3x4 affine, the
// world-to-camera step and the trilinear lattice lookup.  Every definition in include/afx.h that uses one of them states it operation by
// operation, and the units are pinned bit for bit against NumPy restatements: the order of the operations below is that order.
// Contraction is off from here on (the pragma at file scope also covers the including unit, which repeats it for its own kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/afx.h"

#pragma clang fp contract(off)

namespace afx {

struct ViewRecord {                                   // AFX_HULL_VIEW_DOUBLES = 16
  double R[9];                                        // cam2world's rotation, row-major: R[3 r + n] = R[r][n]
  double c[3];                                        // the source position
  double f;
  double pad[3];
};
static_assert(sizeof(ViewRecord) == 8 * AFX_HULL_VIEW_DOUBLES, "the view record is AFX_HULL_VIEW_DOUBLES doubles");

// x = A (a, b, c, 1): the rows of a row-major 3x4 affine, each as ((A0 a + A1 b) + A2 c) + A3
__device__ __forceinline__ void affine_apply(const double* A, double a, double b, double c, double& x0, double& x1, double& x2) {
  x0 = ((A[0] * a + A[1] * b) + A[2] * c) + A[3];
  x1 = ((A[4] * a + A[5] * b) + A[6] * c) + A[7];
  x2 = ((A[8] * a + A[9] * b) + A[10] * c) + A[11];
}

// lattice point p of an (n0, n1, n2) lattice, the innermost axis fastest, through index_to_world
__device__ __forceinline__ void affine_apply_index(const double* A, int32_t p, int32_t n1, int32_t n2, double& x0, double& x1, double& x2) {
  const int32_t k = p % n2, ij = p / n2, j = ij % n1, i = ij / n1;
  affine_apply(A, (double)i, (double)j, (double)k, x0, x1, x2);
}

// the point x in the view's camera frame: e = x - c, q = R^T e.  The depth along the viewing direction is d = -q2.
__device__ __forceinline__ void view_camera(const ViewRecord& vw, double x0, double x1, double x2, double& q0, double& q1, double& q2) {
  const double e0 = x0 - vw.c[0], e1 = x1 - vw.c[1], e2 = x2 - vw.c[2];
  q0 = (vw.R[0] * e0 + vw.R[3] * e1) + vw.R[6] * e2;
  q1 = (vw.R[1] * e0 + vw.R[4] * e1) + vw.R[7] * e2;
  q2 = (vw.R[2] * e0 + vw.R[5] * e1) + vw.R[8] * e2;
}

// the pixel of a camera-frame point at depth d = -q2 on a detector whose centre is (half_w, half_h)
__device__ __forceinline__ void view_pixel(const ViewRecord& vw, double half_w, double half_h, double q0, double q1, double d, double& u, double& w) {
  u = half_w + (vw.f * q0) / d;
  w = half_h - (vw.f * q1) / d;
}

// the blend of the lookups: p + (q - p) t, three roundings
__device__ __forceinline__ double lerp(double p, double q, double t) { return p + (q - p) * t; }

// The trilinear lookup of vol[n0][n1][n2] (n_a >= 2) at the world point x: g = B x (B = world_to_index); inside iff 0 <= g_a <= n_a - 1
// on every axis; i_a = min(floor(g_a), n_a - 2), so that i_a + 1 is a voxel; the blend runs along axis 2, then 1, then 0.  Outside the
// value is `fill`: a NaN or a huge g ends at the comparison, nothing is converted to an integer and nothing is loaded.
// L is the unit's kernel-argument struct, with `double W[12]` (B) and `int32_t n0, n1, n2`.  It is read in place, not handed over as
// four values: each size is then fetched where its comparison needs it, and the callers' instruction streams are what they were with
// their own copies of this function.
template <typename L, typename T>
__device__ __forceinline__ double lattice_lookup(const L& a, const T* __restrict__ vol, double x0, double x1, double x2, double fill) {
  double g0, g1, g2;
  affine_apply(a.W, x0, x1, x2, g0, g1, g2);
  const bool inside = g0 >= 0.0 && g0 <= (double)(a.n0 - 1) && g1 >= 0.0 && g1 <= (double)(a.n1 - 1) && g2 >= 0.0 && g2 <= (double)(a.n2 - 1);
  if (!inside) return fill;
  const double l0 = (double)(a.n0 - 2), l1 = (double)(a.n1 - 2), l2 = (double)(a.n2 - 2);
  double f0 = floor(g0), f1 = floor(g1), f2 = floor(g2);
  f0 = f0 < l0 ? f0 : l0;
  f1 = f1 < l1 ? f1 : l1;
  f2 = f2 < l2 ? f2 : l2;
  const double t0 = g0 - f0, t1 = g1 - f1, t2 = g2 - f2;
  const size_t s1 = (size_t)a.n2, s0 = (size_t)a.n1 * (size_t)a.n2;
  const T* b = vol + ((size_t)(int)f0 * s0 + (size_t)(int)f1 * s1 + (size_t)(int)f2);
  const double p000 = (double)b[0], p001 = (double)b[1], p010 = (double)b[s1], p011 = (double)b[s1 + 1];
  const double p100 = (double)b[s0], p101 = (double)b[s0 + 1], p110 = (double)b[s0 + s1], p111 = (double)b[s0 + s1 + 1];
  const double c00 = lerp(p000, p001, t2), c01 = lerp(p010, p011, t2);
  const double c10 = lerp(p100, p101, t2), c11 = lerp(p110, p111, t2);
  return lerp(lerp(c00, c01, t1), lerp(c10, c11, t1), t0);
}

}  // namespace afx
