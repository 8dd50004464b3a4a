// afx_kernels_frangi3d.hip — the 3-D Frangi vesselness of a density volume (afx_frangi_3d and its workspace query; the definition is in
// include/afx.h, its NumPy / SciPy restatement in tests/frangi3d_reference.py).  Its own translation unit.
//
// Everything is fp64 and every expression is evaluated operation by operation as the restatement evaluates it (no FMA contraction): the
// three Gaussian passes sum in scipy.ndimage's order with its kernel weights, the Hessian takes np.gradient's differences, the eigenvalues
// come from a fixed number of Jacobi sweeps that use + - * / and sqrt only - all correctly rounded on the host and on gfx950 - so the
// device follows the host to the bit up to the exp() of the Gaussian weights and of the vesselness factors.  No floating-point atomics:
// the per-scale max of S = l1^2 + l2^2 + l3^2 (non-negative doubles) is an integer atomicMax on the bit pattern, exact and independent of
// the order.  Nothing allocates or synchronises: the call is hipGraph-capturable and deterministic.
//
// The scales are processed one after another with a running maximum, so the workspace is a few volumes whatever n_sigmas:
//   memset smax; per scale s: gauss axis 0 (x -> A), axis 1 (A -> B), axis 2 (B -> A); eigen (A -> the three eigenvalue volumes, smax[s]);
//   vessel (eigenvalues, smax[s] -> out, scale_index).
// Consecutive lanes always hold consecutive axis-2 voxels: the axis-2 pass walks contiguous memory, the axis-0 and axis-1 passes walk
// their taps with a stride of n1 n2 and n2 elements, every load of a wave coalesced.
// AFX_FRANGI3D_RECOMPUTE (a build variant for measurement): the eigenvalues are not kept; the vessel kernel takes the Hessian
// and the Jacobi sweeps again.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/afx.h"
#include "afx_internal.h"
#include "afx_image_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int F3_BLOCK = 256;
constexpr int F3_SWEEPS = 5;
#ifdef AFX_FRANGI3D_RECOMPUTE
constexpr bool F3_KEEP = false;
#else
constexpr bool F3_KEEP = true;
#endif

struct Dims { int n[3]; };          // n0, n1, n2; the strides are n1 n2, n2, 1

// One 1-D Gaussian pass of scipy.ndimage.gaussian_filter along AXIS (correlate1d with symmetric weights: x[i] w0 first, then the pairs
// from the outermost inwards; mode 'reflect').  The axis-0 pass reads the caller's volume (T = float or double) and applies the
// black-ridge inversion 1 - x on load.  A voxel whose taps all lie inside the line skips the reflection's integer division.
// grid: ceil(N / 256); dynamic LDS (3 r + 2) doubles
template <int AXIS, class T>
__global__ void __launch_bounds__(F3_BLOCK) k_f3_gauss(const T* __restrict__ src, double* __restrict__ dst, Dims d, double sigma, int r, int invert) {
  extern __shared__ double lds[];
  double* wt = lds;
  gauss_weights(sigma, r, wt, lds + (r + 1));
  const int64_t total = (int64_t)d.n[0] * d.n[1] * d.n[2];
  const int64_t p = (int64_t)blockIdx.x * F3_BLOCK + threadIdx.x;
  if (p >= total) return;
  const int n = d.n[AXIS];
  const int64_t stride = AXIS == 0 ? (int64_t)d.n[1] * d.n[2] : AXIS == 1 ? (int64_t)d.n[2] : 1;
  const int i = AXIS == 0 ? (int)(p / stride) : AXIS == 1 ? (int)((p / stride) % n) : (int)(p % n);
  const T* line = src + (p - (int64_t)i * stride);
  auto ld = [&](int k) {
    const double x = (double)line[(int64_t)k * stride];
    return invert ? 1.0 - x : x;
  };
  double acc = ld(i) * wt[0];
  if (i >= r && i + r < n) {
    for (int j = r; j >= 1; --j) acc += (ld(i - j) + ld(i + j)) * wt[j];
  } else {
    for (int j = r; j >= 1; --j) acc += (ld(reflect_index(i - j, n)) + ld(reflect_index(i + j, n))) * wt[j];
  }
  dst[p] = acc;
}

// np.gradient of G along axis A at the voxel whose flat index, with its coordinate along A taken out, is `base` and whose coordinate is c
template <int A>
__device__ __forceinline__ double f3_grad(const double* __restrict__ G, const Dims& d, const int64_t* st, int64_t base, int c) {
  const Diff g = grad_at(c, d.n[A]);
  return (G[base + g.a * st[A]] - G[base + g.b * st[A]]) / g.div;
}

// H_AB = np.gradient(np.gradient(G, axis=A), axis=B) at voxel p = (i[0], i[1], i[2]), A <= B
template <int A, int B>
__device__ __forceinline__ double f3_hess(const double* __restrict__ G, const Dims& d, const int64_t* st, int64_t p, const int* i) {
  const Diff b = grad_at(i[B], d.n[B]);
  const int64_t base = p - i[A] * st[A];
  double hi, lo;
  if (A == B) {
    hi = f3_grad<A>(G, d, st, base, b.a);
    lo = f3_grad<A>(G, d, st, base, b.b);
  } else {
    hi = f3_grad<A>(G, d, st, base + (b.a - i[B]) * st[B], i[A]);
    lo = f3_grad<A>(G, d, st, base + (b.b - i[B]) * st[B], i[A]);
  }
  return (hi - lo) / b.div;
}

// One Jacobi rotation of the pair (p, q), r the third index; a pair whose off-diagonal element is 0 is skipped
__device__ __forceinline__ void f3_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
  if (apq != 0.0) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double tau = s / (1.0 + c);
    const double tapq = t * apq;
    const double nrp = arp - s * (arq + tau * arp);
    const double nrq = arq + s * (arp - tau * arq);
    app = app - tapq;
    aqq = aqq + tapq;
    apq = 0.0;
    arp = nrp;
    arq = nrq;
  }
}

__device__ __forceinline__ void f3_order(double& x, double& y) {      // swaps on strictly-less only: the three-element bubble sort is stable
  if (fabs(y) < fabs(x)) { const double t = x; x = y; y = t; }
}

// The eigenvalues of sigma^2 x the Hessian of G at voxel p, ordered by |lambda| ascending (a tie: the earlier diagonal position first)
__device__ __forceinline__ void f3_eigen(const double* __restrict__ G, const Dims& d, int64_t p, double s2, double& l1, double& l2, double& l3) {
  const int64_t st[3] = {(int64_t)d.n[1] * d.n[2], (int64_t)d.n[2], 1};
  const int i[3] = {(int)(p / st[0]), (int)((p / st[1]) % d.n[1]), (int)(p % d.n[2])};
  double a00 = s2 * f3_hess<0, 0>(G, d, st, p, i), a01 = s2 * f3_hess<0, 1>(G, d, st, p, i), a02 = s2 * f3_hess<0, 2>(G, d, st, p, i);
  double a11 = s2 * f3_hess<1, 1>(G, d, st, p, i), a12 = s2 * f3_hess<1, 2>(G, d, st, p, i), a22 = s2 * f3_hess<2, 2>(G, d, st, p, i);
  for (int sweep = 0; sweep < F3_SWEEPS; ++sweep) {
    f3_rotate(a00, a11, a01, a02, a12);      // (0, 1), r = 2
    f3_rotate(a00, a22, a02, a01, a12);      // (0, 2), r = 1
    f3_rotate(a11, a22, a12, a01, a02);      // (1, 2), r = 0
  }
  f3_order(a00, a11);
  f3_order(a11, a22);
  f3_order(a00, a11);
  l1 = a00; l2 = a11; l3 = a22;
}

__device__ __forceinline__ double f3_sum_squares(double l1, double l2, double l3) { return l1 * l1 + l2 * l2 + l3 * l3; }

// Per voxel the three ordered eigenvalues of one scale (kept in E[3][N] unless the build recomputes them) and the max over the volume of
// S: one LDS atomicMax per lane, one global atomicMax per workgroup, on the bit patterns (S >= 0; a NaN's pattern is above every number
// and so propagates as np.max does).  grid: ceil(N / 256)
__global__ void __launch_bounds__(F3_BLOCK) k_f3_eigen(const double* __restrict__ G, double* __restrict__ E, Dims d, double s2,
                                                      unsigned long long* __restrict__ smax) {
  __shared__ unsigned long long bmax;
  if (threadIdx.x == 0) bmax = 0ull;
  __syncthreads();
  const int64_t total = (int64_t)d.n[0] * d.n[1] * d.n[2];
  const int64_t p = (int64_t)blockIdx.x * F3_BLOCK + threadIdx.x;
  if (p < total) {
    double l1, l2, l3;
    f3_eigen(G, d, p, s2, l1, l2, l3);
    if (F3_KEEP) {
      E[p] = l1;
      E[total + p] = l2;
      E[2 * total + p] = l3;
    }
    atomicMax(&bmax, (unsigned long long)__double_as_longlong(f3_sum_squares(l1, l2, l3)));
  }
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(smax, bmax);
}

// v of one scale from the eigenvalues, and the running maximum over the scales: scale 0 writes out and scale_index, a later scale
// replaces them where its v is larger (or is the first NaN): np.max and np.argmax over the scale axis.  gamma <= 0: gamma_s =
// sqrt(max S) / 2, 1 where that is 0.  grid: ceil(N / 256)
__global__ void __launch_bounds__(F3_BLOCK) k_f3_vessel(const double* __restrict__ G, const double* __restrict__ E, Dims d, double s2, int scale,
                                                       double alpha, double beta, double gamma, const unsigned long long* __restrict__ smax,
                                                       double* __restrict__ out, uint8_t* __restrict__ scale_index) {
  const int64_t total = (int64_t)d.n[0] * d.n[1] * d.n[2];
  const int64_t p = (int64_t)blockIdx.x * F3_BLOCK + threadIdx.x;
  if (p >= total) return;
  double l1, l2, l3;
  if (F3_KEEP) {
    l1 = E[p];
    l2 = E[total + p];
    l3 = E[2 * total + p];
  } else {
    f3_eigen(G, d, p, s2, l1, l2, l3);
  }
  double g = gamma;
  if (!(gamma > 0.0)) {
    g = sqrt(__longlong_as_double((long long)*smax)) / 2.0;
    if (g == 0.0) g = 1.0;
  }
  const double a2 = 2.0 * (alpha * alpha), b2 = 2.0 * (beta * beta), c2 = 2.0 * (g * g);
  double d3 = fabs(l3);
  if (d3 == 0.0) d3 = 1e-10;
  double d23 = sqrt(fabs(l2 * l3));
  if (d23 == 0.0) d23 = 1e-10;
  const double qa = fabs(l2) / d3, qb = fabs(l1) / d23;
  const double ra = qa * qa, rb = qb * qb;
  const double S = f3_sum_squares(l1, l2, l3);
  double v = (1.0 - exp(-ra / a2)) * exp(-rb / b2) * (1.0 - exp(-S / c2));
  if (l2 > 0.0 || l3 > 0.0) v = 0.0;
  if (scale > 0) {
    const double best = out[p];
    if (!(v > best || (v != v && best == best))) return;
  }
  out[p] = v;
  if (scale_index) scale_index[p] = (uint8_t)scale;
}

bool f3_shape_ok(int32_t n0, int32_t n1, int32_t n2) {
  if (n0 < 2 || n1 < 2 || n2 < 2) return false;
  const int64_t lim = (int64_t)1 << 31;
  const int64_t a = (int64_t)n0 * n1;
  return a < lim && a * n2 < lim;
}

struct F3Bufs { double* a; double* b; double* e; unsigned long long* smax; };
F3Bufs f3_carve(afx::Carve& c, int32_t n0, int32_t n1, int32_t n2) {
  const size_t vol = (size_t)n0 * n1 * n2 * sizeof(double);
  F3Bufs w;
  w.a = c.take<double>(vol);
  w.b = c.take<double>(vol);
  w.e = F3_KEEP ? c.take<double>(3 * vol) : nullptr;
  w.smax = c.take<unsigned long long>(IMG_MAX_SIGMAS * sizeof(unsigned long long));
  return w;
}

template <class T>
void f3_launch(const T* x, const Dims& d, const double* sigmas, int32_t n_sigmas, double alpha, double beta, double gamma, int invert, double* out,
               uint8_t* scale_index, const F3Bufs& w, hipStream_t st) {
  const int64_t total = (int64_t)d.n[0] * d.n[1] * d.n[2];
  const unsigned blocks = (unsigned)((total + F3_BLOCK - 1) / F3_BLOCK);
  (void)hipMemsetAsync(w.smax, 0, IMG_MAX_SIGMAS * sizeof(unsigned long long), st);
  for (int s = 0; s < n_sigmas; ++s) {
    const double sigma = sigmas[s];
    const int r = (int)(4.0 * sigma + 0.5);            // scipy.ndimage.gaussian_filter1d: int(truncate * sigma + 0.5), truncate = 4
    const size_t lds = (size_t)(3 * r + 2) * sizeof(double);
    const double s2 = sigma * sigma;
    hipLaunchKernelGGL((k_f3_gauss<0, T>), dim3(blocks), dim3(F3_BLOCK), lds, st, x, w.a, d, sigma, r, invert);
    hipLaunchKernelGGL((k_f3_gauss<1, double>), dim3(blocks), dim3(F3_BLOCK), lds, st, (const double*)w.a, w.b, d, sigma, r, 0);
    hipLaunchKernelGGL((k_f3_gauss<2, double>), dim3(blocks), dim3(F3_BLOCK), lds, st, (const double*)w.b, w.a, d, sigma, r, 0);
    hipLaunchKernelGGL(k_f3_eigen, dim3(blocks), dim3(F3_BLOCK), 0, st, (const double*)w.a, w.e, d, s2, w.smax + s);
    hipLaunchKernelGGL(k_f3_vessel, dim3(blocks), dim3(F3_BLOCK), 0, st, (const double*)w.a, (const double*)w.e, d, s2, s, alpha, beta, gamma,
                       (const unsigned long long*)(w.smax + s), out, scale_index);
  }
}

}  // namespace

extern "C" size_t afx_frangi_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2, int32_t n_sigmas) {
  if (!f3_shape_ok(n0, n1, n2) || n_sigmas <= 0 || n_sigmas > IMG_MAX_SIGMAS) return 0;
  afx::Carve c;
  f3_carve(c, n0, n1, n2);
  return c.end;
}

extern "C" int afx_frangi_3d(const void* x, int32_t x_is_f64, int32_t n0, int32_t n1, int32_t n2, const double* sigmas, int32_t n_sigmas, double alpha,
                             double beta, double gamma, int32_t black_ridges, double* out, uint8_t* scale_index, void* workspace,
                             size_t workspace_bytes, size_t* workspace_needed, void* stream) {
  const char* who = "afx_frangi_3d";
  if (!x || !out) return afx::set_error(AFX_E_INVALID, who, "null volume or output");
  if (!f3_shape_ok(n0, n1, n2)) return afx::set_error(AFX_E_INVALID, who, "need every side >= 2 and n0 n1 n2 < 2^31");
  if (!sigmas || n_sigmas <= 0 || n_sigmas > IMG_MAX_SIGMAS) return afx::set_error(AFX_E_INVALID, who, "need 1 <= n_sigmas <= 16 and a sigma array");
  for (int s = 0; s < n_sigmas; ++s)
    if (!(sigmas[s] > 0.0) || !(4.0 * sigmas[s] + 0.5 <= (double)IMG_MAX_RADIUS + 0.5))
      return afx::set_error(AFX_E_INVALID, who, "every sigma must be > 0 and give a radius int(4 sigma + 0.5) <= 1000");
  if (!(alpha > 0.0) || !(beta > 0.0) || !isfinite(alpha) || !isfinite(beta)) return afx::set_error(AFX_E_INVALID, who, "alpha and beta must be finite and > 0");
  if (gamma != gamma || gamma == INFINITY) return afx::set_error(AFX_E_INVALID, who, "gamma must be finite (<= 0: per-scale sqrt(max S) / 2)");
  const size_t need = afx_frangi_3d_workspace_bytes(n0, n1, n2, n_sigmas);
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(x, "the volume", who)) return rc;
  afx::Carve c;
  c.base = (uintptr_t)workspace;
  const F3Bufs w = f3_carve(c, n0, n1, n2);
  const Dims d = {{n0, n1, n2}};
  if (x_is_f64) f3_launch((const double*)x, d, sigmas, n_sigmas, alpha, beta, gamma, black_ridges != 0, out, scale_index, w, (hipStream_t)stream);
  else f3_launch((const float*)x, d, sigmas, n_sigmas, alpha, beta, gamma, black_ridges != 0, out, scale_index, w, (hipStream_t)stream);
  return afx::launched(who);
}
