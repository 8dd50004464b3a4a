// afx_kernels_image.hip — per-pixel ray-sampling weights of the projections (phantomdata/helpers.py:226-247 get_weighted_img with
// the Frangi vesselness filter of scikit-image 0.18.3, phantomdata/cttoray.py:210-216), and the exact Euclidean distance transform.
// Its own translation unit: the kernels and the host entry points declared in include/afx.h (afx_frangi, afx_distance_transform_edt,
// afx_sampling_weights and their workspace queries).
//
// Everything is fp64 and every expression is evaluated operation by operation as NumPy / SciPy evaluate it (no FMA contraction), so the
// results follow the host pipeline to rounding: the Gaussian passes sum in scipy.ndimage's order with its kernel weights (NumPy's
// pairwise sum normalises them), the Hessian takes np.gradient's differences, and the EDT is exact (integer squared distances, one sqrt).
// No floating-point atomics (the per-image reductions run in one workgroup each; LDS integer atomics build the percentile's histograms):
// the results are deterministic.  Nothing allocates or synchronises: every call is hipGraph-capturable.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/afx.h"
#include "afx_internal.h"
#include "afx_image_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int IMG_MAX_SIDE = 16384;         // squared distances stay in uint32 with room to spare; one EDT row fits in LDS
constexpr int IMG_MAX_GRID_Y = 65535;       // images (x scales) ride on blockIdx.y
constexpr int IMG_BLOCK = 256;
constexpr int IMG_RED_BLOCK = 1024;
constexpr uint32_t EDT_INF = 0xffffffffu;

enum { FG_NONZERO = 0, FG_NORMALISED = 1, FG_SEGMENTATION = 2 };

struct Scales {
  int n;
  double sigma[IMG_MAX_SIGMAS];
  int radius[IMG_MAX_SIGMAS];
};

// One 1-D Gaussian pass of scipy.ndimage.gaussian_filter (correlate1d with symmetric weights: x[i] w0 first, then the pairs from the
// outermost inwards).  AXIS 0 filters along the rows index (the first pass; it reads the image, applies the pre-step threshold
// x > thresh -> 1 and the black-ridge inversion 1 - x on load), AXIS 1 along the columns (reads the first pass's planes).
// grid: (ceil(h w / 256), n_img * n_sigmas); plane (img, s) at ((img * S + s) * h * w).
template <int AXIS>
__global__ void __launch_bounds__(IMG_BLOCK) k_gauss_pass(const double* __restrict__ src, double* __restrict__ dst, int h, int w, Scales sc,
                                                          const double* __restrict__ thresh, int invert) {
  extern __shared__ double lds[];
  const int plane = blockIdx.y, img = plane / sc.n, s = plane % sc.n;
  const int r = sc.radius[s];
  double* wt = lds;
  gauss_weights(sc.sigma[s], r, wt, lds + (r + 1));
  const int64_t hw = (int64_t)h * w;
  const int p = blockIdx.x * IMG_BLOCK + threadIdx.x;
  if (p >= hw) return;
  const int row = p / w, col = p % w;
  double acc;
  if (AXIS == 0) {
    const double* im = src + (int64_t)img * hw;
    const double th = thresh ? thresh[img] : 0.0;
    auto ld = [&](int rr) {
      double x = im[(int64_t)reflect_index(rr, h) * w + col];
      if (thresh && x > th) x = 1.0;
      return invert ? 1.0 - x : x;
    };
    acc = ld(row) * wt[0];
    for (int j = r; j >= 1; --j) acc += (ld(row - j) + ld(row + j)) * wt[j];
  } else {
    const double* ln = src + (int64_t)plane * hw + (int64_t)row * w;
    acc = ln[col] * wt[0];
    for (int j = r; j >= 1; --j) acc += (ln[reflect_index(col - j, w)] + ln[reflect_index(col + j, w)]) * wt[j];
  }
  dst[(int64_t)plane * hw + p] = acc;
}

__device__ __forceinline__ double gcol(const double* G, int w, int r, int c) {
  const Diff d = grad_at(c, w);
  return (G[(int64_t)r * w + d.a] - G[(int64_t)r * w + d.b]) / d.div;
}
__device__ __forceinline__ double grow(const double* G, int h, int w, int r, int c) {
  const Diff d = grad_at(r, h);
  return (G[(int64_t)d.a * w + c] - G[(int64_t)d.b * w + c]) / d.div;
}

// Frangi vesselness (skimage 0.18.3 filters.ridges.frangi, 2-D): per scale, the Hessian of the smoothed image from np.gradient of
// np.gradient (hessian_matrix(order='rc') of that version lists the elements as [d2/dc2, d/dr d/dc, d2/dr2]), times sigma^2, its
// eigenvalues sorted by magnitude, v = exp(-rb / 2 beta^2) (1 - exp(-(l1^2 + l2^2) / 2 gamma^2)), rb = (l1 / |l2|)^2, zero where
// l2 > 0; out = max over the scales.  grid: (ceil(h w / 256), n_img)
__global__ void __launch_bounds__(IMG_BLOCK) k_vesselness(const double* __restrict__ G, double* __restrict__ out, int h, int w, Scales sc,
                                                          double beta, double gamma) {
  const int img = blockIdx.y;
  const int64_t hw = (int64_t)h * w;
  const int p = blockIdx.x * IMG_BLOCK + threadIdx.x;
  if (p >= hw) return;
  const int r = p / w, c = p % w;
  const double beta_sq = 2.0 * (beta * beta), gamma_sq = 2.0 * (gamma * gamma);
  const Diff dr = grad_at(r, h), dc = grad_at(c, w);
  double best = 0.0;
  for (int s = 0; s < sc.n; ++s) {
    const double* g = G + ((int64_t)img * sc.n + s) * hw;
    const double hcc = (gcol(g, w, r, dc.a) - gcol(g, w, r, dc.b)) / dc.div;
    const double hrc = (gcol(g, w, dr.a, c) - gcol(g, w, dr.b, c)) / dr.div;
    const double hrr = (grow(g, h, w, dr.a, c) - grow(g, h, w, dr.b, c)) / dr.div;
    const double s2 = sc.sigma[s] * sc.sigma[s];
    const double m00 = s2 * hcc, m01 = s2 * hrc, m11 = s2 * hrr;
    const double tr = (m00 + m11) / 2.0;
    const double dd = m00 - m11;
    const double disc = sqrt(4.0 * (m01 * m01) + dd * dd) / 2.0;
    const double lp = tr + disc, lm = tr - disc;
    const bool swap = fabs(lm) < fabs(lp);       // a stable sort by |lambda|: on a tie lambda1 = l+
    const double l1 = swap ? lm : lp, l2 = swap ? lp : lm;
    double den = fabs(l2);
    if (den == 0.0) den = 1e-10;
    const double q = l1 / den;
    const double rb = q * q;
    const double rg = l1 * l1 + l2 * l2;
    double v = exp(-rb / beta_sq) * (1.0 - exp(-rg / gamma_sq));
    if (l2 > 0.0) v = 0.0;
    if (s == 0 || !(v <= best)) best = v;        // np.max: a NaN propagates
  }
  out[(int64_t)img * hw + p] = best;
}

__device__ __forceinline__ uint64_t order_key(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_key(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// np.percentile(img, 10) ('linear') per image, one workgroup each: the two order statistics around (n - 1) * 0.1 by an 8-pass radix
// select over order-preserving 64-bit keys (LDS integer histograms), then NumPy's _lerp.  binary != 0: +inf (no pixel is raised).
__global__ void __launch_bounds__(IMG_RED_BLOCK) k_percentile10(const double* __restrict__ img, int64_t hw, int binary, double* __restrict__ thresh) {
  const int n = blockIdx.x;
  if (binary) {
    if (threadIdx.x == 0) thresh[n] = INFINITY;
    return;
  }
  const double* x = img + (int64_t)n * hw;
  __shared__ uint32_t hist[2][256];
  __shared__ uint64_t prefix[2];
  __shared__ uint32_t rank[2];
  const double vidx = (double)(hw - 1) * (10.0 / 100.0);
  const int64_t lo = hw == 1 ? 0 : (int64_t)floor(vidx);
  const int64_t hi = hw == 1 ? 0 : lo + 1;
  if (threadIdx.x == 0) { prefix[0] = prefix[1] = 0; rank[0] = (uint32_t)lo; rank[1] = (uint32_t)hi; }
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    const uint64_t himask = pass == 0 ? 0ull : (~0ull << (shift + 8));
    for (int i = threadIdx.x; i < 512; i += blockDim.x) (&hist[0][0])[i] = 0;
    __syncthreads();
    const uint64_t p0 = prefix[0], p1 = prefix[1];
    for (int64_t i = threadIdx.x; i < hw; i += blockDim.x) {
      const uint64_t k = order_key(x[i]);
      const uint32_t bin = (uint32_t)(k >> shift) & 255u;
      if ((k & himask) == p0) atomicAdd(&hist[0][bin], 1u);
      if ((k & himask) == p1) atomicAdd(&hist[1][bin], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      const int s = threadIdx.x;
      uint32_t cum = 0, want = rank[s];
      int b = 0;
      for (; b < 255; ++b) {
        if (want < cum + hist[s][b]) break;
        cum += hist[s][b];
      }
      rank[s] = want - cum;
      prefix[s] |= (uint64_t)b << shift;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double a = from_key(prefix[0]), b = from_key(prefix[1]);
    const double t = hw == 1 ? 1.0 : vidx - (double)lo;
    const double diff = b - a;
    thresh[n] = t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
  }
}

// Per-image min and max (mm[2 i], mm[2 i + 1]), one workgroup each.  seg != 0: of the segmentation mask (x < 1 -> 1, else 0).
__global__ void __launch_bounds__(IMG_RED_BLOCK) k_minmax(const double* __restrict__ x, int64_t hw, int seg, double* __restrict__ mm) {
  const int n = blockIdx.x;
  const double* v = x + (int64_t)n * hw;
  double lo = INFINITY, hi = -INFINITY;
  bool nan = false;
  for (int64_t i = threadIdx.x; i < hw; i += blockDim.x) {
    double a = v[i];
    if (seg) a = a < 1.0 ? 1.0 : 0.0;
    nan |= a != a;
    lo = a < lo ? a : lo;
    hi = a > hi ? a : hi;
  }
  __shared__ double slo[IMG_RED_BLOCK], shi[IMG_RED_BLOCK];
  __shared__ int snan;
  if (threadIdx.x == 0) snan = 0;
  slo[threadIdx.x] = lo;
  shi[threadIdx.x] = hi;
  __syncthreads();
  if (nan) snan = 1;                                 // a plain store of the same value: no atomic needed
  for (int k = IMG_RED_BLOCK / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) {
      slo[threadIdx.x] = slo[threadIdx.x + k] < slo[threadIdx.x] ? slo[threadIdx.x + k] : slo[threadIdx.x];
      shi[threadIdx.x] = shi[threadIdx.x + k] > shi[threadIdx.x] ? shi[threadIdx.x + k] : shi[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mm[2 * n] = snan ? NAN : slo[0];                 // np.min / np.max propagate a NaN
    mm[2 * n + 1] = snan ? NAN : shi[0];
  }
}

// Foreground test of the EDT input: FG_NONZERO x != 0; FG_NORMALISED (x - min) / (max - min) != 0 (the vesselness after get_weighted_img's
// min-max normalisation); FG_SEGMENTATION the host sampling_weights' mask (x < 1), min-subtracted and divided by its max when positive.
__device__ __forceinline__ bool foreground(double x, int mode, const double* mm) {
  if (mode == FG_NONZERO) return x != 0.0;
  if (mode == FG_NORMALISED) return (x - mm[0]) / (mm[1] - mm[0]) != 0.0;
  double m = (x < 1.0 ? 1.0 : 0.0) - mm[0];
  const double top = mm[1] - mm[0];
  if (top > 0.0) m /= top;
  return m != 0.0;
}

// EDT, first pass: per column, the distance to the nearest background pixel of that column (EDT_INF: none).  grid: (ceil(w / 256), n_img)
__global__ void __launch_bounds__(IMG_BLOCK) k_edt_columns(const double* __restrict__ x, int h, int w, int mode, const double* __restrict__ mm,
                                                           uint32_t* __restrict__ g) {
  const int img = blockIdx.y, c = blockIdx.x * IMG_BLOCK + threadIdx.x;
  if (c >= w) return;
  const int64_t hw = (int64_t)h * w;
  const double* v = x + (int64_t)img * hw;
  uint32_t* o = g + (int64_t)img * hw;
  const double* m = mm ? mm + 2 * img : nullptr;
  int64_t last = -1;                                  // row of the last background pixel seen going down
  for (int r = 0; r < h; ++r) {
    if (!foreground(v[(int64_t)r * w + c], mode, m)) last = r;
    o[(int64_t)r * w + c] = last < 0 ? EDT_INF : (uint32_t)(r - last);
  }
  last = -1;
  for (int r = h - 1; r >= 0; --r) {
    const int64_t i = (int64_t)r * w + c;
    if (o[i] == 0) last = r;
    else if (last >= 0 && (uint32_t)(last - r) < o[i]) o[i] = (uint32_t)(last - r);
  }
}

// EDT, second pass: per row, the exact lower envelope min over c' of g(c')^2 + (c - c')^2 - searched outwards from c, stopping once
// (c - c')^2 alone reaches the best found; the row of g in LDS.  out = sqrt(d^2) in fp64 (+inf: no background pixel in the image).
// grid: (h, n_img), dynamic LDS w * 4 bytes
__global__ void __launch_bounds__(IMG_BLOCK) k_edt_rows(const uint32_t* __restrict__ g, int h, int w, double* __restrict__ out) {
  extern __shared__ uint32_t row[];
  const int img = blockIdx.y, r = blockIdx.x;
  const int64_t off = (int64_t)img * h * w + (int64_t)r * w;
  for (int c = threadIdx.x; c < w; c += blockDim.x) row[c] = g[off + c];
  __syncthreads();
  for (int c = threadIdx.x; c < w; c += blockDim.x) {
    uint32_t best = EDT_INF;
    for (int d = 0; d < w; ++d) {
      const uint32_t d2 = (uint32_t)d * (uint32_t)d;
      if (d2 >= best) break;
      if (c - d >= 0 && row[c - d] != EDT_INF) { const uint32_t v = row[c - d] * row[c - d] + d2; best = v < best ? v : best; }
      if (c + d < w && row[c + d] != EDT_INF) { const uint32_t v = row[c + d] * row[c + d] + d2; best = v < best ? v : best; }
    }
    out[off + c] = best == EDT_INF ? INFINITY : sqrt((double)best);
  }
}

// The last step of get_weighted_img: e = (e - min) / (max - min) + 1e-10.  frangi != 0: an image whose vesselness (fmm) or distance
// transform (emm) has max == min gets NaN (what the reference computes) and status bit 1 / 2; otherwise (the host segmentation rule) the
// division is skipped when max - min is 0.  grid: (ceil(h w / 256), n_img)
__global__ void __launch_bounds__(IMG_BLOCK) k_weights_final(double* __restrict__ e, int64_t hw, int frangi, const double* __restrict__ fmm,
                                                             const double* __restrict__ emm, int32_t* __restrict__ status) {
  const int img = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * IMG_BLOCK + threadIdx.x;
  const double emin = emm[2 * img], etop = emm[2 * img + 1] - emin;
  int flags = 0;
  if (frangi) flags = (fmm[2 * img + 1] - fmm[2 * img] == 0.0 ? 1 : 0) | (etop == 0.0 ? 2 : 0);
  if (status && blockIdx.x == 0 && threadIdx.x == 0) status[img] = flags;
  if (p >= hw) return;
  double v = e[(int64_t)img * hw + p];
  if (flags) v = NAN;
  else {
    v -= emin;
    if (frangi || etop > 0.0) v /= etop;
    v += 1e-10;
  }
  e[(int64_t)img * hw + p] = v;
}

bool shape_ok(int32_t n, int32_t h, int32_t w, int min_side) {
  return n > 0 && h >= min_side && w >= min_side && h <= IMG_MAX_SIDE && w <= IMG_MAX_SIDE && n <= IMG_MAX_GRID_Y;
}

int fill_scales(const double* sigmas, int32_t n_sigmas, int32_t n, Scales* sc, const char* who) {
  if (!sigmas || n_sigmas <= 0 || n_sigmas > IMG_MAX_SIGMAS)
    return afx::set_error(AFX_E_INVALID, who, "need 1 <= n_sigmas <= 16 and a sigma array");
  if ((int64_t)n * n_sigmas > IMG_MAX_GRID_Y) return afx::set_error(AFX_E_INVALID, who, "n_images x n_sigmas must not exceed 65535");
  sc->n = n_sigmas;
  for (int s = 0; s < n_sigmas; ++s) {
    const double sg = sigmas[s];
    if (!(sg > 0.0) || !(4.0 * sg + 0.5 <= (double)IMG_MAX_RADIUS + 0.5))
      return afx::set_error(AFX_E_INVALID, who, "every sigma must be > 0 and give a radius int(4 sigma + 0.5) <= 1000");
    sc->sigma[s] = sg;
    sc->radius[s] = (int)(4.0 * sg + 0.5);           // scipy.ndimage.gaussian_filter1d: int(truncate * sigma + 0.5), truncate = 4
  }
  return AFX_OK;
}

int max_radius(const Scales& sc) {
  int r = 0;
  for (int s = 0; s < sc.n; ++s) r = sc.radius[s] > r ? sc.radius[s] : r;
  return r;
}

struct FrangiBufs { double* t; double* g; };
FrangiBufs carve_frangi(afx::Carve& c, int32_t n, int32_t h, int32_t w, int32_t n_sigmas) {
  const size_t plane = (size_t)n * n_sigmas * h * w * sizeof(double);
  FrangiBufs b;
  b.t = c.take<double>(plane);
  b.g = c.take<double>(plane);
  return b;
}

struct WeightBufs { double* thresh; FrangiBufs fr; uint32_t* g; double* fmm; double* emm; };
WeightBufs carve_weights(afx::Carve& c, int32_t n, int32_t h, int32_t w, int32_t n_sigmas) {
  WeightBufs b;
  b.thresh = c.take<double>((size_t)n * sizeof(double));
  b.fmm = c.take<double>((size_t)2 * n * sizeof(double));
  b.emm = c.take<double>((size_t)2 * n * sizeof(double));
  b.g = c.take<uint32_t>((size_t)n * h * w * sizeof(uint32_t));
  b.fr = n_sigmas > 0 ? carve_frangi(c, n, h, w, n_sigmas) : FrangiBufs{nullptr, nullptr};
  return b;
}

void launch_frangi(const double* img, int32_t n, int32_t h, int32_t w, const Scales& sc, double beta, double gamma, int black_ridges,
                   const double* thresh, double* out, const FrangiBufs& b, hipStream_t st) {
  const int64_t hw = (int64_t)h * w;
  const unsigned bx = (unsigned)((hw + IMG_BLOCK - 1) / IMG_BLOCK);
  const size_t lds = (size_t)(3 * max_radius(sc) + 2) * sizeof(double);      // weights r + 1, raw values 2 r + 1
  hipLaunchKernelGGL(k_gauss_pass<0>, dim3(bx, (unsigned)(n * sc.n)), dim3(IMG_BLOCK), lds, st, img, b.t, h, w, sc, thresh, black_ridges);
  hipLaunchKernelGGL(k_gauss_pass<1>, dim3(bx, (unsigned)(n * sc.n)), dim3(IMG_BLOCK), lds, st, b.t, b.g, h, w, sc, nullptr, 0);
  hipLaunchKernelGGL(k_vesselness, dim3(bx, (unsigned)n), dim3(IMG_BLOCK), 0, st, b.g, out, h, w, sc, beta, gamma);
}

void launch_edt(const double* x, int32_t n, int32_t h, int32_t w, int mode, const double* mm, uint32_t* g, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_edt_columns, dim3((unsigned)((w + IMG_BLOCK - 1) / IMG_BLOCK), (unsigned)n), dim3(IMG_BLOCK), 0, st, x, h, w, mode, mm, g);
  hipLaunchKernelGGL(k_edt_rows, dim3((unsigned)h, (unsigned)n), dim3(IMG_BLOCK), (size_t)w * sizeof(uint32_t), st, g, h, w, out);
}

}  // namespace

extern "C" size_t afx_frangi_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t n_sigmas) {
  if (!shape_ok(n, h, w, 2) || n_sigmas <= 0 || n_sigmas > IMG_MAX_SIGMAS) return 0;
  afx::Carve c;
  carve_frangi(c, n, h, w, n_sigmas);
  return c.end;
}

extern "C" int afx_frangi(const double* img, int32_t n, int32_t h, int32_t w, const double* sigmas, int32_t n_sigmas, double beta, double gamma,
                          int32_t black_ridges, double* out, void* workspace, size_t workspace_bytes, size_t* workspace_needed, void* stream) {
  const char* who = "afx_frangi";
  if (!img || !out) return afx::set_error(AFX_E_INVALID, who, "null image or output");
  if (!shape_ok(n, h, w, 2)) return afx::set_error(AFX_E_INVALID, who, "need 1 <= n <= 65535 images of 2..16384 x 2..16384 pixels");
  Scales sc;
  if (int rc = fill_scales(sigmas, n_sigmas, n, &sc, who)) return rc;
  if (!(beta > 0.0) || !(gamma > 0.0) || !isfinite(beta) || !isfinite(gamma)) return afx::set_error(AFX_E_INVALID, who, "beta and gamma must be finite and > 0");
  const size_t need = afx_frangi_workspace_bytes(n, h, w, n_sigmas);
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(img, "the image", who)) return rc;
  afx::Carve c;
  c.base = (uintptr_t)workspace;
  const FrangiBufs b = carve_frangi(c, n, h, w, n_sigmas);
  launch_frangi(img, n, h, w, sc, beta, gamma, black_ridges, nullptr, out, b, (hipStream_t)stream);
  return afx::launched(who);
}

extern "C" size_t afx_distance_transform_edt_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  if (!shape_ok(n, h, w, 1)) return 0;
  afx::Carve c;
  c.take<uint32_t>((size_t)n * h * w * sizeof(uint32_t));
  return c.end;
}

extern "C" int afx_distance_transform_edt(const double* x, int32_t n, int32_t h, int32_t w, double* out, void* workspace, size_t workspace_bytes,
                                          size_t* workspace_needed, void* stream) {
  const char* who = "afx_distance_transform_edt";
  if (!x || !out) return afx::set_error(AFX_E_INVALID, who, "null input or output");
  if (!shape_ok(n, h, w, 1)) return afx::set_error(AFX_E_INVALID, who, "need 1 <= n <= 65535 images of 1..16384 x 1..16384 pixels");
  const size_t need = afx_distance_transform_edt_workspace_bytes(n, h, w);
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(x, "the image", who)) return rc;
  launch_edt(x, n, h, w, FG_NONZERO, nullptr, (uint32_t*)workspace, out, (hipStream_t)stream);
  return afx::launched(who);
}

extern "C" size_t afx_sampling_weights_workspace_bytes(int32_t strategy, int32_t n, int32_t h, int32_t w, int32_t n_sigmas) {
  if (strategy == AFX_SAMPLING_FRANGI) {
    if (!shape_ok(n, h, w, 2) || n_sigmas <= 0 || n_sigmas > IMG_MAX_SIGMAS) return 0;
  } else if (strategy == AFX_SAMPLING_SEGMENTATION) {
    if (!shape_ok(n, h, w, 1)) return 0;
    n_sigmas = 0;
  } else {
    return 0;
  }
  afx::Carve c;
  carve_weights(c, n, h, w, n_sigmas);
  return c.end;
}

extern "C" int afx_sampling_weights(const double* img, int32_t n, int32_t h, int32_t w, int32_t strategy, int32_t binary, const double* sigmas,
                                    int32_t n_sigmas, double beta, double gamma, double* out, int32_t* status, void* workspace,
                                    size_t workspace_bytes, size_t* workspace_needed, void* stream) {
  const char* who = "afx_sampling_weights";
  if (!img || !out) return afx::set_error(AFX_E_INVALID, who, "null image or output");
  const bool frangi = strategy == AFX_SAMPLING_FRANGI;
  if (!frangi && strategy != AFX_SAMPLING_SEGMENTATION) return afx::set_error(AFX_E_INVALID, who, "unknown strategy");
  if (!shape_ok(n, h, w, frangi ? 2 : 1))
    return afx::set_error(AFX_E_INVALID, who, "need 1 <= n <= 65535 images of up to 16384 x 16384 pixels (2 x 2 at least for frangi)");
  Scales sc{};
  if (frangi) {
    if (int rc = fill_scales(sigmas, n_sigmas, n, &sc, who)) return rc;
    if (!(beta > 0.0) || !(gamma > 0.0) || !isfinite(beta) || !isfinite(gamma)) return afx::set_error(AFX_E_INVALID, who, "beta and gamma must be finite and > 0");
  }
  const size_t need = afx_sampling_weights_workspace_bytes(strategy, n, h, w, frangi ? n_sigmas : 0);
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(img, "the image", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  afx::Carve c;
  c.base = (uintptr_t)workspace;
  const WeightBufs b = carve_weights(c, n, h, w, frangi ? n_sigmas : 0);
  const int64_t hw = (int64_t)h * w;
  const unsigned bx = (unsigned)((hw + IMG_BLOCK - 1) / IMG_BLOCK);
  if (frangi) {
    // cttoray.py:210-216: the percentile pre-step, then get_weighted_img: frangi -> min-max -> EDT -> min-max -> + 1e-10
    hipLaunchKernelGGL(k_percentile10, dim3((unsigned)n), dim3(IMG_RED_BLOCK), 0, st, img, hw, binary, b.thresh);
    launch_frangi(img, n, h, w, sc, beta, gamma, 1, b.thresh, out, b.fr, st);        // the vesselness in `out`
    hipLaunchKernelGGL(k_minmax, dim3((unsigned)n), dim3(IMG_RED_BLOCK), 0, st, out, hw, 0, b.fmm);
    launch_edt(out, n, h, w, FG_NORMALISED, b.fmm, b.g, out, st);
  } else {
    hipLaunchKernelGGL(k_minmax, dim3((unsigned)n), dim3(IMG_RED_BLOCK), 0, st, img, hw, 1, b.fmm);
    launch_edt(img, n, h, w, FG_SEGMENTATION, b.fmm, b.g, out, st);
  }
  hipLaunchKernelGGL(k_minmax, dim3((unsigned)n), dim3(IMG_RED_BLOCK), 0, st, out, hw, 0, b.emm);
  hipLaunchKernelGGL(k_weights_final, dim3(bx, (unsigned)n), dim3(IMG_BLOCK), 0, st, out, hw, frangi ? 1 : 0, b.fmm, b.emm, status);
  return afx::launched(who);
}
