// afx_image_common.h - device helpers shared by the 2-D image unit (afx_kernels_image.hip) and the 3-D vesselness unit
// (afx_kernels_frangi3d.hip): the pieces of scipy.ndimage.gaussian_filter and np.gradient that both restate operation by operation.
// Contraction is off from here on (the pragma at file scope also covers the including unit, which repeats it for its own kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int IMG_MAX_SIGMAS = 16;
constexpr int IMG_MAX_RADIUS = 1000;        // int(4 sigma + 0.5): sigma < 250

// numpy's pairwise summation (numpy/_core/src/umath/loops_utils.h.src, pairwise_sum for contiguous doubles): blocks of at most 128
// elements are summed with 8 interleaved accumulators, longer runs are split in two at a multiple of 8.  D bounds the recursion.
template <int D>
__device__ double np_pairwise_sum(const double* a, int n) {
  if (n < 8) {
    double s = -0.0;
    for (int i = 0; i < n; ++i) s += a[i];
    return s;
  }
  if (n <= 128 || D == 0) {
    double r[8];
    for (int k = 0; k < 8; ++k) r[k] = a[k];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int k = 0; k < 8; ++k) r[k] += a[i + k];
    double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) s += a[i];
    return s;
  }
  if constexpr (D > 0) {
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum<D - 1>(a, n2) + np_pairwise_sum<D - 1>(a + n2, n - n2);
  }
  return 0.0;
}

// scipy.ndimage._gaussian_kernel1d(sigma, 0, radius): phi = exp(-0.5 / sigma^2 * x^2), x = -r..r, divided by its (pairwise) sum.
// Written to w[0..r] (symmetric: w[j] is the weight of offsets +-j); raw[] holds the 2r+1 unnormalised values for the sum.
__device__ void gauss_weights(double sigma, int r, double* w, double* raw) {
  const double k = -0.5 / (sigma * sigma);
  for (int i = threadIdx.x; i <= 2 * r; i += blockDim.x) raw[i] = exp(k * (double)((i - r) * (i - r)));
  __syncthreads();
  __shared__ double total;
  if (threadIdx.x == 0) total = np_pairwise_sum<5>(raw, 2 * r + 1);
  __syncthreads();
  for (int j = threadIdx.x; j <= r; j += blockDim.x) w[j] = raw[r + j] / total;
  __syncthreads();
}

// scipy.ndimage mode 'reflect' (d c b a | a b c d | d c b a): period 2n, also when the radius exceeds the line
__device__ __forceinline__ int reflect_index(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// np.gradient, unit spacing, edge_order 1: the two neighbours of index i on a line of n (n >= 2) and the divisor
struct Diff { int a, b; double div; };
__device__ __forceinline__ Diff grad_at(int i, int n) {
  if (i == 0) return {1, 0, 1.0};
  if (i == n - 1) return {n - 1, n - 2, 1.0};
  return {i + 1, i - 1, 2.0};
}

}  // namespace
