// afx_kernels_metrics.hip — metrics of the evaluation sweep (visualization/visualization.py of the reference): the SSIM of every view
// (torchmetrics' StructuralSimilarityIndexMeasure(data_range=1.0), :267, 411-417) and the ground-truth density grid the DICE 3D / DOT 3D
// scores compare the reconstruction with (gt_interpolator at np.meshgrid(t, t, t), :203-231).  Its own translation unit: the kernels and
// the host entry points declared in include/afx.h (afx_ssim and its workspace query, afx_volume_grid).
//
// fp64 throughout.  No floating-point atomics: a view's SSIM is the sum of per-tile partials taken in a fixed order, so it is bitwise
// reproducible and does not depend on how many views share the call.  Nothing allocates or synchronises: both calls are hipGraph-capturable.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include "../../include/afx.h"
#include "afx_internal.h"

// After the includes: vol_sample (afx_internal.h) keeps the contraction rules k_project_volume is compiled with.
#pragma clang fp contract(off)

namespace {

constexpr int SSIM_K = 11;                  // Gaussian taps (sigma 1.5); a window lies inside the image: h - 10 x w - 10 of them
constexpr int SSIM_TH = 16, SSIM_TW = 64;   // windows per tile: 16 rows x 64 columns (a wave's 64 lanes take one row)
constexpr int SSIM_PH = SSIM_TH + SSIM_K - 1, SSIM_PW = SSIM_TW + SSIM_K - 1;
constexpr int SSIM_BLOCK = 256;
constexpr int64_t MAX_BLOCKS = (1 << 24) - 1;        // gridDim.x * 256 threads stays below 2^32
constexpr int32_t GRID_MAX_N = 1 << 20;               // n^3 points and 4 n^3 bytes stay far inside int64
constexpr int GRID_BLOCK = 256;

struct Gauss { double g[SSIM_K]; };

// torchmetrics _gaussian(11, 1.5): exp(-((m - 5) / 1.5)^2 / 2), divided by the sum; the 2-D window is the outer product g g^T
Gauss ssim_gauss() {
  Gauss w;
  double s = 0.0;
  for (int m = 0; m < SSIM_K; ++m) {
    const double d = (double)(m - SSIM_K / 2) / 1.5;
    w.g[m] = exp(-(d * d) / 2.0);
    s += w.g[m];
  }
  for (int m = 0; m < SSIM_K; ++m) w.g[m] /= s;
  return w;
}

int64_t ssim_tiles(int32_t h, int32_t w) {
  return (int64_t)((h - 10 + SSIM_TH - 1) / SSIM_TH) * ((w - 10 + SSIM_TW - 1) / SSIM_TW);
}

bool ssim_shape_ok(int32_t n, int32_t h, int32_t w) {
  if (n < 1 || h < SSIM_K || w < SSIM_K) return false;
  if ((int64_t)h * w > INT32_MAX) return false;
  return ssim_tiles(h, w) <= MAX_BLOCKS / n;
}

// One workgroup per tile of 16 x 64 windows of one view (blockIdx.x = view * tiles + tile): the (16 + 10) x (64 + 10) patch of both
// images in LDS, the vertical 11-tap sums of x, y, x^2, y^2, x y into LDS, then per window the horizontal sums and torchmetrics'
// _ssim_update map ((2 mu_x mu_y + c1)(2 s_xy + c2)) / ((mu_x^2 + mu_y^2 + c1)(s_x^2 + s_y^2 + c2)), the variances clamped at 0.
// The tile's map values are summed in a fixed order (4 per thread, then a tree over the workgroup) into partial[blockIdx.x].
__global__ void __launch_bounds__(SSIM_BLOCK) k_ssim_tiles(const float* __restrict__ x, const float* __restrict__ y, int h, int w, int tiles_x,
                                                           int64_t tiles, Gauss gw, double* __restrict__ partial) {
  __shared__ double vs[5][SSIM_TH][SSIM_PW];
  __shared__ double red[SSIM_BLOCK];
  __shared__ float px[SSIM_PH][SSIM_PW], py[SSIM_PH][SSIM_PW];
  const int tid = threadIdx.x;
  const int64_t view = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - view * tiles);
  const int i0 = (tile / tiles_x) * SSIM_TH, j0 = (tile % tiles_x) * SSIM_TW;      // first window of the tile (its top-left pixel)
  const int64_t hw = (int64_t)h * w;
  const float* xv = x + view * hw;
  const float* yv = y + view * hw;
  for (int e = tid; e < SSIM_PH * SSIM_PW; e += SSIM_BLOCK) {
    const int r = e / SSIM_PW, c = e % SSIM_PW, gr = i0 + r, gc = j0 + c;
    const bool in = gr < h && gc < w;                  // the rest of the patch feeds no window of the image
    px[r][c] = in ? xv[(int64_t)gr * w + gc] : 0.f;
    py[r][c] = in ? yv[(int64_t)gr * w + gc] : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < SSIM_TH * SSIM_PW; e += SSIM_BLOCK) {
    const int r = e / SSIM_PW, c = e % SSIM_PW;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int k = 0; k < SSIM_K; ++k) {
      const double a = px[r + k][c], b = py[r + k][c], g = gw.g[k];
      s0 += g * a;
      s1 += g * b;
      s2 += g * (a * a);
      s3 += g * (b * b);
      s4 += g * (a * b);
    }
    vs[0][r][c] = s0; vs[1][r][c] = s1; vs[2][r][c] = s2; vs[3][r][c] = s3; vs[4][r][c] = s4;
  }
  __syncthreads();
  const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;    // (k data_range)^2, data_range 1
  double acc = 0.0;
  for (int e = tid; e < SSIM_TH * SSIM_TW; e += SSIM_BLOCK) {
    const int r = e / SSIM_TW, c = e % SSIM_TW;
    if (i0 + r >= h - 10 || j0 + c >= w - 10) continue;
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < SSIM_K; ++k)
      for (int q = 0; q < 5; ++q) m[q] += gw.g[k] * vs[q][r][c + k];
    const double mx2 = m[0] * m[0], my2 = m[1] * m[1], mxy = m[0] * m[1];
    const double sx2 = fmax(m[2] - mx2, 0.0), sy2 = fmax(m[3] - my2, 0.0), sxy = m[4] - mxy;
    const double upper = 2.0 * sxy + c2, lower = (sx2 + sy2) + c2;
    acc += ((2.0 * mxy + c1) * upper) / ((mx2 + my2 + c1) * lower);
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = SSIM_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) partial[blockIdx.x] = red[0];
}

// out[view] = (sum of the view's tile partials, strided per thread then a tree: a fixed order) / ((h - 10)(w - 10)).  grid: n
__global__ void __launch_bounds__(SSIM_BLOCK) k_ssim_finish(const double* __restrict__ partial, int64_t tiles, double count,
                                                            double* __restrict__ out) {
  __shared__ double red[SSIM_BLOCK];
  const int tid = threadIdx.x;
  const double* p = partial + (int64_t)blockIdx.x * tiles;
  double s = 0.0;
  for (int64_t t = tid; t < tiles; t += SSIM_BLOCK) s += p[t];
  red[tid] = s;
  __syncthreads();
  for (int k = SSIM_BLOCK / 2; k > 0; k >>= 1) {
    if (tid < k) red[tid] += red[tid + k];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = red[0] / count;
}

// out[i][j][k] = vol_sample at (t[j], t[i], t[k]) (np.meshgrid's 'xy' order), t[m] = np.linspace(lo, hi, n)[m] rounded to fp32:
// m * ((hi - lo) / (n - 1)) + lo, the last entry exactly hi.  Grid-stride over the n^3 points.
__global__ void __launch_bounds__(GRID_BLOCK) k_volume_grid(const afx::VolArgs v, double lo, double hi, int n, float* __restrict__ out) {
  const int64_t nn = (int64_t)n * n, total = nn * n;
  const double step = (hi - lo) / (double)(n - 1);
  auto t = [&](int64_t m) { return (double)(float)(m == n - 1 ? hi : (double)m * step + lo); };
  for (int64_t p = (int64_t)blockIdx.x * GRID_BLOCK + threadIdx.x; p < total; p += (int64_t)gridDim.x * GRID_BLOCK) {
    const int64_t i = p / nn, r = p - i * nn, j = r / n, k = r - j * n;
    out[p] = (float)afx::vol_sample(v, t(j), t(i), t(k));
  }
}

}  // namespace

extern "C" size_t afx_ssim_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  if (!ssim_shape_ok(n, h, w)) return 0;
  afx::Carve c;
  c.take<double>((size_t)n * ssim_tiles(h, w) * sizeof(double));
  return c.end;
}

extern "C" int afx_ssim(const float* preds, const float* targets, int32_t n, int32_t h, int32_t w, double* out, void* workspace,
                        size_t workspace_bytes, size_t* workspace_needed, void* stream) {
  const char* who = "afx_ssim";
  if (!preds || !targets || !out) return afx::set_error(AFX_E_INVALID, who, "null image or output");
  if (!ssim_shape_ok(n, h, w))
    return afx::set_error(AFX_E_INVALID, who, "need n >= 1 pairs of h x w >= 11 x 11 pixels, h w < 2^31 and n x tiles < 2^24");
  const size_t need = afx_ssim_workspace_bytes(n, h, w);
  if (workspace_needed) *workspace_needed = need;
  if (!workspace || workspace_bytes < need) return afx::set_error(AFX_E_WORKSPACE, who, "workspace too small");
  if (int rc = afx::check_device(preds, "preds", who)) return rc;
  if (int rc = afx::check_device(targets, "targets", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t tiles = ssim_tiles(h, w);
  const int tiles_x = (w - 10 + SSIM_TW - 1) / SSIM_TW;
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(k_ssim_tiles, dim3((unsigned)(n * tiles)), dim3(SSIM_BLOCK), 0, st, preds, targets, h, w, tiles_x, tiles, ssim_gauss(),
                     partial);
  hipLaunchKernelGGL(k_ssim_finish, dim3((unsigned)n), dim3(SSIM_BLOCK), 0, st, partial, tiles, (double)(h - 10) * (double)(w - 10), out);
  return afx::launched(who);
}

extern "C" int afx_volume_grid(const float* vol, int32_t nx, int32_t ny, int32_t nz, const double origin[3], const double spacing[3],
                               float fill_value, double lo, double hi, int32_t n, float* out, void* stream) {
  const char* who = "afx_volume_grid";
  if (!vol || !origin || !spacing || !out) return afx::set_error(AFX_E_INVALID, who, "null argument");
  if (nx < 2 || ny < 2 || nz < 2) return afx::set_error(AFX_E_INVALID, who, "the volume needs >= 2 voxels per axis");
  if (!(spacing[0] > 0 && spacing[1] > 0 && spacing[2] > 0)) return afx::set_error(AFX_E_INVALID, who, "spacing must be > 0");
  if (n < 2 || n > GRID_MAX_N) return afx::set_error(AFX_E_INVALID, who, "need 2 <= n <= 2^20 points per axis");
  if (!(lo < hi) || !isfinite(lo) || !isfinite(hi)) return afx::set_error(AFX_E_INVALID, who, "need finite lo < hi");
  if (int rc = afx::check_device(vol, "the volume", who)) return rc;
  afx::VolArgs v = {};
  v.vol = vol; v.nx = nx; v.ny = ny; v.nz = nz; v.x0 = origin[0]; v.y0 = origin[1]; v.z0 = origin[2];
  v.dx = spacing[0]; v.dy = spacing[1]; v.dz = spacing[2]; v.fill = fill_value;
  const int64_t total = (int64_t)n * n * n;
  const int64_t blocks = std::min<int64_t>((total + GRID_BLOCK - 1) / GRID_BLOCK, 1 << 20);
  hipLaunchKernelGGL(k_volume_grid, dim3((unsigned)blocks), dim3(GRID_BLOCK), 0, (hipStream_t)stream, v, lo, hi, (int)n, out);
  return afx::launched(who);
}
