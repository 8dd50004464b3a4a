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
#include "afx_scan.h"

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

// ---- The exact 3-D Euclidean distance transform and the surface-distance scores built on it (afx_distance_transform_edt_3d,
// afx_surface_metrics_3d).  Integer arithmetic up to the final sqrt / sum, so nothing depends on the order of execution.
constexpr uint32_t EDT3_NONE = AFX_EDT3D_NONE;        // no zero voxel (in the line so far / in the volume)
constexpr uint16_t EDT3_NONE16 = 0xffffu;             // the same for the first pass's 1-D distances (<= 1023)
constexpr int EDT3_BLOCK = 256;
constexpr int SM_BINS = 2048;                         // 11 bits per pass of the radix select: squared distances are below 2^22
constexpr int SM_MAX_PART = 2048;                     // workgroups of the gather = per-direction partial sums

// First pass: g[c] = the distance from voxel c to the nearest zero voxel of its own line along axis 2 (EDT3_NONE16: the line has none).
// A wave per line, 64 voxels at a time: the zero voxels of a chunk are one ballot, the nearest one at or below a lane the highest set
// bit below it (or the last zero of the chunks before); the sweep back does the same from above.  Loads and stores are contiguous.
__global__ void __launch_bounds__(EDT3_BLOCK) k_edt3_axis2(const uint8_t* __restrict__ fg, int64_t lines, int n2, uint16_t* __restrict__ g) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * EDT3_BLOCK + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * EDT3_BLOCK) >> 6;
  for (int64_t line = wave; line < lines; line += n_waves) {
    const uint8_t* v = fg + line * n2;
    uint16_t* o = g + line * n2;
    int last = -1;                                     // the last zero voxel before this chunk (the same in every lane)
    for (int c0 = 0; c0 < n2; c0 += 64) {
      const int c = c0 + lane;
      const bool in = c < n2;
      const unsigned long long m = __ballot(in && v[c] == 0);
      const unsigned long long below = m & ((2ull << lane) - 1ull);                 // zero voxels of the chunk at lanes <= mine
      const int l = below ? c0 + 63 - __builtin_clzll(below) : last;
      if (in) o[c] = l < 0 ? EDT3_NONE16 : (uint16_t)(c - l);
      if (m) last = c0 + 63 - __builtin_clzll(m);
    }
    int next = -1;                                     // the first zero voxel behind this chunk
    for (int c0 = (n2 - 1) / 64 * 64; c0 >= 0; c0 -= 64) {
      const int c = c0 + lane;
      const bool in = c < n2;
      const uint16_t cur = in ? o[c] : EDT3_NONE16;    // this lane's own store of the sweep forward
      const unsigned long long m = __ballot(in && cur == 0);
      const unsigned long long above = m & ~((1ull << lane) - 1ull);                 // zero voxels of the chunk at lanes >= mine
      const int r = above ? c0 + __builtin_ctzll(above) : next;
      if (in && r >= 0 && (uint32_t)(r - c) < (uint32_t)cur) o[c] = (uint16_t)(r - c);
      if (m) next = c0 + __builtin_ctzll(m);
    }
  }
}

// Second and third pass: along an axis of `len` voxels whose neighbours lie `inner` elements apart (axis 1: inner = n2, one launch
// block per (i, tile); axis 0: inner = n1 n2), out[c] = min over c' of g(c') + (c - c')^2 - the exact lower envelope, searched outwards
// from c and stopped once (c - c')^2 alone reaches the best found, as k_edt_rows (afx_kernels_image.hip) does.  A workgroup takes `tw`
// (16 or 32) ADJACENT lines, [len][tw] values in LDS: every global load and store is a run of tw consecutive elements, and the lanes of
// a wave's half read tw distinct LDS banks.  In = uint16_t: g is the first pass's distance, squared here; uint32_t: squared already, and
// the call may work in place (a workgroup has read its whole tile before it writes, and no other workgroup touches that tile).
// grid: outer * tiles, dynamic LDS len * tw * 4 bytes
template <class In>
__global__ void __launch_bounds__(EDT3_BLOCK) k_edt3_lines(const In* g, int len, int64_t inner, int tw_shift, int tiles, uint32_t* d2,
                                                           double* dist) {
  extern __shared__ uint32_t col[];
  const int tw = 1 << tw_shift;
  const int64_t outer = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - outer * tiles);
  const int64_t k0 = (int64_t)tile << tw_shift;
  const int kw = inner - k0 < tw ? (int)(inner - k0) : tw;          // lines of this tile that exist
  const int64_t base = outer * len * inner + k0;
  const int cells = len << tw_shift;
  for (int e = threadIdx.x; e < cells; e += EDT3_BLOCK) {
    const int r = e >> tw_shift, k = e & (tw - 1);
    uint32_t v = EDT3_NONE;
    if (k < kw) {
      const In x = g[base + (int64_t)r * inner + k];
      if (sizeof(In) == 2) v = x == (In)EDT3_NONE16 ? EDT3_NONE : (uint32_t)x * (uint32_t)x;
      else v = (uint32_t)x;
    }
    col[e] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < cells; e += EDT3_BLOCK) {
    const int r = e >> tw_shift, k = e & (tw - 1);
    if (k >= kw) continue;
    uint32_t best = EDT3_NONE;
    for (int d = 0; d < len; ++d) {
      const uint32_t dd = (uint32_t)d * (uint32_t)d;
      if (dd >= best) break;
      if (r - d >= 0) {
        const uint32_t v = col[((r - d) << tw_shift) + k];
        if (v != EDT3_NONE && v + dd < best) best = v + dd;
      }
      if (r + d < len) {
        const uint32_t v = col[((r + d) << tw_shift) + k];
        if (v != EDT3_NONE && v + dd < best) best = v + dd;
      }
    }
    const int64_t at = base + (int64_t)r * inner + k;
    d2[at] = best;
    if (dist) dist[at] = best == EDT3_NONE ? (double)INFINITY : sqrt((double)best);
  }
}

// tile width of k_edt3_lines as a shift: 32 lines while they fit in 64 KiB of LDS (len <= 512), else 16
int edt3_tw_shift(int len) { return len <= 512 ? 5 : 4; }

void launch_edt3(const uint8_t* fg, int32_t n0, int32_t n1, int32_t n2, uint16_t* g16, uint32_t* d2, double* dist, hipStream_t st) {
  const int64_t lines = (int64_t)n0 * n1, inner0 = (int64_t)n1 * n2;
  const int64_t b1 = std::min<int64_t>((lines + 3) / 4, 1 << 16);                 // 4 waves = 4 lines per workgroup, then a stride
  hipLaunchKernelGGL(k_edt3_axis2, dim3((unsigned)b1), dim3(EDT3_BLOCK), 0, st, fg, lines, (int)n2, g16);
  const int s1 = edt3_tw_shift(n1), t1 = (n2 + (1 << s1) - 1) >> s1;
  hipLaunchKernelGGL(k_edt3_lines<uint16_t>, dim3((unsigned)(n0 * t1)), dim3(EDT3_BLOCK), ((size_t)n1 << s1) * sizeof(uint32_t), st,
                     (const uint16_t*)g16, (int)n1, (int64_t)n2, s1, t1, d2, (double*)nullptr);
  const int s0 = edt3_tw_shift(n0), t0 = (int)((inner0 + (1 << s0) - 1) >> s0);
  hipLaunchKernelGGL(k_edt3_lines<uint32_t>, dim3((unsigned)t0), dim3(EDT3_BLOCK), ((size_t)n0 << s0) * sizeof(uint32_t), st,
                     (const uint32_t*)d2, (int)n0, inner0, s0, t0, d2, dist);
}

// Device-side state of afx_surface_metrics_3d between its launches (one 256-byte region of the workspace, zeroed by k_sm_init)
struct SmState {
  unsigned long long cnt[5];      // |A|, |B|, |A & B|, |S(A)|, |S(B)|
  unsigned long long rem[2];      // rank of the two order statistics inside their first-pass bin
  uint32_t bin[2];                // first-pass bin (the high 11 bits) of the two order statistics
  uint32_t mx[2];                 // max d^2 of D_A->B, D_B->A
  uint32_t status, pad;
  double vidx;                    // the virtual index
};
static_assert(sizeof(SmState) <= 256, "SmState has 256 bytes of the workspace");

__global__ void __launch_bounds__(256) k_sm_init(SmState* st, uint32_t* hist) {
  if (threadIdx.x == 0) *st = SmState{};
  for (int i = threadIdx.x; i < 3 * SM_BINS; i += 256) hist[i] = 0;
}

// Masks and counts: A = pred >= thr_pred, B = gt >= thr_gt; a voxel of M is on S(M) when one of its 6 face neighbours is outside M or
// beyond the grid.  na[p] = 0 on S(A), 1 elsewhere (the EDT's foreground: the distance to S(A)); nb likewise.  Counts: integer atomics.
__global__ void __launch_bounds__(256) k_sm_masks(const float* __restrict__ pred, const float* __restrict__ gt, int n0, int n1, int n2,
                                                  float thr_pred, float thr_gt, uint8_t* __restrict__ na, uint8_t* __restrict__ nb,
                                                  SmState* st) {
  __shared__ unsigned int c[5];
  if (threadIdx.x < 5) c[threadIdx.x] = 0;
  __syncthreads();
  const int64_t s0 = (int64_t)n1 * n2, total = s0 * n0;
  unsigned int mine[5] = {0, 0, 0, 0, 0};
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
    const int i = (int)(p / s0), r = (int)(p - i * s0), j = r / n2, k = r - j * n2;
    const bool lo0 = i > 0, hi0 = i < n0 - 1, lo1 = j > 0, hi1 = j < n1 - 1, lo2 = k > 0, hi2 = k < n2 - 1;
    const bool edge = !(lo0 && hi0 && lo1 && hi1 && lo2 && hi2);
    auto surface = [&](const float* v, float thr) {      // v[p] is inside the mask
      if (edge) return true;
      return !(v[p - s0] >= thr && v[p + s0] >= thr && v[p - n2] >= thr && v[p + n2] >= thr && v[p - 1] >= thr && v[p + 1] >= thr);
    };
    const bool a = pred[p] >= thr_pred, b = gt[p] >= thr_gt;
    const bool sa = a && surface(pred, thr_pred), sb = b && surface(gt, thr_gt);
    na[p] = sa ? 0 : 1;
    nb[p] = sb ? 0 : 1;
    mine[0] += a; mine[1] += b; mine[2] += a && b; mine[3] += sa; mine[4] += sb;
  }
  for (int q = 0; q < 5; ++q)
    if (mine[q]) atomicAdd(&c[q], mine[q]);
  __syncthreads();
  if (threadIdx.x < 5 && c[threadIdx.x]) atomicAdd(&st->cnt[threadIdx.x], (unsigned long long)c[threadIdx.x]);
}

// The two multisets, read where the masks mark a surface voxel: D_A->B = d2b at S(A) (na == 0), D_B->A = d2a at S(B).
// PASS 1: the fp64 sums of sqrt(d^2) per direction as one partial per workgroup (a tree: a fixed order), the maxima, and the histogram
// of the merged keys' high 11 bits.  PASS 2: the histograms of the low 11 bits of the keys in the bin of the lower order statistic
// (hist[0..]) and of the upper one (hist[SM_BINS..]).  LDS histograms, added to the global ones with integer atomics.
template <int PASS>
__global__ void __launch_bounds__(256) k_sm_gather(const uint8_t* __restrict__ na, const uint8_t* __restrict__ nb, const uint32_t* __restrict__ d2a,
                                                   const uint32_t* __restrict__ d2b, int64_t total, SmState* st, uint32_t* __restrict__ hist,
                                                   double* __restrict__ partial) {
  __shared__ uint32_t h[PASS == 1 ? 1 : 2][SM_BINS];
  __shared__ double red[2][256];
  __shared__ uint32_t smx[2];
  const int tid = threadIdx.x;
  for (int i = tid; i < (PASS == 1 ? 1 : 2) * SM_BINS; i += 256) (&h[0][0])[i] = 0;
  if (tid < 2) smx[tid] = 0;
  __syncthreads();
  const uint32_t bin0 = st->bin[0], bin1 = st->bin[1];
  double sum[2] = {0.0, 0.0};
  uint32_t mx[2] = {0, 0};
  for (int64_t p = (int64_t)blockIdx.x * 256 + tid; p < total; p += (int64_t)gridDim.x * 256) {
    const bool on[2] = {na[p] == 0, nb[p] == 0};
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
      if (!on[dir]) continue;
      const uint32_t key = dir == 0 ? d2b[p] : d2a[p];
      const uint32_t hi = key >> 11;
      if (PASS == 1) {
        sum[dir] += sqrt((double)key);
        mx[dir] = key > mx[dir] ? key : mx[dir];
        atomicAdd(&h[0][hi < SM_BINS ? hi : SM_BINS - 1], 1u);          // only the no-zero-voxel mark lies beyond: status != 0 then
      } else {
        if (hi == bin0) atomicAdd(&h[0][key & (SM_BINS - 1)], 1u);
        if (hi == bin1) atomicAdd(&h[PASS == 1 ? 0 : 1][key & (SM_BINS - 1)], 1u);
      }
    }
  }
  if (PASS == 1) {
    red[0][tid] = sum[0];
    red[1][tid] = sum[1];
    if (mx[0]) atomicMax(&smx[0], mx[0]);
    if (mx[1]) atomicMax(&smx[1], mx[1]);
  }
  __syncthreads();
  if (PASS == 1) {
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
      __syncthreads();
    }
    if (tid < 2) {
      partial[2 * (int64_t)blockIdx.x + tid] = red[tid][0];
      if (smx[tid]) atomicMax(&st->mx[tid], smx[tid]);
    }
  }
  for (int i = tid; i < (PASS == 1 ? 1 : 2) * SM_BINS; i += 256) {
    const uint32_t v = (&h[0][0])[i];
    if (v) atomicAdd(&hist[i], v);
  }
}

// The bin of hist[SM_BINS] that holds rank r (0-based, ascending) and r's rank inside it; every thread of the 256 calls it and gets the
// same answer (sh: 256 counts and the two results in LDS).  A rank beyond the histogram's total gives bin 0.
struct SmFind { unsigned long long below[256]; unsigned long long rem; uint32_t bin; };
__device__ void sm_find(const uint32_t* hist, unsigned long long r, SmFind* sh, uint32_t* bin, unsigned long long* rem) {
  const int t = threadIdx.x;
  uint32_t c[8];
  unsigned long long s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { c[j] = hist[8 * t + j]; s += c[j]; }
  __syncthreads();                                     // the previous call's results have been read
  sh->below[t] = s;
  if (t == 0) { sh->bin = 0; sh->rem = 0; }
  __syncthreads();
  if (t == 0) {
    unsigned long long run = 0;
    for (int g = 0; g < 256; ++g) { const unsigned long long v = sh->below[g]; sh->below[g] = run; run += v; }
  }
  __syncthreads();
  unsigned long long a = sh->below[t];
  if (a <= r && r < a + s) {                           // exactly one group of 8 bins holds the rank
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (a <= r && r < a + c[j]) { sh->bin = (uint32_t)(8 * t + j); sh->rem = r - a; }
      a += c[j];
    }
  }
  __syncthreads();
  *bin = sh->bin;
  *rem = sh->rem;
}

// One workgroup, after the first histogram: the status, the virtual index v = (M - 1) quant in fp64 (np.percentile's 'linear' rule:
// (n - 1) * (q / 100)), the two ranks floor(v) and min(floor(v) + 1, M - 1), and the first-pass bin of each.
__global__ void __launch_bounds__(256) k_sm_scan(SmState* st, const uint32_t* hist, double quant) {
  __shared__ SmFind sh;
  const unsigned long long m = st->cnt[3] + st->cnt[4];
  const uint32_t status = (st->cnt[0] == 0 ? 1u : 0u) | (st->cnt[1] == 0 ? 2u : 0u);
  if (status) {                                        // the same in every thread
    if (threadIdx.x == 0) { st->status = status; st->vidx = NAN; st->bin[0] = st->bin[1] = EDT3_NONE; }      // no key has this bin
    return;
  }
  const double v = (double)(m - 1) * quant;
  unsigned long long k0 = (unsigned long long)floor(v);
  if (k0 > m - 1) k0 = m - 1;
  const unsigned long long k1 = k0 + 1 < m ? k0 + 1 : m - 1;
  uint32_t b0, b1;
  unsigned long long r0, r1;
  sm_find(hist, k0, &sh, &b0, &r0);
  sm_find(hist, k1, &sh, &b1, &r1);
  if (threadIdx.x == 0) { st->status = 0; st->vidx = v; st->bin[0] = b0; st->bin[1] = b1; st->rem[0] = r0; st->rem[1] = r1; }
}

// One workgroup: the record.  The sums: the gather's partials strided per thread, then a tree.  The order statistics: the rank left
// inside the first-pass bin, looked up in the second histograms.
__global__ void __launch_bounds__(256) k_sm_finish(const SmState* st, const uint32_t* hist2, const double* __restrict__ partial, int n_part,
                                                   unsigned long long* __restrict__ record) {
  __shared__ SmFind sh;
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int g = tid; g < n_part; g += 256) { s0 += partial[2 * g]; s1 += partial[2 * g + 1]; }
  red[0][tid] = s0;
  red[1][tid] = s1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
    __syncthreads();
  }
  const uint32_t status = st->status;
  uint32_t lo[2] = {0, 0};
  unsigned long long rem;
  if (!status) {                                       // the same in every thread
    sm_find(hist2, st->rem[0], &sh, &lo[0], &rem);
    sm_find(hist2 + SM_BINS, st->rem[1], &sh, &lo[1], &rem);
  }
  if (tid != 0) return;
  for (int q = 0; q < 5; ++q) record[q] = st->cnt[q];
  const double nan = NAN;
  record[5] = (unsigned long long)__double_as_longlong(status ? nan : red[0][0]);
  record[6] = (unsigned long long)__double_as_longlong(status ? nan : red[1][0]);
  record[7] = status ? EDT3_NONE : st->mx[0];
  record[8] = status ? EDT3_NONE : st->mx[1];
  record[9] = status ? EDT3_NONE : ((st->bin[0] << 11) | lo[0]);
  record[10] = status ? EDT3_NONE : ((st->bin[1] << 11) | lo[1]);
  record[11] = (unsigned long long)__double_as_longlong(st->vidx);
  record[12] = status;
  for (int q = 13; q < AFX_SURFACE_RECORD_SLOTS; ++q) record[q] = 0;
}

struct SurfaceBufs { uint8_t* na; uint8_t* nb; uint16_t* g16; uint32_t* d2a; uint32_t* d2b; double* partial; uint32_t* hist; SmState* st; };
SurfaceBufs carve_surface(afx::Carve& c, int32_t n0, int32_t n1, int32_t n2) {
  const size_t n = (size_t)n0 * n1 * n2;
  SurfaceBufs b;
  b.na = c.take<uint8_t>(n);
  b.nb = c.take<uint8_t>(n);
  b.g16 = c.take<uint16_t>(n * sizeof(uint16_t));
  b.d2a = c.take<uint32_t>(n * sizeof(uint32_t));
  b.d2b = c.take<uint32_t>(n * sizeof(uint32_t));
  b.partial = c.take<double>((size_t)2 * SM_MAX_PART * sizeof(double));
  b.hist = c.take<uint32_t>((size_t)3 * SM_BINS * sizeof(uint32_t));
  b.st = c.take<SmState>(256);
  return b;
}

// ---- 3-D connected-component labelling (afx_label_components_3d, afx_filter_components_3d): union-find in global memory after Komura
// (2015) and Playne & Hawick (2018).  Labels are a pure function of the input - components numbered 1..K in raster order of their first
// voxel, scipy.ndimage.label's numbering - so the integer atomics below leave nothing to the order of execution.  One fixed launch
// sequence: init, merge, flatten (+ roots per chunk), scan, rank, relabel (+ sizes), finish.
constexpr uint32_t CC_NONE = 0xffffffffu;             // parent[] of a background voxel
constexpr int CC_BLOCK = 256;
constexpr int CC_CHUNK = 2048;                        // consecutive voxels per workgroup of the chunked kernels: 8 per thread, coalesced
constexpr int CC_ITERS = CC_CHUNK / CC_BLOCK;

struct CcState { uint32_t k; };                       // 256 bytes of the workspace: the number of components, written by k_cc_scan

// parent[v] = v on the foreground, CC_NONE elsewhere; sizes[] = 0 (all N entries: those at and beyond K stay 0)
__global__ void __launch_bounds__(CC_BLOCK) k_cc_init(const uint8_t* __restrict__ fg, uint32_t total, uint32_t* __restrict__ parent,
                                                      uint32_t* __restrict__ sizes) {
#pragma unroll
  for (int i = 0; i < CC_ITERS; ++i) {
    const uint32_t v = blockIdx.x * CC_CHUNK + i * CC_BLOCK + threadIdx.x;
    if (v < total) {
      parent[v] = fg[v] ? v : CC_NONE;
      sizes[v] = 0;
    }
  }
}

__device__ __forceinline__ uint32_t cc_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's tree as far as this thread can see it.  Terminates: the walk goes on only to a strictly smaller index.
__device__ __forceinline__ uint32_t cc_find(const uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = cc_load(&parent[x]);
    if (p >= x) return x;                             // a root (parent[x] == x; nothing larger is ever stored)
    x = p;
  }
}

// Unites the sets of a and b.  A thread that holds the duty "a ~ b" (a > b) calls atomicMin(&parent[a], b) and reads what stood there:
// a itself - a was a root and now hangs below b, the duty is done; old > b - the link a -> old was replaced by a -> b, so the duty
// becomes "old ~ b"; old < b - the link a -> old stays and the duty becomes "b ~ old".  In each case the links and duties together
// connect exactly what they connected before, and the larger index of the pair has strictly decreased.
__device__ __forceinline__ void cc_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  a = cc_find(parent, a);
  b = cc_find(parent, b);
  while (a != b) {
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicMin(&parent[a], b);
    if (old >= a) break;                              // old == a: a was a root
    a = cc_find(parent, old);                         // <= old < a
  }
}

// Merge: every foreground voxel unites itself with the foreground neighbours that precede it in raster order (3, 9 or 13 of them for
// C = 1, 2, 3: |di| + |dj| + |dk| <= C, scipy.ndimage.generate_binary_structure(3, C)); beyond the grid is background.
// Every access to parent[] in this launch is an agent-scope atomic (cc_load, atomicMin): no plain store, and nothing depends on a load
// being fresh - parent[x] <= x and it only ever decreases, so a stale value is an older ancestor in the same set, and atomicMin's return
// value is what decides.  No thread waits for another.  TERMINATION, each loop by the thread's own action:
//   (1) cc_find: the index strictly decreases with every step and is bounded below by 0.
//   (2) cc_unite: on every retry max(a, b) strictly decreases (the new a is <= old < the former a = max, b is unchanged or becomes the
//       new max below the former one), so the pair (max, min) decreases lexicographically and the loop ends after at most a steps.
// Roots only ever link to smaller indices, so the final root of a component is its smallest linear index.
template <int C>
__global__ void __launch_bounds__(CC_BLOCK) k_cc_merge(const uint8_t* __restrict__ fg, int n0, int n1, int n2, uint32_t* parent) {
  const int s0 = n1 * n2;
  const uint32_t total = (uint32_t)n0 * (uint32_t)s0;
  const uint32_t v = blockIdx.x * CC_BLOCK + threadIdx.x;
  if (v >= total || !fg[v]) return;
  const int i = (int)(v / (uint32_t)s0), r = (int)(v - (uint32_t)i * (uint32_t)s0), j = r / n2, k = r - j * n2;
#pragma unroll
  for (int di = -1; di <= 0; ++di)
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
      for (int dk = -1; dk <= 1; ++dk) {
        const bool before = di < 0 || (dj < 0 || (dj == 0 && dk < 0));
        if (!before || (di != 0) + (dj != 0) + (dk != 0) > C) continue;
        if (i + di < 0 || j + dj < 0 || j + dj >= n1 || k + dk < 0 || k + dk >= n2) continue;
        const uint32_t u = (uint32_t)((int)v + di * s0 + dj * n2 + dk);
        if (fg[u]) cc_unite(parent, v, u);
      }
}

// Flatten (its own launch: the merge's links are published by the kernel boundary, parent[] is only read): root[v] = the root of v, -1 on
// the background, written to a second array - the labels output - and count[chunk] = the roots among the chunk's voxels.
__global__ void __launch_bounds__(CC_BLOCK) k_cc_flatten(const uint32_t* __restrict__ parent, uint32_t total, int32_t* __restrict__ root,
                                                         uint32_t* __restrict__ count) {
  __shared__ uint32_t wsum[CC_BLOCK / 64];
  uint32_t roots = 0;                                 // of this wave (the same in every lane)
#pragma unroll
  for (int i = 0; i < CC_ITERS; ++i) {
    const uint32_t v = blockIdx.x * CC_CHUNK + i * CC_BLOCK + threadIdx.x;
    bool is_root = false;
    if (v < total) {
      uint32_t x = parent[v];
      if (x == CC_NONE) root[v] = -1;
      else {
        is_root = x == v;
        for (uint32_t p = parent[x]; p < x; p = parent[x]) x = p;
        root[v] = (int32_t)x;
      }
    }
    roots += (uint32_t)__popcll(__ballot(is_root));
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = roots;
  __syncthreads();
  if (threadIdx.x == 0) count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup: count[nb] becomes its own exclusive scan (the roots before each chunk); st->k = the total, K
__global__ void __launch_bounds__(1024) k_cc_scan(uint32_t* count, uint32_t nb, CcState* st) {
  uint32_t b0, b1, p[1] = {0}, tot[1];
  afx::scan_run<1024>(nb, b0, b1);
  for (uint32_t b = b0; b < b1; ++b) p[0] += count[b];
  afx::block_exclusive_scan<1024>(p, tot);            // p: the roots before this thread's chunks
  for (uint32_t b = b0; b < b1; ++b) { const uint32_t c = count[b]; count[b] = p[0]; p[0] += c; }
  if (threadIdx.x == 1023) st->k = tot[0];
}

// Rank: the label of a root is 1 + the number of roots before it in raster order = 1 + pre[chunk] + the roots before it in its chunk
// (ballots per wave and pass, their counts through LDS).  Stored in parent[root]: the merge tree is not needed any more.
__global__ void __launch_bounds__(CC_BLOCK) k_cc_rank(const int32_t* __restrict__ root, uint32_t total, const uint32_t* __restrict__ pre,
                                                      uint32_t* __restrict__ parent) {
  __shared__ uint32_t wc[CC_ITERS][CC_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long m[CC_ITERS];
#pragma unroll
  for (int i = 0; i < CC_ITERS; ++i) {
    const uint32_t v = blockIdx.x * CC_CHUNK + i * CC_BLOCK + threadIdx.x;
    m[i] = __ballot(v < total && root[v] == (int32_t)v);
    if (lane == 0) wc[i][wave] = (uint32_t)__popcll(m[i]);
  }
  __syncthreads();
  uint32_t run = pre[blockIdx.x] + 1;
#pragma unroll
  for (int i = 0; i < CC_ITERS; ++i) {
    uint32_t before = run;
    for (int w = 0; w < wave; ++w) before += wc[i][w];
    if ((m[i] >> lane) & 1ull)
      parent[blockIdx.x * CC_CHUNK + i * CC_BLOCK + threadIdx.x] = before + (uint32_t)__popcll(m[i] & ((1ull << lane) - 1ull));
    run += wc[i][0] + wc[i][1] + wc[i][2] + wc[i][3];
  }
}

// Relabel and sizes: labels[v] = the label of v's root (0 on the background), in place over the roots.  sizes[label - 1] counts with
// integer atomics, aggregated first: a wave adds once per DISTINCT label among its 64 consecutive voxels (ballots), and while the
// foreground lanes of its passes all carry one label (a dense mask: nearly every voxel on one counter, holes or not) it keeps the count
// and adds once at the end - one add per 512 voxels on a contended counter.  (Adding once per run of equal labels was measured first:
// at 90 % random foreground the holes cut the runs to about ten voxels and the launch took 9.4 ms of the call's 13.)
__global__ void __launch_bounds__(CC_BLOCK) k_cc_relabel(int32_t* __restrict__ labels, uint32_t total, const uint32_t* __restrict__ parent,
                                                         uint32_t* __restrict__ sizes) {
  const int lane = threadIdx.x & 63;
  uint32_t held = 0, held_n = 0;                      // a label whose count this wave still holds (the same in every lane; 0: none)
#pragma unroll
  for (int i = 0; i < CC_ITERS; ++i) {
    const uint32_t v = blockIdx.x * CC_CHUNK + i * CC_BLOCK + threadIdx.x;
    uint32_t l = 0;
    if (v < total) {
      const int32_t r = labels[v];
      if (r >= 0) l = parent[r];
      labels[v] = (int32_t)l;
    }
    const unsigned long long fgm = __ballot(l != 0);
    if (fgm == 0) continue;                           // a wave of background (the same decision in every lane, as all below)
    const uint32_t l0 = __shfl(l, __builtin_ctzll(fgm));
    const unsigned long long same = __ballot(l == l0);
    if (same == fgm) {                                // one label among the foreground lanes
      if (l0 != held) {
        if (held && lane == 0) atomicAdd(&sizes[held - 1], held_n);
        held = l0;
        held_n = 0;
      }
      held_n += (uint32_t)__popcll(same);
      continue;
    }
    if (held && lane == 0) atomicAdd(&sizes[held - 1], held_n);
    held = 0;
    held_n = 0;
    unsigned long long todo = fgm;                    // several labels: one add each; every pass clears at least its first lane's bit
    while (todo) {
      const int first = __builtin_ctzll(todo);
      const uint32_t lx = __shfl(l, first);
      const unsigned long long m = __ballot(l == lx);
      if (lane == first) atomicAdd(&sizes[lx - 1], (uint32_t)__popcll(m));
      todo &= ~m;
    }
  }
  if (held && lane == 0) atomicAdd(&sizes[held - 1], held_n);
}

// One workgroup: the record.  The largest component has the greatest size, ties going to the smaller label: the maximum of
// (size << 32) | ~label.  Its first voxel is its root, which lies in the chunk c with pre[c] < label <= pre[c + 1] and is the first
// voxel there that carries the label.
__global__ void __launch_bounds__(1024) k_cc_finish(const CcState* st, const uint32_t* __restrict__ sizes, const int32_t* __restrict__ labels,
                                                    uint32_t total, const uint32_t* __restrict__ pre, uint32_t nb,
                                                    unsigned long long* __restrict__ record) {
  __shared__ unsigned long long best[1024], sum[1024];
  __shared__ uint32_t first;
  const int t = threadIdx.x;
  const uint32_t k = st->k;
  unsigned long long b = 0, s = 0;
  for (uint32_t q = t; q < k; q += 1024) {
    const unsigned long long n = sizes[q];
    const unsigned long long key = (n << 32) | (unsigned long long)(~(q + 1));
    b = key > b ? key : b;
    s += n;
  }
  best[t] = b;
  sum[t] = s;
  if (t == 0) first = CC_NONE;
  __syncthreads();
  for (int d = 512; d > 0; d >>= 1) {
    if (t < d) {
      best[t] = best[t + d] > best[t] ? best[t + d] : best[t];
      sum[t] += sum[t + d];
    }
    __syncthreads();
  }
  const uint32_t largest = k ? ~(uint32_t)best[0] : 0;
  if (k) {                                            // the same in every thread
    uint32_t lo = 0, hi = nb - 1;                     // the last chunk with pre[c] < largest (pre[0] = 0 < largest)
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (pre[mid] < largest) lo = mid; else hi = mid - 1;
    }
    for (uint32_t e = t; e < CC_CHUNK; e += 1024) {
      const uint32_t v = lo * CC_CHUNK + e;
      if (v < total && labels[v] == (int32_t)largest) atomicMin(&first, v);
    }
  }
  __syncthreads();
  if (t != 0) return;
  record[0] = sum[0];
  record[1] = k;
  record[2] = k ? best[0] >> 32 : 0;
  record[3] = largest;
  record[4] = k ? first : 0;
  for (int q = 5; q < AFX_COMPONENTS_RECORD_SLOTS; ++q) record[q] = 0;
}

__global__ void __launch_bounds__(CC_BLOCK) k_cc_filter(const int32_t* __restrict__ labels, const uint32_t* __restrict__ sizes,
                                                        const unsigned long long* __restrict__ record, uint32_t total, int largest_only,
                                                        uint32_t min_size, uint8_t* __restrict__ out) {
  const uint32_t v = blockIdx.x * CC_BLOCK + threadIdx.x;
  if (v >= total) return;
  const int32_t l = labels[v];
  bool keep = l > 0 && sizes[l - 1] >= min_size;
  if (keep && largest_only) keep = (unsigned long long)l == record[3];
  out[v] = keep ? 1 : 0;
}

struct CcBufs { uint32_t* parent; uint32_t* sizes; uint32_t* count; CcState* st; };
CcBufs carve_components(afx::Carve& c, int32_t n0, int32_t n1, int32_t n2) {
  const size_t n = (size_t)n0 * n1 * n2;
  CcBufs b;
  b.parent = c.take<uint32_t>(n * sizeof(uint32_t));
  b.sizes = c.take<uint32_t>(n * sizeof(uint32_t));
  b.count = c.take<uint32_t>((n + CC_CHUNK - 1) / CC_CHUNK * sizeof(uint32_t));
  b.st = c.take<CcState>(256);
  return b;
}

// ---- 3-D thinning to medial curves (afx_skeletonize_3d): 8-subfield parallel thinning after Bertrand & Aktouf (1995) with Malandain &
// Bertrand's (1992) (26, 6)-simple points; the definition stands in include/afx.h.  Two voxels of one subfield are never 26-neighbours, so
// a subfield launch reads no voxel that the same launch writes, and deleting its voxels together equals deleting them one by one: the
// result is a pure function of the input.  Per pass: mark (the border voxels, as index lists per subfield), 8 subfield launches, advance.
//
// A 3 x 3 x 3 neighbourhood is a 27-bit word, bit (d0 + 1) * 9 + (d1 + 1) * 3 + (d2 + 1); the words below are sets of positions.
constexpr uint32_t sk_where(int axis, int value) {    // the positions whose coordinate (0, 1, 2) along `axis` is `value`
  uint32_t m = 0;
  for (int b = 0; b < 27; ++b) {
    const int c[3] = {b / 9, b / 3 % 3, b % 3};
    if (c[axis] == value) m |= 1u << b;
  }
  return m;
}
constexpr uint32_t sk_offsets(int lo, int hi) {       // the positions with lo..hi non-zero offsets
  uint32_t m = 0;
  for (int b = 0; b < 27; ++b) {
    const int k = (b / 9 != 1) + (b / 3 % 3 != 1) + (b % 3 != 1);
    if (k >= lo && k <= hi) m |= 1u << b;
  }
  return m;
}
constexpr uint32_t SK_N26 = sk_offsets(1, 3), SK_N18 = sk_offsets(1, 2), SK_N6 = sk_offsets(1, 1);
constexpr uint32_t SK_LO0 = sk_where(0, 0), SK_HI0 = sk_where(0, 2), SK_LO1 = sk_where(1, 0), SK_HI1 = sk_where(1, 2),
                   SK_LO2 = sk_where(2, 0), SK_HI2 = sk_where(2, 2);
static_assert(SK_N26 == 0x7ffdfffu && SK_N6 == ((1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22)), "bit layout");
static_assert(__builtin_popcount(SK_N18) == 18 && SK_LO0 == 0x1ffu && SK_HI0 == 0x1ffu << 18 && SK_LO2 == 0x1249249u, "bit layout");

// One step along an axis in both directions: a position's bit moves to the positions next to it along that axis (stride 9, 3, 1); the
// masks keep a bit from leaving its row.  The adjacency of all 27 positions at once - the word form of a per-position adjacency table.
__host__ __device__ inline uint32_t sk_step0(uint32_t x) { return ((x & ~SK_HI0) << 9) | (x >> 9); }
__host__ __device__ inline uint32_t sk_step1(uint32_t x) { return ((x & ~SK_HI1) << 3) | ((x & ~SK_LO1) >> 3); }
__host__ __device__ inline uint32_t sk_step2(uint32_t x) { return ((x & ~SK_HI2) << 1) | ((x & ~SK_LO2) >> 1); }

// The positions of `in` that `seed` reaches: a flood fill on the word, grown until it stops changing (at most 26 rounds; all in registers).
// C26: through the 26 neighbours (a step along each axis in turn is the 3 x 3 x 3 box); else through the 6 face neighbours.
template <bool C26>
__host__ __device__ inline uint32_t sk_fill(uint32_t seed, uint32_t in) {
  for (;;) {
    uint32_t g = seed;
    if (C26) {
      g |= sk_step2(g);
      g |= sk_step1(g);
      g |= sk_step0(g);
    } else {
      g |= sk_step0(seed) | sk_step1(seed) | sk_step2(seed);
    }
    g &= in;
    if (g == seed) return seed;
    seed = g;
  }
}

// (26, 6)-simple (Malandain & Bertrand): the foreground of the 26-neighbourhood is exactly one 26-component, and the background of the
// 18-neighbourhood has exactly one 6-component (joined inside the 18-neighbourhood) that touches the centre by a face.  Bit 13, the
// centre, and the bits from 27 up are ignored.  The one predicate of the device kernels and of afx_simple_point_26.
__host__ __device__ inline bool sk_simple(uint32_t nbr) {
  const uint32_t f = nbr & SK_N26;
  if (f == 0 || sk_fill<true>(f & (0u - f), f) != f) return false;
  const uint32_t bg = ~nbr & SK_N18, faces = bg & SK_N6;
  if (faces == 0) return false;
  return (faces & ~sk_fill<false>(faces & (0u - faces), bg)) == 0;
}

// Step 2 of a pass for a border voxel: it goes when it is not a curve end point (exactly one foreground 26-neighbour) and is simple.
__host__ __device__ inline bool sk_deletable(uint32_t nbr) { return __builtin_popcount(nbr & SK_N26) != 1 && sk_simple(nbr); }

constexpr int SK_BLOCK = 256;
constexpr int SK_CHUNK = 2048;                        // consecutive voxels per workgroup of the init and mark launches
constexpr int SK_ITERS = SK_CHUNK / SK_BLOCK;
constexpr unsigned SK_MAX_GRID = 1024;                // workgroups of a subfield launch; they stride over the list
enum { SK_PASSES = 0, SK_DELETED = 1, SK_CONVERGED = 2, SK_REMAINING = 3, SK_DELETED_LAST = 4, SK_INPUT = 5 };      // the record's slots

struct SkState { uint32_t count[8]; uint32_t deleted; uint32_t input; };      // 256 bytes of the workspace: list lengths, counters

__global__ void k_sk_reset(SkState* st, unsigned long long* record) {
  for (int s = 0; s < 8; ++s) st->count[s] = 0;
  st->deleted = st->input = 0;
  for (int q = 0; q < AFX_SKELETON_RECORD_SLOTS; ++q) record[q] = 0;
}

// skel = (fg != 0) as 0 / 1 (skel may be fg: every thread reads and writes its own voxels), the foreground counted once per wave
__global__ void __launch_bounds__(SK_BLOCK) k_sk_init(const uint8_t* fg, uint32_t total, uint8_t* skel, SkState* st) {
  uint32_t n = 0;                                     // of this wave (the same in every lane)
#pragma unroll
  for (int i = 0; i < SK_ITERS; ++i) {
    const uint32_t v = blockIdx.x * SK_CHUNK + i * SK_BLOCK + threadIdx.x;
    const bool on = v < total && fg[v] != 0;
    if (v < total) skel[v] = on ? 1 : 0;
    n += (uint32_t)__popcll(__ballot(on));
  }
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&st->input, n);
}

// Mark: B, the foreground voxels with a background face neighbour (beyond the grid is background), appended to the list of their
// subfield (i & 1) * 4 + (j & 1) * 2 + (k & 1): list[s * cap ..], cap = ceil(n0 / 2) ceil(n1 / 2) ceil(n2 / 2) >= the voxels of any
// subfield.  A wave reserves its places with one integer add per subfield it holds; the order inside a list is left to the hardware and
// does not matter, since a subfield's voxels are decided independently of each other.
__global__ void __launch_bounds__(SK_BLOCK) k_sk_mark(const uint8_t* __restrict__ skel, int n0, int n1, int n2, uint32_t cap,
                                                      const unsigned long long* __restrict__ record, SkState* st, uint32_t* __restrict__ list) {
  if (record[SK_CONVERGED]) return;
  const int s0 = n1 * n2, lane = threadIdx.x & 63;
  const uint32_t total = (uint32_t)n0 * (uint32_t)s0;
#pragma unroll 1
  for (int it = 0; it < SK_ITERS; ++it) {
    const uint32_t v = blockIdx.x * SK_CHUNK + it * SK_BLOCK + threadIdx.x;
    bool is_border = false;
    uint32_t sub = 0;
    if (v < total && skel[v]) {
      const int i = (int)(v / (uint32_t)s0), r = (int)(v - (uint32_t)i * (uint32_t)s0), j = r / n2, k = r - j * n2;
      is_border = i == 0 || i == n0 - 1 || j == 0 || j == n1 - 1 || k == 0 || k == n2 - 1;      // checked first: the loads below stay inside
      if (!is_border) is_border = !skel[v - s0] || !skel[v + s0] || !skel[v - n2] || !skel[v + n2] || !skel[v - 1] || !skel[v + 1];
      sub = (uint32_t)((i & 1) * 4 + (j & 1) * 2 + (k & 1));
    }
    unsigned long long todo = __ballot(is_border);    // every pass clears at least its first lane's bit
    while (todo) {
      const int first = __builtin_ctzll(todo);
      const uint32_t sx = __shfl(sub, first);
      const unsigned long long m = __ballot(is_border && sub == sx);
      uint32_t base = 0;
      if (lane == first) base = atomicAdd(&st->count[sx], (uint32_t)__popcll(m));
      base = __shfl(base, first);
      if (is_border && sub == sx) list[(size_t)sx * cap + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = v;
      todo &= ~m;
    }
  }
}

// Subfield s: every listed voxel gathers its 26 neighbours from the byte mask (beyond the grid: background) and is cleared, with a plain
// store, when the rule says so.  Its neighbours all lie in other subfields, so nothing read here is written by this launch.  (The gather
// is 26 byte loads per border voxel, some 10^4 voxels of a vessel mask, served by L2; an LDS tile with halo would stage mostly voxels no
// candidate needs.  Not measured against one.)
__global__ void __launch_bounds__(SK_BLOCK) k_sk_subfield(uint8_t* skel, int n0, int n1, int n2, uint32_t cap, int s,
                                                          const unsigned long long* __restrict__ record, SkState* st,
                                                          const uint32_t* __restrict__ list) {
  if (record[SK_CONVERGED]) return;
  const uint32_t n = st->count[s];                    // <= cap
  const int s0 = n1 * n2;
  uint32_t gone = 0;
  for (uint32_t q = blockIdx.x * SK_BLOCK + threadIdx.x; q < n; q += gridDim.x * SK_BLOCK) {
    const uint32_t v = list[(size_t)s * cap + q];
    const int i = (int)(v / (uint32_t)s0), r = (int)(v - (uint32_t)i * (uint32_t)s0), j = r / n2, k = r - j * n2;
    uint32_t nbr = 0;
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
        for (int dk = -1; dk <= 1; ++dk) {
          if (di == 0 && dj == 0 && dk == 0) continue;
          const bool inside = i + di >= 0 && i + di < n0 && j + dj >= 0 && j + dj < n1 && k + dk >= 0 && k + dk < n2;
          if (inside && skel[(int)v + di * s0 + dj * n2 + dk]) nbr |= 1u << ((di + 1) * 9 + (dj + 1) * 3 + (dk + 1));
        }
    if (sk_deletable(nbr)) {
      skel[v] = 0;
      ++gone;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) gone += __shfl_xor(gone, d);
  if ((threadIdx.x & 63) == 0 && gone) atomicAdd(&st->deleted, gone);
}

// One lane: the pass is over.  Rolls the record and empties the lists for the next pass; a pass that deleted nothing sets converged,
// after which every launch of a later pass returns at once and the record stands.
__global__ void k_sk_advance(SkState* st, unsigned long long* record) {
  if (!record[SK_CONVERGED]) {
    const unsigned long long d = st->deleted;
    record[SK_PASSES] += 1;
    record[SK_DELETED] += d;
    record[SK_DELETED_LAST] = d;
    record[SK_INPUT] = st->input;
    record[SK_REMAINING] = st->input - record[SK_DELETED];
    if (d == 0) record[SK_CONVERGED] = 1;
  }
  st->deleted = 0;
  for (int s = 0; s < 8; ++s) st->count[s] = 0;
}

uint32_t sk_cap(int32_t n0, int32_t n1, int32_t n2) { return (uint32_t)((n0 + 1) / 2) * (uint32_t)((n1 + 1) / 2) * (uint32_t)((n2 + 1) / 2); }

struct SkBufs { uint32_t* list; SkState* st; };
SkBufs carve_skeleton(afx::Carve& c, int32_t n0, int32_t n1, int32_t n2) {
  SkBufs b;
  b.list = c.take<uint32_t>((size_t)8 * sk_cap(n0, n1, n2) * sizeof(uint32_t));
  b.st = c.take<SkState>(256);
  return b;
}

}  // namespace

extern "C" int afx_simple_point_26(uint32_t nbr) { return sk_simple(nbr) ? 1 : 0; }

extern "C" size_t afx_skeletonize_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2) {
  if (!afx::volume_shape_ok(n0, n1, n2)) return 0;
  afx::Carve c;
  carve_skeleton(c, n0, n1, n2);
  return c.end;
}

extern "C" int afx_skeletonize_3d(const uint8_t* fg, int32_t n0, int32_t n1, int32_t n2, int32_t max_passes, int32_t sync_every, uint8_t* skel,
                                  void* record, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "afx_skeletonize_3d";
  if (!fg || !skel || !record) return afx::set_error(AFX_E_INVALID, who, "null volume, skeleton or record");
  if (!afx::volume_shape_ok(n0, n1, n2)) return afx::set_error(AFX_E_INVALID, who, "need a volume of 1..1024 voxels along each axis");
  if (max_passes < 1) return afx::set_error(AFX_E_INVALID, who, "max_passes must be at least 1");
  if (sync_every < 0) return afx::set_error(AFX_E_INVALID, who, "sync_every must be 0 (no read-back) or the passes between two read-backs");
  const size_t need = afx_skeletonize_3d_workspace_bytes(n0, n1, n2);
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(fg, "the volume", who)) return rc;
  if (int rc = afx::check_device(skel, "the skeleton", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  afx::Carve c;
  c.base = (uintptr_t)workspace;
  const SkBufs b = carve_skeleton(c, n0, n1, n2);
  unsigned long long* rec = (unsigned long long*)record;
  const uint32_t total = (uint32_t)n0 * (uint32_t)n1 * (uint32_t)n2, cap = sk_cap(n0, n1, n2);      // total <= 2^30
  const unsigned chunks = (total + SK_CHUNK - 1) / SK_CHUNK, grid = std::min((cap + SK_BLOCK - 1) / SK_BLOCK, SK_MAX_GRID);
  hipLaunchKernelGGL(k_sk_reset, dim3(1), dim3(1), 0, st, b.st, rec);
  hipLaunchKernelGGL(k_sk_init, dim3(chunks), dim3(SK_BLOCK), 0, st, fg, total, skel, b.st);
  for (int32_t p = 1; p <= max_passes; ++p) {
    hipLaunchKernelGGL(k_sk_mark, dim3(chunks), dim3(SK_BLOCK), 0, st, (const uint8_t*)skel, (int)n0, (int)n1, (int)n2, cap,
                       (const unsigned long long*)rec, b.st, b.list);
    for (int s = 0; s < 8; ++s)
      hipLaunchKernelGGL(k_sk_subfield, dim3(grid), dim3(SK_BLOCK), 0, st, skel, (int)n0, (int)n1, (int)n2, cap, s,
                         (const unsigned long long*)rec, b.st, (const uint32_t*)b.list);
    hipLaunchKernelGGL(k_sk_advance, dim3(1), dim3(1), 0, st, b.st, rec);
    if (sync_every > 0 && (p % sync_every == 0 || p == max_passes)) {
      if (int rc = afx::launched(who)) return rc;
      unsigned long long converged = 0;
      hipError_t e = hipMemcpyAsync(&converged, rec + SK_CONVERGED, sizeof converged, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) return afx::set_error(AFX_E_HIP, who, hipGetErrorString(e));
      if (converged) return AFX_OK;
    }
  }
  if (sync_every > 0)                                 // not a failure: the mask after max_passes passes and a record that says converged = 0
    return afx::set_error(AFX_OK, who, "stopped at max_passes before a pass deleted nothing: the record's converged slot is 0");
  return afx::launched(who);
}

extern "C" size_t afx_label_components_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2) {
  if (!afx::volume_shape_ok(n0, n1, n2)) return 0;
  afx::Carve c;
  carve_components(c, n0, n1, n2);
  return c.end;
}

extern "C" int afx_label_components_3d(const uint8_t* fg, int32_t n0, int32_t n1, int32_t n2, int32_t connectivity, int32_t* labels,
                                       uint32_t* sizes, void* record, void* workspace, size_t workspace_bytes, size_t* workspace_needed,
                                       void* stream) {
  const char* who = "afx_label_components_3d";
  if (!fg || !labels || !record) return afx::set_error(AFX_E_INVALID, who, "null volume, labels or record");
  if (!afx::volume_shape_ok(n0, n1, n2)) return afx::set_error(AFX_E_INVALID, who, "need a volume of 1..1024 voxels along each axis");
  if (connectivity < 1 || connectivity > 3) return afx::set_error(AFX_E_INVALID, who, "connectivity must be 1, 2 or 3 (6, 18 or 26 neighbours)");
  const size_t need = afx_label_components_3d_workspace_bytes(n0, n1, n2);
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(fg, "the volume", who)) return rc;
  if (int rc = afx::check_device(labels, "labels", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  afx::Carve c;
  c.base = (uintptr_t)workspace;
  const CcBufs b = carve_components(c, n0, n1, n2);
  uint32_t* sz = sizes ? sizes : b.sizes;
  const uint32_t total = (uint32_t)n0 * (uint32_t)n1 * (uint32_t)n2;                 // <= 2^30
  const unsigned chunks = (total + CC_CHUNK - 1) / CC_CHUNK, blocks = (total + CC_BLOCK - 1) / CC_BLOCK;
  hipLaunchKernelGGL(k_cc_init, dim3(chunks), dim3(CC_BLOCK), 0, st, fg, total, b.parent, sz);
  if (connectivity == 1) hipLaunchKernelGGL(k_cc_merge<1>, dim3(blocks), dim3(CC_BLOCK), 0, st, fg, (int)n0, (int)n1, (int)n2, b.parent);
  else if (connectivity == 2) hipLaunchKernelGGL(k_cc_merge<2>, dim3(blocks), dim3(CC_BLOCK), 0, st, fg, (int)n0, (int)n1, (int)n2, b.parent);
  else hipLaunchKernelGGL(k_cc_merge<3>, dim3(blocks), dim3(CC_BLOCK), 0, st, fg, (int)n0, (int)n1, (int)n2, b.parent);
  hipLaunchKernelGGL(k_cc_flatten, dim3(chunks), dim3(CC_BLOCK), 0, st, (const uint32_t*)b.parent, total, labels, b.count);
  hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(1024), 0, st, b.count, (uint32_t)chunks, b.st);
  hipLaunchKernelGGL(k_cc_rank, dim3(chunks), dim3(CC_BLOCK), 0, st, (const int32_t*)labels, total, (const uint32_t*)b.count, b.parent);
  hipLaunchKernelGGL(k_cc_relabel, dim3(chunks), dim3(CC_BLOCK), 0, st, labels, total, (const uint32_t*)b.parent, sz);
  hipLaunchKernelGGL(k_cc_finish, dim3(1), dim3(1024), 0, st, (const CcState*)b.st, (const uint32_t*)sz, (const int32_t*)labels, total,
                     (const uint32_t*)b.count, (uint32_t)chunks, (unsigned long long*)record);
  return afx::launched(who);
}

extern "C" int afx_filter_components_3d(const int32_t* labels, const uint32_t* sizes, const void* record, int32_t n0, int32_t n1, int32_t n2,
                                        int32_t largest_only, uint32_t min_size, uint8_t* out, void* stream) {
  const char* who = "afx_filter_components_3d";
  if (!labels || !sizes || !record || !out) return afx::set_error(AFX_E_INVALID, who, "null labels, sizes, record or output");
  if (!afx::volume_shape_ok(n0, n1, n2)) return afx::set_error(AFX_E_INVALID, who, "need a volume of 1..1024 voxels along each axis");
  if (min_size == 0) return afx::set_error(AFX_E_INVALID, who, "min_size must be at least 1");
  if (int rc = afx::check_device(labels, "labels", who)) return rc;
  if (int rc = afx::check_device(out, "the output mask", who)) return rc;
  const uint32_t total = (uint32_t)n0 * (uint32_t)n1 * (uint32_t)n2;
  hipLaunchKernelGGL(k_cc_filter, dim3((total + CC_BLOCK - 1) / CC_BLOCK), dim3(CC_BLOCK), 0, (hipStream_t)stream, labels, sizes,
                     (const unsigned long long*)record, total, (int)(largest_only != 0), min_size, out);
  return afx::launched(who);
}

extern "C" size_t afx_distance_transform_edt_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2) {
  if (!afx::volume_shape_ok(n0, n1, n2)) return 0;
  afx::Carve c;
  c.take<uint16_t>((size_t)n0 * n1 * n2 * sizeof(uint16_t));
  return c.end;
}

extern "C" int afx_distance_transform_edt_3d(const uint8_t* fg, int32_t n0, int32_t n1, int32_t n2, uint32_t* d2, double* dist, void* workspace,
                                             size_t workspace_bytes, size_t* workspace_needed, void* stream) {
  const char* who = "afx_distance_transform_edt_3d";
  if (!fg || !d2) return afx::set_error(AFX_E_INVALID, who, "null volume or squared-distance output");
  if (!afx::volume_shape_ok(n0, n1, n2)) return afx::set_error(AFX_E_INVALID, who, "need a volume of 1..1024 voxels along each axis");
  const size_t need = afx_distance_transform_edt_3d_workspace_bytes(n0, n1, n2);
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(fg, "the volume", who)) return rc;
  launch_edt3(fg, n0, n1, n2, (uint16_t*)workspace, d2, dist, (hipStream_t)stream);
  return afx::launched(who);
}

extern "C" size_t afx_surface_metrics_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2) {
  if (!afx::volume_shape_ok(n0, n1, n2)) return 0;
  afx::Carve c;
  carve_surface(c, n0, n1, n2);
  return c.end;
}

extern "C" int afx_surface_metrics_3d(const float* pred, const float* gt, int32_t n0, int32_t n1, int32_t n2, float thr_pred, float thr_gt,
                                      double q, void* record, void* workspace, size_t workspace_bytes, size_t* workspace_needed,
                                      void* stream) {
  const char* who = "afx_surface_metrics_3d";
  if (!pred || !gt || !record) return afx::set_error(AFX_E_INVALID, who, "null volume or record");
  if (!afx::volume_shape_ok(n0, n1, n2)) return afx::set_error(AFX_E_INVALID, who, "need volumes of 1..1024 voxels along each axis");
  if (thr_pred != thr_pred || thr_gt != thr_gt) return afx::set_error(AFX_E_INVALID, who, "a threshold is NaN");
  if (!(q >= 0.0 && q <= 100.0)) return afx::set_error(AFX_E_INVALID, who, "the percentile q must lie in [0, 100]");
  const size_t need = afx_surface_metrics_3d_workspace_bytes(n0, n1, n2);
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(pred, "pred", who)) return rc;
  if (int rc = afx::check_device(gt, "gt", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  afx::Carve c;
  c.base = (uintptr_t)workspace;
  const SurfaceBufs b = carve_surface(c, n0, n1, n2);
  const int64_t total = (int64_t)n0 * n1 * n2;
  const unsigned blocks = (unsigned)std::min<int64_t>((total + 2047) / 2048, SM_MAX_PART);      // ~8 voxels per thread, then a stride
  hipLaunchKernelGGL(k_sm_init, dim3(1), dim3(256), 0, st, b.st, b.hist);
  hipLaunchKernelGGL(k_sm_masks, dim3(blocks), dim3(256), 0, st, pred, gt, (int)n0, (int)n1, (int)n2, thr_pred, thr_gt, b.na, b.nb, b.st);
  launch_edt3(b.na, n0, n1, n2, b.g16, b.d2a, nullptr, st);                  // the distance to S(A)
  launch_edt3(b.nb, n0, n1, n2, b.g16, b.d2b, nullptr, st);                  // the distance to S(B)
  hipLaunchKernelGGL(k_sm_gather<1>, dim3(blocks), dim3(256), 0, st, (const uint8_t*)b.na, (const uint8_t*)b.nb, (const uint32_t*)b.d2a,
                     (const uint32_t*)b.d2b, total, b.st, b.hist, b.partial);
  hipLaunchKernelGGL(k_sm_scan, dim3(1), dim3(256), 0, st, b.st, (const uint32_t*)b.hist, q / 100.0);
  hipLaunchKernelGGL(k_sm_gather<2>, dim3(blocks), dim3(256), 0, st, (const uint8_t*)b.na, (const uint8_t*)b.nb, (const uint32_t*)b.d2a,
                     (const uint32_t*)b.d2b, total, b.st, b.hist + SM_BINS, (double*)nullptr);
  hipLaunchKernelGGL(k_sm_finish, dim3(1), dim3(256), 0, st, (const SmState*)b.st, (const uint32_t*)(b.hist + SM_BINS), (const double*)b.partial,
                     (int)blocks, (unsigned long long*)record);
  return afx::launched(who);
}

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
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
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
