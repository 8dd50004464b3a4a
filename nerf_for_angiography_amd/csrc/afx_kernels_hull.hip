// afx_kernels_hull.hip - the visual hull of the training views (afx_visual_hull) and the byte mask that carves an occupancy grid with it
// (afx_grid_apply_mask); both definitions stand in include/afx.h.  afx_visual_hull: one lane per lattice point, the innermost axis
// fastest, so that neighbouring lanes project to neighbouring pixels and the gathers from the distance images stay in a few cache lines.
// Every lane loops over all the views and keeps its two counts in registers; each is stored once.  The view records (128 bytes: R, c, f)
// are read through addresses that are the same in every lane (the kernel argument plus the loop counter), which the compiler turns into
// scalar loads: no LDS, no barrier, and a view set of any size needs no staging chunks.  No atomics, nothing allocated, nothing read
// back.  NOTHING CAN HANG: no lane waits for another, and the loop runs V times, a kernel argument.  The only indexed load, D[v][iw][iu],
// is made with iu, iw clamped into the image in fp64 before they become integers.
#include "afx_internal.h"
#include "afx_geom.h"
#include <cmath>

// every fp64 product, quotient and sum below is rounded on its own (the definition is stated operation by operation)
#pragma clang fp contract(off)

namespace {

constexpr int VH_BLOCK = 256;
constexpr double VH_SQRT_HALF = 0x1.6a09e667f3bcdp-1;      // sqrt(0.5) rounded to fp64: how far rounding to a pixel centre moves a point

struct HullArgs {
  double A[12];
  double rho, m, half_w, half_h, w_last, h_last;      // W / 2, H / 2, W - 1, H - 1
  int32_t P, n1, n2, V, W, H;
};

__global__ void __launch_bounds__(VH_BLOCK) k_visual_hull(const HullArgs a, const afx::ViewRecord* __restrict__ views, const double* __restrict__ D,
                                                          uint16_t* __restrict__ seen, uint16_t* __restrict__ rejects) {
  const int64_t p64 = (int64_t)blockIdx.x * VH_BLOCK + threadIdx.x;
  if (p64 >= a.P) return;
  const int32_t p = (int32_t)p64;
  double x0, x1, x2;
  afx::affine_apply_index(a.A, p, a.n1, a.n2, x0, x1, x2);
  const size_t image = (size_t)a.W * (size_t)a.H;
  uint32_t n_seen = 0, n_rej = 0;
  for (int32_t v = 0; v < a.V; ++v) {
    const afx::ViewRecord& vw = views[v];             // the same address in every lane
    double q0, q1, q2, u, w;
    afx::view_camera(vw, x0, x1, x2, q0, q1, q2);
    const double d = -q2;
    const double near = d - a.rho;
    if (!(near > 0.0)) continue;                      // behind the source, or too close to it to bound the projection (a NaN ends here too)
    afx::view_pixel(vw, a.half_w, a.half_h, q0, q1, d, u, w);
    const double l = sqrt(q0 * q0 + q1 * q1);
    const double r = ((vw.f * a.rho) * (d + l)) / (d * near) + a.m;
    double dx = 0.0 > -u ? 0.0 : -u, dy = 0.0 > -w ? 0.0 : -w;
    const double ox = u - a.w_last, oy = w - a.h_last;
    dx = dx > ox ? dx : ox;
    dy = dy > oy ? dy : oy;
    if (!(dx <= r && dy <= r)) continue;              // not seen
    ++n_seen;
    const double delta = sqrt(dx * dx + dy * dy);
    double fu = floor(u + 0.5), fw = floor(w + 0.5);
    fu = fu < 0.0 ? 0.0 : (fu > a.w_last ? a.w_last : fu);      // clamped in fp64: the conversion below cannot overflow
    fw = fw < 0.0 ? 0.0 : (fw > a.h_last ? a.h_last : fw);
    const double dist = D[(size_t)v * image + (size_t)(int32_t)fw * (size_t)a.W + (size_t)(int32_t)fu];
    if (dist > (r + VH_SQRT_HALF) + delta) ++n_rej;
  }
  seen[p] = (uint16_t)n_seen;                         // V <= 65 535
  rejects[p] = (uint16_t)n_rej;
}

// one lane per cell; the wavefront's ballot is the two 32-cell words of its 64 cells.  Every lane of a launched wave reaches the ballot
// (cells past n vote 0 and store nothing), and a word is written by one lane of the one wave that owns it.
__global__ void __launch_bounds__(VH_BLOCK) k_grid_apply_mask(const uint8_t* __restrict__ mask, int64_t n, float* __restrict__ occs,
                                                              uint8_t* __restrict__ binary, uint32_t* __restrict__ bits) {
  const int64_t c = (int64_t)blockIdx.x * VH_BLOCK + threadIdx.x;
  bool on = false;
  if (c < n) {
    if (mask[c] == 0) {
      if (occs) occs[c] = 0.f;
      binary[c] = 0;
    } else {
      on = binary[c] != 0;
    }
  }
  const unsigned long long vote = __ballot(on);
  const int lane = threadIdx.x & 63;
  const int64_t word = (c >> 6) * 2 + lane;           // lanes 0 and 1 write the wave's two words
  if (lane < 2 && word * 32 < n) bits[word] = (uint32_t)(vote >> (32 * lane));
}

}  // namespace

extern "C" int afx_visual_hull(int32_t n0, int32_t n1, int32_t n2, const double* index_to_world, double radius, const double* views,
                               int32_t n_views, int32_t width, int32_t height, double margin_px, const double* dist, uint16_t* seen,
                               uint16_t* rejects, void* stream) {
  const char* who = "afx_visual_hull";
  if (!index_to_world) return afx::set_error(AFX_E_INVALID, who, "null index_to_world");
  if (!views) return afx::set_error(AFX_E_INVALID, who, "null views");
  if (!dist) return afx::set_error(AFX_E_INVALID, who, "null dist");
  if (!seen || !rejects) return afx::set_error(AFX_E_INVALID, who, "null seen or rejects");
  if (n_views < 1 || n_views > 65535) return afx::set_error(AFX_E_INVALID, who, "n_views must lie in 1..65535");
  if (n0 < 1 || n1 < 1 || n2 < 1) return afx::set_error(AFX_E_INVALID, who, "n0, n1, n2 must be positive");
  if (width < 1 || height < 1) return afx::set_error(AFX_E_INVALID, who, "width and height must be positive");
  if (int rc = afx::check_lattice_size(n0, n1, n2, who)) return rc;
  if (!afx::all_finite(index_to_world, 12)) return afx::set_error(AFX_E_INVALID, who, "index_to_world must be finite");
  if (!(radius >= 0.0) || !std::isfinite(radius)) return afx::set_error(AFX_E_INVALID, who, "radius must be finite and >= 0");
  if (!(margin_px >= 0.0) || !std::isfinite(margin_px)) return afx::set_error(AFX_E_INVALID, who, "margin_px must be finite and >= 0");
  if (int rc = afx::check_device(views, "views", who)) return rc;
  if (int rc = afx::check_device(dist, "dist", who)) return rc;
  if (int rc = afx::check_device(seen, "seen", who)) return rc;
  if (int rc = afx::check_device(rejects, "rejects", who)) return rc;
  HullArgs a;
  for (int i = 0; i < 12; ++i) a.A[i] = index_to_world[i];
  a.rho = radius, a.m = margin_px;
  a.half_w = (double)width / 2.0, a.half_h = (double)height / 2.0, a.w_last = (double)(width - 1), a.h_last = (double)(height - 1);
  a.P = (int32_t)((int64_t)n0 * n1 * n2), a.n1 = n1, a.n2 = n2, a.V = n_views, a.W = width, a.H = height;
  const unsigned blocks = (unsigned)(((int64_t)a.P + VH_BLOCK - 1) / VH_BLOCK);
  hipLaunchKernelGGL(k_visual_hull, dim3(blocks), dim3(VH_BLOCK), 0, (hipStream_t)stream, a, (const afx::ViewRecord*)views, dist, seen, rejects);
  return afx::launched(who);
}

extern "C" int afx_grid_apply_mask(const afx_grid_desc* grid, const uint8_t* mask, float* occs, uint8_t* binary, uint32_t* bits, void* stream) {
  const char* who = "afx_grid_apply_mask";
  if (!grid) return afx::set_error(AFX_E_INVALID, who, "null grid");
  for (int i = 0; i < 3; ++i)
    if (grid->resolution[i] < 1 || grid->resolution[i] > 2048) return afx::set_error(AFX_E_INVALID, who, "resolution must be in 1..2048");
  if (!mask || !binary || !bits) return afx::set_error(AFX_E_INVALID, who, "null mask, binary or bits");
  const int64_t n = (int64_t)grid->resolution[0] * grid->resolution[1] * grid->resolution[2];
  const unsigned blocks = (unsigned)((n + VH_BLOCK - 1) / VH_BLOCK);
  hipLaunchKernelGGL(k_grid_apply_mask, dim3(blocks), dim3(VH_BLOCK), 0, (hipStream_t)stream, mask, n, occs, binary, bits);
  return afx::launched(who);
}
