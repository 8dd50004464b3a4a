// afx_kernels_sirt.hip - the two operators of the sparse-view algebraic reconstruction (SIRT): afx_xray_project, the ray-driven line
// integrals of an fp64 volume, optionally fused to the weighted residual, and afx_xray_backproject, the voxel-driven gather of the views'
// images, optionally fused to the SIRT update.  Both definitions stand in include/afx.h, operation by operation; every fp64 operation
// here is written in that order and rounded on its own, so the device equals the NumPy restatement tests/sirt_reference.py bit for bit.
//
// Layout, and why (the results do not depend on it: a lane's arithmetic is the definition).
//   Projector: one lane per ray.  A workgroup is 256 lanes = a 16 x 16 pixel block of one view; each of its four wavefronts is an 8 x 8
//   pixel tile (lane & 7 along u, lane >> 3 along w), not a 64-pixel row.  At one depth the 64 samples of a wavefront then lie in a patch
//   about 8 x 8 voxels across instead of a line 64 long: the eight corner loads of a trilinear sample touch a few dozen 128-byte lines per
//   wavefront instead of a hundred and more, and the neighbouring tiles of the workgroup re-use them from the CU's L1.  The volume
//   (65 MB at 201^3) stays in the Infinity Cache between launches.  The view record is read through blockIdx.z: scalar loads.  A lane
//   tests every sample against the lattice with the definition's own comparison and loads nothing for a sample outside - the definition
//   lets it contribute +0.0, and acc, which starts at +0.0, is unchanged by adding +0.0 (it can never be -0.0: a sum is -0.0 only when
//   both terms are), so skipping the addition is exact.  No further clipping of the sample range is done: the test costs 18 fp64
//   operations a sample against the 8 loads and 21 operations of a sample inside, and with near / far bracketing the lattice most samples
//   are inside.  The sample body is afx::lattice_lookup (afx_geom.h) written out, with afx::affine_apply and afx::lerp for its pieces;
//   it is the one kernel that does not call the helper.  The helper forms n_a - 1 and n_a - 2 from the lattice sizes; here n_a - 1 comes
//   ready in the kernel arguments, in scalar registers.  Through the helper all six bounds sit in vector registers for the whole loop
//   (48 -> 54), which measured 2.2 % slower at 201^3 against 25 views of 512^2 (3.940 ms against 3.854 and 3.844 ms of this form; equal
//   at 128^3).
//   Backprojector: one lane per lattice point, k fastest as in k_visual_hull, so neighbouring lanes project to neighbouring pixels and
//   the four loads of the bilinear sample stay in a few lines; the loop over the views runs in order and reads the records through
//   wave-uniform addresses (scalar loads).  The images (52 MB at 25 x 512^2) stay in the Infinity Cache.  A lane reads and writes its
//   own voxel only, so the fused update is in place.
// No atomics, no LDS, no workspace, nothing read back: both calls can be captured in a graph.  NOTHING CAN HANG: no lane waits for
// another, and the loops run S and V times, kernel arguments.  Every indexed load is made with indices that the definition's own
// comparisons have placed inside the array (0 <= g <= n - 1, then min(floor(g), n - 2): a NaN fails the comparison and loads nothing).
#include "afx_internal.h"
#include "afx_geom.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int XR_BLOCK = 256;

struct ProjectArgs {
  double B[12];
  double half_w, half_h, near, dt, last0, last1, last2;         // W / 2, H / 2, (far - near) / S, n_a - 1
  int32_t n0, n1, n2, W, H, S;
};

__global__ void __launch_bounds__(XR_BLOCK) k_xray_project(const ProjectArgs a, const afx::ViewRecord* __restrict__ views, const double* __restrict__ vol,
                                                           const double* __restrict__ target, const double* __restrict__ weight,
                                                           double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t iu = (int32_t)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int32_t iw = (int32_t)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (iu >= a.W || iw >= a.H) return;
  const afx::ViewRecord& vw = views[blockIdx.z];      // the same address in every lane
  const double ca = ((double)iu - a.half_w) / vw.f;
  const double cb = -(((double)iw - a.half_h) / vw.f);
  const double d0 = (vw.R[0] * ca + vw.R[1] * cb) - vw.R[2];
  const double d1 = (vw.R[3] * ca + vw.R[4] * cb) - vw.R[5];
  const double d2 = (vw.R[6] * ca + vw.R[7] * cb) - vw.R[8];
  const double len = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
  const size_t s1 = (size_t)a.n2, s0 = (size_t)a.n1 * (size_t)a.n2;
  const double top0 = (double)(a.n0 - 2), top1 = (double)(a.n1 - 2), top2 = (double)(a.n2 - 2);
  double acc = 0.0;
  for (int32_t s = 0; s < a.S; ++s) {
    const double t = a.near + ((double)s + 0.5) * a.dt;
    double g0, g1, g2;
    afx::affine_apply(a.B, vw.c[0] + t * d0, vw.c[1] + t * d1, vw.c[2] + t * d2, g0, g1, g2);
    if (!(g0 >= 0.0 && g0 <= a.last0 && g1 >= 0.0 && g1 <= a.last1 && g2 >= 0.0 && g2 <= a.last2)) continue;      // contributes +0.0
    double f0 = floor(g0), f1 = floor(g1), f2 = floor(g2);
    f0 = f0 < top0 ? f0 : top0, f1 = f1 < top1 ? f1 : top1, f2 = f2 < top2 ? f2 : top2;      // in 0 .. n_a - 2
    const double p0 = g0 - f0, p1 = g1 - f1, p2 = g2 - f2;
    const double* b = vol + ((size_t)(int32_t)f0 * s0 + (size_t)(int32_t)f1 * s1 + (size_t)(int32_t)f2);
    const double c00 = afx::lerp(b[0], b[1], p2), c01 = afx::lerp(b[s1], b[s1 + 1], p2);
    const double c10 = afx::lerp(b[s0], b[s0 + 1], p2), c11 = afx::lerp(b[s0 + s1], b[s0 + s1 + 1], p2);
    acc += afx::lerp(afx::lerp(c00, c01, p1), afx::lerp(c10, c11, p1), p0);
  }
  const double y = (acc * a.dt) * len;
  const size_t at = ((size_t)blockIdx.z * (size_t)a.H + (size_t)iw) * (size_t)a.W + (size_t)iu;
  out[at] = target ? weight[at] * (target[at] - y) : y;
}

struct BackprojectArgs {
  double A[12];
  double half_w, half_h, w_last, h_last, u_top, w_top, relax;   // W / 2, H / 2, W - 1, H - 1, W - 2, H - 2
  int32_t P, n1, n2, V, W, H, nonneg;
};

__global__ void __launch_bounds__(XR_BLOCK) k_xray_backproject(const BackprojectArgs a, const afx::ViewRecord* __restrict__ views,
                                                               const double* __restrict__ img, double* __restrict__ acc_out,
                                                               uint16_t* __restrict__ seen, double* __restrict__ x_inout,
                                                               const uint8_t* __restrict__ mask) {
  const int64_t p64 = (int64_t)blockIdx.x * XR_BLOCK + threadIdx.x;
  if (p64 >= a.P) return;
  const int32_t p = (int32_t)p64;
  double x0, x1, x2;
  afx::affine_apply_index(a.A, p, a.n1, a.n2, x0, x1, x2);
  const size_t row = (size_t)a.W, image = (size_t)a.W * (size_t)a.H;
  double acc = 0.0;
  uint32_t cnt = 0;
  for (int32_t v = 0; v < a.V; ++v) {
    const afx::ViewRecord& vw = views[v];               // the same address in every lane
    double q0, q1, q2, u, w;
    afx::view_camera(vw, x0, x1, x2, q0, q1, q2);
    const double d = -q2;
    if (!(d > 0.0)) continue;                           // behind the source (a NaN ends here too)
    afx::view_pixel(vw, a.half_w, a.half_h, q0, q1, d, u, w);
    if (!(u >= 0.0 && u <= a.w_last && w >= 0.0 && w <= a.h_last)) continue;      // not seen
    double fu = floor(u), fw = floor(w);
    fu = fu < a.u_top ? fu : a.u_top, fw = fw < a.w_top ? fw : a.w_top;           // in 0 .. W - 2, 0 .. H - 2
    const double pu = u - fu, pw = w - fw;
    const double* b = img + ((size_t)v * image + (size_t)(int32_t)fw * row + (size_t)(int32_t)fu);
    const double top = afx::lerp(b[0], b[1], pu), bot = afx::lerp(b[row], b[row + 1], pu);
    acc += afx::lerp(top, bot, pw);
    ++cnt;
  }
  if (acc_out) acc_out[p] = acc;
  if (seen) seen[p] = (uint16_t)cnt;                    // V <= 65 535
  if (x_inout) {
    const double upd = cnt > 0 ? acc / (double)cnt : 0.0;
    double y = x_inout[p] + a.relax * upd;
    if (a.nonneg) y = y > 0.0 ? y : 0.0;
    if (mask && mask[p] == 0) y = 0.0;
    x_inout[p] = y;
  }
}

int xr_check_device(const void* p, const char* what, const char* who) { return afx::check_device_memory(p, what, who); }

// the checks the two entry points share; 0 when they pass
int xr_check_shapes(const char* who, int32_t n0, int32_t n1, int32_t n2, int32_t n_views, int32_t width, int32_t height) {
  if (n_views < 1 || n_views > 65535) return afx::set_error(AFX_E_INVALID, who, "n_views must lie in 1..65535");
  if (n0 < 2 || n1 < 2 || n2 < 2) return afx::set_error(AFX_E_INVALID, who, "n0, n1, n2 must be at least 2");
  if (int rc = afx::check_lattice_size(n0, n1, n2, who)) return rc;
  if (width < 2 || height < 2) return afx::set_error(AFX_E_INVALID, who, "width and height must be at least 2");
  return AFX_OK;
}

}  // namespace

extern "C" int afx_xray_project(const double* volume, int32_t n0, int32_t n1, int32_t n2, const double* world_to_index, const double* views,
                                int32_t n_views, int32_t width, int32_t height, double near, double far, int32_t n_samples,
                                const double* target, const double* weight, double* out, void* stream) {
  const char* who = "afx_xray_project";
  if (!volume) return afx::set_error(AFX_E_INVALID, who, "null volume");
  if (!world_to_index) return afx::set_error(AFX_E_INVALID, who, "null world_to_index");
  if (!views) return afx::set_error(AFX_E_INVALID, who, "null views");
  if (!out) return afx::set_error(AFX_E_INVALID, who, "null out");
  if (int rc = xr_check_shapes(who, n0, n1, n2, n_views, width, height)) return rc;
  if (n_samples < 1) return afx::set_error(AFX_E_INVALID, who, "n_samples must be positive");
  if (!afx::all_finite(world_to_index, 12)) return afx::set_error(AFX_E_INVALID, who, "world_to_index must be finite");
  if (!std::isfinite(near) || !std::isfinite(far)) return afx::set_error(AFX_E_INVALID, who, "near and far must be finite");
  if (!(far > near)) return afx::set_error(AFX_E_INVALID, who, "far must be greater than near");
  if ((target != nullptr) != (weight != nullptr)) return afx::set_error(AFX_E_INVALID, who, "target and weight are given together or not at all");
  if (int rc = xr_check_device(volume, "volume", who)) return rc;
  if (int rc = xr_check_device(views, "views", who)) return rc;
  if (int rc = xr_check_device(out, "out", who)) return rc;
  if (target) {
    if (int rc = xr_check_device(target, "target", who)) return rc;
    if (int rc = xr_check_device(weight, "weight", who)) return rc;
  }
  ProjectArgs a;
  for (int i = 0; i < 12; ++i) a.B[i] = world_to_index[i];
  a.half_w = (double)width / 2.0, a.half_h = (double)height / 2.0, a.near = near, a.dt = (far - near) / (double)n_samples;
  a.last0 = (double)(n0 - 1), a.last1 = (double)(n1 - 1), a.last2 = (double)(n2 - 1);
  a.n0 = n0, a.n1 = n1, a.n2 = n2, a.W = width, a.H = height, a.S = n_samples;
  const dim3 grid((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16), (unsigned)n_views);
  if (grid.y > 65535u) return afx::set_error(AFX_E_INVALID, who, "height must stay below 2^20");
  hipLaunchKernelGGL(k_xray_project, grid, dim3(XR_BLOCK), 0, (hipStream_t)stream, a, (const afx::ViewRecord*)views, volume, target, weight, out);
  return afx::launched(who);
}

extern "C" int afx_xray_backproject(const double* images, const double* views, int32_t n_views, int32_t width, int32_t height, int32_t n0,
                                    int32_t n1, int32_t n2, const double* index_to_world, double* acc, uint16_t* seen, double* x_inout,
                                    double relax, int32_t nonneg, const uint8_t* mask, void* stream) {
  const char* who = "afx_xray_backproject";
  if (!images) return afx::set_error(AFX_E_INVALID, who, "null images");
  if (!views) return afx::set_error(AFX_E_INVALID, who, "null views");
  if (!index_to_world) return afx::set_error(AFX_E_INVALID, who, "null index_to_world");
  if (!acc && !seen && !x_inout) return afx::set_error(AFX_E_INVALID, who, "no output: acc, seen and x_inout are all null");
  if (mask && !x_inout) return afx::set_error(AFX_E_INVALID, who, "mask belongs to the fused update: null x_inout");
  if (int rc = xr_check_shapes(who, n0, n1, n2, n_views, width, height)) return rc;
  if (!afx::all_finite(index_to_world, 12)) return afx::set_error(AFX_E_INVALID, who, "index_to_world must be finite");
  if (!std::isfinite(relax)) return afx::set_error(AFX_E_INVALID, who, "relax must be finite");
  if (int rc = xr_check_device(images, "images", who)) return rc;
  if (int rc = xr_check_device(views, "views", who)) return rc;
  if (acc)
    if (int rc = xr_check_device(acc, "acc", who)) return rc;
  if (seen)
    if (int rc = xr_check_device(seen, "seen", who)) return rc;
  if (x_inout)
    if (int rc = xr_check_device(x_inout, "x_inout", who)) return rc;
  if (mask)
    if (int rc = xr_check_device(mask, "mask", who)) return rc;
  BackprojectArgs a;
  for (int i = 0; i < 12; ++i) a.A[i] = index_to_world[i];
  a.half_w = (double)width / 2.0, a.half_h = (double)height / 2.0, a.w_last = (double)(width - 1), a.h_last = (double)(height - 1);
  a.u_top = (double)(width - 2), a.w_top = (double)(height - 2), a.relax = relax;
  a.P = (int32_t)((int64_t)n0 * n1 * n2), a.n1 = n1, a.n2 = n2, a.V = n_views, a.W = width, a.H = height, a.nonneg = nonneg != 0;
  const unsigned blocks = (unsigned)(((int64_t)a.P + XR_BLOCK - 1) / XR_BLOCK);
  hipLaunchKernelGGL(k_xray_backproject, dim3(blocks), dim3(XR_BLOCK), 0, (hipStream_t)stream, a, (const afx::ViewRecord*)views, images, acc, seen,
                     x_inout, mask);
  return afx::launched(who);
}
