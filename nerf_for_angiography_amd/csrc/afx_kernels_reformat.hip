// afx_kernels_reformat.hip - planes sampled out of a volume (afx_reformat_planes); the definition stands in include/afx.h.  Every plane of
// a list (centre, two in-plane unit vectors: the frames carried along a centreline) is sampled at the Q in-plane offsets of one table, each
// sample the mean or the maximum of a slab of 2 H + 1 trilinear lookups.  One lane per (plane, table row), the table row fastest: the order
// of the table decides which samples share a wavefront, and the caller owns that order.  No LDS, no atomics, nothing allocated.
// NOTHING CAN HANG: no lane waits for a value that another lane or wave writes, and the slab loop runs 2 H + 1 times, a count that is a
// kernel argument.  Every load of the volume is made after the index test of the definition passed; p < P and q < Q before a row is read.
#include "afx_internal.h"
#include "afx_geom.h"
#include <cmath>

// every fp64 product and sum below is rounded on its own (the definition is stated operation by operation); plain operators under this
// pragma, as in afx_kernels_lumen.hip
#pragma clang fp contract(off)

namespace {

constexpr int RF_BLOCK = 256;                         // 4 waves
constexpr int64_t RF_GRID_X = (int64_t)1 << 22;       // blocks along x; the rest of a larger launch goes along y
constexpr int64_t RF_GRID_Y = 65535;
constexpr int RF_MAX_HALF_SLAB = 127;
constexpr int64_t RF_MAX_TABLE = (int64_t)1 << 20;

struct ReformatArgs {
  double W[12];
  double fill, count;                                 // count = 2 H + 1 as a double
  int64_t P, Q;
  int32_t n0, n1, n2, H, mode;
};

// the lookup of afx_lumen_profile's step 4 with `fill` outside: afx::lattice_lookup
template <typename T>
__device__ __forceinline__ double rf_lookup(const ReformatArgs& a, const T* __restrict__ vol, double x0, double x1, double x2) {
  return afx::lattice_lookup(a, vol, x0, x1, x2, a.fill);
}

template <typename T>
__global__ void __launch_bounds__(RF_BLOCK) k_reformat_planes(const ReformatArgs a, const T* __restrict__ vol, const double* __restrict__ planes,
                                                              const double* __restrict__ table, double* __restrict__ out) {
  const int64_t block = (int64_t)blockIdx.y * (int64_t)gridDim.x + (int64_t)blockIdx.x;
  const int64_t flat = block * RF_BLOCK + threadIdx.x;
  if (flat >= a.P * a.Q) return;                      // P <= 2^31 - 1, Q <= 2^20: the product stays below 2^51
  const int64_t p = flat / a.Q, q = flat - p * a.Q;
  const double* pl = planes + 9 * p;
  const double* tb = table + 4 * q;
  const double c0 = pl[0], c1 = pl[1], c2 = pl[2], u0 = pl[3], u1 = pl[4], u2 = pl[5], v0 = pl[6], v1 = pl[7], v2 = pl[8];
  const double ta = tb[0], tb_ = tb[1], sa = tb[2], sb = tb[3];
  double acc = 0.0;
#pragma unroll 1
  for (int m = -a.H; m <= a.H; ++m) {
    const double dm = (double)m;
    const double alpha = ta + dm * sa, beta = tb_ + dm * sb;
    const double f = rf_lookup(a, vol, (c0 + alpha * u0) + beta * v0, (c1 + alpha * u1) + beta * v1, (c2 + alpha * u2) + beta * v2);
    if (a.mode == 0)
      acc = acc + f;
    else
      acc = (m == -a.H || f > acc) ? f : acc;
  }
  out[flat] = a.mode == 0 ? acc / a.count : acc;
}

}  // namespace

extern "C" int afx_reformat_planes(const void* vol, int32_t vol_is_f64, int32_t n0, int32_t n1, int32_t n2, const double* world_to_index,
                                   const double* planes, int64_t n_planes, const double* table, int64_t n_table, int32_t half_slab,
                                   int32_t mode, double fill, double* out, void* stream) {
  const char* who = "afx_reformat_planes";
  if (!vol) return afx::set_error(AFX_E_INVALID, who, "null vol");
  if (!world_to_index) return afx::set_error(AFX_E_INVALID, who, "null world_to_index");
  if (n0 < 2 || n1 < 2 || n2 < 2) return afx::set_error(AFX_E_INVALID, who, "n0, n1, n2: need at least 2 voxels along each axis");
  if (int rc = afx::check_lattice_size(n0, n1, n2, who)) return rc;
  if (n_planes < 0 || n_planes > 0x7fffffff) return afx::set_error(AFX_E_INVALID, who, "n_planes must lie in 0..2^31 - 1");
  if (n_table < 0 || n_table > RF_MAX_TABLE) return afx::set_error(AFX_E_INVALID, who, "n_table must lie in 0..2^20");
  if (half_slab < 0 || half_slab > RF_MAX_HALF_SLAB) return afx::set_error(AFX_E_INVALID, who, "half_slab must lie in 0..127");
  if (mode != AFX_REFORMAT_MEAN && mode != AFX_REFORMAT_MAX) return afx::set_error(AFX_E_INVALID, who, "mode must be 0 (mean) or 1 (max)");
  if (!std::isfinite(fill)) return afx::set_error(AFX_E_INVALID, who, "fill must be finite");
  if (!afx::all_finite(world_to_index, 12)) return afx::set_error(AFX_E_INVALID, who, "world_to_index must be finite");
  const int64_t blocks = (n_planes * n_table + RF_BLOCK - 1) / RF_BLOCK;      // < 2^43
  const int64_t gx = blocks < RF_GRID_X ? blocks : RF_GRID_X, gy = gx ? (blocks + gx - 1) / gx : 0;
  if (gy > RF_GRID_Y) return afx::set_error(AFX_E_INVALID, who, "n_planes n_table: more samples than one launch holds (2^46)");
  if (n_planes == 0 || n_table == 0) return AFX_OK;   // nothing to launch
  if (!planes) return afx::set_error(AFX_E_INVALID, who, "null planes");
  if (!table) return afx::set_error(AFX_E_INVALID, who, "null table");
  if (!out) return afx::set_error(AFX_E_INVALID, who, "null out");
  if (int rc = afx::check_device(vol, "the volume", who)) return rc;
  if (int rc = afx::check_device(planes, "planes", who)) return rc;
  if (int rc = afx::check_device(table, "table", who)) return rc;
  if (int rc = afx::check_device(out, "out", who)) return rc;
  ReformatArgs a;
  for (int i = 0; i < 12; ++i) a.W[i] = world_to_index[i];
  a.fill = fill, a.count = (double)(2 * half_slab + 1), a.P = n_planes, a.Q = n_table;
  a.n0 = n0, a.n1 = n1, a.n2 = n2, a.H = half_slab, a.mode = mode;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (vol_is_f64)
    hipLaunchKernelGGL(k_reformat_planes<double>, grid, dim3(RF_BLOCK), 0, st, a, (const double*)vol, planes, table, out);
  else
    hipLaunchKernelGGL(k_reformat_planes<float>, grid, dim3(RF_BLOCK), 0, st, a, (const float*)vol, planes, table, out);
  return afx::launched(who);
}
