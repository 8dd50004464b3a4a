// afx_kernels_tv.hip - afx_tv_denoise_3d: the proximal operator of the isotropic 3-D total variation (the Rudin-Osher-Fatemi model) of an
// fp64 volume by Chambolle's dual iteration.  The definition stands in include/afx.h, operation by operation; every fp64 operation here is
// written in that order and rounded on its own, so the device equals the NumPy restatement tests/tv_reference.py bit for bit.
//
// Layout, and why (the results do not depend on it: a voxel's arithmetic is the definition, whoever carries it out).
//   One launch per iteration, the three dual fields p ping-ponged between the two triples of the workspace.  A workgroup of 512 lanes owns
//   a tile of 4 x 8 x 16 voxels (k fastest: a row of the tile is 16 doubles, one 128-byte line; a wavefront is four such rows).  It first
//   forms u = x - div p on the tile plus one layer on the high side of every axis, 5 x 9 x 17 = 765 values (6 120 bytes of LDS), each
//   from x, the old p at the voxel and at its three low neighbours; the layer is recomputed from the same operands by the same operations
//   as the neighbouring workgroup computes it, so no value depends on the tiling.  After one barrier every lane takes its three forward
//   differences from LDS and writes its three new p.  765 / 512 = 1.49 u per voxel; the tile's own loads are shared through the CU's L1
//   and the layer's through the L2, so the traffic to memory stays near x and three p read, three p written (56 bytes a voxel).  At
//   6 KB of LDS and 512 lanes a CU holds its four workgroups (32 wavefronts): occupancy is bound by the wavefront slots, not by LDS.
//   Workgroups are handed to the eight XCDs in turn, each XCD with an L2 of its own, so workgroup v takes tile (v % 8) chunk + v / 8:
//   the workgroups that share an L2 walk consecutive tiles, and the layer a tile shares with its neighbour is read from memory once
//   instead of once per XCD (measured at 201^3: 120 -> 42 bytes read per voxel and iteration, 178 -> 147 us; profiles/r24_tv_denoise.md).
//   The first iteration reads no p at all: p = +0 gives div = (+0 + +0) + +0 = +0 exactly, so nothing has to be cleared.
//   A last launch, a lane per voxel, writes out = x - div p with the clamp and the mask; it reads and writes its own voxel only, so out
//   may be x.
// No atomics, no reduction, nothing read back: the call can be captured in a graph.  NOTHING CAN HANG: the only wait is the workgroup's
// barrier, reached by all 512 lanes the same number of times (the tile loop's bounds are kernel arguments and uniform in the workgroup).
// Every load and store is made at a voxel (i, j, k) with 0 <= i < n0, 0 <= j < n1, 0 <= k < n2, or at its low neighbour behind i_a > 0.
#include "afx_internal.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int TV_T0 = 4, TV_T1 = 8, TV_T2 = 16;                 // the tile: AFX_TV_TILE_0, _1, _2 of include/afx.h
static_assert(TV_T0 == AFX_TV_TILE_0 && TV_T1 == AFX_TV_TILE_1 && TV_T2 == AFX_TV_TILE_2, "the tile is the one the header states");
constexpr int TV_BLOCK = TV_T0 * TV_T1 * TV_T2;                 // 512 lanes
constexpr int TV_H1 = TV_T1 + 1, TV_H2 = TV_T2 + 1;
constexpr int TV_HALO = (TV_T0 + 1) * TV_H1 * TV_H2;            // 765 values of u
constexpr int TV_FINISH_BLOCK = 256;
constexpr uint32_t TV_MAX_BLOCKS = 1u << 22;                    // blocks x lanes stays below 2^32; a workgroup walks further tiles in a loop

struct TvArgs {
  double tau, c;                                      // c = tau / weight
  int32_t n0, n1, n2, b1, b2;                         // b_a: tiles along axis a
  uint32_t tiles, chunk;                              // chunk = ceil(tiles / 8): the consecutive tiles of one XCD's workgroups
  int32_t zero_p;                                    // the old p is +0 everywhere and is not read
};

// div at voxel `at` = (i, j, k): (b_0 + b_1) + b_2, b_a = p_a[i] - (i_a > 0 ? p_a[i - e_a] : +0).  p: the triple p_0, p_1, p_2, N apart.
__device__ __forceinline__ double tv_div(const double* p, size_t n, int32_t i, int32_t j, int32_t k, size_t at, size_t s0, size_t s1) {
  const double* p1 = p + n;
  const double* p2 = p1 + n;
  const double b0 = p[at] - (i > 0 ? p[at - s0] : 0.0);
  const double b1 = p1[at] - (j > 0 ? p1[at - s1] : 0.0);
  const double b2 = p2[at] - (k > 0 ? p2[at - 1] : 0.0);
  return (b0 + b1) + b2;
}

__global__ void __launch_bounds__(TV_BLOCK) k_tv_iterate(const TvArgs a, const double* __restrict__ x, const double* __restrict__ p_old,
                                                         double* __restrict__ p_new) {
  __shared__ double u[TV_HALO];
  const size_t s1 = (size_t)a.n2, s0 = (size_t)a.n1 * (size_t)a.n2, n = (size_t)a.n0 * s0;
  const int tid = threadIdx.x;
  const int lk = tid % TV_T2, lj = (tid / TV_T2) % TV_T1, li = tid / (TV_T2 * TV_T1);
  for (uint32_t v = blockIdx.x; v < 8 * a.chunk; v += gridDim.x) {
    const uint32_t t = (v % 8) * a.chunk + v / 8;     // the workgroups v, v + 8, ... share an XCD: they take consecutive tiles
    if (t >= a.tiles) continue;                       // (uniform in the workgroup)
    const int32_t tk = (int32_t)(t % (uint32_t)a.b2), tj = (int32_t)((t / (uint32_t)a.b2) % (uint32_t)a.b1);
    const int32_t ti = (int32_t)(t / ((uint32_t)a.b2 * (uint32_t)a.b1));
    const int32_t i0 = ti * TV_T0, j0 = tj * TV_T1, k0 = tk * TV_T2;       // inside the volume: 0 <= i0 < n0, ...
    const int32_t r0 = a.n0 - i0, r1 = a.n1 - j0, r2 = a.n2 - k0;          // voxels left from the tile's corner, >= 1
    for (int e = tid; e < TV_HALO; e += TV_BLOCK) {
      const int ek = e % TV_H2, ej = (e / TV_H2) % TV_H1, ei = e / (TV_H2 * TV_H1);
      if (ei < r0 && ej < r1 && ek < r2) {
        const int32_t i = i0 + ei, j = j0 + ej, k = k0 + ek;
        const size_t at = (size_t)i * s0 + (size_t)j * s1 + (size_t)k;
        u[e] = x[at] - (a.zero_p ? 0.0 : tv_div(p_old, n, i, j, k, at, s0, s1));
      }
    }
    __syncthreads();
    if (li < r0 && lj < r1 && lk < r2) {
      const int c = (li * TV_H1 + lj) * TV_H2 + lk;
      const double uc = u[c];
      const double g0 = li + 1 < r0 ? u[c + TV_H1 * TV_H2] - uc : 0.0;      // i < n0 - 1
      const double g1 = lj + 1 < r1 ? u[c + TV_H2] - uc : 0.0;
      const double g2 = lk + 1 < r2 ? u[c + 1] - uc : 0.0;
      const double m = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
      const double den = 1.0 + a.c * m;
      const size_t at = (size_t)(i0 + li) * s0 + (size_t)(j0 + lj) * s1 + (size_t)(k0 + lk);
      const double q0 = a.zero_p ? 0.0 : p_old[at], q1 = a.zero_p ? 0.0 : p_old[n + at], q2 = a.zero_p ? 0.0 : p_old[2 * n + at];
      p_new[at] = (q0 - a.tau * g0) / den;
      p_new[n + at] = (q1 - a.tau * g1) / den;
      p_new[2 * n + at] = (q2 - a.tau * g2) / den;
    }
    __syncthreads();                                  // u is overwritten by the next tile
  }
}

// out = x - div p (p == nullptr: no iteration was made, out = x), clamped and masked.  x and out may be the same array.
__global__ void __launch_bounds__(TV_FINISH_BLOCK) k_tv_finish(int32_t count, int32_t n1, int32_t n2, const double* x, const double* __restrict__ p,
                                                               int32_t nonneg, const uint8_t* __restrict__ mask, double* out) {
  const int64_t at64 = (int64_t)blockIdx.x * TV_FINISH_BLOCK + threadIdx.x;
  if (at64 >= count) return;
  const int32_t at = (int32_t)at64;
  double y = x[at];
  if (p) {
    const int32_t k = at % n2, ij = at / n2, j = ij % n1, i = ij / n1;
    y = y - tv_div(p, (size_t)count, i, j, k, (size_t)at, (size_t)n1 * (size_t)n2, (size_t)n2);
  }
  if (nonneg) y = y > 0.0 ? y : 0.0;
  if (mask && mask[at] == 0) y = 0.0;
  out[at] = y;
}

// the voxel count, or 0 when an extent is below 1 or the product does not fit in 31 bits
int64_t tv_count(int32_t n0, int32_t n1, int32_t n2) {
  if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
  const int64_t n01 = (int64_t)n0 * n1;
  if (n01 >= (int64_t)1 << 31 || n01 * n2 >= (int64_t)1 << 31) return 0;
  return n01 * n2;
}

}  // namespace

extern "C" size_t afx_tv_denoise_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2) {
  return (size_t)tv_count(n0, n1, n2) * 6 * sizeof(double);
}

extern "C" int afx_tv_denoise_3d(const double* x, int32_t n0, int32_t n1, int32_t n2, double weight, double tau, int32_t iterations,
                                 int32_t nonneg, const uint8_t* mask, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "afx_tv_denoise_3d";
  if (!x) return afx::set_error(AFX_E_INVALID, who, "null x");
  if (!out) return afx::set_error(AFX_E_INVALID, who, "null out");
  if (n0 < 1 || n1 < 1 || n2 < 1) return afx::set_error(AFX_E_INVALID, who, "n0, n1, n2 must be at least 1");
  const int64_t count = tv_count(n0, n1, n2);
  if (count == 0) return afx::set_error(AFX_E_INVALID, who, "n0 n1 n2 must stay below 2^31");
  if (!(std::isfinite(weight) && weight > 0.0)) return afx::set_error(AFX_E_INVALID, who, "weight must be finite and positive");
  if (!(std::isfinite(tau) && tau > 0.0)) return afx::set_error(AFX_E_INVALID, who, "tau must be finite and positive");
  if (iterations < 0) return afx::set_error(AFX_E_INVALID, who, "iterations must not be negative");
  if (iterations > 0) {
    if (!workspace) return afx::set_error(AFX_E_INVALID, who, "null workspace");
    if ((uintptr_t)workspace % sizeof(double)) return afx::set_error(AFX_E_INVALID, who, "workspace must be aligned to 8 bytes");
    if (workspace_bytes < afx_tv_denoise_3d_workspace_bytes(n0, n1, n2))
      return afx::set_error(AFX_E_INVALID, who, "workspace_bytes is below afx_tv_denoise_3d_workspace_bytes");
  }
  if (int rc = afx::check_device_memory(x, "x", who)) return rc;
  if (int rc = afx::check_device_memory(out, "out", who)) return rc;
  if (mask)
    if (int rc = afx::check_device_memory(mask, "mask", who)) return rc;
  if (iterations > 0)
    if (int rc = afx::check_device_memory(workspace, "workspace", who)) return rc;
  TvArgs a;
  a.tau = tau, a.c = tau / weight;
  a.n0 = n0, a.n1 = n1, a.n2 = n2;
  a.b1 = (n1 - 1) / TV_T1 + 1, a.b2 = (n2 - 1) / TV_T2 + 1;
  a.tiles = (uint32_t)((int64_t)((n0 - 1) / TV_T0 + 1) * a.b1 * a.b2);          // < 2^31: a tile holds a voxel at least
  a.chunk = (a.tiles - 1) / 8 + 1;
  const unsigned blocks = 8 * a.chunk < TV_MAX_BLOCKS ? 8 * a.chunk : TV_MAX_BLOCKS;          // a multiple of 8
  double* const triple[2] = {(double*)workspace, (double*)workspace + 3 * count};
  for (int32_t it = 0; it < iterations; ++it) {
    a.zero_p = it == 0;
    hipLaunchKernelGGL(k_tv_iterate, dim3(blocks), dim3(TV_BLOCK), 0, (hipStream_t)stream, a, x, (const double*)triple[(it + 1) & 1],
                       triple[it & 1]);
  }
  const double* p = iterations > 0 ? triple[(iterations - 1) & 1] : nullptr;
  hipLaunchKernelGGL(k_tv_finish, dim3((unsigned)((count + TV_FINISH_BLOCK - 1) / TV_FINISH_BLOCK)), dim3(TV_FINISH_BLOCK), 0,
                     (hipStream_t)stream, (int32_t)count, n1, n2, x, p, (int32_t)(nonneg != 0), mask, out);
  return afx::launched(who);
}
