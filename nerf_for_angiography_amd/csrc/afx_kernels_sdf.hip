// afx_kernels_sdf.hip — a triangle mesh back into a volume: the signed distance field of an indexed triangle mesh on a regular grid
// (afx_mesh_sdf_3d) and the unsigned distance of arbitrary points to a mesh (afx_mesh_point_distance).  Its own translation unit: the
// kernels and the host entry points declared in include/afx.h.  The definition - the squared distance of a point to a triangle as the
// minimum of three segment terms and a plane term, the nearest triangle, the generalised winding number and the sign - is in the
// header, operation by operation; every implementation that follows it gives the same distance and the same nearest index.
//
// The grid call: a prepare kernel (one thread per triangle: is it valid, its nine coordinates as fp64 in a structure of arrays, its
// bounding sphere) and one kernel in which a workgroup owns a brick of 8 x 8 x 8 neighbouring grid points.  The workgroup first finds the
// exact distance of the brick's centre to the mesh (its threads share the triangles), then walks the triangles in tiles: every thread
// tests one triangle's bounding sphere against the brick, the survivors are compacted into LDS in index order, and every thread runs
// over the survivors only - all lanes read the same LDS address, a broadcast - skipping those whose sphere lies beyond the nearest
// distance the thread has found so far, and evaluating the exact distance of the rest.  The brick-level test is what makes the work
// scale with the surface near the brick; it cannot drop anything when the whole mesh is smaller than the brick's reach (every triangle
// then lies within dc + 2 R of the centre), which is where the per-point test still halves the work.  The minimum is exact (a
// comparison), so it does not depend on which other triangles were looked at: the culled result equals the unculled one bit for bit,
// as long as neither test drops a triangle that attains the minimum (see sdf_keep).  Then the sign: the winding number, per point and
// in triangle order (the sum is fp64 and its order is part of the definition), or once per brick where the caller promised a closed
// mesh and the surface does not come near the brick.
//
// Brick size: 8 x 8 x 8 points = 512 threads = 8 waves, one 8 x 8 slab of the brick per wave.  -Rpass-analysis=kernel-resource-usage
// gives k_sdf_grid 114 VGPRs without spills, 4 waves per SIMD: registers, not LDS (58 KiB per workgroup: 36 of triangle tile, 2 of
// indices, 16 of bounding spheres, 4 of reduction scratch), bound the occupancy, so a CU holds 16 waves as two 8 x 8 x 8 workgroups or
// as four 8 x 8 x 4 ones.  At the same occupancy the larger brick halves the per-brick work (the distance of the centre to every
// triangle and one sphere test per triangle), which is the part the culling cannot remove; hence 8 x 8 x 8.
//
// Integer atomics only (the 64-bit counters of the record).  Nothing allocates or synchronises: both calls are hipGraph-capturable and
// give the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include "../../include/afx.h"
#include "afx_internal.h"

// every product and sum below is rounded on its own (the distance is defined operation by operation)
#pragma clang fp contract(off)

namespace {

constexpr int SDF_SIDE = 8;                           // a brick is SDF_SIDE^3 grid points, one per thread
constexpr int SDF_BLOCK = SDF_SIDE * SDF_SIDE * SDF_SIDE;
constexpr int SDF_TILE = AFX_MESH_SDF_TILE;           // triangles per LDS tile: one per thread
constexpr int SDF_WAVES = SDF_BLOCK / 64;
constexpr int PREP_BLOCK = 256;
constexpr int PD_BLOCK = 256;                         // afx_mesh_point_distance: points per workgroup = triangles per LDS tile
constexpr double SDF_REL = 1e-12;                     // the pad of the conservative tests (sdf_keep)
constexpr double FOUR_PI = 12.566370614359172;        // 4 pi rounded to fp64
enum { SDF_VALID = 0, SDF_SKIPPED = 1, SDF_CLEAR = 2, SDF_PAIRS = 3 };
static_assert(SDF_TILE == SDF_BLOCK, "one triangle of a tile per thread");

struct SdfAffine { double m[12]; };                   // rows m[r][0..2], o[r]: index_to_world as the caller gave it

struct SdfBufs {
  double* tv;           // [9][Tp] the triangles' coordinates, ax ay az bx by bz cx cy cz, fp64 (zero for a skipped triangle)
  double* ts;           // [4][Tp] bounding sphere: centre, radius; radius -1 marks a skipped triangle
  size_t Tp;            // max(T, 1)
};

SdfBufs carve_sdf(afx::Carve& c, int64_t n_triangles) {
  SdfBufs b;
  b.Tp = (size_t)std::max<int64_t>(n_triangles, 1);
  b.tv = c.take<double>(9 * b.Tp * sizeof(double));
  b.ts = c.take<double>(4 * b.Tp * sizeof(double));
  return b;
}

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return (ax * bx + ay * by) + az * bz;
}

// |p - (a + t ab)|^2, t = ((p - a) . ab) / (ab . ab) clamped to [0, 1], 0 for a segment of length 0
__device__ __forceinline__ double seg_d2(double px, double py, double pz, double ax, double ay, double az, double bx, double by, double bz) {
  const double ex = bx - ax, ey = by - ay, ez = bz - az;
  const double wx = px - ax, wy = py - ay, wz = pz - az;
  const double den = dot3(ex, ey, ez, ex, ey, ez);
  double t = den > 0.0 ? dot3(wx, wy, wz, ex, ey, ez) / den : 0.0;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  const double dx = px - (ax + t * ex), dy = py - (ay + t * ey), dz = pz - (az + t * ez);
  return dot3(dx, dy, dz, dx, dy, dz);
}

// ((e x w) . n), e an edge, w = p - the edge's start
__device__ __forceinline__ double edge_fn(double ex, double ey, double ez, double wx, double wy, double wz, double nx, double ny, double nz) {
  return dot3(ey * wz - ez * wy, ez * wx - ex * wz, ex * wy - ey * wx, nx, ny, nz);
}

// The squared distance from p to the triangle t[0..8] = a, b, c: the header's definition, in its order.
__device__ __forceinline__ double tri_d2(double px, double py, double pz, const double* t) {
  const double ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
  double d = seg_d2(px, py, pz, ax, ay, az, bx, by, bz);
  const double d1 = seg_d2(px, py, pz, bx, by, bz, cx, cy, cz);
  d = d1 < d ? d1 : d;
  const double d2 = seg_d2(px, py, pz, cx, cy, cz, ax, ay, az);
  d = d2 < d ? d2 : d;
  const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
  const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const double nn = dot3(nx, ny, nz, nx, ny, nz);
  if (nn > 0.0) {
    const double wx = px - ax, wy = py - ay, wz = pz - az;
    const double e0 = edge_fn(ux, uy, uz, wx, wy, wz, nx, ny, nz);
    const double e1 = edge_fn(cx - bx, cy - by, cz - bz, px - bx, py - by, pz - bz, nx, ny, nz);
    const double e2 = edge_fn(ax - cx, ay - cy, az - cz, px - cx, py - cy, pz - cz, nx, ny, nz);
    if (e0 > 0.0 && e1 > 0.0 && e2 > 0.0) {
      const double h = dot3(wx, wy, wz, nx, ny, nz);
      const double pl = (h * h) / nn;
      d = pl < d ? pl : d;
    }
  }
  return d;
}

// One term of the winding number: 2 atan2(det[A B C], |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|), A = a - p, B = b - p, C = c - p
__device__ __forceinline__ double winding_term(double px, double py, double pz, const double* t) {
  const double ax = t[0] - px, ay = t[1] - py, az = t[2] - pz;
  const double bx = t[3] - px, by = t[4] - py, bz = t[5] - pz;
  const double cx = t[6] - px, cy = t[7] - py, cz = t[8] - pz;
  const double det = dot3(ax, ay, az, by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx);
  const double la = __dsqrt_rn(dot3(ax, ay, az, ax, ay, az)), lb = __dsqrt_rn(dot3(bx, by, bz, bx, by, bz));
  const double lc = __dsqrt_rn(dot3(cx, cy, cz, cx, cy, cz));
  const double den = (((la * lb) * lc + dot3(ax, ay, az, bx, by, bz) * lc) + dot3(bx, by, bz, cx, cy, cz) * la) + dot3(cx, cy, cz, ax, ay, az) * lb;
  return 2.0 * atan2(det, den);
}

// Triangle t of the caller's arrays as nine doubles; false (nothing usable in o) when it names a vertex outside 0..V-1 or one with a
// non-finite coordinate.  Nothing is read beyond the vertex array.
__device__ __forceinline__ bool load_triangle(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ tri, size_t t, double* o) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int32_t i = tri[3 * t + j];
    const bool in = i >= 0 && (int64_t)i < V;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = in ? vertices[3 * (size_t)i + k] : 0.0f;
      ok = ok && in && isfinite(x);
      o[3 * j + k] = (double)x;
    }
  }
  return ok;
}

__global__ void k_sdf_zero_record(unsigned long long* __restrict__ rec) {
  if (threadIdx.x < AFX_MESH_SDF_RECORD_SLOTS) rec[threadIdx.x] = 0ull;
}

// Prepare: one thread per triangle.  The bounding sphere is centred on the middle of the bounding box; its radius is the largest
// computed distance of a corner from there (the rounding is covered by the pad of the tests that use it).
__global__ void __launch_bounds__(PREP_BLOCK) k_sdf_prepare(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ tri,
                                                            size_t T, SdfBufs b, unsigned long long* __restrict__ rec) {
  const size_t t = (size_t)blockIdx.x * PREP_BLOCK + threadIdx.x;
  bool ok = false;
  if (t < T) {
    double o[9];
    ok = load_triangle(vertices, V, tri, t, o);
    double c[3], r2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double lo = fmin(o[k], fmin(o[3 + k], o[6 + k])), hi = fmax(o[k], fmax(o[3 + k], o[6 + k]));
      c[k] = 0.5 * lo + 0.5 * hi;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double dx = o[3 * j] - c[0], dy = o[3 * j + 1] - c[1], dz = o[3 * j + 2] - c[2];
      r2 = fmax(r2, dot3(dx, dy, dz, dx, dy, dz));
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) b.tv[k * b.Tp + t] = ok ? o[k] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) b.ts[k * b.Tp + t] = ok ? c[k] : 0.0;
    b.ts[3 * b.Tp + t] = ok ? __dsqrt_rn(r2) : -1.0;
  }
  const unsigned long long good = __ballot(ok), all = __ballot(t < T);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(rec + SDF_VALID, (unsigned long long)__popcll(good));
    atomicAdd(rec + SDF_SKIPPED, (unsigned long long)(__popcll(all) - __popcll(good)));
  }
}

__device__ __forceinline__ void sdf_world(const SdfAffine& a, double q0, double q1, double q2, double* w) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double* m = a.m + 4 * r;
    w[r] = ((m[3] + m[0] * q0) + m[1] * q1) + m[2] * q2;
  }
}

// The conservative test of the cull.  In exact arithmetic a triangle inside the sphere (ct, rt) is farther from every point of the brick
// (a ball of radius R about cb) than the nearest triangle when |ct - cb| - rt - R > dc + R, dc the distance of cb to the mesh: a point p
// of the brick has d(p) <= dc + |p - cb| <= dc + R.  So a triangle is kept when |ct - cb| <= dc + 2 R + rt, and every triangle that
// attains the minimum at some point of the brick - ties included - is kept.  The quantities are rounded: each is a short chain of fp64
// operations on coordinates, off by a few units of 2^-53 relative to the largest magnitude involved (the coordinates themselves for the
// differences, the distances for the rest), and so are the d^2 values whose comparison the argument is about.  The test therefore keeps
// a triangle up to (1 + 1e-12) times the limit plus 1e-12 times the coordinates' magnitude: four orders of magnitude above any of those
// errors, and far below anything that would keep a triangle for no reason.
__device__ __forceinline__ bool sdf_keep(double dist, double limit, double mag) {
  return dist <= limit * (1.0 + SDF_REL) + SDF_REL * mag;
}

__device__ __forceinline__ double block_min(double x, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = x;
  __syncthreads();
  for (int s = SDF_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = red[t + s] < red[t] ? red[t + s] : red[t];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double block_sum(double x, double* red) {      // a fixed tree
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = x;
  __syncthreads();
  for (int s = SDF_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = red[t] + red[t + s];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(SDF_BLOCK) k_sdf_grid(SdfBufs b, size_t T, int n0, int n1, int n2, SdfAffine aff, int brute, int closed,
                                                        float* __restrict__ sdf, int32_t* __restrict__ nearest, double* __restrict__ winding,
                                                        unsigned long long* __restrict__ rec) {
  __shared__ double s_tri[SDF_TILE * 9];
  __shared__ int32_t s_idx[SDF_TILE];
  __shared__ double s_sph[SDF_TILE * 4];            // the survivors' spheres: centre, and the radius padded for the per-point test
  __shared__ double s_red[SDF_BLOCK];
  __shared__ int s_wcnt[SDF_WAVES];
  __shared__ unsigned long long s_pairs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_pairs = 0ull;
  const uint32_t nb1 = (uint32_t)(n1 + SDF_SIDE - 1) / SDF_SIDE, nb2 = (uint32_t)(n2 + SDF_SIDE - 1) / SDF_SIDE;
  const uint32_t bid = blockIdx.x, b2 = bid % nb2, b1 = (bid / nb2) % nb1, b0 = bid / (nb2 * nb1);
  const int lo0 = (int)b0 * SDF_SIDE, lo1 = (int)b1 * SDF_SIDE, lo2 = (int)b2 * SDF_SIDE;
  const int hi0 = min(lo0 + SDF_SIDE - 1, n0 - 1), hi1 = min(lo1 + SDF_SIDE - 1, n1 - 1), hi2 = min(lo2 + SDF_SIDE - 1, n2 - 1);
  const int i0 = lo0 + (tid >> 6), i1 = lo1 + ((tid >> 3) & 7), i2 = lo2 + (tid & 7);
  const bool active = i0 <= hi0 && i1 <= hi1 && i2 <= hi2;
  double p[3];
  sdf_world(aff, (double)i0, (double)i1, (double)i2, p);

  // the brick as a ball: the centre of its index box and the farthest of its eight corners (the affine may shear)
  double cb[3], R2 = 0.0;
  sdf_world(aff, 0.5 * (double)(lo0 + hi0), 0.5 * (double)(lo1 + hi1), 0.5 * (double)(lo2 + hi2), cb);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double w[3];
    sdf_world(aff, (double)((k & 4) ? hi0 : lo0), (double)((k & 2) ? hi1 : lo1), (double)((k & 1) ? hi2 : lo2), w);
    const double dx = w[0] - cb[0], dy = w[1] - cb[1], dz = w[2] - cb[2];
    R2 = fmax(R2, dot3(dx, dy, dz, dx, dy, dz));
  }
  const double R = __dsqrt_rn(R2);
  const double magb = fmax(fabs(cb[0]), fmax(fabs(cb[1]), fabs(cb[2]))) + R;

  // ---- the bound: the exact distance of the centre to the mesh
  double dc = INFINITY;
  if (!brute || closed) {
    double m = INFINITY;
    for (size_t t = tid; t < T; t += SDF_BLOCK) {
      if (b.ts[3 * b.Tp + t] < 0.0) continue;
      double o[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) o[k] = b.tv[k * b.Tp + t];
      const double d = tri_d2(cb[0], cb[1], cb[2], o);
      m = d < m ? d : m;
    }
    dc = __dsqrt_rn(block_min(m, s_red));
  }
  const double reach = dc + 2.0 * R;

  // ---- cull and evaluate, tile by tile.  Survivors keep their index order, so the first strict minimum is the smallest index.
  // Per point a survivor is skipped when its sphere lies beyond the best distance so far: |p - ct| - rt > sqrt(best) means that every
  // point of the triangle is farther than a triangle already seen, so it cannot attain the minimum, not even as a tie.  Padded like
  // the brick's test: the radius by a relative 1e-12 and 1e-12 of the coordinates' magnitude (once per survivor), sqrt(best) by a
  // relative 1e-12.
  double best = INFINITY, sbest = INFINITY;            // sbest: sqrt(best) (1 + 1e-12)
  int32_t bi = -1;
  unsigned long long evaluated = 0;                    // exact evaluations of this thread
  for (size_t t0 = 0; t0 < T; t0 += SDF_TILE) {
    const size_t t = t0 + tid;
    bool keep = false;
    double cx = 0.0, cy = 0.0, cz = 0.0, rpad = 0.0;
    if (t < T) {
      const double rt = b.ts[3 * b.Tp + t];
      if (rt >= 0.0) {
        if (brute) {
          keep = true;
        } else {
          cx = b.ts[t], cy = b.ts[b.Tp + t], cz = b.ts[2 * b.Tp + t];
          const double dx = cx - cb[0], dy = cy - cb[1], dz = cz - cb[2];
          const double mag = magb + fmax(fabs(cx), fmax(fabs(cy), fabs(cz))) + rt;
          keep = sdf_keep(__dsqrt_rn(dot3(dx, dy, dz, dx, dy, dz)), reach + rt, mag);
          rpad = rt * (1.0 + SDF_REL) + SDF_REL * mag;
        }
      }
    }
    const unsigned long long vote = __ballot(keep);
    if (lane == 0) s_wcnt[wave] = __popcll(vote);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SDF_WAVES; ++w) {
      const int c = s_wcnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (keep) {
      const int pos = before + __popcll(vote & ((1ull << lane) - 1ull));
#pragma unroll
      for (int k = 0; k < 9; ++k) s_tri[pos * 9 + k] = b.tv[k * b.Tp + t];
      s_idx[pos] = (int32_t)t;
      s_sph[pos * 4] = cx; s_sph[pos * 4 + 1] = cy; s_sph[pos * 4 + 2] = cz; s_sph[pos * 4 + 3] = rpad;
    }
    __syncthreads();
    if (active)
      for (int s = 0; s < total; ++s) {
        if (!brute) {
          const double* sp = s_sph + s * 4;
          const double dx = p[0] - sp[0], dy = p[1] - sp[1], dz = p[2] - sp[2], lim = sbest + sp[3];
          if (dot3(dx, dy, dz, dx, dy, dz) > lim * lim) continue;
        }
        const double d = tri_d2(p[0], p[1], p[2], s_tri + s * 9);
        ++evaluated;
        if (d < best) { best = d; bi = s_idx[s]; sbest = __dsqrt_rn(d) * (1.0 + SDF_REL); }
      }
    __syncthreads();
  }
  if (evaluated) atomicAdd(&s_pairs, evaluated);       // (an integer sum: the same whatever the order)

  // ---- the sign.  Clear: the caller promised a closed mesh and no triangle comes nearer the centre than the brick reaches (padded as
  // above), so the winding number is the same at every point of the brick: one evaluation at the centre, shared, its terms summed by a
  // fixed tree.  Otherwise every point sums all the triangles in index order.
  const bool clear = closed && !winding && dc > R * (1.0 + SDF_REL) + SDF_REL * magb;
  double wsum = 0.0;
  if (clear) {
    double part = 0.0;
    for (size_t t = tid; t < T; t += SDF_BLOCK) {
      if (b.ts[3 * b.Tp + t] < 0.0) continue;
      double o[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) o[k] = b.tv[k * b.Tp + t];
      part += winding_term(cb[0], cb[1], cb[2], o);
    }
    wsum = block_sum(part, s_red);
  } else {
    for (size_t t0 = 0; t0 < T; t0 += SDF_TILE) {
      const size_t t = t0 + tid;
      if (t < T) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s_tri[tid * 9 + k] = b.tv[k * b.Tp + t];
        s_idx[tid] = b.ts[3 * b.Tp + t] >= 0.0 ? 1 : 0;
      }
      __syncthreads();
      const int count = (int)min((size_t)SDF_TILE, T - t0);
      if (active)
        for (int s = 0; s < count; ++s)
          if (s_idx[s]) wsum += winding_term(p[0], p[1], p[2], s_tri + s * 9);
      __syncthreads();
    }
  }

  if (active) {
    const size_t v = ((size_t)i0 * (size_t)n1 + (size_t)i1) * (size_t)n2 + (size_t)i2;
    const double w = wsum / FOUR_PI, d = __dsqrt_rn(best);
    sdf[v] = (float)((w >= 0.5 && d > 0.0) ? -d : d);
    if (nearest) nearest[v] = bi;
    if (winding) winding[v] = w;
  }
  __syncthreads();
  if (tid == 0) {
    atomicAdd(rec + SDF_PAIRS, s_pairs);
    if (clear) atomicAdd(rec + SDF_CLEAR, 1ull);
  }
}

// afx_mesh_point_distance: one thread per point, the triangles through LDS in tiles of PD_BLOCK (each thread loads and checks one), all
// pairs.  The workgroup of the first points also counts the valid triangles and writes the record: plain stores, no atomics.
__global__ void __launch_bounds__(PD_BLOCK) k_mesh_point_distance(const float* __restrict__ points, int64_t P, const float* __restrict__ vertices,
                                                                  int64_t V, const int32_t* __restrict__ tri, size_t T, float* __restrict__ dist,
                                                                  int32_t* __restrict__ nearest, unsigned long long* __restrict__ rec) {
  __shared__ double s_tri[PD_BLOCK * 9];
  __shared__ int32_t s_ok[PD_BLOCK];
  __shared__ unsigned long long s_cnt[PD_BLOCK / 64];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * PD_BLOCK + tid;
  const bool active = i < P;
  double p[3] = {0.0, 0.0, 0.0};
  if (active)
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = (double)points[3 * (size_t)i + k];
  double best = INFINITY;
  int32_t bi = -1;
  unsigned long long valid = 0;                        // per wave: the valid triangles its lanes loaded
  for (size_t t0 = 0; t0 < T; t0 += PD_BLOCK) {
    const size_t t = t0 + tid;
    bool ok = false;
    if (t < T) {
      double o[9];
      ok = load_triangle(vertices, V, tri, t, o);
#pragma unroll
      for (int k = 0; k < 9; ++k) s_tri[tid * 9 + k] = o[k];
      s_ok[tid] = ok ? 1 : 0;
    }
    valid += (unsigned long long)__popcll(__ballot(ok));
    __syncthreads();
    const int count = (int)min((size_t)PD_BLOCK, T - t0);
    if (active)
      for (int s = 0; s < count; ++s) {
        if (!s_ok[s]) continue;
        const double d = tri_d2(p[0], p[1], p[2], s_tri + s * 9);
        if (d < best) { best = d; bi = (int32_t)(t0 + s); }
      }
    __syncthreads();
  }
  if (active) {
    dist[i] = (float)__dsqrt_rn(best);
    if (nearest) nearest[i] = bi;
  }
  if (blockIdx.x == 0) {
    if ((tid & 63) == 0) s_cnt[tid >> 6] = valid;
    __syncthreads();
    if (tid == 0) {
      unsigned long long good = 0;
      for (int w = 0; w < PD_BLOCK / 64; ++w) good += s_cnt[w];
      rec[SDF_VALID] = good;
      rec[SDF_SKIPPED] = (unsigned long long)T - good;
      rec[SDF_CLEAR] = 0ull;
      rec[SDF_PAIRS] = good * (unsigned long long)P;
      for (int k = 4; k < AFX_MESH_SDF_RECORD_SLOTS; ++k) rec[k] = 0ull;
    }
  }
}

int mesh_args_ok(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const char* who) {
  if (n_vertices < 0 || n_vertices > INT32_MAX || n_triangles < 0 || n_triangles > INT32_MAX)
    return afx::set_error(AFX_E_INVALID, who, "the vertex and triangle counts must lie in 0..2^31 - 1");
  if ((n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles))
    return afx::set_error(AFX_E_INVALID, who, "a count above 0 needs its array");
  return AFX_OK;
}

}  // namespace

extern "C" size_t afx_mesh_sdf_3d_workspace_bytes(int64_t n_triangles) {
  if (n_triangles < 0 || n_triangles > INT32_MAX) return 0;
  afx::Carve c;
  carve_sdf(c, n_triangles);
  return c.end;
}

extern "C" int afx_mesh_sdf_3d(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, int32_t n0, int32_t n1,
                               int32_t n2, const double index_to_world[12], uint32_t flags, float* sdf_out, int32_t* nearest_out,
                               double* winding_out, void* record, void* workspace, size_t workspace_bytes, size_t* workspace_needed,
                               void* stream) {
  const char* who = "afx_mesh_sdf_3d";
  if (!sdf_out || !record || !index_to_world) return afx::set_error(AFX_E_INVALID, who, "null sdf_out, record or index_to_world");
  if (int rc = mesh_args_ok(vertices, n_vertices, triangles, n_triangles, who)) return rc;
  if (!afx::volume_shape_ok(n0, n1, n2)) return afx::set_error(AFX_E_INVALID, who, "need a grid of 1..1024 points along each axis");
  if (flags & ~(uint32_t)(AFX_MESH_SDF_BRUTE | AFX_MESH_SDF_CLOSED)) return afx::set_error(AFX_E_INVALID, who, "unknown flag bits");
  SdfAffine aff;
  for (int k = 0; k < 12; ++k) {
    aff.m[k] = index_to_world[k];
    if (!isfinite(aff.m[k])) return afx::set_error(AFX_E_INVALID, who, "index_to_world has a non-finite entry");
  }
  const double* m = aff.m;
  const double det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
  if (!(det != 0.0) || !isfinite(det)) return afx::set_error(AFX_E_INVALID, who, "index_to_world is singular (det(m) is 0 or not finite)");
  const size_t need = afx_mesh_sdf_3d_workspace_bytes(n_triangles);
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(sdf_out, "sdf_out", who)) return rc;
  if (int rc = afx::check_device(record, "the record", who)) return rc;
  if (int rc = afx::check_device(workspace, "the workspace", who)) return rc;
  if (vertices) if (int rc = afx::check_device(vertices, "vertices", who)) return rc;
  if (triangles) if (int rc = afx::check_device(triangles, "triangles", who)) return rc;
  if (nearest_out) if (int rc = afx::check_device(nearest_out, "nearest_out", who)) return rc;
  if (winding_out) if (int rc = afx::check_device(winding_out, "winding_out", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  afx::Carve c;
  c.base = (uintptr_t)workspace;
  const SdfBufs b = carve_sdf(c, n_triangles);
  const size_t T = (size_t)n_triangles;
  unsigned long long* rec = (unsigned long long*)record;
  hipLaunchKernelGGL(k_sdf_zero_record, dim3(1), dim3(64), 0, st, rec);
  if (T > 0)
    hipLaunchKernelGGL(k_sdf_prepare, dim3((unsigned)((T + PREP_BLOCK - 1) / PREP_BLOCK)), dim3(PREP_BLOCK), 0, st, vertices, n_vertices,
                       triangles, T, b, rec);
  const unsigned bricks = (unsigned)((n0 + SDF_SIDE - 1) / SDF_SIDE) * (unsigned)((n1 + SDF_SIDE - 1) / SDF_SIDE) *
                          (unsigned)((n2 + SDF_SIDE - 1) / SDF_SIDE);                          // <= 2^21
  hipLaunchKernelGGL(k_sdf_grid, dim3(bricks), dim3(SDF_BLOCK), 0, st, b, T, (int)n0, (int)n1, (int)n2, aff,
                     (int)((flags & AFX_MESH_SDF_BRUTE) != 0), (int)((flags & AFX_MESH_SDF_CLOSED) != 0), sdf_out, nearest_out, winding_out, rec);
  return afx::launched(who);
}

extern "C" int afx_mesh_point_distance(const float* points, int64_t n_points, const float* vertices, int64_t n_vertices, const int32_t* triangles,
                                       int64_t n_triangles, float* dist_out, int32_t* nearest_out, void* record, void* stream) {
  const char* who = "afx_mesh_point_distance";
  if (!record) return afx::set_error(AFX_E_INVALID, who, "null record");
  if (n_points < 0 || n_points > INT32_MAX) return afx::set_error(AFX_E_INVALID, who, "the point count must lie in 0..2^31 - 1");
  if (n_points > 0 && (!points || !dist_out)) return afx::set_error(AFX_E_INVALID, who, "a point count above 0 needs points and dist_out");
  if (int rc = mesh_args_ok(vertices, n_vertices, triangles, n_triangles, who)) return rc;
  if (int rc = afx::check_device(record, "the record", who)) return rc;
  if (points) if (int rc = afx::check_device(points, "points", who)) return rc;
  if (dist_out) if (int rc = afx::check_device(dist_out, "dist_out", who)) return rc;
  if (nearest_out) if (int rc = afx::check_device(nearest_out, "nearest_out", who)) return rc;
  if (vertices) if (int rc = afx::check_device(vertices, "vertices", who)) return rc;
  if (triangles) if (int rc = afx::check_device(triangles, "triangles", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, (n_points + PD_BLOCK - 1) / PD_BLOCK);      // the first one writes the record
  hipLaunchKernelGGL(k_mesh_point_distance, dim3(blocks), dim3(PD_BLOCK), 0, st, points, n_points, vertices, n_vertices, triangles,
                     (size_t)n_triangles, dist_out, nearest_out, (unsigned long long*)record);
  return afx::launched(who);
}
