// afx_kernels_mesh.hip — the reconstructed vessel as a surface: marching tetrahedra on the Kuhn (Freudenthal) split of every grid cube
// (afx_isosurface_3d) and the area and enclosed volume of an indexed triangle mesh (afx_mesh_measures).  Its own translation unit: the
// kernels and the host entry points declared in include/afx.h.  The definitions - which voxel is inside, which edge owns a vertex, the
// order of vertices and triangles, the winding - are in the header; every implementation that follows them gives the same mesh.
//
// No table is typed in: the six tetrahedra, their corner codes, the 16 cases of a tetrahedron and the winding are derived from the
// permutation index and from the four inside bits.  No atomics at all.  Nothing allocates or synchronises: both calls are
// hipGraph-capturable and give the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include "../../include/afx.h"
#include "afx_internal.h"
#include "afx_scan.h"

// every product and sum below is rounded on its own (the vertex positions and the measures are defined operation by operation)
#pragma clang fp contract(off)

namespace {

constexpr int ISO_BLOCK = 256;
constexpr int ISO_ITERS = 4;
constexpr int ISO_CHUNK = ISO_BLOCK * ISO_ITERS;      // consecutive grid points per workgroup: 4 per thread, coalesced
constexpr int ISO_SCAN = 1024;                        // threads of the one scanning workgroup
constexpr int MM_BLOCK = 256;
constexpr int MM_MAX_PART = 2048;                     // workgroups (= partial sums per quantity) of afx_mesh_measures
enum { ISO_V = 0, ISO_T = 1, ISO_E = 2, ISO_B = 3, ISO_22 = 4, ISO_STATUS = 5 };

struct IsoAffine { double m[12]; };                   // rows m[r][0..2], o[r]: index_to_world as the caller gave it

struct IsoBufs {
  uint8_t* mask;        // [N] bit d: the edge from this grid point in direction d is crossed
  uint16_t* vpre;       // [N] vertices owned by the grid points before this one in its chunk
  uint16_t* tpre;       // [N] triangles of the cubes before this one in its chunk
  uint32_t *cv, *ct, *cf, *cb, *c22;      // [chunks] vertices, triangles, crossed faces, crossed boundary faces, 2-2 tetrahedra per chunk
  unsigned long long *voff, *toff;        // [chunks] vertices / triangles before the chunk (written by the scan)
};

IsoBufs carve_iso(afx::Carve& c, int32_t n0, int32_t n1, int32_t n2) {
  const size_t total = (size_t)n0 * n1 * n2, chunks = (total + ISO_CHUNK - 1) / ISO_CHUNK;
  IsoBufs b;
  b.mask = c.take<uint8_t>(total);
  b.vpre = c.take<uint16_t>(total * sizeof(uint16_t));
  b.tpre = c.take<uint16_t>(total * sizeof(uint16_t));
  b.cv = c.take<uint32_t>(chunks * sizeof(uint32_t));
  b.ct = c.take<uint32_t>(chunks * sizeof(uint32_t));
  b.cf = c.take<uint32_t>(chunks * sizeof(uint32_t));
  b.cb = c.take<uint32_t>(chunks * sizeof(uint32_t));
  b.c22 = c.take<uint32_t>(chunks * sizeof(uint32_t));
  b.voff = c.take<unsigned long long>(chunks * sizeof(unsigned long long));
  b.toff = c.take<unsigned long long>(chunks * sizeof(unsigned long long));
  return b;
}

// ---- the Kuhn split, derived.  A corner of the unit cube has the code 4 d0 + 2 d1 + d2 (axis x is bit 2 - x); the direction d of
// an edge is the code of its offset minus 1.  Tetrahedron p = 0..5 belongs to the p-th permutation of (0, 1, 2) in lexicographic
// order: (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0); its corners are 0, e[p0], e[p0] + e[p1], (1,1,1).
struct Kuhn { int codes; int neg; };                  // the four corner codes, 3 bits each (corner j at bits 3j..3j+2); odd permutation

__host__ __device__ constexpr Kuhn kuhn(int p) {
  const int p0 = p >> 1, lo = p0 == 0 ? 1 : 0, hi = p0 == 2 ? 1 : 2;
  const int p1 = (p & 1) ? hi : lo, p2 = (p & 1) ? lo : hi;
  const int k1 = 4 >> p0, k2 = k1 | (4 >> p1);
  return Kuhn{(k1 << 3) | (k2 << 6) | (7 << 9), ((p0 > p1) + (p0 > p2) + (p1 > p2)) & 1};
}

struct IsoCell { int i0, i1, i2; uint32_t valid; };   // valid: bit c set when the grid point + the offset of code c lies in the grid

// `none`: an axis of one voxel - there is no cube, so no edge of the triangulation: only the grid point itself counts
__device__ __forceinline__ IsoCell iso_cell(uint32_t v, int n0, int n1, int n2, int none) {
  const uint32_t s0 = (uint32_t)n1 * (uint32_t)n2;
  IsoCell c;
  c.i0 = (int)(v / s0);
  const uint32_t r = v - (uint32_t)c.i0 * s0;
  c.i1 = (int)(r / (uint32_t)n2);
  c.i2 = (int)(r - (uint32_t)c.i1 * (uint32_t)n2);
  const bool a0 = c.i0 + 1 < n0 && !none, a1 = c.i1 + 1 < n1 && !none, a2 = c.i2 + 1 < n2 && !none;
  c.valid = 1u;
#pragma unroll
  for (int k = 1; k < 8; ++k)
    if ((!(k & 4) || a0) && (!(k & 2) || a1) && (!(k & 1) || a2)) c.valid |= 1u << k;
  return c;
}

// bit c: the corner with code c lies in the grid and is inside (f >= iso; a NaN is outside)
__device__ __forceinline__ uint32_t iso_inside(const float* __restrict__ f, uint32_t v, uint32_t valid, int n1, int n2, float iso) {
  uint32_t in = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if ((valid >> k) & 1u) {
      const uint32_t u = v + (uint32_t)(((k >> 2) & 1) * n1 * n2 + ((k >> 1) & 1) * n2 + (k & 1));
      in |= (uint32_t)(f[u] >= iso) << k;
    }
  return in;
}

__device__ __forceinline__ uint32_t iso_edge_mask(uint32_t in, uint32_t valid) {      // bit d = code - 1
  const uint32_t self = (in & 1u) ? 0xffu : 0u;
  return ((in ^ self) & valid) >> 1;
}

// the four inside bits of tetrahedron `codes`
__device__ __forceinline__ int iso_tet_bits(uint32_t in, int codes) {
  int s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) s |= (int)((in >> ((codes >> (3 * j)) & 7)) & 1u) << j;
  return s;
}

// Classify: one thread per grid point, ISO_ITERS of them.  The edge mask of the point, the triangles and 2-2 tetrahedra of its cube,
// the crossed faces it owns (a face of the triangulation belongs to its smallest corner x: (x, x + g, x + h) with g a proper non-empty
// subset of h; h with two bits lies in a coordinate plane, h = 7 inside the cube), the prefix of the vertex and triangle counts inside
// the chunk (both in one word: at most 7 * 1024 and 12 * 1024) and the chunk's five sums.  The eight corner loads of neighbouring
// threads overlap: they are served by the L2 (the volume is read about once from HBM).
__global__ void __launch_bounds__(ISO_BLOCK) k_iso_classify(const float* __restrict__ f, int n0, int n1, int n2, float iso, int none,
                                                            IsoBufs b) {
  __shared__ uint32_t wfb[ISO_BLOCK / 64][3];
  const uint32_t total = (uint32_t)n0 * (uint32_t)n1 * (uint32_t)n2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t cnt[ISO_ITERS], sum[ISO_ITERS];            // per pass: the point's packed counts, then those before it in the pass; the pass's sum
  uint32_t faces = 0, bfaces = 0, n22 = 0;
#pragma unroll
  for (int i = 0; i < ISO_ITERS; ++i) {
    const uint32_t v = blockIdx.x * ISO_CHUNK + i * ISO_BLOCK + threadIdx.x;
    cnt[i] = 0;
    if (v < total) {
      const IsoCell c = iso_cell(v, n0, n1, n2, none);
      const uint32_t in = iso_inside(f, v, c.valid, n1, n2, iso);
      const uint32_t mask = iso_edge_mask(in, c.valid);
      b.mask[v] = (uint8_t)mask;
      uint32_t nt = 0;
      if (c.valid & 0x80u) {                          // the base of a cube
#pragma unroll
        for (int p = 0; p < 6; ++p) {
          const int ns = __popc(iso_tet_bits(in, kuhn(p).codes));
          nt += (ns == 2) ? 2u : (ns == 1 || ns == 3) ? 1u : 0u;
          n22 += ns == 2;
        }
      }
#pragma unroll
      for (int h = 3; h < 8; ++h) {
        if (__popc(h) < 2 || !((c.valid >> h) & 1u)) continue;
        // a face in a coordinate plane lies on the boundary when its plane is the first or the last of the axis it is normal to
        const int axis = h == 3 ? 0 : h == 5 ? 1 : 2, at = axis == 0 ? c.i0 : axis == 1 ? c.i1 : c.i2, last = axis == 0 ? n0 : axis == 1 ? n1 : n2;
        const bool edge = h != 7 && (at == 0 || at == last - 1);
#pragma unroll
        for (int g = 1; g < h; ++g) {
          if ((g & ~h) != 0) continue;
          const uint32_t a = in & 1u, x = (in >> g) & 1u, y = (in >> h) & 1u;
          const bool crossed = a != x || a != y;
          faces += crossed;
          bfaces += crossed && edge;
        }
      }
      cnt[i] = (uint32_t)__popc(mask) | (nt << 16);
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    faces += __shfl_down(faces, d);
    bfaces += __shfl_down(bfaces, d);
    n22 += __shfl_down(n22, d);
  }
  if (lane == 0) { wfb[wave][0] = faces; wfb[wave][1] = bfaces; wfb[wave][2] = n22; }
  afx::block_exclusive_scan<ISO_BLOCK>(cnt, sum);     // (its barriers also publish wfb)
  uint32_t run = 0;
#pragma unroll
  for (int i = 0; i < ISO_ITERS; ++i) {
    const uint32_t v = blockIdx.x * ISO_CHUNK + i * ISO_BLOCK + threadIdx.x;
    if (v < total) {
      const uint32_t ex = run + cnt[i];
      b.vpre[v] = (uint16_t)(ex & 0xffffu);
      b.tpre[v] = (uint16_t)(ex >> 16);
    }
    run += sum[i];
  }
  if (threadIdx.x == 0) {
    b.cv[blockIdx.x] = run & 0xffffu;
    b.ct[blockIdx.x] = run >> 16;
    b.cf[blockIdx.x] = wfb[0][0] + wfb[1][0] + wfb[2][0] + wfb[3][0];
    b.cb[blockIdx.x] = wfb[0][1] + wfb[1][1] + wfb[2][1] + wfb[3][1];
    b.c22[blockIdx.x] = wfb[0][2] + wfb[1][2] + wfb[2][2] + wfb[3][2];
  }
}

// one workgroup: voff[] / toff[] = the exclusive scans of cv[] / ct[] (64-bit: 7 * 2^30 vertices do not fit 32), and the record
__global__ void __launch_bounds__(ISO_SCAN) k_iso_scan(IsoBufs b, uint32_t nb, unsigned long long max_vertices, unsigned long long max_triangles,
                                                       unsigned long long* __restrict__ rec) {
  uint32_t b0, b1;
  afx::scan_run<ISO_SCAN>(nb, b0, b1);
  unsigned long long p[5] = {0, 0, 0, 0, 0}, tot[5];  // vertices, triangles, crossed faces, boundary faces, 2-2 tetrahedra
  for (uint32_t k = b0; k < b1; ++k) { p[0] += b.cv[k]; p[1] += b.ct[k]; p[2] += b.cf[k]; p[3] += b.cb[k]; p[4] += b.c22[k]; }
  afx::block_exclusive_scan<ISO_SCAN>(p, tot);
  for (uint32_t k = b0; k < b1; ++k) {
    b.voff[k] = p[0]; p[0] += b.cv[k];
    b.toff[k] = p[1]; p[1] += b.ct[k];
  }
  if (threadIdx.x == 0) {
    const unsigned long long V = tot[0], T = tot[1], F = tot[2], B = tot[3], N22 = tot[4];
    rec[ISO_V] = V; rec[ISO_T] = T; rec[ISO_E] = F + N22; rec[ISO_B] = B; rec[ISO_22] = N22;
    rec[ISO_STATUS] = (V > max_vertices ? 1ull : 0ull) | (T > max_triangles ? 2ull : 0ull);
    rec[6] = 0; rec[7] = 0;
  }
}

// the id of the vertex on the edge between the cube corners with codes ka and kb (one a subset of the other), v = the cube's base
__device__ __forceinline__ unsigned long long iso_vertex_id(const IsoBufs& b, uint32_t v, int n1, int n2, int ka, int kb) {
  const int lo = ka < kb ? ka : kb, d = (ka ^ kb) - 1;
  const uint32_t a = v + (uint32_t)(((lo >> 2) & 1) * n1 * n2 + ((lo >> 1) & 1) * n2 + (lo & 1));
  return b.voff[a / ISO_CHUNK] + b.vpre[a] + (unsigned long long)__popc((uint32_t)b.mask[a] & ((1u << d) - 1u));
}

__device__ __forceinline__ void iso_put_triangle(int32_t* __restrict__ tri, unsigned long long t, unsigned long long max_triangles,
                                                 unsigned long long x, unsigned long long y, unsigned long long z) {
  if (t < max_triangles) {
    tri[3 * t + 0] = (int32_t)x;
    tri[3 * t + 1] = (int32_t)y;
    tri[3 * t + 2] = (int32_t)z;
  }
}

// Emit: one thread per grid point.  Its owned vertices, at the ids voff[chunk] + vpre + the rank of d in its mask, and the triangles
// of its cube from toff[chunk] + tpre on, tetrahedron by tetrahedron.  A tetrahedron with the inside bits s (corner j = bit j):
//   one corner L apart (s has 1 or 3 bits): the vertices on L-X, L-Y, L-Z, X < Y < Z the other corners.  Their normal points away
//     from L exactly when (L, X, Y, Z) is positively oriented in world space: the parity of the permutation (L is moved over L
//     corners), of the tetrahedron's own permutation and the sign of det(m).  It has to point away from L when L is inside.
//   two and two (inside A < B, outside C < D): the quadrilateral AC, AD, BD, BC cut along AC-BD into (AC, AD, BD) and (AC, BD, BC),
//     wound from inside to outside exactly when (A, B, C, D) is positively oriented.
// Nothing is written at or beyond the capacities.
__global__ void __launch_bounds__(ISO_BLOCK) k_iso_emit(const float* __restrict__ f, int n0, int n1, int n2, float iso, int none, IsoAffine aff,
                                                        int det_neg, IsoBufs b, float* __restrict__ vertices, unsigned long long max_vertices,
                                                        int32_t* __restrict__ tri, unsigned long long max_triangles) {
  const uint32_t total = (uint32_t)n0 * (uint32_t)n1 * (uint32_t)n2;
#pragma unroll 1
  for (int i = 0; i < ISO_ITERS; ++i) {
    const uint32_t v = blockIdx.x * ISO_CHUNK + i * ISO_BLOCK + threadIdx.x;
    if (v >= total) continue;
    const uint32_t mask = b.mask[v];
    const IsoCell c = iso_cell(v, n0, n1, n2, none);
    if (mask) {
      unsigned long long id = b.voff[blockIdx.x] + b.vpre[v];
      const double fa = (double)f[v], di = (double)iso;
#pragma unroll
      for (int d = 0; d < 7; ++d) {
        if (!((mask >> d) & 1u)) continue;
        if (id < max_vertices) {
          const int k = d + 1;
          const double fb = (double)f[v + (uint32_t)(((k >> 2) & 1) * n1 * n2 + ((k >> 1) & 1) * n2 + (k & 1))];
          const double t = __dadd_rn(di, -fa) / __dadd_rn(fb, -fa);
          const double q0 = (k & 4) ? __dadd_rn((double)c.i0, t) : (double)c.i0;
          const double q1 = (k & 2) ? __dadd_rn((double)c.i1, t) : (double)c.i1;
          const double q2 = (k & 1) ? __dadd_rn((double)c.i2, t) : (double)c.i2;
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const double* m = aff.m + 4 * r;
            const double w = __dadd_rn(__dadd_rn(__dadd_rn(m[3], __dmul_rn(m[0], q0)), __dmul_rn(m[1], q1)), __dmul_rn(m[2], q2));
            vertices[3 * id + r] = (float)w;
          }
        }
        ++id;
      }
    }
    if (!(c.valid & 0x80u)) continue;
    const uint32_t in = iso_inside(f, v, c.valid, n1, n2, iso);
    if (in == 0u || in == 0xffu) continue;
    unsigned long long t = b.toff[blockIdx.x] + b.tpre[v];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const Kuhn kh = kuhn(p);
      const int s = iso_tet_bits(in, kh.codes), ns = __popc(s);
      if (ns == 0 || ns == 4) continue;
      auto code = [&](int j) { return (kh.codes >> (3 * j)) & 7; };
      if (ns != 2) {
        const int L = __ffs(ns == 1 ? s : (~s & 15)) - 1;
        const int X = L == 0 ? 1 : 0, Y = L <= 1 ? 2 : 1, Z = L == 3 ? 2 : 3;
        const int flip = ((L & 1) ^ kh.neg ^ det_neg) ^ (ns == 3);
        const unsigned long long a = iso_vertex_id(b, v, n1, n2, code(L), code(X));
        const unsigned long long y = iso_vertex_id(b, v, n1, n2, code(L), code(Y));
        const unsigned long long z = iso_vertex_id(b, v, n1, n2, code(L), code(Z));
        iso_put_triangle(tri, t++, max_triangles, a, flip ? z : y, flip ? y : z);
      } else {
        const int o = ~s & 15;
        const int A = __ffs(s) - 1, B = 31 - __clz(s), C = __ffs(o) - 1, D = 31 - __clz(o);
        const int inv = __popc(o & ((1 << A) - 1)) + __popc(o & ((1 << B) - 1));      // pairs (inside, outside) out of order
        const int flip = (inv & 1) ^ kh.neg ^ det_neg;
        const unsigned long long ac = iso_vertex_id(b, v, n1, n2, code(A), code(C)), ad = iso_vertex_id(b, v, n1, n2, code(A), code(D));
        const unsigned long long bd = iso_vertex_id(b, v, n1, n2, code(B), code(D)), bc = iso_vertex_id(b, v, n1, n2, code(B), code(C));
        iso_put_triangle(tri, t++, max_triangles, ac, flip ? bd : ad, flip ? ad : bd);
        iso_put_triangle(tri, t++, max_triangles, ac, flip ? bc : bd, flip ? bd : bc);
      }
    }
  }
}

// ---- afx_mesh_measures: per-workgroup partial sums of the triangles' areas and signed volumes (strided per thread, then a tree),
// then one finishing workgroup - a fixed order.  V and T come from the device record, cut to the capacities; a triangle with an index
// outside [0, V) is skipped, so nothing is read beyond the vertex buffer.
__global__ void __launch_bounds__(MM_BLOCK) k_mm_partial(const float* __restrict__ vertices, const int32_t* __restrict__ tri,
                                                         const unsigned long long* __restrict__ rec, unsigned long long max_vertices,
                                                         unsigned long long max_triangles, double r0, double r1, double r2,
                                                         double* __restrict__ partial) {
  __shared__ double red[2][MM_BLOCK];
  const unsigned long long V = min(rec[ISO_V], max_vertices), T = min(rec[ISO_T], max_triangles);
  double area = 0.0, vol = 0.0;
  for (unsigned long long t = (unsigned long long)blockIdx.x * MM_BLOCK + threadIdx.x; t < T; t += (unsigned long long)gridDim.x * MM_BLOCK) {
    const int32_t ia = tri[3 * t], ib = tri[3 * t + 1], ic = tri[3 * t + 2];
    if (ia < 0 || ib < 0 || ic < 0 || (unsigned long long)ia >= V || (unsigned long long)ib >= V || (unsigned long long)ic >= V) continue;
    const float* pa = vertices + 3 * (size_t)ia;
    const float* pb = vertices + 3 * (size_t)ib;
    const float* pc = vertices + 3 * (size_t)ic;
    const double ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2], cx = pc[0], cy = pc[1], cz = pc[2];
    const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    area += 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
    const double ex = ax - r0, ey = ay - r1, ez = az - r2, fx = bx - r0, fy = by - r1, fz = bz - r2, gx = cx - r0, gy = cy - r1, gz = cz - r2;
    vol += ((ex * (fy * gz - fz * gy) + ey * (fz * gx - fx * gz)) + ez * (fx * gy - fy * gx)) / 6.0;
  }
  red[0][threadIdx.x] = area;
  red[1][threadIdx.x] = vol;
  __syncthreads();
  for (int s = MM_BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = red[0][0];
    partial[MM_MAX_PART + blockIdx.x] = red[1][0];
  }
}

__global__ void __launch_bounds__(MM_BLOCK) k_mm_finish(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
  __shared__ double red[2][MM_BLOCK];
  double area = 0.0, vol = 0.0;
  for (int k = threadIdx.x; k < blocks; k += MM_BLOCK) { area += partial[k]; vol += partial[MM_MAX_PART + k]; }
  red[0][threadIdx.x] = area;
  red[1][threadIdx.x] = vol;
  __syncthreads();
  for (int s = MM_BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = red[0][0]; out[1] = red[1][0]; }
}

}  // namespace

extern "C" size_t afx_isosurface_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2) {
  if (!afx::volume_shape_ok(n0, n1, n2)) return 0;
  afx::Carve c;
  carve_iso(c, n0, n1, n2);
  return c.end;
}

extern "C" int afx_isosurface_3d(const float* f, int32_t n0, int32_t n1, int32_t n2, float iso, const double index_to_world[12], float* vertices,
                                 int64_t max_vertices, int32_t* triangles, int64_t max_triangles, void* record, void* workspace,
                                 size_t workspace_bytes, size_t* workspace_needed, void* stream) {
  const char* who = "afx_isosurface_3d";
  if (!f || !record || !index_to_world) return afx::set_error(AFX_E_INVALID, who, "null volume, record or index_to_world");
  if (!afx::volume_shape_ok(n0, n1, n2)) return afx::set_error(AFX_E_INVALID, who, "need a volume of 1..1024 voxels along each axis");
  if (iso != iso) return afx::set_error(AFX_E_INVALID, who, "iso is NaN");
  if (max_vertices < 0 || max_vertices > INT32_MAX || max_triangles < 0 || max_triangles > INT32_MAX)
    return afx::set_error(AFX_E_INVALID, who, "capacities must lie in 0..2^31 - 1");
  if ((max_vertices > 0 && !vertices) || (max_triangles > 0 && !triangles))
    return afx::set_error(AFX_E_INVALID, who, "a capacity above 0 needs its array");
  IsoAffine aff;
  for (int k = 0; k < 12; ++k) {
    aff.m[k] = index_to_world[k];
    if (!isfinite(aff.m[k])) return afx::set_error(AFX_E_INVALID, who, "index_to_world has a non-finite entry");
  }
  const double* m = aff.m;
  const double det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
  if (!(det != 0.0) || !isfinite(det)) return afx::set_error(AFX_E_INVALID, who, "index_to_world is singular (det(m) is 0 or not finite)");
  const size_t need = afx_isosurface_3d_workspace_bytes(n0, n1, n2);
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(f, "the volume", who)) return rc;
  if (int rc = afx::check_device(record, "the record", who)) return rc;
  if (vertices) if (int rc = afx::check_device(vertices, "vertices", who)) return rc;
  if (triangles) if (int rc = afx::check_device(triangles, "triangles", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  afx::Carve c;
  c.base = (uintptr_t)workspace;
  const IsoBufs b = carve_iso(c, n0, n1, n2);
  const uint32_t total = (uint32_t)n0 * (uint32_t)n1 * (uint32_t)n2;                 // <= 2^30
  const unsigned chunks = (total + ISO_CHUNK - 1) / ISO_CHUNK;
  const int none = n0 == 1 || n1 == 1 || n2 == 1;
  hipLaunchKernelGGL(k_iso_classify, dim3(chunks), dim3(ISO_BLOCK), 0, st, f, (int)n0, (int)n1, (int)n2, iso, none, b);
  hipLaunchKernelGGL(k_iso_scan, dim3(1), dim3(ISO_SCAN), 0, st, b, (uint32_t)chunks, (unsigned long long)max_vertices,
                     (unsigned long long)max_triangles, (unsigned long long*)record);
  if (max_vertices > 0 || max_triangles > 0)
    hipLaunchKernelGGL(k_iso_emit, dim3(chunks), dim3(ISO_BLOCK), 0, st, f, (int)n0, (int)n1, (int)n2, iso, none, aff, (int)(det < 0.0), b,
                       vertices, (unsigned long long)max_vertices, triangles, (unsigned long long)max_triangles);
  return afx::launched(who);
}

extern "C" size_t afx_mesh_measures_workspace_bytes(void) {
  afx::Carve c;
  c.take<double>(2 * (size_t)MM_MAX_PART * sizeof(double));
  return c.end;
}

extern "C" int afx_mesh_measures(const float* vertices, int64_t max_vertices, const int32_t* triangles, int64_t max_triangles, const void* record,
                                 const double ref_point[3], double* out, void* workspace, size_t workspace_bytes, size_t* workspace_needed,
                                 void* stream) {
  const char* who = "afx_mesh_measures";
  if (!record || !out) return afx::set_error(AFX_E_INVALID, who, "null record or output");
  if (max_vertices < 0 || max_vertices > INT32_MAX || max_triangles < 0 || max_triangles > INT32_MAX)
    return afx::set_error(AFX_E_INVALID, who, "capacities must lie in 0..2^31 - 1");
  if ((max_vertices > 0 && !vertices) || (max_triangles > 0 && !triangles))
    return afx::set_error(AFX_E_INVALID, who, "a capacity above 0 needs its array");
  double r[3] = {0.0, 0.0, 0.0};
  if (ref_point)
    for (int k = 0; k < 3; ++k) {
      r[k] = ref_point[k];
      if (!isfinite(r[k])) return afx::set_error(AFX_E_INVALID, who, "ref_point has a non-finite entry");
    }
  const size_t need = afx_mesh_measures_workspace_bytes();
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(record, "the record", who)) return rc;
  if (int rc = afx::check_device(out, "the output", who)) return rc;
  if (vertices) if (int rc = afx::check_device(vertices, "vertices", who)) return rc;
  if (triangles) if (int rc = afx::check_device(triangles, "triangles", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  // without triangles the loops of the partial kernel run zero times whatever the record says (T is cut to the capacity)
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((max_triangles + MM_BLOCK - 1) / MM_BLOCK, MM_MAX_PART));
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(k_mm_partial, dim3(blocks), dim3(MM_BLOCK), 0, st, vertices, triangles, (const unsigned long long*)record,
                     (unsigned long long)max_vertices, (unsigned long long)max_triangles, r[0], r[1], r[2], partial);
  hipLaunchKernelGGL(k_mm_finish, dim3(1), dim3(MM_BLOCK), 0, st, (const double*)partial, blocks, out);
  return afx::launched(who);
}
