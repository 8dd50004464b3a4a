// afx_kernels_graph.hip - the centreline graph of a 3-D mask (afx_centreline_graph) and spur pruning (afx_prune_spurs); the definitions
// stand in include/afx.h.  Every output is a pure function of the input: canonical labels (afx_label_components_3d, called twice through
// its C entry, not copied), paths ordered from a canonical start, integer step counts, fp64 formed from them in a stated order.  Integer
// atomics only (min / add on counters whose result does not depend on the order), nothing allocated or synchronised.
// NOTHING CAN HANG: no thread waits for a value that another thread writes, and every loop runs a number of times the thread holds
// before it enters - the 26 neighbours, CG_ITERS, the chunk counts, and in the walk the branch's own size.
#include "afx_internal.h"
#include "afx_scan.h"
#include <algorithm>
#include <cmath>

// every fp64 product and sum below is rounded on its own (lengths and radius sums are defined operation by operation).  They are written
// as plain * and + under this pragma: __dmul_rn / __dadd_rn are inline functions of a header compiled with contraction allowed, and a
// product and a sum made of them were fused into one fma here.
#pragma clang fp contract(off)

namespace {

constexpr int CG_BLOCK = 256;
constexpr int CG_CHUNK = 2048;                        // consecutive voxels (or branch sizes) per workgroup of the chunked kernels
constexpr int CG_ITERS = CG_CHUNK / CG_BLOCK;
constexpr unsigned CG_WALK_GRID = 1024;               // workgroups of the walk; they stride over the branches
constexpr uint32_t CG_NONE = 0xffffffffu;
constexpr uint32_t CG_INNER = 0x80000000u;            // start key of a voxel that is no extreme (linear indices stay below 2^30)

// slots of the graph record and of a branch row (include/afx.h)
enum { GR_ON = 0, GR_J = 1, GR_P = 2, GR_NODES = 3, GR_BRANCHES = 4, GR_DEG0 = 5, GR_DEG1 = 6, GR_FREE = 7, GR_CYCLES = 8, GR_SPURS = 9,
       GR_LENGTH = 10, GR_STATUS = 11, GR_D2MIN = 12 };
enum { BR_SIZE = 0, BR_FLAGS = 1, BR_NODES = 2, BR_D2 = 3, BR_D2J = 4, BR_COUNTS = 5, BR_LENGTH = 12, BR_RSUM = 13, BR_ENDS = 14 };
enum { PR_ROUNDS = 0, PR_BRANCHES = 1, PR_VOXELS = 2, PR_CONVERGED = 3, PR_REMAINING = 4, PR_INPUT = 5, PR_LAST = 6 };

// 256 bytes of the workspace.  Counters of one graph build (zeroed by k_cg_reset) and, behind them, those of the pruning rounds.
struct CgState {
  unsigned long long steps[13];                       // the step counts of all branches
  unsigned long long cycles, spurs, killed;           // killed: the spurs the pruning rule takes in this build
  uint32_t on, deg0, deg1, nj;
  uint32_t d2min;
  uint32_t gone;                                      // pruning: voxels deleted in this round
  uint32_t input;                                     // pruning: on voxels of the input
};
static_assert(sizeof(CgState) <= 256, "CgState has 256 bytes of the workspace");

struct Lengths { double l[13]; };

__global__ void k_cg_reset(CgState* st) {
  for (int c = 0; c < 13; ++c) st->steps[c] = 0;
  st->cycles = st->spurs = st->killed = 0;
  st->on = st->deg0 = st->deg1 = st->nj = 0;
  st->d2min = CG_NONE;
}

__device__ __forceinline__ void cg_coords(uint32_t v, int s0, int n2, int& i, int& j, int& k) {
  i = (int)(v / (uint32_t)s0);
  const int r = (int)(v - (uint32_t)i * (uint32_t)s0);
  j = r / n2;
  k = r - j * n2;
}

// Classify: deg(v) = the on voxels among v's 26 neighbours (beyond the grid is off); jmask = on and deg >= 3, pmask = on and deg <= 2,
// as 0 / 1 bytes.  The counts take one integer add per wave and counter.
__global__ void __launch_bounds__(CG_BLOCK) k_cg_classify(const uint8_t* __restrict__ skel, int n0, int n1, int n2, uint8_t* __restrict__ jmask,
                                                          uint8_t* __restrict__ pmask, CgState* st) {
  const int s0 = n1 * n2, lane = threadIdx.x & 63;
  const uint32_t total = (uint32_t)n0 * (uint32_t)s0;
  uint32_t on = 0, d0 = 0, d1 = 0, nj = 0;            // of this wave (the same in every lane)
#pragma unroll 1
  for (int it = 0; it < CG_ITERS; ++it) {
    const uint32_t v = blockIdx.x * CG_CHUNK + it * CG_BLOCK + threadIdx.x;
    int deg = -1;                                     // off
    if (v < total && skel[v]) {
      int i, j, k;
      cg_coords(v, s0, n2, i, j, k);
      deg = 0;
#pragma unroll
      for (int di = -1; di <= 1; ++di)
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
          for (int dk = -1; dk <= 1; ++dk) {
            if (di == 0 && dj == 0 && dk == 0) continue;
            const bool inside = i + di >= 0 && i + di < n0 && j + dj >= 0 && j + dj < n1 && k + dk >= 0 && k + dk < n2;
            if (inside && skel[(int)v + di * s0 + dj * n2 + dk]) ++deg;
          }
    }
    if (v < total) {
      jmask[v] = deg >= 3 ? 1 : 0;
      pmask[v] = deg >= 0 && deg <= 2 ? 1 : 0;
    }
    on += (uint32_t)__popcll(__ballot(deg >= 0));
    d0 += (uint32_t)__popcll(__ballot(deg == 0));
    d1 += (uint32_t)__popcll(__ballot(deg == 1));
    nj += (uint32_t)__popcll(__ballot(deg >= 3));
  }
  if (lane == 0) {
    if (on) atomicAdd(&st->on, on);
    if (d0) atomicAdd(&st->deg0, d0);
    if (d1) atomicAdd(&st->deg1, d1);
    if (nj) atomicAdd(&st->nj, nj);
  }
}

// start[b] = CG_NONE for the B branches (B is read from the labelling's record: nothing comes back to the host)
__global__ void __launch_bounds__(CG_BLOCK) k_cg_start_init(const unsigned long long* __restrict__ rec_p, uint32_t total, uint32_t* __restrict__ start) {
  const uint32_t nb = (uint32_t)rec_p[1];             // <= total
#pragma unroll
  for (int it = 0; it < CG_ITERS; ++it) {
    const uint32_t b = blockIdx.x * CG_CHUNK + it * CG_BLOCK + threadIdx.x;
    if (b < nb && b < total) start[b] = CG_NONE;
  }
}

// Terminals: start[b] = min over the branch's voxels of (v for an extreme - fewer than 2 P-neighbours - and v | CG_INNER for the
// others): the smallest extreme where the branch has one, else (a cycle) the smallest voxel with CG_INNER set.
__global__ void __launch_bounds__(CG_BLOCK) k_cg_terminals(const uint8_t* __restrict__ pmask, const int32_t* __restrict__ blab, int n0, int n1,
                                                           int n2, uint32_t* start) {
  const int s0 = n1 * n2;
  const uint32_t total = (uint32_t)n0 * (uint32_t)s0;
  const uint32_t v = blockIdx.x * CG_BLOCK + threadIdx.x;
  if (v >= total || !pmask[v]) return;
  int i, j, k;
  cg_coords(v, s0, n2, i, j, k);
  int np = 0;
#pragma unroll
  for (int di = -1; di <= 1; ++di)
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
      for (int dk = -1; dk <= 1; ++dk) {
        if (di == 0 && dj == 0 && dk == 0) continue;
        const bool inside = i + di >= 0 && i + di < n0 && j + dj >= 0 && j + dj < n1 && k + dk >= 0 && k + dk < n2;
        if (inside && pmask[(int)v + di * s0 + dj * n2 + dk]) ++np;
      }
  const int32_t b = blab[v];                          // 1..B on a P voxel
  if (b > 0) atomicMin(&start[b - 1], np < 2 ? v : (v | CG_INNER));
}

// The exclusive scan of sizes[0..total) (the entries at and beyond B are 0) in three launches: PASS 0 - the sum of every chunk of
// CG_CHUNK entries; k_cg_scan_chunks - one workgroup turns those sums into their own exclusive scan; PASS 1 - offs[i] = the chunk's
// prefix + the entries before i in the chunk (8 consecutive entries per thread, the threads' sums scanned through LDS).
template <int PASS>
__global__ void __launch_bounds__(CG_BLOCK) k_cg_scan(const uint32_t* __restrict__ sizes, uint32_t total, uint32_t* __restrict__ chunk,
                                                      uint32_t* __restrict__ offs) {
  const uint32_t e0 = blockIdx.x * CG_CHUNK + threadIdx.x * CG_ITERS;
  uint32_t x[CG_ITERS], p[1] = {0}, tot[1];
#pragma unroll
  for (int q = 0; q < CG_ITERS; ++q) {
    x[q] = e0 + q < total ? sizes[e0 + q] : 0;
    p[0] += x[q];
  }
  afx::block_exclusive_scan<CG_BLOCK>(p, tot);
  if (PASS == 0) {
    if (threadIdx.x == CG_BLOCK - 1) chunk[blockIdx.x] = tot[0];
    return;
  }
  p[0] += chunk[blockIdx.x];
#pragma unroll
  for (int q = 0; q < CG_ITERS; ++q) {
    if (e0 + q < total) offs[e0 + q] = p[0];
    p[0] += x[q];
  }
}

__global__ void __launch_bounds__(1024) k_cg_scan_chunks(uint32_t* chunk, uint32_t nb) {
  uint32_t b0, b1, p[1] = {0}, tot[1];
  afx::scan_run<1024>(nb, b0, b1);
  for (uint32_t b = b0; b < b1; ++b) p[0] += chunk[b];
  afx::block_exclusive_scan<1024>(p, tot);
  for (uint32_t b = b0; b < b1; ++b) { const uint32_t c = chunk[b]; chunk[b] = p[0]; p[0] += c; }
}

// (((n_0 L_0) + n_1 L_1) + ...) + n_12 L_12, every product and sum rounded on its own
__device__ __forceinline__ double cg_length(const unsigned long long* n, const Lengths& L) {
  double acc = (double)n[0] * L.l[0];
#pragma unroll
  for (int c = 1; c < 13; ++c) {
    const double term = (double)n[c] * L.l[c];
    acc = acc + term;
  }
  return acc;
}

__device__ __forceinline__ unsigned long long cg_wave_sum(unsigned long long x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
  return x;
}

// Walk: one lane per branch, the workgroups striding over the B branches.  The lane starts at start[b] and takes exactly sizes[b]
// steps; each step writes the voxel into path_voxels, looks at the 26 neighbours in the P mask (at most two are on: a < b' in raster
// order) and goes on to the one it did not come from - from a cycle's first voxel to the smaller one.  At the two ends of a path it
// looks at the J mask as well (the attachments).  Step classes are counted in 13 registers (a compare per class, no indexed array).
// kill (pruning; may be NULL): kill[b] = 1 where branch b is a spur with length <= factor sqrt(d2 at its J voxel).
__global__ void __launch_bounds__(CG_BLOCK) k_cg_walk(const uint8_t* __restrict__ jmask, const uint8_t* __restrict__ pmask,
                                                      const int32_t* __restrict__ jlab, const uint32_t* __restrict__ d2, int n0, int n1, int n2,
                                                      const unsigned long long* __restrict__ rec_p, const uint32_t* __restrict__ sizes,
                                                      const uint32_t* __restrict__ offs, const uint32_t* __restrict__ start, const Lengths L,
                                                      int32_t* __restrict__ path, unsigned long long* __restrict__ rows, uint32_t max_rows,
                                                      uint8_t* __restrict__ kill, double factor, CgState* st) {
  const int s0 = n1 * n2, lane = threadIdx.x & 63;
  const uint32_t total = (uint32_t)n0 * (uint32_t)s0;
  const uint32_t nb = min((uint32_t)rec_p[1], total);
  unsigned long long tot[13], n_cyc = 0, n_spur = 0, n_kill = 0;
#pragma unroll
  for (int c = 0; c < 13; ++c) tot[c] = 0;
  uint32_t gmin = CG_NONE;
  for (uint32_t b0 = blockIdx.x * CG_BLOCK; b0 < nb; b0 += gridDim.x * CG_BLOCK) {      // the same trip count in every lane of the workgroup
    const uint32_t b = b0 + threadIdx.x;
    if (b >= nb) continue;
    const uint32_t n = sizes[b], off = offs[b], key = start[b];
    const bool cyc = (key & CG_INNER) != 0;
    const uint32_t first = key & ~CG_INNER;
    if (n == 0 || key == CG_NONE || first >= total || (unsigned long long)off + n > total) continue;      // cannot happen; keeps every access inside
    unsigned long long cnt[13];
#pragma unroll
    for (int c = 0; c < 13; ++c) cnt[c] = 0;
    uint32_t cur = first, prev = CG_NONE, last = first;
    uint32_t dmin = CG_NONE, dmax = 0, argmin = 0, node_a = 0, node_b = 0, d2_a = 0, d2_b = 0, att = 0;
    double rsum = 0.0;
    for (uint32_t t = 0; t < n; ++t) {
      path[off + t] = (int32_t)cur;
      last = cur;
      if (d2) {
        const uint32_t d = d2[cur];
        if (d < dmin) { dmin = d; argmin = t; }
        dmax = d > dmax ? d : dmax;
        rsum = rsum + __dsqrt_rn((double)d);
      }
      int i, j, k;
      cg_coords(cur, s0, n2, i, j, k);
      const bool at_end = !cyc && (t == 0 || t == n - 1);
      uint32_t pa = CG_NONE, pb = CG_NONE, ja = CG_NONE, jb = CG_NONE;
      int ca = 0, cb = 0, cja = 0, cjb = 0, cclose = -1;
#pragma unroll
      for (int di = -1; di <= 1; ++di)
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
          for (int dk = -1; dk <= 1; ++dk) {
            if (di == 0 && dj == 0 && dk == 0) continue;
            const bool inside = i + di >= 0 && i + di < n0 && j + dj >= 0 && j + dj < n1 && k + dk >= 0 && k + dk < n2;
            if (!inside) continue;
            const int code = (di + 1) * 9 + (dj + 1) * 3 + (dk + 1);
            const int cls = code > 13 ? code - 14 : 12 - code;
            const uint32_t u = (uint32_t)((int)cur + di * s0 + dj * n2 + dk);
            if (pmask[u]) {
              if (pa == CG_NONE) { pa = u; ca = cls; }
              else if (pb == CG_NONE) { pb = u; cb = cls; }
              if (u == first) cclose = cls;
            } else if (at_end && jmask[u]) {
              if (ja == CG_NONE) { ja = u; cja = cls; }
              else if (jb == CG_NONE) { jb = u; cjb = cls; }
            }
          }
      if (at_end) {                                   // attachments: the link's class, the node and the radius at the J voxel
        if (n == 1) {
          if (ja != CG_NONE) { node_a = (uint32_t)jlab[ja]; d2_a = d2 ? d2[ja] : 0; ++att; }
          if (jb != CG_NONE) { node_b = (uint32_t)jlab[jb]; d2_b = d2 ? d2[jb] : 0; ++att; }
        } else if (ja != CG_NONE) {
          if (t == 0) { node_a = (uint32_t)jlab[ja]; d2_a = d2 ? d2[ja] : 0; }
          else { node_b = (uint32_t)jlab[ja]; d2_b = d2 ? d2[ja] : 0; }
          ++att;
          jb = CG_NONE;
        }
#pragma unroll
        for (int c = 0; c < 13; ++c) cnt[c] += (ja != CG_NONE && cja == c) + (jb != CG_NONE && cjb == c);
      }
      int cstep = -1;
      uint32_t nxt = CG_NONE;
      if (t + 1 < n) {                                // the step to the next voxel of the path
        if (pa != CG_NONE && pa != prev) { nxt = pa; cstep = ca; }
        else { nxt = pb; cstep = cb; }
      } else if (cyc) cstep = cclose;                 // the closing step of a cycle
#pragma unroll
      for (int c = 0; c < 13; ++c) cnt[c] += cstep == c;
      if (t + 1 < n) {
        if (nxt == CG_NONE) break;                    // cannot happen in a component of P; never step outside the volume
        prev = cur;
        cur = nxt;
      }
    }
    const uint32_t free_ends = (cyc ? 0u : 2u) - att;
    const bool spur = free_ends == 1 && att == 1;
    const double len = cg_length(cnt, L);
    bool dead = false;
    if (kill) {
      dead = spur && len <= factor * __dsqrt_rn((double)(node_a ? d2_a : d2_b));
      kill[b] = dead ? 1 : 0;
    }
    if (b < max_rows) {
      unsigned long long* r = rows + (size_t)b * AFX_GRAPH_BRANCH_SLOTS;
      r[BR_SIZE] = (unsigned long long)n | ((unsigned long long)off << 32);
      r[BR_FLAGS] = (unsigned long long)((cyc ? 1u : 0u) | (spur ? 2u : 0u) | (free_ends << 8) | (att << 16)) | ((unsigned long long)argmin << 32);
      r[BR_NODES] = (unsigned long long)node_a | ((unsigned long long)node_b << 32);
      r[BR_D2] = d2 ? (unsigned long long)dmin | ((unsigned long long)dmax << 32) : 0ull;
      r[BR_D2J] = (unsigned long long)d2_a | ((unsigned long long)d2_b << 32);
#pragma unroll
      for (int q = 0; q < 7; ++q) r[BR_COUNTS + q] = cnt[2 * q] | (q < 6 ? cnt[2 * q + 1] << 32 : 0ull);
      r[BR_LENGTH] = (unsigned long long)__double_as_longlong(len);
      r[BR_RSUM] = (unsigned long long)__double_as_longlong(rsum);
      r[BR_ENDS] = (unsigned long long)first | ((unsigned long long)last << 32);
      r[15] = 0;
    }
#pragma unroll
    for (int c = 0; c < 13; ++c) tot[c] += cnt[c];
    n_cyc += cyc;
    n_spur += spur;
    n_kill += dead;
    gmin = dmin < gmin ? dmin : gmin;
  }
  // every lane of the workgroup arrives here: one integer add per wave and counter
#pragma unroll
  for (int c = 0; c < 13; ++c) {
    const unsigned long long s = cg_wave_sum(tot[c]);
    if (lane == 0 && s) atomicAdd(&st->steps[c], s);
  }
  n_cyc = cg_wave_sum(n_cyc);
  n_spur = cg_wave_sum(n_spur);
  n_kill = cg_wave_sum(n_kill);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) gmin = min(gmin, (uint32_t)__shfl_xor(gmin, d));
  if (lane == 0) {
    if (n_cyc) atomicAdd(&st->cycles, n_cyc);
    if (n_spur) atomicAdd(&st->spurs, n_spur);
    if (n_kill) atomicAdd(&st->killed, n_kill);
    if (gmin != CG_NONE) atomicMin(&st->d2min, gmin);
  }
}

// one lane: the record
__global__ void k_cg_finish(const CgState* st, const unsigned long long* __restrict__ rec_j, const unsigned long long* __restrict__ rec_p,
                            const Lengths L, uint32_t max_rows, int has_d2, unsigned long long* __restrict__ record) {
  record[GR_ON] = st->on;
  record[GR_J] = st->nj;
  record[GR_P] = st->on - st->nj;
  record[GR_NODES] = rec_j[1];
  record[GR_BRANCHES] = rec_p[1];
  record[GR_DEG0] = st->deg0;
  record[GR_DEG1] = st->deg1;
  record[GR_FREE] = (unsigned long long)st->deg1 + 2ull * st->deg0;
  record[GR_CYCLES] = st->cycles;
  record[GR_SPURS] = st->spurs;
  record[GR_LENGTH] = (unsigned long long)__double_as_longlong(cg_length(st->steps, L));
  record[GR_STATUS] = rec_p[1] > max_rows ? 1 : 0;
  record[GR_D2MIN] = has_d2 ? st->d2min : CG_NONE;
  for (int q = GR_D2MIN + 1; q < AFX_GRAPH_RECORD_SLOTS; ++q) record[q] = 0;
}

// ---- pruning
__global__ void k_pr_reset(CgState* st, unsigned long long* record) {
  st->gone = st->input = 0;
  for (int q = 0; q < AFX_PRUNE_RECORD_SLOTS; ++q) record[q] = 0;
}

// out = (skel != 0) as 0 / 1 (out may be skel: every thread reads and writes its own voxels), the on voxels counted once per wave
__global__ void __launch_bounds__(CG_BLOCK) k_pr_init(const uint8_t* skel, uint32_t total, uint8_t* out, CgState* st) {
  uint32_t n = 0;
#pragma unroll
  for (int it = 0; it < CG_ITERS; ++it) {
    const uint32_t v = blockIdx.x * CG_CHUNK + it * CG_BLOCK + threadIdx.x;
    const bool on = v < total && skel[v] != 0;
    if (v < total) out[v] = on ? 1 : 0;
    n += (uint32_t)__popcll(__ballot(on));
  }
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&st->input, n);
}

// Delete: the voxels of the branches the walk marked, all together.  J voxels carry no branch label and stay.
__global__ void __launch_bounds__(CG_BLOCK) k_pr_delete(const int32_t* __restrict__ blab, const uint8_t* __restrict__ kill, uint32_t total,
                                                        const unsigned long long* __restrict__ record, uint8_t* __restrict__ out, CgState* st) {
  if (record[PR_CONVERGED]) return;
  uint32_t n = 0;
#pragma unroll
  for (int it = 0; it < CG_ITERS; ++it) {
    const uint32_t v = blockIdx.x * CG_CHUNK + it * CG_BLOCK + threadIdx.x;
    bool dead = false;
    if (v < total) {
      const int32_t b = blab[v];
      dead = b > 0 && kill[b - 1];
      if (dead) out[v] = 0;
    }
    n += (uint32_t)__popcll(__ballot(dead));
  }
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&st->gone, n);
}

// One lane: the round is over.  A round that deleted nothing sets converged; the record then stands, whatever later rounds are issued
// (they find the same graph, mark the same nothing, and k_pr_delete returns at once).
__global__ void k_pr_advance(CgState* st, unsigned long long* record) {
  if (!record[PR_CONVERGED]) {
    const unsigned long long d = st->gone;
    record[PR_ROUNDS] += 1;
    record[PR_BRANCHES] += d ? st->killed : 0;
    record[PR_VOXELS] += d;
    record[PR_LAST] = d;
    record[PR_INPUT] = st->input;
    record[PR_REMAINING] = st->input - record[PR_VOXELS];
    if (d == 0) record[PR_CONVERGED] = 1;
  }
  st->gone = 0;
}

// The labelling's workspace is free once the second labelling has finished: start[] and offs[] lie in it.
struct CgBufs { uint8_t* jmask; uint8_t* pmask; uint32_t* sizes; char* shared; size_t shared_bytes; uint32_t* start; uint32_t* offs; uint32_t* chunk;
                unsigned long long* rec_j; unsigned long long* rec_p; CgState* st; };
CgBufs carve_graph(afx::Carve& c, int32_t n0, int32_t n1, int32_t n2) {
  const size_t n = (size_t)n0 * n1 * n2;
  CgBufs b;
  b.jmask = c.take<uint8_t>(n);
  b.pmask = c.take<uint8_t>(n);
  b.sizes = c.take<uint32_t>(n * sizeof(uint32_t));
  afx::Carve two;
  two.take<uint32_t>(n * sizeof(uint32_t));
  two.take<uint32_t>(n * sizeof(uint32_t));
  b.shared_bytes = std::max(afx_label_components_3d_workspace_bytes(n0, n1, n2), two.end);
  b.shared = c.take<char>(b.shared_bytes);
  afx::Carve in;
  in.base = (uintptr_t)b.shared;
  b.start = in.take<uint32_t>(n * sizeof(uint32_t));
  b.offs = in.take<uint32_t>(n * sizeof(uint32_t));
  b.chunk = c.take<uint32_t>((n + CG_CHUNK - 1) / CG_CHUNK * sizeof(uint32_t));
  b.rec_j = c.take<unsigned long long>(256);
  b.rec_p = c.take<unsigned long long>(256);
  b.st = c.take<CgState>(256);
  return b;
}

struct PrBufs { CgBufs g; int32_t* jlab; int32_t* blab; int32_t* path; uint8_t* kill; unsigned long long* rec_g; };
PrBufs carve_prune(afx::Carve& c, int32_t n0, int32_t n1, int32_t n2) {
  const size_t n = (size_t)n0 * n1 * n2;
  PrBufs b;
  b.g = carve_graph(c, n0, n1, n2);
  b.jlab = c.take<int32_t>(n * sizeof(int32_t));
  b.blab = c.take<int32_t>(n * sizeof(int32_t));
  b.path = c.take<int32_t>(n * sizeof(int32_t));
  b.kill = c.take<uint8_t>(n);
  b.rec_g = c.take<unsigned long long>(256);
  return b;
}

Lengths cg_lengths(const double* step_lengths) {
  Lengths L;
  for (int c = 0; c < 13; ++c) {
    const int code = c + 14, nz = (code / 9 != 1) + (code / 3 % 3 != 1) + (code % 3 != 1);
    L.l[c] = step_lengths ? step_lengths[c] : std::sqrt((double)nz);
  }
  return L;
}

// The launch sequence of one graph build, arguments checked by the callers.
int graph_launch(const uint8_t* skel, const uint32_t* d2, int32_t n0, int32_t n1, int32_t n2, const Lengths& L, int32_t* jlab, int32_t* blab,
                 int32_t* path, unsigned long long* rows, uint32_t max_rows, unsigned long long* record, const CgBufs& b, uint8_t* kill,
                 double factor, hipStream_t st, const char* who) {
  const uint32_t total = (uint32_t)n0 * (uint32_t)n1 * (uint32_t)n2;                 // <= 2^30
  const unsigned chunks = (total + CG_CHUNK - 1) / CG_CHUNK, blocks = (total + CG_BLOCK - 1) / CG_BLOCK;
  hipLaunchKernelGGL(k_cg_reset, dim3(1), dim3(1), 0, st, b.st);
  hipLaunchKernelGGL(k_cg_classify, dim3(chunks), dim3(CG_BLOCK), 0, st, skel, (int)n0, (int)n1, (int)n2, b.jmask, b.pmask, b.st);
  if (int rc = afx_label_components_3d(b.jmask, n0, n1, n2, 3, jlab, nullptr, b.rec_j, b.shared, b.shared_bytes, nullptr, st)) return rc;
  if (int rc = afx_label_components_3d(b.pmask, n0, n1, n2, 3, blab, b.sizes, b.rec_p, b.shared, b.shared_bytes, nullptr, st)) return rc;
  hipLaunchKernelGGL(k_cg_start_init, dim3(chunks), dim3(CG_BLOCK), 0, st, (const unsigned long long*)b.rec_p, total, b.start);
  hipLaunchKernelGGL(k_cg_terminals, dim3(blocks), dim3(CG_BLOCK), 0, st, (const uint8_t*)b.pmask, (const int32_t*)blab, (int)n0, (int)n1, (int)n2,
                     b.start);
  hipLaunchKernelGGL(k_cg_scan<0>, dim3(chunks), dim3(CG_BLOCK), 0, st, (const uint32_t*)b.sizes, total, b.chunk, b.offs);
  hipLaunchKernelGGL(k_cg_scan_chunks, dim3(1), dim3(1024), 0, st, b.chunk, (uint32_t)chunks);
  hipLaunchKernelGGL(k_cg_scan<1>, dim3(chunks), dim3(CG_BLOCK), 0, st, (const uint32_t*)b.sizes, total, b.chunk, b.offs);
  hipLaunchKernelGGL(k_cg_walk, dim3(std::min(blocks, CG_WALK_GRID)), dim3(CG_BLOCK), 0, st, (const uint8_t*)b.jmask, (const uint8_t*)b.pmask,
                     (const int32_t*)jlab, d2, (int)n0, (int)n1, (int)n2, (const unsigned long long*)b.rec_p, (const uint32_t*)b.sizes,
                     (const uint32_t*)b.offs, (const uint32_t*)b.start, L, path, rows, max_rows, kill, factor, b.st);
  hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(1), 0, st, (const CgState*)b.st, (const unsigned long long*)b.rec_j,
                     (const unsigned long long*)b.rec_p, L, max_rows, (int)(d2 != nullptr), record);
  return afx::launched(who);
}

}  // namespace

extern "C" size_t afx_centreline_graph_workspace_bytes(int32_t n0, int32_t n1, int32_t n2) {
  if (!afx::volume_shape_ok(n0, n1, n2)) return 0;
  afx::Carve c;
  carve_graph(c, n0, n1, n2);
  return c.end;
}

extern "C" int afx_centreline_graph(const uint8_t* skel, const uint32_t* d2, int32_t n0, int32_t n1, int32_t n2, const double* step_lengths,
                                    int32_t* node_labels, int32_t* branch_labels, int32_t* path_voxels, void* branches, int64_t max_branches,
                                    void* record, void* workspace, size_t workspace_bytes, size_t* workspace_needed, void* stream) {
  const char* who = "afx_centreline_graph";
  if (!skel || !node_labels || !branch_labels || !path_voxels || !record)
    return afx::set_error(AFX_E_INVALID, who, "null mask, node labels, branch labels, path voxels or record");
  if (!afx::volume_shape_ok(n0, n1, n2)) return afx::set_error(AFX_E_INVALID, who, "need a volume of 1..1024 voxels along each axis");
  if (max_branches < 0 || max_branches > 0x7fffffff || (max_branches > 0 && !branches))
    return afx::set_error(AFX_E_INVALID, who, "max_branches must lie in 0..2^31 - 1 and be 0 when there is no branch table");
  if (step_lengths)
    for (int c = 0; c < 13; ++c)
      if (!(step_lengths[c] >= 0.0) || std::isinf(step_lengths[c])) return afx::set_error(AFX_E_INVALID, who, "step_lengths must be finite and >= 0");
  const size_t need = afx_centreline_graph_workspace_bytes(n0, n1, n2);
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(skel, "the mask", who)) return rc;
  if (int rc = afx::check_device(path_voxels, "path_voxels", who)) return rc;
  afx::Carve c;
  c.base = (uintptr_t)workspace;
  const CgBufs b = carve_graph(c, n0, n1, n2);
  return graph_launch(skel, d2, n0, n1, n2, cg_lengths(step_lengths), node_labels, branch_labels, path_voxels, (unsigned long long*)branches,
                      (uint32_t)max_branches, (unsigned long long*)record, b, nullptr, 0.0, (hipStream_t)stream, who);
}

extern "C" size_t afx_prune_spurs_workspace_bytes(int32_t n0, int32_t n1, int32_t n2) {
  if (!afx::volume_shape_ok(n0, n1, n2)) return 0;
  afx::Carve c;
  carve_prune(c, n0, n1, n2);
  return c.end;
}

extern "C" int afx_prune_spurs(const uint8_t* skel, const uint32_t* d2, int32_t n0, int32_t n1, int32_t n2, double factor, int32_t max_rounds,
                               int32_t sync_every, uint8_t* out, void* record, void* workspace, size_t workspace_bytes, size_t* workspace_needed,
                               void* stream) {
  const char* who = "afx_prune_spurs";
  if (!skel || !d2 || !out || !record) return afx::set_error(AFX_E_INVALID, who, "null mask, squared distances, output or record");
  if (!afx::volume_shape_ok(n0, n1, n2)) return afx::set_error(AFX_E_INVALID, who, "need a volume of 1..1024 voxels along each axis");
  if (!(factor >= 0.0) || std::isinf(factor)) return afx::set_error(AFX_E_INVALID, who, "factor must be finite and >= 0");
  if (max_rounds < 1) return afx::set_error(AFX_E_INVALID, who, "max_rounds must be at least 1");
  if (sync_every < 0) return afx::set_error(AFX_E_INVALID, who, "sync_every must be 0 (no read-back) or the rounds between two read-backs");
  const size_t need = afx_prune_spurs_workspace_bytes(n0, n1, n2);
  if (workspace_needed) *workspace_needed = need;
  if (int rc = afx::check_workspace(workspace, workspace_bytes, need, who)) return rc;
  if (int rc = afx::check_device(skel, "the mask", who)) return rc;
  if (int rc = afx::check_device(out, "the output mask", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  afx::Carve c;
  c.base = (uintptr_t)workspace;
  const PrBufs b = carve_prune(c, n0, n1, n2);
  unsigned long long* rec = (unsigned long long*)record;
  const uint32_t total = (uint32_t)n0 * (uint32_t)n1 * (uint32_t)n2;
  const unsigned chunks = (total + CG_CHUNK - 1) / CG_CHUNK;
  const Lengths L = cg_lengths(nullptr);
  hipLaunchKernelGGL(k_pr_reset, dim3(1), dim3(1), 0, st, b.g.st, rec);
  hipLaunchKernelGGL(k_pr_init, dim3(chunks), dim3(CG_BLOCK), 0, st, skel, total, out, b.g.st);
  for (int32_t r = 1; r <= max_rounds; ++r) {
    if (int rc = graph_launch(out, d2, n0, n1, n2, L, b.jlab, b.blab, b.path, nullptr, 0, b.rec_g, b.g, b.kill, factor, st, who)) return rc;
    hipLaunchKernelGGL(k_pr_delete, dim3(chunks), dim3(CG_BLOCK), 0, st, (const int32_t*)b.blab, (const uint8_t*)b.kill, total,
                       (const unsigned long long*)rec, out, b.g.st);
    hipLaunchKernelGGL(k_pr_advance, dim3(1), dim3(1), 0, st, b.g.st, rec);
    if (sync_every > 0 && (r % sync_every == 0 || r == max_rounds)) {
      if (int rc = afx::launched(who)) return rc;
      unsigned long long converged = 0;
      hipError_t e = hipMemcpyAsync(&converged, rec + PR_CONVERGED, sizeof converged, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) return afx::set_error(AFX_E_HIP, who, hipGetErrorString(e));
      if (converged) return AFX_OK;
    }
  }
  if (sync_every > 0)                                 // not a failure: the mask after max_rounds rounds and a record that says converged = 0
    return afx::set_error(AFX_OK, who, "stopped at max_rounds before a round deleted nothing: the record's converged slot is 0");
  return afx::launched(who);
}
