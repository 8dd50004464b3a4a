// afx_kernels_grid.hip — occupancy-grid acceleration of the reference's training loop as gfx950 kernels
// (nerf/run_nerf_acc.py:196-198,284-287; nerf/nerf_helpers_acc.py:10-31,65-78), a device ray sampler
// (nerf/nerf_helpers.py:137-150) and the counter-based generator both use in "perf mode".
//
// The reference delegates the grid and the march to nerfacc 0.3.x (CUDA, neither vendored nor pinned: absent here), so
// what is implemented is that package's PUBLISHED algorithm, restated in oracle/angio_oracle.py for the tests — parity
// unpinned at that third-party boundary.  All of this is HBM/latency-bound integer and fp32 work: one thread per ray or
// per cell, coalesced reads, no MFMA.  The MLP evaluations between the kernels (occupancy of jittered cell points,
// alpha of the candidate samples) are afx_mlp_infer launches on the points these kernels emit.
//
// Float arithmetic that decides an INDEX (cell of a point, number of steps of a ray) is written with explicit
// round-to-nearest single operations in the order of the torch expressions it restates, so that indices are bit-exact.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "afx_scan.h"

namespace afx {

// ---------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. 2011): counter-based, so "perf mode" randomness needs no state buffer and no ordering:
// value i of stream (seed, offset) is a pure function.  u in [0,1): top 24 bits.
// ---------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// uniform [0,1) number `i` of stream (seed, stream id)
__host__ __device__ __forceinline__ float philox_uniform(uint64_t seed, uint64_t stream, uint64_t i) {
  uint32_t o[4];
  philox4x32_10((uint32_t)(i >> 2), (uint32_t)(i >> 34), (uint32_t)stream, (uint32_t)(stream >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), o);
  return (float)(o[i & 3] >> 8) * (1.0f / 16777216.0f);
}

struct GridDesc {
  float lo[3], hi[3];      // roi_aabb
  int32_t res[3];
};

// cell of a world point: u = (p - lo) / (hi - lo); inside <=> 0 <= u < 1 on every axis; ijk = min(floor(u * res), res - 1)
__device__ __forceinline__ bool grid_cell(const GridDesc& g, float px, float py, float pz, int64_t& idx) {
  const float p[3] = {px, py, pz};
  int ijk[3];
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float u = __fdiv_rn(__fsub_rn(p[a], g.lo[a]), __fsub_rn(g.hi[a], g.lo[a]));
    inside = inside && (u >= 0.f) && (u < 1.f);
    int c = (int)floorf(__fmul_rn(u, (float)g.res[a]));
    c = c < 0 ? 0 : c;
    ijk[a] = c > g.res[a] - 1 ? g.res[a] - 1 : c;
  }
  idx = ((int64_t)ijk[0] * g.res[1] + ijk[1]) * g.res[2] + ijk[2];
  return inside;
}

// One fp32 operation, rounded on its own.  HIP's __fadd_rn / __fmul_rn are plain operators inside header functions that allow contraction, and
// hipcc fuses __fadd_rn(__fmul_rn(a, b), c) into one fma; these carry the contraction-off pragma in their own bodies, so a product formed by
// mul_rn reaches the following add_rn already rounded.
__device__ __forceinline__ float add_rn(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}
__device__ __forceinline__ float sub_rn(float x, float y) {
#pragma clang fp contract(off)
  return x - y;
}
__device__ __forceinline__ float mul_rn(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}

// --- OccupancyGrid._update, step 1: one jittered world point per selected cell -----------------------------------
// cell_idx == nullptr: all cells (cell i).  jitter [n,3] in [0,1) (parity mode) or nullptr: Philox(seed, stream 3*?).
// afx_grid_refresh: count_dev bounds the work of a launch sized for the capacity n, and the stream id is stream | *step_dev, the training
// step read on the device (a replayed graph does not freeze it).  Both null: the host's n and stream.
__global__ void k_grid_points(const int32_t* cell_idx, int64_t n, const float* jitter, uint64_t seed, uint64_t stream, GridDesc g, float* pts,
                              const int64_t* count_dev = nullptr, const int64_t* step_dev = nullptr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (count_dev && i >= *count_dev)) return;
  if (step_dev) stream |= (uint64_t)*step_dev;
  const int64_t c = cell_idx ? cell_idx[i] : i;
  const int k = (int)(c % g.res[2]);
  const int j = (int)((c / g.res[2]) % g.res[1]);
  const int ii = (int)(c / ((int64_t)g.res[2] * g.res[1]));
  const int ijk[3] = {ii, j, k};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float u = jitter ? jitter[3 * i + a] : philox_uniform(seed, stream, 3 * (uint64_t)i + a);
    // x = (coords + u) / resolution; x * (hi - lo) + lo, the product and the sum rounded separately as in the torch expression
    const float x = __fdiv_rn(add_rn((float)ijk[a], u), (float)g.res[a]);
    pts[3 * i + a] = add_rn(mul_rn(x, sub_rn(g.hi[a], g.lo[a])), g.lo[a]);
  }
}

// --- step 2: occs[c] = max(occs[c] * decay, occ).  Two passes so that a cell drawn twice gets max(old * decay, occ_a, occ_b)
// whatever the order: (i) every selected cell drops to its decayed value, formed from a snapshot of the values BEFORE the
// update (idempotent under duplicates); (ii) an integer atomicMax on the bit patterns of the non-negative floats folds
// the new occupancies in - order-independent, so the result is deterministic.  (count_dev: as in k_grid_points.)
__global__ void k_grid_decay(float* occs, const float* occs_before, const int32_t* cell_idx, int64_t n, float decay, const int64_t* count_dev = nullptr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (count_dev && i >= *count_dev)) return;
  const int64_t c = cell_idx ? cell_idx[i] : i;
  occs[c] = fmaxf(__fmul_rn(occs_before[c], decay), 0.f);
}
__global__ void k_grid_ema(float* occs, const int32_t* cell_idx, const float* occ_new, int64_t n, const int64_t* count_dev = nullptr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (count_dev && i >= *count_dev)) return;
  const int64_t c = cell_idx ? cell_idx[i] : i;
  const float v = occ_new[i];
  if (v > 0.f) atomicMax((unsigned int*)(occs + c), __float_as_uint(v));
}

// --- step 3: binary = occs > min(mean(occs), occ_thre); also the packed bitfield the march reads ------------------------
// fixed-order two-level sum (deterministic): partial[b] = sum of block b's slice in a tree of fixed shape
__global__ void __launch_bounds__(256) k_grid_sum(const float* occs, int64_t n, double* partial) {
  __shared__ double red[256];
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t b0 = (int64_t)blockIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
  double s = 0.0;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) s += (double)occs[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ void k_grid_binarize(const float* occs, int64_t n, const double* partial, int n_partial, float occ_thre, uint8_t* binary, uint32_t* bits) {
  double tot = 0.0;
  for (int i = 0; i < n_partial; ++i) tot += partial[i];
  const float mean = (float)(tot / (double)n);
  const float thr = mean < occ_thre ? mean : occ_thre;
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;        // one 32-cell word per thread
  if (w * 32 >= n) return;
  uint32_t word = 0;
  for (int b = 0; b < 32; ++b) {
    const int64_t c = w * 32 + b;
    if (c >= n) break;
    const bool on = occs[c] > thr;
    binary[c] = on ? 1 : 0;
    word |= (on ? 1u : 0u) << b;
  }
  bits[w] = word;
}

// bitfield of a byte mask that did not come out of k_grid_binarize (a restored grid): bits[w] bit b = binary[32 w + b] != 0
__global__ void k_grid_pack(const uint8_t* binary, int64_t n, uint32_t* bits) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w * 32 >= n) return;
  uint32_t word = 0;
  for (int b = 0; b < 32; ++b) {
    const int64_t c = w * 32 + b;
    if (c >= n) break;
    word |= (binary[c] ? 1u : 0u) << b;
  }
  bits[w] = word;
}

// --- the cells of a post-warm-up refresh, drawn on the device (afx_grid_select_cells; the draw rule is written in include/afx.h) ---------------
// nerfacc draws n = num_cells / 4 uniform cells and n among the occupied ones (all of them, in index order, when there are at most n).  The
// occupied cells are read from the packed bitfield the march reads: k_grid_occ_count counts the set bits per word and forms per-workgroup word
// prefixes, k_grid_occ_scan scans the workgroup totals (a few hundred at 128^3) and posts n_occ and the selected count n + min(n, n_occ), and
// k_grid_select maps draw i to its cell (block by binary search over the block prefixes, word by binary search over the word prefixes, then the
// set bit inside the word).  Nothing leaves the device.
constexpr int SEL_WORDS = 256;      // bitfield words per workgroup of k_grid_occ_count (one per thread)

// top 24 bits of number i of stream (seed, stream id): philox_uniform's u = philox_u24 / 2^24
__host__ __device__ __forceinline__ uint32_t philox_u24(uint64_t seed, uint64_t stream, uint64_t i) {
  uint32_t o[4];
  philox4x32_10((uint32_t)(i >> 2), (uint32_t)(i >> 34), (uint32_t)stream, (uint32_t)(stream >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), o);
  return o[i & 3] >> 8;
}
// word w of the bitfield with the bits past the last cell cleared
__device__ __forceinline__ uint32_t grid_word(const uint32_t* bits, int64_t w, int64_t n_cells) {
  uint32_t v = bits[w];
  const int64_t rem = n_cells - w * 32;
  if (rem < 32) v &= (1u << rem) - 1u;
  return v;
}
// word_pre[w]: set bits in the words of w's workgroup before w; block_tot[b]: set bits in workgroup b's SEL_WORDS words
__global__ void __launch_bounds__(256) k_grid_occ_count(const uint32_t* bits, int64_t n_cells, int64_t n_words, int32_t* word_pre, int32_t* block_tot) {
  const int64_t w = (int64_t)blockIdx.x * SEL_WORDS + threadIdx.x;
  int32_t c[1] = {w < n_words ? (int32_t)__popc(grid_word(bits, w, n_cells)) : 0}, tot[1];
  block_exclusive_scan<256>(c, tot);
  if (w < n_words) word_pre[w] = c[0];
  if (threadIdx.x == 255) block_tot[blockIdx.x] = tot[0];
}
// one workgroup: block_pre = exclusive scan of block_tot[nb]; n_occ[0] = the total, count[0] = n_draw + min(n_draw, total)
__global__ void __launch_bounds__(1024) k_grid_occ_scan(const int32_t* block_tot, int64_t nb, int32_t* block_pre, int64_t n_draw, int64_t* n_occ,
                                                         int64_t* count) {
  int64_t b0, b1, p[1] = {0}, tot[1];
  scan_run<1024>(nb, b0, b1);
  for (int64_t b = b0; b < b1; ++b) p[0] += block_tot[b];
  block_exclusive_scan<1024>(p, tot);
  for (int64_t b = b0; b < b1; ++b) { block_pre[b] = (int32_t)p[0]; p[0] += block_tot[b]; }
  if (threadIdx.x == 1023) {
    *n_occ = tot[0];
    *count = n_draw + (n_draw < tot[0] ? n_draw : tot[0]);
  }
}
// cells[i], i < n_draw: the uniform draw ((u24 * num_cells) >> 24); i = n_draw + j: the occupied cell of rank (u24 * n_occ) >> 24 when n_draw < n_occ,
// else of rank j (j < n_occ; the slots behind the count are not written).  u24 = philox_u24(seed, stream | *step_dev, i).
__global__ void k_grid_select(const uint32_t* bits, int64_t n_cells, int64_t n_words, const int32_t* word_pre, const int32_t* block_pre, int64_t nb,
                              int64_t n_draw, uint64_t seed, uint64_t stream, const int64_t* step_dev, const int64_t* n_occ_dev, int32_t* cells) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * n_draw) return;
  if (step_dev) stream |= (uint64_t)*step_dev;
  if (i < n_draw) {
    cells[i] = (int32_t)(((uint64_t)philox_u24(seed, stream, (uint64_t)i) * (uint64_t)n_cells) >> 24);
    return;
  }
  const int64_t j = i - n_draw, n_occ = *n_occ_dev;
  int64_t k;
  if (n_draw < n_occ) k = (int64_t)(((uint64_t)philox_u24(seed, stream, (uint64_t)i) * (uint64_t)n_occ) >> 24);
  else if (j < n_occ) k = j;
  else return;
  int64_t lo = 0, hi = nb - 1;              // the last workgroup whose prefix is <= k holds the k-th set bit
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (block_pre[mid] <= k) lo = mid; else hi = mid - 1;
  }
  const int64_t r = k - block_pre[lo];
  int64_t wlo = lo * SEL_WORDS, whi = (wlo + SEL_WORDS < n_words ? wlo + SEL_WORDS : n_words) - 1;
  while (wlo < whi) {
    const int64_t mid = (wlo + whi + 1) >> 1;
    if (word_pre[mid] <= r) wlo = mid; else whi = mid - 1;
  }
  uint32_t v = grid_word(bits, wlo, n_cells);
  for (int64_t q = r - word_pre[wlo]; q > 0; --q) v &= v - 1u;      // drop the lower set bits
  cells[i] = (int32_t)(wlo * 32 + (v ? __ffs(v) - 1 : 0));
}

// --- ray marching (nerfacc.ray_marching, fixed-step lattice, AABB contraction) ----------------------------------------
// Every operation of the lattice t_min + k dt, of the mid-points and of the position a step is decided at is rounded on its own (add_rn, sub_rn,
// mul_rn above k_grid_points).  hipcc fused t_min + k dt and o + d m into one fma each when they were written with __fadd_rn / __fmul_rn: the
// lattice then differed by an ulp from the oracle's and from the one the host's afx_march_max_steps walks, and a ray starting at max(0, near)
// could keep one step more than that bound.
struct MarchArgs {
  const float* org; const float* dir;      // [R,3]
  int64_t n_rays;
  int32_t has_aabb; float aabb[6];        // scene_aabb
  int32_t has_near, has_far; float near_plane, far_plane;
  float dt;
  const uint32_t* bits;                    // grid bitfield or nullptr
  GridDesc g;
};
__device__ __forceinline__ void march_range(const MarchArgs& a, int64_t r, float o[3], float d[3], float& tmin, int& n_steps) {
#pragma unroll
  for (int q = 0; q < 3; ++q) { o[q] = a.org[3 * r + q]; d[q] = a.dir[3 * r + q]; }
  float t_min = 0.f, t_max = 1e10f;
  if (a.has_aabb) {
    // slab test; rays that miss get t_min = t_max = 1e10
    float lo = -INFINITY, hi = INFINITY;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float inv = __fdiv_rn(1.0f, d[q] == 0.f ? 1e-12f : d[q]);
      const float t0 = mul_rn(sub_rn(a.aabb[q], o[q]), inv), t1 = mul_rn(sub_rn(a.aabb[3 + q], o[q]), inv);
      lo = fmaxf(lo, fminf(t0, t1));
      hi = fminf(hi, fmaxf(t0, t1));
    }
    const bool miss = hi < fmaxf(lo, 0.f);
    t_min = miss ? 1e10f : fmaxf(lo, 0.f);
    t_max = miss ? 1e10f : hi;
  }
  if (a.has_near) t_min = fmaxf(t_min, a.near_plane);
  if (a.has_far) t_max = fminf(t_max, a.far_plane);
  float ns = ceilf(__fdiv_rn(sub_rn(t_max, t_min), a.dt));
  if (!(ns > 0.f)) ns = 0.f;
  n_steps = t_min >= 1e10f ? 0 : (ns > 2.0e9f ? 2000000000 : (int)ns);
  // nerfacc marches `while (t_mid < far)`: a step belongs to the ray when its MID-POINT lies before t_max (not its start), so the
  // ceil() above is corrected by the step(s) at the end whose mid-point falls outside / inside - same fp32 expressions as the loops below
  auto mid_of = [&](int k) { const float ts = add_rn(t_min, mul_rn((float)k, a.dt)); return mul_rn(add_rn(ts, add_rn(ts, a.dt)), 0.5f); };
  if (n_steps < 2000000000) {
    while (n_steps > 0 && !(mid_of(n_steps - 1) < t_max)) --n_steps;
    for (int i = 0; i < 2 && t_min < 1e10f && mid_of(n_steps) < t_max; ++i) ++n_steps;
  }
  tmin = t_min;
}
__device__ __forceinline__ bool march_keep(const MarchArgs& a, const float o[3], const float d[3], float ts, float te) {
  if (!a.bits) return true;
  const float m = mul_rn(add_rn(ts, te), 0.5f);
  int64_t idx;
  if (!grid_cell(a.g, add_rn(o[0], mul_rn(d[0], m)), add_rn(o[1], mul_rn(d[1], m)), add_rn(o[2], mul_rn(d[2], m)), idx)) return false;
  return (a.bits[idx >> 5] >> (idx & 31)) & 1u;
}
// The five per-ray kernels below run ONE WAVEFRONT PER RAY (blocks of 256 threads = 4 rays): the 64 lanes take 64 consecutive steps /
// samples of the ray at a time, compaction offsets come from a ballot + prefix population count, so the writes of a chunk are
// contiguous and the arithmetic per step is exactly the one-thread-per-ray version's (same expressions, same order where order matters).
// (One thread per ray left 5 625 rays x 300 dependent steps on 88 wavefronts: 0.66 ms of a 2.1 ms training iteration.)
__device__ __forceinline__ int lane_prefix(uint64_t ballot) {      // kept lanes below this one
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}
// pass 1: kept steps per ray.  pass 2 (offsets = exclusive scan of the counts): packed (ray_indices, t_starts, t_ends[, mid-points]).
__global__ void __launch_bounds__(256) k_march_count(const MarchArgs a, int32_t* counts) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= a.n_rays) return;
  float o[3], d[3], tmin;
  int ns;
  march_range(a, r, o, d, tmin, ns);
  int c = 0;
  for (int k0 = 0; k0 < ns; k0 += 64) {
    const int k = k0 + lane;
    bool keep = false;
    if (k < ns) {
      const float ts = add_rn(tmin, mul_rn((float)k, a.dt)), te = add_rn(ts, a.dt);
      keep = march_keep(a, o, d, ts, te);
    }
    c += __popcll(__ballot(keep));
  }
  if (lane == 0) counts[r] = c;
}
__global__ void __launch_bounds__(256) k_march_write(const MarchArgs a, const int64_t* offsets, int32_t* ray_indices, float* t_starts, float* t_ends, float* mid_pts) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= a.n_rays) return;
  float o[3], d[3], tmin;
  int ns;
  march_range(a, r, o, d, tmin, ns);
  int64_t base = offsets[r];
  for (int k0 = 0; k0 < ns; k0 += 64) {
    const int k = k0 + lane;
    bool keep = false;
    float ts = 0.f, te = 0.f;
    if (k < ns) {
      ts = add_rn(tmin, mul_rn((float)k, a.dt));
      te = add_rn(ts, a.dt);
      keep = march_keep(a, o, d, ts, te);
    }
    const uint64_t bal = __ballot(keep);
    if (keep) {
      const int64_t w = base + lane_prefix(bal);
      ray_indices[w] = (int32_t)r; t_starts[w] = ts; t_ends[w] = te;
      if (mid_pts) {
        // positions = o + d * (t_s + t_e) / 2.0   (alpha_fn, nerf_helpers_acc.py:13-15)
        const float sm = add_rn(ts, te);
#pragma unroll
        for (int q = 0; q < 3; ++q) mid_pts[3 * w + q] = add_rn(o[q], __fdiv_rn(mul_rn(d[q], sm), 2.0f));
      }
    }
    base += __popcll(bal);
  }
}
// alpha of the candidates from the raw MLP output: 1 - exp(-sigmoid(raw) * (t_e - t_s))  (alpha_fn, nerf_helpers_acc.py:19-23),
// then nerfacc's render_visibility per ray over its packed segment: steps with alpha < alpha_thre are skipped WITHOUT
// attenuating T; the ray stops once T < early_stop_eps.  keep[i] in {0,1}; counts[r] = kept steps of ray r.
// The 64 lanes form the alphas of 64 samples at once (the transcendental part); the transmittance product then runs over them IN ORDER
// (wave-uniform loop of lane broadcasts: the same multiplications in the same order as a sequential march, so the kept set is the same bit for bit).
// alpha_fn's expression for one candidate (nerf_helpers_acc.py:19-23) - shared by k_march_visibility and the single-evaluation composite kernel,
// so both decide the kept set from the same bits
__device__ __forceinline__ float march_alpha(float raw, float ts, float te) {
  const float sg = 1.f / (1.f + expf(-raw));
  return 1.f - expf(-__fmul_rn(sg, __fsub_rn(te, ts)));
}
// One 64-sample chunk of render_visibility, one wavefront (`valid`: the lane holds a sample; `sfw`: the wave's 64 floats of LDS).  Returns whether
// the lane's sample is kept and advances the transmittance T (wave-uniform) past the chunk.
// The transmittance in front of each of the 64 samples, IN ORDER and branch-free.  A thin (or absent) sample multiplies by exactly 1, so lane j's
// p = ((T f_0) f_1) ... f_(j-1) is the sequential march's value bit for bit: every lane runs the same 64 multiplications on factors that come
// back from LDS as broadcast reads (all issued up front), with f_k replaced by 1 in the lanes <= k.  Sample j is kept iff it is thick and p has
// not fallen below early_stop_eps (T never grows, so the products behind the stop - which a sequential march does not form - cannot bring a
// sample back).  Replaces a loop with two branches and a ds_bpermute per sample, on which the kernel was latency-bound.
__device__ __forceinline__ bool vis_chunk(float alpha, bool valid, float early_stop_eps, float alpha_thre, float& T, float* sfw, int lane) {
  const bool thick = valid && !(alpha < alpha_thre);
  bool mine = false;
  if (!(T < early_stop_eps)) {                   // (wave-uniform)
    const float f = thick ? 1.f - alpha : 1.f;
    sfw[lane] = f;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (one wave: its LDS operations complete in order; the fence is for the compiler)
    float fk[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) fk[k] = sfw[k];
    float p = T;
#pragma unroll
    for (int k = 0; k < 64; ++k) p = __fmul_rn(p, k < lane ? fk[k] : 1.f);
    mine = thick && !(p < early_stop_eps);
    T = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, __fmul_rn(p, f)), 63));
    asm volatile("" ::: "memory");               // (the next chunk overwrites the factors behind these reads)
  }
  return mine;
}
// alpha of the candidates from the raw MLP output: 1 - exp(-sigmoid(raw) * (t_e - t_s))  (alpha_fn, nerf_helpers_acc.py:19-23),
// then nerfacc's render_visibility per ray over its packed segment: steps with alpha < alpha_thre are skipped WITHOUT
// attenuating T; the ray stops once T < early_stop_eps.  keep[i] in {0,1}; counts[r] = kept steps of ray r.
// The 64 lanes form the alphas of 64 samples at once (the transcendental part); the transmittance product then runs over them IN ORDER
// (vis_chunk: the same multiplications in the same order as a sequential march, so the kept set is the same bit for bit).
__global__ void __launch_bounds__(256) k_march_visibility(const float* raw, int is_alpha, const float* t_starts, const float* t_ends, const int64_t* offsets, int64_t n_rays,
                                                          float early_stop_eps, float alpha_thre, uint8_t* keep, int32_t* counts) {
  __shared__ float sf[4][64];
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n_rays) return;
  const int64_t i0 = offsets[r], i1 = offsets[r + 1];
  float T = 1.f;
  int c = 0;
  for (int64_t b = i0; b < i1; b += 64) {
    const int64_t i = b + lane;
    float alpha = 0.f;
    if (i < i1) {
      alpha = raw[i];           // is_alpha: the caller's alpha_fn output
      if (!is_alpha) alpha = march_alpha(alpha, t_starts[i], t_ends[i]);
    }
    const bool mine = vis_chunk(alpha, i < i1, early_stop_eps, alpha_thre, T, sf[threadIdx.x >> 6], lane);
    if (i < i1) keep[i] = mine ? 1 : 0;
    c += __popcll(__ballot(mine));
  }
  if (lane == 0) counts[r] = c;
}

// Forward-only grid render (afx_march_render): visibility and compositing per ray from the ONE raw output of the candidates, i.e. what
// afx_march_visibility -> afx_march_compact -> get_predictions over the kept samples -> afx_composite_packed gives, without the second evaluation.
//  - the kept set: k_march_visibility's arithmetic (march_alpha, vis_chunk), bit for bit;
//  - pixel = prod exp(-sigmoid(raw) (t_e - t_s)) over the kept samples IN ORDER, k_composite_packed's expressions.  A dropped sample (and an
//    absent lane) contributes a factor of exactly 1, which leaves the product unchanged, so the 64 factors of a chunk are multiplied in lane order
//    from an LDS broadcast, every lane forming the same product: the sequence of multiplications of k_composite_packed's loop, bit for bit;
//  - binary_pixel (optional): the same product with factor 1 also for kept samples whose sigmoid(raw) < binary_thresh (the zero_idx of the
//    reference's binary render, visualization/visualization.py:349-352: sigma forced to 0 gives exp(-0) = 1);
//  - kept_counts (optional): kept samples per ray.  A ray without candidates gets 1 in both pixels.
// One wavefront per ray; reads stay inside the ray's segment [offsets[r], offsets[r + 1]).
__global__ void __launch_bounds__(256) k_march_render_composite(const float* raw, const float* t_starts, const float* t_ends, const int64_t* offsets,
                                                                int64_t n_rays, float early_stop_eps, float alpha_thre, float binary_thresh,
                                                                float* pixel, float* binary_pixel, int32_t* kept_counts) {
  __shared__ float sf[4][64];      // vis_chunk's transmittance factors
  __shared__ float sp[4][64];      // the chunk's pixel factors
  __shared__ float sb[4][64];      // ... and binary-pixel factors
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (r >= n_rays) return;
  const int64_t i0 = offsets[r], i1 = offsets[r + 1];
  const bool want_binary = binary_pixel != nullptr;
  float T = 1.f, P = 1.f, B = 1.f;
  int c = 0;
  for (int64_t b = i0; b < i1; b += 64) {
    const int64_t i = b + lane;
    const bool valid = i < i1;
    float alpha = 0.f, sg = 0.f, e = 1.f;
    if (valid) {
      const float x = raw[i], ts = t_starts[i], te = t_ends[i];
      alpha = march_alpha(x, ts, te);
      sg = sigmoidf_(x);                                   // k_composite_packed's expressions
      e = expf(-__fmul_rn(sg, __fsub_rn(te, ts)));
    }
    const bool mine = vis_chunk(alpha, valid, early_stop_eps, alpha_thre, T, sf[w], lane);
    c += __popcll(__ballot(mine));
    sp[w][lane] = mine ? e : 1.f;
    if (want_binary) sb[w][lane] = (mine && !(sg < binary_thresh)) ? e : 1.f;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (one wave: its LDS operations complete in order; the fence is for the compiler)
    float fk[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) fk[k] = sp[w][k];
#pragma unroll
    for (int k = 0; k < 64; ++k) P = __fmul_rn(P, fk[k]);
    if (want_binary) {
#pragma unroll
      for (int k = 0; k < 64; ++k) fk[k] = sb[w][k];
#pragma unroll
      for (int k = 0; k < 64; ++k) B = __fmul_rn(B, fk[k]);
    }
    asm volatile("" ::: "memory");               // (the next chunk overwrites the factors behind these reads)
  }
  if (lane == 0) {
    pixel[r] = P;
    if (want_binary) binary_pixel[r] = B;
    if (kept_counts) kept_counts[r] = c;
  }
}

// Rays of afx_march_render's pose mode, written to its workspace: load_ray (the dense fused kernels' get_ray_values, ray r = ray_id0 + r of
// [n_proj, H, W]), so the march sees the rays those kernels generate, bit for bit.  One thread per ray.
__global__ void k_pose_rays(const ChainArgs a, int64_t n_rays, float* org, float* dir) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  float ox, oy, oz, dx, dy, dz;
  load_ray(a, (int)r, ox, oy, oz, dx, dy, dz);
  org[3 * r + 0] = ox; org[3 * r + 1] = oy; org[3 * r + 2] = oz;
  dir[3 * r + 0] = dx; dir[3 * r + 1] = dy; dir[3 * r + 2] = dz;
}

// Single-evaluation grid step (afx_march_train_step_mse_single_eval): visibility, optical depth, MSE and the finished dL/draw per ray, from the
// outputs of the packed step's forward half run over the CANDIDATES (candidate i of ray r sits at padded row 32 goff[r] + i - offsets[r]).
//  - the kept set: k_march_visibility's arithmetic (march_alpha, vis_chunk) on the forward half's own raw output;
//  - the optical depth: tau of the kept samples summed as the compacted list of afx_march_train_step_mse sums it - 32-sample groups of consecutive
//    kept samples, each reduced by the forward half's 16/8/4/2/1 butterfly (lane 0's value; padding slots add 0), the group partials added in
//    order as k_finish_mse_packed does - so pixel and dL/d(optical depth) are those of the two-evaluation step bit for bit;
//  - gpart[row] (PHASE 1 left g' = dt sigma (1 - sigma)): dod g' for kept rows (PHASE 2's product), 0 for dropped ones (padding rows are 0 already).
// Writes keep[i], kept_counts[r] and the ray's pixel into pix[r]; k_single_eval_finish publishes the pixels once the kept total is known.
// One wavefront per ray; `stg` stages the tau of kept samples until a group of 32 is complete.
__global__ void __launch_bounds__(256) k_single_eval_composite(const float* row_raw, const float* row_tau, const float* t_starts, const float* t_ends,
                                                               const int64_t* offsets, const int64_t* goff, int64_t n_rays, float early_stop_eps,
                                                               float alpha_thre, const float* target, float inv_n, uint8_t* keep, float* gpart,
                                                               int32_t* kept_counts, float* pix) {
  __shared__ float sf[4][64];
  __shared__ float stg[4][96];
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (r >= n_rays) return;
  const int64_t i0 = offsets[r], i1 = offsets[r + 1], row0 = goff[r] * GROUP - i0;      // padded row of candidate i: row0 + i
  float* st = stg[w];
  auto group_sum = [&](int cnt) {      // the butterfly of the forward half over slots 0 .. cnt-1 (cnt <= 32) of the stage; lane 0's value
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float v = lane < cnt ? st[lane] : 0.f;
#pragma unroll
    for (int sh = 16; sh >= 1; sh >>= 1) v += __shfl_xor(v, sh);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
  };
  float T = 1.f, od = 0.f;
  int c = 0, ns = 0;      // kept samples of the ray, staged ones (< 32 between chunks)
  for (int64_t b = i0; b < i1; b += 64) {
    const int64_t i = b + lane;
    const bool valid = i < i1;
    const float alpha = valid ? march_alpha(row_raw[row0 + i], t_starts[i], t_ends[i]) : 0.f;
    const bool mine = vis_chunk(alpha, valid, early_stop_eps, alpha_thre, T, sf[w], lane);
    const uint64_t bal = __ballot(mine);
    if (valid) keep[i] = mine ? 1 : 0;
    if (mine) st[ns + lane_prefix(bal)] = row_tau[row0 + i];
    else if (valid) gpart[row0 + i] = 0.f;
    ns += __popcll(bal);
    c += __popcll(bal);
    while (ns >= 32) {
      od += group_sum(32);
      const float x = lane < ns - 32 ? st[32 + lane] : 0.f;      // shift the rest of the stage down (reads complete before the writes)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane < ns - 32) st[lane] = x;
      ns -= 32;
    }
  }
  if (ns > 0) od += group_sum(ns);
  const float T_ = expf(-od);      // k_finish_mse_packed
  const float dod = -T_ * (2.f * (T_ - target[r]) * inv_n);
  for (int64_t i = i0 + lane; i < i1; i += 64)
    if (keep[i]) gpart[row0 + i] = dod * gpart[row0 + i];
  if (lane == 0) { kept_counts[r] = c; pix[r] = T_; }
}

// counts[R] -> offsets[R+1] (exclusive prefix sums, int64), optionally the offsets of the group-aligned copy (ceil(count / 32) groups per
// ray) and the two totals in one place for the host's single read.  One block: R is a batch of rays (5 625 in the reference), and the
// torch sequence this replaces (zeros, cumsum = 2 rocprim launches, for the groups another 4) was a quarter of the launches of the
// dispatch-bound grid iteration.
// `mailbox` (host-mapped, fine-grained memory; afx_march_train_step_mse): the two totals and then `tag`, behind a system-scope fence - the host
// polls the tag instead of queueing a copy and a stream synchronisation behind the kernel.
__global__ void __launch_bounds__(1024) k_ray_offsets(const int32_t* counts, int64_t n_rays, int64_t* offsets, int64_t* group_offsets, int64_t* totals,
                                                       volatile int64_t* mailbox = nullptr, int64_t tag = 0) {
  int64_t r0, r1, p[2] = {0, 0}, tot[2];             // samples, 32-sample groups
  scan_run<1024>(n_rays, r0, r1);
  for (int64_t r = r0; r < r1; ++r) { const int64_t c = counts[r]; p[0] += c; p[1] += (c + 31) >> 5; }
  block_exclusive_scan<1024>(p, tot);
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t c = counts[r];
    offsets[r] = p[0];
    if (group_offsets) group_offsets[r] = p[1];
    p[0] += c; p[1] += (c + 31) >> 5;
  }
  if (threadIdx.x == 1023) {
    offsets[n_rays] = tot[0];
    if (group_offsets) group_offsets[n_rays] = tot[1];
    if (totals) { totals[0] = tot[0]; totals[1] = tot[1]; }
    if (mailbox) {
      mailbox[0] = tot[0]; mailbox[1] = tot[1];
      __threadfence_system();
      mailbox[2] = tag;
    }
  }
}

// The sizes of a grid training iteration, on the device (afx_march_train_step_mse_capturable): from the totals of the two offsets kernels
// (totals[0] candidates, totals[2] kept samples, totals[3] their 32-sample groups) the counters the caller reads (counts[3] = candidates, kept,
// groups), the optimizer's skip flag (1.0 when nothing survived the march) and the size block the capacity launches of the packed step read
// (SZ_* slots): one chunk of `tile`-sample tiles holding ng groups, split by wgrad_split as the host splits it, so the weight-gradient sums run
// in the same order as in afx_march_train_step_mse.  One thread.
__device__ __forceinline__ void grid_step_sizes(int64_t ng, int tile, int splits0, int max_splits, int max_small, int64_t* dsz) {
  const int64_t n_total = ng * GROUP, rows = (n_total + tile - 1) / tile * tile;
  const WgradSplit s = wgrad_split(rows, splits0, max_splits, max_small);
  dsz[SZ_NTOTAL] = n_total; dsz[SZ_ROWS] = rows; dsz[SZ_SPLITS] = s.splits; dsz[SZ_RPS] = s.rows_per_split; dsz[SZ_SMALL] = s.n_small;
  dsz[SZ_GROUPS] = ng;
}
__global__ void k_grid_step_sizes(const int64_t* totals, int tile, int splits0, int max_splits, int max_small, int64_t* counts, float* skip, int64_t* dsz) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t n = totals[0], kept = totals[2], ng = totals[3];
  counts[0] = n; counts[1] = kept; counts[2] = ng;
  *skip = kept == 0 ? 1.f : 0.f;
  grid_step_sizes(ng, tile, splits0, max_splits, max_small, dsz);
}
// The single-evaluation step's size block: the step runs over the candidates' groups (totals[1], afx_ray_offsets over the march's counts).  One thread.
__global__ void k_single_eval_sizes(const int64_t* totals, int tile, int splits0, int max_splits, int max_small, int64_t* dsz) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  grid_step_sizes(totals[1], tile, splits0, max_splits, max_small, dsz);
}
// ... and its end: totals[2] / totals[3] = kept samples and the groups the compacted list would have (afx_ray_offsets over kept_counts).  The
// caller's counters and skip flag; when nothing was kept the pixels stay untouched and the size block is cut to zero rows, so the backward half
// and the weight-gradient kernels behind this one do nothing and leave the gradient untouched (k_reduce_all / k_reduce_coef); else pix -> pixel.
__global__ void k_single_eval_finish(const int64_t* totals, const float* pix, int64_t n_rays, float* pixel, int64_t* counts, float* skip, int64_t* dsz) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t kept = totals[2];
  if (r == 0) {
    counts[0] = totals[0]; counts[1] = kept; counts[2] = totals[3];
    *skip = kept == 0 ? 1.f : 0.f;
    if (kept == 0) { dsz[SZ_NTOTAL] = 0; dsz[SZ_ROWS] = 0; }
  }
  if (kept == 0 || r >= n_rays) return;
  pixel[r] = pix[r];
}

__global__ void __launch_bounds__(256) k_march_compact(const uint8_t* keep, const int64_t* offsets_in, const int64_t* offsets_out, int64_t n_rays,
                                                       const float* ts_in, const float* te_in, int32_t* ri_out, float* ts_out, float* te_out) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n_rays) return;
  int64_t w = offsets_out[r];
  const int64_t i1 = offsets_in[r + 1];
  for (int64_t b = offsets_in[r]; b < i1; b += 64) {
    const int64_t i = b + lane;
    const bool k = i < i1 && keep[i] != 0;
    const uint64_t bal = __ballot(k);
    if (k) {
      const int64_t o = w + lane_prefix(bal);
      ri_out[o] = (int32_t)r; ts_out[o] = ts_in[i]; te_out[o] = te_in[i];
    }
    w += __popcll(bal);
  }
}

// Group-aligned copy of a packed, ray-sorted sample list for the fused packed training step: ray r's samples start at padded index
// 32 goff[r] (goff = exclusive scan of ceil(count / 32)); the rest of its last 32-sample group is dead padding (ts = te = 0); group_ray[g] = r.
__global__ void __launch_bounds__(256) k_pack_groups(const int64_t* offsets, const int64_t* goff, int64_t n_rays, const float* ts_in, const float* te_in,
                                                     float* ts_pad, float* te_pad, int32_t* group_ray) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n_rays) return;
  const int64_t i0 = offsets[r], cnt = offsets[r + 1] - i0, g0 = goff[r], g1 = goff[r + 1];
  for (int64_t k = lane; k < (g1 - g0) * 32; k += 64) {
    ts_pad[g0 * 32 + k] = k < cnt ? ts_in[i0 + k] : 0.f;
    te_pad[g0 * 32 + k] = k < cnt ? te_in[i0 + k] : 0.f;
  }
  for (int64_t g = g0 + lane; g < g1; g += 64) group_ray[g] = (int32_t)r;
}

// --- device ray sampler (sample_pixel_rays, nerf/nerf_helpers.py:137-150): weighted sampling WITHOUT replacement of k of n
// rays.  Efraimidis-Spirakis keys: key_i = u_i^(1/w_i) (log form: log(u_i)/w_i), the k largest keys are a weighted sample
// without replacement; u from Philox (perf mode) or supplied.  The top-k selection is the radix select below.
// (blockIdx.y = batch b of afx_sample_batches: Philox stream `stream + b`, keys row b; a plain call has one row)
// afx_sample_batches_dev: the first stream id is stream + *stream_dev, a device counter read when the kernel runs (a captured call follows it).
__global__ void k_sample_keys(const float* weights, int64_t n, const float* u_in, uint64_t seed, uint64_t stream, float* keys,
                              const int64_t* stream_dev = nullptr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (stream_dev) stream += (uint64_t)*stream_dev;
  const float w = weights ? weights[i] : 1.f;
  float u = u_in ? u_in[i] : philox_uniform(seed, stream + blockIdx.y, (uint64_t)i);
  u = fmaxf(u, 5.9604645e-08f);
  keys[(int64_t)blockIdx.y * n + i] = w > 0.f ? logf(u) / w : -INFINITY;
}
// --- top-k by radix select (the sampler's selection step; a full device sort of the 900 000 keys was 13 % of the reference's
// training iteration).  Keys map to uint32 monotonically; three histogram passes (11 + 11 + 10 bits, each over the keys that
// match the prefix found so far) locate the k-th largest key T exactly; the selected set {key > T} plus the first `need_eq`
// keys equal to T (lowest index first) is then written in ASCENDING INDEX order by a counted, two-level compaction - no
// atomics on the output, so the result is deterministic.  Byte/integer work, HBM-bound: 5 reads of the key array.
// Every kernel takes blockIdx.y as a batch index (afx_sample_batches: B independent selections per launch - at 900 000 keys a selection is
// 11 launches of a few microseconds each, i.e. launch latency; B of them share the 11 launches): row b of keys [B][n], hist [B][SEL_BINS],
// state [B], counts [B][nb], output [B][k].
__device__ __forceinline__ uint32_t key_bits(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
struct SelState { uint32_t prefix, remaining, pad0, pad1; };
constexpr int SEL_BINS = 2048;
constexpr int SEL_PER_BLOCK = 1024;      // elements per block of the compaction kernels (256 threads x 4)

__global__ void __launch_bounds__(256) k_sel_init(SelState* st, uint32_t k, uint32_t* hist) {
  st += blockIdx.y; hist += (size_t)blockIdx.y * SEL_BINS;
  if (threadIdx.x == 0) { st->prefix = 0; st->remaining = k; }
  for (int i = threadIdx.x; i < SEL_BINS; i += 256) hist[i] = 0;
}
__global__ void __launch_bounds__(256) k_sel_hist(const float* keys, int64_t n, const SelState* st, uint32_t himask, int shift,
                                                  uint32_t binmask, uint32_t* hist) {
  __shared__ uint32_t h[SEL_BINS];
  keys += (int64_t)blockIdx.y * n; st += blockIdx.y; hist += (size_t)blockIdx.y * SEL_BINS;
  for (int i = threadIdx.x; i < SEL_BINS; i += 256) h[i] = 0;
  __syncthreads();
  const uint32_t prefix = st->prefix;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t u = key_bits(keys[i]);
    if ((u & himask) == prefix) atomicAdd(&h[(u >> shift) & binmask], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SEL_BINS; i += 256)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}
// one block: the bin (from the top) in which the remaining rank falls; extends the prefix, leaves the histogram zeroed
__global__ void __launch_bounds__(256) k_sel_scan(uint32_t* hist, SelState* st, int shift) {
  __shared__ uint32_t part[256];
  __shared__ uint32_t above[256];      // keys in the groups above group t
  st += blockIdx.y; hist += (size_t)blockIdx.y * SEL_BINS;
  const int t = threadIdx.x;           // group t = bins [8 (255 - t), 8 (255 - t) + 7], i.e. t = 0 is the top group
  const uint32_t r = st->remaining;    // read by every thread BEFORE the barriers; one thread rewrites it behind them
  uint32_t c[8], s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { c[j] = hist[8 * (255 - t) + (7 - j)]; s += c[j]; }     // c[0] = the group's top bin
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (int g = 0; g < 256; ++g) { above[g] = run; run += part[g]; }
  }
  __syncthreads();
  uint32_t a = above[t];
  if (a < r && r <= a + s) {           // exactly one group holds the r-th largest candidate
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (a < r && r <= a + c[j]) {
        st->prefix |= (uint32_t)(8 * (255 - t) + (7 - j)) << shift;
        st->remaining = r - a;          // rank inside the bin (>= 1)
      }
      a += c[j];
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) hist[8 * t + j] = 0;
}
// per block of 1024 keys: how many are above the threshold / equal to it
__global__ void __launch_bounds__(256) k_sel_count(const float* keys, int64_t n, const SelState* st, uint32_t* cnt_gt, uint32_t* cnt_eq) {
  __shared__ uint32_t sg[256], se[256];
  keys += (int64_t)blockIdx.y * n; st += blockIdx.y; cnt_gt += (size_t)blockIdx.y * gridDim.x; cnt_eq += (size_t)blockIdx.y * gridDim.x;
  const uint32_t T = st->prefix;
  const int64_t base = (int64_t)blockIdx.x * SEL_PER_BLOCK + 4 * threadIdx.x;
  uint32_t g = 0, e = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (base + j < n) { const uint32_t u = key_bits(keys[base + j]); g += u > T; e += u == T; }
  sg[threadIdx.x] = g; se[threadIdx.x] = e;
  __syncthreads();
  for (int sft = 128; sft >= 1; sft >>= 1) {
    if ((int)threadIdx.x < sft) { sg[threadIdx.x] += sg[threadIdx.x + sft]; se[threadIdx.x] += se[threadIdx.x + sft]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { cnt_gt[blockIdx.x] = sg[0]; cnt_eq[blockIdx.x] = se[0]; }
}
// one block: exclusive prefix sums of the per-block counts, in place
__global__ void __launch_bounds__(1024) k_sel_offsets(uint32_t* cnt_gt, uint32_t* cnt_eq, int64_t nb) {
  cnt_gt += (size_t)blockIdx.y * nb; cnt_eq += (size_t)blockIdx.y * nb;
  int64_t b0, b1;
  scan_run<1024>(nb, b0, b1);
  uint32_t p[2] = {0, 0}, tot[2];                     // above, equal
  for (int64_t b = b0; b < b1; ++b) { p[0] += cnt_gt[b]; p[1] += cnt_eq[b]; }
  block_exclusive_scan<1024>(p, tot);
  for (int64_t b = b0; b < b1; ++b) { const uint32_t a = cnt_gt[b], c = cnt_eq[b]; cnt_gt[b] = p[0]; cnt_eq[b] = p[1]; p[0] += a; p[1] += c; }
}
// output position of a selected key = (# keys above T before it) + min(# keys equal to T before it, need_eq)
__global__ void __launch_bounds__(256) k_sel_write(const float* keys, int64_t n, const SelState* st, const uint32_t* off_gt,
                                                   const uint32_t* off_eq, int64_t k, int64_t* out_idx) {
  keys += (int64_t)blockIdx.y * n; st += blockIdx.y; off_gt += (size_t)blockIdx.y * gridDim.x; off_eq += (size_t)blockIdx.y * gridDim.x;
  out_idx += (int64_t)blockIdx.y * k;
  const uint32_t T = st->prefix, need_eq = st->remaining;
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * SEL_PER_BLOCK + 4 * t;
  uint32_t u[4], p[2] = {0, 0}, tot[2];               // keys above T, equal to T
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    u[j] = base + j < n ? key_bits(keys[base + j]) : 0u;
    if (base + j < n) { p[0] += u[j] > T; p[1] += u[j] == T; }
  }
  block_exclusive_scan<256>(p, tot);
  uint32_t g = off_gt[blockIdx.x] + p[0], e = off_eq[blockIdx.x] + p[1];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (base + j >= n) break;
    const bool gt = u[j] > T, eq = u[j] == T;
    if (gt || (eq && e < need_eq)) {
      const int64_t pos = (int64_t)g + (e < need_eq ? e : need_eq);
      if (pos < k) out_idx[pos] = base + j;
    }
    g += gt; e += eq;
  }
}

// gather the sampled rays of a device-resident ray table (o, d, pixel) by index
__global__ void k_gather_rays(const float* org, const float* dir, const float* pix, const int64_t* idx, int64_t k, float* o_out, float* d_out, float* p_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int64_t s = idx[i];
#pragma unroll
  for (int q = 0; q < 3; ++q) { o_out[3 * i + q] = org[3 * s + q]; d_out[3 * i + q] = dir[3 * s + q]; }
  if (pix && p_out) p_out[i] = pix[s];
}
__global__ void k_philox_fill(uint64_t seed, uint64_t stream, int64_t n, float* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = philox_uniform(seed, stream, (uint64_t)i);
}

// --- the bookkeeping between two captured grid iterations (afx_train_round_advance): what the training loop does on the host after a
// step - the next learning rate, the step's loss / counts / skip flag kept for the display point, the sample total, the step counter -
// from device memory, so that a graph holding several iterations needs no host in between.  One lane; every write is a plain store.
struct TrainRoundArgs {
  int64_t* step_dev; const float* lr_table; int64_t n_table; float* lr_dev;
  const float *skip, *loss; const int64_t* counts;
  int64_t round_len; float* loss_hist; int64_t* counts_hist; float* skip_hist; float* last_loss; int64_t* n_marched;
};
__global__ void k_train_round_advance(TrainRoundArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t s = *a.step_dev;
  const int64_t li = s < 0 ? 0 : (s < a.n_table ? s : a.n_table - 1);      // (a negative counter never indexes before the table)
  int64_t slot = s % a.round_len;
  if (slot < 0) slot += a.round_len;
  const float loss = *a.loss, skip = *a.skip;
  const int64_t c0 = a.counts[0], c1 = a.counts[1], c2 = a.counts[2];
  a.lr_dev[0] = a.lr_table[li];
  a.loss_hist[slot] = loss;
  a.counts_hist[3 * slot + 0] = c0; a.counts_hist[3 * slot + 1] = c1; a.counts_hist[3 * slot + 2] = c2;
  a.skip_hist[slot] = skip;
  if (!(skip > 0.f)) *a.last_loss = loss;      // (the last step that kept samples)
  *a.n_marched += c1;
  *a.step_dev = s + 1;
}

}  // namespace afx
