// afx_kernels_territory.hip - the exact 3-D feature transform (for every voxel the squared distance to the nearest site AND which site that
// is, ties to the lowest linear index) and the per-label overlap counts built on it (afx_feature_transform_3d, afx_label_overlap_3d; the
// definition stands in include/afx.h).  Integer arithmetic only.  Four kernels:
//   k_ft3_axis2      a wave per line along axis 2, 64 voxels at a time, as k_edt3_axis2: the sites of a chunk are one ballot, the nearest
//                    one at or below a lane the highest set bit below it, the sweep back the same from above.  On an equal distance the
//                    lower side (the lower index) stays.  Writes d2 (the squared 1-D distance) and nearest (the site's linear index).
//   k_ft3_lines      along axis 1, then axis 0, as k_edt3_lines: a workgroup takes a tile of 16 (lines of up to 512 voxels) or 8 adjacent
//                    lines into LDS as 8-byte cells d2 << 32 | site (all ones: no site), and every voxel searches the lower envelope
//                    outwards.  The pair (value, site) is minimised lexicographically - one unsigned 64-bit compare - and the search
//                    stops only once (c - c')^2 alone is GREATER than the best value: at equality a site straight along the axis ties
//                    and may carry a lower index.  In place: a workgroup has read its whole tile before it writes, and no other
//                    workgroup touches that tile.
//   k_overlap_zero   counts = 0.
//   k_overlap_count  grid-stride over the voxels in runs of 64 per wave; the lanes of a wave that hold the same label meet in ballots
//                    (one round per distinct label of the wave), the first of them adds the four counts to the workgroup's LDS table,
//                    and the table goes to global memory once per workgroup with 64-bit integer atomics.
// NOTHING CAN HANG: every loop is bounded by an argument (the rounds of a wave by its 64 lanes), the loops that hold a ballot or a barrier
// have wave- and workgroup-uniform trip counts.  NOTHING IS INDEXED BY DATA except labels[s], whose index s is range-checked against n
// first, and the count rows, whose label is range-checked against n_labels first.
#include "afx_internal.h"
#include <algorithm>

namespace {

constexpr int FT3_BLOCK = 256;
constexpr uint32_t FT3_NONE = AFX_EDT3D_NONE;
constexpr unsigned long long FT3_NONE64 = ~0ull;      // the packed cell of "no site": larger than every real pair
constexpr int OV_BLOCK = 256;
constexpr int OV_MAX_BLOCKS = 2048;

__global__ void __launch_bounds__(FT3_BLOCK) k_ft3_axis2(const uint8_t* __restrict__ sites, int64_t lines, int n2, uint32_t* __restrict__ d2,
                                                         int32_t* __restrict__ nearest) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * FT3_BLOCK + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * FT3_BLOCK) >> 6;
  for (int64_t line = wave; line < lines; line += n_waves) {
    const uint8_t* v = sites + line * n2;
    uint32_t* od = d2 + line * n2;
    int32_t* on = nearest + line * n2;
    const int32_t first = (int32_t)(line * n2);        // the linear index of the line's voxel 0 (n0 n1 n2 <= 2^30)
    int last = -1;                                     // the last site before this chunk (the same in every lane)
    for (int c0 = 0; c0 < n2; c0 += 64) {
      const int c = c0 + lane;
      const bool in = c < n2;
      const unsigned long long m = __ballot(in && v[c] != 0);
      const unsigned long long below = m & ((2ull << lane) - 1ull);                 // sites of the chunk at lanes <= mine
      const int l = below ? c0 + 63 - __builtin_clzll(below) : last;
      if (in) {
        od[c] = l < 0 ? FT3_NONE : (uint32_t)(c - l) * (uint32_t)(c - l);
        on[c] = l < 0 ? -1 : first + l;
      }
      if (m) last = c0 + 63 - __builtin_clzll(m);
    }
    int next = -1;                                     // the first site behind this chunk
    for (int c0 = (n2 - 1) / 64 * 64; c0 >= 0; c0 -= 64) {
      const int c = c0 + lane;
      const bool in = c < n2;
      const unsigned long long m = __ballot(in && v[c] != 0);
      const unsigned long long above = m & ~((1ull << lane) - 1ull);                 // sites of the chunk at lanes >= mine
      const int r = above ? c0 + __builtin_ctzll(above) : next;
      if (in && r >= 0) {
        const uint32_t dr = (uint32_t)(r - c) * (uint32_t)(r - c);
        if (dr < od[c]) od[c] = dr, on[c] = first + r;  // this lane's own store of the sweep forward; strictly nearer only: a tie stays below
      }
      if (m) next = c0 + __builtin_ctzll(m);
    }
  }
}

// grid: outer * tiles, dynamic LDS len * tw * 8 bytes; d2 and nearest are read and written in place
__global__ void __launch_bounds__(FT3_BLOCK) k_ft3_lines(int len, int64_t inner, int tw_shift, int tiles, uint32_t* d2, int32_t* nearest) {
  extern __shared__ unsigned long long ft3_col[];
  const int tw = 1 << tw_shift;
  const int64_t outer = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - outer * tiles);
  const int64_t k0 = (int64_t)tile << tw_shift;
  const int kw = inner - k0 < tw ? (int)(inner - k0) : tw;          // lines of this tile that exist
  const int64_t base = outer * len * inner + k0;
  const int cells = len << tw_shift;
  for (int e = threadIdx.x; e < cells; e += FT3_BLOCK) {
    const int r = e >> tw_shift, k = e & (tw - 1);
    unsigned long long v = FT3_NONE64;
    if (k < kw) {
      const int64_t at = base + (int64_t)r * inner + k;
      const uint32_t x = d2[at];
      if (x != FT3_NONE) v = ((unsigned long long)x << 32) | (unsigned long long)(uint32_t)nearest[at];
    }
    ft3_col[e] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < cells; e += FT3_BLOCK) {
    const int r = e >> tw_shift, k = e & (tw - 1);
    if (k >= kw) continue;
    unsigned long long best = FT3_NONE64;
    for (int d = 0; d < len; ++d) {
      const uint32_t dd = (uint32_t)d * (uint32_t)d;
      if (dd > (uint32_t)(best >> 32)) break;          // greater, not greater or equal: at equality a site along the axis still ties
      const unsigned long long add = (unsigned long long)dd << 32;
      if (r - d >= 0) {
        const unsigned long long v = ft3_col[((r - d) << tw_shift) + k];
        if (v != FT3_NONE64 && v + add < best) best = v + add;
      }
      if (r + d < len) {
        const unsigned long long v = ft3_col[((r + d) << tw_shift) + k];
        if (v != FT3_NONE64 && v + add < best) best = v + add;
      }
    }
    const int64_t at = base + (int64_t)r * inner + k;
    d2[at] = (uint32_t)(best >> 32);                   // all ones stays AFX_EDT3D_NONE and -1
    nearest[at] = (int32_t)(uint32_t)best;
  }
}

// tile width of k_ft3_lines as a shift: 16 lines while they fit in 64 KiB of LDS (len <= 512), else 8
int ft3_tw_shift(int len) { return len <= 512 ? 4 : 3; }

__global__ void __launch_bounds__(OV_BLOCK) k_overlap_zero(unsigned long long* __restrict__ counts, int cells) {
  const int i = blockIdx.x * OV_BLOCK + threadIdx.x;
  if (i < cells) counts[i] = 0ull;
}

// dynamic LDS: (n_labels + 1) * 4 uint32; a workgroup sees fewer than 2^32 voxels (n <= 2^40, 2048 workgroups from n = 2^22 on)
__global__ void __launch_bounds__(OV_BLOCK) k_overlap_count(const int32_t* __restrict__ labels, const int32_t* __restrict__ index,
                                                            const uint32_t* __restrict__ d2, uint32_t max_d2, const uint8_t* __restrict__ a,
                                                            const uint8_t* __restrict__ b, int64_t n, int32_t n_labels,
                                                            unsigned long long* __restrict__ counts, int32_t* __restrict__ territory) {
  extern __shared__ uint32_t ov_tab[];
  const int cells = (n_labels + 1) * 4;
  for (int i = threadIdx.x; i < cells; i += OV_BLOCK) ov_tab[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * OV_BLOCK; base < n; base += (int64_t)gridDim.x * OV_BLOCK) {      // uniform over the workgroup
    const int64_t v = base + threadIdx.x;
    const bool in = v < n;
    int32_t l = 0;
    bool ia = false, ib = false;
    if (in) {
      const int64_t s = index ? (int64_t)index[v] : v;
      const bool out = s < 0 || s >= n || (d2 && d2[v] > max_d2);
      if (!out) {
        l = labels[s];
        if (l < 1 || l > n_labels) l = 0;
      }
      ia = a[v] != 0;
      ib = b && b[v] != 0;
      if (territory) territory[v] = l;
    }
    const unsigned long long ma = __ballot(ia), mb = __ballot(ib);
    unsigned long long rem = __ballot(in);             // lanes whose voxel is not counted yet: the same value in every lane
    while (rem) {
      const int lead = __builtin_ctzll(rem);
      const int32_t l0 = __shfl(l, lead, 64);
      const unsigned long long m = __ballot(in && l == l0) & rem;
      if (lane == lead) {
        uint32_t* row = ov_tab + 4 * l0;
        atomicAdd(row, (uint32_t)__builtin_popcountll(m));
        const uint32_t ca = (uint32_t)__builtin_popcountll(m & ma), cb = (uint32_t)__builtin_popcountll(m & mb);
        const uint32_t cab = (uint32_t)__builtin_popcountll(m & ma & mb);
        if (ca) atomicAdd(row + 1, ca);
        if (cb) atomicAdd(row + 2, cb);
        if (cab) atomicAdd(row + 3, cab);
      }
      rem &= ~m;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += OV_BLOCK) {
    const uint32_t c = ov_tab[i];
    if (c) atomicAdd(counts + i, (unsigned long long)c);
  }
}

}  // namespace

extern "C" int afx_feature_transform_3d(const uint8_t* sites, int32_t n0, int32_t n1, int32_t n2, uint32_t* d2, int32_t* nearest, void* stream) {
  const char* who = "afx_feature_transform_3d";
  if (!sites) return afx::set_error(AFX_E_INVALID, who, "null sites");
  if (!d2) return afx::set_error(AFX_E_INVALID, who, "null d2");
  if (!nearest) return afx::set_error(AFX_E_INVALID, who, "null nearest");
  if (!afx::volume_shape_ok(n0, n1, n2)) return afx::set_error(AFX_E_INVALID, who, "need a volume of 1..1024 voxels along each axis");
  if (int rc = afx::check_device_memory(sites, "sites", who)) return rc;
  if (int rc = afx::check_device_memory(d2, "d2", who)) return rc;
  if (int rc = afx::check_device_memory(nearest, "nearest", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t lines = (int64_t)n0 * n1, inner0 = (int64_t)n1 * n2;
  const int64_t b1 = std::min<int64_t>((lines + 3) / 4, 1 << 16);                 // 4 waves = 4 lines per workgroup, then a stride
  hipLaunchKernelGGL(k_ft3_axis2, dim3((unsigned)b1), dim3(FT3_BLOCK), 0, st, sites, lines, (int)n2, d2, nearest);
  const int s1 = ft3_tw_shift(n1), t1 = (n2 + (1 << s1) - 1) >> s1;
  hipLaunchKernelGGL(k_ft3_lines, dim3((unsigned)(n0 * t1)), dim3(FT3_BLOCK), ((size_t)n1 << s1) * sizeof(unsigned long long), st, (int)n1,
                     (int64_t)n2, s1, t1, d2, nearest);
  const int s0 = ft3_tw_shift(n0), t0 = (int)((inner0 + (1 << s0) - 1) >> s0);
  hipLaunchKernelGGL(k_ft3_lines, dim3((unsigned)t0), dim3(FT3_BLOCK), ((size_t)n0 << s0) * sizeof(unsigned long long), st, (int)n0, inner0, s0,
                     t0, d2, nearest);
  return afx::launched(who);
}

extern "C" int afx_label_overlap_3d(const int32_t* labels, const int32_t* index, const uint32_t* d2, uint32_t max_d2, const uint8_t* a,
                                    const uint8_t* b, int64_t n, int32_t n_labels, uint64_t* counts, int32_t* territory, void* stream) {
  const char* who = "afx_label_overlap_3d";
  if (!labels) return afx::set_error(AFX_E_INVALID, who, "null labels");
  if (!a) return afx::set_error(AFX_E_INVALID, who, "null a");
  if (!counts) return afx::set_error(AFX_E_INVALID, who, "null counts");
  if (n < 0 || n > AFX_LABEL_OVERLAP_MAX_N) return afx::set_error(AFX_E_INVALID, who, "n must lie in 0..2^40");
  if (n_labels < 0 || n_labels > AFX_LABEL_OVERLAP_MAX_LABELS) return afx::set_error(AFX_E_INVALID, who, "n_labels must lie in 0..4095");
  if (int rc = afx::check_device_memory(labels, "labels", who)) return rc;
  if (int rc = afx::check_device_memory(a, "a", who)) return rc;
  if (int rc = afx::check_device_memory(counts, "counts", who)) return rc;
  if (index)
    if (int rc = afx::check_device_memory(index, "index", who)) return rc;
  if (d2)
    if (int rc = afx::check_device_memory(d2, "d2", who)) return rc;
  if (b)
    if (int rc = afx::check_device_memory(b, "b", who)) return rc;
  if (territory)
    if (int rc = afx::check_device_memory(territory, "territory", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int cells = (n_labels + 1) * 4;
  hipLaunchKernelGGL(k_overlap_zero, dim3((unsigned)((cells + OV_BLOCK - 1) / OV_BLOCK)), dim3(OV_BLOCK), 0, st, (unsigned long long*)counts, cells);
  if (n > 0) {
    // 8 runs of 256 voxels per workgroup until the grid stops growing at 2048 workgroups: a workgroup's share stays below 2^40 / 2048 + 2048
    const int64_t blocks = std::min<int64_t>((n + OV_BLOCK * 8 - 1) / (OV_BLOCK * 8), OV_MAX_BLOCKS);
    hipLaunchKernelGGL(k_overlap_count, dim3((unsigned)blocks), dim3(OV_BLOCK), (size_t)cells * sizeof(uint32_t), st, labels, index, d2, max_d2, a, b,
                       n, n_labels, (unsigned long long*)counts, territory);
  }
  return afx::launched(who);
}
