// afx_kernels_viewmap.hip - the foreshortening and overlap map of a vessel tree over C-arm views (afx_view_map; the definition stands in
// include/afx.h).  Four kernels, every one with integer or per-lane results only:
//   k_vm_zero     zeroes area, shared and tree (the caller hands over uninitialised buffers; count is stored in full by the raster).
//   k_vm_check    a lane per segment: a branch id outside 1..B, a decreasing one or seg_branch[N - 1] != B raises tree[0][3].
//   k_vm_raster   a workgroup is a 16 x 16 pixel tile of one view (four 8 x 8 wavefront tiles).  It walks the segments in chunks of 256:
//                 thread i projects segment chunk + i (the view record is read through the wave-uniform address views + blockIdx.z),
//                 tests the padded box of its capsule against the tile, and the survivors are compacted IN ORDER into an LDS list
//                 (afx::block_exclusive_scan).  After a barrier every pixel walks the list - all lanes read the same LDS address, a
//                 broadcast - and keeps cur (the branch of the run it is in), flag (covered by that branch so far) and cnt in registers,
//                 carried across chunks.  When the list's branch id changes the run ends: cnt += flag, and one lane adds the popcount of
//                 the wavefront's __ballot(flag) to area[v][cur] with one integer atomicAdd.  `shared` needs the final cnt, which every
//                 pixel holds in a register after the walk: the same workgroup walks the segments a second time and ballots
//                 flag && cnt >= 2 - only where some pixel of the tile has cnt >= 2 (__syncthreads_or), which on a vessel tree is a
//                 minority of the tiles.
//   k_vm_foreshortening   a lane per (branch, view), the view fastest so that a wavefront reads one segment and 64 sources; the branch's
//                 segment range is found by two bounded binary searches of the non-decreasing seg_branch; the sums run in segment order.
// NOTHING CAN HANG: no thread of the raster returns before the last barrier (a pixel past W or H stays in with flag = false; the one
// early exit, after the first pass, is taken by the whole workgroup on the value of __syncthreads_or); every loop is bounded by
// n_segments (the searches by 32 steps); no lane waits on another outside __syncthreads.  NOTHING IS INDEXED BY DATA except area and
// shared by the branch id, and a segment whose id lies outside 1..B is dropped before it reaches the list.
#include "afx_internal.h"
#include "afx_geom.h"
#include "afx_scan.h"
#include <cmath>

// every fp64 product, quotient and sum below is rounded on its own (the definition is stated operation by operation)
#pragma clang fp contract(off)

namespace {

constexpr int VM_BLOCK = 256;
constexpr int VM_TILE = 16;
constexpr double VM_CULL_LIMIT = 1073741824.0;        // 2^30: the box test is trusted for coordinates below it

using VmView = afx::ViewRecord;

struct VmSegment {                                    // AFX_VIEWMAP_SEGMENT_DOUBLES = 8
  double p0[3], p1[3], r, pad;
};
static_assert(sizeof(VmSegment) == 8 * AFX_VIEWMAP_SEGMENT_DOUBLES, "the segment record is AFX_VIEWMAP_SEGMENT_DOUBLES doubles");

struct VmArgs {
  const VmSegment* seg;
  const int32_t* branch;
  const VmView* views;
  uint16_t* count;
  int32_t *area, *shared, *tree;
  double half_w, half_h;
  int32_t N, B, V, W, H, brute;
};

__global__ void __launch_bounds__(VM_BLOCK) k_vm_zero(int32_t* __restrict__ area, int32_t* __restrict__ shared, int32_t* __restrict__ tree,
                                                      int64_t n_vb, int64_t n_tree) {
  const int64_t i = (int64_t)blockIdx.x * VM_BLOCK + threadIdx.x;
  if (i < n_vb) area[i] = 0, shared[i] = 0;
  if (i < n_tree) tree[i] = 0;
}

__global__ void __launch_bounds__(VM_BLOCK) k_vm_check(const int32_t* __restrict__ branch, int32_t n, int32_t n_branches, int32_t* __restrict__ tree) {
  const int64_t s = (int64_t)blockIdx.x * VM_BLOCK + threadIdx.x;
  if (s >= n) return;
  const int32_t b = branch[s];
  bool bad = b < 1 || b > n_branches;
  if (s > 0 && branch[s - 1] > b) bad = true;
  if (s == n - 1 && b != n_branches) bad = true;
  if (bad) tree[AFX_VIEWMAP_TREE_BAD] = 1;            // every lane that writes, writes 1
}

// u, w and d of a point: afx::view_camera and afx::view_pixel, as afx_visual_hull projects
__device__ __forceinline__ void vm_project(const VmView& vw, const double* p, double half_w, double half_h, double& u, double& w, double& d) {
  double q0, q1, q2;
  afx::view_camera(vw, p[0], p[1], p[2], q0, q1, q2);
  d = -q2;
  afx::view_pixel(vw, half_w, half_h, q0, q1, d, u, w);
}

__global__ void __launch_bounds__(VM_BLOCK) k_vm_raster(const VmArgs a) {
  __shared__ double s_ax[VM_BLOCK], s_ay[VM_BLOCK], s_gx[VM_BLOCK], s_gy[VM_BLOCK], s_g2[VM_BLOCK], s_rr[VM_BLOCK];
  __shared__ int32_t s_br[VM_BLOCK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t v = blockIdx.z;
  const int32_t tx0 = (int32_t)blockIdx.x * VM_TILE, ty0 = (int32_t)blockIdx.y * VM_TILE;
  const int32_t px = tx0 + (wave & 1) * 8 + (lane & 7), py = ty0 + (wave >> 1) * 8 + (lane >> 3);
  const bool inside = px < a.W && py < a.H;
  const double fx = (double)px, fy = (double)py;
  // the tile's pixel centres, clipped to the detector
  const double bx0 = (double)tx0, by0 = (double)ty0;
  const double bx1 = (double)(tx0 + VM_TILE - 1 < a.W - 1 ? tx0 + VM_TILE - 1 : a.W - 1);
  const double by1 = (double)(ty0 + VM_TILE - 1 < a.H - 1 ? ty0 + VM_TILE - 1 : a.H - 1);
  const bool tally_segments = blockIdx.x == 0 && blockIdx.y == 0;      // one tile per view counts the invisible segments
  const VmView& vw = a.views[v];                      // the same address in every lane
  const size_t row = (size_t)v * (size_t)a.B;
  uint32_t cnt = 0;
  bool multi = false;
  for (int pass = 0; pass < 2; ++pass) {
    int32_t* const tally = pass == 0 ? a.area : a.shared;
    int32_t cur = 0;                                  // the branch of the current run; 0: none yet
    bool flag = false;
    for (int32_t chunk = 0; chunk < a.N; chunk += VM_BLOCK) {
      const int32_t s = chunk + tid;
      int32_t keep = 0, br = 0;
      bool invisible = false;
      double ax = 0.0, ay = 0.0, gx = 0.0, gy = 0.0, g2 = 0.0, rr = 0.0;
      if (s < a.N) {
        const VmSegment& sg = a.seg[s];
        double u0, w0, d0, u1, w1, d1;
        vm_project(vw, sg.p0, a.half_w, a.half_h, u0, w0, d0);
        vm_project(vw, sg.p1, a.half_w, a.half_h, u1, w1, d1);
        const bool visible = d0 > 0.0 && d1 > 0.0;
        invisible = !visible;
        br = a.branch[s];
        if (visible && br >= 1 && br <= a.B) {
          const double rho = (vw.f * sg.r) / (0.5 * (d0 + d1));
          ax = u0, ay = w0;
          gx = u1 - u0, gy = w1 - w0;
          g2 = gx * gx + gy * gy;
          rr = rho * rho;
          // The cull: the box of the two end points padded by rho + 1 misses the tile's pixel centres.  Trusted only where every
          // number is below 2^30 in size (a NaN fails the test and is kept: it covers nothing either way).
          const double pad = rho + 1.0;
          const double lo_x = (u0 < u1 ? u0 : u1) - pad, hi_x = (u0 > u1 ? u0 : u1) + pad;
          const double lo_y = (w0 < w1 ? w0 : w1) - pad, hi_y = (w0 > w1 ? w0 : w1) + pad;
          const bool small = fabs(u0) < VM_CULL_LIMIT && fabs(u1) < VM_CULL_LIMIT && fabs(w0) < VM_CULL_LIMIT && fabs(w1) < VM_CULL_LIMIT &&
                             rho < VM_CULL_LIMIT;
          const bool misses = hi_x < bx0 || lo_x > bx1 || hi_y < by0 || lo_y > by1;
          keep = (a.brute || !small || !misses) ? 1 : 0;
        }
      }
      if (pass == 0 && tally_segments) {              // uniform over the workgroup
        const unsigned long long m = __ballot(invisible);
        if (lane == 0 && m) atomicAdd(&a.tree[4 * (size_t)v + AFX_VIEWMAP_TREE_INVISIBLE], (int32_t)__popcll(m));
      }
      int32_t pos[1] = {keep}, total[1];
      afx::block_exclusive_scan<VM_BLOCK, int32_t, 1>(pos, total);      // its barriers stand between the last walk and these stores
      if (keep) {
        const int32_t q = pos[0];
        s_ax[q] = ax, s_ay[q] = ay, s_gx[q] = gx, s_gy[q] = gy, s_g2[q] = g2, s_rr[q] = rr, s_br[q] = br;
      }
      __syncthreads();
      for (int32_t j = 0; j < total[0]; ++j) {        // total and the list are the same in every lane
        const int32_t b = s_br[j];
        if (b != cur) {
          if (cur) {
            const bool mine = pass == 0 ? flag : (flag && multi);
            const unsigned long long m = __ballot(mine);
            if (pass == 0) cnt += flag ? 1u : 0u;
            if (lane == 0 && m) atomicAdd(&tally[row + (size_t)(cur - 1)], (int32_t)__popcll(m));
          }
          cur = b, flag = false;
        }
        const double lx = s_gx[j], ly = s_gy[j], l2 = s_g2[j];
        const double hx = fx - s_ax[j], hy = fy - s_ay[j];
        double t = l2 > 0.0 ? (hx * lx + hy * ly) / l2 : 0.0;
        if (t < 0.0) t = 0.0;
        if (t > 1.0) t = 1.0;
        const double ex = hx - t * lx, ey = hy - t * ly;
        if (inside && ex * ex + ey * ey <= s_rr[j]) flag = true;
      }
    }
    if (cur) {                                        // the last run
      const bool mine = pass == 0 ? flag : (flag && multi);
      const unsigned long long m = __ballot(mine);
      if (pass == 0) cnt += flag ? 1u : 0u;
      if (lane == 0 && m) atomicAdd(&tally[row + (size_t)(cur - 1)], (int32_t)__popcll(m));
    }
    if (pass == 0) {
      if (inside) a.count[((size_t)v * (size_t)a.H + (size_t)py) * (size_t)a.W + (size_t)px] = (uint16_t)cnt;      // cnt <= B <= 65 535
      multi = cnt >= 2;
      const unsigned long long m1 = __ballot(cnt >= 1), m2 = __ballot(multi);
      if (lane == 0 && m1) atomicAdd(&a.tree[4 * (size_t)v + AFX_VIEWMAP_TREE_UNION], (int32_t)__popcll(m1));
      if (lane == 0 && m2) atomicAdd(&a.tree[4 * (size_t)v + AFX_VIEWMAP_TREE_MULTI], (int32_t)__popcll(m2));
      if (!__syncthreads_or(multi ? 1 : 0)) break;    // the whole workgroup: no pixel of the tile is shared
    }
  }
}

// the first segment whose branch id is >= b (n: none): at most 32 halvings of [0, n]
__device__ __forceinline__ int32_t vm_lower_bound(const int32_t* __restrict__ branch, int32_t n, int32_t b) {
  int32_t lo = 0, hi = n;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (branch[mid] < b) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(VM_BLOCK) k_vm_foreshortening(const VmSegment* __restrict__ seg, const int32_t* __restrict__ branch, int32_t n,
                                                                int32_t n_branches, const VmView* __restrict__ views, int32_t n_views,
                                                                double* __restrict__ proj, double* __restrict__ length) {
  const int64_t i = (int64_t)blockIdx.x * VM_BLOCK + threadIdx.x;
  if (i >= (int64_t)n_views * n_branches) return;
  const int32_t v = (int32_t)(i % n_views), b = (int32_t)(i / n_views);      // the view fastest
  const int32_t s0 = vm_lower_bound(branch, n, b + 1);
  int32_t s1 = vm_lower_bound(branch, n, b + 2);
  if (s1 < s0) s1 = s0;                               // (a seg_branch that decreases: the call's flag is up; the loop stays bounded)
  const double c0 = views[v].c[0], c1 = views[v].c[1], c2 = views[v].c[2];
  double sum_perp = 0.0, sum_len = 0.0;
  for (int32_t s = s0; s < s1; ++s) {
    const VmSegment& sg = seg[s];
    const double l0 = sg.p1[0] - sg.p0[0], l1 = sg.p1[1] - sg.p0[1], l2c = sg.p1[2] - sg.p0[2];
    const double e0 = (sg.p0[0] - c0) + (sg.p1[0] - c0), e1 = (sg.p0[1] - c1) + (sg.p1[1] - c1), e2 = (sg.p0[2] - c2) + (sg.p1[2] - c2);
    const double n2 = (e0 * e0 + e1 * e1) + e2 * e2;
    const double le = (l0 * e0 + l1 * e1) + l2c * e2;
    const double l2 = (l0 * l0 + l1 * l1) + l2c * l2c;
    const double perp2 = l2 - (le * le) / n2;
    sum_perp = sum_perp + sqrt(perp2 > 0.0 ? perp2 : 0.0);
    sum_len = sum_len + sqrt(l2);
  }
  if (proj) proj[(size_t)v * (size_t)n_branches + (size_t)b] = sum_perp;
  if (length && v == 0) length[b] = sum_len;
}

}  // namespace

extern "C" int afx_view_map(const double* segments, const int32_t* seg_branch, int32_t n_segments, int32_t n_branches, const double* views,
                            int32_t n_views, int32_t width, int32_t height, uint32_t flags, uint16_t* count, int32_t* area, int32_t* shared,
                            int32_t* tree, double* proj, double* length, void* stream) {
  const char* who = "afx_view_map";
  if (!segments) return afx::set_error(AFX_E_INVALID, who, "null segments");
  if (!seg_branch) return afx::set_error(AFX_E_INVALID, who, "null seg_branch");
  if (!views) return afx::set_error(AFX_E_INVALID, who, "null views");
  const int n_raster = (count != nullptr) + (area != nullptr) + (shared != nullptr) + (tree != nullptr);
  if (n_raster != 0 && n_raster != 4) return afx::set_error(AFX_E_INVALID, who, "count, area, shared and tree are given together or not at all");
  if (n_raster == 0 && !proj && !length) return afx::set_error(AFX_E_INVALID, who, "no output: count, area, shared, tree, proj and length are all null");
  if (n_views < 1 || n_views > 65535) return afx::set_error(AFX_E_INVALID, who, "n_views must lie in 1..65535");
  if (n_segments < 1 || n_segments > (1 << 30)) return afx::set_error(AFX_E_INVALID, who, "n_segments must lie in 1..2^30");
  if (n_branches < 1 || n_branches > 65535) return afx::set_error(AFX_E_INVALID, who, "n_branches must lie in 1..65535");
  if (width < 1 || height < 1 || width > 16384 || height > 16384)
    return afx::set_error(AFX_E_INVALID, who, "width and height must lie in 1..16384");
  if (flags & ~(uint32_t)AFX_VIEWMAP_BRUTE) return afx::set_error(AFX_E_INVALID, who, "unknown bits in flags");
  if (int rc = afx::check_device_memory(segments, "segments", who)) return rc;
  if (int rc = afx::check_device_memory(seg_branch, "seg_branch", who)) return rc;
  if (int rc = afx::check_device_memory(views, "views", who)) return rc;
  if (n_raster) {
    if (int rc = afx::check_device_memory(count, "count", who)) return rc;
    if (int rc = afx::check_device_memory(area, "area", who)) return rc;
    if (int rc = afx::check_device_memory(shared, "shared", who)) return rc;
    if (int rc = afx::check_device_memory(tree, "tree", who)) return rc;
  }
  if (proj)
    if (int rc = afx::check_device_memory(proj, "proj", who)) return rc;
  if (length)
    if (int rc = afx::check_device_memory(length, "length", who)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_vb = (int64_t)n_views * n_branches;
  if (n_raster) {
    const int64_t n_tree = 4 * (int64_t)n_views, n_zero = n_vb > n_tree ? n_vb : n_tree;
    hipLaunchKernelGGL(k_vm_zero, dim3((unsigned)((n_zero + VM_BLOCK - 1) / VM_BLOCK)), dim3(VM_BLOCK), 0, st, area, shared, tree, n_vb, n_tree);
    hipLaunchKernelGGL(k_vm_check, dim3((unsigned)(((int64_t)n_segments + VM_BLOCK - 1) / VM_BLOCK)), dim3(VM_BLOCK), 0, st, seg_branch,
                       n_segments, n_branches, tree);
    VmArgs a;
    a.seg = (const VmSegment*)segments, a.branch = seg_branch, a.views = (const VmView*)views;
    a.count = count, a.area = area, a.shared = shared, a.tree = tree;
    a.half_w = (double)width / 2.0, a.half_h = (double)height / 2.0;
    a.N = n_segments, a.B = n_branches, a.V = n_views, a.W = width, a.H = height, a.brute = (flags & AFX_VIEWMAP_BRUTE) ? 1 : 0;
    const dim3 grid((unsigned)((width + VM_TILE - 1) / VM_TILE), (unsigned)((height + VM_TILE - 1) / VM_TILE), (unsigned)n_views);
    hipLaunchKernelGGL(k_vm_raster, grid, dim3(VM_BLOCK), 0, st, a);
  }
  if (proj || length)
    hipLaunchKernelGGL(k_vm_foreshortening, dim3((unsigned)((n_vb + VM_BLOCK - 1) / VM_BLOCK)), dim3(VM_BLOCK), 0, st, (const VmSegment*)segments,
                       seg_branch, n_segments, n_branches, (const VmView*)views, n_views, proj, length);
  return afx::launched(who);
}
