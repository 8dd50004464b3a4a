// afx_kernels_pose.hip - rigid 2D-3D registration of C-arm poses: the chamfer cost of a point set (the vessel centreline) against one
// distance image per view, its Gauss-Newton normal equations, the Levenberg-Marquardt step and the coarse search's selection
// (afx_pose_chamfer, afx_pose_compose, afx_pose_select, afx_pose_lm_step; the definition stands in include/afx.h).  Four kernels:
//   k_pose_chamfer   grid (S, K), 256 threads: the workgroup is slice s of record k.  The record is read through the wave-uniform
//                    address records + k (scalar loads); thread t takes the slice's points t, t + 256, ... in ascending order into 30
//                    fp64 accumulators and 4 counters in registers.  The 256 thread values meet in the adjacent-pair tree: six
//                    __shfl_xor levels inside a wavefront (lane i adds lane i ^ m: both lanes of a pair form the same sum, fp64 addition
//                    commutes, so every lane ends with the tree's value of its wavefront), then the four wave totals through
//                    4 x 30 doubles of LDS as (w0 + w1) + (w2 + w3).  No 256 x 30 array.
//   k_pose_compose   a lane per output record.
//   k_pose_select    a lane per view: the candidate of lowest cost, ties to the lowest index.
//   k_pose_lm_step   a lane per view: adds the slices, accepts or rejects the trial, solves the damped 6 x 6 system, composes the trial.
// NOTHING CAN HANG: no thread of k_pose_chamfer leaves before the last barrier (a record whose view index is out of range is dropped by
// the whole workgroup, on a wave-uniform value, and still reaches the store); every loop is bounded by N, S, M or 6.  NOTHING IS INDEXED
// BY DATA except the field, by indices that are clamped to the detector as doubles before they become integers, and the view, which is
// range-checked first.  No atomics, no allocation, no synchronisation.
#include "afx_internal.h"
#include "afx_geom.h"
#include <cmath>

// every fp64 product, quotient and sum below is rounded on its own (the definition is stated operation by operation)
#pragma clang fp contract(off)

namespace {

constexpr int POSE_BLOCK = 256;
constexpr int POSE_WAVES = POSE_BLOCK / 64;
constexpr int POSE_ACC = 30;                          // cost, sum r, sum w, g[6], H[21]

using PoseRecord = afx::ViewRecord;

struct PoseArgs {
  const double* field;
  const double* points;
  const double* radius;
  const double* weight;
  const PoseRecord* records;
  const int32_t* rec_view;
  double* sums;
  int32_t* counts;
  double trunc, half_w, half_h, max_u, max_w;
  int64_t slice_len;
  int32_t N, V, W, H, cost_only;
};

// compose(rec, xi): R' = R C(a)^T, c' = c - R' t; xi = 0 in all six returns the record as it is
__device__ __forceinline__ void pose_compose(const double* __restrict__ rec, const double* __restrict__ xi, double* __restrict__ out) {
  const double a0 = xi[0], a1 = xi[1], a2 = xi[2], t0 = xi[3], t1 = xi[4], t2 = xi[5];
  if (a0 == 0.0 && a1 == 0.0 && a2 == 0.0 && t0 == 0.0 && t1 == 0.0 && t2 == 0.0) {
    for (int i = 0; i < AFX_HULL_VIEW_DOUBLES; ++i) out[i] = rec[i];
    return;
  }
  const double n = (a0 * a0 + a1 * a1) + a2 * a2;
  const double s = 1.0 - n, den = 1.0 + n;
  double c[9];
  c[0] = (s + 2.0 * (a0 * a0)) / den, c[1] = (2.0 * (a0 * a1) - 2.0 * a2) / den, c[2] = (2.0 * (a0 * a2) + 2.0 * a1) / den;
  c[3] = (2.0 * (a0 * a1) + 2.0 * a2) / den, c[4] = (s + 2.0 * (a1 * a1)) / den, c[5] = (2.0 * (a1 * a2) - 2.0 * a0) / den;
  c[6] = (2.0 * (a0 * a2) - 2.0 * a1) / den, c[7] = (2.0 * (a1 * a2) + 2.0 * a0) / den, c[8] = (s + 2.0 * (a2 * a2)) / den;
  double rn[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) rn[3 * i + j] = (rec[3 * i] * c[3 * j] + rec[3 * i + 1] * c[3 * j + 1]) + rec[3 * i + 2] * c[3 * j + 2];
  const double cc[3] = {rec[9], rec[10], rec[11]};
  for (int i = 0; i < 9; ++i) out[i] = rn[i];
  for (int i = 0; i < 3; ++i) out[9 + i] = cc[i] - ((rn[3 * i] * t0 + rn[3 * i + 1] * t1) + rn[3 * i + 2] * t2);
  for (int i = 12; i < AFX_HULL_VIEW_DOUBLES; ++i) out[i] = rec[i];
}

__global__ void __launch_bounds__(POSE_BLOCK) k_pose_chamfer(const PoseArgs a) {
  __shared__ double s_acc[POSE_WAVES][POSE_ACC];
  __shared__ int32_t s_cnt[POSE_WAVES][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t s = blockIdx.x, k = blockIdx.y;
  const int32_t v = a.rec_view[k];                    // the same address in every lane
  const bool dropped = v < 0 || v >= a.V;             // uniform over the workgroup
  double acc[POSE_ACC];
#pragma unroll
  for (int j = 0; j < POSE_ACC; ++j) acc[j] = 0.0;
  int32_t cnt[4] = {0, 0, 0, 0};
  if (!dropped) {
    const PoseRecord& rc = a.records[k];              // the same address in every lane
    const double* const fld = a.field + (size_t)v * (size_t)a.H * (size_t)a.W;
    const int64_t lo = (int64_t)s * a.slice_len;
    const int64_t hi = lo + a.slice_len < (int64_t)a.N ? lo + a.slice_len : (int64_t)a.N;
    for (int64_t i = lo + tid; i < hi; i += POSE_BLOCK) {
      double q0, q1, q2;                              // q, su and sw enter the Jacobian below: the pixel is formed here, not by afx::view_pixel
      afx::view_camera(rc, a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2], q0, q1, q2);
      const double d = -q2;
      const double su = (rc.f * q0) / d, sw = (rc.f * q1) / d;
      const double u = a.half_w + su, w = a.half_h - sw;
      const bool ok = d > 0.0 && u >= 0.0 && u <= a.max_u && w >= 0.0 && w <= a.max_w;      // a NaN is lost
      const double wt = a.weight ? a.weight[i] : 1.0;
      double r = a.trunc;
      int kind = 3;
      if (ok) {
        double fu = floor(u), fw = floor(w);          // 0 <= u <= W - 1 and 0 <= w <= H - 1 hold here: clamped before they are integers
        fu = fu < a.max_u - 1.0 ? fu : a.max_u - 1.0;
        fw = fw < a.max_w - 1.0 ? fw : a.max_w - 1.0;
        const int32_t iu = (int32_t)fu, iw = (int32_t)fw;
        const double pu = u - fu, pw = w - fw;
        const double* const row = fld + (size_t)iw * (size_t)a.W + (size_t)iu;
        const double f00 = row[0], f01 = row[1], f10 = row[a.W], f11 = row[a.W + 1];
        const double ga = f01 - f00, gb = f11 - f10;
        const double top = f00 + pu * ga, bot = f10 + pu * gb;
        const double gw = bot - top;
        const double val = top + pw * gw;
        const double gu = ga + pw * (gb - ga);
        const double rad = a.radius ? a.radius[i] : 0.0;
        const double err = val + (rc.f * rad) / d;
        if (err <= 0.0) {
          r = 0.0, kind = 1;
        } else if (err >= a.trunc) {
          kind = 2;
        } else {
          r = err, kind = 0;
          if (!a.cost_only) {
            const double fd = rc.f / d;
            double J[6];
            J[3] = gu * fd;
            J[4] = -(gw * fd);
            J[5] = (gu * su - gw * sw) / d;
            J[0] = 2.0 * (q1 * J[5] - q2 * J[4]);
            J[1] = 2.0 * (q2 * J[3] - q0 * J[5]);
            J[2] = 2.0 * (q0 * J[4] - q1 * J[3]);
            double wj[6];
#pragma unroll
            for (int p = 0; p < 6; ++p) wj[p] = wt * J[p];
#pragma unroll
            for (int p = 0; p < 6; ++p) acc[3 + p] = acc[3 + p] + wj[p] * r;
            int n = 9;
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
              for (int l = p; l < 6; ++l, ++n) acc[n] = acc[n] + wj[p] * J[l];
          }
        }
      }
      const double wr = wt * r;
      acc[0] = acc[0] + wr * r;
      acc[1] = acc[1] + wr;
      acc[2] = acc[2] + wt;
      cnt[0] += kind == 0, cnt[1] += kind == 1, cnt[2] += kind == 2, cnt[3] += kind == 3;
    }
  }
  // the adjacent-pair tree over the 256 thread values: levels 1..6 inside the wavefront
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
    for (int j = 0; j < POSE_ACC; ++j) acc[j] = acc[j] + __shfl_xor(acc[j], m, 64);
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt[j] += __shfl_xor(cnt[j], m, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < POSE_ACC; ++j) s_acc[wave][j] = acc[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) s_cnt[wave][j] = cnt[j];
  }
  __syncthreads();                                    // the last barrier: every thread of the workgroup reaches it
  const size_t slot = (size_t)k * gridDim.x + (size_t)s;
  if (tid < AFX_POSE_SUM_DOUBLES) {
    double out = 0.0;                                 // [30], [31]
    if (tid < POSE_ACC) out = (s_acc[0][tid] + s_acc[1][tid]) + (s_acc[2][tid] + s_acc[3][tid]);
    if (dropped) out = tid == 0 ? HUGE_VAL : 0.0;
    a.sums[slot * AFX_POSE_SUM_DOUBLES + tid] = out;
  } else if (tid >= 64 && tid < 68) {
    const int j = tid - 64;
    a.counts[slot * 4 + j] = dropped ? -1 : (s_cnt[0][j] + s_cnt[1][j]) + (s_cnt[2][j] + s_cnt[3][j]);
  }
}

__global__ void __launch_bounds__(POSE_BLOCK) k_pose_compose(const double* __restrict__ records, int32_t n_records, const double* __restrict__ xi,
                                                             int32_t n_xi, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * POSE_BLOCK + threadIdx.x;
  const int64_t total = n_xi > 0 ? (int64_t)n_records * n_xi : (int64_t)n_records;
  if (i >= total) return;
  const int64_t r = n_xi > 0 ? i / n_xi : i, x = n_xi > 0 ? i % n_xi : i;
  double rec[AFX_HULL_VIEW_DOUBLES], inc[6], res[AFX_HULL_VIEW_DOUBLES];
  for (int j = 0; j < AFX_HULL_VIEW_DOUBLES; ++j) rec[j] = records[r * AFX_HULL_VIEW_DOUBLES + j];
  for (int j = 0; j < 6; ++j) inc[j] = xi[x * 6 + j];
  pose_compose(rec, inc, res);
  for (int j = 0; j < AFX_HULL_VIEW_DOUBLES; ++j) out[i * AFX_HULL_VIEW_DOUBLES + j] = res[j];
}

__global__ void __launch_bounds__(POSE_BLOCK) k_pose_select(const double* __restrict__ sums, int32_t n_views, int32_t n_candidates, int32_t n_slices,
                                                            const double* __restrict__ cand, int32_t* __restrict__ selected,
                                                            double* __restrict__ records_out) {
  const int64_t v = (int64_t)blockIdx.x * POSE_BLOCK + threadIdx.x;
  if (v >= n_views) return;
  int32_t best = 0;
  double best_cost = 0.0;
  for (int32_t m = 0; m < n_candidates; ++m) {
    const double* p = sums + ((size_t)v * n_candidates + m) * (size_t)n_slices * AFX_POSE_SUM_DOUBLES;
    double cost = 0.0;
    for (int32_t s = 0; s < n_slices; ++s) cost = cost + p[(size_t)s * AFX_POSE_SUM_DOUBLES];
    if (m == 0 || cost < best_cost) best = m, best_cost = cost;
  }
  selected[v] = best;
  if (records_out)
    for (int j = 0; j < AFX_HULL_VIEW_DOUBLES; ++j)
      records_out[v * AFX_HULL_VIEW_DOUBLES + j] = cand[((size_t)v * n_candidates + best) * AFX_HULL_VIEW_DOUBLES + j];
}

// (H + lambda diag H) delta = -g by Cholesky, in the order include/afx.h states; false: a pivot is not > 0 and delta = 0
__device__ __forceinline__ bool pose_solve(const double* __restrict__ g, const double* __restrict__ h, double lambda, uint32_t dof, double* delta) {
  double A[6][6], b[6], L[6][6];
  int n = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int l = k; l < 6; ++l, ++n) A[k][l] = h[n], A[l][k] = h[n];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    if (!((dof >> k) & 1u)) {
#pragma unroll
      for (int l = 0; l < 6; ++l) A[k][l] = 0.0, A[l][k] = 0.0;
      A[k][k] = 1.0, b[k] = 0.0;
    } else {
      A[k][k] = A[k][k] + lambda * A[k][k];
      b[k] = -g[k];
    }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
#pragma unroll
    for (int p = 0; p < j; ++p) s = s - L[j][p] * L[j][p];
    if (!(s > 0.0)) ok = false;
    L[j][j] = sqrt(s);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i][j];
#pragma unroll
      for (int p = 0; p < j; ++p) t = t - L[i][p] * L[j][p];
      L[i][j] = t / L[j][j];
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double t = b[i];
#pragma unroll
    for (int p = 0; p < i; ++p) t = t - L[i][p] * y[p];
    y[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double t = y[i];
#pragma unroll
    for (int p = i + 1; p < 6; ++p) t = t - L[p][i] * delta[p];
    delta[i] = t / L[i][i];
  }
  if (!ok)                                            // the first failing pivot ends the factorisation: whatever followed it is dropped
#pragma unroll
    for (int i = 0; i < 6; ++i) delta[i] = 0.0;
  return ok;
}

__global__ void __launch_bounds__(POSE_BLOCK) k_pose_lm_step(double* __restrict__ state, int32_t n_views, const double* __restrict__ sums,
                                                             int32_t n_slices, int32_t phase, uint32_t dof, double lambda0,
                                                             const double* __restrict__ records_in, double* __restrict__ trial_records) {
  const int64_t v = (int64_t)blockIdx.x * POSE_BLOCK + threadIdx.x;
  if (v >= n_views) return;
  double* const st = state + v * AFX_POSE_STATE_DOUBLES;
  double tot[POSE_ACC];
#pragma unroll
  for (int j = 0; j < POSE_ACC; ++j) tot[j] = 0.0;
  for (int32_t s = 0; s < n_slices; ++s) {
    const double* p = sums + ((size_t)v * n_slices + s) * AFX_POSE_SUM_DOUBLES;
#pragma unroll
    for (int j = 0; j < POSE_ACC; ++j) tot[j] = tot[j] + p[j];
  }
  bool take = false;
  if (phase == AFX_POSE_LM_INIT) {
    for (int j = 0; j < AFX_POSE_STATE_DOUBLES; ++j) st[j] = 0.0;
    for (int j = 0; j < AFX_HULL_VIEW_DOUBLES; ++j) st[AFX_POSE_ST_RECORD + j] = records_in[v * AFX_HULL_VIEW_DOUBLES + j];
    st[AFX_POSE_ST_LAMBDA] = lambda0;
    take = true;
  } else if (tot[0] < st[AFX_POSE_ST_COST]) {
    for (int j = 0; j < AFX_HULL_VIEW_DOUBLES; ++j) st[AFX_POSE_ST_RECORD + j] = st[AFX_POSE_ST_TRIAL + j];
    const double l = st[AFX_POSE_ST_LAMBDA] / 3.0;
    st[AFX_POSE_ST_LAMBDA] = l > 1e-12 ? l : 1e-12;
    st[AFX_POSE_ST_ACCEPTED] = st[AFX_POSE_ST_ACCEPTED] + 1.0;
    take = true;
  } else {
    const double l = 4.0 * st[AFX_POSE_ST_LAMBDA];
    st[AFX_POSE_ST_LAMBDA] = l < 1e12 ? l : 1e12;
    st[AFX_POSE_ST_REJECTED] = st[AFX_POSE_ST_REJECTED] + 1.0;
  }
  if (take) {
    st[AFX_POSE_ST_COST] = tot[0];
#pragma unroll
    for (int j = 0; j < 6; ++j) st[AFX_POSE_ST_G + j] = tot[3 + j];
#pragma unroll
    for (int j = 0; j < 21; ++j) st[AFX_POSE_ST_H + j] = tot[9 + j];
  }
  double cur[AFX_HULL_VIEW_DOUBLES], trial[AFX_HULL_VIEW_DOUBLES];
  for (int j = 0; j < AFX_HULL_VIEW_DOUBLES; ++j) cur[j] = st[AFX_POSE_ST_RECORD + j];
  if (phase == AFX_POSE_LM_FINAL) {
    for (int j = 0; j < AFX_HULL_VIEW_DOUBLES; ++j) trial[j] = cur[j];
  } else {
    double g[6], h[21], delta[6];
    for (int j = 0; j < 6; ++j) g[j] = st[AFX_POSE_ST_G + j];
    for (int j = 0; j < 21; ++j) h[j] = st[AFX_POSE_ST_H + j];
    if (!pose_solve(g, h, st[AFX_POSE_ST_LAMBDA], dof, delta)) st[AFX_POSE_ST_SINGULAR] = st[AFX_POSE_ST_SINGULAR] + 1.0;
    pose_compose(cur, delta, trial);
  }
  for (int j = 0; j < AFX_HULL_VIEW_DOUBLES; ++j) st[AFX_POSE_ST_TRIAL + j] = trial[j], trial_records[v * AFX_HULL_VIEW_DOUBLES + j] = trial[j];
}

inline unsigned pose_blocks(int64_t n) { return (unsigned)((n + POSE_BLOCK - 1) / POSE_BLOCK); }

}  // namespace

extern "C" int afx_pose_chamfer(const double* field, int32_t n_views, int32_t width, int32_t height, const double* points, const double* radius,
                                const double* weight, int32_t n_points, const double* records, const int32_t* rec_view, int32_t n_records,
                                double trunc, int32_t n_slices, uint32_t flags, double* sums, int32_t* counts, void* stream) {
  const char* who = "afx_pose_chamfer";
  if (!field) return afx::set_error(AFX_E_INVALID, who, "null field");
  if (!points) return afx::set_error(AFX_E_INVALID, who, "null points");
  if (!records) return afx::set_error(AFX_E_INVALID, who, "null records");
  if (!rec_view) return afx::set_error(AFX_E_INVALID, who, "null rec_view");
  if (!sums) return afx::set_error(AFX_E_INVALID, who, "null sums");
  if (!counts) return afx::set_error(AFX_E_INVALID, who, "null counts");
  if (n_views < 1 || n_views > 65535) return afx::set_error(AFX_E_INVALID, who, "n_views must lie in 1..65535");
  if (width < 2 || height < 2 || width > 16384 || height > 16384) return afx::set_error(AFX_E_INVALID, who, "width and height must lie in 2..16384");
  if (n_points < 1 || n_points > (1 << 30)) return afx::set_error(AFX_E_INVALID, who, "n_points must lie in 1..2^30");
  if (n_records < 1 || n_records > 65535) return afx::set_error(AFX_E_INVALID, who, "n_records must lie in 1..65535");
  if (n_slices < 1 || n_slices > 4096) return afx::set_error(AFX_E_INVALID, who, "n_slices must lie in 1..4096");
  if (!(trunc > 0.0) || !std::isfinite(trunc)) return afx::set_error(AFX_E_INVALID, who, "trunc must be finite and > 0");
  if (flags & ~(uint32_t)AFX_POSE_COST_ONLY) return afx::set_error(AFX_E_INVALID, who, "unknown bits in flags");
  if (int rc = afx::check_device_memory(field, "field", who)) return rc;
  if (int rc = afx::check_device_memory(points, "points", who)) return rc;
  if (radius)
    if (int rc = afx::check_device_memory(radius, "radius", who)) return rc;
  if (weight)
    if (int rc = afx::check_device_memory(weight, "weight", who)) return rc;
  if (int rc = afx::check_device_memory(records, "records", who)) return rc;
  if (int rc = afx::check_device_memory(rec_view, "rec_view", who)) return rc;
  if (int rc = afx::check_device_memory(sums, "sums", who)) return rc;
  if (int rc = afx::check_device_memory(counts, "counts", who)) return rc;
  PoseArgs a;
  a.field = field, a.points = points, a.radius = radius, a.weight = weight, a.records = (const PoseRecord*)records, a.rec_view = rec_view;
  a.sums = sums, a.counts = counts, a.trunc = trunc;
  a.half_w = (double)width / 2.0, a.half_h = (double)height / 2.0, a.max_u = (double)(width - 1), a.max_w = (double)(height - 1);
  const int64_t per = ((int64_t)n_points + n_slices - 1) / n_slices;
  a.slice_len = (per + POSE_BLOCK - 1) / POSE_BLOCK * POSE_BLOCK;
  a.N = n_points, a.V = n_views, a.W = width, a.H = height, a.cost_only = (flags & AFX_POSE_COST_ONLY) ? 1 : 0;
  hipLaunchKernelGGL(k_pose_chamfer, dim3((unsigned)n_slices, (unsigned)n_records), dim3(POSE_BLOCK), 0, (hipStream_t)stream, a);
  return afx::launched(who);
}

extern "C" int afx_pose_compose(const double* records, int32_t n_records, const double* xi, int32_t n_xi, double* out, void* stream) {
  const char* who = "afx_pose_compose";
  if (!records) return afx::set_error(AFX_E_INVALID, who, "null records");
  if (!xi) return afx::set_error(AFX_E_INVALID, who, "null xi");
  if (!out) return afx::set_error(AFX_E_INVALID, who, "null out");
  if (n_records < 1 || n_records > 65535) return afx::set_error(AFX_E_INVALID, who, "n_records must lie in 1..65535");
  if (n_xi < 0 || n_xi > 65535) return afx::set_error(AFX_E_INVALID, who, "n_xi must lie in 0..65535");
  if (int rc = afx::check_device_memory(records, "records", who)) return rc;
  if (int rc = afx::check_device_memory(xi, "xi", who)) return rc;
  if (int rc = afx::check_device_memory(out, "out", who)) return rc;
  const int64_t total = n_xi > 0 ? (int64_t)n_records * n_xi : (int64_t)n_records;
  hipLaunchKernelGGL(k_pose_compose, dim3(pose_blocks(total)), dim3(POSE_BLOCK), 0, (hipStream_t)stream, records, n_records, xi, n_xi, out);
  return afx::launched(who);
}

extern "C" int afx_pose_select(const double* sums, int32_t n_views, int32_t n_candidates, int32_t n_slices, const double* cand_records,
                               int32_t* selected, double* records_out, void* stream) {
  const char* who = "afx_pose_select";
  if (!sums) return afx::set_error(AFX_E_INVALID, who, "null sums");
  if (!selected) return afx::set_error(AFX_E_INVALID, who, "null selected");
  if (records_out && !cand_records) return afx::set_error(AFX_E_INVALID, who, "records_out needs cand_records");
  if (n_views < 1 || n_views > 65535) return afx::set_error(AFX_E_INVALID, who, "n_views must lie in 1..65535");
  if (n_candidates < 1 || n_candidates > 65535) return afx::set_error(AFX_E_INVALID, who, "n_candidates must lie in 1..65535");
  if (n_slices < 1 || n_slices > 4096) return afx::set_error(AFX_E_INVALID, who, "n_slices must lie in 1..4096");
  if (int rc = afx::check_device_memory(sums, "sums", who)) return rc;
  if (int rc = afx::check_device_memory(selected, "selected", who)) return rc;
  if (records_out) {
    if (int rc = afx::check_device_memory(cand_records, "cand_records", who)) return rc;
    if (int rc = afx::check_device_memory(records_out, "records_out", who)) return rc;
  }
  hipLaunchKernelGGL(k_pose_select, dim3(pose_blocks(n_views)), dim3(POSE_BLOCK), 0, (hipStream_t)stream, sums, n_views, n_candidates, n_slices,
                     cand_records, selected, records_out);
  return afx::launched(who);
}

extern "C" int afx_pose_lm_step(double* state, int32_t n_views, const double* sums, int32_t n_slices, int32_t phase, uint32_t dof_mask,
                                double lambda0, const double* records_in, double* trial_records, void* stream) {
  const char* who = "afx_pose_lm_step";
  if (!state) return afx::set_error(AFX_E_INVALID, who, "null state");
  if (!sums) return afx::set_error(AFX_E_INVALID, who, "null sums");
  if (!trial_records) return afx::set_error(AFX_E_INVALID, who, "null trial_records");
  if (phase != AFX_POSE_LM_INIT && phase != AFX_POSE_LM_UPDATE && phase != AFX_POSE_LM_FINAL)
    return afx::set_error(AFX_E_INVALID, who, "phase must be AFX_POSE_LM_INIT, AFX_POSE_LM_UPDATE or AFX_POSE_LM_FINAL");
  if (phase == AFX_POSE_LM_INIT && !records_in) return afx::set_error(AFX_E_INVALID, who, "null records_in (AFX_POSE_LM_INIT)");
  if (n_views < 1 || n_views > 65535) return afx::set_error(AFX_E_INVALID, who, "n_views must lie in 1..65535");
  if (n_slices < 1 || n_slices > 4096) return afx::set_error(AFX_E_INVALID, who, "n_slices must lie in 1..4096");
  if (dof_mask > 63u) return afx::set_error(AFX_E_INVALID, who, "dof_mask must lie in 0..63");
  if (!(lambda0 > 0.0) || !std::isfinite(lambda0)) return afx::set_error(AFX_E_INVALID, who, "lambda0 must be finite and > 0");
  if (int rc = afx::check_device_memory(state, "state", who)) return rc;
  if (int rc = afx::check_device_memory(sums, "sums", who)) return rc;
  if (int rc = afx::check_device_memory(trial_records, "trial_records", who)) return rc;
  if (phase == AFX_POSE_LM_INIT)
    if (int rc = afx::check_device_memory(records_in, "records_in", who)) return rc;
  hipLaunchKernelGGL(k_pose_lm_step, dim3(pose_blocks(n_views)), dim3(POSE_BLOCK), 0, (hipStream_t)stream, state, n_views, sums, n_slices, phase,
                     dof_mask, lambda0, records_in, trial_records);
  return afx::launched(who);
}
