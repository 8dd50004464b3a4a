// afx_internal.h — shared between the C-ABI host code and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <cmath>
#include "../../include/afx.h"

namespace afx {

constexpr int TILE = 128;            // samples per workgroup tile (4 waves x 32 sample-columns)
constexpr int GROUP = 32;            // samples per wave column group; s_pad is a multiple of this

// Geometry of the bf16 chain kernels' weight ring, shared by the kernels and the host (LDS size, prepared layout).
// A step streams TPS consecutive 32-row output tiles of one layer into one LDS slot (at least 8 KiB: one LDS-DMA
// piece per wave of an 8-wave workgroup); a ring of RING slots is requested RING-1 steps ahead.  Forward-only
// kernels: 2 slots of 4 tiles.  Backward kernel: its ReLU masks fill half the LDS: 2 slots of 2 tiles (a 4-slot
// ring of one-tile steps, requested 3 steps ahead, measured 5 ms slower per 512^2x128 step: twice the barriers).
// tiles per step: 4 in the forward-only kernels and, at width 128 (a layer is 4 tiles, its slabs 32 KiB), also in the backward kernel -
// one barrier per layer; at width 256 the backward kernel's ReLU masks leave LDS room for 2-tile steps only
// PHASE 2 (the backward half of the split training step) at widths <= 128: TWO workgroups per CU.  At those widths
// a tile is 8 MFMAs against an epilogue of the same length as at width 256, so a lone workgroup - whose two waves per SIMD run in lockstep
// behind the step barrier - leaves the matrix pipe idle most of the time; a second, unsynchronised workgroup fills it.  That needs <= 128
// VGPRs per wave (the backward half fits: no forward activations, no in-kernel group sums) and <= 80 KB of LDS: two-tile steps.
constexpr bool chain_occ2(int nt, int phase) { return phase == 2 && nt <= 4; }
constexpr int chain_tps(int nt, bool bwd, bool x3, int phase = 0) {
  return chain_occ2(nt, phase) ? (nt >= 2 ? 2 : 1) : ((nt >= 4 && !x3 && (!bwd || nt == 4)) ? 4 : (nt >= 2 ? 2 : 1));
}
constexpr uint32_t chain_slab0_bytes(int nk0) { return ((uint32_t)nk0 * 2048u + 4095u) / 4096u * 4096u; }
constexpr uint32_t chain_slot_bytes(int nt, int nk0, bool bwd, bool x3, int phase = 0) {
  const uint32_t s0 = phase == 2 ? 0u : (uint32_t)chain_tps(nt, bwd, x3, phase) * chain_slab0_bytes(nk0);      // (the backward half streams no first-layer slab)
  const uint32_t sh = (uint32_t)chain_tps(nt, bwd, x3, phase) * (uint32_t)nt * 2048u * (x3 ? 2u : 1u);
  return s0 > sh ? s0 : sh;
}

// Arguments of the fused chain kernels (by value, < 512 B).
struct ChainArgs {
  // prepared weights
  const char* stream_fwd;   // slab0, then n_hidden*NT forward slabs (layer 1..N, tile 0..NT-1)
  const char* stream_bwd;   // n_hidden*NT transposed slabs (layer N..1, tile 0..NT-1); bf16: directly behind stream_fwd
  const char* stream_lo;    // split-bf16 only: the lo parts of the forward hidden slabs, same order as the hi parts
  const float* small;       // permuted biases, output weights, bout, encoding aux
  uint32_t small_floats;    // multiple of 4
  uint32_t small_bytes_pad; // LDS bytes reserved for `small` (multiple of 1024)
  uint32_t slab0_bytes, slabh_bytes, slot_bytes;   // multiples of 4096
  uint32_t slabh_stride, slabt_bytes;              // bf16: distance between forward slabs; transposed slab size
  int32_t n_hidden, k0, nq, enc, n_freq;
  // work range
  int32_t tile0, tile1;     // global tile ids [tile0, tile1), in units of the kernel's tile (128 or 256 samples)
  int64_t n_total;          // samples: n_rays * s_pad, or n_pts
  int32_t mode;             // 0 = points, 1 = rays
  // inputs
  const float* pts;
  const float* org;
  const float* dir;
  const double* poses;
  const int32_t* ray_ids;
  int64_t ray_id0;
  int32_t width, height;
  double focal;
  int32_t n_samples, s_pad, depth_mode;
  float t_near, t_step;
  float t_far;              // AFX_DEPTH_STRATIFIED
  uint64_t jitter_seed, jitter_stream;
  const float* z;
  // outputs
  float* out;               // points mode
  int32_t apply_sigmoid;
  float* od_part;           // [R, s_pad/32]
  float* sigma;             // optional [R,S]
  float* tau;               // optional [R,S]
  // backward only
  const float* dod;         // [R] dL/d(optical depth)
  float* stash_h;           // [(N+1), rows, F]   post-activation H_0..H_N
  float* stash_dz;          // [(N+1), rows, F]   dL/dZ_0..dZ_N
  float* stash_e;           // f32 kernels / raw-coordinate inputs: [rows, 2*nq] fp32 encoded inputs.  16-bit kernels WITH an encoding: 16-bit
                            // chunk-major stash [row>>5][8 chunks][row&31][8 values] of the 64 input columns, and behind it (stash_rows*128 B)
                            // the same layout of d(enc)/d(coef)/(2 pi) when coef_cols > 0
  float* graw;              // [rows]             dL/draw
  int64_t stash_rows;
  int32_t persistent;       // unused; kept for the layout
  int32_t fused;            // backward kernel computes pixel, MSE gradient and dL/draw itself (train step)
  const float* target;      // [R] (fused)
  float* pixel;             // [R] out (fused)
  float inv_n;              // 1 / global ray count (fused)
  int32_t debug;            // unused; kept for the layout
  // in-kernel small gradients (bf16 backward, rays mode, no encoding): per 32-sample group [SW[F] S0[F] S1[F] c[3] d[3] sum_g -]
  float* small_part;        // null: H_N, dZ_0, encoded inputs and dL/draw are stashed for k_small_grads_bf16 instead
  uint32_t* gmax;           // f16 mode: bit pattern of max |dL/draw| over the chunk (integer atomicMax; zeroed per chunk)
  int32_t stash8;           // f16 mode: 8-bit (bf8) stash of H_l and dZ'_l
  int32_t* gexp;            // 8-bit stash: power-of-two exponent of each 32-sample group's largest |dL/draw| [rows/32]
  uint32_t* hexp;           // 6-bit H stash: [N][rows/32] the E8M0 block scales of H_l, one byte per 64-feature tile pair
  int32_t coef_cols;        // 3*n_freq when the fourier coefficients train (the chain kernel then also stashes d(enc)/d(coef)/(2 pi)), else 0
  // hierarchical step with coarse re-use (afx_hier_train_step_mse): PHASE 1 runs before the samples' final step lengths are known (the fine depths
  // depend on this very pass): it stashes H_N as well (the output layer's gradient is contracted from the stash later) and forms no g' sums;
  // PHASE 2 then reads the finished dL/draw per sample from gpart (dod == null)
  int32_t defer_out;
  // packed, group-aligned samples (AFX_DEPTH_PACKED = 4: the occupancy-grid march's output): sample n of the padded list belongs to ray
  // group_ray[n >> 5]; its interval is [z[n], te[n]) (dead padding slots: te <= ts); optical-depth partials are indexed by group
  const float* te;
  const int32_t* group_ray;
  int32_t act;              // activation of the hidden layers: 0 ReLU (every kernel), 1 tanh, 2 sine (forward-only kernels)
  float act_w0;             // sine: the first layer's frequency factor w0 (model/CPPN.py:53-57)
  // split phases of the 8-bit-stash training kernel (rays that straddle workgroup tiles)
  char* masks;              // [tiles of the chunk][(N+1) x NT x 512 x u16]: the ReLU-mask LDS image of each tile (PHASE 1 writes, PHASE 2 reads)
  float* gpart;             // [rows] g' = dt sigma (1 - sigma) of each sample (PHASE 1 writes, PHASE 2 reads)
  // device-resident sample count (afx_march_train_step_mse_capturable): null = n_total / tile1 are the work range (every other caller).
  // Otherwise the launch is sized for the capacity n_total / tile1 and the kernel bounds its work by min(*n_dev, n_total) samples.
  const int64_t* n_dev;
  // single-evaluation grid step (afx_march_train_step_mse_single_eval): PHASE 1 also writes, per padded row n of a live sample, the output-layer
  // value before the sigmoid (row_raw[n]) and tau = sigma dt (row_tau[n]) - the inputs of the visibility / composite kernel.  Null: not written.
  float* row_raw;
  float* row_tau;
};

struct WgradArgs {
  const float* stash_h;
  const float* stash_dz;
  const float* stash_e;
  const float* graw;
  int64_t rows;             // rows to contract over (multiple of TILE)
  int64_t stride_rows;      // layer stride of the stash (rows of a full chunk)
  int32_t n_hidden, k0, k0pad;
  int32_t n_splits, rows_per_split;   // rows_per_split even
  float* partial;           // [(N+2), n_splits, F*F]: slot l = layer l; slot N+1 = the d(enc)/d(coef) contraction
  float* partial2;          // [(N+2), n_splits, F+4]
  int32_t debug;            // unused; kept for the layout
  float* partial_s;         // bf16 path: [n_small, F*k0pad + 2F + 4] first-layer / output-layer partials
  int32_t small_groups;     // 1: the chain kernel left per-group sums where H_N's stash would be (k_small_from_groups)
  const uint32_t* gmax;     // f16 mode: the chunk's max |dL/draw| (scale of the contraction, wgrad_scale_exp)
  int32_t stash_esz;        // bytes per stash element (4 f32, 2 bf16/f16, 1 bf8)
  const int32_t* gexp;      // 8-bit stash: group exponents (block scales of the MX contraction)
  int y0;                   // k_wgrad_s8: grid row of the launch's first block row (hidden layers 0..N-1, then the encoded first layer's rows)
  const uint32_t* hexp;     // 6-bit H stash: [N][stride_rows/32] E8M0 bytes of H_l's tile pairs (B operand's block scales)
  int32_t enc16;            // 16-bit kernels with an encoding: stash_e is the 16-bit chunk-major input stash; k_wgrad_bf16 contracts layer 0 on
                            // the matrix pipe (blockIdx.y = n_hidden) and, with coef_cols > 0, d(enc)/d(coef) as well (blockIdx.y = n_hidden + 1)
  int32_t coef_cols;        // 3*n_freq when the fourier coefficients train, else 0
  // split phases: the output-layer group sums were formed with g' (without the ray's dL/d(optical depth)); k_small_from_groups applies it
  const float* dod;         // [n_rays] or null (fused kernel: the sums already carry it)
  const int32_t* group_ray; // packed samples: ray of each group (then dod[group_ray[g]]), else null (dod[(group0 + g) / gpr])
  const float* records;     // the group records when they do not lie where H_N's stash would be (hierarchical step with coarse re-use), else null
  int32_t no_sw;            // hierarchical step with coarse re-use: the group records hold the first-layer sums only (output layer: k_wout_stash8)
  const float* gfull;       // ... and dL/draw per stash row for k_wout_stash8
  int32_t gpr;              // 32-sample groups per ray (s_pad / 32)
  int64_t group0;           // global index of the chunk's first group
  int64_t n_groups_valid;   // groups that belong to a ray (the chunk's last tile may be padded with dead groups beyond them)
  const int64_t* dsz;       // device-resident sizes (SZ_* slots; afx_march_train_step_mse_capturable) or null: rows / n_splits / rows_per_split /
                            // n_groups_valid above and the record count (gridDim.x) are the work range.  Otherwise the launch is sized for the capacity
                            // and the kernels take the sizes from dsz: workgroups beyond the device counts exit without writing
};

struct ReduceArgs {
  const float* partial;
  const float* partial2;
  int32_t n_hidden, k0, k0pad, n_splits;
  int32_t hidden_only;      // bf16 path: layer 0 and the output layer are reduced by k_reduce_small
  int32_t layer0_mfma;      // ... unless layer 0 came out of k_wgrad_bf16 (enc16): then k_reduce_w / k_reduce_b take it like a hidden layer
  int32_t n_small;
  const float* partial_s;
  float* grad;              // flat parameter gradient, accumulated into
  const uint32_t* gmax;     // f16 mode: hidden-layer partials carry the factor 2^-e (wgrad_scale_exp); null otherwise
  int32_t scale_shift;      // 8-bit stash: and the factor 2^scale_shift of the stashed J
  const float* w0;          // k_reduce_coef: the first layer's fp32 weights [F, k0]
  float* d_coef;            // k_reduce_coef: d loss / d fourier coefficients [coef_cols], accumulated into
  int32_t coef_cols;
  const int64_t* dsz;       // device-resident sizes (as WgradArgs::dsz) or null: n_splits / n_small above; dsz[SZ_ROWS] == 0: nothing to add
};

// Slots of the device-resident size block of afx_march_train_step_mse_capturable (k_grid_step_sizes writes them from the offsets kernels'
// totals with wgrad_split below, as the host does, so the capturable step sums in the same order as the one-call step)
enum { SZ_NTOTAL = 0, SZ_ROWS = 1, SZ_SPLITS = 2, SZ_RPS = 3, SZ_SMALL = 4, SZ_GROUPS = 5, SZ_COUNT = 8 };

// How the weight-gradient kernels share out `rows` stash rows: `splits` ranges of rows_per_split rows (whole 32-/64-sample stages) - splits0,
// the launch's base count, cut to one range per 256 rows and to 1..max_splits - and n_small group records (a block per ~4 groups, so that a
// sparse list does not write and sum max_small mostly-empty records).  The split and the record count fix the order of the fp32 sums: the
// host launches and the device size block (grid_step_sizes) both take them from here.
struct WgradSplit { int64_t splits, rows_per_split, n_small; };
__host__ __device__ __forceinline__ WgradSplit wgrad_split(int64_t rows, int splits0, int max_splits, int max_small) {
  int64_t splits = splits0;
  if (splits > rows / 256) splits = rows / 256;
  if (splits < 1) splits = 1;
  if (splits > max_splits) splits = max_splits;
  int64_t rps = (rows + splits - 1) / splits;
  rps = (rps + 63) / 64 * 64;
  int64_t n_small = (rows / GROUP + 3) / 4;
  if (n_small < 64) n_small = 64;
  if (n_small > max_small) n_small = max_small;
  return {splits, rps, n_small};
}

// Hands out the regions of a workspace in order, each rounded up to `align` bytes; `end` is how far the carve has got.  The base is an
// integer, so that the one function that describes a workspace both sizes it (base 0: nothing is dereferenced) and carves the caller's.
struct Carve {
  uintptr_t base = 0;
  size_t end = 0;
  template <class T = char>
  T* take(size_t bytes, size_t align = 256) {
    T* p = (T*)(base + end);
    end += (bytes + align - 1) / align * align;
    return p;
  }
};

// Sets afx_last_error()'s message to "<who>: <msg>" and returns `code` (defined in afx_api.hip, for the other translation units).
int set_error(int code, const char* who, const char* msg);

// The caller's workspace, checked on the host before check_device and before any launch: not null, at least `need` bytes, and its base
// a multiple of WORKSPACE_ALIGN bytes - each refused with `code` (the entry point's workspace error) and a message that says which.
// Why 16: every carved offset is a multiple of Carve's 256-byte granule, so the base decides the alignment of every region, and the widest
// access any kernel makes to carved memory is one 16-byte vector (the u32x4 / f32x4 casts of the stash, mask and group-record planes in
// afx_kernels_bf16.hip and afx_kernels_f32.hip; the wider vector types there are MFMA register operands, never a memory access).  The
// doubles and the 64-bit atomic targets carved by the analysis units need 8.
constexpr size_t WORKSPACE_ALIGN = 16;
inline int check_workspace(const void* ptr, size_t bytes, size_t need, const char* who, const char* query = nullptr, int code = AFX_E_WORKSPACE) {
  char msg[192];
  if (!ptr) return set_error(code, who, "workspace is null");
  if (bytes < need) {      // `query`: the size query to name in the message, when the entry point has one of its own
    snprintf(msg, sizeof msg, "workspace too small: %zu < %zu bytes%s%s%s", bytes, need, query ? " (" : "", query ? query : "", query ? ")" : "");
    return set_error(code, who, msg);
  }
  if ((uintptr_t)ptr % WORKSPACE_ALIGN) {
    snprintf(msg, sizeof msg, "workspace must be aligned to %zu bytes", WORKSPACE_ALIGN);
    return set_error(code, who, msg);
  }
  return AFX_OK;
}

// A voxel volume vol[nx][ny][nz] (fp32) on a regular grid: axis a has its first sample at a0 and spacing da.  vol_sample is scipy's
// RegularGridInterpolator(method='linear', bounds_error=False, fill_value=fill) at (px, py, pz) in fp64: the 8-voxel trilinear blend,
// `fill` outside the box (the box's faces belong to it).  k_project_volume (ground-truth projections) and k_volume_grid (the
// ground-truth density grid) share it; type_ct is the projector's only.
struct VolArgs {
  const float* vol;
  int32_t nx, ny, nz;
  double x0, y0, z0, dx, dy, dz;
  float fill;
  int32_t type_ct;
};

__device__ __forceinline__ bool vol_axis(double p, double a0, double da, int n, int& i, double& t) {
  const double a1 = a0 + da * (n - 1);
  if (!(p >= a0 && p <= a1)) return false;
  double u = (p - a0) / da;
  i = (int)u;
  if (i > n - 2) i = n - 2;
  if (i < 0) i = 0;
  t = u - i;
  return true;
}

__device__ __forceinline__ double vol_sample(const VolArgs& v, double px, double py, double pz) {
  const size_t sy = (size_t)v.nz, sx = (size_t)v.ny * v.nz;
  int ix, iy, iz;
  double tx, ty, tz;
  double mu = v.fill;
  if (vol_axis(px, v.x0, v.dx, v.nx, ix, tx) && vol_axis(py, v.y0, v.dy, v.ny, iy, ty) && vol_axis(pz, v.z0, v.dz, v.nz, iz, tz)) {
    const float* b = v.vol + ix * sx + iy * sy + iz;
    const double c00 = b[0] * (1 - tz) + b[1] * tz, c01 = b[sy] * (1 - tz) + b[sy + 1] * tz;
    const double c10 = b[sx] * (1 - tz) + b[sx + 1] * tz, c11 = b[sx + sy] * (1 - tz) + b[sx + sy + 1] * tz;
    mu = (c00 * (1 - ty) + c01 * ty) * (1 - tx) + (c10 * (1 - ty) + c11 * ty) * tx;
  }
  return mu;
}

// The C entry points of the image and metric units: `p` (named `what` in the message) is memory of the current device (launches go to a
// stream of the current device); and the launches just made were accepted.
inline int check_device(const void* p, const char* what, const char* who) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return set_error(AFX_E_HIP, who, "no HIP device");
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();                          // not HIP memory: leave no error behind for the next launch check
    char msg[96];
    snprintf(msg, sizeof msg, "%s is not memory of a HIP device", what);
    return set_error(AFX_E_INVALID, who, msg);
  }
  if (at.device != dev) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s lives on another device than the current one", what);
    return set_error(AFX_E_INVALID, who, msg);
  }
  return AFX_OK;
}

// check_device behind a refusal of plain host memory, which the runtime may know as an "unregistered" pointer and report with success
inline int check_device_memory(const void* p, const char* what, const char* who) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeUnregistered) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s is not memory of a HIP device", what);
    return set_error(AFX_E_INVALID, who, msg);
  }
  (void)hipGetLastError();                            // (a failed query is check_device's to report)
  return check_device(p, what, who);
}

// Host-side checks of the lattice entry points: the n doubles at p are all finite; and a flat index of an (n0, n1, n2) lattice fits an int32
// (the one message every such entry point gives); and every side of a volume lies in 1..AFX_EDT3D_MAX_SIDE (the callers word the refusal).
inline bool all_finite(const double* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

inline int check_lattice_size(int32_t n0, int32_t n1, int32_t n2, const char* who) {
  if ((int64_t)n0 * n1 >= (int64_t)1 << 31 || (int64_t)n0 * n1 * n2 >= (int64_t)1 << 31)
    return set_error(AFX_E_INVALID, who, "n0 n1 n2 must stay below 2^31");
  return AFX_OK;
}

inline bool volume_shape_ok(int32_t n0, int32_t n1, int32_t n2) {
  return n0 >= 1 && n1 >= 1 && n2 >= 1 && n0 <= AFX_EDT3D_MAX_SIDE && n1 <= AFX_EDT3D_MAX_SIDE && n2 <= AFX_EDT3D_MAX_SIDE;
}

inline int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? AFX_OK : set_error(AFX_E_HIP, who, hipGetErrorString(e));
}

}  // namespace afx
