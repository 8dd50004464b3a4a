// afx_kernels_ingrad.hip — gradients with respect to the model's INPUTS (sample points, ray origins and directions) for
// afx_mlp_backward_inputs / afx_render_backward_inputs.  Included by afx_api.hip after afx_kernels_f32.hip and afx_kernels_bf16.hip.
//
// The backward chain kernels leave dZ_0 = dL/d(first-layer pre-activation) per sample in the layer-0 plane of their dZ stash (the
// configuration without in-kernel group sums and without the 8-bit stash: fp32 in the exact kernel, bf16 / f16 in the 16-bit ones).
// k_input_grads contracts it with the first layer and the encoding's Jacobian, one sample per lane, in fp32:
//   u = W_0^T dZ_0 (k0 values),  dx_c = sum over encoded columns k of coordinate c of (d enc_k / d x_c) u_k
// and writes dx per point (points mode) or, per 32-sample group of one ray, (sum dx, sum t dx) (rays mode).  k_ray_input_grads sums a
// ray's groups in order and adds the step-length term of the dense conventions.  Fixed summation orders, no atomics: the results do not
// depend on the chunking of the call.

// Where k_input_grads finds dZ_0 and the first layer.
struct InGradArgs {
  const char* stash_dz;     // layer-0 plane of the chunk's dZ stash
  const float* graw;        // [rows] dL/draw (f16 stash: J_0 = dZ_0 / g)
  const char* slab0;        // first-layer slabs of the prepared buffer
  uint32_t slab0_bytes;     // bytes per slab (16-bit: one per 32-row tile)
  const float* aux;         // encoding constants in the prepared buffer: BARF [freq | weight], FOURIER [coef]
  int32_t k0, enc, n_freq, n_tiles;
  int64_t row0;             // global sample index of the chunk's first stash row (a multiple of 32)
  int64_t rows;             // stash rows of the chunk
  float* d_pts;             // points mode: [n_total, 3] out
  float* gpart;             // rays mode: [groups, 8] out: sum dx (3), sum t dx (3), 2 unused
};

// W_0[f][k] from the prepared first-layer slabs.  FMT 0 (exact fp32): [q][t][lane] = W0[32t + (lane&31)][2q + (lane>>5)].
// 16-bit: slab t, [((q*2 + part)*64 + lane)*8 + j] = W0[32t + (lane&31)][16q + 8(lane>>5) + j], split bf16 (hi + lo).
template <int FMT>
__device__ __forceinline__ float ingrad_w0(const InGradArgs& g, int f, int k) {
  const int t = f >> 5;
  if (FMT == 0) {
    const int lane = (f & 31) + 32 * (k & 1);
    return ((const float*)g.slab0)[((int64_t)(k >> 1) * g.n_tiles + t) * 64 + lane];
  }
  const int lane = (f & 31) + 32 * ((k >> 3) & 1);
  const unsigned short* s = (const unsigned short*)(g.slab0 + (size_t)t * g.slab0_bytes);
  const int base = ((k >> 4) * 2 * 64 + lane) * 8 + (k & 7);
  const float hi = __builtin_bit_cast(float, (unsigned)s[base] << 16);
  const float lo = __builtin_bit_cast(float, (unsigned)s[base + 64 * 8] << 16);
  return hi + lo;
}

// One lane per stash row.  KM: encoded columns held per lane (4: raw coordinates, 64: an encoding).  FMT: 0 fp32 [rows][F] stash,
// 1 bf16 dZ_0, 2 f16 J_0 = dZ_0 / g (chunk-major stash, stash_off / fperm of afx_kernels_bf16.hip).  LDS: W_0 as [F][KM] fp32.
template <int F, int KM, int FMT>
__global__ void __launch_bounds__(256) k_input_grads(const ChainArgs a, const InGradArgs g) {
  extern __shared__ __attribute__((aligned(16))) float w0s[];
  for (int i = threadIdx.x; i < F * KM; i += 256) {
    const int f = i / KM, k = i % KM;
    w0s[i] = k < g.k0 ? ingrad_w0<FMT>(g, f, k) : 0.f;
  }
  __syncthreads();
  const int nb = 3 * g.n_freq;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < g.rows; base += (int64_t)gridDim.x * 256) {
    const int64_t r = base + threadIdx.x;
    const int64_t n = g.row0 + r;
    const bool valid = r < g.rows;
    Sample sp = make_sample(a, valid ? n : a.n_total);
    float u[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) u[k] = 0.f;
    if (sp.live) {
      if (FMT == 0) {
        const float* z = (const float*)g.stash_dz + r * F;
        for (int f = 0; f < F; ++f) {
          const float d = z[f];
#pragma unroll
          for (int k = 0; k < KM; ++k) u[k] = fmaf(w0s[f * KM + k], d, u[k]);
        }
      } else {
        const float sc = FMT == 2 ? g.graw[r] : 1.f;
        for (int ch = 0; ch < F / 8; ++ch) {
          const u32x4 x = *(const u32x4*)(g.stash_dz + stash_off<F>((uint32_t)r, ch));
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const unsigned w = x[i >> 1];
            const float d = ((i & 1) ? hi_t<FMT == 2>(w) : lo_t<FMT == 2>(w)) * sc;
            const int f = fperm(ch * 8 + i);
#pragma unroll
            for (int k = 0; k < KM; ++k) u[k] = fmaf(w0s[f * KM + k], d, u[k]);
          }
        }
      }
    }
    // d enc_k / d x_c: encoded column k depends on coordinate k % 3 alone (3 raw columns, then sin and cos blocks of 3 n_freq)
    const float xs[3] = {sp.px, sp.py, sp.pz};
    float dx[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      if (k >= g.k0) break;
      float ck = 1.f;
      if (k >= 3) {
        int m = k - 3;
        const bool is_cos = m >= nb;
        if (is_cos) m -= nb;
        const float x = xs[k % 3];
        float v, fac;
        if (g.enc == AFX_ENC_BARF) {      // w sin|cos(freq x), w held constant
          v = __fmul_rn(g.aux[m], x);
          fac = g.aux[nb + m] * g.aux[m];
        } else {                          // sin|cos((2 pi x) coef)
          v = __fmul_rn(__fmul_rn(6.283185307179586f, x), g.aux[m]);
          fac = 6.283185307179586f * g.aux[m];
        }
        ck = is_cos ? -fac * enc_sincos(v, false) : fac * enc_sincos(v, true);
      }
      dx[k % 3] = fmaf(ck, u[k], dx[k % 3]);
    }
    if (a.mode == 0) {
      if (sp.live) {
        g.d_pts[3 * n + 0] = dx[0];
        g.d_pts[3 * n + 1] = dx[1];
        g.d_pts[3 * n + 2] = dx[2];
      }
      continue;
    }
    // rays mode: p = o + t d, so dL/do = sum dx and dL/dd = sum t dx (+ the step-length term, k_ray_input_grads); a 32-sample group
    // belongs to one ray (s_pad is a multiple of 32) and is summed over its lanes in a fixed butterfly
    float t = 0.f;
    if (sp.live) {
      float ddx, ddy, ddz;
      ray_param(a, sp, t, ddx, ddy, ddz);
    }
    float v[6] = {dx[0], dx[1], dx[2], t * dx[0], t * dx[1], t * dx[2]};
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      if (!sp.live) v[j] = 0.f;
#pragma unroll
      for (int sh = 16; sh >= 1; sh >>= 1) v[j] += __shfl_xor(v[j], sh);
    }
    if (valid && n < a.n_total && (threadIdx.x & 31) == 0) {      // (a last tile's padding rows lie beyond the rays' groups)
      float* o = g.gpart + (n >> 5) * 8;
#pragma unroll
      for (int j = 0; j < 6; ++j) o[j] = v[j];
    }
  }
}

// Per ray: d_org = sum of the groups' sum dx, d_dir = sum of their sum t dx, in group order.  Dense conventions (od_part != null): the step
// lengths dt_s = dist_s ||d|| also depend on d: tau_s = sigma_s dist_s ||d||, d tau_s / d d = tau_s d / ||d||^2, and dL/dtau_s = dod for every
// sample (pixel = exp(-sum tau)), so the term is dod * OD * d / ||d||^2 with OD = the ray's optical depth (the forward pass's group partials).
__global__ void k_ray_input_grads(const float* gpart, const float* od_part, const float* dod, const float* dirs, int64_t n_rays, int gpr,
                                  float* d_org, float* d_dir) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < gpr; ++q) {
    const float* p = gpart + ((size_t)r * gpr + q) * 8;
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] += p[j];
  }
  if (od_part) {
    float od = 0.f;
    for (int q = 0; q < gpr; ++q) od += od_part[(size_t)r * gpr + q];
    const float dx = dirs[3 * r + 0], dy = dirs[3 * r + 1], dz = dirs[3 * r + 2];
    const float n2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    const float f = n2 > 0.f ? dod[r] * od / n2 : 0.f;
    s[3] = fmaf(f, dx, s[3]);
    s[4] = fmaf(f, dy, s[4]);
    s[5] = fmaf(f, dz, s[5]);
  }
  if (d_org) { d_org[3 * r + 0] = s[0]; d_org[3 * r + 1] = s[1]; d_org[3 * r + 2] = s[2]; }
  if (d_dir) { d_dir[3 * r + 0] = s[3]; d_dir[3 * r + 1] = s[4]; d_dir[3 * r + 2] = s[5]; }
}
