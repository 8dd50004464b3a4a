/* afx.h — C-ABI of the MI355X-native angiography-NeRF hot path ("afx").
 *
 * The upstream reference (kirstenmaas/nerf-for-angiography) has no FFI/plugin
 * boundary: its hot path is Python calling torch.  The boundary this library
 * replaces is therefore the set of Python functions cited on each entry point
 * below (file:line in the upstream tree).  Everything here is plain C: raw
 * device pointers, sizes and a hipStream_t passed as void*.  No torch types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative afx_status otherwise;
 *     afx_last_error() gives a thread-local message.  Nothing throws or exits.
 *   - the CALLER owns every buffer (parameters, gradients, outputs, prepared
 *     weights, workspace).  The library allocates nothing on the device and
 *     holds only immutable descriptors => calls are hipGraph-capturable, with
 *     three exceptions: afx_march_train_step_mse reads two sizes back (it polls),
 *     afx_march_render reads one, and afx_profile_read synchronises.  The grid iteration's capturable form
 *     is afx_march_train_step_mse_capturable (or afx_march_train_step_mse_single_eval).
 *   - all other calls are asynchronous on the stream passed in.
 *   - results are deterministic: no floating-point atomics anywhere.
 *   - workspaces (every `void* workspace, size_t workspace_bytes` pair, as a parameter or in an args struct; the sizes come from the
 *     *_workspace_bytes functions and the AFX_Q_*_WORKSPACE queries): device memory whose BASE IS A MULTIPLE OF 16 BYTES (hipMalloc and the
 *     PyTorch allocator give 256 and more).  A null base, fewer bytes than the call needs, or a misaligned base is refused on the host with
 *     the entry point's workspace error (AFX_E_WORKSPACE unless its comment says otherwise), before anything is launched or written.  The
 *     library lays its regions out at multiples of 256 bytes from the base and reads or writes them with accesses of up to 16 bytes.
 *     Nothing is assumed about the contents: every byte a kernel reads was written by the same call, so the buffer may hold whatever an
 *     earlier call - of this or another entry point, on a larger problem - left in it.  Nothing beyond workspace_bytes is touched.
 *     afx_tv_denoise_3d keeps its own rule (8 bytes, AFX_E_INVALID).
 */
#ifndef AFX_H
#define AFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct afx_ctx afx_ctx;

enum afx_status {
  AFX_OK = 0,
  AFX_E_INVALID = -1,      /* bad argument / unsupported configuration */
  AFX_E_WORKSPACE = -2,    /* workspace or prepared-weights buffer too small */
  AFX_E_HIP = -3           /* a HIP runtime call failed (message has the code) */
};

/* Positional encodings of CPPN.pos_enc (model/CPPN.py:207-234). */
enum { AFX_ENC_NONE = 0, AFX_ENC_BARF = 1, AFX_ENC_FOURIER = 2 };

/* Arithmetic of the MLP contractions.
 *   F32    : v_mfma_f32_32x32x2_f32, exact fp32 (strict parity mode)
 *   BF16X3 : split-bf16 (hi+lo) operands, 3 bf16 MFMAs per product, fp32
 *            accumulate: fp32-grade accuracy at 1/3 of the bf16 rate
 *   BF16   : bf16 operands, fp32 accumulate (first layer always split)
 *   F16    : f16 operands in the hidden layers (v_mfma_f32_32x32x16_f16: 11
 *            significant bits at the bf16 rate), fp32 accumulate, first layer
 *            split bf16.  Rendered pixels within ~1e-5 relative L2 of fp32.
 *            Backward: the input-gradient chain runs normalised by dL/draw
 *            (no loss scaling needed), the weight-gradient contraction carries
 *            a power-of-two scale taken from the batch's largest |dL/draw|.
 *            RANGE: f16 holds |x| <= 65504 - a hidden activation beyond that becomes inf and the pixel NaN (the
 *            conversion is v_cvt_pk_f16_f32, round-to-nearest, no saturation: a clamp would cost two VALU
 *            instructions per packed pair in the hottest epilogue).  With nn.Linear-initialised weights and world
 *            coordinates of +-100 the activations of an 8x256 model stay below ~1e2; a model that can exceed the
 *            range belongs on BF16 / BF16X3 (fp32 exponent range).  The training driver stops on a non-finite loss.
 *   F16S8  : F16 arithmetic; the backward pass keeps its per-sample stash
 *            (H_l, and the normalised chain J_l) as bf8 (e5m2) instead of f16:
 *            half the HBM round trip that bounds a training step.  Forward
 *            results are identical to F16; weight gradients carry the extra
 *            bf8 rounding of the two contraction operands (H to nearest, dZ'
 *            stochastically: its errors are systematic otherwise), averaged over
 *            the samples: 2e-3 relative L2 of the whole gradient (F16: 5e-4).  Rays mode (with an input encoding
 *            the encoded inputs are stashed as bf8 as well); points mode
 *            (afx_mlp_backward) runs exactly as F16.
 *            RANGE: the stashed chain is J_l = d raw / d z_l (a product of the weights alone; 1e-4 ... 1 for nn.Linear-initialised
 *            models) times 2^10 and the sample's normalised dL/draw (<= 1), converted through f16: a |J_l| of 64 or more - an
 *            output layer with such a weight, say - can become inf, and that neuron's row of the weight gradient NaN.  Such
 *            a model belongs on F16 or BF16.                                                                                */
enum { AFX_PREC_F32 = 0, AFX_PREC_BF16X3 = 1, AFX_PREC_BF16 = 2, AFX_PREC_F16 = 3, AFX_PREC_F16S8 = 4 };

/* CPPN(model_definition) — model/CPPN.py:10-139.  The configuration
 * nerf/run_nerf_acc.py:168-183 builds is accelerated end to end (ReLU, no skip block,
 * no view-direction head, one output channel); tanh / sine variants of it in the forward direction at every precision and in the
 * backward direction at AFX_PREC_F32. */
/* act_func of the hidden layers (model/CPPN.py:53-60).  ReLU is what nerf/run_nerf_acc.py trains and what every kernel takes.
 * tanh and sine (Sine(w0) on the first layer, Sine() behind it, CPPN.py:278-300) are evaluated by the FORWARD entry points
 * (afx_mlp_infer, afx_render_forward: inference, evaluation renders, density grids; without an input encoding) at every precision.  The
 * backward entry points (afx_mlp_backward, afx_render_backward) take them at AFX_PREC_F32 - the exact-fp32 chain kernel keeps d act / dz per
 * element in the slot of the dZ_l stash (ReLU: one mask bit in LDS) - and return AFX_E_INVALID for them at the 16-bit precisions. */
enum { AFX_ACT_RELU = 0, AFX_ACT_TANH = 1, AFX_ACT_SINE = 2 };

typedef struct afx_model_desc {
  int32_t n_in;        /* num_input_channels (3)                              */
  int32_t enc;         /* AFX_ENC_*                                           */
  int32_t n_freq;      /* pos_enc_basis L (ignored for AFX_ENC_NONE).  With an encoding afx_create admits 1 <= L <= 10, i.e. K0 = 3 + 6 L =
                        * 9 ... 63 first-layer columns, and asks that K0 rounded up to an even count (K0 + 1) fits the layer: 4 + 6 L <= width
                        * (width 64 takes every admitted L; L = 10 fills it exactly).  At AFX_PREC_F32 the LDS a launch needs grows with L:
                        * the backward entry points refuse an 8-hidden-layer width-256 model at L = 9 and L = 10 with AFX_E_INVALID
                        * ("needs ... B of LDS"; its forward runs, L <= 8 trains); the 16-bit precisions' LDS does not depend on L. */
  int32_t width;       /* num_filters: 64, 128 or 256                         */
  int32_t n_hidden;    /* num_early_layers N  (Linear count = N + 2)          */
  int32_t act;         /* AFX_ACT_*                                           */
  float act_w0;        /* AFX_ACT_SINE: sine_weights (first-layer frequency factor); ignored otherwise */
} afx_model_desc;

/* Flat fp32 parameter buffer layout (same order as the state-dict of the
 * reference): W0[width,K0] b0[width] W1[width,width] b1 ... WN bN
 * Wout[1,width] bout[1], K0 = n_in (+ 2*n_in*n_freq when encoded).           */

int  afx_create(const afx_model_desc* desc, afx_ctx** out);
void afx_destroy(afx_ctx* ctx);
const char* afx_last_error(void);

enum afx_query_what {
  AFX_Q_PARAM_COUNT = 0,       /* floats in the flat parameter buffer               */
  AFX_Q_K0 = 1,                /* encoded input width                               */
  AFX_Q_PREPARED_BYTES = 2,    /* bytes of the prepared-weights buffer (arg = prec) */
  AFX_Q_FWD_WORKSPACE = 3,     /* bytes needed by afx_render_forward  (arg0 = n_rays, arg1 = n_samples) */
  AFX_Q_BWD_WORKSPACE_MIN = 4, /* smallest sensible backward workspace (arg0 = n_rays, 0 for afx_mlp_backward; arg1 = n_samples when the split training step is meant) */
  AFX_Q_BWD_WORKSPACE_FULL = 5, /* workspace that lets backward run in one chunk (arg0 = n_rays, arg1 = n_samples; afx_mlp_backward: arg0 = 0, arg1 = n_pts) */
  AFX_Q_BWD_INPUTS_WORKSPACE_MIN = 6,  /* smallest workspace afx_mlp_backward_inputs / afx_render_backward_inputs take (arg0 = n_rays, 0 for points;
                                          arg1 = n_samples, or n_pts; arg2 = prec) */
  AFX_Q_BWD_INPUTS_WORKSPACE_FULL = 7  /* the same, letting the call run in one chunk */
};
int64_t afx_query(const afx_ctx* ctx, int what, int64_t arg0, int64_t arg1, int64_t arg2);

/* Offset (in floats) and shape of linear layer `layer` (0 .. n_hidden+1) inside
 * the flat parameter buffer. */
int afx_param_layout(const afx_ctx* ctx, int layer, int64_t* w_off, int64_t* b_off,
                     int32_t* rows, int32_t* cols);

/* Re-tile the flat fp32 parameters into the MFMA operand order the kernels
 * stream through LDS (forward slabs, transposed slabs for the input-gradient
 * chain, permuted biases).  Must be re-run after every optimizer step.
 * enc_aux: BARF: 2*n_in*n_freq floats = [freq | weight] (CPPN.barf_freq,
 * CPPN.barf_weights, model/CPPN.py:84-85,244-259); FOURIER: n_in*n_freq
 * coefficients (CPPN.py:73-75); may be NULL for AFX_ENC_NONE. */
int afx_prepare_weights(afx_ctx* ctx, int prec, const float* params, const float* enc_aux,
                        void* prepared, size_t prepared_bytes, void* stream);

/* get_predictions(model, flattened_query_points, chunksize) — nerf/nerf_helpers.py:31-45
 * and get_predictions_vis — visualization/helpers.py:21-45 (density grid).
 * pts[P,3] fp32 -> out[P] = raw, or sigmoid(raw) when apply_sigmoid != 0.
 * The chunk loop of the reference is unnecessary (nothing is materialised). */
int afx_mlp_infer(afx_ctx* ctx, int prec, const void* prepared, const float* pts, int64_t n_pts,
                  float* out, int apply_sigmoid, void* stream);

/* Backward of afx_mlp_infer (apply_sigmoid = 0): grad_flat += d(sum_p d_out[p]*raw[p])/d(params).
 * This is what loss.backward() does through get_predictions (nerf/run_nerf_acc.py:294,306)
 * when compositing is done outside the fused kernel. */
int afx_mlp_backward(afx_ctx* ctx, int prec, const void* prepared, const float* pts, int64_t n_pts,
                     const float* d_out, float* grad_flat, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Backward of afx_mlp_infer with respect to the POINTS as well: d_pts[p] = d(sum_q d_out[q]*raw[q])/d(pts[p]) (written, [n_pts,3]),
 * and, when grad_flat is not NULL, grad_flat += the parameter gradient exactly as afx_mlp_backward adds it (same kernels, same order:
 * bit-identical when both run in one chunk).  grad_flat == NULL: the weight-gradient kernels are not launched (a frozen model).
 * This is what autograd returns for x through CPPN.forward (model/CPPN.py:166-205) when x requires grad.  Input encodings: the BARF
 * weights are constants (as upstream), the fourier coefficients too (their own gradient: afx_set_encoding_grad).
 * How: the chain kernel runs in the configuration that stashes dZ_0 = dL/d(first-layer pre-activation) per sample (fp32 in the exact
 * kernel; bf16, or f16 normalised by dL/draw, in the 16-bit ones - never the 8-bit stash: AFX_PREC_F16S8 runs as AFX_PREC_F16 here) and a
 * second kernel contracts it per sample in fp32: dx = J_enc(x)^T W_0^T dZ_0.  Deterministic (no atomics, results
 * independent of the chunking); nothing allocated, no synchronisation: graph-capturable.  The workspace must hold at least
 * afx_query(AFX_Q_BWD_INPUTS_WORKSPACE_MIN, 0, n_pts, prec) bytes, else AFX_E_WORKSPACE (AFX_Q_BWD_INPUTS_WORKSPACE_FULL: one chunk). */
int afx_mlp_backward_inputs(afx_ctx* ctx, int prec, const void* prepared, const float* pts, int64_t n_pts, const float* d_out,
                            float* grad_flat /* nullable */, float* d_pts, void* workspace, size_t workspace_bytes, void* stream);

/* Where rays come from. */
enum { AFX_RAYS_ARRAYS = 0,   /* origins[R,3], dirs[R,3] fp32 (sample_pixel_rays output, nerf_helpers.py:137-150) */
       AFX_RAYS_POSE = 1 };   /* generated in-kernel: get_ray_values, phantomdata/helpers.py:156-175 */
/* Where depths along a ray come from, and which compositing convention. */
enum { AFX_DEPTH_UNIFORM_MID = 0, /* t_s = near+i*step, t_e = t_s+step, evaluate at (t_s+t_e)/2, dt = t_e-t_s:
                                     acc_ray_marching w/o grid + acc_render_volume_density, nerf_helpers_acc.py:10-63 */
       AFX_DEPTH_SHARED_Z = 1,    /* z[S] shared by all rays; render_volume_density, nerf_helpers.py:59-123:
                                     dt_i = (z[i+1]-z[i])*||d||, last dt = 1e10*||d||                                   */
       AFX_DEPTH_PER_RAY_Z = 2,   /* z[R,S] (hierarchical sampling, nerf_helpers.py:178-195); same convention   */
       AFX_DEPTH_STRATIFIED = 3 };/* randomize_depth (nerf_helpers.py:13-22) of z = linspace(t_near, t_far, S) IN the kernel:
                                     one jitter vector per call from Philox stream (jitter_seed, jitter_stream);
                                     render_volume_density convention.  Perf mode: parity mode passes the host's z (SHARED_Z) */

typedef struct afx_render_args {
  int64_t n_rays;
  int32_t n_samples;           /* S, samples per ray                                     */
  int32_t ray_mode;            /* AFX_RAYS_*                                             */
  const float* origins;        /* [R,3]  (AFX_RAYS_ARRAYS)                               */
  const float* dirs;           /* [R,3]                                                  */
  const double* poses;         /* [n_proj,3,4] row-major cam->world (AFX_RAYS_POSE), device */
  const int32_t* ray_ids;      /* [R] index into [n_proj,H,W]; NULL => ray r is index ray_id0 + r */
  int64_t ray_id0;
  int32_t width, height;
  double focal;
  int32_t depth_mode;          /* AFX_DEPTH_*                                            */
  float t_near, t_far;         /* AFX_DEPTH_UNIFORM_MID                                  */
  const float* z;              /* [S] or [R,S]                                           */
  float* pixel;                /* out [R]: rgb_map (transmittance)                       */
  float* sigma;                /* optional out [R,S]: sigmoid(raw)                       */
  float* tau;                  /* optional out [R,S]: sigma*dt (optical depth per sample) */
  void* workspace;
  size_t workspace_bytes;
  uint64_t jitter_seed, jitter_stream;   /* AFX_DEPTH_STRATIFIED */
} afx_render_args;

/* Fused ray generation -> sampling -> encoding -> MLP -> Beer-Lambert product.
 * Replaces the body of nerf/run_nerf_acc.py:287-296 (and :340-349 for eval). */
int afx_render_forward(afx_ctx* ctx, int prec, const void* prepared, const afx_render_args* args,
                       void* stream);

/* Backward of afx_render_forward w.r.t. the flat parameters:
 * grad_flat[param_count] += d(sum_r dL_dpixel[r] * pixel[r]) / d(params).
 * `pixel` in args must hold the forward result.  Replaces loss.backward()
 * through nerf/run_nerf_acc.py:289-296.  The workspace bounds the ray chunk
 * processed per pass (activations are recomputed, then stashed per chunk for
 * the weight-gradient contraction over samples). */
int afx_render_backward(afx_ctx* ctx, int prec, const void* prepared, const afx_render_args* args,
                        const float* dL_dpixel, float* grad_flat, void* stream);

/* Backward of afx_render_forward with respect to the RAYS as well (AFX_RAYS_ARRAYS): with p_s = o + t_s d the sample points,
 *   d_origins[r] = sum_s dL/dp_s,   d_dirs[r] = sum_s t_s dL/dp_s  (+ for the render_volume_density conventions - AFX_DEPTH_SHARED_Z,
 *   PER_RAY_Z, STRATIFIED - the step lengths dt_s = dist_s ||d||: + dL/dOD * OD * d / ||d||^2, OD = the ray's optical depth, the 1e10 tail
 *   included; AFX_DEPTH_UNIFORM_MID has dt = t_e - t_s and no such term).
 * Both are written ([R,3]); either may be NULL.  grad_flat (nullable) += the parameter gradient as afx_render_backward adds it (same
 * kernels and order: bit-identical when the call runs in one chunk); grad_flat == NULL skips the weight-gradient kernels.  Where
 * afx_render_backward keeps no dZ_0 stash (16-bit rays without an encoding, the 8-bit-stash precision) the input gradients take a chain pass
 * of their own (AFX_PREC_F16S8 runs it as AFX_PREC_F16); the dense conventions add one forward pass (the optical depths) when d_dirs is set.
 * The per-sample gradients are summed per 32-sample group, then per ray in group order: deterministic whatever the chunking, no atomics,
 * nothing allocated, graph-capturable.  AFX_E_INVALID: AFX_RAYS_POSE with d_origins or d_dirs (rays made in the kernel have no input to
 * differentiate), nothing requested, or what afx_render_backward refuses.  args->workspace: at least afx_query(AFX_Q_BWD_INPUTS_WORKSPACE_MIN,
 * n_rays, n_samples, prec) bytes, else AFX_E_WORKSPACE. */
int afx_render_backward_inputs(afx_ctx* ctx, int prec, const void* prepared, const afx_render_args* args, const float* dL_dpixel,
                               float* grad_flat /* nullable */, float* d_origins, float* d_dirs, void* stream);

/* ---- The reference's own iteration body on packed samples (nerf/run_nerf_acc.py:287-306): after the occupancy-grid march
 * (afx_march_* -> packed, ray-sorted t_starts / t_ends, offsets[R+1]) the reference gathers positions, evaluates the MLP (get_predictions),
 * multiplies the per-ray transmittances (acc_render_volume_density), takes the MSE and backpropagates.  afx_train_step_packed_mse does
 * all of that as the split-phase training step (forward half / per-ray reduction / backward half, see afx_train_step_mse) on a
 * GROUP-ALIGNED copy of the list: ray r's samples start at padded index 32 * group_offsets[r] (group_offsets = exclusive scan of
 * ceil(count_r / 32), int64 [R+1], the caller's cumsum), the tail of its last 32-sample group is dead padding (t_end <= t_start),
 * group_ray[g] = r - so a wavefront's 32 samples always belong to one ray.  afx_pack_groups builds ts_pad / te_pad / group_ray.
 * pixel[r] = prod exp(-sigmoid(raw) (t_e - t_s)) (1 for a ray without samples), L = inv_n sum_r (pixel_r - target_r)^2, grad_flat += dL/dparams.
 * AFX_PREC_F16S8; the workspace (AFX_Q_BWD_WORKSPACE_FULL with arg0 = n_rays, arg1 = 32 * n_groups / n_rays rounded up,
 * or simply arg0 = 0, arg1 = 32 * n_groups plus n_rays + n_groups floats) must hold the whole list in one chunk. */
int afx_pack_groups(const int64_t* offsets, const int64_t* group_offsets, int64_t n_rays, const float* t_starts, const float* t_ends,
                    float* ts_pad, float* te_pad, int32_t* group_ray, void* stream);
int afx_train_step_packed_mse(afx_ctx* ctx, int prec, const void* prepared, const float* origins, const float* dirs, int64_t n_rays,
                              const int64_t* group_offsets, const int32_t* group_ray, int64_t n_groups, const float* ts_pad,
                              const float* te_pad, const float* target, float inv_n, float* pixel, float* grad_flat,
                              void* workspace, size_t workspace_bytes, void* stream);

/* One fused training pass over a ray batch — the body of nerf/run_nerf_acc.py:287-306 (render, mse_loss,
 * backward) without materialising anything between the steps: the backward kernel's forward recompute IS the
 * forward pass; it composites each ray in-kernel, forms dL/dpixel = 2 (pixel - target) * inv_n
 * (L = inv_n * sum_r (pixel_r - target_r)^2, inv_n = 1 / global ray count) and runs the gradient chain.
 * grad_flat += dL/dparams; args->pixel receives the rendered pixels.  16-bit precisions only.
 * Rays whose padded sample count divides 256 lie inside one workgroup tile: ONE kernel per ray chunk.  Any other count (the
 * reference's own 300 samples per ray, nerf/run_nerf_acc.py:129; the 128 + 64 of the hierarchical pass) is taken by
 * AFX_PREC_F16S8 (with or without an input encoding) as the SAME work in two kernels per chunk - the forward half stashes H_l, the ReLU
 * masks and g' = dt sigma (1 - sigma) per sample, a per-ray reduction forms pixel and dL/d(optical depth), the backward half
 * runs the input-gradient chain from the masks - so nothing is computed twice; the workspace must then also hold
 * n_rays * (1 + padded samples / 32) floats (AFX_Q_BWD_WORKSPACE_FULL with arg0 = n_rays, arg1 = n_samples includes them).
 * Other precisions return AFX_E_INVALID for such counts (render, then afx_render_backward). */
int afx_train_step_mse(afx_ctx* ctx, int prec, const void* prepared, const afx_render_args* args,
                       const float* target, float inv_n, float* grad_flat, void* stream);

/* render_volume_density(radiance_field, ray_directions, depth_values) for one output channel —
 * nerf/nerf_helpers.py:59-123 (C == 1 branch), from a raw tensor already in memory.
 * raw[R,S], dirs[R,3], z[S] (z_per_ray=0) or [R,S]; all outputs optional except rgb_map.
 * weights = (1-alpha+1e-10)*cumprod_exclusive(alpha); depth_map = sum(alpha*z) (sic);
 * entropy per nerf_helpers.py:125-135. */
int afx_composite_dense(const float* raw, const float* dirs, const float* z, int z_per_ray,
                        int64_t n_rays, int32_t n_samples, float* rgb_map, float* depth_map,
                        float* weights, float* entropy, float* sigma, void* stream);
/* d raw = backward of rgb_map only (the quantity the loss uses). */
int afx_composite_dense_backward(const float* raw, const float* dirs, const float* z, int z_per_ray,
                                 int64_t n_rays, int32_t n_samples, const float* rgb_map,
                                 const float* d_rgb_map, float* d_raw, void* stream);

/* acc_render_volume_density(predictions, ray_indices, t_starts, t_ends, n_rays, ...) —
 * nerf/nerf_helpers_acc.py:45-63.  ray_indices must be sorted ascending (packed samples,
 * as nerfacc.ray_marching returns them).  rgb_map[r] = prod_{i in ray r} exp(-sigmoid(pred_i)*(te_i-ts_i)). */
int afx_composite_packed(const float* pred, const int32_t* ray_indices, const float* t_starts,
                         const float* t_ends, int64_t n, int64_t n_rays, float* rgb_map, void* stream);
int afx_composite_packed_backward(const float* pred, const int32_t* ray_indices, const float* t_starts,
                                  const float* t_ends, int64_t n, int64_t n_rays, const float* rgb_map,
                                  const float* d_rgb_map, float* d_pred, void* stream);

/* get_ray_entropy(sigmas, rgb_map, threshold) with its gradient — nerf/nerf_helpers.py:125-135 and nerf/nerf_helpers_acc.py:33-43, for packed,
 * ray-sorted samples (ray_indices ascending, every value in [0, n_rays)).  sigma_i = sigmoid(pred_i), eps = 1e-10, per ray:
 *   D = sum sigma_i + eps, p_i = sigma_i / D, entropy[r] = -sum p_i log(p_i + eps) * [(1 - rgb_map[r]) > threshold]
 * (the mask carries no gradient; rgb_map is an input, what afx_composite_packed wrote).  A ray without samples has entropy 0.
 * ray_sums [n_rays,2] receives {D, sum_j p_j u_j}, u_i = log(p_i + eps) + p_i / (p_i + eps): what the backward needs per ray.
 * One wavefront per ray, sums in a fixed order, no atomics: bit-reproducible. */
int afx_ray_entropy_packed(const float* pred, const int32_t* ray_indices, int64_t n, const float* rgb_map, int64_t n_rays,
                           float threshold, float* entropy, float* ray_sums /* [n_rays,2] */, void* stream);
/* d_pred[i] (+)= d_entropy[r] * mask_r * (-(u_i - ray_sums[r][1]) / ray_sums[r][0]) * sigma_i (1 - sigma_i), r = ray_indices[i];
 * accumulate != 0 adds to d_pred (e.g. onto afx_composite_packed_backward's output), 0 overwrites it. */
int afx_ray_entropy_packed_backward(const float* pred, const int32_t* ray_indices, int64_t n, const float* rgb_map, float threshold,
                                    const float* ray_sums, const float* d_entropy, int accumulate, float* d_pred, void* stream);
/* The same for the dense layout raw[n_rays, n_samples] (nerf/nerf_helpers.py:119,125-135): the value afx_composite_dense writes to `entropy`,
 * summed in another order, and its gradient d_raw[n_rays, n_samples]. */
int afx_ray_entropy_dense(const float* raw, int64_t n_rays, int32_t n_samples, const float* rgb_map, float threshold,
                          float* entropy, float* ray_sums /* [n_rays,2] */, void* stream);
int afx_ray_entropy_dense_backward(const float* raw, int64_t n_rays, int32_t n_samples, const float* rgb_map, float threshold,
                                   const float* ray_sums, const float* d_entropy, int accumulate, float* d_raw, void* stream);

/* sample_pdf(bins, weights, N_samples) — nerf/nerf_helpers.py:197-222, with the uniform
 * draw u[R,n_fine] supplied by the caller; and the depth part of fine_sampling (:179-186):
 * bins = mid-points of z_coarse, weights = w_coarse[:,1:-1], output = sort(cat(z_coarse, samples)).
 * z_coarse [S] (z_per_ray=0) or [R,S]; w_coarse[R,S]; z_out[R,S+n_fine]. */
int afx_fine_depths(const float* z_coarse, int z_per_ray, const float* w_coarse, const float* u,
                    int64_t n_rays, int32_t n_coarse, int32_t n_fine, float* z_out, void* stream);

/* The same from the coarse pass's per-sample optical depths tau[R,S] (afx_render_forward's `tau` output) instead of its weights:
 * weights = (1 - alpha + 1e-10) * cumprod_exclusive(alpha), alpha = exp(-tau) (nerf/nerf_helpers.py:107-108) are formed per ray inside
 * the kernel, so the coarse -> fine hand-over of the hierarchical step needs no [R,S] passes in between. */
int afx_fine_depths_from_tau(const float* z_coarse, int z_per_ray, const float* tau_coarse, const float* u, int64_t n_rays,
                             int32_t n_coarse, int32_t n_fine, float* z_out, void* stream);

/* The hierarchical training step `fine_sampling` belongs to (nerf/nerf_helpers.py:178-195: coarse pass, sample_pdf on its weights, re-evaluation
 * of all S + N_f depths, compositing, MSE, backward through the fine pass), WITHOUT evaluating the coarse depths twice: coarse and fine network
 * are the same model here (fine_model = None, `:190`), and the coarse depths are a subset of the merged ones, so the coarse pass runs as the
 * forward HALF of the training kernel over the S coarse depths (stash, masks, sigma, tau), sample_pdf draws the N_f new depths from its weights, a
 * second forward half evaluates ONLY those, a per-ray kernel composites the merged list (step lengths of the merged order, last 1e10, x ||d||),
 * forms pixel, the MSE gradient and every sample's finished dL/draw, and the two backward halves + weight gradients follow.  The samples are
 * detached as upstream (`:186`).  args: rays (either ray mode), depth_mode AFX_DEPTH_SHARED_Z / PER_RAY_Z with the COARSE depths z, n_samples = S,
 * pixel out [R], workspace of afx_hier_workspace_bytes (fewer bytes: more ray chunks).  u[R, n_fine]: the uniform draws of sample_pdf.
 * z_all: optional out [R, S + n_fine], the merged depths.  AFX_PREC_F16S8, ReLU, no input encoding. */
int64_t afx_hier_workspace_bytes(const afx_ctx* ctx, int64_t n_rays, int32_t n_coarse, int32_t n_fine);
int afx_hier_train_step_mse(afx_ctx* ctx, int prec, const void* prepared, const afx_render_args* args, int32_t n_fine, const float* u,
                            const float* target, float inv_n, float* z_all, float* grad_flat, void* stream);

/* Ground-truth projector ray_tracing(interpolator, ...) — phantomdata/helpers.py:192-224 — for a voxel volume
 * vol[nx,ny,nz] (C order) on the regular grid axis_k = origin_k + i*spacing_k, trilinear interpolation with
 * `fill_value` outside (scipy RegularGridInterpolator(method='linear', bounds_error=False, fill_value) as built by
 * get_interpolator_from_* :72-154).  Rays and depths come from `args` (ray_mode, z[S] shared, pixel out [R]).
 * type_ct != 0: img = prod exp(-mu*dz*||d||), last dz = 1e10;  type_ct == 0: img = prod exp(-mu). */
int afx_project_volume(const float* vol, int32_t nx, int32_t ny, int32_t nz, const double origin[3], const double spacing[3],
                       float fill_value, const afx_render_args* args, int type_ct, void* stream);

/* ---- Occupancy-grid acceleration of the training loop (nerf/run_nerf_acc.py:196-198,284-287;
 * nerf/nerf_helpers_acc.py:10-31,65-78).  Upstream these are nerfacc 0.3.x calls (OccupancyGrid.every_n_step,
 * ray_marching with alpha_fn, render_visibility); nerfacc is neither vendored nor pinned by the reference and absent
 * here, so the entry points implement its published algorithm (parity unpinned at that boundary; restated for the
 * tests in oracle/).  The MLP evaluations between the steps are afx_mlp_infer calls on the points emitted here;
 * exclusive scans of the per-ray counts are the caller's (one cumsum).  All buffers are the caller's. */
typedef struct afx_grid_desc {
  float roi_aabb[6];            /* xmin ymin zmin xmax ymax zmax */
  int32_t resolution[3];
} afx_grid_desc;

/* OccupancyGrid._update, step 1: x = (cell + u) / resolution * (hi - lo) + lo for the n selected cells (cell_idx NULL:
 * cells 0..n-1).  jitter[n,3] in [0,1) supplied by the caller (parity mode), or NULL: drawn in-kernel from the
 * counter-based Philox4x32-10 stream (seed, stream_id) (perf mode). */
int afx_grid_points(const afx_grid_desc* grid, const int32_t* cell_idx, int64_t n, const float* jitter, uint64_t seed,
                    uint64_t stream_id, float* pts, void* stream);
/* step 2: occs[c] = max(occs[c] * ema_decay, occ_new) for the selected cells; deterministic when a cell is selected more
 * than once (max over its draws).  occs_scratch: n_cells floats (snapshot of occs).  cell_idx (here and in afx_grid_points): every index
 * in [0, num_cells), unchecked - a check would need a device read; NULL: cells 0..n-1, n <= num_cells.  A selected cell first drops to
 * its decayed value, taken once from the snapshot however often it is drawn (not above 0: +0), then rises to the largest of its draws
 * that are > 0; draws that are 0, negative or NaN change nothing, and cells that are not selected keep their bits. */
int afx_grid_update(const afx_grid_desc* grid, float* occs, float* occs_scratch, const int32_t* cell_idx, int64_t n,
                    const float* occ_new, float ema_decay, void* stream);
/* step 3: binary[c] = occs[c] > min(mean(occs), occ_thre) as bytes (the module's `binary` tensor) and as the packed
 * bitfield the march reads (n_cells/32 words, rounded up).  partial_ws: 256 doubles. */
int afx_grid_binarize(const afx_grid_desc* grid, const float* occs, float occ_thre, uint8_t* binary, uint32_t* bits,
                      double* partial_ws, void* stream);

/* Restoring a trained grid: the reference assigns `acc_grid._binary = grid_occupancy` (visualization/visualization.py:162)
 * before query_occ / acc_ray_marching.  Packs a caller-supplied byte mask binary[n_cells] (non-zero = occupied) into the
 * bitfield the march reads. */
int afx_grid_pack(const afx_grid_desc* grid, const uint8_t* binary, uint32_t* bits, void* stream);

/* ---- The grid refresh on the device (OccupancyGrid.every_n_step's update with the cell draw made on the GPU): no allocation, no
 * synchronisation, no copy to the host (device-to-device copies only), so the calls can be captured into a HIP graph.
 *
 * Draw rule of the post-warm-up cells (exact; tests restate it from afx_philox_uniform).  N = num_cells, n = n_draw (nerfacc: N / 4),
 * n_occ = set bits of `bits` (the cells past N in the last word are ignored), u24_i = top 24 bits of number i of the Philox4x32-10 stream
 * (seed, AFX_GRID_SELECT_TAG | step), i.e. afx_philox_uniform's u_i * 2^24:
 *   cells[i]     = (u24_i * N) >> 24                                   i < n          (uniform cells)
 *   cells[n + j] = occupied cell of rank (u24_(n+j) * n_occ) >> 24    j < n, when n < n_occ
 *                = occupied cell of rank j                            j < n_occ, otherwise (all occupied cells, index order)
 * (ranks count the occupied cells in index order from 0).  The selected count n + min(n, n_occ) stays on the device.
 * The in-cell jitter of the refresh is afx_grid_points' Philox stream (seed, AFX_GRID_JITTER_TAG | step). */
#define AFX_GRID_JITTER_TAG 0x4752494400000000ull   /* "GRID" << 32 */
#define AFX_GRID_SELECT_TAG 0x53454C4300000000ull   /* "SELC" << 32 */

/* The draw alone: cells_out[2 n_draw] (int32; slots behind the count unwritten), count_dev[1] (int64) = n_draw + min(n_draw, n_occ).  The step is
 * *step_dev (device int64, read when the kernels run) or, with step_dev NULL, `step`; 0 <= step < 2^32.  workspace:
 * afx_grid_select_workspace_bytes(grid) bytes of device memory.  1 <= n_draw <= num_cells < 2^31. */
size_t afx_grid_select_workspace_bytes(const afx_grid_desc* grid);
int afx_grid_select_cells(const afx_grid_desc* grid, const uint32_t* bits, int64_t n_draw, uint64_t seed, int64_t step, const int64_t* step_dev,
                          int32_t* cells_out, int64_t* count_dev, void* workspace, size_t workspace_bytes, void* stream);

/* One refresh of one grid, in place: the cells (all of them with all_cells != 0 - warm-up -, else the draw above from `bits`), one jittered
 * point per cell (afx_grid_points, stream AFX_GRID_JITTER_TAG | step), occupancy = sigmoid(MLP) (afx_mlp_infer with apply_sigmoid, at `prec`
 * on `prepared`; after the draw a launch over the capacity 2 n_draw bounded by the device count), then afx_grid_update's snapshot, decay and
 * EMA (ema_decay) and afx_grid_binarize (occ_thre) into occs, binary and bits.  Equal bit for bit to that sequence of entry points on the same
 * cells.  workspace: afx_grid_refresh_workspace_bytes(grid, n_draw, all_cells) bytes (-1: invalid arguments, see afx_last_error); a smaller
 * one returns AFX_E_WORKSPACE before anything is written.  AFX_E_INVALID: null pointers, n_draw <= 0 or > num_cells (when all_cells == 0),
 * num_cells >= 2^31, a capacity (num_cells or 2 n_draw) beyond afx_mlp_infer's 2^31 - 256 points, a host step outside [0, 2^32). */
typedef struct afx_grid_refresh_args {
  afx_grid_desc grid;
  float* occs;                  /* [num_cells] */
  uint8_t* binary;              /* [num_cells] */
  uint32_t* bits;               /* [(num_cells + 31) / 32]: read by the draw, rewritten at the end */
  int32_t all_cells;            /* 1: every cell (warm-up); 0: the draw */
  int64_t n_draw;
  uint64_t seed;
  int64_t step;                 /* used when step_dev is NULL */
  const int64_t* step_dev;      /* device int64: the training step, read when the kernels run */
  float occ_thre, ema_decay;
  void* workspace;
  size_t workspace_bytes;
} afx_grid_refresh_args;
int64_t afx_grid_refresh_workspace_bytes(const afx_grid_desc* grid, int64_t n_draw, int32_t all_cells);
int afx_grid_refresh(afx_ctx* ctx, int prec, const void* prepared, const afx_grid_refresh_args* args, void* stream);

/* nerfacc.ray_marching: t range = ray / scene_aabb intersection clipped to [near, far]; fixed-step lattice
 * t_min + k*step; a step belongs to the ray while its mid-point lies before t_max (nerfacc marches `while (t_mid < far)`) and
 * is kept when the cell holding its mid-point is occupied (grid_bits NULL: every step). */
typedef struct afx_march_args {
  const float* origins;         /* [R,3] */
  const float* dirs;            /* [R,3] */
  int64_t n_rays;
  int32_t has_aabb;  float scene_aabb[6];
  int32_t has_near, has_far;  float near_plane, far_plane;
  float step;                   /* render_step_size */
  const uint32_t* grid_bits;    /* from afx_grid_binarize, or NULL */
  afx_grid_desc grid;
} afx_march_args;
int afx_march_count(const afx_march_args* args, int32_t* counts, void* stream);                    /* kept steps per ray */
/* packed, ray-sorted samples at offsets = exclusive scan of the counts; mid_points optional [n,3] = o + d*(t_s+t_e)/2 */
int afx_march_write(const afx_march_args* args, const int64_t* offsets, int32_t* ray_indices, float* t_starts,
                    float* t_ends, float* mid_points, void* stream);
/* alpha_fn of nerf_helpers_acc.py:11-25 on the raw MLP output of the candidates + nerfacc's render_visibility: steps with
 * alpha < alpha_thre are dropped without attenuating the transmittance, the ray ends once it falls below early_stop_eps.
 * input_is_alpha != 0: `raw` already holds the caller's alpha_fn values.  offsets[R+1]; keep[n] in {0,1}; counts[r] = kept steps. */
int afx_march_visibility(const float* raw, int32_t input_is_alpha, const float* t_starts, const float* t_ends, const int64_t* offsets,
                         int64_t n_rays, float early_stop_eps, float alpha_thre, uint8_t* keep, int32_t* counts, void* stream);
/* counts[R] (afx_march_count / afx_march_visibility) -> offsets[R+1], the exclusive prefix sums both take back; optionally (non-null)
 * group_offsets[R+1], the same over ceil(count / 32) - the offsets of the group-aligned copy afx_pack_groups lays out - and
 * totals[2] = {samples, groups} for the caller's one host read.  One launch in place of the caller's zeros / cumsum sequence. */
int afx_ray_offsets(const int32_t* counts, int64_t n_rays, int64_t* offsets, int64_t* group_offsets, int64_t* totals, void* stream);
int afx_march_compact(const uint8_t* keep, const int64_t* offsets_in, const int64_t* offsets_out, int64_t n_rays,
                      const float* t_starts_in, const float* t_ends_in, int32_t* ray_indices_out, float* t_starts_out,
                      float* t_ends_out, void* stream);

/* The whole grid iteration of nerf/run_nerf_acc.py:284-306 in ONE call: afx_march_count / afx_ray_offsets / afx_march_write (candidates),
 * afx_mlp_infer at the candidates' mid-points + afx_march_visibility (the reference's alpha_fn + nerfacc's render_visibility),
 * afx_march_compact / afx_pack_groups, afx_train_step_packed_mse - the same entry points in the same order, so the results are those of
 * the call-by-call sequence bit for bit.  (At the reference's batch the GPU is busy for 0.27 ms of an iteration; the ~30 launches cost more
 * when a Python loop issues them.)  Two host read-backs inside (sizes are data: the host polls a mapped mailbox, or copies and
 * synchronises where no mapped memory can be had), so the call is NOT graph-capturable - see afx_march_train_step_mse_capturable below.  Every array
 * between the steps lives in `workspace`; when it is too small the call returns AFX_E_WORKSPACE with `workspace_needed` set (nothing the
 * caller owns has been written) - grow and call again.  n_kept == 0 on return: no sample survived, pixel / grad_flat untouched (the
 * reference skips the optimizer step, :293). */
typedef struct afx_march_train_args {
  afx_march_args march;             /* rays, scene box, planes, step, occupancy bits: as for afx_march_count */
  float early_stop_eps, alpha_thre; /* render_visibility thresholds (run_nerf_acc.py:68-70) */
  const float* target;              /* [R] */
  float inv_n;                      /* 1 / rays of the global batch */
  float* pixel;                     /* [R] out */
  float* grad_flat;                 /* += dL/dparams */
  void* workspace; size_t workspace_bytes;
  int64_t n_candidates, n_kept, n_groups;      /* out */
  size_t workspace_needed;                     /* out, with AFX_E_WORKSPACE */
} afx_march_train_args;
int afx_march_train_step_mse(afx_ctx* ctx, int prec, const void* prepared, afx_march_train_args* args, void* stream);

/* The same iteration with its sizes kept on the device: no host read-back, synchronisation or allocation, so the call can be captured
 * into a HIP graph and replayed.  Same entry-point sequence and arguments as afx_march_train_step_mse (f16s8 only; the march needs a far
 * plane) and the same results bit for bit: every buffer is carved for the worst case - every step of every ray occupied, the bound
 * afx_march_max_steps gives - every launch is sized for it, and the kernels bound their work by the counts the offsets kernels leave on the
 * device.  Out (device memory, written by the call's kernels): counts_dev[3] = (n_candidates, n_kept, n_groups); skip_dev[1] = 1.0f when
 * nothing survived the march (pixel and grad_flat are then untouched), else 0.0f - usable as an optimizer's found-inf flag.  The
 * host-side n_candidates / n_kept / n_groups of `args` are not written.  The workspace must hold afx_march_train_workspace_bytes(ctx, prec,
 * n_rays, afx_march_max_steps(&args->march)) bytes (else AFX_E_WORKSPACE with workspace_needed set); a worst case beyond the one-chunk
 * sample limit of the packed step (2^32 / width group-padded samples) is refused with AFX_E_INVALID. */
int64_t afx_march_max_steps(const afx_march_args* args);      /* >= the steps k_march_count can give any ray; -1: error */
int64_t afx_march_train_workspace_bytes(const afx_ctx* ctx, int prec, int64_t n_rays, int64_t max_steps_per_ray);      /* -1: error */
int afx_march_train_step_mse_capturable(afx_ctx* ctx, int prec, const void* prepared, afx_march_train_args* args, int64_t* counts_dev,
                                        float* skip_dev, void* stream);

/* The same iteration with ONE evaluation of the model: the packed step's forward half runs over the march's candidates (group-aligned) and
 * doubles as the alpha pass - visibility is decided on its own raw output with afx_march_visibility's arithmetic, the optical depth of the kept
 * samples is summed in the order of the compacted list, and the backward half and weight gradients run over the candidate rows with dL/draw = 0
 * for dropped samples.  Nothing is compacted; the only data-dependent size is the candidate count, kept on the device, so the call is
 * graph-capturable (no host read-back, synchronisation or allocation).  Same arguments and out-contract as afx_march_train_step_mse_capturable
 * (counts_dev[3] = (n_candidates, n_kept, n_kept_groups) - the kept groups being those the compacted list would have; skip_dev[1] = 1.0f when
 * nothing was kept: pixel and grad_flat untouched).  Relation to the two-evaluation step: where the forward half's raw output equals
 * afx_mlp_infer's at the mid-points (tests/test_gpu_grid_single_eval.py pins it), the counters, pixels, loss and skip flag are equal bit for bit;
 * the weight gradient sums over the candidate rows in another order and agrees to the f16s8 tolerance.  The backward work grows with the candidates,
 * not the kept samples.  f16s8, ReLU, no input encoding, a far plane; the workspace must hold afx_march_single_eval_workspace_bytes(ctx, prec,
 * n_rays, afx_march_max_steps(&args->march)) bytes (else AFX_E_WORKSPACE with workspace_needed set); a worst case beyond the one-chunk sample
 * limit is refused with AFX_E_INVALID. */
int64_t afx_march_single_eval_workspace_bytes(const afx_ctx* ctx, int prec, int64_t n_rays, int64_t max_steps_per_ray);      /* -1: error */
int afx_march_train_step_mse_single_eval(afx_ctx* ctx, int prec, const void* prepared, afx_march_train_args* args, int64_t* counts_dev,
                                         float* skip_dev, void* stream);

/* Forward-only render through the occupancy grid with ONE evaluation of the model: the evaluation renders of the reference
 * (nerf/run_nerf_acc.py:338-349 under the grid; visualization/visualization.py:335-352, with the binary image) - acc_ray_marching (march,
 * alpha pass, render_visibility), get_predictions over the kept samples, acc_render_volume_density - without evaluating the kept samples
 * a second time.  Inside: the march (afx_march_count, afx_ray_offsets, afx_march_write: candidates and their mid-points), afx_mlp_infer
 * at the mid-points (any precision and activation it takes), then one per-ray kernel that decides the kept set with afx_march_visibility's
 * arithmetic and multiplies exp(-sigmoid(raw) (t_e - t_s)) over the kept samples in order, as afx_composite_packed does.  Each sample's raw
 * output is a function of its own point, so the pixels equal the operator sequence's bit for bit.
 * Rays: ray_mode AFX_RAYS_ARRAYS - march.origins / march.dirs, march.n_rays rays; AFX_RAYS_POSE - generated in-kernel as afx_render_forward
 * does without ray_ids (ray r = ray_id0 + r of [n_proj, height, width]; n_rays rays; march.origins / dirs / n_rays are ignored).
 * grid_bits == NULL: every step inside the box / planes is a candidate.  Outputs: pixel [R] (required); binary_pixel [R] (optional: the
 * same product with sigma forced to 0 where sigmoid(raw) < binary_thresh, visualization.py:349-352); kept_counts [R] (optional); on the
 * host, n_candidates.  A ray without candidates gets 1.
 * ONE host read-back per call (the candidate count: the host polls a mapped mailbox, or copies and synchronises where no mapped
 * memory can be had, as afx_march_train_step_mse does), so the call is NOT graph-capturable.  Every buffer is carved for the worst case before the first launch:
 * every step of every ray a candidate, afx_march_max_steps(&march) steps (the march needs a far plane); the workspace must hold
 * afx_march_render_workspace_bytes(ray_mode, R, that bound) bytes, else AFX_E_WORKSPACE with workspace_needed set and nothing the caller owns
 * written.  A worst case beyond afx_mlp_infer's 2^31 - 256 points per call is refused with AFX_E_INVALID: split the rays. */
typedef struct afx_march_render_args {
  afx_march_args march;             /* scene box, planes, step, occupancy bits; the rays in AFX_RAYS_ARRAYS mode */
  int32_t ray_mode;                 /* AFX_RAYS_ARRAYS or AFX_RAYS_POSE */
  const double* poses;              /* [n_proj,3,4] row-major cam->world, device (AFX_RAYS_POSE) */
  int32_t width, height;
  double focal;
  int64_t ray_id0, n_rays;          /* AFX_RAYS_POSE */
  float early_stop_eps, alpha_thre; /* render_visibility thresholds */
  float* pixel;                     /* out [R] */
  float* binary_pixel;              /* optional out [R] */
  float binary_thresh;
  int32_t* kept_counts;             /* optional out [R] */
  void* workspace; size_t workspace_bytes;
  int64_t n_candidates;             /* out */
  size_t workspace_needed;          /* out, with AFX_E_WORKSPACE */
} afx_march_render_args;
int64_t afx_march_render_workspace_bytes(int32_t ray_mode, int64_t n_rays, int64_t max_steps_per_ray);      /* -1: error */
int afx_march_render(afx_ctx* ctx, int prec, const void* prepared, afx_march_render_args* args, void* stream);

/* Indices of the k largest of keys[n] (ties: lowest index first), written in ASCENDING INDEX order - the selection step of the
 * weighted ray sampler (the batch of nerf/nerf_helpers.py:137-150 is a set; its order carries no meaning).  Radix select:
 * three histogram passes + a counted compaction, deterministic, no full sort.  workspace: afx_topk_workspace_bytes(n) bytes
 * of device memory; n < 2^32. */
size_t afx_topk_workspace_bytes(int64_t n);
int afx_topk_indices(const float* keys, int64_t n, int64_t k, int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);

/* The ray batches of `n_batches` consecutive training iterations in one launch sequence: out_idx[b][k] = what afx_sample_keys(weights, n,
 * u = NULL, seed, stream_id0 + b) followed by afx_topk_indices(k) returns, bit for bit (sample_pixel_rays draws one batch per iteration,
 * nerf/run_nerf_acc.py:277; a draw is 11 launches of a few microseconds - launch latency, 5 % of the reference's 1.3 ms iteration - and the
 * draws of different iterations are independent, so they share the launches: blockIdx.y = b).  workspace:
 * afx_sample_batches_workspace_bytes(n, n_batches) bytes of device memory (the keys of every batch: n_batches x n floats); n < 2^32,
 * n_batches <= 65535. */
size_t afx_sample_batches_workspace_bytes(int64_t n, int32_t n_batches);
int afx_sample_batches(const float* weights, int64_t n, uint64_t seed, uint64_t stream_id0, int32_t n_batches, int64_t k, int64_t* out_idx,
                       void* workspace, size_t workspace_bytes, void* stream);
/* afx_sample_batches with the first stream id in device memory: batch b uses Philox stream (seed, *stream_id0_dev + b), and the value is
 * read by the kernels when they run, not by the host when the call is issued - out_idx equals afx_sample_batches(..., stream_id0 = that
 * value, ...) index for index (the same kernels).  The call is launches only - no host read-back, synchronisation or allocation - so it can
 * be captured into a HIP graph, whose replays follow the counter.  The counter is taken as non-negative and below 2^32 (the range of the
 * refresh step).  Same workspace.  AFX_E_INVALID (before any HIP call): a null stream_id0_dev, out_idx or workspace, n_batches outside
 * 1..65535, n outside 1..2^32 - 1, k outside 0..n. */
int afx_sample_batches_dev(const float* weights, int64_t n, uint64_t seed, const int64_t* stream_id0_dev, int32_t n_batches, int64_t k,
                           int64_t* out_idx, void* workspace, size_t workspace_bytes, void* stream);

/* The host's bookkeeping between two grid training iterations as ONE single-lane kernel, so that a HIP graph can hold several iterations
 * (render.GridTrainRoundGraph captures it behind every iteration's optimizer step).  With s = *step_dev, in this order:
 *   lr_dev[0] = lr_table[min(s, n_table - 1)]           the learning rate of the NEXT iteration, from a table the host built (a pow on the
 *                                                        device would not reproduce the host's double-precision schedule bit for bit);
 *   loss_hist[s % round_len] = *loss;  counts_hist[s % round_len][0..2] = counts[0..2];  skip_hist[s % round_len] = *skip;
 *   *last_loss = *skip > 0 ? *last_loss : *loss         the loss of the last step that kept samples;
 *   *n_marched += counts[1];  *step_dev = s + 1.
 * skip / counts: the outputs of afx_march_train_step_mse_capturable (or _single_eval); loss: one float on the device.  Every pointer is
 * device memory; every write is a plain vector store.  AFX_E_INVALID (before any HIP call): a null pointer, n_table < 1, round_len < 1. */
typedef struct afx_train_round_args {
  int64_t* step_dev;            /* the iteration counter */
  const float* lr_table;        /* [n_table] */
  int64_t n_table;
  float* lr_dev;                /* [1] the optimizer's device-resident learning rate */
  const float* skip;            /* [1] */
  const float* loss;            /* [1] */
  const int64_t* counts;        /* [3] candidates, kept samples, groups */
  int64_t round_len;
  float* loss_hist;             /* [round_len] */
  int64_t* counts_hist;         /* [round_len][3] */
  float* skip_hist;             /* [round_len] */
  float* last_loss;             /* [1] */
  int64_t* n_marched;           /* [1] */
} afx_train_round_args;
int afx_train_round_advance(const afx_train_round_args* args, void* stream);

/* ---- Device-resident ray batches (sample_pixel_rays, nerf/nerf_helpers.py:137-150: weighted sampling without
 * replacement over all pixels of all training projections).  keys[i] = log(u_i) / w_i (Efraimidis-Spirakis): the k
 * largest keys are a weighted sample without replacement; u[n] supplied, or NULL: Philox stream (seed, stream_id).
 * afx_gather_rays copies the selected rows of the resident ray table. */
int afx_sample_keys(const float* weights, int64_t n, const float* u, uint64_t seed, uint64_t stream_id, float* keys, void* stream);
int afx_gather_rays(const float* origins, const float* dirs, const float* pixels, const int64_t* idx, int64_t k,
                    float* origins_out, float* dirs_out, float* pixels_out, void* stream);
/* out[i] = uniform [0,1) number i of Philox4x32-10 stream (seed, stream_id): the generator of every "perf mode" draw */
int afx_philox_uniform(uint64_t seed, uint64_t stream_id, int64_t n, float* out, void* stream);

/* ---- Ray-sampling weights of the projections (sampling_strategy='frangi' | 'segmentation'; phantomdata/cttoray.py:210-216 and
 * get_weighted_img, phantomdata/helpers.py:226-247).  N images of one size h x w, row-major fp64 [N, h, w], in one fixed sequence of
 * launches whatever N and the number of scales.  fp64 throughout, no floating-point atomics (deterministic), nothing allocated or
 * synchronised (hipGraph-capturable); the image must be memory of the current device.  AFX_E_INVALID: null pointers, n outside
 * 1..65535, h or w outside 1..16384 (2..16384 wherever a Hessian is taken), a bad sigma list or beta / gamma <= 0.  A workspace smaller
 * than the query (the queries return 0 for arguments the call refuses) gives AFX_E_WORKSPACE, with *workspace_needed set when it is
 * not NULL.
 *
 * afx_frangi: the Frangi vesselness filter as scikit-image 0.18.3 computes it (filters.ridges.frangi; 0.19 changed the default gamma,
 * the Hessian and the background rule).  For each image I and each sigma in sigmas[n_sigmas] (1..16 values, each > 0 with
 * int(4 sigma + 0.5) <= 1000):
 *   1. black_ridges != 0: I <- 1 - I
 *   2. G = scipy.ndimage.gaussian_filter(I, sigma): separable (axis 0, then axis 1), radius r = int(4 sigma + 0.5), weights
 *      exp(-j^2 / 2 sigma^2) normalised to sum 1, mode 'reflect' (d c b a | a b c d | d c b a, period 2n, also for r >= n)
 *   3. np.gradient of G along both axes, np.gradient of those (unit spacing, central inside, one-sided at the edges): Hrr, Hrc, Hcc
 *   4. times sigma^2
 *   5. l+- = (Hrr + Hcc) / 2 +- sqrt(4 Hrc^2 + (Hrr - Hcc)^2) / 2; lambda1 the one of smaller |l| (a tie: l+), lambda2 the other
 *   6. v = exp(-rb / 2 beta^2) (1 - exp(-(lambda1^2 + lambda2^2) / 2 gamma^2)), rb = (lambda1 / d)^2, d = |lambda2| (1e-10 where 0);
 *      v = 0 where lambda2 > 0 (alpha has no effect in 2-D: there is no alpha argument)
 *   7. out = max over the scales of v
 * Workspace: 2 regions of N x n_sigmas x h x w doubles, each rounded up to 256 bytes.
 *
 * afx_distance_transform_edt: scipy.ndimage.distance_transform_edt per image, bit for bit: the distance from every non-zero pixel to the
 * nearest zero pixel (sqrt of the exact integer squared distance in fp64); +inf everywhere in an image without a zero pixel.
 * Workspace: N x h x w uint32, rounded up to 256 bytes.
 *
 * afx_sampling_weights: strategy AFX_SAMPLING_FRANGI - binary == 0: pixels > np.percentile(img, 10) ('linear') are set to 1 first;
 * f = afx_frangi(img, sigmas, beta, gamma, black ridges); f = (f - min f) / (max f - min f); e = EDT(f); out = (e - min e) / (max e -
 * min e) + 1e-10 (cttoray.py passes beta = 0.5 and alpha = 12 (binary) / 0.5, which has no effect).  Where a max - min is 0 the reference
 * divides by zero: out is NaN for that image and status[i] (when status is not NULL) gets bit 1 (flat vesselness) and / or bit 2 (flat
 * distance transform); status[i] = 0 otherwise.  AFX_SAMPLING_SEGMENTATION - the host sampling_weights(img, 'segmentation') of
 * phantomdata/dataset.py: mask = img < 1, min-subtracted and divided by its max when that is > 0, e = EDT(mask), the same normalisation
 * skipped when max e - min e is 0, + 1e-10 (sigmas, beta, gamma, binary ignored; status[i] = 0).
 * Workspace (afx_sampling_weights_workspace_bytes; n_sigmas ignored for segmentation): in order, each rounded up to 256 bytes, N doubles,
 * 2 N doubles, 2 N doubles, N x h x w uint32, then (frangi) afx_frangi's two planes. */
enum { AFX_SAMPLING_FRANGI = 0, AFX_SAMPLING_SEGMENTATION = 1 };
size_t afx_frangi_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t n_sigmas);
int afx_frangi(const double* img, int32_t n, int32_t h, int32_t w, const double* sigmas, int32_t n_sigmas, double beta, double gamma,
               int32_t black_ridges, double* out, void* workspace, size_t workspace_bytes, size_t* workspace_needed, void* stream);
size_t afx_distance_transform_edt_workspace_bytes(int32_t n, int32_t h, int32_t w);
int afx_distance_transform_edt(const double* x, int32_t n, int32_t h, int32_t w, double* out, void* workspace, size_t workspace_bytes,
                               size_t* workspace_needed, void* stream);
size_t afx_sampling_weights_workspace_bytes(int32_t strategy, int32_t n, int32_t h, int32_t w, int32_t n_sigmas);
int afx_sampling_weights(const double* img, int32_t n, int32_t h, int32_t w, int32_t strategy, int32_t binary, const double* sigmas,
                         int32_t n_sigmas, double beta, double gamma, double* out, int32_t* status, void* workspace, size_t workspace_bytes,
                         size_t* workspace_needed, void* stream);

/* ---- Metrics of the evaluation sweep (visualization/visualization.py: SSIM per view :267, 411-417; DICE 3D / DOT 3D :203-231, 480-495).
 * Device pointers; the calls allocate nothing, never synchronise and use no floating-point atomics: results are bitwise reproducible and
 * the calls can be captured in a graph.
 *
 * afx_ssim: out[i] = SSIM(preds[i], targets[i]) (fp64) for n pairs of h x w fp32 images, row-major [n][h][w] - torchmetrics'
 * StructuralSimilarityIndexMeasure(data_range=1.0) (_ssim_update, gaussian kernel), computed in fp64:
 *   g[m] = exp(-((m - 5) / 1.5)^2 / 2), m = 0..10, normalised to sum 1; the 2-D window is g g^T (applied separably)
 *   over every 11 x 11 window lying inside the image: mu_x, mu_y, E[x^2], E[y^2], E[xy] (window means)
 *   s_x^2 = max(E[x^2] - mu_x^2, 0), s_y^2 = max(E[y^2] - mu_y^2, 0), s_xy = E[xy] - mu_x mu_y, c1 = 0.01^2, c2 = 0.03^2
 *   map = ((2 mu_x mu_y + c1)(2 s_xy + c2)) / ((mu_x^2 + mu_y^2 + c1)(s_x^2 + s_y^2 + c2))
 *   out[i] = mean of the map over the (h - 10) x (w - 10) windows (torchmetrics pads by 5 and crops 5 from every side: the same windows)
 * A view's result does not depend on n or on the other views.  AFX_E_INVALID: a null pointer, n < 1, h < 11, w < 11, h w > 2^31 - 1, or
 * n ceil((h - 10) / 16) ceil((w - 10) / 64) > 2^24 - 1 (workgroups of one launch).  Workspace (afx_ssim_workspace_bytes; 0 for those
 * shapes): n ceil((h - 10) / 16) ceil((w - 10) / 64) doubles (per-tile partial sums), rounded up to 256 bytes; AFX_E_WORKSPACE when it
 * is smaller, with workspace_needed (when not NULL) set.
 *
 * afx_volume_grid: the ground-truth density grid, out[i][j][k] (fp32, n^3) = mu(t[j], t[i], t[k]) (np.meshgrid(t, t, t) with its 'xy'
 * order, as the reconstructed grid is laid out), t = np.linspace(lo, hi, n) in fp64 - t[m] = m ((hi - lo) / (n - 1)) + lo, t[n - 1] = hi -
 * rounded to fp32.  mu is afx_project_volume's lookup: trilinear on the regular grid vol[nx][ny][nz] (axis a: origin[a] + spacing[a] x
 * index), fill_value outside it, in fp64 (scipy RegularGridInterpolator(method='linear', bounds_error=False, fill_value)), rounded to fp32.
 * AFX_E_INVALID: a null pointer, fewer than 2 voxels on an axis, a spacing <= 0, n < 2 or n > 2^20, lo >= hi or either not finite. */
size_t afx_ssim_workspace_bytes(int32_t n, int32_t h, int32_t w);
int afx_ssim(const float* preds, const float* targets, int32_t n, int32_t h, int32_t w, double* out, void* workspace, size_t workspace_bytes,
             size_t* workspace_needed, void* stream);
int afx_volume_grid(const float* vol, int32_t nx, int32_t ny, int32_t nz, const double origin[3], const double spacing[3], float fill_value,
                    double lo, double hi, int32_t n, float* out, void* stream);

/* ---- Surface-distance scores of the 3-D reconstruction: the Dice of the vessel class, the average symmetric surface distance, the
 * Hausdorff distance and its percentile (medpy.metric.binary dc / assd / hd / hd95 at unit spacing).  The rules above hold: device
 * pointers, nothing allocated or synchronised, no floating-point atomics (integer atomics only, so every result is independent of the
 * order of execution), hipGraph-capturable, the same bits on every run.
 *
 * afx_distance_transform_edt_3d: the exact Euclidean distance transform of a uint8 volume fg[n0][n1][n2] (row-major; non-zero =
 * foreground).  d2 (uint32, required): the integer squared distance, in voxels, from every voxel to the nearest zero voxel - 0 at a zero
 * voxel, AFX_EDT3D_NONE everywhere when the volume has no zero voxel.  dist (fp64, may be NULL): sqrt((double)d2), +inf for
 * AFX_EDT3D_NONE (afx_distance_transform_edt's convention; scipy.ndimage.distance_transform_edt bit for bit wherever a zero voxel
 * exists).  Three separable passes in integer arithmetic: the nearest zero along axis 2 (a wave per line), then along axis 1 and along
 * axis 0 the exact lower envelope min over c' of g(c') + (c - c')^2, a workgroup taking a tile of 32 (lines of up to 512 voxels) or 16
 * adjacent lines into LDS, so that the global loads and stores of the strided passes run along axis 2.
 * AFX_E_INVALID: a null fg or d2, an axis outside 1..1024 (squared distances stay below 2^22, a tile of lines fits in 64 KiB of LDS;
 * n0 n1 n2 <= 2^30 follows).  Workspace (afx_distance_transform_edt_3d_workspace_bytes; 0 for a refused shape): n0 n1 n2 uint16 (the
 * distances of the first pass), rounded up to 256 bytes; AFX_E_WORKSPACE when smaller, with *workspace_needed (when not NULL) set.
 *
 * afx_surface_metrics_3d: pred and gt are fp32 volumes [n0][n1][n2];  A = pred >= thr_pred, B = gt >= thr_gt (a NaN is outside);
 * S(M) = the voxels of M with at least one of the 6 face neighbours outside M, a neighbour beyond the grid counting as outside
 * (M & ~scipy.ndimage.binary_erosion(M, generate_binary_structure(3, 1), border_value=0));  D_A->B = the multiset { EDT(~S(B))[v] :
 * v in S(A) }, D_B->A likewise.  One fixed launch sequence (masks and counts, two EDTs, a gather with the first histogram, a scan, the
 * second histogram, the finish) writes `record`, AFX_SURFACE_RECORD_SLOTS slots of 8 bytes on the device:
 *   [0] |A|  [1] |B|  [2] |A & B|  [3] |S(A)|  [4] |S(B)|                                   uint64
 *   [5] sum of D_A->B  [6] sum of D_B->A                                                   fp64: per-workgroup partials (a tree), summed
 *                                                                                          strided per thread, then a tree - a fixed order
 *   [7] max d^2 of D_A->B  [8] max d^2 of D_B->A                                           uint64 (squared voxel distances)
 *   [9] [10] the d^2 at indices floor(v) and min(floor(v) + 1, M - 1) of the sorted merged multiset D_A->B + D_B->A, M = |S(A)| +
 *            |S(B)|: the two values np.percentile(..., q) ('linear') interpolates between               uint64
 *   [11] v = (M - 1) * (q / 100), the virtual index, computed in fp64 on the device                      fp64
 *   [12] status: bit 1 (value 1) A is empty, bit 2 (value 2) B is empty                                  uint64
 *   [13..15] zero
 * With status != 0 no surface distance exists: [5], [6] and [11] are NaN, [7]..[10] are AFX_EDT3D_NONE.  The order statistics come
 * from a radix select over the 22-bit keys (two passes of 11 bits, LDS histograms added to global ones with integer atomics, as
 * afx_topk_indices does).  AFX_E_INVALID: a null pred, gt or record, an axis outside 1..1024, a NaN threshold, q outside [0, 100].
 * Workspace (afx_surface_metrics_3d_workspace_bytes; 0 for a refused shape), each region rounded up to 256 bytes, N = n0 n1 n2: two
 * uint8 [N] (~S(A), ~S(B)), uint16 [N] (the EDT's), two uint32 [N] (the squared distance fields), 2 x 2048 doubles (partial sums),
 * 3 x 2048 uint32 (histograms) and 256 bytes of counters. */
#define AFX_EDT3D_NONE 0xffffffffu
#define AFX_EDT3D_MAX_SIDE 1024
#define AFX_SURFACE_RECORD_SLOTS 16
size_t afx_distance_transform_edt_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int afx_distance_transform_edt_3d(const uint8_t* fg, int32_t n0, int32_t n1, int32_t n2, uint32_t* d2, double* dist, void* workspace,
                                  size_t workspace_bytes, size_t* workspace_needed, void* stream);
size_t afx_surface_metrics_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int afx_surface_metrics_3d(const float* pred, const float* gt, int32_t n0, int32_t n1, int32_t n2, float thr_pred, float thr_gt, double q,
                           void* record, void* workspace, size_t workspace_bytes, size_t* workspace_needed, void* stream);

/* ---- Connected components of a 3-D mask: how many pieces a thresholded reconstruction has, how large they are, and the mask without
 * its specks (scipy.ndimage.label with generate_binary_structure(3, connectivity)).  The rules above hold: device pointers, nothing
 * allocated or synchronised, integer atomics only, hipGraph-capturable, the same bits on every run.
 *
 * afx_label_components_3d: fg is a uint8 volume [n0][n1][n2] (row-major; non-zero = foreground); connectivity 1, 2 or 3 joins voxels
 * that differ by 1 along at most that many axes (6, 18 or 26 neighbours); beyond the grid is background.  labels (int32 [n0][n1][n2],
 * required): 0 on the background, 1..K on the components, numbered in the order of their smallest linear index (raster order of their
 * first voxel) - exactly scipy.ndimage.label's numbering, a pure function of the input.  sizes (uint32 [n0 n1 n2], may be NULL):
 * sizes[l - 1] = the voxels of component l; K <= n0 n1 n2 always, and the entries at and beyond K are written as 0.  record:
 * AFX_COMPONENTS_RECORD_SLOTS uint64 slots on the device:
 *   [0] foreground voxels  [1] K  [2] the size of the largest component  [3] its label (0 when K = 0; of equal sizes the smaller
 *   label)  [4] its smallest linear index  [5..7] zero
 * Union-find in global memory (Komura 2015; Playne & Hawick 2018) as one fixed launch sequence with no host loop and no read-back:
 * init (parent[v] = v); merge (every voxel unites itself with the 3, 9 or 13 foreground neighbours before it in raster order:
 * find both roots, atomicMin(&parent[larger], smaller), go on from the returned value if that was not the expected root - roots only
 * ever link to smaller indices, so a component's final root is its smallest linear index); flatten (every voxel's root into `labels`,
 * roots counted per chunk of 2048 voxels); scan (one workgroup); rank (label of a root = 1 + the roots before it); relabel (with the
 * sizes: one integer add per distinct label in a wave, passes of one label combined); finish (the record).
 * AFX_E_INVALID: a null fg, labels or record, an axis outside 1..AFX_EDT3D_MAX_SIDE (indices then fit int32), connectivity outside
 * 1..3.  Workspace (afx_label_components_3d_workspace_bytes; 0 for a refused shape), each region rounded up to 256 bytes, N = n0 n1 n2:
 * two uint32 [N] (the parent links; the sizes when the caller passes none - the query does not know whether the call will, and the
 * record's largest component needs the sizes either way), uint32 [ceil(N / 2048)] (roots per chunk) and 256 bytes of state;
 * AFX_E_WORKSPACE when smaller, with *workspace_needed (when not NULL) set.  Cost at the top of the shape range: the scan and the
 * finish are one workgroup each, over N / 2048 chunk counts and over the K sizes - microseconds for a vessel mask, but K can reach
 * N / 2 (a 6-neighbour checkerboard), about 2 GB read by one workgroup at 1024^3.
 *
 * afx_filter_components_3d: out[v] (uint8) = 1 where labels[v] != 0, sizes[labels[v] - 1] >= min_size and - when largest_only is
 * non-zero - labels[v] is the record's largest label; 0 elsewhere.  labels, sizes and record are those afx_label_components_3d wrote
 * (sizes required here); the record is read on the device, so label-then-filter needs no host round trip.  AFX_E_INVALID: a null
 * pointer, a refused shape, min_size == 0. */
#define AFX_COMPONENTS_RECORD_SLOTS 8
size_t afx_label_components_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int afx_label_components_3d(const uint8_t* fg, int32_t n0, int32_t n1, int32_t n2, int32_t connectivity, int32_t* labels,
                            uint32_t* sizes /* [n0 n1 n2], may be NULL */, void* record, void* workspace, size_t workspace_bytes,
                            size_t* workspace_needed, void* stream);
int afx_filter_components_3d(const int32_t* labels, const uint32_t* sizes, const void* record, int32_t n0, int32_t n1, int32_t n2,
                             int32_t largest_only, uint32_t min_size, uint8_t* out, void* stream);

/* ---- The centreline of a 3-D mask: thinning to medial curves, the skeleton that clDice (Shit et al. 2021) scores a vessel tree by.
 * 8-subfield parallel thinning after Bertrand & Aktouf (1995) with the (26, 6)-simple points of Malandain & Bertrand (1992), defined
 * here so that every implementation gives the same voxels.  The foreground is 26-connected, the background 6-connected, beyond the
 * grid is background.  Passes repeat until one deletes nothing:
 *   1. B = the foreground voxels that have a background face neighbour at the start of the pass (so a pass takes one layer);
 *   2. for s = 0..7 in this order, subfield s = (i0 & 1) * 4 + (i1 & 1) * 2 + (i2 & 1): every voxel of B in subfield s is deleted
 *      when, in the mask as it stands when subfield s starts, it does NOT have exactly one foreground 26-neighbour (curve end points
 *      stay) and is SIMPLE: the foreground of its 26-neighbourhood (centre excluded) is exactly one 26-connected component, and the
 *      background of its 18-neighbourhood holds exactly one 6-connected component (joined inside the 18-neighbourhood) that is
 *      6-adjacent to the centre.
 * Two voxels of one subfield are never 26-neighbours, so deleting a subfield's voxels at once equals deleting them one after another
 * in any order: the result is a pure function of the input, equal voxel for voxel to the sequential restatement, the same bits on
 * every run.  Deleting simple points keeps the 26-components, the 6-cavities and the tunnels (the Euler characteristic); the result
 * is a subset of the input and thinning it again changes nothing.  Which of several equally medial voxels stays depends on the order
 * of the subfields (a solid cube thins to its main diagonal, a tube's end may keep a short spur): a property of the definition;
 * nothing is pruned.
 *
 * afx_skeletonize_3d: fg and skel are uint8 volumes [n0][n1][n2] (row-major; fg: non-zero = foreground; skel: 1 on the skeleton, 0
 * elsewhere; skel may be fg).  record: AFX_SKELETON_RECORD_SLOTS uint64 slots on the device:
 *   [0] passes run (the one that deleted nothing included)  [1] voxels deleted  [2] converged: 1 once a pass has deleted nothing
 *   [3] voxels that remain  [4] voxels the last pass run deleted  [5] foreground voxels of the input  [6..7] zero
 * Launches, all on `stream`, one after another: reset, init (skel = fg != 0, counted), then per pass: mark (B as lists of voxel
 * indices, one list per subfield), 8 subfield launches (each voxel of a list gathers its 26 neighbours into a word, applies the rule
 * and clears itself with a plain store; deletions counted by an integer add per wave), advance (one lane rolls the record).  Every
 * launch of a pass returns at once when the record says converged, so issuing more passes than needed changes nothing.
 * sync_every = 0: exactly max_passes passes are issued, nothing is read back, allocated or synchronised - hipGraph-capturable; look
 * at record[2].  sync_every > 0: after every sync_every passes, and after the last, the call copies record[2] to the host and waits
 * for the stream; it returns at convergence, or after max_passes passes with converged = 0 - still AFX_OK, skel is the mask after
 * that many passes, and afx_last_error() says that it stopped early.  Not capturable in this form.
 * AFX_E_INVALID: a null fg, skel or record, an axis outside 1..AFX_EDT3D_MAX_SIDE, max_passes < 1, sync_every < 0.  Workspace
 * (afx_skeletonize_3d_workspace_bytes; 0 for a refused shape): uint32 [8][ceil(n0 / 2) ceil(n1 / 2) ceil(n2 / 2)], rounded up to 256
 * bytes, and 256 bytes of state; AFX_E_WORKSPACE when smaller.
 *
 * afx_simple_point_26: the predicate SIMPLE on the host, by the very function the kernels call.  nbr holds the 3 x 3 x 3
 * neighbourhood, bit (d0 + 1) * 9 + (d1 + 1) * 3 + (d2 + 1) for the offset (d0, d1, d2); bit 13 (the centre) and bits 27..31 are
 * ignored.  Returns 1 or 0; needs no device. */
#define AFX_SKELETON_RECORD_SLOTS 8
size_t afx_skeletonize_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int afx_skeletonize_3d(const uint8_t* fg, int32_t n0, int32_t n1, int32_t n2, int32_t max_passes, int32_t sync_every, uint8_t* skel,
                       void* record, void* workspace, size_t workspace_bytes, void* stream);
int afx_simple_point_26(uint32_t nbr);

/* ---- The reconstructed vessel as a surface: an indexed triangle mesh of the level set f = iso of a 3-D volume, and its area and
 * enclosed volume.  Marching tetrahedra on the Kuhn (Freudenthal) split of every grid cube, defined here so that every implementation
 * gives the same mesh.  The rules above hold: device pointers, nothing allocated or synchronised, no atomics at all,
 * hipGraph-capturable, the same bits on every run.
 *
 * The volume f is fp32 [n0][n1][n2], row-major; a voxel is INSIDE when f >= iso (afx_surface_metrics_3d's rule).  Values must be
 * finite: a NaN voxel is outside, and the vertices on the edges that lead to it are NaN.  Every cube of eight neighbouring voxels is
 * split into six tetrahedra, one per permutation p of the axes, numbered 0..5 in lexicographic order - (0,1,2) (0,2,1) (1,0,2) (1,2,0)
 * (2,0,1) (2,1,0) - with the corners c0 = the cube's base, c1 = c0 + e[p0], c2 = c1 + e[p1], c3 = c0 + (1,1,1).  The split is the
 * same in every cube, so neighbouring cubes agree on the diagonal of their common face: the surface is that of the continuous
 * piecewise-linear interpolant of f on this triangulation, and no case is ambiguous.
 *   Vertices: one per crossed edge of the triangulation (one end inside, one outside).  An edge belongs to its lexicographically smaller
 *     end a and has one of seven directions d = 0..6: (0,0,1) (0,1,0) (0,1,1) (1,0,0) (1,0,1) (1,1,0) (1,1,1); b = a + direction.  The
 *     vertex ids 0..V-1 increase with the key linear_index(a) * 7 + d: the mesh is welded and its numbering canonical.  Position, every
 *     operation in fp64 and rounded on its own: t = ((double)iso - (double)f[a]) / ((double)f[b] - (double)f[a]); q[x] = (double)a[x] + t
 *     on the axes where b differs from a, (double)a[x] on the others; w[r] = ((o[r] + m[r][0] q[0]) + m[r][1] q[1]) + m[r][2] q[2] with
 *     index_to_world = { m[0][0], m[0][1], m[0][2], o[0], m[1][0], ... o[2] } (12 doubles on the host); w is rounded to fp32.
 *   Triangles: by cube in raster order of its base, then by tetrahedron p = 0..5.  A tetrahedron with one corner L on one side and
 *     X < Y < Z (in the order c0..c3) on the other gives one triangle, of the vertices on L-X, L-Y, L-Z; one with the corners A < B
 *     inside and C < D outside gives two, (AC, AD, BD) and (AC, BD, BC) - the quadrilateral AC, AD, BD, BC cut along AC-BD.  Winding:
 *     the right-hand-rule normal of (v0, v1, v2) in WORLD space points from inside to outside; where that asks for the other
 *     orientation the last two vertices of the triangle are exchanged ((LX, LZ, LY); (AC, BD, AD) and (AC, BC, BD)).  The winding is
 *     therefore reversed when det(m) < 0 (an index_to_world that exchanges two axes, as the density grid's meshgrid 'xy' layout asks).
 *     Voxels exactly equal to iso are inside; the mesh stays combinatorially closed, some of its triangles degenerate to a point or a
 *     line.
 *
 * afx_isosurface_3d: vertices is fp32 [max_vertices][3], triangles int32 [max_triangles][3]; record, AFX_ISOSURFACE_RECORD_SLOTS uint64
 * slots on the device:
 *   [0] V  [1] T  [2] E, the edges of the mesh  [3] B, its boundary edges (edges with one triangle: on the faces of the grid, where the
 *   surface leaves it)  [4] the tetrahedra cut two and two  [5] status: bit 1 (value 1) V exceeds max_vertices, bit 2 (value 2) T exceeds
 *   max_triangles  [6..7] zero
 * The counts are the true ones whatever the capacities; nothing is written at or beyond a capacity (vertices and triangles below it are
 * the same as in a call with room for all; with status bit 1 set, a triangle may name a vertex that was not written).  Both capacities
 * 0 (the arrays may then be NULL) is the counting call.  E and B come from the classification, not from matching edges: every crossed
 * triangular face of the triangulation carries exactly one mesh edge and every two-and-two tetrahedron one more, its diagonal: E = crossed
 * faces + [4], B = the crossed faces in the six outer planes of the grid.  V - E + T is the Euler characteristic of the surface - of the
 * interpolant's level set: the Kuhn split joins a voxel to 14 neighbours, so it is not the Euler number of a 6- or 26-connected mask.
 * An axis of one voxel has no cube: the mesh is empty, every count 0.  Launches: classify (one thread per grid point: its edge mask, the
 * triangles of its cube, the faces it owns, prefixes inside chunks of 1024 points, the chunk sums), scan (one workgroup: the chunk
 * offsets, the record), emit (skipped by the counting call).
 * AFX_E_INVALID: a null f, record or index_to_world; an axis outside 1..AFX_EDT3D_MAX_SIDE; a NaN iso; a capacity below 0 or above
 * 2^31 - 1, or above 0 with a null array; a non-finite entry of index_to_world or det(m) = m00 (m11 m22 - m12 m21) - m01 (m10 m22 -
 * m12 m20) + m02 (m10 m21 - m11 m20) equal to 0 or not finite.  Workspace (afx_isosurface_3d_workspace_bytes; 0 for a refused shape),
 * each region rounded up to 256 bytes, N = n0 n1 n2, C = ceil(N / 1024): uint8 [N] (edge masks), two uint16 [N] (the vertex and triangle
 * prefixes inside a chunk), five uint32 [C] (chunk sums) and two uint64 [C] (chunk offsets: 7 N vertices do not fit 32 bits);
 * AFX_E_WORKSPACE when smaller, with *workspace_needed (when not NULL) set.
 *
 * afx_mesh_measures: out[0] (fp64, device) = the surface area, the sum over the triangles of |(v1 - v0) x (v2 - v0)| / 2; out[1] = the
 * enclosed volume, the sum of (v0 - r) . ((v1 - r) x (v2 - r)) / 6 - positive for a closed mesh wound as above; r = ref_point (3
 * doubles on the host; NULL = the origin), best chosen inside the mesh: the terms then cancel less.  fp64 from the fp32 vertices, no
 * contraction; per-workgroup partial sums (strided per thread, then a tree) and one finishing workgroup: a fixed order for a given
 * max_triangles.  V and T are read from `record` on the device (slots [0] and [1] of afx_isosurface_3d's record, cut to max_vertices
 * and max_triangles), so extract-then-measure needs no host round trip; a triangle that names a vertex outside 0..V-1 adds nothing.
 * AFX_E_INVALID: a null record or out, a capacity below 0 or above 2^31 - 1, or above 0 with a null array, a non-finite ref_point.
 * Workspace (afx_mesh_measures_workspace_bytes): 2 x 2048 doubles; AFX_E_WORKSPACE when smaller. */
#define AFX_ISOSURFACE_RECORD_SLOTS 8
size_t afx_isosurface_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int afx_isosurface_3d(const float* f, int32_t n0, int32_t n1, int32_t n2, float iso, const double index_to_world[12], float* vertices,
                      int64_t max_vertices, int32_t* triangles, int64_t max_triangles, void* record, void* workspace, size_t workspace_bytes,
                      size_t* workspace_needed, void* stream);
size_t afx_mesh_measures_workspace_bytes(void);
int afx_mesh_measures(const float* vertices, int64_t max_vertices, const int32_t* triangles, int64_t max_triangles, const void* record,
                      const double ref_point[3], double* out, void* workspace, size_t workspace_bytes, size_t* workspace_needed, void* stream);

/* ---- A triangle mesh back into a volume: the signed distance field of an indexed triangle mesh on a regular grid, and the unsigned
 * distance of arbitrary points to a mesh.  Defined here operation by operation, so that every implementation gives the same distance and
 * the same nearest triangle.  The rules above hold: device pointers, nothing allocated or synchronised, no floating-point atomics (the
 * record's 64-bit counters are integer atomics), hipGraph-capturable, the same bits on every run.
 *
 * Inputs: vertices fp32 [V][3] in world coordinates, triangles int32 [T][3].  Every coordinate is widened to fp64 first; all that follows
 * is fp64, every operation rounded on its own (no contraction), dot(u, v) = (u0 v0 + u1 v1) + u2 v2, cross(u, v) = (u1 v2 - u2 v1,
 * u2 v0 - u0 v2, u0 v1 - u1 v0).  Grid point (i0, i1, i2) lies at p[r] = ((o[r] + m[r][0] i0) + m[r][1] i1) + m[r][2] i2, index_to_world =
 * { m[0][0], m[0][1], m[0][2], o[0], m[1][0], ... o[2] } as for afx_isosurface_3d, and is NOT rounded to fp32.  A triangle that names a
 * vertex outside 0..V-1, or a vertex with a non-finite coordinate (afx_isosurface_3d emits NaN vertices next to NaN voxels), is SKIPPED:
 * it takes part in nothing and is counted in the record.  Points (afx_mesh_point_distance) must be finite.
 *   Distance.  d2(p, triangle a b c) = the minimum of
 *     seg(p, a, b), seg(p, b, c), seg(p, c, a), with seg(p, a, b): e = b - a, w = p - a, den = dot(e, e), t = dot(w, e) / den when
 *       den > 0, else 0; t below 0 becomes 0, above 1 becomes 1; q = a + t e (per component), g = p - q; seg = dot(g, g);
 *     and, only when nn = dot(n, n) > 0 for n = cross(b - a, c - a) and the three edge functions dot(cross(b - a, p - a), n),
 *       dot(cross(c - b, p - b), n), dot(cross(a - c, p - c), n) are all > 0: the plane term (h h) / nn, h = dot(p - a, n).
 *     Nothing divides 0 by 0 on a triangle that degenerates to a line or a point (capped isosurface meshes contain such).
 *   d2(p) = the minimum over the triangles that are not skipped, nearest(p) = the smallest index that attains it, d = sqrt(d2).  Without
 *     such a triangle d = +inf and nearest = -1.  A minimum is exact: it does not depend on the order or on which other triangles were
 *     looked at, which is what the culling below rests on.
 *   Sign: the generalised winding number, robust on soups, degenerate triangles and meshes that leave the grid.  Per triangle, with
 *     A = a - p, B = b - p, C = c - p, lA = sqrt(dot(A, A)) (lB, lC alike): term = 2 atan2(dot(A, cross(B, C)), (((lA lB) lC +
 *     dot(A, B) lC) + dot(B, C) lA) + dot(C, A) lB); w(p) = (the terms added in triangle-index order, starting from 0) / (4 pi), 4 pi
 *     rounded to fp64.  p is inside when w(p) >= 0.5.  The value written is fp32: -d inside and +d outside, rounded from fp64; d = 0 gives
 *     +0.0.  (Negative inside is the reference's convention: rev_sigmoid(x, c1 = 2) is about 1 for negative x.)  The library's atan2 need
 *     not equal another one to the bit: only the comparison with 0.5 and winding_out depend on it.
 *
 * afx_mesh_sdf_3d: sdf_out fp32 [n0][n1][n2]; nearest_out int32 [n0][n1][n2] or NULL; winding_out fp64 [n0][n1][n2] or NULL (w at every
 * grid point).  flags: AFX_MESH_SDF_BRUTE switches the culling off (every point against every triangle: the comparator of the culled
 * path, which must give the same bits); AFX_MESH_SDF_CLOSED is the caller's promise that the mesh has no boundary (true for a capped
 * isosurface, record slot B = 0): w is then constant on any region the surface does not enter, so a brick no triangle comes near is
 * evaluated once, at its centre, and the value shared - on a closed mesh this cannot change a sign.  A request for winding_out forces
 * the per-point sum.  record, AFX_MESH_SDF_RECORD_SLOTS uint64 slots on the device:
 *   [0] valid triangles  [1] skipped triangles  [2] bricks classed as clear (0 without AFX_MESH_SDF_CLOSED)  [3] point-triangle pairs the
 *   distance pass evaluated (N T' without culling, T' = [0]: what the culling saved)  [4..7] zero
 * Launches: zero the record; prepare (one thread per triangle: valid or not, the nine coordinates as fp64, the bounding sphere about the
 * middle of its bounding box; skipped when T = 0); the grid kernel, one workgroup of 512 threads per brick of 8 x 8 x 8 neighbouring grid
 * points.  It finds the exact distance dc of the brick's centre to the mesh, then walks the triangles in tiles of AFX_MESH_SDF_TILE
 * through LDS: each thread tests one triangle's sphere against the ball of radius dc + 2 R about the centre (R = the farthest of the
 * brick's eight world-space corners; a triangle beyond it is farther from every point of the brick than the nearest one), padded by a
 * relative 1e-12 and 1e-12 of the coordinates' magnitude against the rounding of all those quantities; the survivors are compacted in
 * index order and every thread walks them, skipping a survivor whose sphere lies beyond the nearest distance the thread has found so far
 * (padded alike) and evaluating the exact distance of the others; [3] counts those evaluations.  T = 0 is valid: every distance +inf, every nearest -1.
 * AFX_E_INVALID: a null sdf_out, record or index_to_world; a count below 0 or above 2^31 - 1, or above 0 with a null array; an axis
 * outside 1..AFX_EDT3D_MAX_SIDE; a non-finite entry of index_to_world or det(m) (as for afx_isosurface_3d) 0 or not finite; unknown flag
 * bits.  Workspace (afx_mesh_sdf_3d_workspace_bytes(T); 0 for a refused count), each region rounded up to 256 bytes, T' = max(T, 1):
 * double [9][T'] and double [4][T']; AFX_E_WORKSPACE when smaller, with *workspace_needed (when not NULL) set.
 *
 * afx_mesh_point_distance: dist_out[i] (fp32, rounded from fp64) = d of point i of points fp32 [P][3], nearest_out int32 [P] or NULL; all
 * pairs, one launch, no workspace: P T is small where it is used (the vertices of one mesh against the triangles of another).  record:
 * the same slots, [2] = 0, [3] = P [0].  AFX_E_INVALID: a null record; a count below 0 or above 2^31 - 1; P > 0 with null points or
 * dist_out; V or T above 0 with a null array. */
#define AFX_MESH_SDF_RECORD_SLOTS 8
#define AFX_MESH_SDF_TILE 512
#define AFX_MESH_SDF_BRUTE 1u
#define AFX_MESH_SDF_CLOSED 2u
size_t afx_mesh_sdf_3d_workspace_bytes(int64_t n_triangles);
int afx_mesh_sdf_3d(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, int32_t n0, int32_t n1, int32_t n2,
                    const double index_to_world[12], uint32_t flags, float* sdf_out, int32_t* nearest_out, double* winding_out, void* record,
                    void* workspace, size_t workspace_bytes, size_t* workspace_needed, void* stream);
int afx_mesh_point_distance(const float* points, int64_t n_points, const float* vertices, int64_t n_vertices, const int32_t* triangles,
                            int64_t n_triangles, float* dist_out, int32_t* nearest_out, void* record, void* stream);

/* ---- The centreline read as a graph: junction nodes, branches in path order, lengths, radii along the branch, and spur pruning.
 * Defined here so that every implementation gives the same result.  The rules above hold: device pointers, nothing allocated or
 * synchronised, integer atomics only, hipGraph-capturable, the same bits on every run.
 *
 * Input: skel, a uint8 volume [n0][n1][n2] (row-major; non-zero = on) - ANY mask, not only afx_skeletonize_3d's output; beyond the grid
 * is off; every axis in 1..AFX_EDT3D_MAX_SIDE.  d2 (uint32 [n0][n1][n2], may be NULL for the graph): the squared EDT of the mask that was
 * thinned, as afx_distance_transform_edt_3d writes it.
 *   deg(v) = the on voxels among v's 26 neighbours.  J = the on voxels with deg >= 3, P = those with deg <= 2.
 *   Junction nodes = the 26-components of J, labelled 1..K_J; branches = the 26-components of P, labelled 1..B; both in the order of
 *     their smallest linear index (afx_label_components_3d at connectivity 3).  A P voxel has at most 2 on neighbours, so a branch is a
 *     simple path, a single voxel or a closed cycle.  An EXTREME is a P voxel with fewer than 2 P-neighbours; a cycle has none, and none
 *     of its voxels touches J.
 *   Path order: a path starts at its extreme with the smaller linear index; a cycle starts at its smallest linear index and steps first
 *     to that voxel's P-neighbour with the smaller linear index.  path_voxels = the linear indices of all P voxels, branch after branch
 *     in label order, each in path order; a branch's offset into it is the exclusive prefix sum of the branch sizes.
 *   Attachments: an extreme is attached to the junction node of each J voxel among its neighbours - at most one per extreme of a path of
 *     >= 2 voxels; a single-voxel branch has at most two: the J neighbour with the smaller linear index is its start side, the other its
 *     end side.  Free ends of a branch = (0 for a cycle, else 2) - attachments; over the volume they sum to (voxels with deg 1) +
 *     2 (voxels with deg 0).  A SPUR is a branch with exactly one free end and exactly one attachment.
 *   Steps: every step between consecutive path voxels, the closing step of a cycle and the link from an attached extreme to its J voxel
 *     has a direction class: with code(d) = (d0 + 1) * 9 + (d1 + 1) * 3 + (d2 + 1), c = code - 14 of whichever of +-offset has
 *     code > 13: 13 classes, c = 0 for (0,0,1) .. c = 12 for (1,1,1).  A branch carries the 13 integer counts n_c; its length is
 *     (((n_0 L_0) + n_1 L_1) + ...) + n_12 L_12 in fp64, every product and sum rounded on its own (no contraction), L = step_lengths[13]
 *     (host, fp64, finite and >= 0; NULL = unit voxels: 1, sqrt 2, sqrt 3 by the number of non-zero components; for a world-space
 *     length pass |A d_c| for the index_to_world matrix A).  The volume's total length is the same formula on the summed counts: no
 *     floating-point sum depends on an order the hardware chooses.
 *   Radii (only with d2): per branch the min and max d2 along the path, the path position of the first minimum, the sum of
 *     sqrt((double)d2) added one after another in path order starting from 0.0 (each sqrt and sum rounded on its own), and the d2 at the
 *     attached J voxel of each side (0 for a free side).
 *   Pruning: one round deletes, together, the voxels of every spur b with len(b) <= factor * sqrt((double)d2[u]) - len the branch's
 *     length with unit step lengths, u the J voxel it is attached to, the product and the comparison in fp64 as above.  J voxels are
 *     never deleted, so the 26-components, cavities and tunnels of the input stay.  The graph is rebuilt and rounds repeat until one
 *     deletes nothing (that round is counted).  The result is a subset of the input; pruning it again changes nothing.
 *
 * afx_centreline_graph: node_labels, branch_labels (int32 [n0][n1][n2]: 0, or the node / branch of the voxel) and path_voxels (int32
 * [n0 n1 n2]: the first record[2] entries are written) are required.  branches: max_branches rows of AFX_GRAPH_BRANCH_SLOTS 8-byte
 * slots (row b - 1 for branch b; may be NULL with max_branches 0).  What path_voxels holds from entry record[2] on, and the rows from
 * min(B, max_branches) on, is unspecified.  lo / hi = the low / high 32 bits of a slot:
 *   [0] lo voxels, hi offset into path_voxels   [1] lo flags: bit 0 cycle, bit 1 spur, bits 8..9 free ends, bits 16..17 attachments;
 *   hi the path position of the first d2 minimum   [2] lo the node of the start side, hi of the end side (0 = free)
 *   [3] lo min d2, hi max d2 along the path (0 without d2)   [4] lo d2 at the start side's J voxel, hi at the end side's (0 = free)
 *   [5..11] the step counts, n_2q in lo and n_2q+1 in hi of slot 5 + q (hi of slot 11 is 0)   [12] length, fp64
 *   [13] the sum of radii, fp64 (0.0 without d2)   [14] lo the path's first voxel, hi its last   [15] zero
 * record: AFX_GRAPH_RECORD_SLOTS uint64 slots on the device:
 *   [0] on voxels  [1] J voxels  [2] P voxels  [3] K_J  [4] B  [5] voxels with deg 0  [6] with deg 1  [7] free ends = [6] + 2 [5]
 *   [8] cycles  [9] spurs  [10] total length, fp64  [11] status: bit 1 (value 1) B exceeds max_branches: rows 1..max_branches are
 *   written, everything else is complete, the call returns AFX_OK  [12] the smallest d2 on any branch (AFX_EDT3D_NONE without d2 or
 *   without a P voxel)  [13..15] zero
 * Launches: reset; classify (degrees, the J and P byte masks, counts by one integer add per wave); afx_label_components_3d on J, then
 * on P with its sizes; terminals (per branch, by integer atomicMin, the smallest extreme, or for a cycle the smallest voxel); offsets
 * (the exclusive scan of the sizes: chunk sums, one workgroup over them, the entries); walk (one lane per branch takes exactly
 * sizes[b] steps of 26 neighbour loads each: path order, step counts, radii, attachments, the row); finish (the record).  No loop
 * depends on a value another thread writes.  Cost at the top of the shape range: besides the labelling's own, the walk of one very
 * long branch is sequential, roughly a microsecond per voxel - a vessel tree's branches are a few hundred voxels, but a single curve
 * that fills a 1024^3 volume (2^28 voxels and more) would take minutes in one lane.
 * AFX_E_INVALID (before any HIP call): a null skel, node_labels, branch_labels, path_voxels or record; an axis outside
 * 1..AFX_EDT3D_MAX_SIDE; max_branches below 0, above 2^31 - 1, or above 0 with a null table; a step length that is negative or not
 * finite.  Workspace (afx_centreline_graph_workspace_bytes; 0 for a refused shape), each region rounded up to 256 bytes, N = n0 n1 n2:
 * two uint8 [N] (the J and P masks), uint32 [N] (branch sizes), max(afx_label_components_3d_workspace_bytes, two uint32 [N]) (the
 * labelling's workspace, afterwards the branch starts and offsets), uint32 [ceil(N / 2048)], and three times 256 bytes (the two
 * labelling records, counters); AFX_E_WORKSPACE when smaller, with *workspace_needed (when not NULL) set.
 *
 * afx_prune_spurs: out (uint8, 1 / 0; may be skel) = skel after the rounds above; d2 is required.  record: AFX_PRUNE_RECORD_SLOTS uint64
 * slots on the device:
 *   [0] rounds run (the one that deleted nothing included)  [1] branches deleted  [2] voxels deleted  [3] converged: 1 once a round has
 *   deleted nothing  [4] voxels that remain  [5] on voxels of the input  [6] voxels the last round run deleted  [7] zero
 * Per round: the graph's launches on `out` (the walk also marks the spurs the rule takes), delete, advance (one lane rolls the record).
 * Once the record says converged, later rounds find the same graph, mark nothing and leave mask and record as they are.  sync_every
 * has afx_skeletonize_3d's meaning: 0 issues exactly max_rounds rounds and reads nothing back (capturable; look at record[3]);
 * sync_every > 0 copies record[3] to the host after every sync_every rounds and after the last, and returns at convergence, or after
 * max_rounds rounds with converged = 0 - still AFX_OK, afx_last_error() says that it stopped early.
 * AFX_E_INVALID (before any HIP call): a null skel, d2, out or record; a refused shape; a factor that is negative, NaN or infinite;
 * max_rounds < 1; sync_every < 0.  Workspace (afx_prune_spurs_workspace_bytes): the graph's, then three int32 [N] (node labels, branch
 * labels, path voxels), uint8 [N] (marks) and 256 bytes (the graph record); AFX_E_WORKSPACE when smaller, *workspace_needed set. */
#define AFX_GRAPH_RECORD_SLOTS 16
#define AFX_GRAPH_BRANCH_SLOTS 16
#define AFX_PRUNE_RECORD_SLOTS 8
size_t afx_centreline_graph_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int afx_centreline_graph(const uint8_t* skel, const uint32_t* d2 /* may be NULL */, int32_t n0, int32_t n1, int32_t n2,
                         const double* step_lengths /* [13] on the host, may be NULL */, int32_t* node_labels, int32_t* branch_labels,
                         int32_t* path_voxels, void* branches, int64_t max_branches, void* record, void* workspace, size_t workspace_bytes,
                         size_t* workspace_needed, void* stream);
size_t afx_prune_spurs_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int afx_prune_spurs(const uint8_t* skel, const uint32_t* d2, int32_t n0, int32_t n1, int32_t n2, double factor, int32_t max_rounds,
                    int32_t sync_every, uint8_t* out, void* record, void* workspace, size_t workspace_bytes, size_t* workspace_needed,
                    void* stream);

/* ---- 3-D Frangi vesselness of a density volume (Frangi et al. 1998): is a bright voxel part of a tube, or of a blob or a plate?
 * Defined here so that every implementation gives the same result; tests/frangi3d_reference.py restates it in NumPy / SciPy.  The rules
 * above hold: device pointers, nothing allocated or synchronised, integer atomics only, hipGraph-capturable, the same bits on every run.
 * fp64 throughout, every expression evaluated operation by operation (no contraction).
 *
 * afx_frangi_3d: x is a volume [n0][n1][n2] (row-major; fp64 when x_is_f64 != 0, else fp32, converted to fp64 on load); sigma in voxels
 * (isotropic unit spacing).  For each sigma s in sigmas[n_sigmas] (1..16 values, each > 0 with int(4 s + 0.5) <= 1000), one after another:
 *   1. black_ridges != 0: x <- 1 - x.  (0 is the default of the Python layer: a density volume has BRIGHT vessels - the opposite of
 *      afx_frangi's projections.)
 *   2. G = scipy.ndimage.gaussian_filter(x, s): separable, axes 0, 1, 2 in that order, radius r = int(4 s + 0.5), weights
 *      exp(-j^2 / 2 s^2) normalised by NumPy's pairwise sum, mode 'reflect' (period 2n, also for r >= n); each pass sums x[i] w_0 first,
 *      then the pairs (x[i - j] + x[i + j]) w_j from j = r down to 1
 *   3. g_a = np.gradient(G, axis=a) and H_ab = (s * s) * np.gradient(g_a, axis=b) for a <= b (unit spacing, central differences inside,
 *      one-sided at the two ends of a line): six entries, each multiplied by the one product s * s
 *   4. the eigenvalues of H by 5 cyclic Jacobi sweeps over the pairs (p, q) = (0,1), (0,2), (1,2), r the third index.  A pair with
 *      a_pq == 0 is skipped; otherwise theta = (a_qq - a_pp) / (2 a_pq), t = (theta < 0 ? -1 : 1) / (|theta| + sqrt(theta theta + 1)),
 *      c = 1 / sqrt(t t + 1), s_ = t c, tau = s_ / (1 + c); a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, and from the old values
 *      a_rp' = a_rp - s_ (a_rq + tau a_rp), a_rq' = a_rq + s_ (a_rp - tau a_rq).  Only + - * / and sqrt: correctly rounded on the host and
 *      on the device alike.  (4 sweeps reach their floor, at most 6.6 eps ||H||_F from LAPACK's eigvalsh over 12 decades; the fifth is spare.)
 *   5. the diagonal ordered by |lambda| ascending, stable (a tie: the earlier diagonal position first): l1, l2, l3
 *   6. ra = (|l2| / d3)^2, d3 = |l3| (1e-10 where 0); rb = (|l1| / d23)^2, d23 = sqrt(|l2 l3|) (1e-10 where 0); S = l1 l1 + l2 l2 + l3 l3;
 *      v = (1 - exp(-ra / (2 alpha^2))) exp(-rb / (2 beta^2)) (1 - exp(-S / (2 gamma_s^2))); v = 0 where l2 > 0 or l3 > 0
 *      gamma <= 0: gamma_s = sqrt(max over the volume of S at this scale) / 2, or 1 where that is 0 (the density scale of a trained model is
 *      arbitrary: a fixed gamma means nothing on it); gamma > 0: that value at every scale
 *   7. out = max over the scales of v (a NaN propagates, as np.max); scale_index (uint8 [n0][n1][n2], may be NULL) = the first scale that
 *      attains it (np.argmax over the scale axis)
 * AFX_E_INVALID (before any HIP call): a null x, out or sigmas; a side < 2 (np.gradient needs two points); n0 n1 n2 >= 2^31; n_sigmas
 * outside 1..16; a bad sigma; alpha or beta not finite and > 0; gamma NaN or +inf.  Workspace (afx_frangi_3d_workspace_bytes; 0 for
 * arguments the call refuses), each region rounded up to 256 bytes, N = n0 n1 n2 - independent of n_sigmas: two fp64 [N] (the passes'
 * volumes), fp64 [3][N] (the eigenvalues of the current scale, which gamma_s needs complete before any v), 16 x 8 bytes (the bit patterns
 * of max S per scale: S >= 0, so an integer atomicMax on them is exact); AFX_E_WORKSPACE when smaller, with *workspace_needed (when not
 * NULL) set.  Launches: one memset, then per scale three Gaussian passes, eigen, vessel. */
size_t afx_frangi_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2, int32_t n_sigmas);
int afx_frangi_3d(const void* x, int32_t x_is_f64, int32_t n0, int32_t n1, int32_t n2, const double* sigmas, int32_t n_sigmas, double alpha,
                  double beta, double gamma /* <= 0: per-scale */, int32_t black_ridges, double* out, uint8_t* scale_index /* may be NULL */,
                  void* workspace, size_t workspace_bytes, size_t* workspace_needed, void* stream);

/* ---- Lumen cross-sections along a centreline: how wide is the vessel at each centreline point, below the voxel?  Defined here so that
 * every implementation gives the same result; tests/lumen_reference.py restates it in NumPy.  The rules above hold: device pointers,
 * nothing allocated or synchronised, no atomics, hipGraph-capturable, the same bits on every run.  fp64 throughout, only + - * / sqrt,
 * floor and comparisons, every product and sum rounded on its own (no contraction).
 *
 * afx_lumen_profile: vol is a volume [n0][n1][n2] (row-major; fp64 when vol_is_f64 != 0, else fp32, converted to fp64 on load), every
 * side >= 2, N = n0 n1 n2 < 2^31.  world_to_index W[3][4] (12 doubles on the host, rows W[a][0..2] and the offset W[a][3]).  points:
 * double [P][3], world coordinates, device.  seg_first, seg_last: int32 [P], device: the first and last point index of the polyline that
 * point k belongs to.  ray_cs: 2 R doubles on the host, cos(2 pi j / R) at [2 j] and sin(2 pi j / R) at [2 j + 1]; area_coef =
 * sin(2 pi / R) / 2; both reach the kernel in its arguments, no copy is issued.  R = n_rays in {8, 16, 32, 64}, h = half_window >= 1,
 * ds = step > 0 in world units, M = max_steps in 1..4096.  Per point k:
 *   1. Tangent.  a = max(k - h, seg_first[k]), b = min(k + h, seg_last[k]), both then clamped into [0, P - 1].  t = points[b] - points[a];
 *      n2 = (t0 t0 + t1 t1) + t2 t2.  b <= a or n2 == 0: flag NO_TANGENT.  Otherwise t <- t / sqrt(n2), component by component.  A cycle is
 *      an open path: no wrap-around.
 *   2. Frame.  e = the unit axis of the first component with the smallest |t_a|; u = t x e (each component two products and one
 *      subtraction: u0 = t1 e2 - t2 e1, u1 = t2 e0 - t0 e2, u2 = t0 e1 - t1 e0), normalised as in step 1; v = t x u.
 *   3. Directions.  d_j,a = (cs_j u_a) + (sn_j v_a).
 *   4. Lookup f(x).  q_a = ((W[a][0] x0 + W[a][1] x1) + W[a][2] x2) + W[a][3].  x is inside iff q_a >= 0 && q_a <= n_a - 1 on all three
 *      axes (a NaN or a huge q is outside); nothing is converted to an integer and nothing is loaded before the test passes.  Outside:
 *      0.0.  Inside: i_a = min(floor(q_a), n_a - 2), tau_a = q_a - i_a; the eight voxels i + {0, 1}^3 converted to fp64;
 *      lerp(p, q, tau) = p + (q - p) tau along axis 2 (four times), then axis 1 (twice), then axis 0.
 *   5. Centre.  f_0 = f(points[k]); !(f_0 >= iso): flag CENTRE_OUTSIDE.
 *   6. March, ray j: for m = 1..M, s_m = m ds (m as a double), x_a = c_a + s_m d_j,a, f_m = f(x).  The crossing is the first m with
 *      f_m < iso: r_j = ds ((m - 1) + (f_{m-1} - iso) / (f_{m-1} - f_m)), the divisor > 0 as f_{m-1} >= iso > f_m.  No crossing within M
 *      steps: r_j = M ds and the ray is OPEN.
 *   7. Reductions, the order part of the definition.  The pairwise tree s(0)_j = r_j r_{(j+1) mod R}, s(l+1)_j = s(l)_2j + s(l)_2j+1,
 *      area = area_coef s(log2 R)_0 - the area of the star-shaped polygon of the crossings about the point, which need not lie on the
 *      axis.  r_mean = the same tree over r_j, divided by R.  r_min, r_max over j.  d_min, d_max over j < R / 2 of r_j + r_{j + R/2}.
 *   8. Outputs.  profile: double [P][AFX_LUMEN_PROFILE_SLOTS] = (area, r_mean, r_min, r_max, d_min, d_max, f_0, 0).  flags: int32 [P]:
 *      bit 0 AFX_LUMEN_NO_TANGENT, bit 1 AFX_LUMEN_CENTRE_OUTSIDE, bits 8..15 the number of open rays.  radii: double [P][R], or NULL:
 *      not written.  With bit 0 or bit 1 set the row is zeros but for f_0 in slot 6, the radii are zeros and the open count is 0.
 * One launch: a lane per ray, 64 / R points per wavefront, 4 wavefronts per workgroup; the reductions are xor-butterflies over the lane
 * distances 1, 2, 4, .. < R (exactly the tree above in every lane).  No lane waits for another and the march count is fixed before
 * entry: the kernel ends on any input.  NaN voxels are out of scope.  There is no workspace: a wavefront owns its points.
 * AFX_E_INVALID, the message naming the argument, before any HIP call: a null vol, world_to_index or ray_cs; a side < 2 or N >= 2^31;
 * n_points < 0 or > 2^31 - 1; n_rays outside the set; half_window < 1; a non-finite iso, world_to_index, ray_cs or area_coef; step not
 * finite or not > 0; max_steps outside 1..4096; and, with n_points > 0, a null points, seg_first, seg_last, profile or flags.
 * n_points == 0 returns AFX_OK without a launch. */
#define AFX_LUMEN_PROFILE_SLOTS 8
#define AFX_LUMEN_NO_TANGENT 1
#define AFX_LUMEN_CENTRE_OUTSIDE 2
int afx_lumen_profile(const void* vol, int32_t vol_is_f64, int32_t n0, int32_t n1, int32_t n2, const double* world_to_index /* [12], host */,
                      const double* points, const int32_t* seg_first, const int32_t* seg_last, int64_t n_points, int32_t half_window,
                      int32_t n_rays, const double* ray_cs /* [2 n_rays], host */, double area_coef, double iso, double step,
                      int32_t max_steps, double* profile, int32_t* flags, double* radii /* may be NULL */, void* stream);

/* ---- The visual hull of the training views (space carving).  On vessel-only data a point whose projection misses the vessel silhouette
 * of some view is empty; the votes of all views over a lattice of points are two counts per point.  All arithmetic is fp64, every
 * operation rounded on its own (no contraction), only + - * / sqrt floor and comparisons: tests/hull_reference.py restates it in NumPy
 * and the device equals the restatement exactly.
 *   Lattice.  Point p = (i n1 + j) n2 + k, x_a = ((A[a][0] i + A[a][1] j) + A[a][2] k) + A[a][3], A = index_to_world (12 doubles, host:
 *      rows A[a][0..2], A[a][3]; i, j, k as doubles).  rho = radius >= 0, in world units: the ball about x the votes speak for (a grid
 *      cell: half its diagonal).
 *   Views.  views: double [n_views][AFX_HULL_VIEW_DOUBLES] on the device: R[r][n] at [3 r + n] (the rotation of the pose cam2world =
 *      [R | c]: camera looks down -z, y up), c at [9..11], the focal length f at [12], [13..15] unused.  width W, height H and the margin
 *      m = margin_px >= 0 (pixels) are common to all views.  dist: double [n_views][H][W], D_v = the distance from each pixel to the
 *      nearest mask pixel (0 on the mask) - the caller refuses a view with an empty mask.
 *   Per point and view, in this order:
 *      e = x - c;  q_n = (R[0][n] e0 + R[1][n] e1) + R[2][n] e2, n = 0, 1, 2;  d = -q_2.
 *      !(d - rho > 0): the view neither sees nor rejects the point; next view.
 *      u = W / 2 + (f q_0) / d;  w = H / 2 - (f q_1) / d      (the inverse of the ray model: pixel centres at the integers)
 *      l = sqrt(q_0 q_0 + q_1 q_1);  r = ((f rho) (d + l)) / (d (d - rho)) + m
 *      dx = max(max(0, -u), u - (W - 1));  dy = max(max(0, -w), w - (H - 1));  delta = sqrt(dx dx + dy dy)
 *      seen iff dx <= r && dy <= r
 *      iu = min(max(floor(u + 0.5), 0), W - 1);  iw = min(max(floor(w + 0.5), 0), H - 1)
 *      reject iff seen && D_v[iw][iu] > (r + sqrt(0.5)) + delta           (sqrt(0.5) rounded to fp64)
 *   Output.  seen, rejects: uint16 [n0 n1 n2], the counts over the views.  The hull is rejects <= max_rejects && seen >= min_seen.
 *   Guarantees (proofs in DESIGN 1.13; R orthonormal).  For |x' - x| <= rho the projection moves by at most
 *      f rho (d + l) / (d (d - rho)) pixels.  G1: if some point within rho of x projects within m of a mask pixel centre of view v,
 *      v does not reject x.  G2: if some point within rho of x projects within m of any pixel centre of v's detector, v sees x.
 * One launch, a lane per point, k fastest; the view records are read through wave-uniform addresses; no LDS, atomics, workspace or
 * synchronisation: the call can be captured in a graph.  AFX_E_INVALID before any launch, the message naming the argument: a null
 * pointer; n_views outside 1..65535; a non-positive extent, width or height; n0 n1 n2 >= 2^31; a non-finite index_to_world; radius or
 * margin_px negative or not finite; views, dist, seen or rejects not memory of the current device. */
#define AFX_HULL_VIEW_DOUBLES 16
int afx_visual_hull(int32_t n0, int32_t n1, int32_t n2, const double* index_to_world /* [12], host */, double radius,
                    const double* views /* device */, int32_t n_views, int32_t width, int32_t height, double margin_px, const double* dist,
                    uint16_t* seen, uint16_t* rejects, void* stream);

/* Carving an occupancy grid: where the byte mask[c] == 0, occs[c] = 0 (occs may be NULL) and binary[c] = 0; bits, the packed bitfield
 * the march reads, is rewritten from the result (bit b of word w = binary[32 w + b] != 0; the spare bits of the last word are 0).
 * In place, one launch, a lane per cell, no atomics, workspace or synchronisation: capturable.  AFX_E_INVALID: a null grid, mask,
 * binary or bits; a resolution outside 1..2048. */
int afx_grid_apply_mask(const afx_grid_desc* grid, const uint8_t* mask, float* occs, uint8_t* binary, uint32_t* bits, void* stream);

/* ---- Sparse-view algebraic reconstruction (SIRT): the line integrals of an fp64 attenuation volume along the rays of the training views
 * and the voxel-driven backprojection of their images.  All arithmetic is fp64, every operation rounded on its own (no contraction), only
 * + - * / sqrt floor and comparisons, in the order written: tests/sirt_reference.py restates both in NumPy and the device equals the
 * restatement exactly.
 *   Lattice.  Point p = (i n1 + j) n2 + k lies at x_a = ((A[a][0] i + A[a][1] j) + A[a][2] k) + A[a][3], A = index_to_world (12 doubles,
 *      host, as afx_visual_hull takes it); B = world_to_index (12 doubles, host), its inverse taken in fp64 by the caller (W = inv(A),
 *      offset -(W o), as for afx_lumen_profile) and handed to the library and the restatement alike.  n_a >= 2.
 *   Views.  views: double [n_views][AFX_HULL_VIEW_DOUBLES] on the device, the records of afx_visual_hull: R[r][n] at [3 r + n], c at
 *      [9..11], f at [12].  width W >= 2, height H >= 2, near, far and the sample count S are common to all views; pixel centres lie at
 *      the integers.  Images are double [n_views][H][W].
 *   afx_xray_project, per ray (v, iw, iu):
 *      a = (iu - W / 2) / f;  b = -((iw - H / 2) / f);  d_r = (R[r][0] a + R[r][1] b) - R[r][2];  L = sqrt((d_0 d_0 + d_1 d_1) + d_2 d_2)
 *      dt = (far - near) / S;  acc = +0;  for s = 0 .. S - 1 in order:
 *         t = near + (s + 0.5) dt;  x_r = c_r + t d_r;  g_a = ((B[a][0] x_0 + B[a][1] x_1) + B[a][2] x_2) + B[a][3]
 *         the sample is inside iff 0 <= g_a <= n_a - 1 for a = 0, 1, 2; outside it contributes +0 (so it may be skipped)
 *         inside: i_a = min(floor(g_a), n_a - 2), phi_a = g_a - i_a; the trilinear value of the 8 voxels i_a, i_a + 1 by lerps
 *         p + phi (q - p) along axis 2 (four), then axis 1 (two), then axis 0;  acc += value
 *      y = (acc dt) L.  out[v][iw][iu] = y, or, with target and weight given (both or neither), weight (target - y).
 *   afx_xray_backproject, per lattice point, over the views in order (acc = +0, cnt = 0):
 *      e = x - c;  q_n = (R[0][n] e_0 + R[1][n] e_1) + R[2][n] e_2;  d = -q_2;  !(d > 0): next view
 *      u = W / 2 + (f q_0) / d;  w = H / 2 - (f q_1) / d;  seen iff 0 <= u <= W - 1 && 0 <= w <= H - 1, else next view
 *      iu = min(floor(u), W - 2), phi_u = u - iu; iw, phi_w likewise;  top = I[iw][iu] + phi_u (I[iw][iu + 1] - I[iw][iu]), bot the same
 *      of row iw + 1;  acc += top + phi_w (bot - top);  cnt += 1
 *      Outputs, each optional (NULL), at least one: acc double [n0 n1 n2]; seen uint16 [n0 n1 n2] = cnt; x_inout double [n0 n1 n2],
 *      the fused SIRT update in place: upd = cnt > 0 ? acc / cnt : 0;  y = x + relax upd;  nonneg != 0: y = y > 0 ? y : 0;
 *      mask (uint8 [n0 n1 n2], may be NULL, only with x_inout) and mask[p] == 0: y = 0;  x[p] = y.
 * The backprojector is the voxel-driven gather, not the adjoint of the projector: every lane owns its voxel, so the sum over the views
 * has one order, needs no fp64 atomics and the update can be fused and captured.  One launch each (projector: a lane per ray, a
 * wavefront an 8 x 8 pixel tile; backprojector: a lane per point, k fastest); no LDS, atomics, workspace or synchronisation.
 * AFX_E_INVALID before any launch, the message naming the argument: a null pointer; n_views outside 1..65535; an extent below 2 or
 * n0 n1 n2 >= 2^31; width or height below 2; n_samples < 1; far <= near; a non-finite world_to_index, index_to_world, near, far or
 * relax; target without weight or the reverse; no output at all; a mask without x_inout; a pointer that is not memory of the current
 * device. */
int afx_xray_project(const double* volume, int32_t n0, int32_t n1, int32_t n2, const double* world_to_index /* [12], host */,
                     const double* views /* device */, int32_t n_views, int32_t width, int32_t height, double near, double far,
                     int32_t n_samples, const double* target /* may be NULL */, const double* weight /* may be NULL */, double* out,
                     void* stream);
int afx_xray_backproject(const double* images, const double* views /* device */, int32_t n_views, int32_t width, int32_t height, int32_t n0,
                         int32_t n1, int32_t n2, const double* index_to_world /* [12], host */, double* acc /* may be NULL */,
                         uint16_t* seen /* may be NULL */, double* x_inout /* may be NULL */, double relax, int32_t nonneg,
                         const uint8_t* mask /* may be NULL */, void* stream);

/* ---- Total-variation denoising of an fp64 volume: the proximal operator of the isotropic 3-D total variation (the Rudin-Osher-Fatemi
 * model: argmin_u 0.5 sum (u - x)^2 + weight TV(u)) by Chambolle's dual iteration.  All arithmetic is fp64, every operation rounded on
 * its own (no contraction), only + - * / sqrt and comparisons, in the order written: tests/tv_reference.py restates it in NumPy and the
 * device equals the restatement exactly.
 *   x: double [n0][n1][n2], k fastest, unit lattice spacing; voxel i = (i_0, i_1, i_2), e_a the unit step along axis a; n_a >= 1.
 *   c = tau / weight, taken once on the host.  Three dual fields p_0, p_1, p_2 of the volume's shape, all +0 at the start.
 *   Per iteration, every voxel from the OLD p only:
 *      div[i] = (b_0 + b_1) + b_2,  b_a = p_a[i] - (i_a > 0 ? p_a[i - e_a] : +0)
 *      u[i] = x[i] - div[i]
 *      g_a[i] = i_a < n_a - 1 ? u[i + e_a] - u[i] : +0
 *      m = sqrt((g_0 g_0 + g_1 g_1) + g_2 g_2)
 *      p_a[i] <- (p_a[i] - tau g_a) / (1 + c m)                 (so p_a stays +0 on the face i_a = n_a - 1)
 *   After `iterations` of these: out[i] = x[i] - div[i] (iterations = 0: out[i] = x[i], no arithmetic); nonneg != 0: out = out > 0 ?
 *   out : 0; then out = 0 where the byte mask (may be NULL) is 0.  out may be x.  A NaN or an infinity in x spreads to the neighbours,
 *   two steps per iteration, and nothing else happens; every loop is bounded by an argument.
 * One launch per iteration and one for out.  A workgroup owns a tile of AFX_TV_TILE_0 x AFX_TV_TILE_1 x AFX_TV_TILE_2 voxels, forms u on
 * the tile and one layer on the high side of each axis in LDS - the layer by the operations the neighbouring workgroup uses, so no bit
 * depends on the tile - and every lane writes the three new p of its voxel; p is ping-ponged between the two triples of the workspace
 * (6 volumes: afx_tv_denoise_3d_workspace_bytes, 0 for a shape the call refuses; not needed, and not looked at, with iterations = 0).
 * No atomics, reduction, synchronisation or read-back: the call can be captured in a graph.
 * AFX_E_INVALID before any launch, the message naming the argument: a null x or out; an extent below 1 or n0 n1 n2 >= 2^31; weight or
 * tau not finite or not positive; iterations < 0; with iterations > 0 a null or misaligned workspace or workspace_bytes too small; x,
 * out, mask or workspace not memory of the current device. */
#define AFX_TV_TILE_0 4
#define AFX_TV_TILE_1 8
#define AFX_TV_TILE_2 16
size_t afx_tv_denoise_3d_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int afx_tv_denoise_3d(const double* x, int32_t n0, int32_t n1, int32_t n2, double weight, double tau, int32_t iterations, int32_t nonneg,
                      const uint8_t* mask /* may be NULL */, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Optimal C-arm views: how much of each branch of a vessel tree a view foreshortens, and how much of it lies under another branch.
 * The tree is a list of capsules (the segments of the centreline polylines with the lumen radius); a view is a record of
 * afx_visual_hull.  All arithmetic is fp64, every operation rounded on its own (no contraction), only + - * / sqrt and comparisons, in
 * the order written; every comparison with a NaN is false.  tests/viewmap_reference.py restates it in NumPy and the device equals the
 * restatement exactly: the integer outputs are counts, and the two floating-point sums have one order.
 *   Inputs.  segments: double [N][AFX_VIEWMAP_SEGMENT_DOUBLES] on the device: p0 at [0..2], p1 at [3..5], the radius r >= 0 at [6], [7]
 *      unused.  seg_branch: int32 [N] on the device, the 1-based branch ids, non-decreasing (the segments of a branch are contiguous),
 *      seg_branch[N - 1] = B = n_branches, 1 <= B <= 65535 (an id that no segment carries is a branch with no segment: area 0, proj +0).
 *      views: double [V][AFX_HULL_VIEW_DOUBLES] on the device, 1 <= V <= 65535.  width W and height H in 1..16384, common to the views.
 *   Projection of a point p in view v (the hull's operations in the hull's order; pixel centres at the integers):
 *      e = p - c;  q_n = (R[0][n] e_0 + R[1][n] e_1) + R[2][n] e_2;  d = -q_2;  u = W / 2 + (f q_0) / d;  w = H / 2 - (f q_1) / d
 *   Visibility.  A segment is visible in v iff d0 > 0 && d1 > 0 (its two ends).  Its 2-D capsule: a = (u0, w0), b = (u1, w1),
 *      rho = (f r) / (0.5 (d0 + d1)).
 *   Coverage of pixel (iu, iw) by a visible segment:
 *      g = b - a;  g2 = g_x g_x + g_y g_y;  h = (iu, iw) - a;  t = g2 > 0 ? (h_x g_x + h_y g_y) / g2 : 0;  t < 0: t = 0;  t > 1: t = 1
 *      e = h - t g;  covered iff e_x e_x + e_y e_y <= rho rho
 *   Outputs per view, integers (given together or not at all):
 *      count  uint16 [V][H][W]   the number of distinct branches with at least one covering visible segment
 *      area   int32 [V][B]       the pixels branch b covers
 *      shared int32 [V][B]       those of them with count >= 2
 *      tree   int32 [V][AFX_VIEWMAP_TREE_SLOTS]   [UNION] the pixels with count >= 1, [MULTI] those with count >= 2, [INVISIBLE] the
 *             segments that are not visible; tree[0][BAD] != 0: seg_branch is not what is stated above (an id outside 1..B, a
 *             decreasing one, or a last one other than B - such segments cover nothing and the other numbers mean nothing); checked on
 *             the device by a launch of its own, the caller reads the flag with the results.
 *   Foreshortening (optional outputs; either, both or neither).  For segment s in view v:
 *      l = p1 - p0;  e = (p0 - c) + (p1 - c);  n2 = (e_0 e_0 + e_1 e_1) + e_2 e_2;  le = (l_0 e_0 + l_1 e_1) + l_2 e_2;
 *      l2 = (l_0 l_0 + l_1 l_1) + l_2 l_2;  perp2 = l2 - (le le) / n2;  perp = sqrt(perp2 > 0 ? perp2 : 0)
 *      proj double [V][B] = the sum of perp over the branch's segments in segment order, from +0;  length double [B] = the same sum of
 *      sqrt(l2).  perp is the segment's length seen at right angles to the ray through its midpoint: a segment that points at the
 *      source projects to 0.  Foreshortening of b in v = 1 - proj / length, overlap = shared / area: taken on the host.
 *   Known bias.  Branches that meet at a junction always share a few pixels around it; the amount is nearly the same in every view,
 *      so the ranking of views survives it.  Branch ends are not trimmed.
 * Launches: one that zeroes area, shared and tree (the caller zeroes nothing), the check of seg_branch, the raster (a workgroup a
 * 16 x 16 pixel tile of one view; segments culled per tile by their box padded by rho + 1 pixel; flag AFX_VIEWMAP_BRUTE
 * switches the cull off and the bytes stay the same) and the foreshortening (a lane per view and branch).  Integer atomicAdd only: the
 * result does not depend on any order.  Nothing is allocated or read back: the call can be captured in a graph.
 * AFX_E_INVALID before any launch, the message naming the argument: null segments, seg_branch or views; some but not all of count,
 * area, shared and tree; no output at all; n_views or n_branches outside 1..65535; n_segments outside 1..2^30; width or height outside
 * 1..16384; unknown flags; a pointer that is not memory of the current device. */
#define AFX_VIEWMAP_SEGMENT_DOUBLES 8
#define AFX_VIEWMAP_BRUTE 1u
#define AFX_VIEWMAP_TREE_SLOTS 4
#define AFX_VIEWMAP_TREE_UNION 0
#define AFX_VIEWMAP_TREE_MULTI 1
#define AFX_VIEWMAP_TREE_INVISIBLE 2
#define AFX_VIEWMAP_TREE_BAD 3
int afx_view_map(const double* segments, const int32_t* seg_branch, int32_t n_segments, int32_t n_branches, const double* views,
                 int32_t n_views, int32_t width, int32_t height, uint32_t flags, uint16_t* count, int32_t* area, int32_t* shared,
                 int32_t* tree, double* proj /* may be NULL */, double* length /* may be NULL */, void* stream);

/* ---- Curved-planar reformation: planes carried along a centreline, sampled out of a volume.  A plane is a centre and two in-plane unit
 * vectors (the rotation-minimising frame of the centreline point, made on the host); the in-plane positions of the samples are one table
 * shared by all planes, so the same call gives the stack of cross-sections (the straightened vessel: a K x K table) and the longitudinal
 * images (a table of lines through the centre at a few angles).  Defined here so that every implementation gives the same result;
 * tests/reformat_reference.py restates it in NumPy and the device equals the restatement exactly.  fp64 throughout, only + - * /, floor
 * and comparisons, every product and sum rounded on its own (no contraction).
 *
 * afx_reformat_planes: vol, vol_is_f64, n0, n1, n2 and world_to_index W as afx_lumen_profile takes them (every side >= 2, N < 2^31, W 12
 * doubles on the host).  planes: double [P][AFX_REFORMAT_PLANE_DOUBLES] on the device, the row = the centre c at [0..2], the in-plane
 * unit vector u at [3..5], the in-plane unit vector v at [6..8], world coordinates.  table: double [Q][AFX_REFORMAT_TABLE_DOUBLES] on
 * the device, the row = (a, b, sa, sb): the sample's in-plane offset along u and v, and the slab step in the same in-plane coordinates.
 * H = half_slab in 0..127, mode AFX_REFORMAT_MEAN or AFX_REFORMAT_MAX, fill a finite double.  Per (p, q), for m = -H .. H in that order:
 *   1. alpha = a + m sa;  beta = b + m sb                         (m as a double; the product, then the sum)
 *   2. x_r = (c_r + alpha u_r) + beta v_r,  r = 0, 1, 2
 *   3. f_m = the lookup of afx_lumen_profile step 4 at x: the same q_a, the same inside test (a NaN or a huge q is outside; nothing is
 *      converted to an integer and nothing is loaded before the test passes), the same i_a = min(floor(q_a), n_a - 2) and the same lerps
 *      along axis 2, 1, 0 - but outside the box it gives `fill`, not 0.  A NaN or infinite plane row is therefore outside: its row is fill.
 *   MEAN: acc = +0.0; acc = acc + f_m in order; out = acc / (2 H + 1)     (the divisor as a double; H = 0: (+0.0 + f_0) / 1.0)
 *   MAX:  out = f_{-H}; then out = f_m > out ? f_m : out                   (H = 0: f_0)
 * out: double [P][Q].  The result of a sample does not depend on where its row stands in the table: the caller may order the table so
 * that a wavefront (64 consecutive rows) covers a compact patch of the plane, and undo the order afterwards.
 * One launch: a lane per (p, q) under a 64-bit flat index p Q + q, q fastest, 4 wavefronts per workgroup; the slab loop is bounded by the
 * argument H and no lane waits for another: the kernel ends on any input.  No LDS, no atomics, no workspace, nothing allocated,
 * synchronised or read back: the call can be captured in a graph.  NaN voxels are out of scope.
 * AFX_E_INVALID, the message naming the argument, before any HIP call: a null vol or world_to_index; a side < 2 or N >= 2^31; n_planes
 * < 0 or > 2^31 - 1; n_table < 0 or > 2^20 (and n_planes n_table beyond the 2^22 x 65535 workgroups of a launch); half_slab outside 0..127; mode outside {0, 1}; a non-finite fill or world_to_index; and,
 * with n_planes > 0 and n_table > 0, a null planes, table or out.  n_planes == 0 or n_table == 0 returns AFX_OK without a launch. */
#define AFX_REFORMAT_PLANE_DOUBLES 9
#define AFX_REFORMAT_TABLE_DOUBLES 4
#define AFX_REFORMAT_MEAN 0
#define AFX_REFORMAT_MAX 1
int afx_reformat_planes(const void* vol, int32_t vol_is_f64, int32_t n0, int32_t n1, int32_t n2, const double* world_to_index /* [12], host */,
                        const double* planes, int64_t n_planes, const double* table, int64_t n_table, int32_t half_slab, int32_t mode,
                        double fill, double* out, void* stream);

/* ---- Registering C-arm poses to the vessel silhouettes: the 2D-3D chamfer cost of a point set (the centreline of the reconstructed
 * vessel, with radii) against one distance image per view, its Gauss-Newton normal equations in a rigid pose increment, a
 * Levenberg-Marquardt step and the selection of a coarse search.  All arithmetic is fp64, every operation rounded on its own (no
 * contraction), only + - * / sqrt floor and comparisons, in the order written; every comparison with a NaN is false; no floating-point
 * atomics: every sum has one order.  tests/pose_reference.py restates it in NumPy and the device equals the restatement exactly.
 *   View record.  The record of afx_visual_hull, AFX_HULL_VIEW_DOUBLES doubles: R[r][n] at [3 r + n], c at [9..11], f at [12].
 *   Field.  field: double [V][H][W] on the device, W, H >= 2, one distance image per VIEW (the Python layer builds the signed distance
 *      EDT(~mask) - EDT(mask): negative inside the silhouette; the kernel does not care what it holds).
 *   Points.  points: double [N][3], world coordinates; radius: double [N], world units (NULL: 0); weight: double [N] (NULL: 1).
 *   Pose increment.  xi = (a0, a1, a2, t0, t1, t2) acts in the camera frame, q' = C(a) q + t, with the Cayley rotation
 *      C(a) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a) (a rotation by theta about a / |a|, |a| = tan(theta / 2)).
 *      afx_pose_compose, record (R, c, f) and xi -> (R', c', f):  all six of xi == 0: the record is returned as it is.  Otherwise
 *        n = (a0 a0 + a1 a1) + a2 a2;  s = 1 - n;  den = 1 + n
 *        C[i][i] = (s + 2 (a_i a_i)) / den;  C[0][1] = (2 (a0 a1) - 2 a2) / den;  C[0][2] = (2 (a0 a2) + 2 a1) / den;
 *        C[1][0] = (2 (a0 a1) + 2 a2) / den;  C[1][2] = (2 (a1 a2) - 2 a0) / den;  C[2][0] = (2 (a0 a2) - 2 a1) / den;
 *        C[2][1] = (2 (a1 a2) + 2 a0) / den
 *        R'[i][j] = (R[i][0] C[j][0] + R[i][1] C[j][1]) + R[i][2] C[j][2]                  (R' = R C^T)
 *        c'_i = c_i - ((R'[i][0] t0 + R'[i][1] t1) + R'[i][2] t2)                        (c' = c - R' t);  [12..15] are copied
 *      records: double [n_records][16]; n_xi == 0: xi double [n_records][6], out[r] = compose(records[r], xi[r]); n_xi >= 1: xi double
 *      [n_xi][6], out[r n_xi + j] = compose(records[r], xi[j]) (every candidate of a search about every view).
 *   afx_pose_chamfer.  records: double [K][16]; rec_view: int32 [K], the view v whose image record k is scored against.  Residual of
 *   point i under record k:
 *        e = x - c;  q_n = (R[0][n] e_0 + R[1][n] e_1) + R[2][n] e_2;  d = -q_2                      (the hull's operations, its order)
 *        su = (f q_0) / d;  sw = (f q_1) / d;  u = W / 2 + su;  w = H / 2 - sw
 *        lost unless d > 0 && u >= 0 && u <= W - 1 && w >= 0 && w <= H - 1:  r = tau
 *        iu = min(floor(u), W - 2), pu = u - iu;  iw, pw likewise;  f00 = F[iw][iu], f01 = F[iw][iu + 1], f10 = F[iw + 1][iu], f11
 *        ga = f01 - f00;  gb = f11 - f10;  top = f00 + pu ga;  bot = f10 + pu gb;  g_w = bot - top;  val = top + pw g_w
 *        g_u = ga + pw (gb - ga);  err = val + (f r_i) / d
 *        err <= 0: satisfied, r = 0;  else err >= tau: saturated, r = tau;  else active, r = err  (tau = trunc, finite and > 0)
 *      Only an active point has a Jacobian row (the radius term's dependence on d is ignored):
 *        fd = f / d;  J_3 = g_u fd;  J_4 = -(g_w fd);  J_5 = (g_u su - g_w sw) / d             (d r / d q)
 *        J_0 = 2 (q_1 J_5 - q_2 J_4);  J_1 = 2 (q_2 J_3 - q_0 J_5);  J_2 = 2 (q_0 J_4 - q_1 J_3)      (d q' / d a = -2 [q]x at a = 0)
 *      Sums per record and slice, AFX_POSE_SUM_DOUBLES = 32 doubles, with wr = w_i r, wJ_k = w_i J_k:
 *        [0] sum (wr) r;  [1] sum wr;  [2] sum w_i (every point);  [3 + k] sum (wJ_k) r;  [9..29] sum (wJ_k) J_l, k <= l, the upper
 *        triangle row-major (active points only: the others are skipped, not multiplied by 0);  [30], [31] = 0.
 *        counts: int32 [4] = active, satisfied, saturated, lost.  AFX_POSE_COST_ONLY leaves [3..29] at 0.
 *      Order of the sums.  n_slices = S >= 1; slice s owns the points [s L, min(N, (s + 1) L)), L = ceil(N / S) rounded up to a multiple
 *        of 256.  Thread t of 256 adds its points s L + t, s L + t + 256, ... in ascending order into accumulators that start at +0.0;
 *        the 256 values meet in the adjacent-pair tree (level l + 1: s_j = s_2j + s_2j+1).  Output sums: double [K][S][32], counts:
 *        int32 [K][S][4]; the slices are NOT combined here (afx_pose_select and afx_pose_lm_step add them in slice order from +0.0).
 *      A record whose rec_view lies outside 0..V - 1 is dropped on the device: its counts are -1, sums[0] = +inf and the rest 0 in every
 *        slice (it is never selected and never accepted); the caller reads that flag with the results.
 *   afx_pose_select.  sums: double [V M][S][32], record v M + m = candidate m of view v.  cost_m = the slices' [0] added in order;
 *      selected[v] = the m of lowest cost, a later one only if strictly lower (ties, and NaN, to the lowest index).  records_out (may be
 *      NULL): double [V][16] = cand_records[v M + selected[v]].
 *   afx_pose_lm_step, a lane per view, on the caller-owned state: double [V][AFX_POSE_STATE_DOUBLES = 64]:
 *        [0..15] the current record; [16] its cost; [17..22] g; [23..43] H (upper triangle); [44] lambda; [45] accepted, [46] rejected,
 *        [47] singular (counts, as doubles); [48..63] the trial record.
 *      tot = the S slice sums of record v added in slice order from +0.0 (sums: double [V][S][32], record v = view v).
 *      AFX_POSE_LM_INIT: the row is zeroed; current = records_in[v]; cost, g, H = tot; lambda = lambda0.
 *      AFX_POSE_LM_UPDATE, AFX_POSE_LM_FINAL: tot is the trial's.  tot[0] < cost (strict): current = trial; cost, g, H = tot;
 *        lambda = max(lambda / 3, 1e-12); accepted += 1.  Otherwise lambda = min(4 lambda, 1e12); rejected += 1.
 *      INIT and UPDATE then solve (H + lambda diag H) delta = -g:  A = H made symmetric, b = -g; a k whose bit of dof_mask is 0 has its
 *        row and column zeroed, A_kk = 1, b_k = +0 (so delta_k = 0 exactly); otherwise A_kk = A_kk + lambda A_kk.  Cholesky, for j = 0..5:
 *        s = A_jj;  s = s - L_jp L_jp for p = 0..j-1 in order;  L_jj = sqrt(s);  for i > j: t = A_ij;  t = t - L_ip L_jp for p < j in
 *        order;  L_ij = t / L_jj.  Forward: t = b_i;  t = t - L_ip y_p, p < i in order;  y_i = t / L_ii.  Backward, i = 5..0: t = y_i;
 *        t = t - L_pi delta_p, p = i + 1..5 in order;  delta_i = t / L_ii.  If any pivot s is not > 0: delta = 0 and singular += 1.
 *        trial = compose(current, delta) (the operations of afx_pose_compose: with delta = 0 the trial is the current record).
 *      AFX_POSE_LM_FINAL solves nothing: trial = current (the last step of a run, whose trial nobody would score).
 *      trial_records: double [V][16] = the trial, the records of the next afx_pose_chamfer.
 *   Known ambiguities.  The residual is one-sided (a point inside the silhouette costs nothing), so a centreline thinner than the vessel
 *      leaves the pose free by the lumen's width; a translation along the view axis moves the projection only by its perspective and is
 *      barely observable at a C-arm's source distance.
 * k_pose_chamfer runs on a grid of (S, K) workgroups of 256 threads: the record through a wave-uniform address, 30 accumulators in
 * registers, the tree by wave shuffles and 4 x 30 doubles of LDS.  No atomics, nothing allocated, synchronised or read back, every loop
 * bounded by an argument: each call is one launch and can be captured in a graph.
 * AFX_E_INVALID before any launch, the message naming the argument: a null pointer (radius, weight, records_out and, outside INIT,
 * records_in may be NULL); n_views, n_records, n_candidates outside 1..65535; n_points outside 1..2^30; n_slices outside 1..4096; width
 * or height outside 2..16384; trunc or lambda0 not finite or not > 0; unknown flags; a phase other than the three; dof_mask above 63;
 * n_xi outside 0..65535; a pointer that is not memory of the current device. */
#define AFX_POSE_SUM_DOUBLES 32
#define AFX_POSE_STATE_DOUBLES 64
#define AFX_POSE_COST_ONLY 1u
#define AFX_POSE_LM_INIT 0
#define AFX_POSE_LM_UPDATE 1
#define AFX_POSE_LM_FINAL 2
#define AFX_POSE_ST_RECORD 0
#define AFX_POSE_ST_COST 16
#define AFX_POSE_ST_G 17
#define AFX_POSE_ST_H 23
#define AFX_POSE_ST_LAMBDA 44
#define AFX_POSE_ST_ACCEPTED 45
#define AFX_POSE_ST_REJECTED 46
#define AFX_POSE_ST_SINGULAR 47
#define AFX_POSE_ST_TRIAL 48
int afx_pose_chamfer(const double* field, int32_t n_views, int32_t width, int32_t height, const double* points,
                     const double* radius /* may be NULL */, const double* weight /* may be NULL */, int32_t n_points, const double* records,
                     const int32_t* rec_view, int32_t n_records, double trunc, int32_t n_slices, uint32_t flags, double* sums, int32_t* counts,
                     void* stream);
int afx_pose_compose(const double* records, int32_t n_records, const double* xi, int32_t n_xi, double* out, void* stream);
int afx_pose_select(const double* sums, int32_t n_views, int32_t n_candidates, int32_t n_slices, const double* cand_records,
                    int32_t* selected, double* records_out /* may be NULL */, void* stream);
int afx_pose_lm_step(double* state, int32_t n_views, const double* sums, int32_t n_slices, int32_t phase, uint32_t dof_mask, double lambda0,
                     const double* records_in /* AFX_POSE_LM_INIT only */, double* trial_records, void* stream);

/* ---- Territories: the exact 3-D feature transform (the nearest labelled voxel of any mask) and per-label overlap counts.  With the
 * voxels of a centreline graph as sites, every vessel voxel gets the branch it lies nearest to, and one counting call gives the
 * per-branch Dice, sensitivity, precision and coverage.  Integer arithmetic only; device pointers; nothing allocated, synchronised or
 * read back; every call is a fixed launch sequence and can be captured in a graph; the same bits on every run.
 * tests/territory_reference.py restates both in NumPy and the device equals the restatement exactly.
 *
 * afx_feature_transform_3d.  sites: uint8 [n0][n1][n2], row-major; a non-zero voxel is a site.  The linear index of voxel (i0, i1, i2)
 * is (i0 n1 + i1) n2 + i2.  For every voxel v = (v0, v1, v2) and every site s = (s0, s1, s2):
 *        dist2(v, s) = (v0 - s0)^2 + (v1 - s1)^2 + (v2 - s2)^2                                  (integers, below 2^22)
 *        d2[v]      = min over the sites s of dist2(v, s)
 *        nearest[v] = the LOWEST linear index among the sites s with dist2(v, s) == d2[v]
 *   i.e. the lexicographic minimum of the pair (dist2(v, s), index of s).  On a site, d2 = 0 and nearest[v] = v.  Without any site
 *   d2 = AFX_EDT3D_NONE and nearest = -1 everywhere.  d2 equals the d2 of afx_distance_transform_edt_3d of the inverted mask
 *   (fg = sites == 0) bit for bit.
 *   Three separable passes, each the lexicographic minimum of (value, carried site index), which reaches the rule above (the pair's
 *   minimum over a plane is the minimum over its lines of the lines' minima, a constant added to the first entry keeping the order):
 *     axis 2:  g2[v] = min over the sites s of v's own line (s0 = v0, s1 = v1) of ((v2 - s2)^2, index of s): a wave per line, ballots
 *              for the nearest site below and above; at an equal distance the lower side stays.
 *     axis 1:  g1[v] = min over c in 0..n1-1 of (g2[(v0, c, v2)].value + (v1 - c)^2, g2[(v0, c, v2)].site), lines without a site left out.
 *     axis 0:  (d2[v], nearest[v]) = min over c in 0..n0-1 of (g1[(c, v1, v2)].value + (v0 - c)^2, g1[(c, v1, v2)].site).
 *   The line passes pack the pair as value << 32 | site (value < 2^22, site < 2^30; all ones = no site) and compare 64-bit unsigned.  A
 *   workgroup takes a tile of 16 adjacent lines (lines of up to 512 voxels; 8 beyond) into 64 KiB of LDS and searches the lower
 *   envelope outwards from each voxel; the search stops once (v - c)^2 alone is GREATER than the best value (at equality a site
 *   straight along the axis still ties and may carry a lower index).  d2 and nearest are the passes' own storage: the axis-2 pass
 *   writes them, the line passes work in place (a workgroup reads its whole tile before it writes and no other workgroup touches that
 *   tile), so the call takes no scratch buffer.  No atomics.
 *   AFX_E_INVALID before any HIP call: a null sites, d2 or nearest; an axis outside 1..AFX_EDT3D_MAX_SIDE.
 *
 * afx_label_overlap_3d.  labels: int32 [n]; index: int32 [n] or NULL; d2: uint32 [n] or NULL; a: uint8 [n]; b: uint8 [n] or NULL;
 * counts: uint64 [n_labels + 1][4]; territory: int32 [n] or NULL.  For every v in 0..n-1:
 *        s = index ? index[v] : v
 *        l = 0                         if s < 0 or s >= n, or if d2 && d2[v] > max_d2      (a voxel exactly at max_d2 is inside)
 *        l = labels[s]                 otherwise; an l outside 1..n_labels becomes 0
 *        territory[v] = l              (when territory is given)
 *        counts[l][0] += 1;  counts[l][1] += (a[v] != 0);  counts[l][2] += (b && b[v] != 0);  counts[l][3] += (a[v] != 0 && b && b[v] != 0)
 *   Row 0 collects what belongs to no label.  counts is zeroed by the call's first launch, so the output is fully defined; n == 0
 *   leaves it all zero.  Integer atomics only, so the result does not depend on the order of execution: the lanes of a wave that hold
 *   the same label meet in ballots and add once to a per-workgroup table in LDS, which goes to global memory once per workgroup.
 *   With index = nearest and d2 of afx_feature_transform_3d and labels = the labels of the sites, l is the territory of v, cut off at
 *   the squared distance max_d2.
 *   AFX_E_INVALID before any HIP call: a null labels, a or counts; n < 0 or n > AFX_LABEL_OVERLAP_MAX_N; n_labels < 0 or
 *   n_labels > AFX_LABEL_OVERLAP_MAX_LABELS (the table of a workgroup fits in 64 KiB of LDS). */
#define AFX_LABEL_OVERLAP_MAX_LABELS 4095
#define AFX_LABEL_OVERLAP_MAX_N (1ll << 40)
int afx_feature_transform_3d(const uint8_t* sites, int32_t n0, int32_t n1, int32_t n2, uint32_t* d2, int32_t* nearest, void* stream);
int afx_label_overlap_3d(const int32_t* labels, const int32_t* index /* may be NULL */, const uint32_t* d2 /* may be NULL */,
                         uint32_t max_d2, const uint8_t* a, const uint8_t* b /* may be NULL */, int64_t n, int32_t n_labels,
                         uint64_t* counts /* [n_labels + 1][4] */, int32_t* territory /* [n], may be NULL */, void* stream);

/* Trainable fourier coefficients (model/CPPN.py:92 makes them an nn.Parameter; fourier_pos_enc, CPPN.py:320-327, is
 * differentiable in them).  After this call every backward entry point (afx_mlp_backward, afx_render_backward,
 * afx_train_step_mse) at a 16-bit precision also does d_enc_aux[3*n_freq] += d loss / d coefficients; `params` is the
 * fp32 flat parameter vector the prepared buffer was made from (W_0 is read from it).  d_enc_aux = NULL switches it
 * off (the default: the coefficients are constants).  AFX_PREC_F32 backward calls fail while it is on. */
int afx_set_encoding_grad(afx_ctx* ctx, const float* params, float* d_enc_aux);

/* Measurement aid (bench.py's roofline leg): when enabled, every launch of the three MFMA kernels is
 * bracketed by HIP events recorded on the launch stream.  afx_profile_read blocks on those events
 * (it synchronises), returns the summed device time and the launch
 * count for one kernel kind, and forgets them. */
enum { AFX_K_CHAIN_FWD = 0, AFX_K_CHAIN_BWD = 1, AFX_K_WGRAD = 2 };
int afx_profile_enable(afx_ctx* ctx, int on);
int afx_profile_read(afx_ctx* ctx, int which, double* ms_total, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* AFX_H */
