"""Fused renderer: ray generation -> sampling -> CPPN -> Beer-Lambert product in one kernel pass per ray
chunk, with autograd.  This is the path that replaces the body of the reference's training/eval
iteration (nerf/run_nerf_acc.py:287-296, :340-349)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from .engine import RenderSpec
from ._lib import AfxError


@dataclass
class RenderOutput:
    rgb_map: torch.Tensor                       # [R] transmittance = predicted pixel
    depth_map: Optional[torch.Tensor] = None    # only with want_aux (dense convention)
    weights: Optional[torch.Tensor] = None
    entropy: Optional[torch.Tensor] = None
    sigma: Optional[torch.Tensor] = None


# Optional hook set by nerf_for_angiography_amd.dist: called on the flat gradient before it is split.
_grad_hook = None


class _RenderFn(torch.autograd.Function):
    """pixel = render(rays) through afx_render_forward / afx_render_backward.  `origins` / `dirs` are the spec's ray arrays (None for
    rays made from poses): when they require grad, afx_render_backward_inputs also returns dL/d(origins, directions).  The backward is
    not itself differentiable (once_differentiable: create_graph=True raises on use)."""

    @staticmethod
    def forward(ctx, model, spec, want_st, origins, dirs, *params):
        prepared = model._prepared()
        pixel, sigma, tau = model.engine.render_forward(prepared, spec, model.precision, want_sigma=want_st,
                                                        want_tau=want_st)
        ctx.model, ctx.spec = model, spec
        ctx.save_for_backward(pixel)
        if want_st:
            ctx.mark_non_differentiable(sigma, tau)
            return pixel, sigma, tau
        return pixel

    @staticmethod
    @once_differentiable
    def backward(ctx, d_pixel, *unused):
        model, spec = ctx.model, ctx.spec
        (pixel,) = ctx.saved_tensors
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            return _RenderFn._backward_inputs(ctx, model, spec, pixel, d_pixel)
        flat_grad = torch.zeros(model.engine.param_count, dtype=torch.float32, device=pixel.device)
        coef_grad = model._coef_grad_buffer()
        with model.engine.encoding_grad(model.flat_params, coef_grad):
            model.engine.render_backward(model._prepared(), spec, pixel, d_pixel.contiguous(), flat_grad, model.precision)
        if _grad_hook is not None:
            _grad_hook(flat_grad)
            if coef_grad is not None:
                _grad_hook(coef_grad)
        return (None, None, None, None, None) + model._fn_grads(flat_grad, coef_grad)

    @staticmethod
    def _backward_inputs(ctx, model, spec, pixel, d_pixel):
        dev = pixel.device
        d_o = torch.empty(spec.n_rays, 3, dtype=torch.float32, device=dev) if ctx.needs_input_grad[3] else None
        d_d = torch.empty(spec.n_rays, 3, dtype=torch.float32, device=dev) if ctx.needs_input_grad[4] else None
        if not any(ctx.needs_input_grad[5:]):      # frozen model: no weight-gradient kernels
            model.engine.render_backward_inputs(model._prepared(), spec, pixel, d_pixel.contiguous(), None, d_o, d_d, model.precision)
            return (None, None, None, d_o, d_d) + (None,) * (len(ctx.needs_input_grad) - 5)
        flat_grad = torch.zeros(model.engine.param_count, dtype=torch.float32, device=dev)
        coef_grad = model._coef_grad_buffer()
        with model.engine.encoding_grad(model.flat_params, coef_grad):
            model.engine.render_backward_inputs(model._prepared(), spec, pixel, d_pixel.contiguous(), flat_grad, d_o, d_d, model.precision)
        if _grad_hook is not None:      # the parameter gradient only: ray gradients belong to this rank's rays
            _grad_hook(flat_grad)
            if coef_grad is not None:
                _grad_hook(coef_grad)
        return (None, None, None, d_o, d_d) + model._fn_grads(flat_grad, coef_grad)


def _check_model(model):
    if not getattr(model, "fused", False):
        if getattr(model, "fused_forward", False) and not torch.is_grad_enabled():
            pass      # tanh / sine models: forward kernels only (evaluation renders, density grids under torch.no_grad())
        else:
            raise NotImplementedError("render_rays: this CPPN configuration is outside the fused kernels (ReLU - or tanh / sine under "
                                      "torch.no_grad() -, no skip block, no view directions, one output channel)")
    if model.flat_params is None or not model.flat_params.is_cuda:
        raise AfxError("render_rays: the model must live on a GPU; there is no CPU fallback")


def render_spec(spec: RenderSpec, model, want_aux: bool = False) -> RenderOutput:
    _check_model(model)
    if not want_aux:
        return RenderOutput(_RenderFn.apply(model, spec, False, spec.origins, spec.dirs, *model._fn_params()))
    pixel, sigma, tau = _RenderFn.apply(model, spec, True, spec.origins, spec.dirs, *model._fn_params())
    out = RenderOutput(pixel, sigma=sigma)
    if spec.mode == "dense":
        # weights / depth_map / entropy of render_volume_density (nerf_helpers.py:107-119) from the
        # per-sample optical depths the kernel wrote; cheap per-ray scans, no MLP work.
        alpha = torch.exp(-tau)
        excl = torch.cat([torch.ones_like(alpha[:, :1]), torch.cumprod(alpha, -1)[:, :-1]], -1)
        out.weights = (1 - alpha + 1e-10) * excl
        z = spec.z if spec.z.dim() == 2 else spec.z[None, :]
        out.depth_map = (alpha * z).sum(-1)
        dens = sigma / (sigma.sum(-1, keepdim=True) + 1e-10)
        ent = -(dens * torch.log(dens + 1e-10)).sum(-1)
        out.entropy = ent * ((1 - pixel.detach()) > 0.4)
    return out


def render_rays(model, ray_origins, ray_directions, depth_samples_per_ray: int = 0, near_thresh: float = 0.0,
                far_thresh: float = 0.0, mode: str = "acc", z: Optional[torch.Tensor] = None,
                want_aux: bool = False) -> RenderOutput:
    """Pixels for rays given as origin/direction arrays (the output of sample_pixel_rays).

    mode='acc'  : depth_samples_per_ray uniform steps in [near, far], mid-point evaluation, dt = step —
                  acc_ray_marching without a grid + acc_render_volume_density (nerf_helpers_acc.py:10-63).
    mode='dense': explicit depths z [S] or [R,S]; render_volume_density convention (nerf_helpers.py:59-123)."""
    n_rays = ray_origins.shape[0]
    if mode == "dense":
        depth_samples_per_ray = z.shape[-1]
    spec = RenderSpec(n_rays=n_rays, n_samples=int(depth_samples_per_ray), origins=ray_origins, dirs=ray_directions,
                      mode=mode, t_near=float(near_thresh), t_far=float(far_thresh), z=z)
    return render_spec(spec, model, want_aux)


def render_projection(model, poses, width: int, height: int, focal: float, depth_samples_per_ray: int,
                      near_thresh: float, far_thresh: float, ray_ids: Optional[torch.Tensor] = None,
                      ray_id0: int = 0, n_rays: Optional[int] = None, mode: str = "acc",
                      z: Optional[torch.Tensor] = None, want_aux: bool = False) -> RenderOutput:
    """Pixels for rays generated in-kernel from C-arm poses (get_ray_values, phantomdata/helpers.py:156-175).
    poses: float64 [n_proj,4,4] or [n_proj,3,4] cam->world (source_matrix); rays are indexed into
    [n_proj, H, W] by `ray_ids` (int32) or enumerated from `ray_id0`."""
    poses = poses[:, :3, :].contiguous()
    if n_rays is None:
        n_rays = ray_ids.numel() if ray_ids is not None else poses.shape[0] * width * height - ray_id0
    if mode == "dense":
        depth_samples_per_ray = z.shape[-1]
    spec = RenderSpec(n_rays=int(n_rays), n_samples=int(depth_samples_per_ray), poses=poses, ray_ids=ray_ids,
                      ray_id0=int(ray_id0), width=int(width), height=int(height), focal=float(focal), mode=mode,
                      t_near=float(near_thresh), t_far=float(far_thresh), z=z)
    return render_spec(spec, model, want_aux)


def _as_f32(t, device):
    return t.to(device=device, dtype=torch.float32)


def _global_rays(n_local: int, n_global: Optional[int], device) -> int:
    """The ray count the loss is the mean over.  An explicit n_global wins; with a multi-rank SUM gradient hook installed
    (dist.GradSync) the ranks' counts are all-reduced, so that a default call is still the gradient of the GLOBAL mean; a
    local-mean hook (GradSync(local_mean=True)) keeps the local count; a foreign multi-rank hook must be told."""
    if n_global:
        return int(n_global)
    if _grad_hook is not None and getattr(_grad_hook, "world", 1) > 1:
        if getattr(_grad_hook, "local_mean", False):
            return int(n_local)
        if hasattr(_grad_hook, "global_count"):
            return _grad_hook.global_count(int(n_local), device)
        raise AfxError("train_step_mse: a multi-rank gradient hook is installed; pass n_global (rays of the step over all ranks)")
    return int(n_local)


def train_step_mse(model, spec: RenderSpec, target: torch.Tensor, n_global: Optional[int] = None):
    """One fused training pass: render `spec`, L = mean over the (global) batch of (pixel - target)^2, backward.

    Replaces `pred = render(...); loss = mse_loss(pred, target); loss.backward()` (nerf/run_nerf_acc.py:287-306):
    the gradients are ACCUMULATED into `.grad` of the model's Linear parameters exactly as loss.backward() would,
    so `optimizer.zero_grad(); train_step_mse(...); optimizer.step()` is the training iteration.  The forward pass
    is the backward kernel's own forward (f16 / bf16 operands), nothing is rendered twice.  Returns (loss, pixels), detached.
    n_global: total rays of the step across all ranks - the mean is over that count.  Default: this batch; with a
    multi-rank gradient hook installed (dist.GradSync, a SUM all-reduce) the ranks' ray counts are all-reduced instead, so
    the default call stays the gradient of the global mean."""
    _check_model(model)
    if model.precision == "f32":
        raise NotImplementedError("train_step_mse needs a 16-bit precision (f16, bf16, bf16x3); with 'f32' use render + autograd")
    n = _global_rays(spec.n_rays, n_global, model.flat_params.device)
    flat_grad = torch.zeros(model.engine.param_count, dtype=torch.float32, device=model.flat_params.device)
    coef_grad = model._coef_grad_buffer()
    with model.engine.encoding_grad(model.flat_params, coef_grad):
        if model.engine.fused_step_available(spec.n_samples, model.precision):
            # one kernel per ray chunk - or, for rays that straddle workgroup tiles (the reference's 300 samples/ray, the 128 + 64 of
            # the hierarchical pass) at the default precision, its two halves with the per-ray reduction between them: no recompute
            pixel = model.engine.train_step_mse(model._prepared(), spec, target, 1.0 / n, flat_grad, model.precision)
        else:
            # such rays at the other precisions / with an input encoding: forward launch, then the backward kernel (which recomputes
            # the forward) with dL/dpixel = 2 (pixel - target) / n
            pixel, _, _ = model.engine.render_forward(model._prepared(), spec, model.precision)
            d_pixel = (pixel - _as_f32(target, pixel.device)) * (2.0 / n)
            model.engine.render_backward(model._prepared(), spec, pixel, d_pixel, flat_grad, model.precision)
    if _grad_hook is not None:
        _grad_hook(flat_grad)
        if coef_grad is not None:
            _grad_hook(coef_grad)
    for p, g in zip(model._fn_params(), model._fn_grads(flat_grad, coef_grad)):
        if p.grad is None:
            p.grad = g
        else:
            p.grad.add_(g)
    loss = torch.nn.functional.mse_loss(pixel, target) if n == spec.n_rays else ((pixel - target) ** 2).sum() / n
    return loss, pixel


def train_step_packed_mse(model, ray_origins, ray_directions, packed, target: torch.Tensor, n_global: Optional[int] = None):
    """The reference's iteration body behind the occupancy-grid march - positions, get_predictions, acc_render_volume_density,
    mse_loss, backward (nerf/run_nerf_acc.py:289-306) - as ONE fused pass over the march's packed samples (engine.PackedGroups, from
    `occupancy.ray_marching(..., return_packed=True)` or `engine.pack_groups`): forward half, per-ray transmittance product, backward
    half, weight gradients; the MLP is evaluated once (the operator sequence evaluates it in the forward and again inside backward).
    f16s8 precision (with or without an input encoding).  Gradients are ACCUMULATED into `.grad` as loss.backward() would.  Returns (loss, pixels[n_rays]);
    a ray without samples renders 1 (the empty product)."""
    _check_model(model)
    if model.precision != "f16s8":
        raise NotImplementedError("train_step_packed_mse: precision 'f16s8' (other precisions: the operator sequence "
                                  "get_predictions -> acc_render_volume_density -> mse_loss -> backward)")
    n = _global_rays(packed.n_rays, n_global, model.flat_params.device)
    flat_grad = torch.zeros(model.engine.param_count, dtype=torch.float32, device=model.flat_params.device)
    coef_grad = model._coef_grad_buffer()
    with model.engine.encoding_grad(model.flat_params, coef_grad):
        pixel = model.engine.train_step_packed_mse(model._prepared(), ray_origins, ray_directions, packed, target, 1.0 / n, flat_grad, model.precision)
    if _grad_hook is not None:
        _grad_hook(flat_grad)
        if coef_grad is not None:
            _grad_hook(coef_grad)
    for p, g in zip(model._fn_params(), model._fn_grads(flat_grad, coef_grad)):
        if p.grad is None:
            p.grad = g
        else:
            p.grad.add_(g)
    loss = torch.nn.functional.mse_loss(pixel, target) if n == packed.n_rays else ((pixel - target) ** 2).sum() / n      # (one launch, not four)
    return loss, pixel


def march_train_step_mse(model, grid, scene_aabb, ray_origins, ray_directions, depth_samples_per_ray: int, near_thresh: float, far_thresh: float,
                         early_stop_eps: float, alpha_thre: float, target: torch.Tensor, n_global: Optional[int] = None, single_eval: bool = False):
    """The reference's whole grid iteration - acc_ray_marching (march through the occupancy grid, alpha_fn pass, render_visibility) followed by the
    body (positions, get_predictions, acc_render_volume_density, mse_loss, backward; nerf/run_nerf_acc.py:284-306) - as ONE library call
    (afx_march_train_step_mse): what `nerf_helpers_acc.acc_ray_marching(..., return_packed=True)` + `train_step_packed_mse` do, entry point for
    entry point and bit for bit, without a Python round trip per launch.  `grid`: nerf.occupancy.OccupancyGrid or None.  f16s8.
    Gradients are ACCUMULATED into `.grad`.  Returns (loss, pixels[n_rays], n_kept) - (None, None, 0) when no sample survived the march (the
    reference then skips the optimizer step, :293).
    `single_eval=True`: afx_march_train_step_mse_single_eval - ONE evaluation of the model (the training step's forward half over the
    candidates doubles as the alpha pass); same pixels and loss where the two forward kernels agree (afx.h), ReLU, no input encoding.  The
    counters are read back once, for the return value."""
    if single_eval and model.use_pos_enc != "none":
        raise NotImplementedError("march_train_step_mse(single_eval=True): no input encoding (pos_enc 'none')")
    _check_model(model)
    if model.precision != "f16s8":
        raise NotImplementedError("march_train_step_mse: precision 'f16s8' (other precisions: acc_ray_marching + the operator sequence)")
    from .nerf.occupancy import _aabb_on_host
    n_rays = ray_origins.shape[0]
    n = _global_rays(n_rays, n_global, model.flat_params.device)
    flat_grad = torch.zeros(model.engine.param_count, dtype=torch.float32, device=model.flat_params.device)
    coef_grad = model._coef_grad_buffer()
    step = (float(far_thresh) - float(near_thresh)) / int(depth_samples_per_ray)
    grid_kw = dict(grid_bits=None if grid is None else grid.bits, grid_aabb=None if grid is None else grid._aabb_host,
                   grid_res=None if grid is None else grid._res_host)
    aabb = None if scene_aabb is None else _aabb_on_host(scene_aabb)
    with model.engine.encoding_grad(model.flat_params, coef_grad):
        if single_eval:
            pixel, counts, _ = model.engine.march_train_step_mse_single_eval(
                model._prepared(), ray_origins, ray_directions, target, 1.0 / n, flat_grad, model.precision, aabb, near_thresh, far_thresh,
                step, early_stop_eps, alpha_thre, **grid_kw)
            model.engine.last_single_eval_counts = tuple(int(x) for x in counts.tolist())      # (candidates, kept, kept groups)
            n_kept = model.engine.last_single_eval_counts[1]
        else:
            pixel, _, n_kept = model.engine.march_train_step_mse(
                model._prepared(), ray_origins, ray_directions, target, 1.0 / n, flat_grad, model.precision, aabb, near_thresh, far_thresh,
                step, early_stop_eps, alpha_thre, **grid_kw)
    if n_kept == 0:
        return None, None, 0
    if _grad_hook is not None:
        _grad_hook(flat_grad)
        if coef_grad is not None:
            _grad_hook(coef_grad)
    for p, g in zip(model._fn_params(), model._fn_grads(flat_grad, coef_grad)):
        if p.grad is None:
            p.grad = g
        else:
            p.grad.add_(g)
    loss = torch.nn.functional.mse_loss(pixel, target) if n == n_rays else ((pixel - target) ** 2).sum() / n
    return loss, pixel, n_kept


def _check_forward_only(model, who: str):
    """march_render / march_render_projection evaluate the model without recording a graph: refuse where autograd would record one."""
    if torch.is_grad_enabled() and any(p.requires_grad for p in model.parameters()):
        raise RuntimeError(f"{who} is forward only (one evaluation of the model, no autograd graph): call it under torch.no_grad(); "
                           "to train through the grid use render.march_train_step_mse")
    if not getattr(model, "fused_forward", False):
        raise NotImplementedError(f"{who}: this CPPN configuration is outside the fused kernels (ReLU, tanh or sine without an encoding, no "
                                  "skip block, no view directions, one output channel)")
    if model.flat_params is None or not model.flat_params.is_cuda:
        raise AfxError(f"{who}: the model must live on a GPU; there is no CPU fallback")


def _march_render(model, grid, scene_aabb, depth_samples_per_ray, near_thresh, far_thresh, early_stop_eps, alpha_thre, binary_thresh, **rays):
    from .nerf.occupancy import _aabb_on_host
    step = (float(far_thresh) - float(near_thresh)) / int(depth_samples_per_ray)
    pixel, binary, kept, n_candidates = model.engine.march_render(
        model._prepared(), model.precision, None if scene_aabb is None else _aabb_on_host(scene_aabb), near_thresh, far_thresh, step,
        early_stop_eps, alpha_thre, grid_bits=None if grid is None else grid.bits, grid_aabb=None if grid is None else grid._aabb_host,
        grid_res=None if grid is None else grid._res_host, binary_thresh=binary_thresh, **rays)
    model.engine.last_kept_counts = kept      # (per ray, for comparisons)
    counts = (int(n_candidates), int(kept.sum()))
    return (pixel, counts) if binary_thresh is None else (pixel, binary, counts)


def march_render(model, grid, scene_aabb, ray_origins, ray_directions, depth_samples_per_ray: int, near_thresh: float, far_thresh: float,
                 early_stop_eps: float = 1e-2, alpha_thre: float = 1e-3, binary_thresh: Optional[float] = None):
    """The reference's evaluation render through the occupancy grid - acc_ray_marching (march, alpha pass, render_visibility), get_predictions
    over the kept samples, acc_render_volume_density (nerf/run_nerf_acc.py:338-349; visualization/visualization.py:335-352) - with ONE
    evaluation of the model (afx_march_render): the raw output of the alpha pass is the one compositing uses, so the pixels equal the operator
    sequence's bit for bit.  Step (far - near) / depth_samples_per_ray; `grid`: nerf.occupancy.OccupancyGrid or None (every step a candidate).
    Forward only, at the model's precision.  Returns (pixels [R], (n_candidates, n_kept)), or with `binary_thresh` (pixels, binary pixels [R],
    (n_candidates, n_kept)): the binary image forces sigma to 0 where sigmoid(raw) < binary_thresh (visualization.py:349-352)."""
    _check_forward_only(model, "march_render")
    if not (ray_origins.is_cuda and ray_directions.is_cuda):
        raise AfxError("march_render: rays must live on a GPU; there is no CPU fallback")
    return _march_render(model, grid, scene_aabb, depth_samples_per_ray, near_thresh, far_thresh, early_stop_eps, alpha_thre, binary_thresh,
                         origins=ray_origins, dirs=ray_directions)


def march_render_projection(model, grid, scene_aabb, poses, width: int, height: int, focal: float, depth_samples_per_ray: int,
                            near_thresh: float, far_thresh: float, early_stop_eps: float = 1e-2, alpha_thre: float = 1e-3,
                            binary_thresh: Optional[float] = None, ray_id0: int = 0, n_rays: Optional[int] = None):
    """march_render for rays generated in-kernel from C-arm poses (float64 [n_proj,4,4] or [n_proj,3,4] cam->world), enumerated as
    render_projection enumerates them without ray_ids: ray r = ray_id0 + r of [n_proj, H, W] - the rays of the dense fused kernels, bit for bit."""
    _check_forward_only(model, "march_render_projection")
    if not poses.is_cuda:
        raise AfxError("march_render_projection: poses must live on a GPU; there is no CPU fallback")
    return _march_render(model, grid, scene_aabb, depth_samples_per_ray, near_thresh, far_thresh, early_stop_eps, alpha_thre, binary_thresh,
                         poses=poses, width=width, height=height, focal=focal, ray_id0=ray_id0, n_rays=n_rays)


def hierarchical_train_step_mse(model, ray_origins, ray_directions, depth_values, depth_samples_per_ray_fine: int,
                                target: torch.Tensor, u: Optional[torch.Tensor] = None, n_global: Optional[int] = None,
                                fine_model=None, reuse_coarse: bool = True):
    """One hierarchical (coarse + fine) training pass on the fused kernels - the training step `fine_sampling`
    (nerf/nerf_helpers.py:178-195) belongs to, for the one-channel absorption model and an MSE loss on the fine render:

      coarse pass, no gradient (the reference detaches the samples, :186): ONE forward launch over the S coarse depths, which
        leaves the per-sample optical depths tau[R,S];
      afx_fine_depths_from_tau: weights = (1 - alpha + 1e-10) cumprod_exclusive(alpha) per ray, inverse-CDF sampling of
        `depth_samples_per_ray_fine` depths from weights[..., 1:-1] over the mid-point bins (sample_pdf, :197-222), merge with
        the coarse depths - nothing [R,S]-shaped is formed by torch operators in between;
      fine pass over the S + N_f per-ray depths with `fine_model or model`: train_step_mse (dense convention) - forward,
        compositing, MSE gradient and backward without recomputing the forward (128 + 64 = 192 samples straddle the 256-sample
        workgroup tiles: the split-phase step of afx_train_step_mse at the f16s8 precision).

    With ONE network (fine_model None, the reference's `fine_model or coarse_model`), f16s8 and no input encoding, the coarse depths are not evaluated
    twice (`reuse_coarse`, default on): the coarse pass IS the forward half of the training kernel over the coarse depths (stash, masks, sigma, tau), a
    second forward half evaluates only the N_f new depths, a per-ray kernel composites the merged list and hands every sample its finished dL/draw, and the
    backward halves + weight gradients of both sets follow (afx_hier_train_step_mse) - a third less MLP work than coarse forward + fine step.

    Gradients are accumulated into `.grad` of the fine network as train_step_mse does.  Returns (loss, fine pixels, merged depths)."""
    _check_model(model)
    from . import engine as _engine
    n_rays = ray_origins.shape[0]
    z = depth_values
    if (reuse_coarse and fine_model is None and model.precision == "f16s8" and model.engine.enc == "none"
            and int(depth_samples_per_ray_fine) >= 2 and 3 <= int(z.shape[-1]) <= 512):
        if u is None:
            u = torch.rand(n_rays, int(depth_samples_per_ray_fine), device=model.flat_params.device)
        n = _global_rays(n_rays, n_global, model.flat_params.device)
        flat_grad = torch.zeros(model.engine.param_count, dtype=torch.float32, device=model.flat_params.device)
        spec_c = RenderSpec(n_rays=n_rays, n_samples=int(z.shape[-1]), origins=ray_origins, dirs=ray_directions, mode="dense", z=z)
        pixel, z_all = model.engine.hier_train_step_mse(model._prepared(), spec_c, int(depth_samples_per_ray_fine), u, target, 1.0 / n, flat_grad,
                                                        model.precision)
        if _grad_hook is not None:
            _grad_hook(flat_grad)
        for p, g in zip(model._fn_params(), model._fn_grads(flat_grad, None)):
            if p.grad is None:
                p.grad = g
            else:
                p.grad.add_(g)
        return ((pixel - target) ** 2).sum() / n, pixel, z_all
    with torch.no_grad():
        spec_c = RenderSpec(n_rays=n_rays, n_samples=int(z.shape[-1]), origins=ray_origins, dirs=ray_directions, mode="dense", z=z)
        _, _, tau = model.engine.render_forward(model._prepared(), spec_c, model.precision, want_tau=True)
        if u is None:
            u = torch.rand(n_rays, int(depth_samples_per_ray_fine), device=tau.device)
        z_all = _engine.fine_depths_from_tau(z, tau, u)
        del tau
    net = model if fine_model is None else fine_model
    spec_f = RenderSpec(n_rays=n_rays, n_samples=int(z_all.shape[-1]), origins=ray_origins, dirs=ray_directions, mode="dense", z=z_all)
    loss, pixel = train_step_mse(net, spec_f, target, n_global)
    return loss, pixel, z_all


def projection_spec(poses, width, height, focal, depth_samples_per_ray, near_thresh, far_thresh, ray_ids=None,
                    ray_id0=0, n_rays=None) -> RenderSpec:
    """RenderSpec for rays generated in-kernel from C-arm poses ('acc' convention)."""
    poses = poses[:, :3, :].contiguous()
    if n_rays is None:
        n_rays = ray_ids.numel() if ray_ids is not None else poses.shape[0] * width * height - ray_id0
    return RenderSpec(n_rays=int(n_rays), n_samples=int(depth_samples_per_ray), poses=poses, ray_ids=ray_ids,
                      ray_id0=int(ray_id0), width=int(width), height=int(height), focal=float(focal), mode="acc",
                      t_near=float(near_thresh), t_far=float(far_thresh))


GRID_PRECISION = "bf16x3"      # default arithmetic of density_grid: split bf16 - fp32-grade (the grid's 1e-4 bar) at 1/3 of the f16 rate


def grid_precision(model) -> str:
    """Arithmetic of a density-grid evaluation: the model's own precision when it is a strict one (f32, bf16x3), else split bf16."""
    if getattr(model, "_act_name", "relu") == "sine":
        return "f32"      # sin(w0 z) amplifies the first layer's operand rounding by w0: split bf16 measures 1e-3 at w0 = 15
    return model.precision if model.precision in ("f32", "bf16x3") else GRID_PRECISION


def density_grid(model, outside: float, n: int, precision: Optional[str] = None) -> torch.Tensor:
    """sigma on meshgrid(t,t,t), t = linspace(-outside, outside, n+1), numpy 'xy' indexing as upstream
    (visualization/visualization.py:100-102,209-229): grid[i,j,k] = sigma(t[j], t[i], t[k]).

    precision: arithmetic of the MLP evaluation.  Default: the model's precision if that is a strict one (f32, bf16x3),
    otherwise GRID_PRECISION (split bf16) whatever the model trains at: the reconstructed grid is held to 1e-4 relative L2 against the reference's fp32 path, which the training
    precisions miss (f16: ~1e-3 on sigmoid(raw), tests/test_gpu_round3.py) - pixels average that error over a ray, a
    grid cell does not.  201^3 points take ~25 ms in split bf16."""
    with torch.no_grad():
        _check_model(model)
    dev = model.flat_params.device
    t = torch.linspace(-outside, outside, n + 1, dtype=torch.float64, device=dev).float()
    gy, gx, gz = torch.meshgrid(t, t, t, indexing="ij")      # [i,j,k] -> (x=t[j], y=t[i], z=t[k])
    pts = torch.stack([gx, gy, gz], -1).reshape(-1, 3).contiguous()
    keep, model.precision = model.precision, (precision or grid_precision(model))
    try:
        with torch.no_grad():
            sig = model.engine.infer(model._prepared(), pts, model.precision, apply_sigmoid=True)
    finally:
        model.precision = keep
    return sig.reshape(n + 1, n + 1, n + 1)


def _copy_state(who, live: dict, saved: dict):
    """load_state_dict of the graph classes: copy every saved tensor INTO the live one (the graphs replay against these addresses)."""
    if set(saved) != set(live):
        raise ValueError(f"{who}.load_state_dict: keys {sorted(saved)}, expected {sorted(live)}")
    with torch.no_grad():
        for k, t in live.items():
            v = torch.as_tensor(saved[k])
            if tuple(v.shape) != tuple(t.shape):
                raise ValueError(f"{who}.load_state_dict: {k} has shape {tuple(v.shape)}, expected {tuple(t.shape)}")
            t.copy_(v)


class GridTrainGraph:
    """The reference's grid training iteration (nerf/run_nerf_acc.py:284-306: march, alpha pass, render_visibility, graded pass, backward,
    optimizer step) captured ONCE into a HIP graph and replayed: weight re-tiling into the module's prepared buffer,
    afx_march_train_step_mse_capturable (sizes stay on the device), the loss, the gradients into `.grad`, `optimizer.step()`.

    `step(origins, dirs, target)` copies the batch into static tensors (device to device), replays, and returns device tensors
    (loss, pixel, counts) - counts = (candidates, kept samples, groups) - without reading anything back.  When nothing survives the march
    the optimizer step is skipped exactly as the reference skips it (:293): `optimizer.found_inf` points at the step's skip flag, which
    PyTorch's fused Adam honours (parameters, moments and `step` unchanged); pixel and loss then hold the previous replay's values.
    Requires `Adam(fused=True, capturable=True)` (a tensor lr can be changed between replays with `fill_`).  The occupancy grid is read
    by address: update it in place between replays (`OccupancyGrid.every_n_step`, `OccupancyGrid.refresh`, `GridUpdateGraph.step`, `set_binary`), never rebind it.  After a
    replay the module's cached prepared weights are marked stale, so eager renders re-tile the updated parameters.
    `single_eval=True` captures afx_march_train_step_mse_single_eval instead (one evaluation of the model per iteration; ReLU, no input
    encoding); everything else is the same."""

    def __init__(self, model, optimizer, grid, scene_aabb, n_rays: int, depth_samples_per_ray: int, near: float, far: float,
                 early_stop_eps: float, alpha_thre: float, n_global: Optional[int] = None, single_eval: bool = False):
        if _grad_hook is not None and getattr(_grad_hook, "world", 1) > 1:
            raise AfxError("GridTrainGraph: a multi-rank gradient hook (dist.GradSync) is installed; the all-reduce cannot be captured - "
                           "use march_train_step_mse")
        if not isinstance(optimizer, torch.optim.Adam) or not all(g.get("fused") and g.get("capturable") for g in optimizer.param_groups):
            raise ValueError("GridTrainGraph: needs torch.optim.Adam(..., fused=True, capturable=True) (the skip of an empty step is its found_inf)")
        _check_model(model)
        if model.precision != "f16s8":
            raise NotImplementedError("GridTrainGraph: precision 'f16s8' only")
        if model._coef_trainable():
            raise NotImplementedError("GridTrainGraph: trainable fourier coefficients are not captured; freeze them or use march_train_step_mse")
        if single_eval and model.use_pos_enc != "none":
            raise NotImplementedError("GridTrainGraph(single_eval=True): no input encoding (pos_enc 'none')")
        self.single_eval = bool(single_eval)
        from .nerf.occupancy import _aabb_on_host
        self.model, self.optimizer, self.grid = model, optimizer, grid
        dev = model.flat_params.device
        eng = model.engine
        self.n_rays = int(n_rays)
        n = _global_rays(self.n_rays, n_global, dev)
        inv_n = 1.0 / n
        self.origins = torch.zeros(self.n_rays, 3, device=dev)
        self.dirs = torch.zeros(self.n_rays, 3, device=dev)
        self.dirs[:, 2] = 1.0
        self.target = torch.zeros(self.n_rays, device=dev)
        self.pixel = torch.ones(self.n_rays, device=dev)
        self.counts = torch.zeros(3, dtype=torch.int64, device=dev)
        self.skip = torch.ones(1, device=dev)
        self.flat_grad = torch.zeros(eng.param_count, device=dev)
        for p, g in zip(model._hip_params(), model._split_grad(self.flat_grad)):
            p.grad = g      # the gradients live in the static buffer the captured step accumulates into
        self._aux_key = self._aux()
        self._buf = model._prepared()      # the module's prepared buffer: the graph re-tiles into it
        aabb = None if scene_aabb is None else _aabb_on_host(scene_aabb)
        step = (float(far) - float(near)) / int(depth_samples_per_ray)
        march = dict(scene_aabb=aabb, near_plane=float(near), far_plane=float(far), step=step, early_stop_eps=float(early_stop_eps),
                     alpha_thre=float(alpha_thre), grid_bits=None if grid is None else grid.bits,
                     grid_aabb=None if grid is None else grid._aabb_host, grid_res=None if grid is None else grid._res_host)

        def body(with_optimizer):
            eng.prepare(model.flat_params, model._enc_aux(), model.precision)      # into the cached buffer (key None: always re-tiles)
            self.flat_grad.zero_()
            fn = eng.march_train_step_mse_single_eval if self.single_eval else eng.march_train_step_mse_capturable
            fn(self._buf, self.origins, self.dirs, self.target, inv_n, self.flat_grad, model.precision, pixel=self.pixel, counts=self.counts,
               skip=self.skip, **march)
            loss = (torch.nn.functional.mse_loss(self.pixel, self.target) if n == self.n_rays
                    else ((self.pixel - self.target) ** 2).sum() / n)      # (as march_train_step_mse forms it)
            if with_optimizer:
                optimizer.step()
            return loss

        # eager warm-up of the library call (sizes the workspace, sets the kernels' attributes; grads are re-zeroed by every replay), and
        # the optimizer's state created by a step it skips (found_inf = 1): state created during the capture would be re-initialised by
        # every replay
        body(False)
        optimizer.found_inf = torch.ones((), device=dev)
        optimizer.step()
        self._found_inf = self.skip.view(())      # (fused Adam takes a 0-dim flag; a view of the step's skip flag)
        optimizer.found_inf = self._found_inf
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(self.graph, stream=side):
                self.loss = body(True)
        torch.cuda.current_stream(dev).wait_stream(side)
        self._mark_stale()

    def _aux(self):
        m = self.model
        return float(m.barf_alpha) if m.use_pos_enc == "barf" else None

    def _mark_stale(self):
        # replays update the parameters without a host-visible optimizer step: the cache keys would still match; a None key makes the next
        # eager model._prepared() re-tile into the same buffer (every precision's: evaluation renders and grid updates may use another)
        cache = self.model.engine._prepared
        for prec, (buf, _) in list(cache.items()):
            cache[prec] = (buf, None)
        cache[self.model.precision] = (self._buf, None)

    def _state(self):
        return dict(counts=self.counts, pixel=self.pixel, skip=self.skip)

    def state_dict(self):
        """The step's device-resident outputs that outlive a replay: counts, and pixel / skip (an empty march keeps the previous replay's)."""
        return {k: t.detach().clone() for k, t in self._state().items()}

    def load_state_dict(self, state):
        """Copied into the static buffers, after the capture: the graph keeps replaying against the same addresses."""
        _copy_state("GridTrainGraph", self._state(), state)

    def step(self, origins, dirs, target):
        if self._aux() != self._aux_key:
            raise AfxError("GridTrainGraph: the BARF schedule moved since the capture (the encoding weights are captured by address); "
                           "build a new GridTrainGraph")
        if self.optimizer.found_inf is not self._found_inf:
            raise AfxError("GridTrainGraph: optimizer.found_inf was replaced; the captured step reads the skip flag by address")
        self.origins.copy_(origins)
        self.dirs.copy_(dirs)
        self.target.copy_(target)
        self.graph.replay()
        self._mark_stale()
        return self.loss, self.pixel, self.counts


class GridUpdateGraph:
    """The occupancy-grid refresh of the reference's grid iteration (nerf/run_nerf_acc.py:285-286: acc_update_n_step for each grid, every n-th
    step) replayed from HIP graphs: re-tiling of the current parameters into the module's prepared buffer, then one afx_grid_refresh per grid
    (`OccupancyGrid.refresh`: cells drawn on the device, sigmoid(MLP), decay / EMA, threshold), captured on one stream.  Two graphs, captured
    lazily on first use: the warm-up one (every cell) and the post-warm-up one (the device draw).  The training step is a device counter that
    `step(n_iter)` fills before the replay, so replays follow it; nothing is read back.

    `grids`: [(grid, occ_thre), ...].  `step(n_iter)` does nothing unless n_iter % n == 0.  After a replay the module's cached prepared weights
    are marked stale (as GridTrainGraph does).  The grids' buffers are used by address: update them in place, never rebind them."""

    def __init__(self, model, grids, warmup_steps: int = 256, n: int = 16, ema_decay: float = 0.95):
        _check_model(model)
        if model._coef_trainable():
            raise NotImplementedError("GridUpdateGraph: trainable fourier coefficients are not captured; freeze them")
        self.model, self.grids = model, [(g, float(t)) for g, t in grids]
        self.warmup_steps, self.n, self.ema_decay = int(warmup_steps), int(n), float(ema_decay)
        self._aux_key = self._aux()
        dev = model.flat_params.device
        self.step_dev = torch.zeros((), dtype=torch.int64, device=dev)
        self._graphs = {}      # all_cells -> CUDAGraph

    def _aux(self):
        m = self.model
        return float(m.barf_alpha) if m.use_pos_enc == "barf" else None

    def _capture(self, all_cells):
        model, eng = self.model, self.model.engine
        dev = model.flat_params.device
        self._buf = model._prepared()      # the module's prepared buffer (allocated now): the graph re-tiles into it
        for g, _ in self.grids:
            g.reserve_refresh_workspace()
        # kernel attributes of the chain launch are set on first use: set them outside the capture (the same kernel as afx_mlp_infer's)
        eng.infer(self._buf, torch.zeros(1, 3, device=dev), model.precision, apply_sigmoid=True)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                eng.prepare(model.flat_params, model._enc_aux(), model.precision)      # into the cached buffer (key None: always re-tiles)
                for g, thre in self.grids:
                    g._refresh(eng, self._buf, model.precision, self.step_dev, thre, self.ema_decay, all_cells)
        torch.cuda.current_stream(dev).wait_stream(side)
        self._graphs[all_cells] = graph
        return graph

    def _mark_stale(self):
        cache = self.model.engine._prepared
        for prec, (buf, _) in list(cache.items()):
            cache[prec] = (buf, None)

    def state_dict(self):
        """The device step counter (step() fills it before every replay; kept so that a restored object equals the saved one)."""
        return dict(step=self.step_dev.detach().clone())

    def load_state_dict(self, state):
        _copy_state("GridUpdateGraph", dict(step=self.step_dev), state)

    def step(self, n_iter: int):
        if n_iter % self.n:
            return
        if self._aux() != self._aux_key:
            raise AfxError("GridUpdateGraph: the BARF schedule moved since the capture (the encoding weights are captured by address); "
                           "build a new GridUpdateGraph")
        all_cells = n_iter < self.warmup_steps
        graph = self._graphs.get(all_cells)
        if graph is None:
            graph = self._capture(all_cells)
        self.step_dev.fill_(int(n_iter))
        graph.replay()
        self._mark_stale()


def lr_decay_table(lr0: float, decay_rate: float, decay_steps: float, n: int):
    """The training driver's learning-rate schedule as a float32 table: entry i = lr0 * decay_rate ** (i / decay_steps), evaluated in Python
    doubles and rounded to float32 - the value `lr.fill_(...)` leaves in a float32 device tensor after iteration i, bit for bit."""
    import numpy as np
    return np.array([lr0 * (decay_rate ** (i / decay_steps)) for i in range(int(n))], dtype=np.float32)


def grid_round_schedule(start: int, n: int, round_len: int = 16, warmup: int = 256):
    """What GridTrainRoundGraph.run(n) replays from iteration `start`, as a list - a pure function of its arguments:
      ("round", step, all_cells)    one graph launch: the refresh at `step` (a multiple of round_len), then iterations step .. step + round_len - 1
      ("refresh", step, all_cells)  the refresh alone, ahead of a tail iteration at a multiple of round_len
      ("tail", step)                one iteration without a refresh
    all_cells = step < warmup (the warm-up refresh evaluates every cell).  A whole round runs when the step is a multiple of round_len and
    at least round_len iterations remain; every multiple of round_len in [start, start + n) gets exactly one refresh."""
    start, n, round_len, warmup = int(start), int(n), int(round_len), int(warmup)
    if start < 0 or n < 0 or round_len < 1:
        raise ValueError("grid_round_schedule: need start >= 0, n >= 0, round_len >= 1")
    ops, s, end = [], start, start + n
    while s < end:
        if s % round_len == 0 and end - s >= round_len:
            ops.append(("round", s, s < warmup))
            s += round_len
            continue
        if s % round_len == 0:
            ops.append(("refresh", s, s < warmup))
        ops.append(("tail", s))
        s += 1
    return ops


class GridTrainRoundGraph:
    """Whole refresh periods of the grid training loop from ONE graph launch each: what the driver's loop does per iteration with
    RayBatchSampler.draw, GridUpdateGraph.step, GridTrainGraph.step and the learning-rate `fill_` - in that order, with the same kernels on the
    same inputs - captured with the batch draw (afx_sample_batches_dev: the Philox stream id is the device step counter) and the loop's
    bookkeeping (afx_train_round_advance) inside.  A round graph holds: re-tiling, the refresh of every grid at the counter's step, the draw of
    `round_len` batches, then round_len times [gather batch j into the static batch, re-tile, zero the gradient, the capturable (or
    single-evaluation) step, the loss, optimizer.step() with found_inf = the skip flag, afx_train_round_advance].  Two of them (the warm-up
    refresh evaluates every cell, the later ones draw their cells on the device) and a tail graph (one iteration, a draw of one, no refresh)
    are captured on first use over one set of static buffers, each on one stream.

    grids: [(grid, occ_thre), ...] - every one is refreshed, the first is marched.  ray_table: (origins [n,3], dirs [n,3], pixels [n],
    weights [n]) on the device.  lr_table: float32 schedule (lr_decay_table); after iteration i the optimizer's learning rate - one float32
    device tensor shared by every param group - is lr_table[min(i, len - 1)]; iteration start_iter runs at lr_table[start_iter - 1] (the tensor's
    own value when start_iter is 0).  Requires Adam(fused=True, capturable=True), f16s8, no trainable fourier coefficients, one rank.

    run(n) advances n iterations (grid_round_schedule); nothing is read back: the class keeps a host mirror of the counter (`iter`).  A tail
    iteration at a multiple of round_len gets its refresh from the same calls issued eagerly.  history() returns the device tensors the
    replays write: the last round_len iterations' loss, counts and skip flag (slot = iteration % round_len), last_loss (the loss of the last
    iteration that kept samples), n_marched (kept samples summed; the caller may zero_() it) and the counter.  The grids' buffers, the ray table
    and the learning-rate tensor are used by address: update them in place, never rebind them."""

    def __init__(self, model, optimizer, grids, ray_table, scene_aabb, n_rays: int, depth_samples_per_ray: int, near: float, far: float,
                 early_stop_eps: float, alpha_thre: float, seed: int = 0, lr_table=None, round_len: int = 16, single_eval: bool = False,
                 start_iter: int = 0, warmup_steps: int = 256, ema_decay: float = 0.95, last_loss: float = float("nan")):
        who = "GridTrainRoundGraph"
        if _grad_hook is not None and getattr(_grad_hook, "world", 1) > 1:
            raise AfxError(f"{who}: a multi-rank gradient hook (dist.GradSync) is installed; the all-reduce cannot be captured - "
                           "use march_train_step_mse")
        if not isinstance(optimizer, torch.optim.Adam) or not all(g.get("fused") and g.get("capturable") for g in optimizer.param_groups):
            raise ValueError(f"{who}: needs torch.optim.Adam(..., fused=True, capturable=True) (the skip of an empty step is its found_inf)")
        _check_model(model)
        if model.precision != "f16s8":
            raise NotImplementedError(f"{who}: precision 'f16s8' only")
        if model._coef_trainable():
            raise NotImplementedError(f"{who}: trainable fourier coefficients are not captured; freeze them or use march_train_step_mse")
        if single_eval and model.use_pos_enc != "none":
            raise NotImplementedError(f"{who}(single_eval=True): no input encoding (pos_enc 'none')")
        from . import engine as _engine
        from .nerf.occupancy import _aabb_on_host
        dev = model.flat_params.device
        lr = optimizer.param_groups[0]["lr"]
        if not torch.is_tensor(lr) or lr.device != dev or lr.dtype != torch.float32 or lr.numel() != 1 \
                or any(g["lr"] is not lr for g in optimizer.param_groups):
            raise ValueError(f"{who}: the optimizer's lr must be ONE float32 tensor on {dev} shared by every param group (the captured "
                             "bookkeeping writes the schedule into it)")
        if lr_table is None or len(lr_table) < 1:
            raise ValueError(f"{who}: lr_table (lr_decay_table) is required")
        if not grids:
            raise ValueError(f"{who}: at least one (grid, occ_thre)")
        if int(round_len) < 1 or int(start_iter) < 0 or int(start_iter) + 1 >= 1 << 32:
            raise ValueError(f"{who}: need round_len >= 1 and 0 <= start_iter < 2^32 - 1")
        self._engine = _engine
        self.single_eval = bool(single_eval)
        self.model, self.optimizer = model, optimizer
        self.grids = [(g, float(t)) for g, t in grids]
        self.grid = self.grids[0][0]
        self.round_len, self.warmup_steps, self.ema_decay, self.seed = int(round_len), int(warmup_steps), float(ema_decay), int(seed)
        eng = model.engine
        self.n_rays = int(n_rays)
        self._table = tuple(t.to(device=dev, dtype=torch.float32).contiguous() for t in ray_table)
        tab_o, tab_d, tab_p, tab_w = self._table
        n_tab = tab_o.shape[0]
        if tuple(tab_o.shape) != (n_tab, 3) or tuple(tab_d.shape) != (n_tab, 3) or tab_p.numel() != n_tab or tab_w.numel() != n_tab:
            raise ValueError(f"{who}: ray_table = (origins [n,3], dirs [n,3], pixels [n], weights [n])")
        if not 0 < self.n_rays <= n_tab:
            raise ValueError(f"{who}: need 0 < n_rays <= {n_tab} table rays")
        inv_n = 1.0 / self.n_rays
        L = self.round_len
        # the static buffers every graph is captured over
        self.origins = torch.zeros(self.n_rays, 3, device=dev)
        self.dirs = torch.zeros(self.n_rays, 3, device=dev)
        self.dirs[:, 2] = 1.0
        self.target = torch.zeros(self.n_rays, device=dev)
        self.pixel = torch.ones(self.n_rays, device=dev)
        self.counts = torch.zeros(3, dtype=torch.int64, device=dev)
        self.skip = torch.ones(1, device=dev)
        self.flat_grad = torch.zeros(eng.param_count, device=dev)
        for p, g in zip(model._hip_params(), model._split_grad(self.flat_grad)):
            p.grad = g      # the gradients live in the static buffer the captured step accumulates into
        self.iter = int(start_iter)      # the host's mirror of step_dev
        self.step_dev = torch.full((), self.iter, dtype=torch.int64, device=dev)
        self.lr, self.lr_table = lr, torch.as_tensor(lr_table, dtype=torch.float32).to(dev).contiguous()
        if self.iter > 0:
            lr.copy_(self.lr_table[min(self.iter, self.lr_table.numel()) - 1])
        self.idx = torch.zeros(L, self.n_rays, dtype=torch.int64, device=dev)
        self._sample_ws = torch.empty(max(_engine.sample_batches_workspace_bytes(n_tab, L), 1), dtype=torch.uint8, device=dev)
        self.loss_hist = torch.full((L,), float("nan"), device=dev)
        self.counts_hist = torch.zeros(L, 3, dtype=torch.int64, device=dev)
        self.skip_hist = torch.ones(L, device=dev)
        self.last_loss = torch.full((), float(last_loss), device=dev)
        self.n_marched = torch.zeros((), dtype=torch.int64, device=dev)
        self._aux_key = self._aux()
        self._buf = model._prepared()      # the module's prepared buffer: the graphs re-tile into it
        aabb = None if scene_aabb is None else _aabb_on_host(scene_aabb)
        step = (float(far) - float(near)) / int(depth_samples_per_ray)
        self._march = dict(scene_aabb=aabb, near_plane=float(near), far_plane=float(far), step=step, early_stop_eps=float(early_stop_eps),
                           alpha_thre=float(alpha_thre), grid_bits=self.grid.bits, grid_aabb=self.grid._aabb_host, grid_res=self.grid._res_host)
        self._inv_n = inv_n
        # eagerly, before any capture (as GridTrainGraph and GridUpdateGraph do): the refresh workspaces, the chain kernels' attributes, the
        # step's workspace (one call on the placeholder batch; every replay re-zeroes the gradient), and the optimizer's state, created by
        # a step it skips (found_inf = 1)
        for g, _ in self.grids:
            g.reserve_refresh_workspace()
        eng.infer(self._buf, torch.zeros(1, 3, device=dev), model.precision, apply_sigmoid=True)
        self._train_step()
        optimizer.found_inf = torch.ones((), device=dev)
        optimizer.step()
        self._found_inf = self.skip.view(())      # (fused Adam takes a 0-dim flag; a view of the step's skip flag)
        optimizer.found_inf = self._found_inf
        self._graphs = {}      # "warmup" | "round" | "tail" -> CUDAGraph
        self._mark_stale()

    def _aux(self):
        m = self.model
        return float(m.barf_alpha) if m.use_pos_enc == "barf" else None

    def _mark_stale(self):
        cache = self.model.engine._prepared
        for prec, (buf, _) in list(cache.items()):
            cache[prec] = (buf, None)
        cache[self.model.precision] = (self._buf, None)

    def _train_step(self):
        """Re-tiling, zeroed gradient, the step on the static batch, the loss (GridTrainGraph's body)."""
        model, eng = self.model, self.model.engine
        eng.prepare(model.flat_params, model._enc_aux(), model.precision)      # into the cached buffer (key None: always re-tiles)
        self.flat_grad.zero_()
        fn = eng.march_train_step_mse_single_eval if self.single_eval else eng.march_train_step_mse_capturable
        fn(self._buf, self.origins, self.dirs, self.target, self._inv_n, self.flat_grad, model.precision, pixel=self.pixel, counts=self.counts,
           skip=self.skip, **self._march)
        return torch.nn.functional.mse_loss(self.pixel, self.target)

    def _refresh(self, all_cells):
        """GridUpdateGraph's body: re-tiling, then every grid's refresh at the counter's step."""
        model, eng = self.model, self.model.engine
        eng.prepare(model.flat_params, model._enc_aux(), model.precision)
        for g, thre in self.grids:
            g._refresh(eng, self._buf, model.precision, self.step_dev, thre, self.ema_decay, all_cells)

    def _iterations(self, n):
        """The draw of n batches at the counter's step, then n iterations, each followed by the device bookkeeping."""
        E = self._engine
        tab_o, tab_d, tab_p, tab_w = self._table
        E.sample_batches_dev(tab_w, self.seed, self.step_dev, n, self.n_rays, out_idx=self.idx[:n], workspace=self._sample_ws)
        for j in range(n):
            E.gather_rays(tab_o, tab_d, tab_p, self.idx[j], self.origins, self.dirs, self.target)
            loss = self._train_step()
            self.optimizer.step()
            E.train_round_advance(self.step_dev, self.lr_table, self.lr, self.skip, loss, self.counts, self.loss_hist, self.counts_hist,
                                  self.skip_hist, self.last_loss, self.n_marched)

    def _graph(self, kind):
        graph = self._graphs.get(kind)
        if graph is not None:
            return graph
        dev = self.model.flat_params.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):      # one stream, no forked branches: a linear graph
            with torch.cuda.graph(graph, stream=side):
                if kind == "tail":
                    self._iterations(1)
                else:
                    self._refresh(kind == "warmup")
                    self._iterations(self.round_len)
        torch.cuda.current_stream(dev).wait_stream(side)
        self._graphs[kind] = graph
        return graph

    def run(self, n: int):
        """Advance n iterations from the current counter."""
        if self._aux() != self._aux_key:
            raise AfxError("GridTrainRoundGraph: the BARF schedule moved since the capture (the encoding weights are captured by address); "
                           "build a new GridTrainRoundGraph")
        if self.optimizer.found_inf is not self._found_inf:
            raise AfxError("GridTrainRoundGraph: optimizer.found_inf was replaced; the captured step reads the skip flag by address")
        if self.iter + int(n) >= 1 << 32:
            raise ValueError("GridTrainRoundGraph: the step counter stays below 2^32")
        for op in grid_round_schedule(self.iter, n, self.round_len, self.warmup_steps):
            if op[0] == "round":
                self._graph("warmup" if op[2] else "round").replay()
                self.iter += self.round_len
            elif op[0] == "refresh":
                with torch.no_grad():
                    self._refresh(op[2])
            else:
                self._graph("tail").replay()
                self.iter += 1
        if n > 0:
            self._mark_stale()

    def _state(self):
        return dict(step=self.step_dev, lr=self.lr, loss_hist=self.loss_hist, counts_hist=self.counts_hist, skip_hist=self.skip_hist,
                    last_loss=self.last_loss, n_marched=self.n_marched, counts=self.counts, pixel=self.pixel, skip=self.skip)

    def state_dict(self):
        """The device-resident state of the rounds: the step counter (the learning-rate table is indexed by it), the learning rate, the
        loss / counts / skip history, last_loss, n_marched and the step's own outputs.  Reads the device (call it between runs)."""
        return {k: t.detach().clone() for k, t in self._state().items()}

    def load_state_dict(self, state):
        """Copied into the static buffers - before or after the graphs are captured, they replay against the same addresses - and the
        host's mirror of the counter set from the restored one."""
        _copy_state("GridTrainRoundGraph", self._state(), state)
        self.iter = int(torch.as_tensor(state["step"]))

    def history(self):
        """The device tensors the replays write, without synchronising."""
        return dict(loss=self.loss_hist, counts=self.counts_hist, skip=self.skip_hist, last_loss=self.last_loss, n_marched=self.n_marched,
                    step=self.step_dev)
