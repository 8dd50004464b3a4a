"""Mirror of the reference's nerf/nerf_helpers.py call surface (names, argument order, return arity),
with the arithmetic routed to the HIP library for GPU tensors.  Citations are upstream file:line."""
import numpy as np
import torch

from .. import engine as _engine


def randomize_depth(z_vals, device):
    """Stratified jitter (nerf/nerf_helpers.py:13-22).  With the 1-D z the driver passes, one jitter vector
    is shared by the whole ray batch.  (In-kernel variant: RenderSpec mode 'stratified'.)"""
    from .._geometry import jitter_depths
    return jitter_depths(z_vals, torch.rand(z_vals.shape).to(device)).to(device)


def get_minibatches(inputs, chunksize=1024 * 8):
    return [inputs[i:i + chunksize] for i in range(0, inputs.shape[0], chunksize)]


def get_predictions(model, flattened_query_points, chunksize, target_img_idx=None):
    """nerf/nerf_helpers.py:31-45.  The reference chunks only to bound the activation memory of its unfused layers; the fused kernel
    materialises nothing but [P,1], so a fused model on the GPU takes all points in ONE launch (and one backward) whatever
    `chunksize` says - 13 launches and 13 backward passes less per iteration of the reference loop (1.7 M points, chunk 131 072).
    Other models / an image index: the reference's chunk loop."""
    if not target_img_idx and getattr(model, "fused", False) and flattened_query_points.is_cuda \
            and flattened_query_points.shape[0] < (1 << 31) - 256:
        return model(flattened_query_points)
    predictions = []
    for batch in get_minibatches(flattened_query_points, chunksize=chunksize):
        if target_img_idx:
            indices = torch.Tensor([target_img_idx]).repeat((batch.shape[0], 1)).to(model.device)
            predictions.append(model(torch.cat((batch, indices), dim=-1)))
        else:
            predictions.append(model(batch))
    return torch.cat(predictions, dim=0)


def cumprod_exclusive(tensor):
    """Exclusive running product along the last axis: out[..., i] = prod(tensor[..., :i]) (nerf_helpers.py:47-57)."""
    shifted = torch.nn.functional.pad(tensor[..., :-1], (1, 0), value=1.0)
    return torch.cumprod(shifted, dim=-1)


class _CompositeDenseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, dirs, z):
        rgb, depth, w, ent, sig = _engine.composite_dense(raw, dirs, z)
        ctx.save_for_backward(raw, dirs, z, rgb)
        ctx.mark_non_differentiable(depth, w, ent, sig)
        return rgb, depth, w, ent, sig

    @staticmethod
    def backward(ctx, d_rgb, *unused):
        raw, dirs, z, rgb = ctx.saved_tensors
        return _engine.composite_dense_backward(raw, dirs, z, rgb, d_rgb.contiguous()), None, None


def get_ray_entropy(sigmas, rgb_map, threshold=0.4):
    """Entropy of each ray's normalised density profile, kept only for rays that absorb more than `threshold`
    (nerf/nerf_helpers.py:125-135)."""
    p = sigmas / (sigmas.sum(dim=-1, keepdim=True) + 1e-10)
    entropy = -(p * torch.log(p + 1e-10)).sum(dim=-1)
    return entropy * ((1 - rgb_map) > threshold).detach()


class _DenseEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, rgb, threshold):
        ent, sums = _engine.ray_entropy_dense(raw, rgb, threshold)
        ctx.save_for_backward(raw, rgb, sums)
        ctx.threshold = threshold
        return ent

    @staticmethod
    def backward(ctx, d_ent):
        raw, rgb, sums = ctx.saved_tensors
        return _engine.ray_entropy_dense_backward(raw, rgb, sums, d_ent.contiguous(), ctx.threshold), None, None


def ray_entropy(raw, rgb_map, threshold=0.4):
    """The entropy render_volume_density forms (nerf/nerf_helpers.py:119, get_ray_entropy :125-135) from the model's one-channel output
    raw [R,S] or [R,S,1] (before the sigmoid) and the rays' rgb_map [R] -> entropy[R], differentiable on the GPU (afx_ray_entropy_dense;
    render_volume_density returns the same values detached).  The gradient flows to `raw` only; rgb_map only selects the rays."""
    if not raw.is_cuda:
        from .._lib import AfxError
        raise AfxError("ray_entropy: tensors must live on the GPU; there is no CPU fallback")
    if raw.dim() == 3:
        if raw.shape[-1] != 1:
            raise ValueError("ray_entropy: expected raw[R,S] or raw[R,S,1]")
        raw = raw[..., 0]
    return _DenseEntropyFn.apply(raw.float().contiguous(), rgb_map.detach().reshape(-1).float().contiguous(), float(threshold))


def _render_volume_density_ops(radiance_field, ray_directions, depth_values):
    """The two branches of nerf/nerf_helpers.py:59-123 the reference's training path never takes, on PyTorch-ROCm operators
    (same device; kept for capability, not accelerated):
      C == 2 (:67-83): emission-absorption - density relu(last channel), colour sigmoid(first), opacity 1 - exp(-sigma dz)
        with the PLAIN depth differences (no ||d||), weights = opacity * exclusive transmittance, entropy of the opacity
        profile averaged over the rays whose opacities add up to more than 0.7 (a scalar);
      C  > 2 (:86-87): density relu(mean over channels), then the one-channel absorption formulas (||d||-scaled steps,
        rgb_map = prod exp(-sigma dz), depth_map = sum(alpha z), per-ray entropy masked at 1 - rgb_map > 0.4)."""
    z = depth_values
    step = torch.cat((z[..., 1:] - z[..., :-1], torch.full_like(z[..., :1], 1e10)), dim=-1)
    if radiance_field.shape[-1] == 2:
        sigma_a, rgb = torch.relu(radiance_field[..., 1]), torch.sigmoid(radiance_field[..., :1])
        opacity = 1.0 - torch.exp(-sigma_a * step)
        weights = opacity * cumprod_exclusive(1.0 - opacity + 1e-10)
        rgb_map = (weights.unsqueeze(-1) * rgb).sum(dim=-2).squeeze()
        depth_map = (weights * z).sum(dim=-1)
        total = opacity.sum(dim=-1)
        p = opacity / (total.unsqueeze(-1) + 1e-10)
        per_ray = -(p * torch.log(p + 1e-10)).sum(dim=-1) * (total > 0.7).detach()
        return rgb_map, depth_map, weights, per_ray.mean(), [sigma_a, rgb]
    sigma_a = torch.relu(radiance_field.mean(dim=-1))
    trans = torch.exp(-sigma_a * (step * ray_directions.norm(dim=-1, keepdim=True)))
    weights = (1.0 - trans + 1e-10) * cumprod_exclusive(trans)
    rgb_map = trans.prod(dim=-1)
    depth_map = (trans * z).sum(dim=-1)
    rgb = torch.ones(*sigma_a.shape[:2], 1, device=sigma_a.device)
    return rgb_map, depth_map, weights, get_ray_entropy(sigma_a, rgb_map), [sigma_a, rgb]


def render_volume_density(radiance_field, ray_directions, depth_values, raw_noise_std=0.):
    """nerf/nerf_helpers.py:59-123 -> (rgb_map, depth_map, weights, entropy, [sigma_a, rgb]).  The configuration the reference
    trains - ONE output channel (sigmoid density, absorption only) - runs in the HIP library (afx_composite_dense; the gradient
    flows through rgb_map, the quantity the loss uses; depth_map / weights / entropy are returned detached).  The reference's
    quirks are kept in the kernel: last distance 1e10 (D3), ||d|| scaling (D4), depth_map = sum(alpha*z) (D5).  The
    emission-absorption (2-channel) and mean-relu (> 2) branches, which the reference's training path never takes, run on
    PyTorch-ROCm operators (same device, not accelerated).  Host tensors are refused - there is no CPU fallback (tests
    compare with oracle/)."""
    if not radiance_field.is_cuda:
        from .._lib import AfxError
        raise AfxError("render_volume_density: tensors must live on the GPU; there is no CPU fallback")
    if radiance_field.shape[-1] != 1:
        return _render_volume_density_ops(radiance_field.float(), ray_directions.float(), depth_values.float())
    raw = radiance_field[..., 0].float().contiguous()
    rgb_map, depth_map, weights, entropy, sigma_a = _CompositeDenseFn.apply(raw, ray_directions.float().contiguous(),
                                                                             depth_values.float().contiguous())
    return rgb_map, depth_map, weights, entropy, [sigma_a, torch.ones(*sigma_a.shape, 1, device=raw.device)]


def sample_pixel_rays(train_ray_df, img_sample_size, device, weights=None, unseen=False):
    """Weighted sampling without replacement over all pixels of all training projections, then shuffle
    (nerf/nerf_helpers.py:137-150) -> [origins[R,3], directions[R,3], pixel_values[R]] fp32 on device."""
    ray_batch = train_ray_df.sample(n=img_sample_size, weights=weights).sample(frac=1)
    batch_pix_vals = None
    if not unseen:
        batch_pix_vals = torch.from_numpy(ray_batch['pixel_value'].to_numpy()).to(device).float()
    batch_origins = torch.from_numpy(np.asarray(ray_batch['ray_origins'].tolist(), dtype=np.float32)).to(device)
    batch_directions = torch.from_numpy(np.asarray(ray_batch['ray_directions'].tolist(), dtype=np.float32)).to(device)
    return [batch_origins, batch_directions, batch_pix_vals]


def sample_image_rays(train_df, train_ray_df, img_sample_size, device, random=False):
    """nerf/nerf_helpers.py:152-176."""
    proj_id = train_df.sample(n=1).index[0]
    rays = train_ray_df[train_ray_df['image_id'] == proj_id].copy()
    if not random:
        side = int(np.sqrt(img_sample_size))
        pix = torch.zeros(side, side)
        pix[rays['x_position'].tolist(), rays['y_position'].tolist()] = torch.Tensor(rays['pixel_value'].tolist())
        pix = pix.flatten().to(device)
    else:
        rays = rays.sample(n=img_sample_size)
        pix = torch.Tensor(rays['pixel_value'].tolist()).to(device)
    origins = torch.from_numpy(np.asarray(rays['ray_origins'].tolist(), dtype=np.float32)).to(device)
    directions = torch.from_numpy(np.asarray(rays['ray_directions'].tolist(), dtype=np.float32)).to(device)
    return [origins, directions, pix]


def sample_pdf(bins, weights, N_samples, device, u=None):
    """Inverse-CDF sampling of `N_samples` depths per ray from the piecewise-constant density `weights` over `bins`
    (nerf/nerf_helpers.py:197-222).  `u` lets the caller supply the uniform draw (parity tests); default torch.rand."""
    mass = weights + 1e-5
    cdf = torch.cumsum(mass / mass.sum(dim=-1, keepdim=True), dim=-1)
    cdf = torch.nn.functional.pad(cdf, (1, 0))                            # leading 0
    if u is None:
        u = torch.rand(*cdf.shape[:-1], N_samples).to(weights)
    hi = torch.searchsorted(cdf, u.contiguous(), right=True)
    lo = (hi - 1).clamp(min=0)
    hi = hi.clamp(max=cdf.shape[-1] - 1)
    c0, c1 = cdf.gather(-1, lo), cdf.gather(-1, hi)
    b0, b1 = bins.gather(-1, lo), bins.gather(-1, hi)
    width = c1 - c0
    width = torch.where(width < 1e-5, torch.ones_like(width), width)      # empty interval: take its left edge
    return b0 + (u - c0) / width * (b1 - b0)


def fine_sampling(depth_values, weights_coarse, ray_origins, ray_directions, coarse_model, fine_model,
                  depth_samples_per_ray_fine, chunksize, u=None):
    """Hierarchical re-sampling and re-rendering (nerf/nerf_helpers.py:178-195) ->
    (rgb_map_fine, depth_map_fine, entropy_fine).  The upstream call at :191 passes a stray positional
    argument to get_predictions and cannot run; it is restated without it.  The merged depths
    (bins = mid-points of the coarse depths, weights[..., 1:-1], sort(cat(coarse, samples))) come from afx_fine_depths
    and the fine pass is the fused renderer; GPU only."""
    from ..render import render_rays
    network = coarse_model if fine_model is None else fine_model
    if not weights_coarse.is_cuda:
        from .._lib import AfxError
        raise AfxError("fine_sampling: tensors must live on the GPU; there is no CPU fallback")
    n_rays = ray_origins.shape[0]
    if u is None:
        u = torch.rand(n_rays, depth_samples_per_ray_fine, device=weights_coarse.device)
    depth_vals = _engine.fine_depths(depth_values.float().contiguous(), weights_coarse.detach().float().contiguous(), u)
    if not getattr(network, "fused", False):
        # configurations outside the fused kernels (tanh / sine / skip block / several channels): the reference's own sequence
        # (:187-192) on the module's PyTorch-ROCm operators - points, chunked predictions, dense compositing
        pts = ray_origins[..., None, :] + ray_directions[..., None, :] * depth_vals[..., :, None]
        raw = get_predictions(network, pts.reshape(-1, 3), chunksize).reshape(n_rays, depth_vals.shape[-1], -1)
        rgb_map, depth_map, _, entropy, _ = render_volume_density(raw, ray_directions, depth_vals)
        return rgb_map, depth_map, entropy
    out = render_rays(network, ray_origins, ray_directions, mode="dense", z=depth_vals, want_aux=True)
    return out.rgb_map, out.depth_map, out.entropy


def sample_depth(batch_directions, depth_samples_per_ray_coarse, device):
    """nerf/nerf_helpers.py:245-257: jittered depths on the unit interval -> (near, far, z)."""
    from .._geometry import uniform_depths
    return 0, 1, randomize_depth(uniform_depths(0, 1, depth_samples_per_ray_coarse).to(device), device)
