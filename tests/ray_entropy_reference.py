"""The torch restatement of the per-ray entropy the ray-entropy tests measure the HIP kernels against, and their tolerance rule.

    D = sum_i sigma_i + eps, p_i = sigma_i / D, E = -sum_i p_i log(p_i + eps), entropy = E * [(1 - T) > threshold]

(get_ray_entropy of the reference, nerf/nerf_helpers.py:125-135 and nerf/nerf_helpers_acc.py:33-43.)  tests/test_ray_entropy_cpu.py pins
`entropy_dense` against the reference's own outputs and autograd gradient (fixture g12); `entropy_packed` is the same six lines with
index_add_ sums, for the packed layout, which has no importable reference."""
import torch

EPS = 1e-10


def entropy_dense(raw, rgb_map, threshold=0.4):
    """raw[R,S] (before the sigmoid), rgb_map[R] -> entropy[R]; differentiable in raw, in raw's dtype."""
    sigma = torch.sigmoid(raw)
    p = sigma / (sigma.sum(dim=-1, keepdim=True) + EPS)
    e = -(p * torch.log(p + EPS)).sum(dim=-1)
    return e * ((1 - rgb_map) > threshold).detach()


def entropy_packed(pred, rgb_map, ray_indices, n_rays, threshold=0.4):
    """pred[n], rgb_map[n_rays], ray_indices[n] (sorted) -> entropy[n_rays]; a ray without samples gives 0."""
    ri = ray_indices.long()
    sigma = torch.sigmoid(pred)
    p = sigma / (torch.zeros(n_rays, dtype=pred.dtype).index_add_(0, ri, sigma) + EPS)[ri]
    e = -torch.zeros(n_rays, dtype=pred.dtype).index_add_(0, ri, p * torch.log(p + EPS))
    return e * ((1 - rgb_map) > threshold).detach()


def value_and_grad(fn, x, *args):
    x = x.detach().clone().requires_grad_(True)
    e = fn(x, *args)
    (g,) = torch.autograd.grad(e.sum(), x)
    return e.detach(), g


def rel_l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    den = float(b.norm())
    return float((a - b).norm()) / (den if den > 0 else 1.0)


def bars(fn, x32, rgb_map, *args, sample_mask=None):
    """The tolerance rule: the same torch expression on the CPU in fp32 and in fp64 on the test's inputs; the bar for the kernel is
    10 x that fp32-vs-fp64 relative L2 (separately for value and gradient, floor 1e-6): the margin covers another summation order and
    logf / expf differences of a few ulp.  The gradient norm is taken over the samples of rays with mask 1 (`sample_mask`).
    -> (entropy64, grad64, value bar, gradient bar)."""
    x32 = x32.detach().float().cpu()
    e64, g64 = value_and_grad(fn, x32.double(), rgb_map.double().cpu(), *args)
    e32, g32 = value_and_grad(fn, x32, rgb_map.float().cpu(), *args)
    m = slice(None) if sample_mask is None else sample_mask
    return e64, g64, max(10.0 * rel_l2(e32, e64), 1e-6), max(10.0 * rel_l2(g32[m], g64[m]), 1e-6)


# ---- the problems of tests/test_gpu_ray_entropy.py (built on the CPU from a seeded generator, so their preconditions hold everywhere) ----
RAGGED = [0, 1, 2, 31, 32, 33, 63, 64, 65, 130, 0, 300]      # segments of 0, 1, < 64, == 64, > 64 samples; empty rays inside the list


def ragged_problem(lengths, seed, pred=None):
    """A packed, ray-sorted list: pred ~ N(0, 1.5) fp32 (or the given one), ray_indices int32, random t_starts < t_ends whose total
    length per ray is drawn so that the rays' absorption 1 - T spreads over both sides of the 0.4 threshold."""
    g = torch.Generator().manual_seed(seed)
    lengths = torch.as_tensor(lengths)
    n = int(lengths.sum())
    ri = torch.arange(len(lengths), dtype=torch.int32).repeat_interleave(lengths)
    if pred is None:
        pred = 1.5 * torch.randn(n, generator=g)
    per_ray = 0.2 + 2.2 * torch.rand(len(lengths), generator=g)      # sum of the ray's interval lengths (sigma ~ 0.5: optical depth 0.1 .. 1.2)
    dt = torch.rand(n, generator=g) + 0.1
    dt = dt / torch.zeros(len(lengths)).index_add_(0, ri.long(), dt)[ri.long()] * per_ray[ri.long()]
    gap = 0.05 * torch.rand(n, generator=g)
    t_ends = torch.cumsum(dt + gap, 0)
    t_starts = t_ends - dt
    return pred.float(), ri, t_starts.float().contiguous(), t_ends.float().contiguous()


def transmittance(pred, ri, t_starts, t_ends, n_rays):
    """acc_render_volume_density's rgb_map in pred's dtype: exp(-sum_i sigmoid(pred_i) (t_end_i - t_start_i)) per ray."""
    tau = torch.sigmoid(pred) * (t_ends.to(pred.dtype) - t_starts.to(pred.dtype))
    return torch.exp(-torch.zeros(n_rays, dtype=pred.dtype).index_add_(0, ri.long(), tau))


def mask_margin(rgb_map64, threshold=0.4):
    """The precondition of every comparison: no ray within 1e-3 of the threshold, so fp32 and fp64 agree on the mask."""
    return float(((1.0 - rgb_map64) - threshold).abs().min())


MODULE_CFG = dict(num_early_layers=2, num_filters=64)      # the 2 x 64 ReLU CPPN of the combined-loss test


def module_problem(seed, n_rays=37):
    """37 rays with a ragged packed list (empty rays and segments beyond 64 samples among them), one query point per sample, a target
    pixel per ray and nn.Linear-style parameters (oracle.init_params; the output weights scaled by 8 so the densities along a ray differ)."""
    from oracle import angio_oracle as orc
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(1, 90, (n_rays,), generator=g)
    lengths[torch.randperm(n_rays, generator=g)[:4]] = 0
    pts = 2.0 * torch.rand(int(lengths.sum()), 3, generator=g) - 1.0
    _, ri, ts, te = ragged_problem(lengths, seed + 1, pred=torch.zeros(int(lengths.sum())))
    target = torch.rand(n_rays, generator=g)
    params = orc.init_params(MODULE_CFG, seed)
    params["output_linear.0.weight"] = params["output_linear.0.weight"] * 8.0
    return lengths, pts, ri, ts, te, target, params


def combined_loss(pred, ri, ts, te, target, weight, threshold=0.4):
    """mse(rgb_map, target) + weight * mean(entropy) from torch operators, on pred's device and in its dtype; rgb_map detached in the mask."""
    n_rays, ril = target.numel(), ri.long()
    sigma = torch.sigmoid(pred)
    zeros = torch.zeros(n_rays, dtype=pred.dtype, device=pred.device)
    rgb = torch.exp(-zeros.index_add(0, ril, sigma * (te.to(pred.dtype) - ts.to(pred.dtype))))
    p = sigma / (zeros.index_add(0, ril, sigma) + EPS)[ril]
    ent = -zeros.index_add(0, ril, p * torch.log(p + EPS)) * ((1 - rgb) > threshold).detach()
    return torch.nn.functional.mse_loss(rgb, target.to(pred.dtype)) + weight * ent.mean()


def module_grads_cpu(problem, weight, dtype):
    """Parameter gradients of combined_loss through the oracle's CPPN on the CPU in `dtype` -> (flat gradient, rgb_map)."""
    from oracle import angio_oracle as orc
    _, pts, ri, ts, te, target, params = problem
    leaf = {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    pred = orc.cppn_forward(pts.to(dtype), MODULE_CFG, leaf).reshape(-1)
    loss = combined_loss(pred, ri, ts, te, target, weight)
    grads = torch.autograd.grad(loss, [leaf[k] for k in sorted(leaf)])
    return torch.cat([x.reshape(-1) for x in grads]), transmittance(pred.detach(), ri, ts, te, target.numel())
