#!/usr/bin/env python3
"""Capture fixture G12 (per-ray entropy of the density profile and its gradient) from the upstream reference's
nerf/nerf_helpers.py: render_volume_density (:59-123, one output channel) with get_ray_entropy (:125-135), and
d(entropy.sum())/d raw from the reference's own autograd.

    AFX_REFERENCE=<checkout of the reference> python tools/make_golden_g12.py

The inputs are float32 values; the reference runs on them in float64, so the fixture is a yardstick for fp32 kernels.
Both mask states occur (rays with 1 - rgb_map above and below the 0.4 threshold) and no ray lies within 1e-3 of the
threshold, so fp32 and fp64 agree on the mask.  The fixture is data only; nothing under tests/, bench.py or the
package imports this script."""
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get("AFX_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("set AFX_REFERENCE to a checkout of the reference project")
sys.path.insert(0, REF)

import numpy as np
import torch

from nerf import nerf_helpers as nh  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
R, S, THRESHOLD = 48, 33, 0.4

g = torch.Generator().manual_seed(12)
# D3: the last distance is 1e10, so rgb_map is 0 unless the last sample's density vanishes: raw[:, -1] = -40.  The other raws are
# N(0, 1.5) shifted per ray so that the optical depth sum sigma dz ||d|| runs from ~0.1 to ~1.3 across the rays (-log(0.6) = 0.51)
z = torch.linspace(2.0, 6.0, S)
dirs = torch.randn(R, 3, generator=g)
dirs = dirs / dirs.norm(dim=-1, keepdim=True) * (0.8 + 0.4 * torch.rand(R, 1, generator=g))
shift = torch.linspace(-4.5, -1.0, R)[torch.randperm(R, generator=g)]
raw = 1.5 * torch.randn(R, S, generator=g) + shift[:, None]
raw[:, -1] = -40.0
raw, dirs, z = raw.float(), dirs.float(), z.float()

raw64 = raw.double().requires_grad_(True)
rgb_map, depth_map, weights, entropy, _ = nh.render_volume_density(raw64[..., None], dirs.double(), z.double())
(d_raw,) = torch.autograd.grad(entropy.sum(), raw64)

margin = (1.0 - rgb_map.detach() - THRESHOLD).abs().min()
mask = (1.0 - rgb_map.detach()) > THRESHOLD
assert float(margin) >= 1e-3, f"a ray lies within 1e-3 of the mask threshold (margin {float(margin):.2e}): change the seed"
assert 0.3 * R <= int(mask.sum()) <= 0.7 * R, f"{int(mask.sum())} of {R} rays above the threshold: both mask states must be well populated"
assert bool((entropy.detach()[mask] > 0).all()) and bool((entropy.detach()[~mask] == 0).all())

path = os.path.join(OUT, "g12_ray_entropy.npz")
np.savez(path, raw=raw.numpy(), dirs=dirs.numpy(), z=z.numpy(), rgb_map=rgb_map.detach().numpy(), entropy=entropy.detach().numpy(),
         d_raw=d_raw.numpy(), threshold=np.array(THRESHOLD))
print(f"g12_ray_entropy: {os.path.getsize(path) / 1024:.1f} KiB, {int(mask.sum())} of {R} rays above the threshold, "
      f"closest |1 - T - {THRESHOLD}| = {float(margin):.3e}")
