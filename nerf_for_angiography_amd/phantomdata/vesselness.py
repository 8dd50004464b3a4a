"""The Frangi vesselness filter and the Euclidean distance transform on the GPU (HIP kernels behind afx_frangi and
afx_distance_transform_edt, include/afx.h): what get_weighted_img (phantomdata/helpers.py:226-247 upstream) takes from
scikit-image and SciPy.

`frangi` follows scikit-image 0.18.3 (skimage/filters/ridges.py::frangi with compute_hessian_eigenvalues and
skimage/feature/corner.py::hessian_matrix / hessian_matrix_eigvals); the reference pins no version, and 0.19 changed the
default gamma, how the Hessian is built and the background rule.  For each image I (float64) and each sigma:
  1. black_ridges: I <- 1 - I
  2. G = scipy.ndimage.gaussian_filter(I, sigma), truncate 4, mode 'reflect'
  3. np.gradient of G along both axes, np.gradient of those (unit spacing): Hrr, Hrc, Hcc, each times sigma^2
  4. eigenvalues l+- = (Hrr + Hcc) / 2 +- sqrt(4 Hrc^2 + (Hrr - Hcc)^2) / 2, sorted by magnitude: |lambda1| <= |lambda2|
     (a tie: lambda1 = l+)
  5. v = exp(-rb / 2 beta^2) (1 - exp(-(lambda1^2 + lambda2^2) / 2 gamma^2)), rb = (lambda1 / |lambda2|)^2 (|lambda2| = 0 -> 1e-10),
     and v = 0 where lambda2 > 0
  6. out = max over the sigmas
alpha only weighs the plate-like term of 3-D images (r_a = inf in 2-D): it is accepted and has no effect.

`distance_transform_edt` is scipy.ndimage.distance_transform_edt bit for bit: the distance from every non-zero pixel to the
nearest zero pixel (an image without a zero pixel gives +inf everywhere, where SciPy's result is undefined).

Both take device tensors [H, W] or [N, H, W] (all images in one launch sequence) and return float64 of the same shape.  Host
tensors are refused: there is no CPU path."""
from __future__ import annotations

import torch

from .. import engine


def frangi(images: torch.Tensor, sigmas=range(1, 10, 2), alpha: float = 0.5, beta: float = 0.5, gamma: float = 15,
           black_ridges: bool = True) -> torch.Tensor:
    """skimage.filters.frangi (0.18.3) of a [H, W] or [N, H, W] device tensor, float64."""
    del alpha                      # no effect in 2-D (see the module docstring)
    out = engine.frangi(images, sigmas=tuple(sigmas), beta=beta, gamma=gamma, black_ridges=black_ridges)
    return out if images.dim() == 3 else out[0]


def distance_transform_edt(x: torch.Tensor) -> torch.Tensor:
    """scipy.ndimage.distance_transform_edt of a [H, W] or [N, H, W] device tensor (non-zero = foreground), float64."""
    out = engine.distance_transform_edt(x)
    return out if x.dim() == 3 else out[0]
