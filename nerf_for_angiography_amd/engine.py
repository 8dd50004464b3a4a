"""Host-side driver of libafx.so: owns the torch buffers (prepared weights, workspace) the C-ABI
works on and exposes the fused kernels to the Python mirror of the reference interface.
PyTorch is used for device memory and streams only."""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import AfxError, ModelDesc, RenderArgs


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- the buffer vocabulary of every wrapper: each tensor whose pointer goes to the library passes _buffer, _out or _scratch on the host, before the
# first launch - dtype, count and contiguity against the device of the wrapper's first tensor, then _on_gpu; nothing is converted but a strided input ----
EDT3D_MAX_SIDE = 1024                 # AFX_EDT3D_MAX_SIDE


def _on_gpu(t, name: str, who: str):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise AfxError(f"{who}: {name} must be a tensor on a GPU; there is no CPU path")
    return t


def _buffer(t, name: str, dtype, shape, dev, who: str, exact_shape: bool = False, at_least: bool = False, copy: bool = False):
    """A tensor the library reads or writes through its pointer: contiguous, of `dtype` (one, or a tuple of admitted ones), on `dev`, with
    prod(shape) elements (`shape` may be the count itself; None: any number; at_least: that many or more; exact_shape: of that very
    shape) -> t.  copy: an input the library only reads may be strided (a column-major ray table, a [:, None] view) and comes back as a
    contiguous copy.  ValueError otherwise, in one wording."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    shape = shape if shape is None or isinstance(shape, (tuple, torch.Size)) else (int(shape),)
    if isinstance(t, torch.Tensor) and t.dtype in dtypes and t.device == dev and (copy or t.is_contiguous()):
        if shape is None or (tuple(t.shape) == tuple(shape) if exact_shape else
                             t.numel() >= math.prod(shape) if at_least else t.numel() == math.prod(shape)):
            return t.contiguous() if copy else t
    size = "" if shape is None else f" of shape {tuple(shape)}" if exact_shape else \
        f" of {'at least ' if at_least else ''}{math.prod(shape)} elements {tuple(shape)}"
    got = f"{t.dtype} {tuple(t.shape)} on {t.device}, contiguous = {t.is_contiguous()}" if isinstance(t, torch.Tensor) else type(t).__name__
    raise ValueError(f"{who}: {name} must be a {'' if copy else 'contiguous '}{' or '.join(str(d) for d in dtypes)} tensor{size} on {dev}, got {got}")


def _out(t, name: str, dtype, shape, dev, who: str, ok: bool = True, exact_shape: bool = False, at_least: bool = False):
    """An output, record or state buffer: allocated unless the caller passed it, else checked as `_buffer` does.  ok=False: a shape the
    library refuses gets a one-element buffer, so the call reports the limits instead of the allocator failing first (a buffer the
    caller passed is then not held to the count: the library refuses before it writes)."""
    if t is None:
        return torch.empty(shape if ok else (1,), dtype=dtype, device=dev)
    return _buffer(t, name, dtype, shape if ok else None, dev, who, exact_shape, at_least)


def _scratch(workspace, nbytes: int, dev, who: str):
    """-> (workspace, its size in bytes): max(nbytes, 1) fresh bytes unless the caller passed a contiguous tensor on `dev`.  Whether that one
    is large enough is the library's to say (afx::check_workspace)."""
    if workspace is None:
        workspace = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    elif not isinstance(workspace, torch.Tensor) or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"{who}: workspace must be a contiguous tensor on {dev}")
    return workspace, workspace.numel() * workspace.element_size()


def _volume_side_ok(shape) -> bool:
    """Every side of a volume within the library's 1..AFX_EDT3D_MAX_SIDE."""
    return all(1 <= int(n) <= EDT3D_MAX_SIDE for n in shape)


def ray_window(who: str, n_proj: int, width: int, height: int, ray_id0: int = 0, n_rays=None, ray_ids=None) -> int:
    """The rays a pose-mode call asks for, out of the [n_proj, height, width] ray table -> their number.  `ray_ids` (any integer tensor)
    names them one by one; otherwise they are ray_id0 .. ray_id0 + n_rays, n_rays defaulting to the rest of the table.  Anything outside
    the table is refused here: the kernels index `poses` by ray id / (height width) without a check of their own."""
    table = int(n_proj) * int(width) * int(height)
    shape = f"the {int(n_proj)} x {int(height)} x {int(width)} table"
    if int(n_proj) < 0 or int(width) < 0 or int(height) < 0:
        raise ValueError(f"{who}: n_proj, height and width must be >= 0, got {shape}")
    if ray_ids is not None:
        if ray_ids.is_floating_point() or ray_ids.dtype == torch.bool:
            raise ValueError(f"{who}: ray_ids: dtype {ray_ids.dtype}, expected an integer type")
        n_rays = ray_ids.numel() if n_rays is None else int(n_rays)
        if n_rays < 0 or n_rays > ray_ids.numel():
            raise ValueError(f"{who}: n_rays = {n_rays} with {ray_ids.numel()} ray_ids")
        if n_rays:
            lo, hi = int(ray_ids.reshape(-1)[:n_rays].min()), int(ray_ids.reshape(-1)[:n_rays].max())
            if lo < 0 or hi >= table:
                raise ValueError(f"{who}: ray_ids {lo} .. {hi} outside {shape} (0 .. {table - 1})")
        return n_rays
    ray_id0 = int(ray_id0)
    n_rays = table - ray_id0 if n_rays is None else int(n_rays)
    if ray_id0 < 0 or n_rays < 0 or ray_id0 + n_rays > table:
        what = "ray_id0" if ray_id0 < 0 or ray_id0 > table else "n_rays"
        raise ValueError(f"{who}: {what}: rays {ray_id0} .. {ray_id0 + n_rays} outside {shape} (0 .. {table})")
    return n_rays


@dataclass
class RenderSpec:
    """One ray batch for the fused renderer.

    Rays: either origins/dirs [R,3] fp32 (what sample_pixel_rays returns), or poses [n_proj,3,4] float64 +
    ray_ids (int32 index into [n_proj,H,W]; None => rays ray_id0 .. ray_id0+R-1) + width/height/focal
    (in-kernel get_ray_values).  Depths: mode 'acc' (uniform mid-point march t_near..t_far, the convention of
    nerf_helpers_acc.py), 'dense' with z [S] or [R,S] (render_volume_density convention), 'stratified' (dense convention
    with randomize_depth(linspace(t_near, t_far, S)) drawn in the kernel from Philox (jitter_seed, jitter_stream))."""
    n_rays: int
    n_samples: int
    origins: Optional[torch.Tensor] = None
    dirs: Optional[torch.Tensor] = None
    poses: Optional[torch.Tensor] = None
    ray_ids: Optional[torch.Tensor] = None
    ray_id0: int = 0
    width: int = 0
    height: int = 0
    focal: float = 0.0
    mode: str = "acc"
    t_near: float = 0.0
    t_far: float = 0.0
    z: Optional[torch.Tensor] = None
    jitter_seed: int = 0          # mode 'stratified': Philox stream of the in-kernel randomize_depth draw
    jitter_stream: int = 0


class Engine:
    """One CPPN geometry on one GPU."""

    def __init__(self, width: int, n_hidden: int, enc: str = "none", n_freq: int = 0,
                 max_workspace_bytes: int = 24 << 30, variant: str = "", act: str = "relu", act_w0: float = 1.0):
        self.lib = _lib.load(variant)
        self.act = act
        self.desc = ModelDesc(3, _lib.ENC[enc], int(n_freq), int(width), int(n_hidden), _lib.ACT[act], float(act_w0))
        h = C.c_void_p()
        self._check(self.lib.afx_create(C.byref(self.desc), C.byref(h)), "afx_create")
        self.h = h
        self.width, self.n_hidden, self.enc, self.n_freq = width, n_hidden, enc, int(n_freq)
        self._prepared_bytes = {}      # prec -> the size of its prepared buffer
        self.param_count = int(self.lib.afx_query(h, _lib.Q_PARAM_COUNT, 0, 0, 0))
        self.k0 = int(self.lib.afx_query(h, _lib.Q_K0, 0, 0, 0))
        self.max_workspace_bytes = int(max_workspace_bytes)
        self._prepared = {}      # prec -> (buffer, version key)
        self._ws = None
        self._ws_captured = False
        self._retired = []       # workspaces a captured graph still points at

    def _check(self, rc, what):
        _lib.check(rc, what, self.lib)

    def _last_error(self) -> str:
        msg = self.lib.afx_last_error()
        return msg.decode() if msg else "?"

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.afx_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- measurement ---------------------------------------------------------------------------
    KERNELS = {"chain_fwd": 0, "chain_bwd": 1, "wgrad": 2}

    def profile(self, on: bool):
        self._check(self.lib.afx_profile_enable(self.h, int(on)), "afx_profile_enable")

    def profile_read(self, kernel: str):
        """(total device ms, launches) of one kernel kind since the last read (HIP events on the launch stream)."""
        ms, n = C.c_double(), C.c_int64()
        self._check(self.lib.afx_profile_read(self.h, self.KERNELS[kernel], C.byref(ms), C.byref(n)), "afx_profile_read")
        return ms.value, n.value

    # ---- parameter layout ------------------------------------------------------------------
    def layout(self, layer: int):
        wo, bo, r, c = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        self._check(self.lib.afx_param_layout(self.h, layer, C.byref(wo), C.byref(bo), C.byref(r), C.byref(c)),
                   "afx_param_layout")
        return wo.value, bo.value, r.value, c.value

    @staticmethod
    def _stream(device):
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def _workspace(self, nbytes: int, device) -> torch.Tensor:
        """The (one) workspace buffer, grown on demand.  A HIP graph captured over a call keeps the buffer's address:
        a buffer that a capture has seen is never freed when a later, larger request replaces it, and growing it
        DURING a capture is refused (run the step once eagerly first - that sizes it)."""
        capturing = device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            if capturing:
                raise AfxError("the workspace must be sized before graph capture: run the same call once eagerly first")
            if self._ws is not None and self._ws_captured:
                self._retired.append(self._ws)
            # a request that outgrows the buffer gets 25 % head-room (within the cap): the packed / points paths ask for a slightly different
            # size every iteration, and a hipMalloc per new maximum (several ms at GB sizes) would dominate them
            grow = self._ws is not None and self._ws.device == device
            self._ws = None
            size = int(nbytes)
            if grow:
                size = max(size, min(int(size * 1.25), max(self.max_workspace_bytes, size)))
            self._ws = torch.empty(size, dtype=torch.uint8, device=device)
            self._ws_captured = False
        if capturing:
            self._ws_captured = True
        return self._ws

    # ---- weights -----------------------------------------------------------------------------
    def _model(self, who: str, prepared, prec: str, grad_flat=None):
        """-> prepared's device.  `prepared` holds at least the bytes prepare() allocates at `prec` (asked of the library once per
        precision), `grad_flat` (None: not given) is float32 [param_count] on that device: the kernels add param_count floats to it."""
        if prec not in self._prepared_bytes:
            self._prepared_bytes[prec] = int(self.lib.afx_query(self.h, _lib.Q_PREPARED_BYTES, _lib.PREC[prec], 0, 0))
        dev = prepared.device
        _buffer(prepared, "prepared", torch.uint8, self._prepared_bytes[prec], dev, who, at_least=True)
        if grad_flat is not None:
            _buffer(grad_flat, "grad_flat", torch.float32, self.param_count, dev, who)
        return dev

    def prepare(self, flat: torch.Tensor, enc_aux: Optional[torch.Tensor], prec: str, key=None):
        """Re-tile the flat parameters for `prec` unless `key` says the cached copy is current."""
        dev = flat.device
        flat = _buffer(flat, "flat parameters", torch.float32, self.param_count, dev, "prepare", copy=True)
        _on_gpu(flat, "flat parameters", "prepare")
        p = _lib.PREC[prec]
        cached = self._prepared.get(prec)
        if cached is not None and key is not None and cached[1] == key and cached[0].device == flat.device:
            return cached[0]
        nbytes = int(self.lib.afx_query(self.h, _lib.Q_PREPARED_BYTES, p, 0, 0))
        buf = cached[0] if cached is not None and cached[0].device == flat.device else torch.empty(
            nbytes, dtype=torch.uint8, device=flat.device)
        if enc_aux is not None:
            enc_aux = _buffer(enc_aux, "enc_aux", torch.float32, None, dev, "prepare", copy=True)
        self._check(self.lib.afx_prepare_weights(self.h, p, _ptr(flat), _ptr(enc_aux), _ptr(buf), nbytes,
                                                self._stream(flat.device)), "afx_prepare_weights")
        self._prepared[prec] = (buf, key)
        return buf

    # ---- MLP on explicit points --------------------------------------------------------------
    def infer(self, prepared: torch.Tensor, pts: torch.Tensor, prec: str, apply_sigmoid: bool = False):
        dev = self._model("infer", prepared, prec)
        pts = _buffer(pts, "points", torch.float32, None, dev, "infer", copy=True)
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"points: shape {tuple(pts.shape)}, expected [P,3]")
        _on_gpu(prepared, "prepared", "infer")
        out = torch.empty(pts.shape[0], dtype=torch.float32, device=dev)
        self._check(self.lib.afx_mlp_infer(self.h, _lib.PREC[prec], _ptr(prepared), _ptr(pts), pts.shape[0], _ptr(out),
                                          int(apply_sigmoid), self._stream(dev)), "afx_mlp_infer")
        return out

    @contextlib.contextmanager
    def encoding_grad(self, flat: torch.Tensor, d_aux: Optional[torch.Tensor]):
        """Backward calls inside this scope also accumulate d loss / d fourier coefficients into `d_aux`
        (afx_set_encoding_grad); None: plain scope."""
        if d_aux is None:
            yield
            return
        _buffer(flat, "flat", torch.float32, self.param_count, flat.device, "encoding_grad")
        # (only the fourier encoding has coefficients, 3 n_freq of them; which encodings train is the library's to say)
        _buffer(d_aux, "d_aux", torch.float32, 3 * self.n_freq if self.enc == "fourier" else None, flat.device, "encoding_grad")
        _on_gpu(flat, "flat", "encoding_grad")
        self._check(self.lib.afx_set_encoding_grad(self.h, _ptr(flat), _ptr(d_aux)), "afx_set_encoding_grad")
        try:
            yield
        finally:
            self.lib.afx_set_encoding_grad(self.h, None, None)

    def mlp_backward(self, prepared, pts, d_out, grad_flat, prec: str):
        dev = self._model("mlp_backward", prepared, prec, grad_flat)
        pts = _buffer(pts, "points", torch.float32, None, dev, "mlp_backward", copy=True)
        n = pts.shape[0]
        d_out = _buffer(d_out, "d_out", torch.float32, n, dev, "mlp_backward", copy=True)
        _on_gpu(prepared, "prepared", "mlp_backward")
        full = int(self.lib.afx_query(self.h, _lib.Q_BWD_WORKSPACE_FULL, 0, n, _lib.PREC[prec]))
        ws = self._workspace(min(full, self.max_workspace_bytes), dev)
        self._check(self.lib.afx_mlp_backward(self.h, _lib.PREC[prec], _ptr(prepared), _ptr(pts), n, _ptr(d_out),
                                             _ptr(grad_flat), _ptr(ws), ws.numel(), self._stream(dev)),
                   "afx_mlp_backward")

    def mlp_backward_inputs(self, prepared, pts, d_out, grad_flat, d_pts, prec: str):
        """afx_mlp_backward_inputs: d_pts [P,3] = dL/dpts (written); grad_flat += dL/dparams unless it is None."""
        dev = self._model("mlp_backward_inputs", prepared, prec, grad_flat)
        pts = _buffer(pts, "points", torch.float32, None, dev, "mlp_backward_inputs", copy=True)
        n = pts.shape[0]
        d_out = _buffer(d_out, "d_out", torch.float32, n, dev, "mlp_backward_inputs", copy=True)
        _buffer(d_pts, "d_pts", torch.float32, (n, 3), dev, "mlp_backward_inputs", exact_shape=True)
        _on_gpu(prepared, "prepared", "mlp_backward_inputs")
        full = int(self.lib.afx_query(self.h, _lib.Q_BWD_INPUTS_WORKSPACE_FULL, 0, n, _lib.PREC[prec]))
        ws = self._workspace(min(full, self.max_workspace_bytes), dev)
        self._check(self.lib.afx_mlp_backward_inputs(self.h, _lib.PREC[prec], _ptr(prepared), _ptr(pts), n, _ptr(d_out), _ptr(grad_flat),
                                                    _ptr(d_pts), _ptr(ws), ws.numel(), self._stream(dev)), "afx_mlp_backward_inputs")

    # ---- fused renderer ----------------------------------------------------------------------
    def _render_args(self, spec: RenderSpec, dev, pixel, sigma=None, tau=None):
        a = RenderArgs()
        keep = []
        a.n_rays, a.n_samples = int(spec.n_rays), int(spec.n_samples)
        if spec.poses is not None:
            poses = _buffer(spec.poses, "poses", torch.float64, None, dev, "render", copy=True).reshape(-1, 12)
            keep.append(poses)
            a.ray_mode, a.poses = _lib.RAYS_POSE, poses.data_ptr()
            if spec.ray_ids is not None:
                ids = _buffer(spec.ray_ids, "ray_ids", torch.int32, spec.n_rays, dev, "render", copy=True)
                keep.append(ids)
                a.ray_ids = ids.data_ptr()
            a.ray_id0, a.width, a.height, a.focal = int(spec.ray_id0), int(spec.width), int(spec.height), float(spec.focal)
        else:
            o = _buffer(spec.origins, "origins", torch.float32, (spec.n_rays, 3), dev, "render", exact_shape=True, copy=True)
            d = _buffer(spec.dirs, "dirs", torch.float32, (spec.n_rays, 3), dev, "render", exact_shape=True, copy=True)
            keep += [o, d]
            a.ray_mode, a.origins, a.dirs = _lib.RAYS_ARRAYS, o.data_ptr(), d.data_ptr()
        if spec.mode == "acc":
            a.depth_mode, a.t_near, a.t_far = _lib.DEPTH_UNIFORM_MID, float(spec.t_near), float(spec.t_far)
        elif spec.mode == "dense":
            z = _buffer(spec.z, "z", torch.float32, None, dev, "render", copy=True)
            if z.dim() == 1 and z.shape[0] == spec.n_samples:
                a.depth_mode = _lib.DEPTH_SHARED_Z
            elif tuple(z.shape) == (spec.n_rays, spec.n_samples):
                a.depth_mode = _lib.DEPTH_PER_RAY_Z
            else:
                raise ValueError(f"z: shape {tuple(z.shape)}, expected [S] or [R,S]")
            keep.append(z)
            a.z = z.data_ptr()
        elif spec.mode == "stratified":
            a.depth_mode, a.t_near, a.t_far = _lib.DEPTH_STRATIFIED, float(spec.t_near), float(spec.t_far)
            a.jitter_seed, a.jitter_stream = int(spec.jitter_seed), int(spec.jitter_stream)
        else:
            raise ValueError(f"mode {spec.mode!r}: expected 'acc', 'dense' or 'stratified'")
        a.pixel = pixel.data_ptr()
        if sigma is not None:
            a.sigma = sigma.data_ptr()
        if tau is not None:
            a.tau = tau.data_ptr()
        return a, keep

    def render_forward(self, prepared, spec: RenderSpec, prec: str, want_sigma=False, want_tau=False):
        dev = self._model("render_forward", prepared, prec)
        pixel = torch.empty(spec.n_rays, dtype=torch.float32, device=dev)
        sigma = torch.empty(spec.n_rays, spec.n_samples, dtype=torch.float32, device=dev) if want_sigma else None
        tau = torch.empty(spec.n_rays, spec.n_samples, dtype=torch.float32, device=dev) if want_tau else None
        a, keep = self._render_args(spec, dev, pixel, sigma, tau)
        _on_gpu(prepared, "prepared", "render_forward")
        ws = self._workspace(int(self.lib.afx_query(self.h, _lib.Q_FWD_WORKSPACE, spec.n_rays, spec.n_samples, 0)), dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        self._check(self.lib.afx_render_forward(self.h, _lib.PREC[prec], _ptr(prepared), C.byref(a), self._stream(dev)),
                   "afx_render_forward")
        del keep
        return pixel, sigma, tau

    def render_backward(self, prepared, spec: RenderSpec, pixel, d_pixel, grad_flat, prec: str):
        dev = self._model("render_backward", prepared, prec, grad_flat)
        pixel = _buffer(pixel, "pixel", torch.float32, spec.n_rays, dev, "render_backward", copy=True)
        d_pixel = _buffer(d_pixel, "d_pixel", torch.float32, spec.n_rays, dev, "render_backward", copy=True)
        a, keep = self._render_args(spec, dev, pixel)
        _on_gpu(prepared, "prepared", "render_backward")
        full = int(self.lib.afx_query(self.h, _lib.Q_BWD_WORKSPACE_FULL, spec.n_rays, spec.n_samples, _lib.PREC[prec]))
        ws = self._workspace(min(full, self.max_workspace_bytes), dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        self._check(self.lib.afx_render_backward(self.h, _lib.PREC[prec], _ptr(prepared), C.byref(a), _ptr(d_pixel),
                                                _ptr(grad_flat), self._stream(dev)), "afx_render_backward")
        del keep

    def render_backward_inputs(self, prepared, spec: RenderSpec, pixel, d_pixel, grad_flat, d_origins, d_dirs, prec: str):
        """afx_render_backward_inputs: d_origins / d_dirs [R,3] (either None) = dL/d(ray origins / directions), written;
        grad_flat += dL/dparams unless it is None."""
        who = "render_backward_inputs"
        dev = self._model(who, prepared, prec, grad_flat)
        pixel = _buffer(pixel, "pixel", torch.float32, spec.n_rays, dev, who, copy=True)
        d_pixel = _buffer(d_pixel, "d_pixel", torch.float32, spec.n_rays, dev, who, copy=True)
        for t, name in ((d_origins, "d_origins"), (d_dirs, "d_dirs")):
            if t is not None:
                _buffer(t, name, torch.float32, (spec.n_rays, 3), dev, who, exact_shape=True)
        a, keep = self._render_args(spec, dev, pixel)
        _on_gpu(prepared, "prepared", who)
        full = int(self.lib.afx_query(self.h, _lib.Q_BWD_INPUTS_WORKSPACE_FULL, spec.n_rays, spec.n_samples, _lib.PREC[prec]))
        ws = self._workspace(min(full, self.max_workspace_bytes), dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        self._check(self.lib.afx_render_backward_inputs(self.h, _lib.PREC[prec], _ptr(prepared), C.byref(a), _ptr(d_pixel), _ptr(grad_flat),
                                                       _ptr(d_origins), _ptr(d_dirs), self._stream(dev)), "afx_render_backward_inputs")
        del keep

    def train_step_packed_mse(self, prepared, origins, dirs, packed: "PackedGroups", target, inv_n: float, grad_flat, prec: str):
        """afx_train_step_packed_mse: the reference's iteration body on the march's packed samples; returns the pixels [n_rays]."""
        who, n_rays, n_groups = "train_step_packed_mse", packed.n_rays, packed.n_groups
        dev = self._model(who, prepared, prec, grad_flat)
        o = _buffer(origins, "origins", torch.float32, (n_rays, 3), dev, who, exact_shape=True, copy=True)
        d = _buffer(dirs, "dirs", torch.float32, (n_rays, 3), dev, who, exact_shape=True, copy=True)
        target = _buffer(target, "target", torch.float32, n_rays, dev, who, copy=True)
        _buffer(packed.group_offsets, "group_offsets", torch.int64, n_rays + 1, dev, who)
        _buffer(packed.group_ray, "group_ray", torch.int32, n_groups, dev, who)
        _buffer(packed.ts_pad, "ts_pad", torch.float32, 32 * n_groups, dev, who)
        _buffer(packed.te_pad, "te_pad", torch.float32, 32 * n_groups, dev, who)
        _on_gpu(prepared, "prepared", who)
        pixel = torch.empty(n_rays, dtype=torch.float32, device=dev)
        full = int(self.lib.afx_query(self.h, _lib.Q_BWD_WORKSPACE_FULL, 0, max(packed.n_groups, 1) * 32, _lib.PREC[prec]))
        full += 4 * (n_rays + packed.n_groups) + 1024
        if full > self.max_workspace_bytes:
            raise AfxError(f"train_step_packed_mse: {packed.n_groups * 32} packed samples need a {full >> 20} MiB workspace in one piece "
                           f"(max_workspace_bytes = {self.max_workspace_bytes >> 20} MiB)")
        ws = self._workspace(full, dev)
        self._check(self.lib.afx_train_step_packed_mse(self.h, _lib.PREC[prec], _ptr(prepared), _ptr(o), _ptr(d), n_rays,
                                                      _ptr(packed.group_offsets), _ptr(packed.group_ray), packed.n_groups,
                                                      _ptr(packed.ts_pad), _ptr(packed.te_pad), _ptr(target), float(inv_n), _ptr(pixel),
                                                      _ptr(grad_flat), _ptr(ws), ws.numel(), self._stream(dev)), "afx_train_step_packed_mse")
        return pixel

    def march_train_step_mse(self, prepared, origins, dirs, target, inv_n: float, grad_flat, prec: str, scene_aabb, near_plane, far_plane,
                             step: float, early_stop_eps: float, alpha_thre: float, grid_bits=None, grid_aabb=None, grid_res=None):
        """afx_march_train_step_mse: the reference's grid iteration (march, alpha pass, visibility, packed training step) in one call.
        Returns (pixels [n_rays], n_candidates, n_kept); n_kept == 0: nothing survived, pixels / grad_flat untouched."""
        who = "march_train_step_mse"
        dev = self._model(who, prepared, prec, grad_flat)
        o, d, target = (_buffer(t, name, torch.float32, None, dev, who, copy=True) for t, name in ((origins, "origins"), (dirs, "dirs"), (target, "target")))
        n_rays = o.shape[0]
        if tuple(o.shape) != (n_rays, 3) or tuple(d.shape) != (n_rays, 3) or target.numel() != n_rays:
            raise ValueError("march_train_step_mse: origins/dirs [n_rays,3] and target [n_rays] expected")
        pixel = torch.empty(n_rays, dtype=torch.float32, device=dev)
        a = _lib.MarchTrainArgs()
        _fill_march_args(a.march, o, d, scene_aabb, near_plane, far_plane, step, grid_bits, grid_aabb, grid_res, dev, who)
        _on_gpu(prepared, "prepared", who)
        a.early_stop_eps, a.alpha_thre, a.inv_n = float(early_stop_eps), float(alpha_thre), float(inv_n)
        a.target, a.pixel, a.grad_flat = target.data_ptr(), pixel.data_ptr(), grad_flat.data_ptr()
        need = max(64 << 20, self._ws.numel() if self._ws is not None and self._ws.device == dev else 0)
        for _ in range(4):
            if need > self.max_workspace_bytes:
                raise AfxError(f"march_train_step_mse: the iteration needs a {need >> 20} MiB workspace (max_workspace_bytes = "
                               f"{self.max_workspace_bytes >> 20} MiB)")
            ws = self._workspace(need, dev)
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
            rc = self.lib.afx_march_train_step_mse(self.h, _lib.PREC[prec], _ptr(prepared), C.byref(a), self._stream(dev))
            if rc == -2 and a.workspace_needed > ws.numel():      # AFX_E_WORKSPACE: sizes are data - grow (25 % head-room) and run the iteration again
                need = int(a.workspace_needed)
                continue
            self._check(rc, "afx_march_train_step_mse")
            self.last_march_counts = (int(a.n_candidates), int(a.n_kept), int(a.n_groups))      # (the group count as well, for comparisons)
            return pixel, int(a.n_candidates), int(a.n_kept)
        raise AfxError("march_train_step_mse: the workspace did not converge")

    def march_train_workspace_bytes(self, prec: str, n_rays: int, max_steps_per_ray: int) -> int:
        """Workspace of afx_march_train_step_mse_capturable: fixed by the ray count and the per-ray step bound (march_max_steps), not by data."""
        nbytes = int(self.lib.afx_march_train_workspace_bytes(self.h, _lib.PREC[prec], int(n_rays), int(max_steps_per_ray)))
        if nbytes < 0:
            raise AfxError(f"afx_march_train_workspace_bytes: {self._last_error()}")
        return nbytes

    def march_single_eval_workspace_bytes(self, prec: str, n_rays: int, max_steps_per_ray: int) -> int:
        """Workspace of afx_march_train_step_mse_single_eval: fixed by the ray count and the per-ray step bound, not by data."""
        nbytes = int(self.lib.afx_march_single_eval_workspace_bytes(self.h, _lib.PREC[prec], int(n_rays), int(max_steps_per_ray)))
        if nbytes < 0:
            raise AfxError(f"afx_march_single_eval_workspace_bytes: {self._last_error()}")
        return nbytes

    def march_train_step_mse_capturable(self, prepared, origins, dirs, target, inv_n: float, grad_flat, prec: str, scene_aabb, near_plane,
                                        far_plane, step: float, early_stop_eps: float, alpha_thre: float, grid_bits=None, grid_aabb=None,
                                        grid_res=None, pixel=None, counts=None, skip=None):
        """afx_march_train_step_mse_capturable: the grid iteration of march_train_step_mse with its sizes on the device - no host read-back,
        so it can be captured into a HIP graph.  The workspace is sized once, from the worst case of the march arguments (every step of every
        ray occupied); a capture never grows it (size it with one eager call first).  Writes pixel [n_rays] (float32), counts [3] (int64:
        candidates, kept samples, groups) and skip [1] (float32: 1.0 when nothing was kept - pixel / grad_flat untouched); pass them to
        reuse static buffers.  Returns (pixel, counts, skip), device tensors only."""
        return self._march_step_device_sizes("afx_march_train_step_mse_capturable", "afx_march_train_workspace_bytes", prepared, origins, dirs,
                                             target, inv_n, grad_flat, prec, scene_aabb, near_plane, far_plane, step, early_stop_eps, alpha_thre,
                                             grid_bits, grid_aabb, grid_res, pixel, counts, skip)

    def march_train_step_mse_single_eval(self, prepared, origins, dirs, target, inv_n: float, grad_flat, prec: str, scene_aabb, near_plane,
                                         far_plane, step: float, early_stop_eps: float, alpha_thre: float, grid_bits=None, grid_aabb=None,
                                         grid_res=None, pixel=None, counts=None, skip=None):
        """afx_march_train_step_mse_single_eval: the grid iteration with ONE evaluation of the model - the training step's forward half over the
        march's candidates doubles as the alpha pass.  Same arguments, buffers and results as march_train_step_mse_capturable (counts[2]: the
        kept samples' groups); graph-capturable likewise.  f16s8, ReLU, no input encoding."""
        return self._march_step_device_sizes("afx_march_train_step_mse_single_eval", "afx_march_single_eval_workspace_bytes", prepared, origins,
                                             dirs, target, inv_n, grad_flat, prec, scene_aabb, near_plane, far_plane, step, early_stop_eps,
                                             alpha_thre, grid_bits, grid_aabb, grid_res, pixel, counts, skip)

    def _march_step_device_sizes(self, fn: str, ws_fn: str, prepared, origins, dirs, target, inv_n, grad_flat, prec, scene_aabb, near_plane,
                                 far_plane, step, early_stop_eps, alpha_thre, grid_bits, grid_aabb, grid_res, pixel, counts, skip):
        who = fn[4:]
        dev = self._model(who, prepared, prec, grad_flat)
        o, d, target = (_buffer(t, name, torch.float32, None, dev, who, copy=True) for t, name in ((origins, "origins"), (dirs, "dirs"), (target, "target")))
        n_rays = o.shape[0]
        if tuple(o.shape) != (n_rays, 3) or tuple(d.shape) != (n_rays, 3) or target.numel() != n_rays:
            raise ValueError(f"{who}: origins/dirs [n_rays,3] and target [n_rays] expected")
        if far_plane is None:
            raise ValueError(f"{who}: the workspace bound needs a far plane")
        pixel = _out(pixel, "pixel", torch.float32, n_rays, dev, who)
        counts = _out(counts, "counts", torch.int64, 3, dev, who)
        skip = _out(skip, "skip", torch.float32, 1, dev, who)
        a = _lib.MarchTrainArgs()
        _fill_march_args(a.march, o, d, scene_aabb, near_plane, far_plane, step, grid_bits, grid_aabb, grid_res, dev, who)
        _on_gpu(prepared, "prepared", who)
        a.early_stop_eps, a.alpha_thre, a.inv_n = float(early_stop_eps), float(alpha_thre), float(inv_n)
        a.target, a.pixel, a.grad_flat = target.data_ptr(), pixel.data_ptr(), grad_flat.data_ptr()
        max_steps = int(self.lib.afx_march_max_steps(C.byref(a.march)))
        if max_steps < 0:
            raise AfxError(f"afx_march_max_steps: {self._last_error()}")
        nbytes = int(getattr(self.lib, ws_fn)(self.h, _lib.PREC[prec], int(n_rays), int(max_steps)))
        if nbytes < 0:
            raise AfxError(f"{ws_fn}: {self._last_error()}")
        if nbytes > self.max_workspace_bytes:
            raise AfxError(f"{who}: {n_rays} rays x {max_steps} steps need a {nbytes >> 20} MiB workspace "
                           f"(max_workspace_bytes = {self.max_workspace_bytes >> 20} MiB)")
        ws = self._workspace(nbytes, dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        self._check(getattr(self.lib, fn)(self.h, _lib.PREC[prec], _ptr(prepared), C.byref(a), _ptr(counts), _ptr(skip), self._stream(dev)), fn)
        return pixel, counts, skip

    def march_render(self, prepared, prec: str, scene_aabb, near_plane, far_plane, step: float, early_stop_eps: float, alpha_thre: float,
                     origins=None, dirs=None, poses=None, width: int = 0, height: int = 0, focal: float = 0.0, ray_id0: int = 0, n_rays=None,
                     grid_bits=None, grid_aabb=None, grid_res=None, binary_thresh=None):
        """afx_march_render: forward-only render through the occupancy grid with one evaluation of the model (march, afx_mlp_infer over the
        candidates, visibility and compositing per ray).  Rays: origins / dirs [R,3], or poses [n_proj,3,4] float64 + width / height / focal
        (ray r = ray_id0 + r of [n_proj, H, W]; n_rays defaults to the rest of the table).  The rays are split into calls whose worst case
        (every step of every ray a candidate) fits max_workspace_bytes and afx_mlp_infer's 2^31 - 256 points; each ray's result depends on
        that ray alone, so the split changes nothing.  One host read-back per call.
        Returns (pixel [R], binary_pixel [R] or None, kept_counts int32 [R], n_candidates)."""
        dev = self._model("march_render", prepared, prec)
        pose = poses is not None
        if pose:
            poses = _buffer(poses[:, :3, :], "poses", torch.float64, None, dev, "march_render", copy=True)
            n_rays = ray_window("march_render", poses.shape[0], width, height, ray_id0, n_rays)
            o = d = None
        else:
            o = _buffer(origins, "origins", torch.float32, None, dev, "march_render", copy=True)
            d = _buffer(dirs, "dirs", torch.float32, None, dev, "march_render", copy=True)
            n_rays = o.shape[0]
            if tuple(o.shape) != (n_rays, 3) or tuple(d.shape) != (n_rays, 3):
                raise ValueError("march_render: origins/dirs [n_rays,3] expected")
        n_rays = int(n_rays)
        if far_plane is None:
            raise ValueError("march_render: the workspace bound needs a far plane")
        a = _lib.MarchRenderArgs()
        _fill_march_args(a.march, None, None, scene_aabb, near_plane, far_plane, step, grid_bits, grid_aabb, grid_res, dev, "march_render")
        _on_gpu(prepared, "prepared", "march_render")
        mode = _lib.RAYS_POSE if pose else _lib.RAYS_ARRAYS
        a.ray_mode = mode
        if pose:
            a.poses, a.width, a.height, a.focal = poses.data_ptr(), int(width), int(height), float(focal)
        a.early_stop_eps, a.alpha_thre = float(early_stop_eps), float(alpha_thre)
        a.binary_thresh = float(binary_thresh) if binary_thresh is not None else 0.0
        pixel = torch.empty(n_rays, dtype=torch.float32, device=dev)
        binary = torch.empty(n_rays, dtype=torch.float32, device=dev) if binary_thresh is not None else None
        kept = torch.empty(n_rays, dtype=torch.int32, device=dev)
        if n_rays == 0:
            return pixel, binary, kept, 0
        max_steps = int(self.lib.afx_march_max_steps(C.byref(a.march)))
        if max_steps < 0:
            raise AfxError(f"afx_march_max_steps: {self._last_error()}")

        def ws_bytes(r):
            nb = int(self.lib.afx_march_render_workspace_bytes(mode, int(r), max_steps))
            if nb < 0:
                raise AfxError(f"afx_march_render_workspace_bytes: {self._last_error()}")
            return nb
        chunk = min(n_rays, ((1 << 31) - 256) // max(max_steps, 1))
        while ws_bytes(chunk) > self.max_workspace_bytes:
            if chunk == 1:
                raise AfxError(f"march_render: one ray of {max_steps} steps needs a {ws_bytes(1) >> 20} MiB workspace (max_workspace_bytes = "
                               f"{self.max_workspace_bytes >> 20} MiB)")
            chunk = max(1, min(chunk - 1, chunk * self.max_workspace_bytes // ws_bytes(chunk)))
        ws = self._workspace(ws_bytes(chunk), dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        n_candidates = 0
        for r0 in range(0, n_rays, chunk):
            r1 = min(n_rays, r0 + chunk)
            if pose:
                a.ray_id0, a.n_rays = int(ray_id0) + r0, r1 - r0
            else:
                a.march.origins, a.march.dirs, a.march.n_rays = o[r0:r1].data_ptr(), d[r0:r1].data_ptr(), r1 - r0
            a.pixel, a.kept_counts = pixel[r0:r1].data_ptr(), kept[r0:r1].data_ptr()
            a.binary_pixel = binary[r0:r1].data_ptr() if binary is not None else None
            self._check(self.lib.afx_march_render(self.h, _lib.PREC[prec], _ptr(prepared), C.byref(a), self._stream(dev)), "afx_march_render")
            n_candidates += int(a.n_candidates)
        return pixel, binary, kept, n_candidates

    def hier_train_step_mse(self, prepared, spec: RenderSpec, n_fine: int, u, target, inv_n: float, grad_flat, prec: str, want_z_all=True):
        """afx_hier_train_step_mse: hierarchical step with coarse re-use; `spec` carries the rays and the COARSE depths (mode 'dense').
        Returns (pixels [R], merged depths [R, S + n_fine] | None)."""
        who = "hier_train_step_mse"
        dev = self._model(who, prepared, prec, grad_flat)
        target = _buffer(target, "target", torch.float32, spec.n_rays, dev, who, copy=True)
        u = _buffer(u, "u", torch.float32, (spec.n_rays, int(n_fine)), dev, who, exact_shape=True, copy=True)
        pixel = torch.empty(spec.n_rays, dtype=torch.float32, device=dev)
        z_all = torch.empty(spec.n_rays, spec.n_samples + int(n_fine), dtype=torch.float32, device=dev) if want_z_all else None
        a, keep = self._render_args(spec, dev, pixel)
        _on_gpu(prepared, "prepared", who)
        full = int(self.lib.afx_hier_workspace_bytes(self.h, spec.n_rays, spec.n_samples, int(n_fine)))
        ws = self._workspace(min(full, self.max_workspace_bytes), dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        self._check(self.lib.afx_hier_train_step_mse(self.h, _lib.PREC[prec], _ptr(prepared), C.byref(a), int(n_fine), _ptr(u), _ptr(target),
                                                    float(inv_n), _ptr(z_all), _ptr(grad_flat), self._stream(dev)), "afx_hier_train_step_mse")
        del keep
        return pixel, z_all

    def fused_step_available(self, n_samples: int, prec: str) -> bool:
        """afx_train_step_mse takes this ray length at this precision: rays that fit a 256-sample workgroup tile always (one
        kernel per chunk); any other length (300, 128 + 64, ...) as two half-kernels per chunk with the 8-bit-stash kernel
        (include/afx.h)."""
        s_pad = (int(n_samples) + 31) // 32 * 32
        return 256 % s_pad == 0 or (prec == "f16s8" and os.environ.get("AFX_SMALL_IN_KERNEL", "1") != "0"
                                    and os.environ.get("AFX_NO_SPLIT", "0") == "0")      # (AFX_NO_SPLIT=1: A/B against the two-launch path)

    def train_step_mse(self, prepared, spec: RenderSpec, target, inv_n: float, grad_flat, prec: str):
        """Fused forward + MSE + backward (afx_train_step_mse); returns the rendered pixels."""
        dev = self._model("train_step_mse", prepared, prec, grad_flat)
        target = _buffer(target, "target", torch.float32, spec.n_rays, dev, "train_step_mse", copy=True)
        pixel = torch.empty(spec.n_rays, dtype=torch.float32, device=dev)
        a, keep = self._render_args(spec, dev, pixel)
        _on_gpu(prepared, "prepared", "train_step_mse")
        full = int(self.lib.afx_query(self.h, _lib.Q_BWD_WORKSPACE_FULL, spec.n_rays, spec.n_samples, _lib.PREC[prec]))
        ws = self._workspace(min(full, self.max_workspace_bytes), dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        self._check(self.lib.afx_train_step_mse(self.h, _lib.PREC[prec], _ptr(prepared), C.byref(a), _ptr(target),
                                               float(inv_n), _ptr(grad_flat), self._stream(dev)), "afx_train_step_mse")
        del keep
        return pixel


# ---- packed samples of the occupancy-grid march, group-aligned for the fused packed training step
class PackedGroups:
    """A packed, ray-sorted sample list re-laid out for the fused packed training step (afx_pack_groups): every ray starts on a
    32-sample group (`group_offsets` int64 [R+1] in groups), dead padding behind a ray's last sample, `group_ray` int32 [n_groups]."""

    def __init__(self, n_rays, n_groups, group_offsets, group_ray, ts_pad, te_pad):
        self.n_rays, self.n_groups = int(n_rays), int(n_groups)
        self.group_offsets, self.group_ray, self.ts_pad, self.te_pad = group_offsets, group_ray, ts_pad, te_pad


def pack_groups(offsets, t_starts, t_ends, n_groups=None, group_offsets=None) -> PackedGroups:
    """offsets int64 [R+1] (exclusive scan of the per-ray sample counts), t_starts / t_ends [n] -> PackedGroups."""
    lib = _lib.load()
    dev = offsets.device
    n_rays = _buffer(offsets, "offsets", torch.int64, None, dev, "pack_groups").numel() - 1
    if group_offsets is not None:
        _buffer(group_offsets, "group_offsets", torch.int64, n_rays + 1, dev, "pack_groups")
    ts = _buffer(t_starts.reshape(-1), "t_starts", torch.float32, None, dev, "pack_groups", copy=True)
    te = _buffer(t_ends.reshape(-1), "t_ends", torch.float32, ts.numel(), dev, "pack_groups", copy=True)
    _on_gpu(offsets, "offsets", "pack_groups")
    if group_offsets is None:
        cnt = offsets[1:] - offsets[:-1]
        group_offsets = torch.zeros(n_rays + 1, dtype=torch.int64, device=dev)
        torch.cumsum((cnt + 31) // 32, 0, out=group_offsets[1:])
    if n_groups is None:
        n_groups = int(group_offsets[-1])
    ts_pad = torch.empty(n_groups * 32, device=dev)
    te_pad = torch.empty(n_groups * 32, device=dev)
    group_ray = torch.empty(n_groups, dtype=torch.int32, device=dev)
    if n_groups:
        _lib.check(lib.afx_pack_groups(_ptr(offsets), _ptr(group_offsets), n_rays, _ptr(ts), _ptr(te), _ptr(ts_pad), _ptr(te_pad),
                                       _ptr(group_ray), Engine._stream(dev)), "afx_pack_groups")
    return PackedGroups(n_rays, n_groups, group_offsets, group_ray, ts_pad, te_pad)


# ---- stand-alone compositing / sampling kernels (no model) -----------------------------------
def composite_dense(raw, dirs, z, want_aux=True):
    """afx_composite_dense: raw [R,S], dirs [R,3], z [S] or [R,S] -> (rgb [R], depth [R], weights [R,S], entropy [R], sigma [R,S])."""
    lib = _lib.load()
    dev, who = raw.device, "composite_dense"
    raw = _buffer(raw, "raw", torch.float32, None, dev, who, copy=True)
    r, s = raw.shape
    dirs = _buffer(dirs, "dirs", torch.float32, (r, 3), dev, who, exact_shape=True, copy=True)
    z = _buffer(z, "z", torch.float32, (r, s) if z.dim() == 2 else (s,), dev, who, exact_shape=True, copy=True)
    _on_gpu(raw, "raw", who)
    rgb = torch.empty(r, device=dev)
    depth = torch.empty(r, device=dev) if want_aux else None
    w = torch.empty(r, s, device=dev) if want_aux else None
    ent = torch.empty(r, device=dev) if want_aux else None
    sig = torch.empty(r, s, device=dev) if want_aux else None
    _lib.check(lib.afx_composite_dense(_ptr(raw), _ptr(dirs), _ptr(z), int(z.dim() == 2), r, s, _ptr(rgb), _ptr(depth),
                                       _ptr(w), _ptr(ent), _ptr(sig), Engine._stream(dev)), "afx_composite_dense")
    return rgb, depth, w, ent, sig


def composite_dense_backward(raw, dirs, z, rgb, d_rgb):
    lib = _lib.load()
    dev, who = raw.device, "composite_dense_backward"
    raw = _buffer(raw, "raw", torch.float32, None, dev, who, copy=True)
    r, s = raw.shape
    dirs = _buffer(dirs, "dirs", torch.float32, (r, 3), dev, who, exact_shape=True, copy=True)
    z = _buffer(z, "z", torch.float32, (r, s) if z.dim() == 2 else (s,), dev, who, exact_shape=True, copy=True)
    rgb, d_rgb = _buffer(rgb, "rgb", torch.float32, r, dev, who, copy=True), _buffer(d_rgb, "d_rgb", torch.float32, r, dev, who, copy=True)
    _on_gpu(raw, "raw", who)
    d_raw = torch.empty_like(raw)
    _lib.check(lib.afx_composite_dense_backward(_ptr(raw), _ptr(dirs), _ptr(z), int(z.dim() == 2), r, s, _ptr(rgb), _ptr(d_rgb), _ptr(d_raw),
                                                Engine._stream(dev)), "afx_composite_dense_backward")
    return d_raw


def composite_packed(pred, ray_indices, t_starts, t_ends, n_rays):
    """afx_composite_packed: pred[n] (before the sigmoid), ray_indices[n] int32 ascending, t_starts / t_ends [n] -> rgb_map[n_rays].
    Nothing is converted: an int64 ray_indices or a float64 t_starts would otherwise be read as something else."""
    lib = _lib.load()
    dev, who, n_rays = getattr(pred, "device", None), "composite_packed", int(n_rays)
    pred = _buffer(pred, "pred", torch.float32, None, dev, who, copy=True)
    n = pred.numel()
    ts, te = _buffer(t_starts, "t_starts", torch.float32, n, dev, who, copy=True), _buffer(t_ends, "t_ends", torch.float32, n, dev, who, copy=True)
    _buffer(ray_indices, "ray_indices", torch.int32, n, dev, who)
    _on_gpu(pred, "pred", who)
    rgb = torch.empty(n_rays, device=dev)
    _lib.check(lib.afx_composite_packed(_ptr(pred), _ptr(ray_indices), _ptr(ts), _ptr(te), n, n_rays,
                                        _ptr(rgb), Engine._stream(dev)), "afx_composite_packed")
    return rgb


def composite_packed_backward(pred, ray_indices, t_starts, t_ends, n_rays, rgb, d_rgb):
    """afx_composite_packed_backward: rgb = composite_packed's result, d_rgb[n_rays] -> d_pred, in pred's shape."""
    lib = _lib.load()
    dev, who, n_rays = getattr(pred, "device", None), "composite_packed_backward", int(n_rays)
    flat = _buffer(pred, "pred", torch.float32, None, dev, who, copy=True)
    n = flat.numel()
    ts, te = _buffer(t_starts, "t_starts", torch.float32, n, dev, who, copy=True), _buffer(t_ends, "t_ends", torch.float32, n, dev, who, copy=True)
    rgb, d_rgb = _buffer(rgb, "rgb", torch.float32, n_rays, dev, who, copy=True), _buffer(d_rgb, "d_rgb", torch.float32, n_rays, dev, who, copy=True)
    _buffer(ray_indices, "ray_indices", torch.int32, n, dev, who)
    _on_gpu(flat, "pred", who)
    d_pred = torch.empty(pred.shape, device=dev)
    _lib.check(lib.afx_composite_packed_backward(_ptr(flat), _ptr(ray_indices), _ptr(ts), _ptr(te), n,
                                                 n_rays, _ptr(rgb), _ptr(d_rgb), _ptr(d_pred),
                                                 Engine._stream(dev)), "afx_composite_packed_backward")
    return d_pred


# ---- per-ray entropy of the density profile (get_ray_entropy) with its gradient ---------------
def ray_entropy_packed(pred, ray_indices, rgb_map, n_rays, threshold=0.4):
    """afx_ray_entropy_packed: pred[n] (before the sigmoid), ray_indices[n] int32 ascending, rgb_map[n_rays] -> (entropy[n_rays],
    ray_sums[n_rays,2] for ray_entropy_packed_backward)."""
    lib = _lib.load()
    dev, who, n_rays = getattr(pred, "device", None), "ray_entropy_packed", int(n_rays)
    pred = _buffer(pred, "pred", torch.float32, None, dev, who, copy=True)
    ri = _buffer(ray_indices, "ray_indices", torch.int32, pred.numel(), dev, who, copy=True)
    rgb_map = _buffer(rgb_map, "rgb_map", torch.float32, n_rays, dev, who, copy=True)
    _on_gpu(pred, "pred", who)
    ent = torch.empty(n_rays, device=dev)
    sums = torch.empty(n_rays, 2, device=dev)
    _lib.check(lib.afx_ray_entropy_packed(_ptr(pred), _ptr(ri), pred.numel(), _ptr(rgb_map), n_rays, float(threshold), _ptr(ent), _ptr(sums),
                                          Engine._stream(dev)), "afx_ray_entropy_packed")
    return ent, sums


def ray_entropy_packed_backward(pred, ray_indices, rgb_map, ray_sums, d_entropy, threshold=0.4, out=None):
    """afx_ray_entropy_packed_backward -> d_pred[n].  `out`: a gradient buffer the result is ADDED to (the accumulate flag), e.g. the one
    composite_packed_backward returned; without it a new tensor is written."""
    lib = _lib.load()
    dev, who = getattr(pred, "device", None), "ray_entropy_packed_backward"
    pred = _buffer(pred, "pred", torch.float32, None, dev, who, copy=True).reshape(-1)
    ri = _buffer(ray_indices, "ray_indices", torch.int32, pred.numel(), dev, who, copy=True)
    rgb_map = _buffer(rgb_map, "rgb_map", torch.float32, None, dev, who, copy=True)
    ray_sums = _buffer(ray_sums, "ray_sums", torch.float32, (rgb_map.numel(), 2), dev, who, exact_shape=True, copy=True)
    d_entropy = _buffer(d_entropy, "d_entropy", torch.float32, rgb_map.numel(), dev, who, copy=True)
    if out is not None:
        _buffer(out, "out", torch.float32, pred.numel(), dev, who)
    _on_gpu(pred, "pred", who)
    d_pred = torch.empty_like(pred) if out is None else out
    _lib.check(lib.afx_ray_entropy_packed_backward(_ptr(pred), _ptr(ri), pred.numel(), _ptr(rgb_map), float(threshold), _ptr(ray_sums),
                                                   _ptr(d_entropy), int(out is not None), _ptr(d_pred), Engine._stream(dev)),
               "afx_ray_entropy_packed_backward")
    return d_pred


def ray_entropy_dense(raw, rgb_map, threshold=0.4):
    """afx_ray_entropy_dense: raw[R,S] (before the sigmoid), rgb_map[R] -> (entropy[R], ray_sums[R,2])."""
    lib = _lib.load()
    dev, who = getattr(raw, "device", None), "ray_entropy_dense"
    raw = _buffer(raw, "raw", torch.float32, None, dev, who, copy=True)
    if raw.dim() != 2 or raw.shape[1] < 1:
        raise ValueError("ray_entropy_dense: expected raw[R,S] with S >= 1 and rgb_map[R]")
    r, s = raw.shape
    rgb_map = _buffer(rgb_map, "rgb_map", torch.float32, r, dev, who, copy=True)
    _on_gpu(raw, "raw", who)
    ent = torch.empty(r, device=dev)
    sums = torch.empty(r, 2, device=dev)
    _lib.check(lib.afx_ray_entropy_dense(_ptr(raw), r, s, _ptr(rgb_map), float(threshold), _ptr(ent), _ptr(sums), Engine._stream(dev)),
               "afx_ray_entropy_dense")
    return ent, sums


def ray_entropy_dense_backward(raw, rgb_map, ray_sums, d_entropy, threshold=0.4, out=None):
    """afx_ray_entropy_dense_backward -> d_raw[R,S]; `out` as in ray_entropy_packed_backward."""
    lib = _lib.load()
    dev, who = getattr(raw, "device", None), "ray_entropy_dense_backward"
    raw = _buffer(raw, "raw", torch.float32, None, dev, who, copy=True)
    if raw.dim() != 2 or raw.shape[1] < 1:
        raise ValueError("ray_entropy_dense_backward: expected raw[R,S], rgb_map[R], ray_sums[R,2], d_entropy[R]")
    r, s = raw.shape
    rgb_map = _buffer(rgb_map, "rgb_map", torch.float32, r, dev, who, copy=True)
    ray_sums = _buffer(ray_sums, "ray_sums", torch.float32, (r, 2), dev, who, exact_shape=True, copy=True)
    d_entropy = _buffer(d_entropy, "d_entropy", torch.float32, r, dev, who, copy=True)
    d_raw = _out(out, "out", torch.float32, (r, s), dev, who, exact_shape=True)
    _on_gpu(raw, "raw", who)
    _lib.check(lib.afx_ray_entropy_dense_backward(_ptr(raw), r, s, _ptr(rgb_map), float(threshold), _ptr(ray_sums), _ptr(d_entropy),
                                                  int(out is not None), _ptr(d_raw), Engine._stream(dev)), "afx_ray_entropy_dense_backward")
    return d_raw


def project_volume(vol, origin, spacing, fill_value, depth_values, origins=None, dirs=None, poses=None, width=0, height=0,
                   focal=0.0, ray_ids=None, ray_id0=0, n_rays=None, type_ct=True):
    """afx_project_volume: X-ray projection of a voxel volume (trilinear lookup) along rays -> pixel[R].  Rays: origins / dirs [R,3]
    float32, or poses [n_proj,3 or 4,4] + width / height / focal, generated in fp64 in the kernel: the rays `ray_ids` (any integer tensor)
    of the [n_proj, H, W] table, or ray_id0 .. ray_id0 + n_rays of it (n_rays defaults to the rest).  Rays outside the table raise."""
    lib = _lib.load()
    dev, who = vol.device, "project_volume"
    vol = _buffer(vol, "volume", torch.float32, None, dev, who, copy=True)
    if vol.dim() != 3:
        raise ValueError("volume: expected [nx,ny,nz]")
    z = _buffer(depth_values, "depth_values", torch.float32, None, dev, who, copy=True)
    a = RenderArgs()
    keep = [vol, z]
    if poses is not None:
        if poses.dim() != 3 or poses.shape[1] < 3 or poses.shape[2] != 4:
            raise ValueError(f"project_volume: poses: expected [n_proj, 3 or 4, 4], got {tuple(poses.shape)}")
        n = ray_window("project_volume", poses.shape[0], width, height, ray_id0, n_rays, ray_ids)
        poses = poses[:, :3, :].to(dev, torch.float64).contiguous().reshape(-1, 12)
        keep.append(poses)
        a.ray_mode, a.poses = _lib.RAYS_POSE, poses.data_ptr()
        if ray_ids is not None:
            if poses.shape[0] * int(width) * int(height) > 2 ** 31 - 1:
                raise ValueError("project_volume: ray_ids are int32: the ray table must hold fewer than 2^31 rays")
            ray_ids = ray_ids.reshape(-1).to(dev, torch.int32).contiguous()
            keep.append(ray_ids)
            a.ray_ids = ray_ids.data_ptr()
        a.ray_id0, a.width, a.height, a.focal = int(ray_id0), int(width), int(height), float(focal)
    else:
        o, d = _buffer(origins, "origins", torch.float32, None, dev, who, copy=True), _buffer(dirs, "dirs", torch.float32, None, dev, who, copy=True)
        keep += [o, d]
        n = o.shape[0]
        if tuple(o.shape) != (n, 3) or tuple(d.shape) != (n, 3):
            raise ValueError(f"project_volume: origins/dirs: expected two [n_rays, 3] tensors, got {tuple(o.shape)} and {tuple(d.shape)}")
        a.ray_mode, a.origins, a.dirs = _lib.RAYS_ARRAYS, o.data_ptr(), d.data_ptr()
    _on_gpu(vol, "volume", who)
    pixel = torch.empty(int(n), dtype=torch.float32, device=dev)
    a.n_rays, a.n_samples, a.depth_mode, a.z, a.pixel = int(n), int(z.numel()), _lib.DEPTH_SHARED_Z, z.data_ptr(), pixel.data_ptr()
    org = (C.c_double * 3)(*[float(x) for x in origin])
    spc = (C.c_double * 3)(*[float(x) for x in spacing])
    _lib.check(lib.afx_project_volume(_ptr(vol), vol.shape[0], vol.shape[1], vol.shape[2], org, spc, float(fill_value),
                                      C.byref(a), int(bool(type_ct)), Engine._stream(dev)), "afx_project_volume")
    del keep
    return pixel


def fine_depths(z_coarse, w_coarse, u, fn: str = "afx_fine_depths", name: str = "w_coarse"):
    """afx_fine_depths: z_coarse [S] or [R,S], the coarse pass's weights w_coarse [R,S], the draw u [R,n_fine] -> merged depths [R, S + n_fine]."""
    lib = _lib.load()
    dev, who = w_coarse.device, fn[4:]
    w_coarse = _buffer(w_coarse, name, torch.float32, None, dev, who, copy=True)
    r, s = w_coarse.shape
    z_coarse = _buffer(z_coarse, "z_coarse", torch.float32, (r, s) if z_coarse.dim() == 2 else (s,), dev, who, exact_shape=True, copy=True)
    u = _buffer(u, "u", torch.float32, None, dev, who, copy=True)
    if u.dim() != 2 or u.shape[0] != r:
        raise ValueError(f"{who}: u must have shape [{r}, n_fine], got {tuple(u.shape)}")
    nf = u.shape[1]
    _on_gpu(w_coarse, name, who)
    out = torch.empty(r, s + nf, device=dev)
    _lib.check(getattr(lib, fn)(_ptr(z_coarse), int(z_coarse.dim() == 2), _ptr(w_coarse), _ptr(u), r, s, nf, _ptr(out), Engine._stream(dev)), fn)
    return out


def fine_depths_from_tau(z_coarse, tau_coarse, u):
    """afx_fine_depths_from_tau: merged coarse + fine depths from the coarse pass's per-sample optical depths [R,S]."""
    return fine_depths(z_coarse, tau_coarse, u, "afx_fine_depths_from_tau", "tau_coarse")


# ---- occupancy grid / ray marching / device ray sampler (no model) ---------------------------------------------
def _grid_desc(roi_aabb, resolution) -> "_lib.GridDesc":
    g = _lib.GridDesc()
    for i, v in enumerate([float(x) for x in roi_aabb]):
        g.roi_aabb[i] = v
    for i, v in enumerate([int(x) for x in resolution]):
        g.resolution[i] = v
    return g


def philox_uniform(seed: int, stream_id: int, n: int, device) -> torch.Tensor:
    """n uniform [0,1) numbers of the counter-based stream (seed, stream_id) - the generator of every perf-mode draw."""
    lib = _lib.load()
    out = torch.empty(int(n), dtype=torch.float32, device=device)
    _lib.check(lib.afx_philox_uniform(int(seed), int(stream_id), int(n), _ptr(out), Engine._stream(out.device)), "afx_philox_uniform")
    return out


def _num_cells(resolution) -> int:
    r = [int(x) for x in resolution]
    return r[0] * r[1] * r[2]


def grid_points(roi_aabb, resolution, cell_idx, n, jitter=None, seed=0, stream_id=0, device=None):
    """afx_grid_points: one jittered world point per selected cell -> [n, 3].  cell_idx: None (cells 0 .. n-1) or int32 [n], every index in
    [0, num_cells), unchecked (that would need a device read); jitter: None (the Philox stream (seed, stream_id)) or float32 [n, 3]."""
    lib = _lib.load()
    n, who = int(n), "grid_points"
    if cell_idx is None and jitter is None:
        dev = torch.device(device) if device is not None else None
        if dev is None or dev.type != "cuda":
            raise AfxError("grid_points: the occupancy grid lives on a GPU; there is no CPU path")
    else:
        first = cell_idx if cell_idx is not None else jitter
        dev = getattr(first, "device", None)
        if cell_idx is not None:
            _buffer(cell_idx, "cell_idx", torch.int32, (n,), dev, who, exact_shape=True)
        if jitter is not None:
            _buffer(jitter, "jitter", torch.float32, (n, 3), dev, who, exact_shape=True)
        _on_gpu(first, "cell_idx" if cell_idx is not None else "jitter", who)
        if device is not None and torch.device(device).index not in (None, dev.index):
            raise ValueError(f"grid_points: device {device}, but the tensors are on {dev}")
    g = _grid_desc(roi_aabb, resolution)
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    _lib.check(lib.afx_grid_points(C.byref(g), _ptr(cell_idx), n, _ptr(jitter), int(seed), int(stream_id), _ptr(pts),
                                   Engine._stream(pts.device)), "afx_grid_points")
    return pts


def grid_update(roi_aabb, resolution, occs, cell_idx, occ_new, ema_decay, scratch):
    """afx_grid_update, in place: occs[c] = max(occs[c] * ema_decay, occ_new) over the selected cells.  occs, scratch: float32 [num_cells];
    cell_idx: None (cells 0 .. n-1) or int32 [n], every index in [0, num_cells), unchecked; occ_new: float32, n entries."""
    lib = _lib.load()
    dev, who, nc = getattr(occs, "device", None), "grid_update", _num_cells(resolution)
    _buffer(occs, "occs", torch.float32, nc, dev, who)
    _buffer(scratch, "scratch", torch.float32, nc, dev, who)
    occ_new = _buffer(occ_new, "occ_new", torch.float32, None, dev, who, copy=True)
    n = occ_new.numel()
    if cell_idx is None and n > nc:
        raise ValueError(f"grid_update: occ_new: {n} entries for the first cells of a grid of {nc}")
    if cell_idx is not None:
        _buffer(cell_idx, "cell_idx", torch.int32, (n,), dev, who, exact_shape=True)
    _on_gpu(occs, "occs", who)
    g = _grid_desc(roi_aabb, resolution)
    _lib.check(lib.afx_grid_update(C.byref(g), _ptr(occs), _ptr(scratch), _ptr(cell_idx), n, _ptr(occ_new),
                                   float(ema_decay), Engine._stream(dev)), "afx_grid_update")


def grid_binarize(roi_aabb, resolution, occs, occ_thre, binary_u8, bits, partial_ws):
    """afx_grid_binarize: binary_u8[c] = occs[c] > min(mean(occs), occ_thre) and the march's bitfield.  occs float32 and binary_u8 uint8
    [num_cells], bits int32 [(num_cells + 31) // 32], partial_ws float64, at least 256 entries."""
    lib = _lib.load()
    dev, who, nc = getattr(occs, "device", None), "grid_binarize", _num_cells(resolution)
    _buffer(occs, "occs", torch.float32, nc, dev, who)
    _buffer(binary_u8, "binary_u8", torch.uint8, nc, dev, who)
    _buffer(bits, "bits", torch.int32, (nc + 31) // 32, dev, who)
    _buffer(partial_ws, "partial_ws", torch.float64, 256, dev, who, at_least=True)
    _on_gpu(occs, "occs", who)
    g = _grid_desc(roi_aabb, resolution)
    _lib.check(lib.afx_grid_binarize(C.byref(g), _ptr(occs), float(occ_thre), _ptr(binary_u8), _ptr(bits), _ptr(partial_ws),
                                     Engine._stream(dev)), "afx_grid_binarize")


def grid_pack(roi_aabb, resolution, binary_u8, bits):
    """afx_grid_pack: the march's bitfield from a byte mask (a restored grid).  binary_u8 uint8 [num_cells], bits int32
    [(num_cells + 31) // 32]."""
    lib = _lib.load()
    dev, who, nc = getattr(binary_u8, "device", None), "grid_pack", _num_cells(resolution)
    _buffer(binary_u8, "binary_u8", torch.uint8, nc, dev, who)
    _buffer(bits, "bits", torch.int32, (nc + 31) // 32, dev, who)
    _on_gpu(binary_u8, "binary_u8", who)
    g = _grid_desc(roi_aabb, resolution)
    _lib.check(lib.afx_grid_pack(C.byref(g), _ptr(binary_u8), _ptr(bits), Engine._stream(dev)), "afx_grid_pack")


def _step_args(step, dev, who):
    """(host step, device step pointer) of a training step given as an int or a 0-dim int64 tensor on `dev`."""
    if torch.is_tensor(step):
        if step.device != torch.device(dev) or step.dtype != torch.int64 or step.numel() != 1:
            raise ValueError(f"{who}: a tensor step must be one int64 on {dev}")
        return 0, step.data_ptr()
    return int(step), None


def grid_select_workspace_bytes(roi_aabb, resolution) -> int:
    return int(_lib.load().afx_grid_select_workspace_bytes(C.byref(_grid_desc(roi_aabb, resolution))))


def grid_select_cells(roi_aabb, resolution, bits, n_draw, seed, step, cells=None, count=None, workspace=None):
    """afx_grid_select_cells: the post-warm-up cells of a refresh drawn on the device from the march's bitfield (draw rule: include/afx.h).
    `step`: int or 0-dim int64 device tensor.  Returns (cells [2 n_draw] int32 - valid up to count -, count [1] int64), device tensors."""
    lib = _lib.load()
    dev, who, n_draw = bits.device, "grid_select_cells", int(n_draw)
    g = _grid_desc(roi_aabb, resolution)
    _buffer(bits, "bits", torch.int32, (_num_cells(resolution) + 31) // 32, dev, who)
    cells = _out(cells, "cells", torch.int32, 2 * n_draw, dev, who, ok=n_draw >= 0, at_least=True)
    count = _out(count, "count", torch.int64, 1, dev, who)
    step_h, step_d = _step_args(step, dev, who)
    _on_gpu(bits, "bits", who)
    workspace, nbytes = _scratch(workspace, lib.afx_grid_select_workspace_bytes(C.byref(g)), dev, who)
    _lib.check(lib.afx_grid_select_cells(C.byref(g), _ptr(bits), n_draw, int(seed), step_h, step_d, _ptr(cells), _ptr(count), _ptr(workspace),
                                         nbytes, Engine._stream(dev)), "afx_grid_select_cells")
    return cells, count


def grid_refresh_workspace_bytes(roi_aabb, resolution, n_draw, all_cells) -> int:
    lib = _lib.load()
    n = int(lib.afx_grid_refresh_workspace_bytes(C.byref(_grid_desc(roi_aabb, resolution)), int(n_draw), int(bool(all_cells))))
    if n < 0:
        raise AfxError(f"afx_grid_refresh_workspace_bytes: {lib.afx_last_error().decode()}")
    return n


def grid_refresh(eng: Engine, prepared, prec: str, roi_aabb, resolution, occs, binary_u8, bits, n_draw, all_cells, seed, step, occ_thre,
                 ema_decay, workspace):
    """afx_grid_refresh: one refresh of one grid in place (occs, binary_u8, bits) - cells (all, or the device draw), jittered points,
    sigmoid(MLP) at `prec` on `prepared`, decay / EMA, threshold - with no host synchronisation.  `step`: int or 0-dim int64 device tensor
    (read when the kernels run: a captured call follows it)."""
    dev, who, nc = occs.device, "grid_refresh", _num_cells(resolution)
    _buffer(occs, "occs", torch.float32, nc, dev, who)
    _buffer(binary_u8, "binary_u8", torch.uint8, nc, dev, who)
    _buffer(bits, "bits", torch.int32, (nc + 31) // 32, dev, who)
    eng._model(who, prepared, prec)
    if prepared.device != dev:
        raise ValueError(f"grid_refresh: prepared on {prepared.device}, expected {dev}")
    workspace, nbytes = _scratch(workspace, 0, dev, who)
    _on_gpu(occs, "occs", who)
    a = _lib.GridRefreshArgs()
    a.grid = _grid_desc(roi_aabb, resolution)
    a.occs, a.binary, a.bits = occs.data_ptr(), binary_u8.data_ptr(), bits.data_ptr()
    a.all_cells, a.n_draw, a.seed = int(bool(all_cells)), int(n_draw), int(seed)
    a.step, a.step_dev = _step_args(step, dev, who)
    a.occ_thre, a.ema_decay = float(occ_thre), float(ema_decay)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), nbytes
    eng._check(eng.lib.afx_grid_refresh(eng.h, _lib.PREC[prec], _ptr(prepared), C.byref(a), Engine._stream(dev)), "afx_grid_refresh")


def _fill_march_args(m, o, d, scene_aabb, near_plane, far_plane, step, grid_bits, grid_aabb, grid_res, dev=None, who="march"):
    if o is not None:      # (None: the rays come from elsewhere - afx_march_render's pose mode)
        m.origins, m.dirs, m.n_rays = o.data_ptr(), d.data_ptr(), o.shape[0]
    if scene_aabb is not None:
        m.has_aabb = 1
        for i, v in enumerate([float(x) for x in scene_aabb]):
            m.scene_aabb[i] = v
    if near_plane is not None:
        m.has_near, m.near_plane = 1, float(near_plane)
    if far_plane is not None:
        m.has_far, m.far_plane = 1, float(far_plane)
    m.step = float(step)
    if grid_bits is not None:
        # k_march_count / k_march_write read grid_bits[cell >> 5] without a check of their own
        if grid_aabb is None or grid_res is None:
            raise ValueError("march: grid_bits needs grid_aabb and grid_res")
        res = [int(x) for x in grid_res]
        if len(res) != 3 or min(res) <= 0 or len(list(grid_aabb)) != 6:
            raise ValueError("march: grid_res must be three positive sizes and grid_aabb six numbers")
        _buffer(grid_bits, "grid_bits", torch.int32, (_num_cells(res) + 31) // 32, dev if dev is not None else o.device, who, at_least=True)
        m.grid_bits = grid_bits.data_ptr()
        m.grid = _grid_desc(grid_aabb, grid_res)


def march(origins, dirs, scene_aabb, near_plane, far_plane, step, grid_bits=None, grid_aabb=None, grid_res=None, want_points=True):
    """Grid-skipping fixed-step march -> packed (ray_indices int32 [n], t_starts [n], t_ends [n], mid-points [n,3] | None,
    offsets int64 [R+1]).  Refused before any launch: rays that are not two equal [R, 3] arrays, a step <= 0, a march that neither a scene
    box nor a far plane bounds, and a grid_bits that is not int32, on another device, without box and resolution, or shorter than the grid."""
    lib = _lib.load()
    dev = origins.device
    o, d = _buffer(origins, "origins", torch.float32, None, dev, "march", copy=True), _buffer(dirs, "dirs", torch.float32, None, dev, "march", copy=True)
    if o.dim() != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError(f"march: origins {tuple(o.shape)} and dirs {tuple(d.shape)}: expected [R, 3] both")
    if not float(step) > 0:
        raise ValueError(f"march: step {step} must be > 0")
    if scene_aabb is None and far_plane is None:
        raise ValueError("march: neither a scene box nor a far plane bounds the rays")
    m = _lib.MarchArgs()
    _fill_march_args(m, o, d, scene_aabb, near_plane, far_plane, step, grid_bits, grid_aabb, grid_res, dev)
    _on_gpu(origins, "origins", "march")
    st = Engine._stream(dev)
    counts = torch.empty(o.shape[0], dtype=torch.int32, device=dev)
    _lib.check(lib.afx_march_count(C.byref(m), _ptr(counts), st), "afx_march_count")
    offsets = torch.empty(o.shape[0] + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.check(lib.afx_ray_offsets(_ptr(counts), o.shape[0], _ptr(offsets), None, _ptr(totals), st), "afx_ray_offsets")
    n = int(totals[0])      # the march's one host read
    ri = torch.empty(n, dtype=torch.int32, device=dev)
    ts, te = torch.empty(n, device=dev), torch.empty(n, device=dev)
    pts = torch.empty(n, 3, device=dev) if want_points else None
    if n > 0:
        _lib.check(lib.afx_march_write(C.byref(m), _ptr(offsets), _ptr(ri), _ptr(ts), _ptr(te), _ptr(pts), st), "afx_march_write")
    return ri, ts, te, pts, offsets


def march_visibility(raw, ts, te, offsets, early_stop_eps, alpha_thre, is_alpha=False, return_offsets=False):
    """nerfacc render_visibility on the candidates' raw MLP outputs -> compacted (ray_indices, t_starts, t_ends).
    raw / ts / te [n] float32, offsets int64 [n_rays + 1] are checked for type, size against each other and device; that offsets is
    ascending with offsets[-1] == n is the caller's to keep (the march's own output does): checking it would cost a host read per call,
    and the kernels index the samples by it."""
    lib = _lib.load()
    dev, who = getattr(raw, "device", None), "march_visibility"
    raw = _buffer(raw, "raw", torch.float32, None, dev, who, copy=True)
    ts, te = _buffer(ts, "ts", torch.float32, raw.numel(), dev, who, copy=True), _buffer(te, "te", torch.float32, raw.numel(), dev, who, copy=True)
    n_rays = _buffer(offsets, "offsets", torch.int64, None, dev, who).numel() - 1
    _on_gpu(raw, "raw", who)
    if n_rays < 0:
        raise AfxError("march_visibility: offsets: expected [n_rays + 1] entries")
    keep = torch.empty(ts.numel(), dtype=torch.uint8, device=dev)
    counts = torch.empty(n_rays, dtype=torch.int32, device=dev)
    st = Engine._stream(dev)
    _lib.check(lib.afx_march_visibility(_ptr(raw), int(bool(is_alpha)), _ptr(ts), _ptr(te), _ptr(offsets), n_rays, float(early_stop_eps),
                                        float(alpha_thre), _ptr(keep), _ptr(counts), st), "afx_march_visibility")
    off2 = torch.empty(n_rays + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    goff = torch.empty(n_rays + 1, dtype=torch.int64, device=dev) if return_offsets == "groups" else None      # (the group-aligned copy's offsets)
    _lib.check(lib.afx_ray_offsets(_ptr(counts), n_rays, _ptr(off2), _ptr(goff), _ptr(totals), st), "afx_ray_offsets")
    n2, n_groups = totals.tolist()      # one host read for both
    ri2 = torch.empty(n2, dtype=torch.int32, device=dev)
    ts2, te2 = torch.empty(n2, device=dev), torch.empty(n2, device=dev)
    if n2 > 0:
        _lib.check(lib.afx_march_compact(_ptr(keep), _ptr(offsets), _ptr(off2), n_rays, _ptr(ts), _ptr(te), _ptr(ri2), _ptr(ts2),
                                         _ptr(te2), st), "afx_march_compact")
    if return_offsets == "groups":
        return ri2, ts2, te2, off2, goff, int(n_groups)
    if return_offsets:
        return ri2, ts2, te2, off2
    return ri2, ts2, te2


def topk_indices(keys: torch.Tensor, k: int) -> torch.Tensor:
    """Indices (int64, ascending) of the k largest keys - afx_topk_indices: radix select, deterministic, no full sort."""
    lib = _lib.load()
    keys = _buffer(keys, "keys", torch.float32, None, keys.device, "topk_indices", copy=True)
    n = keys.numel()
    if not 0 <= k <= n:
        raise ValueError(f"topk_indices: k = {k} outside [0, {n}]")
    _on_gpu(keys, "keys", "topk_indices")
    out = torch.empty(int(k), dtype=torch.int64, device=keys.device)
    if k == 0:
        return out
    ws, nbytes = _scratch(None, lib.afx_topk_workspace_bytes(n), keys.device, "topk_indices")
    _lib.check(lib.afx_topk_indices(_ptr(keys), n, int(k), _ptr(out), _ptr(ws), nbytes, Engine._stream(keys.device)), "afx_topk_indices")
    return out


def _images_f64(x: torch.Tensor, who: str) -> torch.Tensor:
    """[H, W] or [N, H, W] device tensor -> contiguous float64 [N, H, W]."""
    if _on_gpu(x, "the images", who).dim() not in (2, 3):
        raise ValueError(f"{who}: expected [H, W] or [N, H, W], got shape {tuple(x.shape)}")
    x = x if x.dim() == 3 else x[None]
    return x.to(torch.float64).contiguous()


def _sigma_array(sigmas):
    s = [float(v) for v in sigmas]
    return (C.c_double * max(len(s), 1))(*s), len(s)


def frangi(images: torch.Tensor, sigmas=(1, 3, 5, 7, 9), beta: float = 0.5, gamma: float = 15.0, black_ridges: bool = True) -> torch.Tensor:
    """afx_frangi: the Frangi vesselness (scikit-image 0.18.3) of every image of a [N, H, W] (or [H, W]) device tensor, float64 [N, H, W]."""
    lib = _lib.load()
    x = _images_f64(images, "frangi")
    n, h, w = x.shape
    sg, ns = _sigma_array(sigmas)
    out = torch.empty_like(x)
    nbytes = int(lib.afx_frangi_workspace_bytes(n, h, w, ns))
    ws = _scratch(None, nbytes, x.device, "frangi")[0]
    _lib.check(lib.afx_frangi(_ptr(x), n, h, w, sg, ns, float(beta), float(gamma), int(bool(black_ridges)), _ptr(out), _ptr(ws), nbytes, None,
                              Engine._stream(x.device)), "afx_frangi")
    return out


def distance_transform_edt(x: torch.Tensor) -> torch.Tensor:
    """afx_distance_transform_edt: scipy.ndimage.distance_transform_edt of every image (non-zero = foreground), bit for bit, float64."""
    lib = _lib.load()
    x = _images_f64(x, "distance_transform_edt")
    n, h, w = x.shape
    out = torch.empty_like(x)
    nbytes = int(lib.afx_distance_transform_edt_workspace_bytes(n, h, w))
    ws = _scratch(None, nbytes, x.device, "distance_transform_edt")[0]
    _lib.check(lib.afx_distance_transform_edt(_ptr(x), n, h, w, _ptr(out), _ptr(ws), nbytes, None, Engine._stream(x.device)),
               "afx_distance_transform_edt")
    return out


def sampling_weights(images: torch.Tensor, strategy: str = "frangi", binary: bool = True, sigmas=(1, 3, 5, 7, 9), beta: float = 0.5,
                     gamma: float = 15.0):
    """afx_sampling_weights over a [N, H, W] device tensor -> (weights float64 [N, H, W], status int32 [N]).  Reads nothing back (the
    call can be captured in a graph): status[i] != 0 marks an image whose weights are NaN (a flat vesselness or distance transform)."""
    lib = _lib.load()
    if strategy not in _lib.SAMPLING:
        raise ValueError(f"sampling_weights: strategy must be one of {sorted(_lib.SAMPLING)}, got {strategy!r}")
    x = _images_f64(images, "sampling_weights")
    n, h, w = x.shape
    sg, ns = _sigma_array(sigmas) if strategy == "frangi" else _sigma_array(())
    st = _lib.SAMPLING[strategy]
    out = torch.empty_like(x)
    status = torch.empty(n, dtype=torch.int32, device=x.device)
    nbytes = int(lib.afx_sampling_weights_workspace_bytes(st, n, h, w, ns))
    ws = _scratch(None, nbytes, x.device, "sampling_weights")[0]
    _lib.check(lib.afx_sampling_weights(_ptr(x), n, h, w, st, int(bool(binary)), sg, ns, float(beta), float(gamma), _ptr(out), _ptr(status),
                                        _ptr(ws), nbytes, None, Engine._stream(x.device)), "afx_sampling_weights")
    return out, status


def ssim(preds: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """afx_ssim: the SSIM (torchmetrics StructuralSimilarityIndexMeasure(data_range=1.0), computed in fp64) of every pair of two [N, H, W]
    (or [H, W]) device tensors, float64 [N].  All views in one launch sequence; nothing is read back."""
    lib = _lib.load()
    _on_gpu(preds, "preds", "ssim"), _on_gpu(targets, "targets", "ssim")
    if preds.shape != targets.shape or preds.dim() not in (2, 3):
        raise ValueError(f"ssim: expected two [H, W] or [N, H, W] tensors of one shape, got {tuple(preds.shape)} and {tuple(targets.shape)}")
    if preds.device != targets.device:
        raise ValueError(f"ssim: preds on {preds.device}, targets on {targets.device}")
    x = (preds if preds.dim() == 3 else preds[None]).to(torch.float32).contiguous()
    y = (targets if targets.dim() == 3 else targets[None]).to(torch.float32).contiguous()
    n, h, w = x.shape
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    nbytes = int(lib.afx_ssim_workspace_bytes(n, h, w))
    ws = _scratch(None, nbytes, x.device, "ssim")[0]
    _lib.check(lib.afx_ssim(_ptr(x), _ptr(y), n, h, w, _ptr(out), _ptr(ws), nbytes, None, Engine._stream(x.device)), "afx_ssim")
    return out


def volume_grid(volume_values: torch.Tensor, origin, spacing, fill, lo: float, hi: float, n: int) -> torch.Tensor:
    """afx_volume_grid: a voxel volume [nx, ny, nz] (trilinear, `fill` outside; what VoxelVolume stands for) sampled at
    np.meshgrid(t, t, t), t = np.linspace(lo, hi, n) rounded to fp32 - float32 [n, n, n], grid[i, j, k] = mu(t[j], t[i], t[k])."""
    lib = _lib.load()
    dev = _on_gpu(volume_values, "the volume", "volume_grid").device
    vol = _buffer(volume_values, "volume", torch.float32, None, dev, "volume_grid", copy=True)
    if vol.dim() != 3:
        raise ValueError("volume: expected [nx,ny,nz]")
    n = int(n)
    out = _out(None, "out", torch.float32, (n,) * 3, dev, "volume_grid", ok=2 <= n <= 1 << 20)
    org = (C.c_double * 3)(*[float(x) for x in origin])
    spc = (C.c_double * 3)(*[float(x) for x in spacing])
    _lib.check(lib.afx_volume_grid(_ptr(vol), vol.shape[0], vol.shape[1], vol.shape[2], org, spc, float(fill), float(lo), float(hi), n,
                                   _ptr(out), Engine._stream(dev)), "afx_volume_grid")
    return out


def _volume_on_gpu(x, name: str, who: str) -> None:
    if _on_gpu(x, name, who).dim() != 3:
        raise ValueError(f"{who}: {name} must have shape [n0, n1, n2], got {tuple(x.shape)}")


def distance_transform_edt_3d(x: torch.Tensor, return_squared: bool = False):
    """afx_distance_transform_edt_3d: the exact Euclidean distance transform of a [n0, n1, n2] device tensor (non-zero = foreground) -
    float64 [n0, n1, n2], the distance in voxels from every voxel to the nearest zero voxel: scipy.ndimage.distance_transform_edt bit for
    bit; +inf everywhere when there is no zero voxel.  return_squared: (distances, the exact integer squared distances as int64,
    0xffffffff for 'no zero voxel')."""
    lib = _lib.load()
    _volume_on_gpu(x, "the volume", "distance_transform_edt_3d")
    fg = (x != 0).to(torch.uint8).contiguous()
    n0, n1, n2 = fg.shape
    nbytes = int(lib.afx_distance_transform_edt_3d_workspace_bytes(n0, n1, n2))      # (0: a shape the library refuses)
    d2 = _out(None, "d2", torch.int32, fg.shape, fg.device, "distance_transform_edt_3d", ok=nbytes > 0)
    dist = _out(None, "dist", torch.float64, fg.shape, fg.device, "distance_transform_edt_3d", ok=nbytes > 0)
    ws = _scratch(None, nbytes, fg.device, "distance_transform_edt_3d")[0]
    _lib.check(lib.afx_distance_transform_edt_3d(_ptr(fg), n0, n1, n2, _ptr(d2), _ptr(dist), _ptr(ws), nbytes, None, Engine._stream(fg.device)),
               "afx_distance_transform_edt_3d")
    if not return_squared:
        return dist
    return dist, d2.to(torch.int64) & 0xffffffff      # the library's uint32 (held in an int32 tensor) as int64


SURFACE_RECORD_SLOTS = 16


def surface_metrics_record(pred: torch.Tensor, gt: torch.Tensor, thr_pred: float, thr_gt: float, q: float = 95.0, record=None,
                           workspace=None) -> torch.Tensor:
    """afx_surface_metrics_3d: the 16-slot device record (int64 tensor; layout in include/afx.h) of two float32 [n0, n1, n2] device
    volumes.  Launches only - nothing is read back, so the call can be captured in a graph (pass `record` and `workspace`, the latter of
    afx_surface_metrics_3d_workspace_bytes bytes, to keep the capture free of allocations)."""
    lib = _lib.load()
    _volume_on_gpu(pred, "pred", "surface_metrics_3d")
    _volume_on_gpu(gt, "gt", "surface_metrics_3d")
    if pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError(f"surface_metrics_3d: pred {tuple(pred.shape)} on {pred.device}, gt {tuple(gt.shape)} on {gt.device}")
    dev = pred.device
    p, g = (_buffer(t, name, torch.float32, None, dev, "surface_metrics_3d", copy=True) for t, name in ((pred, "pred"), (gt, "gt")))
    n0, n1, n2 = p.shape
    record = _out(record, "record", torch.int64, SURFACE_RECORD_SLOTS, dev, "surface_metrics_3d")
    workspace, nbytes = _scratch(workspace, lib.afx_surface_metrics_3d_workspace_bytes(n0, n1, n2), dev, "surface_metrics_3d")
    _lib.check(lib.afx_surface_metrics_3d(_ptr(p), _ptr(g), n0, n1, n2, float(thr_pred), float(thr_gt), float(q), _ptr(record), _ptr(workspace),
                                          nbytes, None, Engine._stream(dev)), "afx_surface_metrics_3d")
    return record


def _lerp(a: float, b: float, t: float) -> float:
    """numpy.lib._function_base_impl._lerp for scalars: a + (b - a) t, taken from b's side once t >= 0.5."""
    diff = b - a
    return b - diff * (1.0 - t) if t >= 0.5 else a + diff * t


def surface_metrics_3d(pred: torch.Tensor, gt: torch.Tensor, thr_pred: float, thr_gt: float, q: float = 95.0) -> dict:
    """The surface-distance scores of A = pred >= thr_pred against B = gt >= thr_gt, in voxel units (medpy.metric.binary dc, assd, hd and
    hd95 at unit spacing; definitions in include/afx.h): dice_vessel = 2 |A & B| / (|A| + |B|), assd = (mean D_A->B + mean D_B->A) / 2,
    hd = the largest surface distance of either direction, hd_percentile = np.percentile(D_A->B + D_B->A, q) - the two order statistics
    come from the device, NumPy's linear interpolation between them is finished here - and the counts n_pred, n_gt, n_overlap,
    n_surface_pred, n_surface_gt.  One launch sequence and one read-back of 128 bytes.  ValueError: a threshold that leaves a volume
    empty (no surface to measure from)."""
    return _surface_scores_from_record(surface_metrics_record(pred, gt, thr_pred, thr_gt, q), q)


def _surface_scores_from_record(record: torch.Tensor, q: float = 95.0) -> dict:
    """The scores of `surface_metrics_3d` from the 16-slot record of `surface_metrics_record` (one read-back of 128 bytes)."""
    import math
    import numpy as np
    rec = record.cpu().numpy()
    f = rec.view(np.float64)
    status = int(rec[12])
    if status:
        empty = [name for bit, name in ((1, "pred"), (2, "gt")) if status & bit]
        raise ValueError(f"surface_metrics_3d: no voxel of {' or '.join(empty)} reaches its threshold: an empty volume has no surface distances")
    n_a, n_b, n_ab, s_a, s_b = (int(v) for v in rec[:5])
    v = float(f[11])
    lo, hi = math.sqrt(float(rec[9])), math.sqrt(float(rec[10]))
    return {"dice_vessel": 2.0 * n_ab / (n_a + n_b), "assd": (float(f[5]) / s_a + float(f[6]) / s_b) / 2.0,
            "hd": math.sqrt(float(max(rec[7], rec[8]))), "hd_percentile": _lerp(lo, hi, v - math.floor(v)), "q": float(q),
            "n_pred": n_a, "n_gt": n_b, "n_overlap": n_ab, "n_surface_pred": s_a, "n_surface_gt": s_b}


COMPONENTS_RECORD_SLOTS = 8


def components_record(x: torch.Tensor, connectivity: int = 1, labels=None, sizes=None, record=None, workspace=None):
    """afx_label_components_3d on a contiguous uint8 [n0, n1, n2] device mask (non-zero = foreground) -> (labels, sizes, record):
    labels int32 [n0, n1, n2] (0 = background, 1..K in scipy.ndimage.label's order), sizes an int32 tensor of n0 n1 n2 entries holding
    the library's uint32 counts (sizes[l - 1] = the voxels of component l, 0 from K on), record the 8-slot int64 device record (layout
    in include/afx.h: foreground voxels, K, the largest component's size, label and first voxel).  Launches only - nothing is read
    back, so the call can be captured in a graph (pass all four buffers, the workspace of afx_label_components_3d_workspace_bytes
    bytes, to keep the capture free of allocations)."""
    lib = _lib.load()
    _volume_on_gpu(x, "the mask", "label_components_3d")
    dev, who = x.device, "components_record"
    _buffer(x, "the mask", torch.uint8, x.shape, dev, who)
    n0, n1, n2 = x.shape
    nbytes = int(lib.afx_label_components_3d_workspace_bytes(n0, n1, n2))      # (0: a shape the library refuses)
    labels = _out(labels, "labels", torch.int32, x.shape, dev, who, ok=nbytes > 0)
    sizes = _out(sizes, "sizes", torch.int32, x.numel(), dev, who, ok=nbytes > 0)
    record = _out(record, "record", torch.int64, COMPONENTS_RECORD_SLOTS, dev, who)
    workspace, nbytes = _scratch(workspace, nbytes, dev, who)
    _lib.check(lib.afx_label_components_3d(_ptr(x), n0, n1, n2, int(connectivity), _ptr(labels), _ptr(sizes), _ptr(record), _ptr(workspace),
                                           nbytes, None, Engine._stream(dev)), "afx_label_components_3d")
    return labels, sizes, record


def label_components_3d(x: torch.Tensor, connectivity: int = 1, return_sizes: bool = False):
    """The connected components of a [n0, n1, n2] device tensor (any dtype, non-zero = foreground; connectivity 1, 2, 3 = 6, 18, 26
    neighbours, scipy.ndimage.generate_binary_structure(3, connectivity)) -> (labels int32 [n0, n1, n2], K): scipy.ndimage.label's
    result exactly - 0 on the background, the components numbered 1..K in raster order of their first voxel.  return_sizes:
    (labels, K, sizes int64 [K]), sizes[l - 1] = the voxels of component l.  One launch sequence and one read-back of 64 bytes."""
    _volume_on_gpu(x, "the volume", "label_components_3d")
    labels, sizes, record = components_record((x != 0).to(torch.uint8).contiguous(), connectivity)
    k = int(record[1])
    if not return_sizes:
        return labels, k
    return labels, k, sizes[:k].to(torch.int64) & 0xffffffff      # the library's uint32 (held in an int32 tensor) as int64


def filter_components_3d(x: torch.Tensor, connectivity: int = 1, largest_only: bool = False, min_size: int = 1) -> torch.Tensor:
    """The foreground of a [n0, n1, n2] device tensor (non-zero) without its small pieces -> bool [n0, n1, n2]: the voxels whose
    component has at least `min_size` voxels and, with largest_only, is the largest one (of equal sizes the one that comes first in
    raster order).  afx_label_components_3d + afx_filter_components_3d: the second reads the first's record on the device, nothing is
    read back.  A volume without foreground gives an empty mask."""
    _volume_on_gpu(x, "the volume", "filter_components_3d")
    labels, sizes, record = components_record((x != 0).to(torch.uint8).contiguous(), connectivity)
    return components_filter(labels, sizes, record, largest_only, min_size).bool()


def components_filter(labels: torch.Tensor, sizes: torch.Tensor, record: torch.Tensor, largest_only: bool = False, min_size: int = 1,
                      out=None) -> torch.Tensor:
    """afx_filter_components_3d on what `components_record` returned -> uint8 [n0, n1, n2] (1 = kept).  Launches only; pass `out` to
    keep a graph capture free of allocations."""
    lib = _lib.load()
    _volume_on_gpu(labels, "labels", "filter_components_3d")
    if not 1 <= int(min_size) <= 0xffffffff:
        raise ValueError(f"filter_components_3d: min_size must lie in 1..2^32 - 1, got {min_size}")
    n0, n1, n2 = labels.shape
    dev, who = labels.device, "filter_components_3d"
    _buffer(labels, "labels", torch.int32, labels.shape, dev, who)
    _buffer(sizes, "sizes", torch.int32, labels.numel(), dev, who)
    _buffer(record, "record", torch.int64, COMPONENTS_RECORD_SLOTS, dev, who)
    out = _out(out, "out", torch.uint8, labels.shape, dev, who)
    _lib.check(lib.afx_filter_components_3d(_ptr(labels), _ptr(sizes), _ptr(record), n0, n1, n2, int(bool(largest_only)), int(min_size),
                                            _ptr(out), Engine._stream(dev)), "afx_filter_components_3d")
    return out


SKELETON_RECORD_SLOTS = 8


def skeleton_record(x: torch.Tensor, max_passes: int, sync_every: int = 0, skel=None, record=None, workspace=None):
    """afx_skeletonize_3d on a contiguous uint8 [n0, n1, n2] device mask (non-zero = foreground) -> (skel, record): skel uint8
    [n0, n1, n2] (1 on the medial curves; pass skel=x to thin in place), record the 8-slot int64 device record (layout in include/afx.h:
    passes, deleted, converged, remaining, deleted by the last pass, input voxels).  sync_every = 0 issues exactly `max_passes` passes
    and reads nothing back, so the call can be captured in a graph (pass all three buffers, the workspace of
    afx_skeletonize_3d_workspace_bytes bytes, to keep the capture free of allocations; passes beyond convergence change nothing);
    sync_every > 0 lets the library look at the record every so many passes and stop at convergence."""
    lib = _lib.load()
    _volume_on_gpu(x, "the mask", "skeletonize_3d")
    dev, who = x.device, "skeleton_record"
    _buffer(x, "the mask", torch.uint8, x.shape, dev, who)
    n0, n1, n2 = x.shape
    nbytes = int(lib.afx_skeletonize_3d_workspace_bytes(n0, n1, n2))      # (0: a shape the library refuses)
    skel = _out(skel, "skel", torch.uint8, x.shape, dev, who, ok=nbytes > 0)
    record = _out(record, "record", torch.int64, SKELETON_RECORD_SLOTS, dev, who)
    workspace, nbytes = _scratch(workspace, nbytes, dev, who)
    _lib.check(lib.afx_skeletonize_3d(_ptr(x), n0, n1, n2, int(max_passes), int(sync_every), _ptr(skel), _ptr(record), _ptr(workspace),
                                      nbytes, Engine._stream(dev)), "afx_skeletonize_3d")
    return skel, record


def skeletonize_3d(x: torch.Tensor, max_passes=None, return_record: bool = False):
    """The medial curves of a [n0, n1, n2] device tensor (any dtype, non-zero = foreground) -> bool [n0, n1, n2]: 8-subfield parallel
    thinning with (26, 6)-simple points, curve end points kept (the definition in include/afx.h) - the same 26-components, cavities and
    tunnels as the input, a subset of it, a pure function of it.  max_passes: stop after that many passes (None: run until a pass
    deletes nothing; the library looks at its record every 4 passes).  return_record: (skeleton, record) with record = {"passes",
    "deleted", "converged", "remaining", "deleted_last", "input"}; converged is 0 when max_passes came first."""
    _volume_on_gpu(x, "the volume", "skeletonize_3d")
    fg = (x != 0).to(torch.uint8).contiguous()
    if max_passes is None:
        max_passes = min(fg.numel() + 1, 2 ** 31 - 1)      # every pass but the last deletes a voxel: never reached
    skel, record = skeleton_record(fg, max_passes, sync_every=4, skel=fg)
    if not return_record:
        return skel.bool()
    r = record.cpu().tolist()
    return skel.bool(), dict(zip(("passes", "deleted", "converged", "remaining", "deleted_last", "input"), r))


ISOSURFACE_RECORD_SLOTS = 8
_IDENTITY_AFFINE = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _affine12(index_to_world, who: str):
    """index_to_world as 12 doubles: rows m[r][0..2], o[r] (a [3, 4] array, a flat sequence of 12, None = the identity)."""
    import numpy as np
    a = np.asarray(_IDENTITY_AFFINE if index_to_world is None else index_to_world, dtype=np.float64).reshape(-1)
    if a.size != 12:
        raise ValueError(f"{who}: index_to_world must hold 12 numbers (a 3 x 4 matrix: rows m[r][0..2], o[r]), got {a.size}")
    return a


def isosurface_record(x: torch.Tensor, iso: float, index_to_world=None, max_vertices: int = 0, max_triangles: int = 0, vertices=None,
                      triangles=None, record=None, workspace=None):
    """afx_isosurface_3d on a float32 [n0, n1, n2] device volume -> (vertices float32 [max_vertices, 3], triangles int32
    [max_triangles, 3], record): marching tetrahedra on the Kuhn split, the mesh of {x >= iso} in the canonical order of include/afx.h;
    record the 8-slot int64 device record (V, T, E, B, the tetrahedra cut two and two, status bit 1: V > max_vertices, bit 2:
    T > max_triangles).  The counts are the true ones whatever the capacities, and nothing is written beyond them: both capacities 0
    is the counting call.  Launches only - nothing is read back, so the call can be captured in a graph (pass all four buffers, the
    workspace of afx_isosurface_3d_workspace_bytes bytes, to keep the capture free of allocations)."""
    lib = _lib.load()
    _volume_on_gpu(x, "the volume", "isosurface_record")
    dev = x.device
    f = _buffer(x, "the volume", torch.float32, None, dev, "isosurface_record", copy=True)
    n0, n1, n2 = f.shape
    aff = (C.c_double * 12)(*_affine12(index_to_world, "isosurface_record"))
    max_vertices, max_triangles = int(max_vertices), int(max_triangles)
    # (the capacities are lower bounds: a longer table is the caller's to pass, nothing is written beyond max_vertices / max_triangles rows)
    vertices = _out(vertices, "vertices", torch.float32, (max_vertices, 3), dev, "isosurface_record", ok=0 <= max_vertices < 2 ** 31, at_least=True)
    triangles = _out(triangles, "triangles", torch.int32, (max_triangles, 3), dev, "isosurface_record", ok=0 <= max_triangles < 2 ** 31, at_least=True)
    record = _out(record, "record", torch.int64, ISOSURFACE_RECORD_SLOTS, dev, "isosurface_record")
    workspace, nbytes = _scratch(workspace, lib.afx_isosurface_3d_workspace_bytes(n0, n1, n2), dev, "isosurface_record")
    _lib.check(lib.afx_isosurface_3d(_ptr(f), n0, n1, n2, float(iso), aff, _ptr(vertices) if max_vertices else None, max_vertices,
                                     _ptr(triangles) if max_triangles else None, max_triangles, _ptr(record), _ptr(workspace),
                                     nbytes, None, Engine._stream(dev)), "afx_isosurface_3d")
    return vertices, triangles, record


def extract_isosurface(x: torch.Tensor, iso: float, index_to_world=None, cap: bool = True, fill: float = 0.0):
    """The surface {x = iso} of a [n0, n1, n2] device volume as an indexed triangle mesh -> (vertices float32 [V, 3], triangles int32
    [T, 3], info): a voxel is inside when x >= iso, the vertices are welded and canonically numbered, the triangles wound so that
    their normals point from inside to outside in the coordinates of index_to_world (12 numbers, rows m[r][0..2], o[r]; None = index
    coordinates).  info = {"V", "T", "E", "B", "n22", "euler"}: vertices, triangles, edges, boundary edges, tetrahedra cut two and two,
    and V - E + T.  The counting call, one read-back of the record (64 bytes), an exact allocation, the emitting call.
    cap: one layer of `fill` is put around the volume first (the affine moves by one index, so the positions do not), which closes the
    surface where the vessel leaves the grid: B = 0.  ValueError when fill >= iso (the cap would be inside)."""
    _volume_on_gpu(x, "the volume", "extract_isosurface")
    dev = x.device
    f = _buffer(x, "the volume", torch.float32, None, dev, "extract_isosurface", copy=True)
    aff = _affine12(index_to_world, "extract_isosurface").reshape(3, 4)
    if cap:
        if not float(fill) < float(iso):
            raise ValueError(f"extract_isosurface: fill = {fill} must lie below iso = {iso}: the cap has to be outside")
        f = torch.nn.functional.pad(f, (1, 1, 1, 1, 1, 1), value=float(fill))
        aff = aff.copy()
        aff[:, 3] = aff[:, 3] - aff[:, :3] @ [1.0, 1.0, 1.0]
    ws = _scratch(None, _lib.load().afx_isosurface_3d_workspace_bytes(*f.shape), dev, "extract_isosurface")[0]
    rec = isosurface_record(f, iso, aff, workspace=ws)[2].cpu().tolist()
    v, t = rec[0], rec[1]
    if v > 2 ** 31 - 1 or t > 2 ** 31 - 1:
        raise ValueError(f"extract_isosurface: the mesh has {v} vertices and {t} triangles, more than 2^31 - 1")
    vertices, triangles, record = isosurface_record(f, iso, aff, v, t, workspace=ws)
    info = {"V": v, "T": t, "E": rec[2], "B": rec[3], "n22": rec[4], "euler": v - rec[2] + t}
    return vertices, triangles, info


def mesh_measures_record(vertices: torch.Tensor, triangles: torch.Tensor, record: torch.Tensor, ref_point=None, out=None, workspace=None):
    """afx_mesh_measures on what `isosurface_record` returned -> float64 [2] on the device: the surface area and the enclosed volume
    about ref_point (3 numbers; None = the origin).  V and T are read from the record on the device.  Launches only; pass `out` and
    the workspace of afx_mesh_measures_workspace_bytes bytes to keep a graph capture free of allocations."""
    lib = _lib.load()
    dev, who = _mesh_on_gpu(vertices, triangles, "mesh_measures"), "mesh_measures"
    _buffer(_on_gpu(record, "the record", who), "the record", torch.int64, ISOSURFACE_RECORD_SLOTS, dev, who)
    out = _out(out, "out", torch.float64, 2, dev, who)
    workspace, nbytes = _scratch(workspace, lib.afx_mesh_measures_workspace_bytes(), dev, who)
    ref = (C.c_double * 3)(*[float(r) for r in (ref_point if ref_point is not None else (0.0, 0.0, 0.0))])
    nv, nt = vertices.shape[0], triangles.shape[0]
    _lib.check(lib.afx_mesh_measures(_ptr(vertices) if nv else None, nv, _ptr(triangles) if nt else None, nt, _ptr(record), ref, _ptr(out),
                                     _ptr(workspace), nbytes, None, Engine._stream(dev)), "afx_mesh_measures")
    return out


def mesh_measures(vertices: torch.Tensor, triangles: torch.Tensor, ref_point=None) -> dict:
    """{"area", "volume"} of an indexed triangle mesh on the device (float32 [V, 3], int32 [T, 3]): the sum of the triangles' areas and
    the enclosed volume, sum of (v0 - r) . ((v1 - r) x (v2 - r)) / 6, in fp64 in a fixed order - positive for a closed mesh whose
    normals point outwards.  ref_point r: None = the mean of the vertices' bounding box (the terms then cancel least)."""
    v, t = _as_mesh(vertices, triangles, "mesh_measures")
    if ref_point is None:
        ref_point = ((v.min(0).values.double() + v.max(0).values.double()) / 2).cpu().tolist() if v.shape[0] else (0.0, 0.0, 0.0)
    record = torch.tensor([v.shape[0], t.shape[0]] + [0] * (ISOSURFACE_RECORD_SLOTS - 2), dtype=torch.int64, device=v.device)
    out = mesh_measures_record(v, t, record, ref_point).cpu().tolist()
    return {"area": out[0], "volume": out[1]}


MESH_SDF_RECORD_SLOTS = 8
MESH_SDF_TILE = 512          # AFX_MESH_SDF_TILE: triangles per LDS tile of the grid kernel
MESH_SDF_BRUTE, MESH_SDF_CLOSED = 1, 2
_MESH_SDF_RECORD_KEYS = ("valid_triangles", "skipped_triangles", "clear_bricks", "pairs_evaluated")


def _mesh_on_gpu(vertices, triangles, who: str):
    """vertices contiguous float32 [V, 3] and triangles contiguous int32 [T, 3] on one GPU -> that device."""
    dev = _on_gpu(vertices, "vertices", who).device
    _on_gpu(triangles, "triangles", who)
    _buffer(vertices, "vertices", torch.float32, vertices.shape[:1] + (3,), dev, who, exact_shape=True)
    _buffer(triangles, "triangles", torch.int32, triangles.shape[:1] + (3,), dev, who, exact_shape=True)
    return dev


def _as_mesh(vertices, triangles, who: str):
    _on_gpu(vertices, "vertices", who), _on_gpu(triangles, "triangles", who)
    return vertices.to(torch.float32).contiguous().view(-1, 3), triangles.to(torch.int32).contiguous().view(-1, 3)


def mesh_sdf_record(vertices: torch.Tensor, triangles: torch.Tensor, shape, index_to_world=None, flags: int = 0, sdf=None, nearest=None,
                    winding=None, record=None, workspace=None):
    """afx_mesh_sdf_3d on a mesh on the device (float32 [V, 3], int32 [T, 3]) -> (sdf float32 [n0, n1, n2], record): the signed distance
    (negative inside) of every point of the grid `shape` whose point (i0, i1, i2) lies at index_to_world (12 numbers, rows m[r][0..2],
    o[r]; None = index coordinates), as include/afx.h defines it.  flags: MESH_SDF_BRUTE | MESH_SDF_CLOSED.  nearest (int32 [n0, n1,
    n2]) and winding (float64 [n0, n1, n2]) are filled when given.  record: the 8-slot int64 device record (valid triangles, skipped
    triangles, clear bricks, pairs the distance pass evaluated).  Launches only - nothing is read back, so the call can be captured in
    a graph (pass sdf, record and the workspace of afx_mesh_sdf_3d_workspace_bytes(T) bytes to keep the capture free of allocations)."""
    lib = _lib.load()
    dev, who = _mesh_on_gpu(vertices, triangles, "mesh_sdf_record"), "mesh_sdf_record"
    n0, n1, n2 = (int(n) for n in shape)
    aff = (C.c_double * 12)(*_affine12(index_to_world, who))
    nv, nt = vertices.shape[0], triangles.shape[0]
    ok = _volume_side_ok((n0, n1, n2))
    sdf = _out(sdf, "sdf", torch.float32, (n0, n1, n2), dev, who, ok=ok)
    if nearest is not None:
        _out(nearest, "nearest", torch.int32, (n0, n1, n2), dev, who, ok=ok)
    if winding is not None:
        _out(winding, "winding", torch.float64, (n0, n1, n2), dev, who, ok=ok)
    record = _out(record, "record", torch.int64, MESH_SDF_RECORD_SLOTS, dev, who)
    workspace, nbytes = _scratch(workspace, lib.afx_mesh_sdf_3d_workspace_bytes(nt), dev, who)
    _lib.check(lib.afx_mesh_sdf_3d(_ptr(vertices) if nv else None, nv, _ptr(triangles) if nt else None, nt, n0, n1, n2, aff, int(flags),
                                   _ptr(sdf), _ptr(nearest), _ptr(winding), _ptr(record), _ptr(workspace), nbytes, None, Engine._stream(dev)),
               "afx_mesh_sdf_3d")
    return sdf, record


def mesh_signed_distance(vertices: torch.Tensor, triangles: torch.Tensor, shape, index_to_world=None, closed: bool = False, brute: bool = False,
                         return_nearest: bool = False, return_winding: bool = False, return_record: bool = False):
    """The signed distance field of a triangle mesh on the device (vertices [V, 3], triangles [T, 3]) on the regular grid `shape` ->
    float32 [n0, n1, n2], negative inside: the exact distance to the nearest triangle, signed by the generalised winding number (robust
    on soups, degenerate triangles, meshes that leave the grid).  closed: the promise that the mesh has no boundary (a capped
    isosurface), which lets bricks the surface does not come near share one winding number.  brute: no culling (the comparator; the
    same bits).  Further results follow in the order nearest (int32, the index of the nearest triangle, -1 without any), winding
    (float64, which forces the per-point sum), record ({"valid_triangles", "skipped_triangles", "clear_bricks", "pairs_evaluated"})."""
    v, t = _as_mesh(vertices, triangles, "mesh_signed_distance")
    n0, n1, n2 = (int(n) for n in shape)
    ok = _volume_side_ok((n0, n1, n2))
    nearest = torch.empty((n0, n1, n2), dtype=torch.int32, device=v.device) if return_nearest and ok else None
    winding = torch.empty((n0, n1, n2), dtype=torch.float64, device=v.device) if return_winding and ok else None
    flags = (MESH_SDF_BRUTE if brute else 0) | (MESH_SDF_CLOSED if closed else 0)
    sdf, record = mesh_sdf_record(v, t, (n0, n1, n2), index_to_world, flags, nearest=nearest, winding=winding)
    out = [sdf] + ([nearest] if return_nearest else []) + ([winding] if return_winding else [])
    if return_record:
        out.append(dict(zip(_MESH_SDF_RECORD_KEYS, record.cpu().tolist())))
    return out[0] if len(out) == 1 else tuple(out)


def mesh_point_distance_record(points: torch.Tensor, vertices: torch.Tensor, triangles: torch.Tensor, dist=None, nearest=None, record=None):
    """afx_mesh_point_distance: the unsigned distance of points (float32 [P, 3], device) to a mesh on the device -> (dist float32 [P],
    record); nearest (int32 [P]) is filled when given.  All pairs, one launch, no workspace; nothing is read back (pass dist and record
    to keep a graph capture free of allocations)."""
    lib = _lib.load()
    dev, who = _mesh_on_gpu(vertices, triangles, "mesh_point_distance_record"), "mesh_point_distance_record"
    _buffer(_on_gpu(points, "points", who), "points", torch.float32, points.shape[:1] + (3,), dev, who, exact_shape=True)
    n = points.shape[0]
    dist = _out(dist, "dist", torch.float32, n, dev, who)
    if nearest is not None:
        _buffer(nearest, "nearest", torch.int32, n, dev, who)
    record = _out(record, "record", torch.int64, MESH_SDF_RECORD_SLOTS, dev, who)
    nv, nt = vertices.shape[0], triangles.shape[0]
    _lib.check(lib.afx_mesh_point_distance(_ptr(points) if n else None, n, _ptr(vertices) if nv else None, nv, _ptr(triangles) if nt else None,
                                           nt, _ptr(dist) if n else None, _ptr(nearest) if nearest is not None and n else None, _ptr(record),
                                           Engine._stream(dev)), "afx_mesh_point_distance")
    return dist, record


def mesh_point_distance(points: torch.Tensor, vertices: torch.Tensor, triangles: torch.Tensor, return_nearest: bool = False):
    """The distance of every point ([P, 3], device) to the nearest triangle of a mesh on the device -> float32 [P] (+inf without a valid
    triangle); with return_nearest also the index of that triangle (int32, the smallest one on a tie, -1 without any)."""
    _on_gpu(points, "points", "mesh_point_distance")
    v, t = _as_mesh(vertices, triangles, "mesh_point_distance")
    p = points.to(torch.float32).contiguous().view(-1, 3)
    nearest = torch.empty(p.shape[0], dtype=torch.int32, device=v.device) if return_nearest else None
    dist, _ = mesh_point_distance_record(p, v, t, nearest=nearest)
    return (dist, nearest) if return_nearest else dist


GRAPH_RECORD_SLOTS = 16
GRAPH_BRANCH_SLOTS = 16
PRUNE_RECORD_SLOTS = 8
_GRAPH_RECORD_NAMES = ("n_on", "n_junction_voxels", "n_path_voxels", "n_nodes", "n_branches", "n_deg0", "n_deg1", "n_free_ends", "n_cycles",
                       "n_spurs")


def _step_class_offsets():
    """The offset of each of the 13 step classes: class c has code c + 14 = (d0 + 1) * 9 + (d1 + 1) * 3 + (d2 + 1)."""
    return [((c + 14) // 9 - 1, (c + 14) // 3 % 3 - 1, (c + 14) % 3 - 1) for c in range(13)]


def graph_step_lengths(index_to_world=None):
    """step_lengths of afx_centreline_graph for an index_to_world ([3, 4] or 12 numbers; None = unit voxels): |A d_c| in fp64 on the host,
    A its 3 x 3 matrix, d_c the offset of step class c."""
    import numpy as np
    if index_to_world is None:
        return None
    a = _affine12(index_to_world, "centreline_graph").reshape(3, 4)[:, :3]
    return [float(np.sqrt(((a @ np.asarray(d, np.float64)) ** 2).sum())) for d in _step_class_offsets()]


def _d2_u32(d2, like: torch.Tensor, who: str):
    """The squared EDT as the library's uint32, held in an int32 tensor (distance_transform_edt_3d returns it as int64)."""
    if d2 is None:
        return None
    _volume_on_gpu(d2, "d2", who)
    if d2.shape != like.shape or d2.device != like.device:
        raise ValueError(f"{who}: d2 {tuple(d2.shape)} on {d2.device}, the mask {tuple(like.shape)} on {like.device}")
    if d2.dtype == torch.int32:
        return d2.contiguous()
    d = d2.to(torch.int64)
    return torch.where(d >= 2 ** 31, d - 2 ** 32, d).to(torch.int32).contiguous()


def centreline_graph_record(skel: torch.Tensor, d2=None, step_lengths=None, max_branches: int = 0, node_labels=None, branch_labels=None,
                            path_voxels=None, branches=None, record=None, workspace=None):
    """afx_centreline_graph on a contiguous uint8 [n0, n1, n2] device mask (non-zero = on; d2: int32 tensor holding the uint32 squared EDT,
    or None) -> (node_labels, branch_labels, path_voxels, branches, record): int32 volumes, int32 [N], int64 [max_branches, 16] rows and
    the 16-slot int64 device record (layouts in include/afx.h).  Launches only - nothing is read back, so the call can be captured in a
    graph (pass every buffer, the workspace of afx_centreline_graph_workspace_bytes bytes, to keep the capture free of allocations)."""
    import ctypes as C
    lib = _lib.load()
    _volume_on_gpu(skel, "the mask", "centreline_graph")
    dev, who = skel.device, "centreline_graph_record"
    _buffer(skel, "the mask", torch.uint8, skel.shape, dev, who)
    if d2 is not None:
        _buffer(d2, "d2", torch.int32, skel.shape, dev, who, exact_shape=True)
    n0, n1, n2 = skel.shape
    nbytes = int(lib.afx_centreline_graph_workspace_bytes(n0, n1, n2))      # (0: a shape the library refuses)
    node_labels = _out(node_labels, "node_labels", torch.int32, skel.shape, dev, who, ok=nbytes > 0)
    branch_labels = _out(branch_labels, "branch_labels", torch.int32, skel.shape, dev, who, ok=nbytes > 0)
    path_voxels = _out(path_voxels, "path_voxels", torch.int32, skel.numel(), dev, who, ok=nbytes > 0)
    branches = _out(branches, "branches", torch.int64, (max(int(max_branches), 0), GRAPH_BRANCH_SLOTS), dev, who)
    record = _out(record, "record", torch.int64, GRAPH_RECORD_SLOTS, dev, who)
    workspace, nbytes = _scratch(workspace, nbytes, dev, who)
    L = None if step_lengths is None else (C.c_double * 13)(*[float(x) for x in step_lengths])
    _lib.check(lib.afx_centreline_graph(_ptr(skel), _ptr(d2), n0, n1, n2, L, _ptr(node_labels), _ptr(branch_labels), _ptr(path_voxels),
                                        _ptr(branches) if int(max_branches) > 0 else None, int(max_branches), _ptr(record), _ptr(workspace),
                                        nbytes, None, Engine._stream(dev)), "afx_centreline_graph")
    return node_labels, branch_labels, path_voxels, branches, record


def _unpack_branch_rows(rows: torch.Tensor) -> dict:
    """The fields of [B, 16] int64 branch rows (include/afx.h) as tensors; device-independent."""
    lo = lambda x: x & 0xffffffff
    hi = lambda x: (x >> 32) & 0xffffffff
    out = {"branch_size": lo(rows[:, 0]), "path_offset": hi(rows[:, 0]), "is_cycle": (rows[:, 1] & 1).bool(), "is_spur": ((rows[:, 1] >> 1) & 1).bool(),
           "free_ends": (rows[:, 1] >> 8) & 3, "attachments": (rows[:, 1] >> 16) & 3, "d2_argmin": hi(rows[:, 1]),
           "node_start": lo(rows[:, 2]), "node_end": hi(rows[:, 2]), "d2_min": lo(rows[:, 3]), "d2_max": hi(rows[:, 3]),
           "d2_start": lo(rows[:, 4]), "d2_end": hi(rows[:, 4]),
           "step_counts": torch.stack([f(rows[:, 5 + q]) for q in range(7) for f in (lo, hi)][:13], dim=1) if rows.shape[0] else
           torch.zeros((0, 13), dtype=torch.int64, device=rows.device),
           "length": rows[:, 12].contiguous().view(torch.float64), "radius_sum": rows[:, 13].contiguous().view(torch.float64),
           "first_voxel": lo(rows[:, 14]), "last_voxel": hi(rows[:, 14])}
    return out


def centreline_graph(skel: torch.Tensor, d2=None, index_to_world=None) -> dict:
    """The centreline of a [n0, n1, n2] device mask (any dtype, non-zero = on; ANY mask, a skeleton is the usual one) read as a graph
    (definitions in include/afx.h): junction nodes = the 26-components of the voxels with 3 or more neighbours, branches = those of the
    voxels with at most 2, each a path, a single voxel or a cycle.  d2: the squared EDT of the mask that was thinned
    (distance_transform_edt_3d(..., return_squared=True)[1]) for the radii; index_to_world ([3, 4]) for lengths in world units (None: voxels).
    -> dict: node_labels, branch_labels (int32 volumes), path_voxels (int64 [P]: the linear indices branch after branch in path order),
    per-branch tensors of B entries (branch_size, path_offset, is_cycle, is_spur, free_ends, attachments, node_start, node_end, step_counts
    [B, 13], length, and with d2: d2_min, d2_max, d2_argmin, d2_start, d2_end, radius_sum), and the integers n_on, n_junction_voxels,
    n_path_voxels, n_nodes, n_branches, n_deg0, n_deg1, n_free_ends, n_cycles, n_spurs, total_length (float), d2_min_all (None without
    d2 or without a branch).  One launch sequence and one read-back of 128 bytes; a second one when more than 1024 branches were found."""
    import numpy as np
    _volume_on_gpu(skel, "the mask", "centreline_graph")
    s = (skel != 0).to(torch.uint8).contiguous()
    d = _d2_u32(d2, s, "centreline_graph")
    L = graph_step_lengths(index_to_world)
    cap = 1024
    nl, bl, pv, rows, record = centreline_graph_record(s, d, L, cap)
    rec = record.cpu().numpy()
    if int(rec[11]) & 1:                                  # the table was too small: once more with the reported B
        nl, bl, pv, rows, record = centreline_graph_record(s, d, L, int(rec[4]))
        rec = record.cpu().numpy()
    nb = int(rec[4])
    out = {"node_labels": nl, "branch_labels": bl, "path_voxels": pv[:int(rec[2])].to(torch.int64), "shape": tuple(s.shape), "has_d2": d is not None}
    out.update(_unpack_branch_rows(rows[:nb]))
    out.update({k: int(v) for k, v in zip(_GRAPH_RECORD_NAMES, rec[:10])})
    out["total_length"] = float(rec.view(np.float64)[10])
    d2_min = int(rec[12]) & 0xffffffff
    out["d2_min_all"] = None if d is None or nb == 0 else d2_min
    return out


def prune_record(skel: torch.Tensor, d2: torch.Tensor, factor: float, max_rounds: int, sync_every: int = 0, out=None, record=None, workspace=None):
    """afx_prune_spurs on a contiguous uint8 [n0, n1, n2] device mask and its int32-held uint32 squared EDT -> (out, record): out uint8
    (1 / 0; pass out=skel to prune in place), record the 8-slot int64 device record (rounds, branches deleted, voxels deleted, converged,
    remaining, input, deleted by the last round).  sync_every = 0 issues exactly max_rounds rounds and reads nothing back (capturable:
    pass all three buffers); sync_every > 0 lets the library look at the record every so many rounds and stop at convergence."""
    lib = _lib.load()
    _volume_on_gpu(skel, "the mask", "prune_spurs")
    dev, who = skel.device, "prune_record"
    _buffer(skel, "the mask", torch.uint8, skel.shape, dev, who)
    _buffer(d2, "d2", torch.int32, skel.shape, dev, who, exact_shape=True)
    n0, n1, n2 = skel.shape
    nbytes = int(lib.afx_prune_spurs_workspace_bytes(n0, n1, n2))      # (0: a shape the library refuses)
    out = _out(out, "out", torch.uint8, skel.shape, dev, who, ok=nbytes > 0)
    record = _out(record, "record", torch.int64, PRUNE_RECORD_SLOTS, dev, who)
    workspace, nbytes = _scratch(workspace, nbytes, dev, who)
    _lib.check(lib.afx_prune_spurs(_ptr(skel), _ptr(d2), n0, n1, n2, float(factor), int(max_rounds), int(sync_every), _ptr(out), _ptr(record),
                                   _ptr(workspace), nbytes, None, Engine._stream(dev)), "afx_prune_spurs")
    return out, record


def prune_spurs(skel: torch.Tensor, d2: torch.Tensor, factor: float = 1.0, max_rounds=None, return_record: bool = False):
    """A [n0, n1, n2] device mask without its spurs -> bool [n0, n1, n2]: round after round, every branch with one free end and one
    junction whose length (in voxels) is at most factor x the radius sqrt(d2) at the junction voxel it hangs on is deleted, until a round
    deletes nothing (include/afx.h).  Junction voxels stay, so components, cavities and tunnels are kept.  max_rounds: stop after that
    many rounds (None: until convergence).  return_record: (mask, record) with record = {"rounds", "branches", "voxels", "converged",
    "remaining", "input", "last"}."""
    _volume_on_gpu(skel, "the mask", "prune_spurs")
    s = (skel != 0).to(torch.uint8).contiguous()
    d = _d2_u32(d2, s, "prune_spurs")
    if d is None:
        raise ValueError("prune_spurs: d2 (the squared EDT of the mask that was thinned) is required")
    if max_rounds is None:
        max_rounds = min(s.numel() + 1, 2 ** 31 - 1)      # every round but the last deletes a voxel: never reached
    out, record = prune_record(s, d, factor, max_rounds, sync_every=1, out=s)
    if not return_record:
        return out.bool()
    r = record.cpu().tolist()
    return out.bool(), dict(zip(("rounds", "branches", "voxels", "converged", "remaining", "input", "last"), r))


def centreline_branch_profile(graph: dict, d2: torch.Tensor, b: int, voxel_size=1.0) -> dict:
    """Arc length and radius along branch b (1-based) of a `centreline_graph` result: {"voxels" (int64 [n] linear indices in path order),
    "arc_length" (float64 [n], 0 at the path's first voxel, the Euclidean steps added up), "radius" (float64 [n]: voxel_size x sqrt(d2),
    an isotropic scalar or the geometric reading along the smallest axis is the caller's choice), "r_min", "r_median", "stenosis" =
    1 - r_min / median(r)}.  voxel_size: a scalar or one size per axis (arc lengths use the per-axis sizes, radii the smallest).  Plain
    torch operations on whatever device the graph lives on.  The radius is the inscribed-sphere radius of the thresholded mask, quantised
    to whole voxels; `centreline_lumen_profile` and `lumen_branch_summary` measure the cross-section's area, diameters and the percent
    stenosis below the voxel, on the density itself."""
    nb = int(graph["n_branches"])
    if not 1 <= int(b) <= nb:
        raise ValueError(f"centreline_branch_profile: branch {b} outside 1..{nb}")
    off, n = int(graph["path_offset"][b - 1]), int(graph["branch_size"][b - 1])
    vox = graph["path_voxels"][off:off + n].to(torch.int64)
    n0, n1, n2 = graph["shape"]
    vs = torch.as_tensor(voxel_size, dtype=torch.float64, device=vox.device).reshape(-1)
    vs = vs.expand(3) if vs.numel() == 1 else vs
    ijk = torch.stack([vox // (n1 * n2), vox // n2 % n1, vox % n2], dim=1).to(torch.float64) * vs
    steps = (ijk[1:] - ijk[:-1]).pow(2).sum(1).sqrt()
    arc = torch.cat([torch.zeros(1, dtype=torch.float64, device=vox.device), torch.cumsum(steps, 0)])
    dd = d2.reshape(-1)[vox.to(d2.device)].to(torch.int64) & 0xffffffff
    radius = dd.to(torch.float64).sqrt().to(vox.device) * vs.min()
    r_min, r_med = float(radius.min()), float(radius.median())
    return {"voxels": vox, "arc_length": arc, "radius": radius, "r_min": r_min, "r_median": r_med,
            "stenosis": 1.0 - r_min / r_med if r_med > 0 else 0.0}


LUMEN_PROFILE_SLOTS = 8
LUMEN_NO_TANGENT, LUMEN_CENTRE_OUTSIDE = 1, 2
_LUMEN_COLUMNS = ("area", "r_mean", "r_min", "r_max", "d_min", "d_max", "centre_value")


def lumen_world_to_index(index_to_world=None):
    """world_to_index of afx_lumen_profile, 12 doubles (rows W[a][0..2], W[a][3]): the inverse of index_to_world ([3, 4] or 12 numbers;
    None = the identity, exactly) taken in fp64 on the host - W = inv(A), offset -(W o).  The library and the NumPy restatement get this
    array alike."""
    import numpy as np
    if index_to_world is None:
        return np.asarray(_IDENTITY_AFFINE, np.float64).reshape(-1).copy()
    a = _affine12(index_to_world, "lumen_profile").reshape(3, 4)
    w = np.linalg.inv(a[:, :3])
    return np.concatenate([w, -(w @ a[:, 3])[:, None]], axis=1).reshape(-1)


def lumen_ray_table(n_rays: int):
    """(ray_cs float64 [2 R]: cos(2 pi j / R) at [2 j] and sin(2 pi j / R) at [2 j + 1]; area_coef = sin(2 pi / R) / 2) of afx_lumen_profile,
    made with NumPy on the host."""
    import numpy as np
    r = int(n_rays)
    if r not in (8, 16, 32, 64):
        raise ValueError(f"lumen_profile: n_rays must be 8, 16, 32 or 64, got {n_rays!r}")
    ang = 2.0 * np.pi * np.arange(r, dtype=np.float64) / r
    cs = np.empty(2 * r, np.float64)
    cs[0::2], cs[1::2] = np.cos(ang), np.sin(ang)
    return cs, float(0.5 * np.sin(2.0 * np.pi / r))


def lumen_default_step(index_to_world=None) -> float:
    """The default march step of lumen_profile: half the smallest |A d| over the three axis steps d of index_to_world's matrix A."""
    import numpy as np
    a = _affine12(index_to_world, "lumen_profile").reshape(3, 4)[:, :3]
    return 0.5 * float(np.sqrt((a * a).sum(axis=0)).min())


def lumen_profile_record(volume: torch.Tensor, points: torch.Tensor, seg_first: torch.Tensor, seg_last: torch.Tensor, world_to_index, iso: float,
                         n_rays: int, step: float, max_steps: int, half_window: int = 3, ray_cs=None, area_coef=None, profile=None, flags=None,
                         radii=None, want_radii: bool = False):
    """afx_lumen_profile on a contiguous float32 or float64 [n0, n1, n2] device volume, points float64 [P, 3] (world) and seg_first /
    seg_last int32 [P] on its device -> (profile float64 [P, 8], flags int32 [P], radii float64 [P, n_rays] or None); the definition, the
    row layout and the flag bits stand in include/afx.h.  world_to_index: 12 host numbers (`lumen_world_to_index`); ray_cs, area_coef:
    `lumen_ray_table(n_rays)` unless given.  Launches only: nothing is read back, and with profile, flags (and radii) passed nothing is
    allocated - the call can be captured in a graph."""
    import numpy as np
    lib = _lib.load()
    _volume_on_gpu(volume, "the volume", "lumen_profile")
    dev, who = volume.device, "lumen_profile_record"
    _buffer(volume, "the volume", (torch.float32, torch.float64), volume.shape, dev, who)
    _on_gpu(points, "points", who), _on_gpu(seg_first, "seg_first", who), _on_gpu(seg_last, "seg_last", who)
    _buffer(points, "points", torch.float64, points.shape[:1] + (3,), dev, who, exact_shape=True)
    n = points.shape[0]
    _buffer(seg_first, "seg_first", torch.int32, n, dev, who), _buffer(seg_last, "seg_last", torch.int32, n, dev, who)
    r = int(n_rays)
    if ray_cs is None or area_coef is None:
        ray_cs, area_coef = lumen_ray_table(r)
    cs = np.ascontiguousarray(ray_cs, np.float64).reshape(-1)
    w = np.ascontiguousarray(world_to_index, np.float64).reshape(-1)
    if w.size != 12 or cs.size != 2 * max(r, 0):
        raise ValueError(f"lumen_profile_record: world_to_index must hold 12 numbers and ray_cs 2 x n_rays, got {w.size} and {cs.size}")
    profile = _out(profile, "profile", torch.float64, (n, LUMEN_PROFILE_SLOTS), dev, who)
    flags = _out(flags, "flags", torch.int32, n, dev, who)
    if radii is not None or want_radii:
        radii = _out(radii, "radii", torch.float64, (n, max(r, 0)), dev, who)
    n0, n1, n2 = volume.shape
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    _lib.check(lib.afx_lumen_profile(_ptr(volume), int(volume.dtype == torch.float64), n0, n1, n2, dp(w), _ptr(points) if n else None,
                                     _ptr(seg_first) if n else None, _ptr(seg_last) if n else None, n, int(half_window), r, dp(cs),
                                     float(area_coef), float(iso), float(step), int(max_steps), _ptr(profile) if n else None,
                                     _ptr(flags) if n else None, _ptr(radii) if radii is not None and n else None, Engine._stream(dev)),
               "afx_lumen_profile")
    return profile, flags, radii


def lumen_profile(volume: torch.Tensor, points, seg_first, seg_last, index_to_world=None, iso: float = 0.5, n_rays: int = 64, step=None,
                  r_max=None, half_window: int = 3, return_radii: bool = False) -> dict:
    """The lumen cross-section at every centreline point (include/afx.h: afx_lumen_profile): a fan of n_rays rays in the plane normal to the
    centreline is marched in steps of `step` (world units) through the trilinearly interpolated float32 / float64 [n0, n1, n2] device volume
    until it falls below `iso`; the crossing radii, interpolated below the step, give the area of the cross-section and its diameters.
    points [P, 3] world coordinates (index (i0, i1, i2) lies at index_to_world, [3, 4]; None: the identity); seg_first / seg_last [P]: the
    first and last point index of the polyline a point belongs to (the tangent window of +-half_window points stops there).  step: half
    the smallest voxel step unless given; r_max: how far a ray goes, 32 steps unless given (max_steps = ceil(r_max / step), at most 4096).
    -> dict of device tensors [P]: area, r_mean, r_min, r_max, d_min, d_max (world units), centre_value (the volume at the point), flags
    (bit 0: no tangent, bit 1: the point is not inside the lumen, bits 8..15: rays that found no crossing), n_open, valid (flags == 0), and
    seg_first; with return_radii also radii [P, n_rays].  A flagged point's numbers are zeros."""
    import math
    _volume_on_gpu(volume, "the volume", "lumen_profile")
    if volume.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"lumen_profile: the volume must be float32 or float64, got {volume.dtype}")
    dev = volume.device
    pts = torch.as_tensor(points, dtype=torch.float64).to(dev).reshape(-1, 3).contiguous()
    sf = torch.as_tensor(seg_first).to(dev, torch.int32).reshape(-1).contiguous()
    sl = torch.as_tensor(seg_last).to(dev, torch.int32).reshape(-1).contiguous()
    if step is None:
        step = lumen_default_step(index_to_world)
    step = float(step)
    if not (step > 0.0 and math.isfinite(step)):
        raise ValueError(f"lumen_profile: step must be finite and > 0, got {step!r}")
    max_steps = 32 if r_max is None else int(math.ceil(float(r_max) / step))
    profile, flags, radii = lumen_profile_record(volume.contiguous(), pts, sf, sl, lumen_world_to_index(index_to_world), iso, n_rays, step,
                                                 max_steps, half_window, want_radii=return_radii)
    out = {name: profile[:, q] for q, name in enumerate(_LUMEN_COLUMNS)}
    out.update(flags=flags, n_open=(flags >> 8) & 0xff, valid=flags == 0, seg_first=sf, step=step, max_steps=max_steps)
    if return_radii:
        out["radii"] = radii
    return out


def centreline_world_points(graph: dict, index_to_world):
    """The path voxels of a `centreline_graph` result in world coordinates -> (points float64 [P, 3], offsets int64 [B + 1]): branch b
    (1-based) is points[offsets[b - 1]:offsets[b]] in path order.  Host arithmetic in fp64 (NumPy): the one place that forms these points
    (`visualization.sweep.centreline_polylines`, `centreline_lumen_profile`)."""
    import numpy as np
    a = np.asarray(index_to_world, np.float64).reshape(3, 4)
    vox = graph["path_voxels"].cpu().numpy().astype(np.int64)
    n0, n1, n2 = graph["shape"]
    ijk = np.stack([vox // (n1 * n2), vox // n2 % n1, vox % n2], axis=1).astype(np.float64)
    points = ijk @ a[:, :3].T + a[:, 3]
    sizes = graph["branch_size"].cpu().numpy().astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return points, offsets


def centreline_segments(points, offsets):
    """(seg_first int32 [P], seg_last int32 [P], branch int64 [P] 1-based, arc_length float64 [P]) of polylines given as points [P, 3] and
    offsets [B + 1]: arc_length is 0 at a branch's first point and adds the Euclidean steps, sqrt((dx dx + dy dy) + dz dz), one after
    another.  NumPy on the host."""
    import numpy as np
    offsets = np.asarray(offsets, np.int64)
    sizes = offsets[1:] - offsets[:-1]
    p = int(offsets[-1]) if offsets.size else 0
    branch = np.repeat(np.arange(1, sizes.size + 1, dtype=np.int64), sizes)
    seg_first = np.repeat(offsets[:-1], sizes).astype(np.int32)
    seg_last = np.repeat(offsets[1:] - 1, sizes).astype(np.int32)
    arc = np.zeros(p, np.float64)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    for b in range(sizes.size):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        d = pts[lo + 1:hi] - pts[lo:hi - 1]
        steps = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        for q in range(steps.size):
            arc[lo + 1 + q] = arc[lo + q] + steps[q]
    return seg_first, seg_last, branch, arc


def centreline_lumen_profile(graph: dict, volume: torch.Tensor, index_to_world, iso: float, **kw) -> dict:
    """`lumen_profile` along every branch of a `centreline_graph` result: the points are the path voxels in world coordinates
    (`centreline_world_points`; junction voxels belong to no branch), each branch a polyline of its own.  -> the dict of `lumen_profile`
    plus points (float64 [P, 3]), branch (int64 [P], 1-based) and arc_length (float64 [P], 0 at a branch's first point), on the volume's
    device; `lumen_branch_summary` reads the narrowing per branch from it."""
    _volume_on_gpu(volume, "the volume", "centreline_lumen_profile")
    a = _affine12(index_to_world, "centreline_lumen_profile")
    points, offsets = centreline_world_points(graph, a)
    seg_first, seg_last, branch, arc = centreline_segments(points, offsets)
    out = lumen_profile(volume, points, seg_first, seg_last, a, iso, **kw)
    dev = volume.device
    out.update(points=torch.from_numpy(points).to(dev), branch=torch.from_numpy(branch).to(dev), arc_length=torch.from_numpy(arc).to(dev))
    return out


def lumen_branch_summary(profile: dict, min_points: int = 5) -> dict:
    """The narrowing of every branch of a lumen profile (`centreline_lumen_profile`; or `lumen_profile`, its polylines numbered from 1 in
    the order of their first points) -> dict of NumPy arrays, one entry per branch: branch (the ids, ascending), n_valid, and for a
    branch with at least min_points valid points (flags == 0): area_min, argmin (the position within the branch's points of the first
    minimum), area_ref = the LOWER median sorted[(n_valid - 1) // 2] of the valid areas, area_stenosis = 1 - area_min / area_ref and
    diameter_stenosis = 1 - sqrt(area_min / area_ref); NaN (argmin -1) for the other branches.  Host arithmetic on the read-back arrays."""
    import numpy as np
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    area, flags = host(profile["area"]).astype(np.float64), host(profile["flags"])
    if "branch" in profile:
        branch = host(profile["branch"]).astype(np.int64)
    else:
        branch = np.unique(host(profile["seg_first"]), return_inverse=True)[1].astype(np.int64).reshape(-1) + 1
    ids = np.unique(branch)
    out = {"branch": ids, "n_valid": np.zeros(ids.size, np.int64), "argmin": np.full(ids.size, -1, np.int64)}
    for name in ("area_min", "area_ref", "area_stenosis", "diameter_stenosis"):
        out[name] = np.full(ids.size, np.nan)
    for q, b in enumerate(ids):
        mine = np.flatnonzero(branch == b)
        ok = mine[flags[mine] == 0]
        out["n_valid"][q] = ok.size
        if ok.size < max(int(min_points), 1):
            continue
        a = area[ok]
        first = int(np.argmin(a))
        ref = np.sort(a)[(ok.size - 1) // 2]
        out["area_min"][q], out["argmin"][q], out["area_ref"][q] = a[first], ok[first] - mine[0], ref
        ratio = a[first] / ref
        out["area_stenosis"][q], out["diameter_stenosis"][q] = 1.0 - ratio, 1.0 - np.sqrt(ratio)
    return out


REFORMAT_PLANE_DOUBLES, REFORMAT_TABLE_DOUBLES = 9, 4
REFORMAT_MODES = {"mean": 0, "max": 1}
REFORMAT_TILE = 8                     # the side of the tiles of a tiled cross-section table
REFORMAT_TILED = True                 # the order straighten_volume hands its table over in: the faster of the two in profiles/r27_cpr.md
FRAME_KEPT = 1                        # rotation_minimising_frames: the point kept the previous frame


def _host(x):
    import numpy as np
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def centreline_main_path(graph: dict, index_to_world, start=None, end=None, d2=None) -> dict:
    """The main path of a `centreline_graph` result, from the ostium side to the farthest distal end, across branches and junctions.
    The path graph: its vertices are the junction nodes and the free ends (a free side of a branch), its edges the non-cycle branches
    weighted by their `length` (a branch from a node back to the same node is no edge).  Shortest paths by Dijkstra in fp64; where two
    ways to a vertex are equally long the one whose last branch has the smaller label stays.  start, end: the linear voxel index of a
    free end.  Default start: the free end with the largest d2 (d2: the squared EDT volume the graph was made with, read at the end
    voxel; without it every free end ties), a tie to the smaller voxel index - the ostium side.  Default end: the free end farthest from
    start, a tie to the smaller voxel index.  -> dict: points (float64 [P, 3], world: the branches' path voxels in travel order, a branch
    reversed when it is entered from its end side; a junction cluster is bridged by the straight step between the two extremes next to
    it), voxels (int64 [P], the linear indices), branches (1-based, in travel order), reversed (per branch), start, end (voxels) and
    length (the sum of the branch lengths).  ValueError: no free end, start or end no free end, start and end not connected.  NumPy on
    the host, as `centreline_world_points`."""
    import heapq
    import numpy as np
    a = _affine12(index_to_world, "centreline_main_path").reshape(3, 4)
    size = _host(graph["branch_size"]).astype(np.int64).reshape(-1)
    nb = size.size
    offset = _host(graph["path_offset"]).astype(np.int64).reshape(-1) if "path_offset" in graph else np.concatenate([[0], np.cumsum(size)[:-1]])
    cyc = _host(graph["is_cycle"]).astype(bool).reshape(-1)
    node = np.stack([_host(graph["node_start"]).astype(np.int64).reshape(-1), _host(graph["node_end"]).astype(np.int64).reshape(-1)], axis=1)
    length = _host(graph["length"]).astype(np.float64).reshape(-1)
    vox = _host(graph["path_voxels"]).astype(np.int64).reshape(-1)
    side_voxel = lambda b, s: int(vox[offset[b] + (size[b] - 1 if s else 0)])
    vertex = lambda b, s: ("n", int(node[b, s])) if node[b, s] else ("f", b, s)
    edges, ends = {}, []                                  # vertex -> [(branch, other vertex)]; the free ends (voxel, vertex)
    for b in range(nb):
        if cyc[b] or size[b] < 1:
            continue
        va, vb = vertex(b, 0), vertex(b, 1)
        ends += [(side_voxel(b, s), v) for s, v in ((0, va), (1, vb)) if v[0] == "f"]
        if va != vb:
            edges.setdefault(va, []).append((b, vb))
            edges.setdefault(vb, []).append((b, va))
    if not ends:
        raise ValueError("centreline_main_path: the graph has no free end")

    def pick(voxel, what):
        found = [v for x, v in ends if x == int(voxel)]
        if not found:
            raise ValueError(f"centreline_main_path: {what} = {voxel} is not the voxel of a free end")
        return found[0]

    if start is None:
        dd = None if d2 is None else _host(d2).reshape(-1)
        key = lambda e: (-(int(dd[e[0]]) & 0xffffffff) if dd is not None else 0, e[0])
        v_start = min(ends, key=key)[1]
    else:
        v_start = pick(start, "start")
    dist, via = {v_start: 0.0}, {}
    heap, done = [(0.0, 0, v_start)], set()
    tick = 1
    while heap:
        d, _, v = heapq.heappop(heap)
        if v in done:
            continue
        done.add(v)
        for b, w in edges.get(v, ()):
            nd = d + float(length[b])
            if w not in done and (w not in dist or nd < dist[w] or (nd == dist[w] and b < via[w][0])):
                dist[w], via[w] = nd, (b, v)
                heapq.heappush(heap, (nd, tick, w))
                tick += 1
    if end is None:
        far = [(-dist[v], x, v) for x, v in ends if v in dist and v != v_start]
        if not far:
            raise ValueError("centreline_main_path: no other free end is connected to start")
        v_end = min(far, key=lambda e: e[:2])[2]
    else:
        v_end = pick(end, "end")
        if v_end == v_start and len([1 for x, v in ends if x == int(end)]) > 1:
            v_end = [v for x, v in ends if x == int(end)][1]          # a lone voxel: its two free sides
    if v_end not in dist:
        raise ValueError("centreline_main_path: start and end are not connected")
    hops, v = [], v_end
    while v != v_start:
        b, prev = via[v]
        hops.append((b, vertex(b, 0) != prev))            # entered from its end side: reversed
        v = prev
    hops.reverse()
    if not hops:
        raise ValueError("centreline_main_path: start and end are the same free end")
    voxels = np.concatenate([vox[offset[b]:offset[b] + size[b]][::-1 if rev else 1] for b, rev in hops])
    n0, n1, n2 = graph["shape"]
    ijk = np.stack([voxels // (n1 * n2), voxels // n2 % n1, voxels % n2], axis=1).astype(np.float64)
    return {"points": ijk @ a[:, :3].T + a[:, 3], "voxels": voxels, "branches": [b + 1 for b, _ in hops], "reversed": [bool(r) for _, r in hops],
            "start": int(voxels[0]), "end": int(voxels[-1]), "length": float(dist[v_end])}


def polyline_smooth(points, passes: int = 8, lam: float = 0.5):
    """Laplacian smoothing of a polyline [P, 3]: `passes` Jacobi passes of x_k <- x_k + lam ((x_{k-1} + x_{k+1}) / 2 - x_k), every point
    from the previous pass, the two ends fixed.  NumPy fp64 on the host."""
    import numpy as np
    x = np.array(points, np.float64).reshape(-1, 3)
    for _ in range(int(passes)):
        if len(x) < 3:
            break
        new = x.copy()
        new[1:-1] = x[1:-1] + float(lam) * ((x[:-2] + x[2:]) / 2.0 - x[1:-1])
        x = new
    return x


def _arc_length(pts):
    """0 at the first point, the Euclidean steps sqrt((dx dx + dy dy) + dz dz) added one after another (as `centreline_segments`)."""
    import numpy as np
    d = pts[1:] - pts[:-1]
    steps = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    arc = np.zeros(len(pts), np.float64)
    for q in range(steps.size):
        arc[q + 1] = arc[q] + steps[q]
    return arc


def polyline_resample(points, spacing: float):
    """A polyline [P, 3] at the arc lengths 0, spacing, 2 spacing, .. (linear interpolation between its points; the last partial step is
    dropped, the first point is kept).  NumPy fp64 on the host."""
    import numpy as np
    x = np.array(points, np.float64).reshape(-1, 3)
    spacing = float(spacing)
    if not (spacing > 0.0 and np.isfinite(spacing)):
        raise ValueError(f"polyline_resample: spacing must be finite and > 0, got {spacing!r}")
    if len(x) < 2:
        return x
    arc = _arc_length(x)
    n = int(np.floor(arc[-1] / spacing)) + 1
    while n > 1 and (n - 1) * spacing > arc[-1]:
        n -= 1
    s = np.arange(n, dtype=np.float64) * spacing
    k = np.clip(np.searchsorted(arc, s, side="right") - 1, 0, len(x) - 2)
    seg = arc[k + 1] - arc[k]
    w = np.where(seg > 0.0, (s - arc[k]) / np.where(seg > 0.0, seg, 1.0), 0.0)
    return x[k] + w[:, None] * (x[k + 1] - x[k])


def rotation_minimising_frames(points, half_window: int = 3):
    """Frames (t, u, v) along one polyline [P, 3] that do not twist about it: the rotation-minimising frame by double reflection (Wang,
    Juettler, Zheng, Liu 2008) -> (t, u, v float64 [P, 3], flags int32 [P]).  dot(a, b) = (a0 b0 + a1 b1) + a2 b2 and cross(a, b) =
    (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0) throughout, every operation in fp64 rounded on its own, in this order:
      tangent (afx_lumen_profile step 1):  a = max(k - h, 0), b = min(k + h, P - 1), d = x_b - x_a, n2 = dot(d, d); b <= a or n2 == 0:
          no tangent; else t_k = d / sqrt(n2)
      first frame (step 2), at the first point k0 that has a tangent:  e = the unit axis of the first smallest |t_a|, w = cross(t, e),
          u = w / sqrt(dot(w, w)), v = cross(t, u)
      from point i to i + 1:  v1 = x_{i+1} - x_i, c1 = dot(v1, v1);  k1 = 2 / c1;  rL = u_i - (k1 dot(v1, u_i)) v1;
          tL = t_i - (k1 dot(v1, t_i)) v1;  v2 = t_{i+1} - tL, c2 = dot(v2, v2);  w = rL when c2 == 0, else
          w = rL - ((2 / c2) dot(v2, rL)) v2;  w <- w - dot(w, t_{i+1}) t_{i+1};  n = sqrt(dot(w, w));  u_{i+1} = w / n;
          v_{i+1} = cross(t_{i+1}, u_{i+1})
    A point without a tangent, with c1 == 0 or with n == 0 keeps the frame (t, u and v) of the point before it and gets flag FRAME_KEPT;
    the points before k0 get the frame of k0 and the flag; a polyline without any tangent gets zeros.  NumPy on the host, point by point:
    centrelines have hundreds to a few thousand points."""
    import numpy as np
    x = np.array(points, np.float64).reshape(-1, 3)
    p, h = len(x), int(half_window)
    if h < 1:
        raise ValueError(f"rotation_minimising_frames: half_window must be at least 1, got {half_window!r}")
    t, u, v, flags = np.zeros((p, 3)), np.zeros((p, 3)), np.zeros((p, 3)), np.zeros(p, np.int32)
    if p == 0:
        return t, u, v, flags
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    cross = lambda a, b: np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    k = np.arange(p)
    ia, ib = np.maximum(k - h, 0), np.minimum(k + h, p - 1)
    d = x[ib] - x[ia]
    n2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    has = (ib > ia) & (n2 > 0.0) & np.isfinite(n2)
    t[has] = d[has] / np.sqrt(n2[has])[:, None]
    if not has.any():
        flags[:] = FRAME_KEPT
        return t, u, v, flags
    k0 = int(np.flatnonzero(has)[0])
    e = np.eye(3)[int(np.argmin(np.abs(t[k0])))]
    w = cross(t[k0], e)
    u[k0] = w / np.sqrt(dot(w, w))
    v[k0] = cross(t[k0], u[k0])
    t[:k0], u[:k0], v[:k0], flags[:k0] = t[k0], u[k0], v[k0], FRAME_KEPT
    for i in range(k0, p - 1):
        v1 = x[i + 1] - x[i]
        c1 = dot(v1, v1)
        n = 0.0
        if has[i + 1] and c1 > 0.0:
            k1 = 2.0 / c1
            r_l = u[i] - (k1 * dot(v1, u[i])) * v1
            t_l = t[i] - (k1 * dot(v1, t[i])) * v1
            v2 = t[i + 1] - t_l
            c2 = dot(v2, v2)
            w = r_l if c2 == 0.0 else r_l - ((2.0 / c2) * dot(v2, r_l)) * v2
            w = w - dot(w, t[i + 1]) * t[i + 1]
            n = np.sqrt(dot(w, w))
        if n > 0.0:
            u[i + 1] = w / n
            v[i + 1] = cross(t[i + 1], u[i + 1])
        else:
            t[i + 1], u[i + 1], v[i + 1], flags[i + 1] = t[i], u[i], v[i], FRAME_KEPT
    return t, u, v, flags


def reformat_table_grid(k: int, step: float, tiled: bool = False):
    """The sample table of a K x K cross-section, K = 2 k + 1, centred -> (table float64 [K K, 4], perm int64 [K K]).  Sample (i, j) lies
    at (a, b) = ((i - k) step, (j - k) step) in the plane, no slab (sa = sb = 0); its row-order position is i K + j.  table[n] is the
    sample perm[n]: tiled = False is the row order (perm = 0, 1, ..); tiled = True walks REFORMAT_TILE x REFORMAT_TILE tiles one after
    another (tiles in row order, the samples of a tile in row order, the tiles at the high edges partial), so that 64 consecutive rows
    cover a compact patch.  A result out [P, K K] of the table is put back into row order by `rows[:, perm] = out`."""
    import numpy as np
    k = int(k)
    if k < 0:
        raise ValueError(f"reformat_table_grid: k must be >= 0, got {k}")
    side = 2 * k + 1
    i, j = np.divmod(np.arange(side * side, dtype=np.int64), side)
    if tiled:
        perm = np.lexsort((j, i, j // REFORMAT_TILE, i // REFORMAT_TILE)).astype(np.int64)      # the last key is the primary one
    else:
        perm = np.arange(side * side, dtype=np.int64)
    table = np.zeros((side * side, REFORMAT_TABLE_DOUBLES), np.float64)
    table[:, 0] = (i[perm] - k).astype(np.float64) * float(step)
    table[:, 1] = (j[perm] - k).astype(np.float64) * float(step)
    return table, perm


def reformat_table_cpr(k: int, step: float, angles, slab_step=None):
    """The sample table of longitudinal images at the in-plane angles `angles` (degrees) -> float64 [A K, 4], K = 2 k + 1: row (n, j) =
    n K + j is the sample at r (cos theta_n, sin theta_n), r = (j - k) step, with the slab direction slab_step (-sin theta_n,
    cos theta_n) at right angles to the line (slab_step: `step` unless given).  cos and sin by NumPy on the host, of np.deg2rad(theta)."""
    import numpy as np
    k = int(k)
    if k < 0:
        raise ValueError(f"reformat_table_cpr: k must be >= 0, got {k}")
    theta = np.deg2rad(np.asarray(angles, np.float64).reshape(-1))
    cs, sn = np.cos(theta)[:, None], np.sin(theta)[:, None]
    r = ((np.arange(2 * k + 1) - k).astype(np.float64) * float(step))[None, :]
    sl = float(step if slab_step is None else slab_step)
    one = np.ones_like(r)
    return np.stack([r * cs, r * sn, (sl * -sn) * one, (sl * cs) * one], axis=2).reshape(-1, REFORMAT_TABLE_DOUBLES)


def reformat_planes_record(volume: torch.Tensor, planes: torch.Tensor, table: torch.Tensor, world_to_index, fill: float = 0.0, half_slab: int = 0,
                           mode: str = "mean", out=None):
    """afx_reformat_planes on a contiguous float32 or float64 [n0, n1, n2] device volume, planes float64 [P, 9] (centre, u, v: world) and
    table float64 [Q, 4] (a, b, sa, sb) on its device -> out float64 [P, Q]; the definition stands in include/afx.h.  world_to_index: 12
    host numbers (`lumen_world_to_index`); mode "mean" or "max" over the slab of 2 half_slab + 1 samples.  Launches only: nothing is read
    back, and with `out` passed nothing is allocated - the call can be captured in a graph."""
    import numpy as np
    lib = _lib.load()
    _volume_on_gpu(volume, "the volume", "reformat_planes")
    dev, who = volume.device, "reformat_planes_record"
    _buffer(volume, "the volume", (torch.float32, torch.float64), volume.shape, dev, who)
    for t, name, cols in ((planes, "planes", REFORMAT_PLANE_DOUBLES), (table, "table", REFORMAT_TABLE_DOUBLES)):
        _buffer(_on_gpu(t, name, who), name, torch.float64, t.shape[:1] + (cols,), dev, who, exact_shape=True)
    if mode not in REFORMAT_MODES:
        raise ValueError(f"reformat_planes_record: mode must be one of {sorted(REFORMAT_MODES)}, got {mode!r}")
    w = np.ascontiguousarray(world_to_index, np.float64).reshape(-1)
    if w.size != 12:
        raise ValueError(f"reformat_planes_record: world_to_index must hold 12 numbers, got {w.size}")
    p, q = planes.shape[0], table.shape[0]
    out = _out(out, "out", torch.float64, (p, q), dev, who)
    n0, n1, n2 = volume.shape
    _lib.check(lib.afx_reformat_planes(_ptr(volume), int(volume.dtype == torch.float64), n0, n1, n2, w.ctypes.data_as(C.POINTER(C.c_double)),
                                       _ptr(planes) if p else None, p, _ptr(table) if q else None, q, int(half_slab), REFORMAT_MODES[mode],
                                       float(fill), _ptr(out) if p * q else None, Engine._stream(dev)), "afx_reformat_planes")
    return out


def _reformat_frames(volume, points, index_to_world, step, half_window, who):
    """The shared front of straighten_volume and cpr_images: the frames of the polyline and the planes on the volume's device."""
    import numpy as np
    _volume_on_gpu(volume, "the volume", who)
    if volume.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{who}: the volume must be float32 or float64, got {volume.dtype}")
    pts = np.ascontiguousarray(_host(points), np.float64).reshape(-1, 3)
    t, u, v, flags = rotation_minimising_frames(pts, half_window)
    step = float(lumen_default_step(index_to_world) if step is None else step)
    if not (step > 0.0 and np.isfinite(step)):
        raise ValueError(f"{who}: step must be finite and > 0, got {step!r}")
    planes = torch.from_numpy(np.ascontiguousarray(np.concatenate([pts, u, v], axis=1))).to(volume.device)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(volume.device)
    fields = {"points": dev(pts), "t": dev(t), "u": dev(u), "v": dev(v), "arc_length": dev(_arc_length(pts)), "flags": dev(flags), "step": step}
    return planes, fields


def straighten_volume(volume: torch.Tensor, points, index_to_world=None, half_width: int = 16, step=None, half_window: int = 3, fill: float = 0.0,
                      tiled=None) -> dict:
    """The vessel straightened along a polyline (world points [P, 3], e.g. `polyline_resample` of a smoothed `centreline_main_path`): at
    every point the K x K cross-section, K = 2 half_width + 1, of the trilinearly interpolated float32 / float64 [n0, n1, n2] device
    volume in the plane of the point's rotation-minimising frame, sample (i, j) at c + (i - half_width) step u + (j - half_width) step v
    (`fill` outside the volume).  step: world units, `lumen_default_step` unless given.  tiled: the order the sample table is handed over
    in (None: REFORMAT_TILED); the result does not depend on it.  -> dict: volume (float64 [P, K, K]), points, t, u, v ([P, 3]),
    arc_length, flags (int32 [P]: FRAME_KEPT) - device tensors - and step."""
    import numpy as np
    planes, out = _reformat_frames(volume, points, index_to_world, step, half_window, "straighten_volume")
    table, perm = reformat_table_grid(half_width, out["step"], REFORMAT_TILED if tiled is None else bool(tiled))
    side = 2 * int(half_width) + 1
    got = reformat_planes_record(volume.contiguous(), planes, torch.from_numpy(table).to(volume.device), lumen_world_to_index(index_to_world), fill)
    rows = torch.empty_like(got)
    rows[:, torch.from_numpy(perm).to(volume.device)] = got
    out["volume"] = rows.reshape(planes.shape[0], side, side)
    return out


def cpr_images(volume: torch.Tensor, points, index_to_world=None, angles=(0.0, 90.0), half_width: int = 16, step=None, slab: int = 0,
               mode: str = "mean", half_window: int = 3, fill: float = 0.0) -> dict:
    """Longitudinal (straightened curved-planar) images of a vessel along a polyline: image n, row p is the line through point p at the
    in-plane angle angles[n] (degrees from u towards v of the point's rotation-minimising frame), K = 2 half_width + 1 samples `step`
    apart, each the mean or the maximum (`mode`) over a slab of 2 slab + 1 samples `step` apart at right angles to the line.  -> the dict
    of `straighten_volume` with images (float64 [A, P, K]) and angles in place of volume."""
    import numpy as np
    planes, out = _reformat_frames(volume, points, index_to_world, step, half_window, "cpr_images")
    ang = np.asarray(angles, np.float64).reshape(-1)
    table = reformat_table_cpr(half_width, out["step"], ang)
    got = reformat_planes_record(volume.contiguous(), planes, torch.from_numpy(table).to(volume.device), lumen_world_to_index(index_to_world), fill,
                                 int(slab), mode)
    out["images"] = got.reshape(planes.shape[0], ang.size, 2 * int(half_width) + 1).permute(1, 0, 2).contiguous()
    out["angles"] = ang
    return out


def centreline_cpr(graph: dict, volume: torch.Tensor, index_to_world, d2=None, smooth_passes: int = 8, spacing=None, start=None, end=None,
                   **kw) -> dict:
    """`cpr_images` along the main path of a `centreline_graph` result: `centreline_main_path` (d2: the squared EDT, for the ostium side),
    `polyline_smooth(smooth_passes)`, `polyline_resample(spacing)` (spacing: the smallest voxel step unless given), then the images.
    -> the dict of `cpr_images` plus path (the dict of `centreline_main_path`) and spacing."""
    _volume_on_gpu(volume, "the volume", "centreline_cpr")
    a = _affine12(index_to_world, "centreline_cpr")
    path = centreline_main_path(graph, a, start=start, end=end, d2=d2)
    spacing = float(2.0 * lumen_default_step(a) if spacing is None else spacing)
    pts = polyline_resample(polyline_smooth(path["points"], smooth_passes), spacing)
    out = cpr_images(volume, pts, a, **kw)
    out.update(path=path, spacing=spacing)
    return out


def frangi_3d_record(x: torch.Tensor, sigmas=(1, 2, 3), alpha: float = 0.5, beta: float = 0.5, gamma=None, black_ridges: bool = False, out=None,
                     scale_index=None, workspace=None, want_scale: bool = True):
    """afx_frangi_3d on a contiguous float32 or float64 [n0, n1, n2] device volume -> (out float64 [n0, n1, n2], scale_index uint8
    [n0, n1, n2] or None): the 3-D Frangi vesselness defined in include/afx.h and the index of the first scale that attains it.  Reads
    nothing back and, with all three buffers passed (the workspace of afx_frangi_3d_workspace_bytes bytes), allocates nothing: the call can
    be captured in a graph.  gamma None: per scale sqrt(max S) / 2.  want_scale False (and no scale_index buffer): no index is written."""
    lib = _lib.load()
    _volume_on_gpu(x, "the volume", "frangi_3d")
    dev, who = x.device, "frangi_3d_record"
    _buffer(x, "the volume", (torch.float32, torch.float64), x.shape, dev, who)
    if gamma is not None and not float(gamma) > 0.0:
        raise ValueError(f"frangi_3d: gamma must be None (per-scale) or > 0, got {gamma!r}")
    n0, n1, n2 = x.shape
    sg, ns = _sigma_array(sigmas)
    nbytes = int(lib.afx_frangi_3d_workspace_bytes(n0, n1, n2, ns))      # (0: a shape the library refuses)
    out = _out(out, "out", torch.float64, x.shape, dev, who, ok=nbytes > 0)
    if scale_index is not None or want_scale:
        scale_index = _out(scale_index, "scale_index", torch.uint8, x.shape, dev, who, ok=nbytes > 0)
    workspace, nbytes = _scratch(workspace, nbytes, dev, who)
    _lib.check(lib.afx_frangi_3d(_ptr(x), int(x.dtype == torch.float64), n0, n1, n2, sg, ns, float(alpha), float(beta),
                                 0.0 if gamma is None else float(gamma), int(bool(black_ridges)), _ptr(out), _ptr(scale_index), _ptr(workspace),
                                 nbytes, None, Engine._stream(dev)), "afx_frangi_3d")
    return out, scale_index


def frangi_3d(x: torch.Tensor, sigmas=(1, 2, 3), alpha: float = 0.5, beta: float = 0.5, gamma=None, black_ridges: bool = False,
              return_scale: bool = False):
    """The 3-D Frangi vesselness (Frangi et al. 1998; the definition in include/afx.h) of a float32 or float64 [n0, n1, n2] device volume ->
    float64 [n0, n1, n2] in [0, 1): near 1 on bright tubes of a radius near one of `sigmas` (in voxels), near 0 on blobs, plates and
    background.  black_ridges=False is the default (a density volume has bright vessels; the 2-D `frangi` defaults to dark ones).
    gamma None: per scale sqrt(max S) / 2, so the result does not depend on the volume's density scale; a float fixes it for all scales.
    return_scale: (vesselness, uint8 index into `sigmas` of the first scale that attains it)."""
    _volume_on_gpu(x, "the volume", "frangi_3d")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"frangi_3d: the volume must be float32 or float64, got {x.dtype}")
    out, idx = frangi_3d_record(x.contiguous(), sigmas, alpha, beta, gamma, black_ridges, want_scale=return_scale)
    return (out, idx) if return_scale else out


# ---- the visual hull of the training views (afx_visual_hull) and the mask that carves a grid with it (afx_grid_apply_mask) ----
HULL_VIEW_DOUBLES = 16


def hull_view_records(poses, focal):
    """The view records of afx_visual_hull, float64 [V, 16] on the host: R row-major at [0..8], c at [9..11], f at [12] of each pose
    cam2world = [R | c] ([V, 4, 4] or [V, 3, 4]; focal: a number, or one per view)."""
    import numpy as np
    p = np.asarray(poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else poses, dtype=np.float64)
    if p.ndim != 3 or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError(f"visual_hull_views: poses must be [V, 4, 4] or [V, 3, 4], got {p.shape}")
    v = p.shape[0]
    if not 1 <= v <= 65535:
        raise ValueError(f"visual_hull_views: 1 to 65535 views, got {v}")
    f = np.asarray(focal.detach().cpu().numpy() if isinstance(focal, torch.Tensor) else focal, dtype=np.float64).reshape(-1)
    if f.size not in (1, v):
        raise ValueError(f"visual_hull_views: focal must be one number or one per view ({v}), got {f.size}")
    f = np.broadcast_to(f, (v,))
    if not (np.isfinite(p).all() and np.isfinite(f).all() and (f > 0).all()):
        raise ValueError("visual_hull_views: poses and focal must be finite, focal > 0")
    rot = p[:, :3, :3]
    if not np.allclose(rot @ rot.transpose(0, 2, 1), np.eye(3), atol=1e-9):
        raise ValueError("visual_hull_views: the rotation of a pose is not orthonormal (the hull's bound needs |R^T e| = |e|)")
    rec = np.zeros((v, HULL_VIEW_DOUBLES), np.float64)
    rec[:, 0:9] = rot.reshape(v, 9)
    rec[:, 9:12] = p[:, :3, 3]
    rec[:, 12] = f
    return rec


def visual_hull_views(poses, masks: torch.Tensor, focal, margin_px: float = 1.0) -> dict:
    """The training views of a visual hull: poses [V, 4, 4] or [V, 3, 4] (cam2world, the project's own pose), masks [V, H, W] on the GPU
    (bool or 0/1: the vessel silhouette of each view), focal (a number, or one per view), margin_px (pixels added to every view's
    tolerance).  Builds the stack of distance images D_v (`distance_transform_edt` of the complement of each mask: 0 on the mask) and the
    device copy of the view records.  A view with an empty mask is refused (ValueError): it would reject everything it sees.
    -> dict(records float64 [V, 16] and dist float64 [V, H, W] on the device, n_views, width, height, margin_px)."""
    import math
    if not isinstance(masks, torch.Tensor) or masks.dim() != 3:
        raise ValueError(f"visual_hull_views: masks must be a [V, H, W] tensor, got {type(masks).__name__}"
                         f"{tuple(masks.shape) if isinstance(masks, torch.Tensor) else ''}")
    rec = hull_view_records(poses, focal)
    v, h, w = masks.shape
    if v != rec.shape[0]:
        raise ValueError(f"visual_hull_views: {rec.shape[0]} poses but {v} masks")
    if not (margin_px >= 0 and math.isfinite(margin_px)):
        raise ValueError(f"visual_hull_views: margin_px must be finite and >= 0, got {margin_px!r}")
    on = masks != 0
    empty = torch.nonzero(~on.reshape(v, -1).any(dim=1)).flatten().tolist()
    if empty:
        raise ValueError(f"visual_hull_views: the mask of view {empty[0]} is empty ({len(empty)} such view(s)): it would reject every point it sees")
    _on_gpu(masks, "the masks", "visual_hull_views")
    dist = distance_transform_edt((~on).to(torch.float64))
    return dict(records=torch.from_numpy(rec).to(masks.device), dist=dist, n_views=v, width=int(w), height=int(h), margin_px=float(margin_px))


def hull_default_radius(index_to_world=None) -> float:
    """Half the longest diagonal of the lattice cell spanned by the three axis steps of index_to_world (12 numbers; None: the identity):
    every point of the cell about a lattice point lies within it."""
    import numpy as np
    a = _affine12(index_to_world, "visual_hull").reshape(3, 4)[:, :3]
    return 0.5 * max(float(np.sqrt(((a[:, 0] + s1 * a[:, 1] + s2 * a[:, 2]) ** 2).sum())) for s1 in (-1.0, 1.0) for s2 in (-1.0, 1.0))


def grid_cell_lattice(roi_aabb, resolution):
    """(index_to_world 12 doubles, radius) of an occupancy grid's cell centres: cell size s_a = (hi_a - lo_a) / res_a, centre
    lo_a + s_a / 2 + s_a i_a, radius = half the cell diagonal - formed in fp64 from the grid's float32 box."""
    import numpy as np
    box = np.asarray([float(x) for x in roi_aabb], np.float32).astype(np.float64)
    res = [int(x) for x in resolution]
    s = (box[3:] - box[:3]) / np.asarray(res, np.float64)
    o = box[:3] + 0.5 * s
    a = np.array([s[0], 0, 0, o[0], 0, s[1], 0, o[1], 0, 0, s[2], o[2]], np.float64)
    return a, 0.5 * float(np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))


def visual_hull_record(views: dict, shape, index_to_world, radius: float, seen=None, rejects=None):
    """afx_visual_hull, the launch alone: the votes of `views` (visual_hull_views) over the lattice x = index_to_world (i, j, k, 1) of
    `shape` = (n0, n1, n2), each point speaking for the ball of `radius` about it -> (seen, rejects) uint16 [n0, n1, n2] on the views'
    device.  Nothing is read back and, with seen and rejects passed, nothing is allocated: the call can be captured in a graph."""
    import numpy as np
    lib = _lib.load()
    rec, dist, who = views["records"], views["dist"], "visual_hull_record"
    dev = _on_gpu(dist, "the views", who).device
    n0, n1, n2 = (int(s) for s in shape)
    v, w, h = int(views["n_views"]), int(views["width"]), int(views["height"])
    _buffer(rec, "records", torch.float64, (v, HULL_VIEW_DOUBLES), dev, who, exact_shape=True)
    _buffer(dist, "dist", torch.float64, (v, h, w), dev, who, exact_shape=True)
    a = np.ascontiguousarray(_affine12(index_to_world, who))
    seen = _out(seen, "seen", torch.uint16, (n0, n1, n2), dev, who)
    rejects = _out(rejects, "rejects", torch.uint16, (n0, n1, n2), dev, who)
    _lib.check(lib.afx_visual_hull(n0, n1, n2, a.ctypes.data_as(C.POINTER(C.c_double)), float(radius), _ptr(rec), v, w, h,
                                   float(views["margin_px"]), _ptr(dist), _ptr(seen), _ptr(rejects), Engine._stream(dev)), "afx_visual_hull")
    return seen, rejects


def visual_hull(views: dict, shape, index_to_world=None, radius=None, max_rejects: int = 0, min_seen: int = 1, return_counts: bool = False):
    """The visual hull of the training views over a lattice (include/afx.h: afx_visual_hull): bool [n0, n1, n2], True where at most
    max_rejects views reject the point and at least min_seen views see it.  A view rejects a point when the whole ball of `radius` about
    it (default: half the lattice cell's diagonal, so a point speaks for its cell) projects further than the views' margin from every
    mask pixel.  return_counts: (hull, seen, rejects), the uint16 votes."""
    if radius is None:
        radius = hull_default_radius(index_to_world)
    seen, rejects = visual_hull_record(views, shape, index_to_world, radius)
    hull = (rejects.to(torch.int32) <= int(max_rejects)) & (seen.to(torch.int32) >= int(min_seen))
    return (hull, seen, rejects) if return_counts else hull


def grid_apply_mask(roi_aabb, resolution, mask_u8, occs, binary_u8, bits):
    """afx_grid_apply_mask: occs[c] = 0 (occs may be None) and binary_u8[c] = 0 where mask_u8[c] == 0, and the march's bitfield rewritten
    from the result; in place, one launch."""
    lib = _lib.load()
    dev = binary_u8.device
    if dev.type != "cuda":
        raise AfxError("grid_apply_mask: the occupancy grid lives on a GPU; there is no CPU fallback")
    g = _grid_desc(roi_aabb, resolution)
    n = g.resolution[0] * g.resolution[1] * g.resolution[2]
    for t, name, dtype, count in ((mask_u8, "mask", torch.uint8, n), (binary_u8, "binary", torch.uint8, n), (occs, "occs", torch.float32, n),
                                  (bits, "bits", torch.int32, (n + 31) // 32)):
        if t is not None:
            _buffer(t, name, dtype, count, dev, "grid_apply_mask")
    _lib.check(lib.afx_grid_apply_mask(C.byref(g), _ptr(mask_u8), _ptr(occs), _ptr(binary_u8), _ptr(bits), Engine._stream(dev)),
               "afx_grid_apply_mask")


# ---- optimal C-arm views: the foreshortening and overlap map of a vessel tree (afx_view_map) ----
VIEWMAP_SEGMENT_DOUBLES = 8
VIEWMAP_BRUTE = 1
VIEWMAP_TREE_SLOTS = 4
VIEWMAP_COUNT_BYTES = 256 << 20      # view_map keeps the count buffer of a chunk of views below this


def view_map_segments(points, offsets, radius):
    """The capsules of polylines -> (segments float64 [N, 8], seg_branch int32 [N]) in NumPy on the host, the inputs of afx_view_map:
    points [P, 3] and offsets [B + 1] as `centreline_world_points` gives them, radius [P] (or one number).  A branch's consecutive points
    i, i + 1 make the segment p0, p1 with r = 0.5 (r_i + r_i+1); a one-point branch becomes one degenerate segment (p0 = p1, r = r_i: a
    disc); a branch without points has no segment.  Branch ids are 1-based and non-decreasing."""
    import numpy as np
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    off = np.asarray(offsets, np.int64).reshape(-1)
    r = np.asarray(radius, np.float64).reshape(-1)
    if r.size == 1:
        r = np.broadcast_to(r, (pts.shape[0],))
    if off.size < 2 or off[0] != 0 or off[-1] != pts.shape[0] or (off[1:] < off[:-1]).any():
        raise ValueError(f"view_map_segments: offsets must rise from 0 to the number of points ({pts.shape[0]}), got {off.tolist()[:8]}...")
    if r.shape[0] != pts.shape[0]:
        raise ValueError(f"view_map_segments: one radius per point ({pts.shape[0]}) or one number, got {r.shape[0]}")
    first, last, ids = [], [], []
    for b in range(off.size - 1):
        lo, hi = int(off[b]), int(off[b + 1])
        if hi - lo == 1:
            first.append(lo), last.append(lo), ids.append(b + 1)
        for i in range(lo, hi - 1):
            first.append(i), last.append(i + 1), ids.append(b + 1)
    i0, i1 = np.asarray(first, np.int64), np.asarray(last, np.int64)
    seg = np.zeros((i0.size, VIEWMAP_SEGMENT_DOUBLES), np.float64)
    seg[:, 0:3], seg[:, 3:6], seg[:, 6] = pts[i0], pts[i1], 0.5 * (r[i0] + r[i1])
    return seg, np.asarray(ids, np.int32)


def view_angles_records(angles, src_pt, focal, translation=(0.0, 0.0, 0.0)):
    """The view records (`hull_view_records`, float64 [V, 16] on the host) of (theta, phi) pairs in degrees: the poses
    source_matrix(src_pt, theta mod 360, phi mod 360, 0, translation) of the evaluation sweep."""
    import numpy as np
    from .phantomdata.proj_helpers import source_matrix
    mats = []
    for theta, phi in np.asarray(angles, np.float64).reshape(-1, 2):
        th = theta if theta >= 0 else 360 + theta
        ph = phi if phi >= 0 else 360 + phi
        mats.append(source_matrix(np.asarray(src_pt, dtype=np.float64), th, ph, 0.0, np.asarray(translation, dtype=np.float64)))
    return hull_view_records(np.stack(mats), focal)


def _view_map_inputs(segments, seg_branch, views, who: str):
    """The three inputs on one GPU, checked: NumPy arrays are uploaded to the device of whichever input is a device tensor (else the
    current GPU); a seg_branch given on the host is checked here, one on the device by the library's own launch."""
    import numpy as np
    given = [t for t in (segments, seg_branch, views) if isinstance(t, torch.Tensor)]
    if any(t.device.type != "cuda" for t in given) or (not given and not torch.cuda.is_available()):
        raise AfxError(f"{who}: the view map is taken on a GPU; there is no CPU path")
    dev = given[0].device if given else torch.device("cuda", torch.cuda.current_device())
    if not isinstance(seg_branch, torch.Tensor):
        br = np.asarray(seg_branch)
        if br.ndim != 1 or br.size < 1 or int(br.min()) < 1 or (br[1:] < br[:-1]).any():
            raise ValueError(f"{who}: seg_branch must be a non-empty, non-decreasing list of branch ids >= 1")
        seg_branch = torch.from_numpy(np.ascontiguousarray(br, np.int32)).to(dev)
    up = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dev)
    segments, views = up(segments), up(views)
    n = seg_branch.numel()
    _buffer(segments, "segments", torch.float64, (n, VIEWMAP_SEGMENT_DOUBLES), dev, who, exact_shape=True)
    _buffer(seg_branch, "seg_branch", torch.int32, (n,), dev, who, exact_shape=True)
    _buffer(views, "views", torch.float64, views.shape[:1] + (HULL_VIEW_DOUBLES,), dev, who, exact_shape=True)
    return segments, seg_branch, views


def view_map_record(segments, seg_branch, views, width: int, height: int, brute: bool = False, counts: bool = True, foreshortening: bool = True,
                    n_branches=None, out=None) -> dict:
    """afx_view_map, the launches alone -> the raw device tensors dict(count uint16 [V, H, W], area int32 [V, B], shared int32 [V, B],
    tree int32 [V, 4] (union, multi, n_invisible; tree[0][3] != 0: a bad seg_branch) with counts; proj float64 [V, B], length float64 [B]
    with foreshortening) of segments [N, 8], seg_branch [N] (`view_map_segments`) and view records [V, 16] (`hull_view_records`,
    `view_angles_records`), each a NumPy array or a device tensor.  n_branches: B, by default the last branch id (read on the host; pass
    it with device inputs to read nothing back).  brute: no culling, the same bytes.  out: a dict of buffers to fill instead of
    allocating; with device inputs, n_branches and out the call reads nothing back, allocates nothing and can be captured in a graph."""
    lib = _lib.load()
    if n_branches is None and not isinstance(seg_branch, torch.Tensor):
        import numpy as np
        n_branches = int(np.asarray(seg_branch).reshape(-1)[-1]) if np.size(seg_branch) else 0
    segments, seg_branch, views = _view_map_inputs(segments, seg_branch, views, "view_map_record")
    if n_branches is None:
        n_branches = int(seg_branch[-1])
    dev = segments.device
    n, v, b, w, h = seg_branch.numel(), views.shape[0], int(n_branches), int(width), int(height)
    if not (counts or foreshortening):
        raise ValueError("view_map_record: counts and foreshortening are both off: nothing to compute")
    ok = 1 <= b <= 65535 and 1 <= v <= 65535 and 1 <= w <= 16384 and 1 <= h <= 16384      # (else the library names the offender)
    want = {}
    if counts:
        want.update(count=((v, h, w), torch.uint16), area=((v, b), torch.int32), shared=((v, b), torch.int32),
                    tree=((v, VIEWMAP_TREE_SLOTS), torch.int32))
    if foreshortening:
        want.update(proj=((v, b), torch.float64), length=((b,), torch.float64))
    res = {name: _out(None if out is None else out.get(name), name, dtype, shape, dev, "view_map_record", ok=ok, exact_shape=True)
           for name, (shape, dtype) in want.items()}
    _lib.check(lib.afx_view_map(_ptr(segments), _ptr(seg_branch), n, b, _ptr(views), v, w, h, VIEWMAP_BRUTE if brute else 0, _ptr(res.get("count")),
                                _ptr(res.get("area")), _ptr(res.get("shared")), _ptr(res.get("tree")), _ptr(res.get("proj")), _ptr(res.get("length")),
                                Engine._stream(dev)), "afx_view_map")
    return res


def view_map(graph_or_segments, views, width: int, height: int, radius=None, chunk_views=None, index_to_world=None, d2=None, voxel_size=1.0,
             return_count: bool = False) -> dict:
    """The foreshortening and overlap of every branch of a vessel tree in every view (include/afx.h: afx_view_map) -> dict of NumPy
    arrays on the host: foreshortening [V, B] = 1 - proj / length (0: seen at right angles, 1: seen end on), overlap [V, B] = shared /
    area (the share of the branch's pixels that another branch covers too; NaN where area == 0), tree_foreshortening [V] = 1 - sum proj
    / sum length, tree_overlap [V] = multi / union (NaN for an empty union), area, shared (int32 [V, B]), union, multi, n_invisible
    (int32 [V]), proj [V, B], length [B], n_segments, and with return_count count (uint16 [V, H, W]).

    graph_or_segments: (segments, seg_branch) of `view_map_segments`, or a `centreline_graph` result - then the points are
    `centreline_world_points(graph, index_to_world)` and the radii `radius` (one per path voxel or one number, e.g. a lumen profile's
    r_mean) or, by default, voxel_size x sqrt(d2) at the path voxels (d2: the squared EDT the graph was made with).  views: records
    [V, 16].  The views are taken in chunks of chunk_views (default: as many as keep the count buffer below 256 MiB).  Branches that
    meet at a junction always share a few pixels around it, in every view alike.  There is no CPU path (AfxError)."""
    import numpy as np
    if isinstance(graph_or_segments, dict):
        graph = graph_or_segments
        points, offsets = centreline_world_points(graph, _affine12(index_to_world, "view_map"))
        if radius is None:
            if d2 is None:
                raise ValueError("view_map: a centreline graph needs radius= or d2= (the squared EDT the graph was made with)")
            vox = graph["path_voxels"].cpu().numpy().astype(np.int64)
            dd = (d2.reshape(-1).cpu().numpy().astype(np.int64) & 0xffffffff)[vox]
            radius = np.sqrt(dd.astype(np.float64)) * float(voxel_size)
        segments, seg_branch = view_map_segments(points, offsets, radius)
        n_branches = offsets.size - 1
    else:
        segments, seg_branch = graph_or_segments
        n_branches = int(seg_branch[-1]) if len(seg_branch) else 0
    if len(seg_branch) == 0:
        raise ValueError("view_map: the tree has no segment")
    segments, seg_branch, views = _view_map_inputs(segments, seg_branch, views, "view_map")
    v, w, h = views.shape[0], int(width), int(height)
    if chunk_views is None:
        chunk_views = max(1, VIEWMAP_COUNT_BYTES // max(2 * w * h, 1))
    chunk_views = max(1, min(int(chunk_views), v))
    parts = []
    for v0 in range(0, v, chunk_views):
        res = view_map_record(segments, seg_branch, views[v0:v0 + chunk_views], w, h, n_branches=n_branches)
        keep = ("area", "shared", "tree", "proj", "length") + (("count",) if return_count else ())
        parts.append({k: res[k].cpu().numpy() if k != "count" else res[k].view(torch.int16).cpu().numpy().view(np.uint16) for k in keep})
    raw = {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0] if k != "length"}
    raw["length"] = parts[0]["length"]
    if raw["tree"][:, 3].any():
        raise ValueError("view_map: seg_branch is not a non-decreasing list of branch ids 1..B ending in B")
    out = view_map_derive(raw)
    out["n_segments"] = int(seg_branch.numel())
    return out


def view_map_derive(raw: dict) -> dict:
    """The host's figures from the read-back outputs of afx_view_map (area, shared, tree, proj, length[, count] as NumPy arrays): what
    `view_map` returns.  fp64 on the host."""
    import numpy as np
    area, shared, tree, proj, length = raw["area"], raw["shared"], raw["tree"], raw["proj"], raw["length"]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = dict(foreshortening=1.0 - proj / length[None],
                   overlap=np.where(area > 0, shared.astype(np.float64) / area.astype(np.float64), np.nan),
                   tree_foreshortening=1.0 - proj.sum(axis=1) / length.sum(),
                   tree_overlap=np.where(tree[:, 0] > 0, tree[:, 1].astype(np.float64) / tree[:, 0].astype(np.float64), np.nan))
    out.update(area=area, shared=shared, union=tree[:, 0].copy(), multi=tree[:, 1].copy(), n_invisible=tree[:, 2].copy(), proj=proj, length=length)
    if "count" in raw:
        out["count"] = raw["count"]
    return out


def optimal_views(vmap: dict, branch=None, overlap_weight: float = 1.0, k: int = 5):
    """The k best views of a `view_map` result -> (indices int64 [k'], scores float64 [k']), k' = min(k, V), best first.  The score of a
    view is foreshortening + overlap_weight x overlap - of branch `branch` (1-based), or of the whole tree (branch None) - lower is
    better.  Views whose score is not a number (the branch covers no pixel there: area == 0, overlap NaN) or in which a segment of the
    tree is invisible come last, among themselves by index, with the score NaN; ties go to the lower index.  Host arithmetic."""
    import numpy as np
    if branch is None:
        fs, ov = np.asarray(vmap["tree_foreshortening"], np.float64), np.asarray(vmap["tree_overlap"], np.float64)
    else:
        nb = np.asarray(vmap["foreshortening"]).shape[1]
        if not 1 <= int(branch) <= nb:
            raise ValueError(f"optimal_views: branch {branch} outside 1..{nb}")
        fs, ov = np.asarray(vmap["foreshortening"], np.float64)[:, int(branch) - 1], np.asarray(vmap["overlap"], np.float64)[:, int(branch) - 1]
    with np.errstate(invalid="ignore"):
        score = fs + float(overlap_weight) * ov
    bad = ~np.isfinite(score)
    if "n_invisible" in vmap:
        bad = bad | (np.asarray(vmap["n_invisible"]) > 0)
    score = np.where(bad, np.nan, score)
    order = np.lexsort((np.arange(score.size), np.where(bad, 0.0, score), bad))      # the last key is the first criterion
    order = order[:max(0, min(int(k), score.size))].astype(np.int64)
    return order, score[order]


# ---- sparse-view algebraic reconstruction: the ray-driven projector (afx_xray_project), the voxel-driven backprojector
# (afx_xray_backproject) and the SIRT iteration made of the two ----
# ---- registering C-arm poses to the vessel silhouettes (afx_pose_chamfer, afx_pose_compose, afx_pose_select, afx_pose_lm_step) ----
POSE_SUM_DOUBLES = 32
POSE_STATE_DOUBLES = 64
POSE_COST_ONLY = 1
POSE_LM_INIT, POSE_LM_UPDATE, POSE_LM_FINAL = 0, 1, 2
POSE_LAMBDA0 = 1e-3
POSE_ST_COST, POSE_ST_LAMBDA, POSE_ST_ACCEPTED, POSE_ST_REJECTED, POSE_ST_SINGULAR, POSE_ST_TRIAL = 16, 44, 45, 46, 47, 48
POSE_DOF = {"all": 63, "rotation": 7, "translation": 56, "inplane": 4 | 8 | 16}      # bits a0 a1 a2 t0 t1 t2 of afx_pose_lm_step's dof_mask


def pose_views(poses, masks: torch.Tensor, focal, signed: bool = True) -> dict:
    """The views a pose is registered against: poses [V, 4, 4] or [V, 3, 4] (cam2world), masks [V, H, W] on the GPU (the vessel
    silhouettes), focal (a number or one per view).  field = EDT(~mask) - EDT(mask), the signed distance in pixels (negative inside the
    silhouette), or with signed=False the hull's unsigned EDT(~mask).  A view with an empty mask is refused, as `visual_hull_views` does.
    -> dict(records float64 [V, 16] and field float64 [V, H, W] on the device, n_views, width, height, poses float64 [V, 4, 4] (host))."""
    import numpy as np
    hull = visual_hull_views(poses, masks, focal, margin_px=0.0)
    field = hull["dist"]
    if signed:
        field = field - distance_transform_edt((masks != 0).to(torch.float64))
    p = np.asarray(poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else poses, dtype=np.float64)
    full = np.tile(np.eye(4), (p.shape[0], 1, 1))
    full[:, :3, :] = p[:, :3, :]
    return dict(records=hull["records"], field=field.contiguous(), n_views=hull["n_views"], width=hull["width"], height=hull["height"], poses=full)


def pose_search_offsets(rot_deg: float, shift: float, steps: int = 3):
    """The in-plane grid of a coarse search -> float64 [steps^3, 6] of increments xi: a2 = tan(theta / 2) for theta in
    linspace(-rot_deg, rot_deg, steps) degrees about the view axis, t0 and t1 in linspace(-shift, shift, steps) world units; a0, a1 and
    t2 are 0.  steps is odd; candidate 0 is the identity (the grid's centre is moved to the front), so a search never raises the cost."""
    import numpy as np
    steps = int(steps)
    if steps < 1 or steps % 2 == 0:
        raise ValueError(f"pose_search_offsets: steps must be odd and >= 1, got {steps}")
    if not (rot_deg >= 0 and shift >= 0 and np.isfinite(rot_deg) and np.isfinite(shift) and rot_deg < 180):
        raise ValueError(f"pose_search_offsets: rot_deg must lie in [0, 180) and shift be finite and >= 0, got {rot_deg!r}, {shift!r}")
    rot = np.tan(np.deg2rad(np.linspace(-rot_deg, rot_deg, steps)) / 2.0)
    sh = np.linspace(-shift, shift, steps)
    rot[steps // 2], sh[steps // 2] = 0.0, 0.0
    grid = np.zeros((steps, steps, steps, 6))
    grid[..., 2], grid[..., 3], grid[..., 4] = rot[:, None, None], sh[None, :, None], sh[None, None, :]
    grid = grid.reshape(-1, 6)
    centre = (steps ** 3) // 2
    return np.ascontiguousarray(np.concatenate([grid[centre:centre + 1], grid[:centre], grid[centre + 1:]]))


def _pose_f64(x, shape, name, dev, who):
    import numpy as np
    if x is None:
        return None
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64)))
    return _buffer(t.to(dev), name, torch.float64, shape, dev, who, exact_shape=True)


def _pose_device(views: dict, who: str):
    return _on_gpu(views["field"], "the views", who).device


def pose_compose(records, xi, outer: bool = False, out=None) -> torch.Tensor:
    """afx_pose_compose: records [R, 16] composed with the increments xi = (a0, a1, a2, t0, t1, t2) in the camera frame (Cayley
    rotation, q' = C(a) q + t) -> [R, 16] with xi [R, 6], or with outer=True and xi [M, 6] every pair, [R, M, 16].  Device tensors in,
    a device tensor out; nothing is read back."""
    lib = _lib.load()
    dev = _on_gpu(records, "the records", "pose_compose").device
    r = records.shape[0]
    records = _pose_f64(records, (r, HULL_VIEW_DOUBLES), "records", dev, "pose_compose")
    m = int(xi.shape[0]) if outer else r
    xi = _pose_f64(xi, (m, 6), "xi", dev, "pose_compose")
    out = _out(out, "out", torch.float64, (r, m, HULL_VIEW_DOUBLES) if outer else (r, HULL_VIEW_DOUBLES), dev, "pose_compose", exact_shape=True)
    _lib.check(lib.afx_pose_compose(_ptr(records), r, _ptr(xi), m if outer else 0, _ptr(out), Engine._stream(dev)), "afx_pose_compose")
    return out


def pose_default_slices(n_points: int, n_records: int) -> int:
    """The slice count `pose_chamfer` and `register_poses` use by default: enough workgroups to fill the device (256 compute units)
    when the records are few, never a slice without a point, at most 64."""
    per = max(1, -(-int(n_points) // 256))
    return int(max(1, min(per, 64, -(-512 // max(1, int(n_records))))))


def pose_chamfer_record(views: dict, points, radius, weight, records, rec_view, trunc: float, n_slices: int = 1, cost_only: bool = False,
                        sums=None, counts=None):
    """afx_pose_chamfer, the launch alone -> (sums float64 [K, S, 32], counts int32 [K, S, 4]) on the device, the slices apart.  points
    float64 [N, 3], radius and weight float64 [N] or None, records float64 [K, 16] and rec_view int32 [K] device tensors.  With sums and
    counts passed nothing is allocated and nothing is read back: the call can be captured in a graph."""
    lib = _lib.load()
    dev = _pose_device(views, "pose_chamfer_record")
    v, w, h = int(views["n_views"]), int(views["width"]), int(views["height"])
    field = _pose_f64(views["field"], (v, h, w), "field", dev, "pose_chamfer_record")
    n, k, s = int(points.shape[0]), int(records.shape[0]), int(n_slices)
    points = _pose_f64(points, (n, 3), "points", dev, "pose_chamfer_record")
    radius = _pose_f64(radius, (n,), "radius", dev, "pose_chamfer_record")
    weight = _pose_f64(weight, (n,), "weight", dev, "pose_chamfer_record")
    records = _pose_f64(records, (k, HULL_VIEW_DOUBLES), "records", dev, "pose_chamfer_record")
    _buffer(rec_view, "rec_view", torch.int32, (k,), dev, "pose_chamfer_record", exact_shape=True)
    ok = k >= 1 and s >= 1
    sums = _out(sums, "sums", torch.float64, (k, s, POSE_SUM_DOUBLES), dev, "pose_chamfer_record", ok=ok, exact_shape=True)
    counts = _out(counts, "counts", torch.int32, (k, s, 4), dev, "pose_chamfer_record", ok=ok, exact_shape=True)
    _lib.check(lib.afx_pose_chamfer(_ptr(field), v, w, h, _ptr(points), _ptr(radius), _ptr(weight), n, _ptr(records), _ptr(rec_view), k,
                                    float(trunc), s, POSE_COST_ONLY if cost_only else 0, _ptr(sums), _ptr(counts), Engine._stream(dev)),
               "afx_pose_chamfer")
    return sums, counts


def _pose_points(points, radius, weight, dev, who):
    import numpy as np
    n = int(points.shape[0])
    if n < 1:
        raise ValueError(f"{who}: no points")
    if radius is not None and not isinstance(radius, torch.Tensor) and np.ndim(radius) == 0:
        radius = np.full(n, float(radius))
    return _pose_f64(points, (n, 3), "points", dev, who), _pose_f64(radius, (n,), "radius", dev, who), _pose_f64(weight, (n,), "weight", dev, who)


def _pose_figures(sums, counts):
    """Host figures of read-back sums [K, S, 32] and counts [K, S, 4]: the slices added in order."""
    import numpy as np
    tot = np.zeros((sums.shape[0], POSE_SUM_DOUBLES))
    for s in range(sums.shape[1]):
        tot = tot + sums[:, s]
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(cost=tot[:, 0], mean_residual=tot[:, 1] / tot[:, 2], rms_residual=np.sqrt(tot[:, 0] / tot[:, 2]),
                    counts=counts.sum(axis=1).astype(np.int64))


def pose_chamfer(points, radius, views: dict, records=None, trunc: float = 8.0, weight=None, n_slices=None) -> dict:
    """The truth-free score of every view's pose: how far the points (the reconstructed centreline; radius in world units or None)
    miss that view's silhouette.  records: [V, 16] to score instead of the views' own.  -> dict of NumPy arrays per view: cost (sum w
    r^2), mean_residual (sum w r / sum w, pixels; a lost or saturated point counts trunc), rms_residual (sqrt(cost / sum w), pixels: the
    figure the registration never raises), counts int64 [V, 4] (active, satisfied, saturated, lost)."""
    dev = _pose_device(views, "pose_chamfer")
    points, radius, weight = _pose_points(points, radius, weight, dev, "pose_chamfer")
    v = int(views["n_views"])
    records = views["records"] if records is None else _pose_f64(records, (v, HULL_VIEW_DOUBLES), "records", dev, "pose_chamfer")
    s = pose_default_slices(points.shape[0], v) if n_slices is None else int(n_slices)
    rec_view = torch.arange(v, dtype=torch.int32, device=dev)
    sums, counts = pose_chamfer_record(views, points, radius, weight, records, rec_view, trunc, s, cost_only=True)
    return _pose_figures(sums.cpu().numpy(), counts.cpu().numpy())


def register_poses_buffers(n_views: int, n_candidates: int, n_slices: int, device) -> dict:
    """Every buffer `register_poses_record` writes, allocated once: with them passed the registration allocates nothing."""
    v, m, s = int(n_views), max(1, int(n_candidates)), int(n_slices)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=device)
    return dict(state=f64(v, POSE_STATE_DOUBLES), trial_records=f64(v, HULL_VIEW_DOUBLES), start=f64(v, HULL_VIEW_DOUBLES),
                sums=f64(v, s, POSE_SUM_DOUBLES), counts=torch.empty((v, s, 4), dtype=torch.int32, device=device),
                cand=f64(v, m, HULL_VIEW_DOUBLES), cand_sums=f64(v * m, s, POSE_SUM_DOUBLES),
                cand_counts=torch.empty((v * m, s, 4), dtype=torch.int32, device=device),
                selected=torch.zeros(v, dtype=torch.int32, device=device), rec_view=torch.arange(v, dtype=torch.int32, device=device),
                cand_view=torch.arange(v, dtype=torch.int32, device=device).repeat_interleave(m).contiguous())


def register_poses_record(views: dict, points, radius, weight, records, iterations: int = 20, trunc: float = 8.0, dof_mask: int = 63,
                          offsets=None, n_slices: int = 1, lambda0: float = POSE_LAMBDA0, buffers=None) -> dict:
    """The whole registration as launches alone: [compose the candidates `offsets` [M, 6] about every record, score them cost-only,
    select] -> score the start -> afx_pose_lm_step INIT -> iterations x [score the trial, step] (the last step FINAL: it solves
    nothing).  All inputs are device tensors; nothing is read back and, with `buffers` (`register_poses_buffers`) passed, nothing is
    allocated: the call can be captured in a graph.  -> the buffers: state [V, 64] (the refined record at [0..15], its cost, lambda and
    the accepted / rejected / singular counts), start [V, 16], selected int32 [V]."""
    lib = _lib.load()
    dev = _pose_device(views, "register_poses_record")
    v, s, it = int(views["n_views"]), int(n_slices), int(iterations)
    if it < 1:
        raise ValueError(f"register_poses_record: iterations must be >= 1, got {iterations}")
    records = _pose_f64(records, (v, HULL_VIEW_DOUBLES), "records", dev, "register_poses_record")
    m = 0 if offsets is None else int(offsets.shape[0])
    b = buffers if buffers is not None else register_poses_buffers(v, m, s, dev)
    stream = Engine._stream(dev)
    if m:
        offsets = _pose_f64(offsets, (m, 6), "offsets", dev, "register_poses_record")
        pose_compose(records, offsets, outer=True, out=b["cand"])
        pose_chamfer_record(views, points, radius, weight, b["cand"].view(v * m, HULL_VIEW_DOUBLES), b["cand_view"], trunc, s, True,
                            b["cand_sums"], b["cand_counts"])
        _lib.check(lib.afx_pose_select(_ptr(b["cand_sums"]), v, m, s, _ptr(b["cand"]), _ptr(b["selected"]), _ptr(b["start"]), stream),
                   "afx_pose_select")
    else:
        b["start"].copy_(records)
        b["selected"].zero_()
    step = lambda phase, rec_in: _lib.check(lib.afx_pose_lm_step(_ptr(b["state"]), v, _ptr(b["sums"]), s, phase, int(dof_mask), float(lambda0),
                                                                  _ptr(rec_in), _ptr(b["trial_records"]), stream), "afx_pose_lm_step")
    pose_chamfer_record(views, points, radius, weight, b["start"], b["rec_view"], trunc, s, False, b["sums"], b["counts"])
    step(POSE_LM_INIT, b["start"])
    for i in range(it):
        pose_chamfer_record(views, points, radius, weight, b["trial_records"], b["rec_view"], trunc, s, False, b["sums"], b["counts"])
        step(POSE_LM_UPDATE if i + 1 < it else POSE_LM_FINAL, None)
    return b


def pose_records_to_matrices(records):
    """View records [V, 16] (NumPy) -> cam2world float64 [V, 4, 4]."""
    import numpy as np
    rec = np.asarray(records, np.float64).reshape(-1, HULL_VIEW_DOUBLES)
    out = np.tile(np.eye(4), (rec.shape[0], 1, 1))
    out[:, :3, :3], out[:, :3, 3] = rec[:, :9].reshape(-1, 3, 3), rec[:, 9:12]
    return out


def pose_projection_shift(points, records_a, records_b, width: int, height: int):
    """The mean pixel displacement of the points between two sets of view records -> float64 [V] (NumPy on the host; points behind a
    source are left out, NaN where none is left)."""
    import numpy as np
    p = np.asarray(points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else points, np.float64).reshape(-1, 3)
    out = []
    for ra, rb in zip(np.asarray(records_a, np.float64), np.asarray(records_b, np.float64)):
        uv = []
        for rec in (ra, rb):
            q = (p - rec[9:12]) @ rec[:9].reshape(3, 3)
            with np.errstate(divide="ignore", invalid="ignore"):
                uv.append((width / 2 + rec[12] * q[:, 0] / -q[:, 2], height / 2 - rec[12] * q[:, 1] / -q[:, 2], -q[:, 2] > 0))
        keep = uv[0][2] & uv[1][2]
        d = np.sqrt((uv[0][0] - uv[1][0]) ** 2 + (uv[0][1] - uv[1][1]) ** 2)[keep]
        out.append(float(d.mean()) if d.size else float("nan"))
    return np.asarray(out)


def register_poses(points, radius, views: dict, iterations: int = 20, trunc: float = 8.0, dof="all", search=None, n_slices=None,
                   weight=None) -> dict:
    """Rigid 2D-3D registration of every view's pose to its silhouette (include/afx.h: afx_pose_chamfer ...): Levenberg-Marquardt on
    the one-sided, truncated chamfer residual of the points (the reconstructed centreline; radius in world units, a number or None)
    against the views' signed distance images (`pose_views`).  dof: "all", "translation", "rotation", "inplane" (a2, t0, t1) or a 6-bit
    mask.  search: None, or (rot_deg, shift, steps) / an [M, 6] array of increments scored first (`pose_search_offsets`; candidate 0
    should be the identity).  -> dict of NumPy arrays: poses [V, 4, 4] and records [V, 16] (refined), cost_before / cost_after,
    mean_residual_before / mean_residual_after and rms_residual_before / rms_residual_after (pixels), counts_before / counts_after, accepted, rejected, singular, selected, shift_px
    (the mean displacement of the points' projections), n_slices."""
    import numpy as np
    dev = _pose_device(views, "register_poses")
    mask = POSE_DOF[dof] if isinstance(dof, str) else int(dof)
    if not 0 <= mask <= 63:
        raise ValueError(f"register_poses: dof must be one of {sorted(POSE_DOF)} or a mask in 0..63")
    points, radius, weight = _pose_points(points, radius, weight, dev, "register_poses")
    v = int(views["n_views"])
    offsets = None
    if search is not None:
        offsets = pose_search_offsets(*search) if isinstance(search, (tuple, list)) and len(search) == 3 and np.ndim(search[0]) == 0 else search
        offsets = _pose_f64(np.asarray(offsets, np.float64).reshape(-1, 6) if not isinstance(offsets, torch.Tensor) else offsets,
                            (len(offsets), 6), "search", dev, "register_poses")
    s = pose_default_slices(points.shape[0], v) if n_slices is None else int(n_slices)
    before = pose_chamfer(points, radius, views, trunc=trunc, weight=weight, n_slices=s)
    b = register_poses_record(views, points, radius, weight, views["records"], iterations, trunc, mask, offsets, s)
    state = b["state"].cpu().numpy()
    rec = np.ascontiguousarray(state[:, :HULL_VIEW_DOUBLES])
    after = pose_chamfer(points, radius, views, records=rec, trunc=trunc, weight=weight, n_slices=s)
    if (before["counts"] < 0).any() or (after["counts"] < 0).any():
        raise AfxError("register_poses: a record was dropped on the device (a view index out of range)")
    given = views["records"].cpu().numpy()
    return dict(poses=pose_records_to_matrices(rec), records=rec, cost_before=before["cost"], cost_after=after["cost"],
                mean_residual_before=before["mean_residual"], mean_residual_after=after["mean_residual"],
                rms_residual_before=before["rms_residual"], rms_residual_after=after["rms_residual"], counts_before=before["counts"],
                counts_after=after["counts"], accepted=state[:, POSE_ST_ACCEPTED].astype(np.int64),
                rejected=state[:, POSE_ST_REJECTED].astype(np.int64), singular=state[:, POSE_ST_SINGULAR].astype(np.int64),
                selected=b["selected"].cpu().numpy(), shift_px=pose_projection_shift(points, given, rec, views["width"], views["height"]),
                n_slices=s)


def centreline_pose_points(graph: dict, index_to_world, radius=None, d2=None, voxel_size=1.0):
    """(points float64 [P, 3], radius float64 [P]) of a `centreline_graph` result, as `view_map` takes them: the path voxels in world
    coordinates and `radius` (one per path voxel or one number) or, by default, voxel_size x sqrt(d2) at the path voxels; without either
    the radius is 0 (the centreline alone)."""
    import numpy as np
    points, _ = centreline_world_points(graph, _affine12(index_to_world, "centreline_pose_points"))
    if radius is None and d2 is not None:
        vox = graph["path_voxels"].cpu().numpy().astype(np.int64)
        radius = np.sqrt(((d2.reshape(-1).cpu().numpy().astype(np.int64) & 0xffffffff)[vox]).astype(np.float64)) * float(voxel_size)
    rad = np.zeros(points.shape[0]) if radius is None else np.broadcast_to(np.asarray(radius, np.float64), (points.shape[0],)).copy()
    return points, rad


def centreline_register_poses(graph: dict, views: dict, index_to_world=None, radius=None, d2=None, voxel_size=1.0, **kw) -> dict:
    """`register_poses` of the centreline of a `centreline_graph` result (`centreline_pose_points`)."""
    points, rad = centreline_pose_points(graph, index_to_world, radius, d2, voxel_size)
    if points.shape[0] == 0:
        raise ValueError("centreline_register_poses: the centreline has no point")
    return register_poses(points, rad, views, **kw)


LABEL_OVERLAP_MAX_LABELS = 4095       # AFX_LABEL_OVERLAP_MAX_LABELS
EDT3D_NONE = 0xffffffff               # AFX_EDT3D_NONE


def feature_transform_record(sites: torch.Tensor, d2=None, nearest=None):
    """afx_feature_transform_3d, the launches alone, on a contiguous uint8 [n0, n1, n2] device mask (non-zero = a site) -> (d2, nearest):
    int32 tensors of the mask's shape, d2 holding the library's uint32 squared distance (0xffffffff as -1: no site), nearest the linear
    index of the nearest site (ties to the lowest index; -1: no site).  With both buffers passed nothing is allocated and nothing is read
    back: the call can be captured in a graph.  There is no workspace: the two outputs are the passes' own storage."""
    lib = _lib.load()
    _volume_on_gpu(sites, "the sites", "feature_transform_3d")
    dev, who = sites.device, "feature_transform_record"
    _buffer(sites, "the sites", torch.uint8, sites.shape, dev, who)
    n0, n1, n2 = sites.shape
    ok = _volume_side_ok(sites.shape)
    d2 = _out(d2 if d2 is None else _on_gpu(d2, "d2", who), "d2", torch.int32, sites.shape, dev, who, ok=ok, exact_shape=True)
    nearest = _out(nearest if nearest is None else _on_gpu(nearest, "nearest", who), "nearest", torch.int32, sites.shape, dev, who, ok=ok,
                   exact_shape=True)
    _lib.check(lib.afx_feature_transform_3d(_ptr(sites), n0, n1, n2, _ptr(d2), _ptr(nearest), Engine._stream(dev)), "afx_feature_transform_3d")
    return d2, nearest


def feature_transform_3d(sites: torch.Tensor):
    """The exact feature transform of a [n0, n1, n2] device tensor (any dtype, non-zero = a site) -> (d2, nearest), both int64
    [n0, n1, n2]: the integer squared distance, in voxels, from every voxel to the nearest site (the library's 0xffffffff without any
    site) and the linear index of that site, the LOWEST index among the sites at that distance (-1 without any site).  d2 equals
    distance_transform_edt_3d(sites == 0, return_squared=True)[1] exactly (include/afx.h: afx_feature_transform_3d)."""
    _volume_on_gpu(sites, "the sites", "feature_transform_3d")
    d2, nearest = feature_transform_record((sites != 0).to(torch.uint8).contiguous())
    return d2.to(torch.int64) & 0xffffffff, nearest.to(torch.int64)


def label_overlap_record(labels: torch.Tensor, a: torch.Tensor, n_labels: int, b=None, index=None, d2=None, max_d2: int = EDT3D_NONE, counts=None,
                         territory=None):
    """afx_label_overlap_3d, the launches alone, on contiguous device tensors of n elements each (any shape): labels int32, a uint8, b
    uint8 or None, index int32 or None, d2 int32 (holding the library's uint32) or None -> (counts int64 [n_labels + 1, 4], territory):
    counts[l] = (voxels, voxels of a, voxels of b, voxels of both) whose label l = labels[index[v]] (labels[v] without index; 0 for a
    negative index, a d2 above max_d2 or a label outside 1..n_labels); territory (int32, written only when passed) = l per voxel.  The
    call zeroes counts itself.  With counts passed nothing is allocated or read back: the call can be captured in a graph."""
    lib = _lib.load()
    who = "label_overlap_record"
    dev, shape, n = _on_gpu(labels, "the labels", "label_overlap_3d").device, tuple(labels.shape), labels.numel()
    for t, name, dtype in ((labels, "labels", torch.int32), (a, "a", torch.uint8), (b, "b", torch.uint8), (index, "index", torch.int32),
                           (d2, "d2", torch.int32), (territory, "territory", torch.int32)):
        if t is not None or name == "a":                  # (a is required: None is refused like any other non-tensor)
            _buffer(_on_gpu(t, name, who), name, dtype, shape, dev, who, exact_shape=True)
    if not 0 <= int(max_d2) <= EDT3D_NONE:
        raise ValueError(f"{who}: max_d2 = {max_d2} must lie in 0..0xffffffff")
    if counts is not None:
        _on_gpu(counts, "counts", who)
    counts = _out(counts, "counts", torch.int64, (int(n_labels) + 1, 4), dev, who, ok=0 <= int(n_labels) <= LABEL_OVERLAP_MAX_LABELS, exact_shape=True)
    _lib.check(lib.afx_label_overlap_3d(_ptr(labels), _ptr(index), _ptr(d2), int(max_d2), _ptr(a), _ptr(b), n, int(n_labels), _ptr(counts),
                                        _ptr(territory), Engine._stream(dev)), "afx_label_overlap_3d")
    return counts, territory


def _u32_in_i32(x: torch.Tensor) -> torch.Tensor:
    """Values 0..2^32 - 1 of any integer dtype as the library's uint32, held in a contiguous int32 tensor."""
    if x.dtype == torch.int32:
        return x.contiguous()
    x = x.to(torch.int64)
    return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32).contiguous()


def label_overlap_3d(labels: torch.Tensor, a: torch.Tensor, b=None, index=None, d2=None, max_d2=None, n_labels=None, return_territory: bool = False):
    """Per-label overlap counts (include/afx.h: afx_label_overlap_3d) -> counts int64 [n_labels + 1, 4] on the device, with
    return_territory (counts, territory int32 of labels' shape).  labels: integer device tensor; a, b: masks of the same shape (non-zero
    = in; b may be None); index: integer tensor of the same shape (e.g. `feature_transform_3d`'s nearest; None: every voxel speaks for
    itself); d2 with max_d2: voxels whose d2 lies above max_d2 go to row 0 (both or neither).  n_labels=None: max(labels), read back.
    counts[l] = (voxels, voxels of a, of b, of both) with label l; row 0 collects what belongs to no label."""
    _on_gpu(labels, "the labels", "label_overlap_3d")
    if (d2 is None) != (max_d2 is None):
        raise ValueError("label_overlap_3d: d2 and max_d2 go together")
    shape, dev = tuple(labels.shape), labels.device
    for name, t in (("a", a), ("b", b), ("index", index), ("d2", d2)):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.device != dev):
            raise ValueError(f"label_overlap_3d: {name} must be a tensor of the labels' shape {shape} on {dev}")
    lab = labels.to(torch.int32).contiguous()
    if n_labels is None:
        n_labels = max(int(lab.max()), 0) if lab.numel() else 0
    mask = lambda m: None if m is None else (m != 0).to(torch.uint8).contiguous()
    territory = torch.empty(shape, dtype=torch.int32, device=dev) if return_territory else None
    counts, _ = label_overlap_record(lab, mask(a), int(n_labels), mask(b), None if index is None else index.to(torch.int32).contiguous(),
                                     None if d2 is None else _u32_in_i32(d2), EDT3D_NONE if max_d2 is None else int(max_d2), territory=territory)
    return (counts, territory) if return_territory else counts


def branch_site_labels(graph: dict):
    """The site labels of `branch_territories` -> (labels int32 [n0, n1, n2], B, K): branch b of a `centreline_graph` result carries
    label b on its path voxels, junction node k label B + k on its voxels, everything else 0."""
    bl, nl = graph["branch_labels"], graph["node_labels"]
    nb, nk = int(graph["n_branches"]), int(graph["n_nodes"])
    return torch.where(bl > 0, bl, torch.where(nl > 0, nl + nb, torch.zeros_like(nl))).to(torch.int32).contiguous(), nb, nk


def branch_territories(graph: dict, max_distance=None) -> dict:
    """The territories of the branches of a `centreline_graph` result: the feature transform (`feature_transform_record`) of the
    centreline's voxels with `branch_site_labels` as their labels -> {"labels" (int32 volume: the sites' labels), "d2", "nearest" (int32
    volumes as the library writes them), "n_branches" B, "n_nodes" K, "n_labels" = B + K, "max_d2" (None, or floor(max_distance^2): a
    voxel farther than max_distance voxels from the centreline belongs to nobody), "names" (B + K strings, "branch b" / "junction k")}.
    A voxel's territory is labels[nearest[v]]: branch b's row is b, junction k's row B + k, so the junction clusters are rows of their
    own and no branch gets their voxels.  `territory_overlap` counts masks over it."""
    labels, nb, nk = branch_site_labels(graph)
    if nb + nk > LABEL_OVERLAP_MAX_LABELS:
        raise ValueError(f"branch_territories: {nb} branches and {nk} junctions are more than {LABEL_OVERLAP_MAX_LABELS} labels")
    if max_distance is not None and not float(max_distance) >= 0.0:
        raise ValueError(f"branch_territories: max_distance = {max_distance} must be >= 0")
    d2, nearest = feature_transform_record((labels > 0).to(torch.uint8))
    max_d2 = None if max_distance is None else min(int(float(max_distance) * float(max_distance)), EDT3D_NONE)
    return {"labels": labels, "d2": d2, "nearest": nearest, "n_branches": nb, "n_nodes": nk, "n_labels": nb + nk, "max_d2": max_d2,
            "names": [f"branch {b}" for b in range(1, nb + 1)] + [f"junction {k}" for k in range(1, nk + 1)], "shape": tuple(labels.shape)}


def territory_overlap(terr: dict, a: torch.Tensor, b=None, return_territory: bool = False, sites_only: bool = False):
    """`label_overlap_3d` of the masks a, b (b may be None) over the territories of a `branch_territories` result -> counts int64
    [B + K + 1, 4] on the device (with return_territory: and the int32 territory volume).  sites_only: every voxel speaks for itself
    (index = None), so only the centreline's own voxels carry a label - a branch's coverage by a mask."""
    if sites_only:
        return label_overlap_3d(terr["labels"], a, b, n_labels=terr["n_labels"], return_territory=return_territory)
    cut = terr["max_d2"] is not None
    return label_overlap_3d(terr["labels"], a, b, index=terr["nearest"], d2=terr["d2"] if cut else None, max_d2=terr["max_d2"] if cut else None,
                            n_labels=terr["n_labels"], return_territory=return_territory)


def line_integrals(images, eps: float = 1e-6) -> torch.Tensor:
    """-log(clamp(I, eps, 1)) in fp64: the line integrals behind transmission images I = exp(-integral), the convention of
    ray_tracing(type='ct')."""
    if not 0.0 < float(eps) <= 1.0:
        raise ValueError(f"line_integrals: eps must lie in (0, 1], got {eps!r}")
    return -torch.log(torch.as_tensor(images).to(torch.float64).clamp(float(eps), 1.0))


def xray_views(poses, focal, width: int, height: int, near: float, far: float, n_samples: int, device=None) -> dict:
    """The views of the SIRT operators: poses [V, 4, 4] or [V, 3, 4] (cam2world), focal (a number, or one per view), the detector
    width x height and the samples of a ray - n_samples of them at near + (s + 0.5) (far - near) / n_samples, common to all views.  The
    records are those of the visual hull (`hull_view_records`), copied to `device` (default: the poses' device when they are a GPU tensor,
    else the current GPU) -> dict(records float64 [V, 16] on the device, n_views, width, height, near, far, n_samples)."""
    import math
    rec = hull_view_records(poses, focal)
    w, h, s = int(width), int(height), int(n_samples)
    if w < 2 or h < 2:
        raise ValueError(f"xray_views: width and height must be at least 2, got {w} x {h}")
    if s < 1:
        raise ValueError(f"xray_views: n_samples must be positive, got {s}")
    if not (math.isfinite(near) and math.isfinite(far) and far > near):
        raise ValueError(f"xray_views: near and far must be finite with far > near, got {near!r}, {far!r}")
    if device is None:
        device = poses.device if isinstance(poses, torch.Tensor) and poses.device.type == "cuda" else torch.device("cuda")
    if torch.device(device).type != "cuda":
        raise AfxError("xray_views: the views must live on a GPU; there is no CPU path")
    return dict(records=torch.from_numpy(rec).to(device), n_views=rec.shape[0], width=w, height=h, near=float(near), far=float(far), n_samples=s)


def _xray_views_checked(views: dict, who: str):
    rec = views["records"]
    dev, v = _on_gpu(rec, "the views", who).device, int(views["n_views"])
    _buffer(rec, "records", torch.float64, (v, HULL_VIEW_DOUBLES), dev, who, exact_shape=True)
    return rec, dev, v, int(views["width"]), int(views["height"])


def xray_project(volume: torch.Tensor, views: dict, index_to_world=None, target=None, weight=None, out=None) -> torch.Tensor:
    """afx_xray_project: the line integrals of the float64 [n0, n1, n2] device `volume`, trilinearly interpolated on the lattice
    x = index_to_world (i, j, k, 1), along every ray of `views` (`xray_views`) -> float64 [V, H, W]; with target and weight (both
    [V, H, W] float64) the fused weighted residual weight (target - y) instead.  The definition stands in include/afx.h.  One launch;
    with `out` passed nothing is allocated and the call can be captured in a graph."""
    import numpy as np
    lib = _lib.load()
    rec, dev, v, w, h = _xray_views_checked(views, "xray_project")
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3:
        raise ValueError("xray_project: the volume must be a [n0, n1, n2] tensor")
    _buffer(volume, "the volume", torch.float64, volume.shape, dev, "xray_project")
    if (target is None) != (weight is None):
        raise ValueError("xray_project: target and weight are given together or not at all")
    b = np.ascontiguousarray(lumen_world_to_index(_affine12(index_to_world, "xray_project")))
    if target is not None:
        _buffer(target, "target", torch.float64, (v, h, w), dev, "xray_project"), _buffer(weight, "weight", torch.float64, (v, h, w), dev, "xray_project")
    out = _out(out, "out", torch.float64, (v, h, w), dev, "xray_project")
    n0, n1, n2 = volume.shape
    _lib.check(lib.afx_xray_project(_ptr(volume), n0, n1, n2, b.ctypes.data_as(C.POINTER(C.c_double)), _ptr(rec), v, w, h, float(views["near"]),
                                    float(views["far"]), int(views["n_samples"]), _ptr(target), _ptr(weight), _ptr(out), Engine._stream(dev)),
               "afx_xray_project")
    return out


def xray_backproject(images: torch.Tensor, views: dict, shape, index_to_world=None, x_inout=None, relax: float = 1.0, nonneg: bool = False,
                     mask=None, acc=None, seen=None):
    """afx_xray_backproject: every point of the lattice x = index_to_world (i, j, k, 1) of `shape` gathers the bilinear value of the
    float64 [V, H, W] device `images` at its projection into every view that sees it (include/afx.h).  Without x_inout -> (acc float64,
    seen uint16) of `shape`: the sum over the views and their number.  With x_inout (float64, `shape`) the SIRT update is fused, in
    place: x += relax acc / seen (0 where no view sees the point), clamped at 0 with nonneg, zeroed where the uint8 `mask` is 0 ->
    x_inout; acc and seen are written only when passed.  One launch, nothing read back: capturable."""
    import numpy as np
    lib = _lib.load()
    rec, dev, v, w, h = _xray_views_checked(views, "xray_backproject")
    n0, n1, n2 = (int(s) for s in shape)
    n = max(n0, 0) * max(n1, 0) * max(n2, 0)
    if images is None:
        raise ValueError("xray_backproject: images must be a float64 [V, H, W] tensor")
    _buffer(images, "images", torch.float64, (v, h, w), dev, "xray_backproject")
    a = np.ascontiguousarray(_affine12(index_to_world, "xray_backproject"))
    if x_inout is None:
        if mask is not None:
            raise ValueError("xray_backproject: mask belongs to the fused update (x_inout)")
        acc = torch.empty((n0, n1, n2), dtype=torch.float64, device=dev) if acc is None else acc
        seen = torch.empty((n0, n1, n2), dtype=torch.uint16, device=dev) if seen is None else seen
    for t, name, dtype in ((acc, "acc", torch.float64), (x_inout, "x_inout", torch.float64), (seen, "seen", torch.uint16), (mask, "mask", torch.uint8)):
        if t is not None:
            _buffer(t, name, dtype, n, dev, "xray_backproject")
    _lib.check(lib.afx_xray_backproject(_ptr(images), _ptr(rec), v, w, h, n0, n1, n2, a.ctypes.data_as(C.POINTER(C.c_double)), _ptr(acc),
                                        _ptr(seen), _ptr(x_inout), float(relax), int(bool(nonneg)), _ptr(mask), Engine._stream(dev)),
               "afx_xray_backproject")
    return x_inout if x_inout is not None else (acc, seen)


def sirt_residual_norm(residual: torch.Tensor) -> torch.Tensor:
    """sqrt(sum r^2) of weighted residual images, a 0-d float64 tensor on their device: the entry of sirt_reconstruct's history."""
    return torch.sqrt(torch.sum(residual * residual))


def tv_denoise_3d_workspace(shape, device) -> torch.Tensor:
    """The workspace of `tv_denoise_3d` for a volume of `shape`: afx_tv_denoise_3d_workspace_bytes (six volumes) as a uint8 tensor."""
    n0, n1, n2 = (int(s) for s in shape)
    return torch.empty(_lib.load().afx_tv_denoise_3d_workspace_bytes(n0, n1, n2), dtype=torch.uint8, device=device)


def tv_denoise_3d(x: torch.Tensor, weight: float, iterations: int = 50, tau: float = 1.0 / 6.0, nonneg: bool = False, mask=None, out=None,
                  workspace=None) -> torch.Tensor:
    """afx_tv_denoise_3d: the float64 [n0, n1, n2] device volume `x` denoised by the proximal operator of the isotropic total variation,
    argmin_u 0.5 sum (u - x)^2 + weight TV(u) (Rudin-Osher-Fatemi), `iterations` of Chambolle's dual iteration at the step tau from
    p = 0 (include/afx.h holds the definition) -> float64 of x's shape; clamped at 0 with nonneg, zeroed where the uint8 or bool `mask`
    of x's shape is 0.  out may be x.  One launch per iteration and one more; with `out` and `workspace` (`tv_denoise_3d_workspace`)
    passed nothing is allocated and the call can be captured in a graph."""
    lib = _lib.load()
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError("tv_denoise_3d: x must be a [n0, n1, n2] tensor")
    dev, who = _on_gpu(x, "the volume", "tv_denoise_3d").device, "tv_denoise_3d"
    _buffer(x, "x", torch.float64, x.shape, dev, who)
    out = _out(out, "out", torch.float64, x.shape, dev, who)
    if mask is not None:
        mask = _buffer(mask, "mask", (torch.uint8, torch.bool), x.shape, dev, who, exact_shape=True).view(torch.uint8)      # (bool: the same bytes)
    n0, n1, n2 = x.shape
    nbytes = 0
    if workspace is not None or int(iterations) > 0:
        workspace, nbytes = _scratch(workspace, lib.afx_tv_denoise_3d_workspace_bytes(n0, n1, n2), dev, who)
    _lib.check(lib.afx_tv_denoise_3d(_ptr(x), n0, n1, n2, float(weight), float(tau), int(iterations), int(bool(nonneg)), _ptr(mask), _ptr(out),
                                     _ptr(workspace), nbytes, Engine._stream(dev)), "afx_tv_denoise_3d")
    return out


def total_variation_3d(x: torch.Tensor) -> torch.Tensor:
    """The isotropic total variation of a [n0, n1, n2] volume: the sum over the voxels of sqrt(g_0^2 + g_1^2 + g_2^2), g_a the forward
    difference along axis a (0 on the last layer), in fp64 -> a 0-d tensor on x's device.  Plain torch: a figure to report, the sum in
    torch's order."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError("total_variation_3d: x must be a [n0, n1, n2] tensor")
    u = x.to(torch.float64)
    sq = torch.zeros_like(u)
    sq[:-1] += (u[1:] - u[:-1]) ** 2
    sq[:, :-1] += (u[:, 1:] - u[:, :-1]) ** 2
    sq[:, :, :-1] += (u[:, :, 1:] - u[:, :, :-1]) ** 2
    return torch.sqrt(sq).sum()


def sirt_reconstruct(views: dict, line_integrals: torch.Tensor, shape, index_to_world=None, iterations: int = 50, relax: float = 1.0,
                     mask=None, x0=None, nonneg: bool = True, return_history: bool = False, tv_weight=None, tv_iterations: int = 10):
    """SIRT: the attenuation volume on the lattice x = index_to_world (i, j, k, 1) of `shape` whose line integrals along the rays of
    `views` (`xray_views`) approach `line_integrals` (float64 [V, H, W] on the GPU; `line_integrals(I)` of transmission images) ->
    float64 `shape`[, history float64 [iterations] on the host].

    Once: l = xray_project(ones), weight = where(l > 0, 1 / l, 0) - the row weights; l is the chord of the ray through the lattice.  Each
    iteration is two launches: r = weight (b - project(x)) (the fused residual) and x += relax backproject(r) / seen, clamped at 0 with
    nonneg and zeroed outside `mask` (bool or uint8, `shape`: a support constraint such as the visual hull) - the fused update; every
    voxel takes the mean of its residuals over the views that see it.  x0: the start volume (default zeros; it is not changed).  The
    buffers are allocated once and nothing is read back inside the loop; return_history adds `sirt_residual_norm` of each iteration's
    residual images (those of the volume BEFORE the iteration's update), read back once at the end.

    tv_weight (default None: plain SIRT, the launches above and nothing else): SIRT-TV - every update is followed by
    `tv_denoise_3d(x, tv_weight, tv_iterations, nonneg=nonneg, mask=mask, out=x)`, in place, its dual fields from zero every time, its
    workspace allocated once before the loop."""
    import math
    rec, dev, v, w, h = _xray_views_checked(views, "sirt_reconstruct")
    shape = tuple(int(s) for s in shape)
    if int(iterations) < 0:
        raise ValueError(f"sirt_reconstruct: iterations must be >= 0, got {iterations}")
    if tv_weight is not None and not (math.isfinite(tv_weight) and tv_weight > 0 and int(tv_iterations) >= 0):
        raise ValueError(f"sirt_reconstruct: tv_weight must be finite and > 0 and tv_iterations >= 0, got {tv_weight!r}, {tv_iterations!r}")
    if not isinstance(line_integrals, torch.Tensor) or line_integrals.device != dev:
        raise AfxError("sirt_reconstruct: the line integrals must live on the views' GPU; there is no CPU path")
    b = line_integrals.to(torch.float64).contiguous()
    if tuple(b.shape) != (v, h, w):
        raise ValueError(f"sirt_reconstruct: line_integrals must be [{v}, {h}, {w}], got {tuple(b.shape)}")
    m8 = None
    if mask is not None:
        if tuple(mask.shape) != shape:
            raise ValueError(f"sirt_reconstruct: mask must have the shape {shape}, got {tuple(mask.shape)}")
        m8 = (mask != 0).to(device=dev, dtype=torch.uint8).contiguous()
    if x0 is None:
        x = torch.zeros(shape, dtype=torch.float64, device=dev)
    else:
        if tuple(x0.shape) != shape:
            raise ValueError(f"sirt_reconstruct: x0 must have the shape {shape}, got {tuple(x0.shape)}")
        x = x0.to(device=dev, dtype=torch.float64).contiguous().clone()
    ell = xray_project(torch.ones(shape, dtype=torch.float64, device=dev), views, index_to_world)
    weight = torch.where(ell > 0, 1.0 / ell, torch.zeros_like(ell))
    residual = ell                                        # (the buffer of the residual images; l is not needed any more)
    history = torch.zeros(int(iterations), dtype=torch.float64, device=dev) if return_history else None
    tv_workspace = tv_denoise_3d_workspace(shape, dev) if tv_weight is not None and int(tv_iterations) > 0 else None
    for it in range(int(iterations)):
        xray_project(x, views, index_to_world, target=b, weight=weight, out=residual)
        if history is not None:
            history[it] = sirt_residual_norm(residual)
        xray_backproject(residual, views, shape, index_to_world, x_inout=x, relax=relax, nonneg=nonneg, mask=m8)
        if tv_weight is not None:
            tv_denoise_3d(x, tv_weight, tv_iterations, nonneg=nonneg, mask=m8, out=x, workspace=tv_workspace)
    return (x, history.cpu()) if return_history else x


class RayBatchSampler:
    """sample_rays for a training loop: the batches of `prefetch` consecutive iterations are drawn by ONE launch sequence
    (afx_sample_batches; a single draw is launch latency, ~70 us of the reference's 1.3 ms iteration) and handed out one per call.
    draw(stream_id) returns exactly what sample_rays(origins, dirs, pixels, weights, k, seed=seed, stream_id=stream_id) returns; stream ids
    are expected to advance by one per iteration (any other id starts a new block of `prefetch` draws at that id)."""

    def __init__(self, origins, dirs, pixels, weights, k, seed=0, prefetch=16):
        self.lib = _lib.load()
        dev, who = origins.device, "RayBatchSampler"
        self.origins, self.dirs, self.weights, self.pixels = (t if t is None else _buffer(t, name, torch.float32, None, dev, who, copy=True) for t, name in
                                                              ((origins, "origins"), (dirs, "dirs"), (weights, "weights"), (pixels, "pixels")))
        n = self.origins.shape[0]
        if tuple(self.origins.shape) != (n, 3) or tuple(self.dirs.shape) != (n, 3) or self.weights.numel() != n \
                or (self.pixels is not None and self.pixels.numel() != n):
            raise ValueError("RayBatchSampler: expected origins/dirs [n,3], pixels/weights [n]")
        _on_gpu(origins, "origins", who)
        if not 0 < int(k) <= n or not 1 <= int(prefetch) <= 65535:
            raise ValueError("RayBatchSampler: need 0 < k <= n and 1 <= prefetch <= 65535")
        self.n, self.k, self.seed, self.prefetch, self.dev = n, int(k), int(seed), int(prefetch), dev
        self._ws, self._ws_bytes = _scratch(None, self.lib.afx_sample_batches_workspace_bytes(n, self.prefetch), dev, "RayBatchSampler")
        self._idx = torch.empty(self.prefetch, self.k, dtype=torch.int64, device=dev)
        self._first = None      # stream id of row 0 of _idx

    def draw(self, stream_id):
        stream_id = int(stream_id)
        st = Engine._stream(self.dev)
        if self._first is None or not self._first <= stream_id < self._first + self.prefetch:
            _lib.check(self.lib.afx_sample_batches(_ptr(self.weights), self.n, self.seed, stream_id, self.prefetch, self.k, _ptr(self._idx),
                                                   _ptr(self._ws), self._ws_bytes, st), "afx_sample_batches")
            self._first = stream_id
        idx = self._idx[stream_id - self._first]
        o, d = torch.empty(self.k, 3, device=self.dev), torch.empty(self.k, 3, device=self.dev)
        p = torch.empty(self.k, device=self.dev) if self.pixels is not None else None
        _lib.check(self.lib.afx_gather_rays(_ptr(self.origins), _ptr(self.dirs), _ptr(self.pixels), _ptr(idx), self.k, _ptr(o), _ptr(d), _ptr(p), st),
                   "afx_gather_rays")
        return o, d, p, idx


def sample_batches_workspace_bytes(n: int, n_batches: int) -> int:
    return int(_lib.load().afx_sample_batches_workspace_bytes(int(n), int(n_batches)))


def sample_batches_dev(weights, seed: int, stream_id0_dev, n_batches: int, k: int, out_idx=None, workspace=None):
    """afx_sample_batches_dev: the index rows of `n_batches` consecutive draws, out_idx[b] = the draw of Philox stream (seed, stream_id0_dev + b)
    - what RayBatchSampler / sample_rays draw for that stream id, index for index - with the first id read from a 0-dim int64 device tensor
    when the kernels run.  Launches only: a graph captured over the call follows the counter.  Pass out_idx [n_batches, k] (int64) and a
    workspace of sample_batches_workspace_bytes(n, n_batches) bytes to reuse static buffers.  Returns out_idx."""
    lib = _lib.load()
    dev, who = weights.device, "sample_batches_dev"
    weights = _buffer(weights, "weights", torch.float32, None, dev, who, copy=True)
    n, n_batches, k = weights.numel(), int(n_batches), int(k)
    if not torch.is_tensor(stream_id0_dev):
        raise ValueError("sample_batches_dev: the first stream id must be a 0-dim int64 device tensor (RayBatchSampler takes host ids)")
    _, step_d = _step_args(stream_id0_dev, dev, who)
    out_idx = _out(out_idx, "out_idx", torch.int64, (max(n_batches, 0), max(k, 0)), dev, who)
    _on_gpu(weights, "weights", who)
    workspace, nbytes = _scratch(workspace, 0 if workspace is not None else lib.afx_sample_batches_workspace_bytes(n, max(n_batches, 1)), dev, who)
    _lib.check(lib.afx_sample_batches_dev(_ptr(weights), n, int(seed), step_d, n_batches, k, _ptr(out_idx), _ptr(workspace), nbytes,
                                          Engine._stream(dev)), "afx_sample_batches_dev")
    return out_idx


def gather_rays(origins, dirs, pixels, idx, origins_out, dirs_out, pixels_out):
    """afx_gather_rays into the caller's buffers: rows idx [k] (int64) of a float32 ray table [n,3], [n,3], [n].  The VALUES of idx are
    not checked (that would need a device read): every index must lie in [0, n)."""
    lib = _lib.load()
    dev, who, n = origins.device, "gather_rays", origins.shape[0]
    _buffer(origins, "origins", torch.float32, (n, 3), dev, who, exact_shape=True)
    _buffer(dirs, "dirs", torch.float32, (n, 3), dev, who, exact_shape=True)
    k = _buffer(idx, "idx", torch.int64, None, dev, who).numel()
    _buffer(origins_out, "origins_out", torch.float32, (k, 3), dev, who)
    _buffer(dirs_out, "dirs_out", torch.float32, (k, 3), dev, who)
    if pixels is not None:      # (either may be None: the kernel copies the pixels when it has both)
        _buffer(pixels, "pixels", torch.float32, n, dev, who)
    if pixels_out is not None:
        _buffer(pixels_out, "pixels_out", torch.float32, k, dev, who)
    _on_gpu(origins, "origins", who)
    _lib.check(lib.afx_gather_rays(_ptr(origins), _ptr(dirs), _ptr(pixels), _ptr(idx), k, _ptr(origins_out), _ptr(dirs_out),
                                   _ptr(pixels_out), Engine._stream(dev)), "afx_gather_rays")


def train_round_advance(step_dev, lr_table, lr_dev, skip, loss, counts, loss_hist, counts_hist, skip_hist, last_loss, n_marched):
    """afx_train_round_advance: the bookkeeping behind one captured grid iteration, on the device (include/afx.h) - the next learning rate
    from `lr_table`, the step's loss / counts / skip flag into slot step % round_len of the history (round_len = loss_hist.numel()),
    last_loss, n_marched, step + 1.  Every argument is a device tensor: int64 step_dev [1], counts [3], counts_hist [round_len, 3],
    n_marched [1]; float32 the rest (lr_table of any length)."""
    lib = _lib.load()
    dev, L = step_dev.device, loss_hist.numel()
    spec = (("step_dev", step_dev, torch.int64, 1), ("lr_table", lr_table, torch.float32, None), ("lr_dev", lr_dev, torch.float32, 1),
            ("skip", skip, torch.float32, 1), ("loss", loss, torch.float32, 1), ("counts", counts, torch.int64, 3),
            ("loss_hist", loss_hist, torch.float32, L), ("counts_hist", counts_hist, torch.int64, 3 * L), ("skip_hist", skip_hist, torch.float32, L),
            ("last_loss", last_loss, torch.float32, 1), ("n_marched", n_marched, torch.int64, 1))
    a = _lib.TrainRoundArgs()
    a.n_table, a.round_len = lr_table.numel(), L
    for name, t, dt, n in spec:
        setattr(a, name, _buffer(t, name, dt, n, dev, "train_round_advance").data_ptr())
    _on_gpu(step_dev, "step_dev", "train_round_advance")
    _lib.check(lib.afx_train_round_advance(C.byref(a), Engine._stream(dev)), "afx_train_round_advance")


def sample_rays(origins, dirs, pixels, weights, k, u=None, seed=0, stream_id=0):
    """Weighted sample WITHOUT replacement of k rows of a device-resident ray table (sample_pixel_rays, nerf_helpers.py:137-150):
    Efraimidis-Spirakis keys log(u)/w, radix-select top-k on the device (afx_topk_indices), gather.  Returns (origins[k,3], dirs[k,3], pixels[k] | None, idx)."""
    lib = _lib.load()
    dev, who = origins.device, "sample_rays"
    # (row-major [n,3] tables: a frame's `df[[x, y, z]].to_numpy()` is usually column-major, and .float().to(device) keeps those strides)
    origins, dirs, weights, pixels, u = (t if t is None else _buffer(t, name, torch.float32, None, dev, who, copy=True) for t, name in
                                         ((origins, "origins"), (dirs, "dirs"), (weights, "weights"), (pixels, "pixels"), (u, "u")))
    n = origins.shape[0]
    if tuple(origins.shape) != (n, 3) or tuple(dirs.shape) != (n, 3) or weights.numel() != n or (pixels is not None and pixels.numel() != n) \
            or (u is not None and u.numel() != n):
        raise ValueError("sample_rays: expected origins/dirs [n,3], pixels/weights/u [n]")
    _on_gpu(origins, "origins", who)
    keys = torch.empty(n, device=dev)
    st = Engine._stream(dev)
    _lib.check(lib.afx_sample_keys(_ptr(weights), n, _ptr(u), int(seed), int(stream_id), _ptr(keys), st), "afx_sample_keys")
    idx = topk_indices(keys, int(k))      # ascending table order: the batch is a set
    o, d = torch.empty(int(k), 3, device=dev), torch.empty(int(k), 3, device=dev)
    p = torch.empty(int(k), device=dev) if pixels is not None else None
    _lib.check(lib.afx_gather_rays(_ptr(origins), _ptr(dirs), _ptr(pixels), _ptr(idx), int(k), _ptr(o), _ptr(d), _ptr(p), st),
               "afx_gather_rays")
    return o, d, p, idx
