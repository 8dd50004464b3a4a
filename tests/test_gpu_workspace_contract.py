"""The caller-workspace contract of every entry point of include/afx.h that takes a workspace (TABLE below; the host side - the table
against the header, the alignment rule - is tests/test_workspace_contract_cpu.py).  Per entry point, on the smallest inputs at which its
kernels still run more than one block and more than one chunk of their two-level passes (ragged tails on purpose):

  baseline  the workspace is the interior of a guard-banded arena (tests/workspace_contract.py) of exactly *_workspace_bytes bytes, zero
            filled, every output buffer that the caller can pass a zero-filled arena of its own; the result R0 is checked against the
            operation's reference with the helper or bar of the operation's own GPU test (imported, not restated);
  fills     0xFF, random bytes and "stale" - the arena as the same operation left it after a call on a larger and denser input, not
            refilled: the specified part of every output equals R0 bit for bit (these operations assert run-to-run equality in their
            own tests, and include/afx.h promises it of all of them: "results are deterministic: no floating-point atomics anywhere"),
            and no guard byte of the workspace or of any output changed;
  one short workspace_bytes = need - 1 is refused on the host with the operation's code; workspace, outputs and guards untouched;
  capacity  the outputs with a caller capacity lie in arenas of exactly that capacity: afx_isosurface_3d at exactly V and T (below them:
            tests/test_gpu_isosurface.py, tests/test_gpu_many_chunks.py), afx_centreline_graph at B, below it and far below it
            (test_centreline_graph_capacity_below_and_at_the_count), afx_grid_select_cells with n_draw below and above the occupied
            count, afx_topk_indices at k and afx_sample_batches at n_batches x k.

Outputs without a guard band: those that the engine's method allocates itself and takes no buffer for - pixel and kept_counts of
afx_march_render, pixel and z_all of afx_hier_train_step_mse, pixel of afx_train_step_packed_mse and of the forward render in front of
afx_render_backward_inputs.  Their values are compared under every fill all the same; grad_flat, d_pts, d_origins and d_dirs of these
entry points lie in arenas, as does every output of every other entry point.

The "specified part" of an output is what include/afx.h says is written: rows below min(count, capacity), everything of a dense output.

Run with -m gpu on an MI355X."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import workspace_contract as wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2

# Volumes: 2 048-voxel chunks of the labelling, thinning and graph kernels (CC_CHUNK, SK_CHUNK, CG_CHUNK), 1 024-point chunks of the
# isosurface scan.  SMALL: 29 667 voxels = 14.5 chunks of 2 048, 29 of 1 024, every extent odd; LARGE (the stale call's): 48 840.
SMALL, LARGE = (33, 31, 29), (40, 37, 33)
IMG_SMALL, IMG_LARGE = (3, 37, 53), (5, 45, 61)             # 2-D images: 1 961 pixels (7.7 blocks of 256; 2 x 1 SSIM tiles), batches of 3


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)            # (a copy: the cached inputs are read-only)


def _lib():
    from nerf_for_angiography_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------- the driver
class Case:
    """One entry point on one pair of inputs.  `inputs(which)`: "small" (the one that is checked) or "large" (what the stale arena is
    primed with).  `call` raises AfxError or returns the C return code."""
    entry = ""
    code = AFX_E_WORKSPACE

    def inputs(self, which):
        raise NotImplementedError

    def need(self, inp):
        raise NotImplementedError

    def out_specs(self, inp):
        """name -> (shape, dtype) of every output buffer"""
        raise NotImplementedError

    def call(self, inp, ws, outs):
        raise NotImplementedError

    def specified(self, inp, outs):
        """name -> the part of each output that include/afx.h says is written (default: everything)"""
        return dict(outs)

    def prepare(self, inp, outs):
        """the start state of outputs that are updated in place (default: none is)"""

    def baseline(self, inp, spec):
        raise NotImplementedError


def _rc(case, inp, ws, outs):
    from nerf_for_angiography_amd._lib import AfxError
    try:
        rc = case.call(inp, ws, outs)
    except AfxError as e:
        m = re.search(r"failed \((-?\d+)\)", str(e))
        assert m, str(e)
        return int(m.group(1))
    return 0 if rc is None else int(rc)


def _out_arenas(case, inp, fill, seed):
    wholes, outs = {}, {}
    for i, (name, (shape, dtype)) in enumerate(case.out_specs(inp).items()):
        wholes[name], outs[name] = wc.typed_arena(shape, dtype, fill, DEV, seed + 1 + i)
    case.prepare(inp, outs)
    return wholes, outs


def _guards_of_outputs(wholes, outs, before, what):
    for name, whole in wholes.items():
        nbytes = outs[name].numel() * outs[name].element_size()
        assert wc.guards_intact(whole, nbytes, before[name]), (what, "guard of output", name)


def _run(case, inp, fill, ws_arena=None, seed=0):
    """One call in arenas painted with `fill` -> clones of the specified parts.  ws_arena: (whole, interior) to use as it is."""
    need = case.need(inp)
    whole, ws = wc.arena(need, fill, DEV, seed) if ws_arena is None else ws_arena
    assert ws.numel() >= need > 0 and ws.data_ptr() % 256 == 0
    wholes, outs = _out_arenas(case, inp, fill, seed)
    before_ws = whole.clone()
    before = {k: v.clone() for k, v in wholes.items()}
    rc = _rc(case, inp, ws, outs)
    torch.cuda.synchronize()
    what = (case.entry, fill)
    assert rc == 0, (what, rc, _lib()[1].afx_last_error())
    assert wc.guards_intact(whole, ws.numel(), before_ws), (what, "guard of the workspace")
    _guards_of_outputs(wholes, outs, before, what)
    return {k: v.clone() for k, v in case.specified(inp, outs).items()}


def _same(case, fill, got, want):
    assert got.keys() == want.keys()
    for name in want:
        assert wc.same_bits(got[name], want[name]), (case.entry, fill, name, "differs from the zero-filled run")


def check_contract(case):
    small, large = case.inputs("small"), case.inputs("large")
    need = case.need(small)
    r0 = _run(case, small, 0x00)
    case.baseline(small, r0)
    for fill in (0xFF, "random"):
        _same(case, fill, _run(case, small, fill, seed=3), r0)
    # stale: the larger call, then the small one in the same arena, not refilled (workspace_bytes stays at the arena's size)
    arena = wc.arena(max(need, case.need(large)), "stale", DEV, seed=5)
    _run(case, large, "stale", ws_arena=arena, seed=5)
    _same(case, "stale", _run(case, small, "stale", ws_arena=arena, seed=7), r0)
    # one byte short: refused on the host, nothing touched
    whole, ws = wc.arena(need, 0xFF, DEV)
    wholes, outs = _out_arenas(case, small, 0xFF, 0)
    before_ws, before = whole.clone(), {k: v.clone() for k, v in wholes.items()}
    rc = _rc(case, small, ws[:need - 1], outs)
    torch.cuda.synchronize()
    assert rc == case.code, (case.entry, "one byte short", rc)
    assert torch.equal(whole, before_ws), (case.entry, "a refused call wrote to the workspace")
    for name in wholes:
        assert torch.equal(wholes[name], before[name]), (case.entry, "a refused call wrote to", name)


# ---------------------------------------------------------------- shared inputs and references (computed once)
@functools.lru_cache(maxsize=None)
def _mask(which):
    """bool volume: the sparse capsule-and-speck volume of the many-chunk tests at SMALL; at LARGE the same with a denser random mask on top."""
    import many_chunks_cases as mc
    if which == "small":
        return mc.sparse_volume(SMALL)
    m = mc.sparse_volume(LARGE) | (np.random.default_rng(17).random(LARGE) < 0.12)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _blob(which):
    """bool volume for the thinning, graph and pruning cases: smoothed noise (skeleton_reference.smooth_noise) - nine thinning passes, a
    skeleton of 143 branches over 382 path voxels and three pruning rounds at SMALL; at LARGE more of the volume is foreground."""
    import skeleton_reference as sk
    m = sk.smooth_noise(SMALL, 3) if which == "small" else sk.smooth_noise(LARGE, 4, fraction=0.5)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _skeleton():
    """(reference skeleton, reference record) of the small blob"""
    import skeleton_reference as sk
    return sk.skeletonize(_blob("small"))


@functools.lru_cache(maxsize=None)
def _d2(which):
    import graph_reference as gr
    return gr.squared_edt(_blob(which))


@functools.lru_cache(maxsize=None)
def _large_skeleton():
    """uint8 device volume: the device's own skeleton of the large blob (only ever the stale call's input: more branches, nodes and path
    voxels than the small case has)"""
    from nerf_for_angiography_amd.engine import skeletonize_3d
    return skeletonize_3d(_dev(_blob("large"))).to(torch.uint8).contiguous()


def _d2_dev(d2):
    return _dev(np.asarray(d2, np.int64).astype(np.uint32).view(np.int32).reshape(np.shape(d2)))


@functools.lru_cache(maxsize=None)
def _images(which):
    """float64 [n, h, w]: blurred dark line segments on a bright background (vesselness_reference.vessel_image)"""
    import vesselness_reference as vr
    n, h, w = IMG_SMALL if which == "small" else IMG_LARGE
    x = np.stack([vr.vessel_image(h, w, seed=10 * (which == "large") + i, n_lines=4 if which == "small" else 9) for i in range(n)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference_mesh(which):
    """(float32 field, affine, reference isosurface) of the mask at level 0.5 under the swapped affine"""
    import isosurface_reference as iso
    from test_isosurface_cpu import SWAPPED
    f = _mask(which).astype(np.float32)
    return f, SWAPPED, (iso.isosurface(f, 0.5, SWAPPED) if which == "small" else None)


SIGMAS_2D = (1.0, 3.0, 5.0)


def _sigmas(s):
    return (C.c_double * len(s))(*[float(v) for v in s]), len(s)


# ---------------------------------------------------------------- the 2-D image family (C entry points: the wrappers take no workspace)
class Frangi2D(Case):
    entry = "afx_frangi"

    def inputs(self, which):
        return {"x": _dev(_images(which)), "which": which}

    def need(self, inp):
        return int(_lib()[1].afx_frangi_workspace_bytes(*inp["x"].shape, len(SIGMAS_2D)))

    def out_specs(self, inp):
        return {"out": (tuple(inp["x"].shape), torch.float64)}

    def call(self, inp, ws, outs):
        sg, ns = _sigmas(SIGMAS_2D)
        n, h, w = inp["x"].shape
        return _lib()[1].afx_frangi(_p(inp["x"]), n, h, w, sg, ns, 0.5, 15.0, 1, _p(outs["out"]), _p(ws), ws.numel(), None, _stream())

    def baseline(self, inp, spec):
        import vesselness_reference as vr
        from test_gpu_vesselness import _check_frangi, _frangi_bar
        got = spec["out"].cpu().numpy()
        for i, im in enumerate(_images("small")):            # 37 x 53 is a small image: the bar follows the restatement's own sensitivity
            _check_frangi(got[i:i + 1], vr.frangi(im, sigmas=SIGMAS_2D)[None], (self.entry, i), rel=_frangi_bar(im, sigmas=SIGMAS_2D))


class Edt2D(Case):
    entry = "afx_distance_transform_edt"

    @staticmethod
    def _masks(which):
        x = _images(which)
        return (x > np.quantile(x, 0.15 if which == "small" else 0.4)).astype(np.float64)      # zero on the vessels: distances of many pixels

    def inputs(self, which):
        return {"x": _dev(self._masks(which))}

    def need(self, inp):
        return int(_lib()[1].afx_distance_transform_edt_workspace_bytes(*inp["x"].shape))

    def out_specs(self, inp):
        return {"out": (tuple(inp["x"].shape), torch.float64)}

    def call(self, inp, ws, outs):
        n, h, w = inp["x"].shape
        return _lib()[1].afx_distance_transform_edt(_p(inp["x"]), n, h, w, _p(outs["out"]), _p(ws), ws.numel(), None, _stream())

    def baseline(self, inp, spec):
        from scipy import ndimage as ndi
        ref = np.stack([ndi.distance_transform_edt(m) for m in self._masks("small")])
        assert np.array_equal(spec["out"].cpu().numpy(), ref)                                 # bit for bit, as test_gpu_vesselness.py


class SamplingWeights(Case):
    entry = "afx_sampling_weights"

    def inputs(self, which):
        return {"x": _dev(_images(which))}

    def need(self, inp):
        _l, lib = _lib()
        return int(lib.afx_sampling_weights_workspace_bytes(_l.SAMPLING["frangi"], *inp["x"].shape, len(SIGMAS_2D)))

    def out_specs(self, inp):
        return {"out": (tuple(inp["x"].shape), torch.float64), "status": ((inp["x"].shape[0],), torch.int32)}

    def call(self, inp, ws, outs):
        _l, lib = _lib()
        sg, ns = _sigmas(SIGMAS_2D)
        n, h, w = inp["x"].shape
        return lib.afx_sampling_weights(_p(inp["x"]), n, h, w, _l.SAMPLING["frangi"], 0, sg, ns, 0.5, 15.0, _p(outs["out"]), _p(outs["status"]),
                                        _p(ws), ws.numel(), None, _stream())

    def baseline(self, inp, spec):
        import vesselness_reference as vr
        from test_gpu_vesselness import WEIGHTS_TOL
        ref = np.stack([vr.sampling_weights(im, binary=False, sigmas=SIGMAS_2D) for im in _images("small")])
        got = spec["out"].cpu().numpy()
        assert int(spec["status"].abs().sum()) == 0
        assert np.abs(got - ref).max() <= WEIGHTS_TOL, np.abs(got - ref).max()


class Ssim(Case):
    entry = "afx_ssim"

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _pairs(which):
        import ssim_reference as sr
        n, h, w = IMG_SMALL if which == "small" else IMG_LARGE
        v = sr.vessel_views(2 * n, h, w, seed=h + w)
        return v[:n], v[n:]

    def inputs(self, which):
        x, y = self._pairs(which)
        return {"x": _dev(x, np.float32), "y": _dev(y, np.float32)}

    def need(self, inp):
        return int(_lib()[1].afx_ssim_workspace_bytes(*inp["x"].shape))

    def out_specs(self, inp):
        return {"out": ((inp["x"].shape[0],), torch.float64)}

    def call(self, inp, ws, outs):
        n, h, w = inp["x"].shape
        return _lib()[1].afx_ssim(_p(inp["x"]), _p(inp["y"]), n, h, w, _p(outs["out"]), _p(ws), ws.numel(), None, _stream())

    def baseline(self, inp, spec):
        import ssim_reference as sr
        from test_gpu_sweep_metrics import SSIM_TOL
        x, y = self._pairs("small")
        err = np.abs(spec["out"].cpu().numpy() - sr.ssim_batch(x, y)).max()
        assert err <= SSIM_TOL, err


# ---------------------------------------------------------------- the volume family
class Edt3D(Case):
    entry = "afx_distance_transform_edt_3d"

    def inputs(self, which):
        return {"fg": _dev(_mask(which), np.uint8)}

    def need(self, inp):
        return int(_lib()[1].afx_distance_transform_edt_3d_workspace_bytes(*inp["fg"].shape))

    def out_specs(self, inp):
        return {"d2": (tuple(inp["fg"].shape), torch.int32), "dist": (tuple(inp["fg"].shape), torch.float64)}

    def call(self, inp, ws, outs):
        return _lib()[1].afx_distance_transform_edt_3d(_p(inp["fg"]), *inp["fg"].shape, _p(outs["d2"]), _p(outs["dist"]), _p(ws), ws.numel(), None,
                                                       _stream())

    def baseline(self, inp, spec):
        import surface_reference as sr
        want = sr.edt(_mask("small"))                                                         # as test_gpu_surface_metrics._check_edt
        d2 = spec["d2"].cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(d2, np.rint(want * want).astype(np.int64))
        assert np.array_equal(spec["dist"].cpu().numpy().view(np.int64), want.view(np.int64))


class SurfaceMetrics(Case):
    entry = "afx_surface_metrics_3d"

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _volumes(which):
        import surface_reference as sr
        shape = SMALL if which == "small" else LARGE
        scale = 1.0 if which == "small" else 1.6                                              # the stale call's surfaces are larger
        return sr.tube_and_ball(shape, radius=2.2 * scale, ball=4.3 * scale), sr.tube_and_ball(shape, offset=(1.5, -1.0, 2.0), radius=2.2 * scale,
                                                                                               ball=4.3 * scale)

    def inputs(self, which):
        a, b = self._volumes(which)
        return {"pred": _dev(a, np.float32), "gt": _dev(b, np.float32)}

    def need(self, inp):
        return int(_lib()[1].afx_surface_metrics_3d_workspace_bytes(*inp["pred"].shape))

    def out_specs(self, inp):
        return {"record": ((16,), torch.int64)}

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import surface_metrics_record
        surface_metrics_record(inp["pred"], inp["gt"], 0.5, 0.5, 95.0, record=outs["record"], workspace=ws)

    def baseline(self, inp, spec):
        import surface_reference as sr
        from nerf_for_angiography_amd.engine import _surface_scores_from_record
        from test_gpu_surface_metrics import _compare_scores
        a, b = self._volumes("small")
        want = sr.surface_metrics(a.astype(np.float32), b.astype(np.float32), 0.5, 0.5, 95.0)
        assert want["n_surface_pred"] > 256 and want["n_surface_gt"] > 256                    # more than one block of surface voxels
        _compare_scores(_surface_scores_from_record(spec["record"], 95.0), want)
        assert spec["record"][13:].tolist() == [0, 0, 0]


class Components(Case):
    entry = "afx_label_components_3d"

    def inputs(self, which):
        return {"x": _dev(_mask(which), np.uint8)}

    def need(self, inp):
        return int(_lib()[1].afx_label_components_3d_workspace_bytes(*inp["x"].shape))

    def out_specs(self, inp):
        shape = tuple(inp["x"].shape)
        return {"labels": (shape, torch.int32), "sizes": ((inp["x"].numel(),), torch.int32), "record": ((8,), torch.int64)}

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import components_record
        components_record(inp["x"], 3, labels=outs["labels"], sizes=outs["sizes"], record=outs["record"], workspace=ws)

    def baseline(self, inp, spec):
        import components_reference as cr
        want, k = cr.label(_mask("small"), 3)                                                 # as test_gpu_components._check
        assert k > 16                                                                         # components in every chunk
        assert spec["record"].tolist() == cr.record(want, k)
        assert np.array_equal(spec["labels"].cpu().numpy(), want)
        sizes = spec["sizes"].cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(sizes[:k], cr.sizes(want)) and not sizes[k:].any()


class Skeleton(Case):
    entry = "afx_skeletonize_3d"

    def inputs(self, which):
        return {"x": _dev(_blob(which), np.uint8), "passes": _skeleton()[1]["passes"] if which == "small" else 6}

    def need(self, inp):
        return int(_lib()[1].afx_skeletonize_3d_workspace_bytes(*inp["x"].shape))

    def out_specs(self, inp):
        return {"skel": (tuple(inp["x"].shape), torch.uint8), "record": ((8,), torch.int64)}

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import skeleton_record
        skeleton_record(inp["x"], inp["passes"], 0, skel=outs["skel"], record=outs["record"], workspace=ws)

    def baseline(self, inp, spec):
        import skeleton_reference as sk
        want, rec = _skeleton()                                                               # as test_gpu_skeleton (sync_every = 0, exactly enough passes)
        assert rec["passes"] >= 3 and rec["converged"] == 1
        assert spec["record"].tolist() == sk.record_list(rec, _blob("small").sum())
        assert np.array_equal(spec["skel"].cpu().numpy(), want.astype(np.uint8))


class Isosurface(Case):
    entry = "afx_isosurface_3d"

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _counts(which):
        """(V, T): the reference's at "small"; the counting call's (capacities 0) at "large" """
        f, affine, want = _reference_mesh(which)
        if want is not None:
            return want["V"], want["T"]
        from nerf_for_angiography_amd.engine import isosurface_record
        rec = isosurface_record(_dev(f), 0.5, affine)[2].cpu().tolist()
        return rec[0], rec[1]

    def inputs(self, which):
        f, affine, _ = _reference_mesh(which)
        v, t = self._counts(which)
        return {"f": _dev(f), "affine": affine, "V": v, "T": t}

    def need(self, inp):
        return int(_lib()[1].afx_isosurface_3d_workspace_bytes(*inp["f"].shape))

    def out_specs(self, inp):
        return {"vertices": ((inp["V"], 3), torch.float32), "triangles": ((inp["T"], 3), torch.int32), "record": ((8,), torch.int64)}

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import isosurface_record
        isosurface_record(inp["f"], 0.5, inp["affine"], inp["V"], inp["T"], vertices=outs["vertices"], triangles=outs["triangles"],
                          record=outs["record"], workspace=ws)

    def baseline(self, inp, spec):
        from test_gpu_isosurface import _same_mesh
        want = _reference_mesh("small")[2]
        assert want["V"] > 2048 and want["T"] > 2048
        rec = spec["record"].tolist()
        assert rec == [want["V"], want["T"], want["E"], want["B"], want["n22"], 0, 0, 0]
        info = {"V": rec[0], "T": rec[1], "E": rec[2], "B": rec[3], "n22": rec[4], "euler": rec[0] - rec[2] + rec[1]}
        _same_mesh((spec["vertices"].cpu().numpy(), spec["triangles"].cpu().numpy(), info), want, self.entry)


class MeshMeasures(Case):
    entry = "afx_mesh_measures"
    REF = (1.0, 2.0, 3.0)

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _mesh(which):
        """(vertices, triangles) ndarrays: the reference mesh at "small", the device's own (checked by the isosurface case) at "large" """
        f, affine, want = _reference_mesh(which)
        if want is not None:
            return want["vertices"], want["triangles"]
        from nerf_for_angiography_amd.engine import extract_isosurface
        v, t, _ = extract_isosurface(_dev(f), 0.5, affine, cap=False)
        return v.cpu().numpy(), t.cpu().numpy()

    def inputs(self, which):
        v, t = self._mesh(which)
        rec = torch.tensor([len(v), len(t), 0, 0, 0, 0, 0, 0], dtype=torch.int64, device=DEV)
        return {"v": _dev(v, np.float32), "t": _dev(t, np.int32), "rec": rec}

    def need(self, inp):
        return int(_lib()[1].afx_mesh_measures_workspace_bytes())

    def out_specs(self, inp):
        return {"out": ((2,), torch.float64)}

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import mesh_measures_record
        mesh_measures_record(inp["v"], inp["t"], inp["rec"], self.REF, out=outs["out"], workspace=ws)

    def baseline(self, inp, spec):
        import math
        import isosurface_reference as iso
        from test_gpu_isosurface import _sum_bound
        v, t = self._mesh("small")
        out = spec["out"].tolist()
        for got, terms in zip(out, iso.measure_terms(v, t, self.REF)):
            assert abs(got - math.fsum(terms)) <= _sum_bound(len(terms), math.fsum(np.abs(terms)))


class MeshSdf(Case):
    entry = "afx_mesh_sdf_3d"
    SHAPE = (17, 9, 10)                                      # several partial 8 x 8 x 8 bricks on every axis

    def inputs(self, which):
        from test_gpu_mesh_sdf import SHEARED, _mesh
        from nerf_for_angiography_amd.engine import MESH_SDF_TILE
        v, t = _mesh("torus")
        assert len(t) >= 2 * MESH_SDF_TILE + 1                                                # more than two LDS tiles of triangles
        if which == "large":                                 # two copies of the mesh: twice the triangle records in the workspace
            v, t = np.concatenate([v, v + np.float32(3.0)]), np.concatenate([t, t + len(v)])
        return {"v": _dev(v, np.float32), "t": _dev(t, np.int32), "shape": self.SHAPE if which == "small" else (24, 17, 10), "affine": SHEARED}

    def need(self, inp):
        return int(_lib()[1].afx_mesh_sdf_3d_workspace_bytes(inp["t"].shape[0]))

    def out_specs(self, inp):
        return {"sdf": (inp["shape"], torch.float32), "nearest": (inp["shape"], torch.int32), "record": ((8,), torch.int64)}

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import mesh_sdf_record
        mesh_sdf_record(inp["v"], inp["t"], inp["shape"], inp["affine"], 0, sdf=outs["sdf"], nearest=outs["nearest"], record=outs["record"],
                        workspace=ws)

    def specified(self, inp, outs):
        return {"sdf": outs["sdf"], "nearest": outs["nearest"], "record": outs["record"][:4]}      # the four slots include/afx.h names

    def baseline(self, inp, spec):
        from test_gpu_mesh_sdf import _reference
        want = _reference("torus", self.SHAPE, "sheared")                                      # as test_distance_nearest_and_sign_equal_the_reference
        assert spec["sdf"].cpu().numpy().tobytes() == want["sdf"].tobytes()
        assert np.array_equal(spec["nearest"].cpu().numpy(), want["nearest"])
        assert spec["record"][:2].tolist() == [inp["t"].shape[0], 0]


class CentrelineGraph(Case):
    entry = "afx_centreline_graph"

    def __init__(self, max_branches=None):
        self.max_branches = max_branches

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _want():
        import graph_reference as gr
        return gr.analyse(_skeleton()[0], _d2("small"))

    def inputs(self, which):
        if which == "small":
            skel, cap = _skeleton()[0], self._want()["record"]["branches"] if self.max_branches is None else self.max_branches
            return {"skel": _dev(skel, np.uint8), "d2": _d2_dev(_d2(which)), "cap": cap}
        return {"skel": _large_skeleton(), "d2": _d2_dev(_d2(which)), "cap": 4096}

    def need(self, inp):
        return int(_lib()[1].afx_centreline_graph_workspace_bytes(*inp["skel"].shape))

    def out_specs(self, inp):
        shape = tuple(inp["skel"].shape)
        return {"node_labels": (shape, torch.int32), "branch_labels": (shape, torch.int32), "path_voxels": ((inp["skel"].numel(),), torch.int32),
                "branches": ((inp["cap"], 16), torch.int64), "record": ((16,), torch.int64)}

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import centreline_graph_record
        centreline_graph_record(inp["skel"], inp["d2"], None, inp["cap"], node_labels=outs["node_labels"], branch_labels=outs["branch_labels"],
                                path_voxels=outs["path_voxels"], branches=outs["branches"], record=outs["record"], workspace=ws)

    def specified(self, inp, outs):
        """path_voxels up to record[2], rows up to min(B, max_branches): the rest is unspecified (include/afx.h)"""
        rec = outs["record"].tolist()
        return {"node_labels": outs["node_labels"], "branch_labels": outs["branch_labels"], "path_voxels": outs["path_voxels"][:rec[2]],
                "branches": outs["branches"][:min(rec[4], inp["cap"])], "record": outs["record"]}

    def baseline(self, inp, spec):
        import graph_reference as gr
        want = self._want()                                                                   # as test_gpu_centreline_graph._check
        nb = want["record"]["branches"]
        assert nb > 16 and want["record"]["p_voxels"] > 256
        assert spec["record"].cpu().numpy().view(np.uint64).tolist() == gr.record_slots(want["record"], self.max_branches)
        assert np.array_equal(spec["node_labels"].cpu().numpy(), want["node_labels"])
        assert np.array_equal(spec["branch_labels"].cpu().numpy(), want["branch_labels"])
        assert spec["path_voxels"].tolist() == want["path_voxels"]
        rows = spec["branches"].cpu().numpy().view(np.uint64)
        assert len(rows) == min(nb, inp["cap"])
        for b in range(len(rows)):
            assert rows[b].tolist() == gr.row_slots(want["branches"][b]), b


class PruneSpurs(Case):
    entry = "afx_prune_spurs"

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _want():
        import graph_reference as gr
        return gr.prune(_skeleton()[0], _d2("small"), 1.0)

    def inputs(self, which):
        if which == "small":
            return {"skel": _dev(_skeleton()[0], np.uint8), "d2": _d2_dev(_d2("small")), "rounds": self._want()[1]["rounds"]}
        return {"skel": _large_skeleton(), "d2": _d2_dev(_d2("large")), "rounds": 3}

    def need(self, inp):
        return int(_lib()[1].afx_prune_spurs_workspace_bytes(*inp["skel"].shape))

    def out_specs(self, inp):
        return {"out": (tuple(inp["skel"].shape), torch.uint8), "record": ((8,), torch.int64)}

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import prune_record
        prune_record(inp["skel"], inp["d2"], 1.0, inp["rounds"], 0, out=outs["out"], record=outs["record"], workspace=ws)

    def baseline(self, inp, spec):
        import graph_reference as gr
        want, rec = self._want()                                                              # as test_gpu_centreline_graph.test_pruning_equals_the_reference
        assert rec["branches"] > 0 and rec["rounds"] >= 2
        assert spec["record"].tolist() == gr.prune_record_slots(rec)
        assert np.array_equal(spec["out"].cpu().numpy(), want.astype(np.uint8))


class Frangi3D(Case):
    entry = "afx_frangi_3d"
    NAME = "24x20x17"                                        # 8 160 voxels: 31.9 blocks of 256, three distinct sides

    def inputs(self, which):
        from test_gpu_frangi3d import CASES, _reference
        if which == "small":
            return {"x": _dev(_reference(self.NAME, np.float64)[0]), "sigmas": CASES[self.NAME][1]}
        import frangi3d_reference as fr                     # (the phantom and noise floor of its test's "40x33x300" case, at LARGE)
        x = fr.shapes_phantom(LARGE, seed=5)[0] + 0.02 * np.random.default_rng(6).random(LARGE)
        return {"x": _dev(x.astype(np.float64)), "sigmas": CASES[self.NAME][1]}

    def need(self, inp):
        return int(_lib()[1].afx_frangi_3d_workspace_bytes(*inp["x"].shape, len(inp["sigmas"])))

    def out_specs(self, inp):
        return {"out": (tuple(inp["x"].shape), torch.float64), "scale_index": (tuple(inp["x"].shape), torch.uint8)}

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import frangi_3d_record
        frangi_3d_record(inp["x"], inp["sigmas"], out=outs["out"], scale_index=outs["scale_index"], workspace=ws)

    def baseline(self, inp, spec):
        from test_gpu_frangi3d import _compare
        _compare(self.NAME, np.float64, spec["out"].cpu().numpy(), spec["scale_index"].cpu().numpy())


class TvDenoise(Case):
    entry = "afx_tv_denoise_3d"
    code = AFX_E_INVALID                                     # its documented code for a short workspace
    ITERATIONS = 15                                          # an odd count: both ping-pong triples of the workspace are read and written

    @staticmethod
    def _shape(which):
        from test_gpu_tv import T0, T1, T2
        return (3 * T0 + 1, 2 * T1 + 3, 2 * T2 + 5) if which == "small" else (4 * T0 + 1, 3 * T1 + 3, 3 * T2 + 5)

    def inputs(self, which):
        from test_gpu_tv import _inputs
        x, weight = _inputs(self._shape(which))[0]["normal"]
        return {"x": _dev(x), "weight": weight, "x_host": x}

    def need(self, inp):
        return int(_lib()[1].afx_tv_denoise_3d_workspace_bytes(*inp["x"].shape))

    def out_specs(self, inp):
        return {"out": (tuple(inp["x"].shape), torch.float64)}

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import tv_denoise_3d
        tv_denoise_3d(inp["x"], inp["weight"], self.ITERATIONS, out=outs["out"], workspace=ws)

    def baseline(self, inp, spec):
        import tv_reference as tv
        from test_gpu_tv import _same_bits
        assert _same_bits(spec["out"], tv.tv_denoise(inp["x_host"], inp["weight"], self.ITERATIONS))


# ---------------------------------------------------------------- the sampler and the grid's cell draw
TOPK_N = {"small": 2 * 1024 + 77, "large": 5 * 1024 + 3}     # SEL_PER_BLOCK = 1 024 keys per block: 3 and 6 blocks, the last one ragged


class TopK(Case):
    entry = "afx_topk_indices"

    def inputs(self, which):
        import many_chunks_cases as mc
        keys = mc.sampler_keys(TOPK_N[which])
        return {"keys": _dev(keys), "k": 300 if which == "small" else 2000, "host": keys}

    def need(self, inp):
        return int(_lib()[1].afx_topk_workspace_bytes(inp["keys"].numel()))

    def out_specs(self, inp):
        return {"idx": ((inp["k"],), torch.int64)}

    def call(self, inp, ws, outs):
        return _lib()[1].afx_topk_indices(_p(inp["keys"]), inp["keys"].numel(), inp["k"], _p(outs["idx"]), _p(ws), ws.numel(), _stream())

    def baseline(self, inp, spec):
        import many_chunks_cases as mc
        assert np.array_equal(spec["idx"].cpu().numpy(), mc.topk_reference(inp["host"], inp["k"]))      # as test_gpu_many_chunks.test_topk


class SampleBatches(Case):
    """n_batches x k indices; the host-id form and the device-id form run the same kernels"""
    SEED, STREAM0 = 11, (3 << 32) | 40

    def __init__(self, dev_id):
        self.dev_id = dev_id
        self.entry = "afx_sample_batches_dev" if dev_id else "afx_sample_batches"

    def inputs(self, which):
        from test_gpu_sampler import _weights
        n = TOPK_N[which]
        return {"w": _weights(n, n, zeros=5), "B": 3 if which == "small" else 5, "k": 300 if which == "small" else 2000,
                "id": torch.tensor(self.STREAM0, dtype=torch.int64, device=DEV)}

    def need(self, inp):
        return int(_lib()[1].afx_sample_batches_workspace_bytes(inp["w"].numel(), inp["B"]))

    def out_specs(self, inp):
        return {"idx": ((inp["B"], inp["k"]), torch.int64)}

    def call(self, inp, ws, outs):
        if self.dev_id:
            from nerf_for_angiography_amd.engine import sample_batches_dev
            sample_batches_dev(inp["w"], self.SEED, inp["id"], inp["B"], inp["k"], out_idx=outs["idx"], workspace=ws)
            return 0
        return _lib()[1].afx_sample_batches(_p(inp["w"]), inp["w"].numel(), self.SEED, self.STREAM0, inp["B"], inp["k"], _p(outs["idx"]), _p(ws),
                                            ws.numel(), _stream())

    def baseline(self, inp, spec):
        import many_chunks_cases as mc
        from test_gpu_sampler import _keys
        for b in range(inp["B"]):        # as test_gpu_sampler.test_selection_is_the_reference_selection_of_the_device_keys
            keys = _keys(inp["w"], None, self.SEED, self.STREAM0 + b).cpu().numpy()
            assert np.array_equal(spec["idx"][b].cpu().numpy(), mc.topk_reference(keys, inp["k"])), b


class GridSelect(Case):
    """n_draw below and above the occupied count: the second half of the list is a draw among, or all of, the occupied cells"""
    entry = "afx_grid_select_cells"
    RES = (37, 29, 23)                                       # 24 679 cells: 772 words, 4 workgroups of SEL_WORDS = 256 words, the last one ragged
    STEP = 272

    def __init__(self, kind):
        self.kind = kind                                     # "dense": n_occ > n_draw; "shell": n_occ < n_draw

    def _grid(self, which):
        from test_gpu_grid_refresh import _grid
        return _grid(list(self.RES), self.kind if which == "small" else "dense", seed=5)

    def inputs(self, which):
        grid = self._grid(which)
        n = grid.num_cells // 4 if which == "small" else grid.num_cells // 2
        return {"grid": grid, "n": n}

    def need(self, inp):
        from nerf_for_angiography_amd.engine import grid_select_workspace_bytes
        return grid_select_workspace_bytes(inp["grid"]._aabb_host, inp["grid"]._res_host)

    def out_specs(self, inp):
        return {"cells": ((2 * inp["n"],), torch.int32), "count": ((1,), torch.int64)}

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import grid_select_cells
        g = inp["grid"]
        grid_select_cells(g._aabb_host, g._res_host, g.bits, inp["n"], g.seed, self.STEP, cells=outs["cells"], count=outs["count"], workspace=ws)

    def specified(self, inp, outs):
        return {"cells": outs["cells"][:int(outs["count"])], "count": outs["count"]}          # "slots behind the count unwritten"

    def baseline(self, inp, spec):
        from test_gpu_grid_refresh import _restated
        g, n = inp["grid"], inp["n"]
        want, _ = _restated(g, self.STEP, n)                                                  # as test_selection_equals_its_restatement
        n_occ = int(g._binary_u8.sum())
        assert (n_occ < n) == (self.kind == "shell") and n_occ > 0
        assert int(spec["count"]) == want.numel() == n + min(n, n_occ)
        assert torch.equal(spec["cells"].long().cpu(), want)


# ---------------------------------------------------------------- the engine-workspace family
# These go through nerf_for_angiography_amd.engine.Engine, which keeps ONE workspace (eng._ws) and asks the library's query for its size.
# The contract run assigns eng._ws the interior of an arena of exactly that size and caps max_workspace_bytes at it, so that the engine
# neither regrows nor replaces it; afterwards eng._ws must still be that tensor.  Ray batches: 300 to 700 rays through a 32^3 grid, 60 steps.
NEAR, FAR, SPR, EPS, THRE = 1400.0, 1600.0, 60, 1e-2, 1e-4
GRID_RES = 32
RAYS = {"small": (500, 17), "large": (700, 23)}              # (rays, seed): 500 x 64 padded samples = 250 tiles of 128, the last chunk ragged


class Outs:
    """The typed output arenas of one engine call, painted with one fill; `check` compares every guard with its copy from before the call."""

    def __init__(self, fill, seed):
        self.fill, self.seed, self.items = fill, seed, []

    def new(self, name, shape, dtype, init=None):
        whole, t = wc.typed_arena(shape, dtype, self.fill, DEV, self.seed + 11 * (len(self.items) + 1))
        if init is not None:
            t.copy_(init) if torch.is_tensor(init) else t.fill_(init)
        self.items.append((name, whole, t.numel() * t.element_size(), whole.clone()))
        return t

    def check(self, what):
        for name, whole, nbytes, before in self.items:
            assert wc.guards_intact(whole, nbytes, before), (what, "guard of output", name)


class EngineCase:
    entry = ""
    short = "need"           # the size one byte below which the call is refused: "need" (the query), or a method name

    def model(self):
        """a fresh model with the same weights every time"""
        raise NotImplementedError

    def problem(self, which):
        raise NotImplementedError

    def need(self, m, prob):
        raise NotImplementedError

    def run(self, m, prob, outs):
        """-> name -> result tensor (the specified part)"""
        raise NotImplementedError

    def baseline(self, prob, r0):
        raise NotImplementedError

    def short_run(self, m, prob, outs):
        """the call that a workspace one byte short must refuse (default: the case's own run)"""
        return self.run(m, prob, outs)


def _engine_run(case, prob, fill, arena=None, seed=0, short_by=0):
    from nerf_for_angiography_amd._lib import AfxError
    m = case.model()
    eng = m.engine
    need = case.need(m, prob) if not short_by else getattr(case, case.short)(m, prob)
    whole, ws = wc.arena(need, fill, DEV, seed) if arena is None else arena
    assert ws.numel() >= need > 0
    eng._ws, eng.max_workspace_bytes, eng._ws_captured = ws, ws.numel(), False
    outs = Outs(fill, seed)
    before = whole.clone()
    what = (case.entry, fill)
    if short_by:             # the engine would replace a buffer that is too small: hand it the short one as it is
        eng._workspace = lambda nbytes, device: ws[:need - short_by]
        with pytest.raises(AfxError, match=r"failed \(-2\)"):
            case.short_run(m, prob, outs)
        torch.cuda.synchronize()
        assert torch.equal(whole, before), (what, "a refused call wrote to the workspace")
        for name, w, _, b in outs.items:
            assert torch.equal(w, b), (what, "a refused call wrote to", name)
        return None
    res = case.run(m, prob, outs)
    torch.cuda.synchronize()
    assert eng._ws is ws, (what, "the engine replaced the workspace")
    assert wc.guards_intact(whole, ws.numel(), before), (what, "guard of the workspace")
    outs.check(what)
    return {k: v.detach().clone() for k, v in res.items()}


def check_engine_contract(case):
    small, large = case.problem("small"), case.problem("large")
    r0 = _engine_run(case, small, 0x00)
    case.baseline(small, r0)
    for fill in (0xFF, "random"):
        _same(case, fill, _engine_run(case, small, fill, seed=3), r0)
    m = case.model()
    arena = wc.arena(max(case.need(m, small), case.need(m, large)), "stale", DEV, seed=5)
    del m
    _engine_run(case, large, "stale", arena=arena, seed=5)
    _same(case, "stale", _engine_run(case, small, "stale", arena=arena, seed=7), r0)
    if case.short is not None:
        _engine_run(case, small, 0xFF, short_by=1)


def _grad_arena(m, outs):
    """grad_flat of a backward entry point (accumulated into: starts at zero under every fill), in the flat parameter buffer's order -
    that of torch.cat([p.grad.reshape(-1) for p in m._hip_params()])"""
    return outs.new("grad_flat", (m.engine.param_count,), torch.float32, init=0.0)


def _grid32(kind, seed=5):
    from test_gpu_grid_refresh import _grid
    return _grid(GRID_RES, kind, seed=seed)


def _grid_rays(which):
    from test_gpu_grid_graph import _rays
    n, seed = RAYS[which]
    return _rays(n, seed)


def _grid_model(layers=4, width=128):
    from test_gpu_grid_graph import _model
    return _model(layers, width, "none")


def _max_steps(eng, o, d):
    from nerf_for_angiography_amd import _lib as L
    from nerf_for_angiography_amd.engine import _fill_march_args
    from test_gpu_grid_graph import AABB
    a = L.MarchArgs()
    _fill_march_args(a, o, d, AABB, NEAR, FAR, (FAR - NEAR) / SPR, None, None, None)
    return int(eng.lib.afx_march_max_steps(C.byref(a)))


class GridStep(EngineCase):
    """afx_march_train_step_mse_capturable / _single_eval: sphere-like grid and 500 rays; the stale call has a full grid and 700 rays, so that
    every per-ray count, candidate list and stash row of the small call lies where the large one left other data"""

    def __init__(self, single_eval):
        self.single_eval = single_eval
        self.entry = "afx_march_train_step_mse_single_eval" if single_eval else "afx_march_train_step_mse_capturable"

    def model(self):
        return _grid_model()

    def problem(self, which):
        o, d, tgt = _grid_rays(which)
        return {"o": o, "d": d, "tgt": tgt, "grid": _grid32("shell" if which == "small" else "dense")}

    def need(self, m, prob):
        f = m.engine.march_single_eval_workspace_bytes if self.single_eval else m.engine.march_train_workspace_bytes
        return f("f16s8", prob["o"].shape[0], _max_steps(m.engine, prob["o"], prob["d"]))

    def _call(self, m, prob, grad, **kw):
        from test_gpu_grid_graph import AABB
        eng, g = m.engine, prob["grid"]
        f = eng.march_train_step_mse_single_eval if self.single_eval else eng.march_train_step_mse_capturable
        return f(m._prepared(), prob["o"], prob["d"], prob["tgt"], 1.0 / prob["o"].shape[0], grad, "f16s8", AABB, NEAR, FAR, (FAR - NEAR) / SPR,
                 EPS, THRE, grid_bits=g.bits, grid_aabb=g._aabb_host, grid_res=g._res_host, **kw)

    def run(self, m, prob, outs):
        n = prob["o"].shape[0]
        grad = outs.new("grad_flat", (m.engine.param_count,), torch.float32, init=0.0)      # accumulated into: starts at zero under every fill
        pixel, counts, skip = (outs.new("pixel", (n,), torch.float32), outs.new("counts", (3,), torch.int64), outs.new("skip", (1,), torch.float32))
        self._call(m, prob, grad, pixel=pixel, counts=counts, skip=skip)
        return {"pixel": pixel, "counts": counts, "skip": skip, "grad_flat": grad}

    def baseline(self, prob, r0):
        from conftest import rel_l2
        from test_gpu_grid_graph import AABB
        assert r0["counts"][1] > 1000 and float(r0["skip"]) == 0.0
        if not self.single_eval:                             # as test_capturable_call_equals_the_one_call_step: the one-call step, bit for bit
            from nerf_for_angiography_amd.render import march_train_step_mse
            m1 = self.model()
            loss1, pix1, kept1 = march_train_step_mse(m1, prob["grid"], AABB, prob["o"], prob["d"], SPR, NEAR, FAR, EPS, THRE, prob["tgt"])
            g1 = torch.cat([p.grad.reshape(-1) for p in m1._hip_params()])
            assert tuple(r0["counts"].tolist()) == m1.engine.last_march_counts and kept1 == int(r0["counts"][1])
            assert torch.equal(pix1, r0["pixel"]) and torch.equal(g1, r0["grad_flat"])
        else:                                                # as test_single_eval_equals_the_two_evaluation_step
            from test_gpu_grid_single_eval import SINGLE_EVAL_GRAD_TOL
            m1 = self.model()
            g1 = torch.zeros(m1.engine.param_count, device=DEV)
            pix1, counts1, skip1 = GridStep(False)._call(m1, prob, g1)
            torch.cuda.synchronize()
            assert counts1.tolist() == r0["counts"].tolist() and torch.equal(skip1, r0["skip"]) and torch.equal(pix1, r0["pixel"])
            assert rel_l2(r0["grad_flat"].cpu().numpy(), g1.cpu().numpy()) < SINGLE_EVAL_GRAD_TOL


class MarchRender(EngineCase):
    """afx_march_render in both ray modes, at f16 (forward only).  Engine.march_render allocates pixel and kept_counts itself and takes no
    buffers: the workspace is guard-banded, these two outputs cannot be."""

    def __init__(self, pose):
        self.pose = pose
        self.entry = "afx_march_render"
    W, H, SRC = 24, 20, [0, 0, 1500.0]

    def model(self):
        from test_gpu_grid_render import _model
        return _model(4, 128, prec="f16")

    def problem(self, which):
        if not self.pose:
            o, d, _ = _grid_rays(which)
            return {"o": o, "d": d, "grid": _grid32("shell" if which == "small" else "dense")}
        from nerf_for_angiography_amd.visualization.sweep import _poses, sweep_angles
        from test_gpu_grid_render import _port_rays
        angles = sweep_angles(40, 20)[:1 if which == "small" else 2]      # views of 24 x 20 = 480 rays
        rays = [_port_rays(th if th >= 0 else 360 + th, ph if ph >= 0 else 360 + ph, self.W, self.H, 13.0 * self.W, self.SRC) for th, ph in angles]
        return {"poses": _poses(angles, self.SRC, (0.0, 0.0, 0.0), DEV), "o": torch.cat([r[0] for r in rays]), "d": torch.cat([r[1] for r in rays]),
                "grid": _grid32("shell" if which == "small" else "dense")}

    def need(self, m, prob):
        from nerf_for_angiography_amd import _lib as L
        n = int(m.engine.lib.afx_march_render_workspace_bytes(L.RAYS_POSE if self.pose else L.RAYS_ARRAYS, prob["o"].shape[0],
                                                              _max_steps(m.engine, prob["o"], prob["d"])))
        assert n > 0
        return n

    def run(self, m, prob, outs):
        from nerf_for_angiography_amd.render import march_render, march_render_projection
        from test_gpu_grid_render import _aabb
        with torch.no_grad():
            if self.pose:
                pix, counts = march_render_projection(m, prob["grid"], _aabb(), prob["poses"], self.W, self.H, 13.0 * self.W, SPR, NEAR, FAR)
            else:
                pix, counts = march_render(m, prob["grid"], _aabb(), prob["o"], prob["d"], SPR, NEAR, FAR)
        return {"pixel": pix, "kept": m.engine.last_kept_counts, "counts": torch.tensor(counts)}

    def baseline(self, prob, r0):
        from test_gpu_grid_render import _op_sequence
        m = self.model()
        with torch.no_grad():                                # as test_gpu_grid_render._check_equal (pose mode: through the port's rays)
            want, ri, *_ = _op_sequence(m, prob["grid"], prob["o"], prob["d"], spr=SPR)
        assert torch.equal(r0["pixel"], want)
        assert torch.equal(r0["kept"].long(), torch.bincount(ri.long(), minlength=prob["o"].shape[0]))
        assert int(r0["counts"][1]) == ri.numel() > 256


class HierStep(EngineCase):
    """afx_hier_train_step_mse: 300 rays, 35 coarse depths per ray (64 padded), 33 fine ones - ragged counts, per-ray coarse depths.  The query
    is the one-chunk size; a smaller workspace means more ray chunks, so there is no one-short refusal at it (tests/test_host_cpu.py pins the
    refusal below the fixed part)."""
    entry = "afx_hier_train_step_mse"
    short = None
    SC, NF = 35, 33

    def model(self):
        from test_gpu_parity import make_model
        torch.manual_seed(3 + 128)
        m = make_model(3, 128, precision="f16s8")
        with torch.no_grad():
            m.output_linear[0].weight.mul_(4.0)
            m.output_linear[0].bias.fill_(-26.0)
        return m

    def problem(self, which):
        from test_gpu_round3 import _ref_iteration_problem
        n = 300 if which == "small" else 520
        sc, nf = (self.SC, self.NF) if which == "small" else (64, 40)
        g = torch.Generator().manual_seed(n + sc)
        o, d, tgt = _ref_iteration_problem(n, seed=sc)
        z = torch.sort(1400.0 + 200.0 * torch.rand(n, sc, generator=g), dim=-1).values
        return {"o": o.to(DEV), "d": d.to(DEV), "tgt": tgt.to(DEV), "z": z.to(DEV), "u": torch.rand(n, nf, generator=g).to(DEV), "nf": nf}

    def need(self, m, prob):
        return int(m.engine.lib.afx_hier_workspace_bytes(m.engine.h, prob["o"].shape[0], prob["z"].shape[-1], prob["nf"]))

    def run(self, m, prob, outs):
        """Engine.hier_train_step_mse as render.hierarchical_train_step_mse calls it, grad_flat in an arena (the engine allocates pixel and
        z_all itself: those two cannot be guard-banded)"""
        from nerf_for_angiography_amd.engine import RenderSpec
        n = prob["o"].shape[0]
        grad = _grad_arena(m, outs)
        spec = RenderSpec(n_rays=n, n_samples=int(prob["z"].shape[-1]), origins=prob["o"], dirs=prob["d"], mode="dense", z=prob["z"])
        pix, z_all = m.engine.hier_train_step_mse(m._prepared(), spec, prob["nf"], prob["u"], prob["tgt"], 1.0 / n, grad, "f16s8")
        return {"pixel": pix, "z_all": z_all, "grad": grad}

    def baseline(self, prob, r0):
        from conftest import rel_l2
        from nerf_for_angiography_amd.render import render_rays
        from test_gpu_round3 import HIER_FEW_PIX_TOL, HIER_FEW_GRAD_TOL
        m = self.model()                                     # as test_hierarchical_step_with_coarse_reuse: the exact-fp32 kernels on the merged depths
        assert torch.all(r0["z_all"][:, 1:] >= r0["z_all"][:, :-1])
        m.precision = "f32"
        out = render_rays(m, prob["o"], prob["d"], mode="dense", z=r0["z_all"])
        torch.nn.functional.mse_loss(out.rgb_map, prob["tgt"]).backward()
        g32 = torch.cat([p.grad.reshape(-1) for p in m._hip_params()]).double()
        assert float(g32.norm()) > 0
        assert rel_l2(r0["pixel"].cpu().numpy(), out.rgb_map.detach().cpu().numpy()) < HIER_FEW_PIX_TOL
        assert float((r0["grad"].double() - g32).norm() / g32.norm()) < HIER_FEW_GRAD_TOL


class PackedStep(EngineCase):
    """afx_train_step_packed_mse on the march's packed samples (no visibility pruning), in a workspace of the size the engine asks for
    (the one-chunk query plus the per-ray and per-group head)"""
    entry = "afx_train_step_packed_mse"
    short = None             # (the engine's size has slack over the least the call takes and no query gives that least: nothing to be one short of)

    def model(self):
        from test_gpu_parity import make_model
        torch.manual_seed(3)
        m = make_model(4, 128, precision="f16s8")
        with torch.no_grad():
            m.output_linear[0].weight.mul_(4.0)
            m.output_linear[0].bias.fill_(-5.0)
        return m

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _problem(which):
        from nerf_for_angiography_amd.nerf.occupancy import ray_marching
        from test_gpu_grid_graph import AABB
        o, d, tgt = _grid_rays(which)
        if which == "small":                                 # some rays that miss everything: no samples, pixel = 1
            d = d.clone()
            d[::7] = torch.tensor([0.9, 0.3, -0.3], device=DEV)
        grid = _grid32("shell" if which == "small" else "dense")
        ri, ts, te, packed = ray_marching(o, d, scene_aabb=torch.tensor(AABB), grid=grid, near_plane=NEAR, far_plane=FAR,
                                          render_step_size=(FAR - NEAR) / SPR, return_packed=True)
        return {"o": o, "d": d, "tgt": tgt, "ri": ri, "ts": ts, "te": te, "packed": packed}

    def problem(self, which):
        return self._problem(which)

    def need(self, m, prob):
        from nerf_for_angiography_amd import _lib as L
        p = prob["packed"]                                   # what Engine.train_step_packed_mse asks for
        return int(m.engine.lib.afx_query(m.engine.h, L.Q_BWD_WORKSPACE_FULL, 0, max(p.n_groups, 1) * 32, L.PREC["f16s8"])) + 4 * (p.n_rays + p.n_groups) + 1024

    def run(self, m, prob, outs):
        """Engine.train_step_packed_mse as render.train_step_packed_mse calls it, grad_flat in an arena (the engine allocates pixel itself:
        it cannot be guard-banded)"""
        grad = _grad_arena(m, outs)
        pix = m.engine.train_step_packed_mse(m._prepared(), prob["o"], prob["d"], prob["packed"], prob["tgt"], 1.0 / prob["o"].shape[0], grad, "f16s8")
        return {"pixel": pix, "grad": grad}

    def baseline(self, prob, r0):
        from conftest import rel_l2
        from nerf_for_angiography_amd.nerf.nerf_helpers import get_predictions
        from nerf_for_angiography_amd.nerf.nerf_helpers_acc import acc_render_volume_density
        from test_gpu_round3 import PACKED_F16_PIX_TOL, PACKED_FEW_GRAD_TOL
        o, d, tgt, ri, ts, te = (prob[k] for k in ("o", "d", "tgt", "ri", "ts", "te"))
        n = o.shape[0]
        cnt = torch.bincount(ri.long(), minlength=n)
        assert 256 < ri.numel() < 100000 and int((cnt == 0).sum()) > 0
        assert bool((r0["pixel"][cnt == 0] == 1.0).all())
        m = self.model()                                     # as test_fused_packed_step_vs_operator_sequence_and_fp32

        def ops_step(prec):
            m.precision = prec
            m.zero_grad(set_to_none=True)
            pos = o[ri.long()] + d[ri.long()] * (ts + te) / 2.0
            pred, _ = acc_render_volume_density(get_predictions(m, pos, 131072), ri, ts, te, n, SPR)
            torch.nn.functional.mse_loss(pred, tgt).backward()
            return pred.detach(), torch.cat([p.grad.reshape(-1) for p in m._hip_params()]).double()

        pix32, g32 = ops_step("f32")
        pix16, _ = ops_step("f16")
        assert rel_l2(r0["pixel"].cpu().numpy(), pix16.cpu().numpy()) < PACKED_F16_PIX_TOL
        assert float((r0["grad"].double() - g32).norm() / g32.norm()) < PACKED_FEW_GRAD_TOL


class PointsInputGrads(EngineCase):
    """afx_mlp_backward_inputs through Engine.mlp_backward_inputs, as model(x) calls it in its backward when x requires a gradient (d_out =
    the weights w of sum_p w_p raw_p): d_pts and grad_flat, both in arenas.  The fills run at the one-chunk size the engine asks for; the
    refusal is one byte below AFX_Q_BWD_INPUTS_WORKSPACE_MIN."""
    short = "min_need"
    N = {"small": 3001, "large": 5003}                       # 23.4 tiles of 128 points

    def __init__(self, prec):
        self.prec = prec
        self.entry = "afx_mlp_backward_inputs"

    def model(self):
        from test_gpu_input_grads import _model
        torch.manual_seed(7)
        return _model(4, 128, "none", self.prec)

    def problem(self, which):
        from test_gpu_input_grads import _points
        pts, w = _points(self.N[which], 1 + (which == "large"))
        return {"pts": pts, "w": w}

    def _query(self, m, prob, what):
        from nerf_for_angiography_amd import _lib as L
        return int(m.engine.lib.afx_query(m.engine.h, what, 0, prob["pts"].shape[0], L.PREC[self.prec]))

    def need(self, m, prob):
        from nerf_for_angiography_amd import _lib as L
        return self._query(m, prob, L.Q_BWD_INPUTS_WORKSPACE_FULL)

    def min_need(self, m, prob):
        from nerf_for_angiography_amd import _lib as L
        return self._query(m, prob, L.Q_BWD_INPUTS_WORKSPACE_MIN)

    def run(self, m, prob, outs):
        pts, w = prob["pts"].to(DEV), prob["w"].to(DEV)
        grad, d_pts = _grad_arena(m, outs), outs.new("d_pts", (pts.shape[0], 3), torch.float32)
        m.engine.mlp_backward_inputs(m._prepared(), pts, w, grad, d_pts, self.prec)
        return {"d_pts": d_pts, "grad": grad}

    def baseline(self, prob, r0):
        from oracle import angio_oracle as orc
        from test_gpu_input_grads import _cfg, _check, _oracle_params
        m = self.model()                                     # as test_points_against_oracle
        x = prob["pts"].double().requires_grad_(True)
        (orc.cppn_forward(x, _cfg(m, 4), _oracle_params(m)).squeeze(-1) * prob["w"].double()).sum().backward()
        _check(f"contract: points 4x128 {self.prec}", r0["d_pts"], x.grad, self.prec)
        assert float(r0["grad"].abs().max()) > 0


class PointsBackward(PointsInputGrads):
    """afx_mlp_backward (f32) through Engine.mlp_backward: the parameter gradient of sum_p w_p raw_p, grad_flat in an arena.  The workspace
    only bounds the chunk: there is no size to be one short of."""
    short = None

    def __init__(self):
        super().__init__("f32")
        self.entry = "afx_mlp_backward"

    def need(self, m, prob):
        from nerf_for_angiography_amd import _lib as L
        return self._query(m, prob, L.Q_BWD_WORKSPACE_FULL)

    def run(self, m, prob, outs):
        grad = _grad_arena(m, outs)
        m.engine.mlp_backward(m._prepared(), prob["pts"].to(DEV), prob["w"].to(DEV), grad, self.prec)
        return {"grad": grad}

    def baseline(self, prob, r0):
        from conftest import rel_l2
        from oracle import angio_oracle as orc
        from test_gpu_input_grads import _cfg, _oracle_params
        from test_gpu_parity import TOL
        m = self.model()
        params = {k: v.requires_grad_(True) for k, v in _oracle_params(m).items()}
        (orc.cppn_forward(prob["pts"].double(), _cfg(m, 4), params).squeeze(-1) * prob["w"].double()).sum().backward()
        want = torch.cat([params[k].grad.reshape(-1) for k in m.state_dict() if params[k].grad is not None])      # the flat buffer's order
        assert want.numel() == r0["grad"].numel()
        assert rel_l2(r0["grad"].cpu().numpy(), want.numpy()) < TOL["f32"]["grad"]
        # include/afx.h: afx_mlp_backward_inputs adds the same parameter gradient, bit for bit when both run in one chunk
        both = _engine_run(PointsInputGrads("f32"), prob, 0x00)
        assert torch.equal(both["grad"], r0["grad"])


class RaysInputGrads(EngineCase):
    """afx_render_backward_inputs through Engine.render_backward_inputs, as render_rays calls it in its backward when origins and directions
    require a gradient (d_pixel = the weights w of sum_r w_r pixel_r): d_origins, d_dirs and grad_flat in arenas.  The forward render that
    gives `pixel` runs in the same workspace first - afx_render_forward under every fill as well; the engine allocates its pixel itself."""
    short = "min_need"
    R = {"small": 300, "large": 420}
    S = {"small": 70, "large": 96}                           # 70 -> 96 padded samples: rays straddle the 128-sample tiles

    def __init__(self, prec):
        self.prec = prec
        self.entry = "afx_render_backward_inputs"

    def model(self):
        from test_gpu_input_grads import _model
        torch.manual_seed(7)
        return _model(4, 64, "none", self.prec)

    def problem(self, which):
        from test_gpu_input_grads import _rays
        o, d, w = _rays(self.R[which], 3 + (which == "large"))
        return {"o": o, "d": d, "w": w, "S": self.S[which]}

    def _query(self, m, prob, what):
        from nerf_for_angiography_amd import _lib as L
        return int(m.engine.lib.afx_query(m.engine.h, what, prob["o"].shape[0], prob["S"], L.PREC[self.prec]))

    def need(self, m, prob):
        from nerf_for_angiography_amd import _lib as L
        return self._query(m, prob, L.Q_BWD_INPUTS_WORKSPACE_FULL)

    def min_need(self, m, prob):
        from nerf_for_angiography_amd import _lib as L
        return self._query(m, prob, L.Q_BWD_INPUTS_WORKSPACE_MIN)

    def _spec(self, prob):
        from nerf_for_angiography_amd.engine import RenderSpec      # (the rays of test_gpu_input_grads._ray_grads: near 1, far 3)
        return RenderSpec(n_rays=prob["o"].shape[0], n_samples=prob["S"], origins=prob["o"].to(DEV), dirs=prob["d"].to(DEV), mode="acc",
                          t_near=1.0, t_far=3.0)

    def _backward(self, m, prob, outs, pixel):
        n = prob["o"].shape[0]
        grad = _grad_arena(m, outs)
        go, gd = outs.new("d_origins", (n, 3), torch.float32), outs.new("d_dirs", (n, 3), torch.float32)
        m.engine.render_backward_inputs(m._prepared(), self._spec(prob), pixel, prob["w"].to(DEV), grad, go, gd, self.prec)
        return {"d_origins": go, "d_dirs": gd, "grad": grad}

    def run(self, m, prob, outs):
        pixel, _, _ = m.engine.render_forward(m._prepared(), self._spec(prob), self.prec)
        return dict(self._backward(m, prob, outs, pixel), pixel=pixel)

    def short_run(self, m, prob, outs):
        """the backward entry point alone (the forward render would write to the workspace first): refused before any launch, so what
        `pixel` holds does not matter"""
        return self._backward(m, prob, outs, torch.ones(prob["o"].shape[0], device=DEV))

    def baseline(self, prob, r0):
        from test_gpu_input_grads import _check, _ray_oracle
        m = self.model()                                     # as test_rays_against_oracle
        wo, wd = _ray_oracle(m, 4, prob["o"], prob["d"], prob["w"], prob["S"], "acc")
        _check(f"contract: d_origins {self.prec}", r0["d_origins"], wo, self.prec)
        _check(f"contract: d_dirs {self.prec}", r0["d_dirs"], wd, self.prec)
        assert float(r0["grad"].abs().max()) > 0


class GridRefresh(Case):
    """afx_grid_refresh, post-warm-up (the device draw): occs, binary and bits are updated in place - they start from the same grid state
    in arenas of their own under every fill"""
    entry = "afx_grid_refresh"
    STEP, OCC_THRE, EMA = 272, 5e-2, 0.95

    @staticmethod
    def _model():
        from test_gpu_grid_refresh import _model
        return _model(4, 128, "f16s8")

    @staticmethod
    def _start(res, kind):
        """a grid with occupancies already in it, so that the EMA and the threshold both act (as test_refresh_equals_the_eager_composition)"""
        from nerf_for_angiography_amd import engine
        from test_gpu_grid_refresh import _grid
        grid = _grid(res, kind, seed=2)
        with torch.no_grad():
            g = torch.Generator(device=DEV).manual_seed(1)
            grid.occs.copy_(torch.rand(grid.num_cells, device=DEV, generator=g) * 0.03)
        if kind == "dense":
            engine.grid_binarize(grid._aabb_host, grid._res_host, grid.occs, 1e-2, grid._binary_u8, grid._bits, grid._partial)
        return grid

    def inputs(self, which):
        grid = self._start(GRID_RES if which == "small" else [37, 41, 33], "shell" if which == "small" else "dense")
        return {"grid": grid, "m": self._model(), "n_draw": grid.num_cells // 4}

    def need(self, inp):
        from nerf_for_angiography_amd.engine import grid_refresh_workspace_bytes
        g = inp["grid"]
        return grid_refresh_workspace_bytes(g._aabb_host, g._res_host, inp["n_draw"], False)

    def out_specs(self, inp):
        g = inp["grid"]
        return {"occs": (tuple(g.occs.shape), g.occs.dtype), "binary": (tuple(g._binary_u8.shape), g._binary_u8.dtype),
                "bits": (tuple(g._bits.shape), g._bits.dtype)}

    def prepare(self, inp, outs):
        g = inp["grid"]
        outs["occs"].copy_(g.occs), outs["binary"].copy_(g._binary_u8), outs["bits"].copy_(g._bits)

    def call(self, inp, ws, outs):
        from nerf_for_angiography_amd.engine import grid_refresh
        g, m = inp["grid"], inp["m"]
        grid_refresh(m.engine, m._prepared(), "f16s8", g._aabb_host, g._res_host, outs["occs"], outs["binary"], outs["bits"], inp["n_draw"], False,
                     g.seed, self.STEP, self.OCC_THRE, self.EMA, ws)

    def baseline(self, inp, spec):
        from test_gpu_grid_refresh import _eager_refresh, _twin
        twin = _twin(inp["grid"])                            # as test_refresh_equals_the_eager_composition
        _eager_refresh(twin, inp["m"], self.STEP, False, self.OCC_THRE, self.EMA)
        assert torch.equal(spec["occs"], twin.occs) and torch.equal(spec["binary"], twin._binary_u8) and torch.equal(spec["bits"], twin._bits)
        n_occ = int(twin._binary_u8.sum())
        assert 0 < n_occ < twin.num_cells and not torch.equal(twin.occs, inp["grid"].occs)


# ---------------------------------------------------------------- the table
# Every function of include/afx.h with a `workspace` parameter, or with a `workspace` field in its args struct, that this module runs:
# name -> a function that runs its contract case(s).  tests/test_workspace_contract_cpu.py checks the names against the header.
def _cases(*cases):
    def run():
        for case in cases:
            check_contract(case)
    return run


def _engine_cases(*cases):
    def run():
        for case in cases:
            check_engine_contract(case)
    return run


TABLE = {
    "afx_frangi": _cases(Frangi2D()),
    "afx_distance_transform_edt": _cases(Edt2D()),
    "afx_sampling_weights": _cases(SamplingWeights()),
    "afx_ssim": _cases(Ssim()),
    "afx_distance_transform_edt_3d": _cases(Edt3D()),
    "afx_surface_metrics_3d": _cases(SurfaceMetrics()),
    "afx_label_components_3d": _cases(Components()),
    "afx_skeletonize_3d": _cases(Skeleton()),
    "afx_isosurface_3d": _cases(Isosurface()),
    "afx_mesh_measures": _cases(MeshMeasures()),
    "afx_mesh_sdf_3d": _cases(MeshSdf()),
    "afx_centreline_graph": _cases(CentrelineGraph()),
    "afx_prune_spurs": _cases(PruneSpurs()),
    "afx_frangi_3d": _cases(Frangi3D()),
    "afx_tv_denoise_3d": _cases(TvDenoise()),
    "afx_topk_indices": _cases(TopK()),
    "afx_sample_batches": _cases(SampleBatches(False)),
    "afx_sample_batches_dev": _cases(SampleBatches(True)),
    "afx_grid_select_cells": _cases(GridSelect("dense"), GridSelect("shell")),
    # the engine-workspace family, at f16s8 unless noted
    "afx_grid_refresh": _cases(GridRefresh()),
    "afx_march_train_step_mse_capturable": _engine_cases(GridStep(False)),
    "afx_march_train_step_mse_single_eval": _engine_cases(GridStep(True)),
    "afx_march_render": _engine_cases(MarchRender(False), MarchRender(True)),          # f16, both ray modes
    "afx_hier_train_step_mse": _engine_cases(HierStep()),
    "afx_train_step_packed_mse": _engine_cases(PackedStep()),
    "afx_mlp_backward": _engine_cases(PointsBackward()),                                # f32
    "afx_mlp_backward_inputs": _engine_cases(PointsInputGrads("f32"), PointsInputGrads("f16")),
    "afx_render_backward_inputs": _engine_cases(RaysInputGrads("f32"), RaysInputGrads("f16")),
}

# Workspace takers this module has no case of its own for, and what does run them against workspace contents.
_STALE_TEST = "tests/test_gpu_parity.py::test_results_do_not_depend_on_stale_workspace"
COVERED_ELSEWHERE = {
    "afx_render_backward": _STALE_TEST + " (autograd)",
    "afx_train_step_mse": _STALE_TEST + " (fused)",
    "afx_render_forward": "here inside the afx_render_backward_inputs cases (the forward render runs in the same arena)",
    "afx_march_train_step_mse": "sizes its workspace itself (a 64 MiB floor, grown on AFX_E_WORKSPACE): no exact size to pin; it is the "
                                "reference the capturable case is compared with",
}
# Takers of afx_render_args that never look at its workspace field.
WORKSPACE_FIELD_UNUSED = ("afx_project_volume",)


@pytest.mark.parametrize("name", list(TABLE))
def test_workspace_contract(name):
    TABLE[name]()


def test_centreline_graph_capacity_below_and_at_the_count():
    """max_branches below B: the rows that fit are the full call's, the status bit is set, the record reports the true B, and the table's
    guards are intact; exactly B: no status bit."""
    nb = CentrelineGraph._want()["record"]["branches"]
    full = _run(CentrelineGraph(), CentrelineGraph().inputs("small"), 0xFF)
    for cap, status in ((nb - 1, 1), (nb // 3, 1), (nb, 0)):
        case = CentrelineGraph(max_branches=cap)
        got = _run(case, case.inputs("small"), "random", seed=cap)
        case.baseline(case.inputs("small"), got)
        rec = got["record"].tolist()
        assert rec[4] == nb and rec[11] == status, (cap, rec)
        assert wc.same_bits(got["branches"], full["branches"][:cap]), cap
