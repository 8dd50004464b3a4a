"""The caller-provided buffers of the analysis wrappers of nerf_for_angiography_amd/engine.py (the helpers alone, on the host:
tests/test_engine_buffers_cpu.py).  On the smallest inputs on which every wrapper launches - a 9 x 8 x 7 mask with an L-shaped line of
voxels and its squared EDT, a ramp volume of that shape and its isosurface, two 8 x 8 views, five points:

  acceptance  the call with every buffer passed returns the very tensors passed, and the part of each that include/afx.h says is written
              equals, bit for bit, what the call that allocates for itself returns;
  refusal     each caller buffer in turn is given a wrong dtype of equal byte size, a non-contiguous view and one element too few: a
              ValueError that names the buffer, and every other output buffer, painted beforehand, keeps its bytes - nothing was launched.

Every wrong buffer is a view into an allocation at least as large as the right one (the short one the leading part of a full-size one),
so a refusal missed by mistake would still write only into memory this test owns.

Run with -m gpu on an MI355X."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (9, 8, 7)
N = 9 * 8 * 7
ISO, CAP, PASSES = 0.47, 4, 2
I32, I64, U8, U16, F32, F64 = torch.int32, torch.int64, torch.uint8, torch.uint16, torch.float32, torch.float64
SAME_SIZE = {I32: F32, F32: I32, I64: F64, F64: I64, U8: torch.int8, U16: torch.int16}


def _eng():
    from nerf_for_angiography_amd import engine
    return engine


def _lib():
    from nerf_for_angiography_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _inputs():
    """The shared inputs, made once and never written to."""
    eng = _eng()
    m = np.zeros(SHAPE, np.uint8)
    m[1:7, 3, 3] = 1
    m[6, 3:7, 3] = 1                                       # an L: two legs that meet at (6, 3, 3)
    mask = torch.from_numpy(m).to(DEV)
    d2 = eng._d2_u32(eng.distance_transform_edt_3d(mask, return_squared=True)[1], mask, "test")
    i, j, k = np.meshgrid(np.arange(9), np.arange(8), np.arange(7), indexing="ij")
    ramp = torch.from_numpy(((i + 0.1 * j + 0.01 * k) / 10.0).astype(np.float32)).to(DEV)
    rec = eng.isosurface_record(ramp, ISO)[2].cpu().tolist()                       # the counting call
    n_v, n_t = rec[0], rec[1]
    assert n_v > 0 and n_t > 0
    verts, tris, mesh_rec = eng.isosurface_record(ramp, ISO, None, n_v, n_t)
    labels, sizes, comp_rec = eng.components_record(mask, 3)
    poses = np.tile(np.eye(4), (2, 1, 1))
    poses[:, 2, 3] = 50.0
    records = torch.from_numpy(eng.hull_view_records(poses, 10.0)).to(DEV)
    images = torch.zeros(2, 8, 8, dtype=F64, device=DEV)
    points = torch.tensor([[1.0, 3, 3], [2, 3, 3], [3, 3, 3], [4, 3, 3], [5, 3, 3]], dtype=F64, device=DEV)
    torch.cuda.synchronize()
    return dict(mask=mask, d2=d2, ramp=ramp, V=n_v, T=n_t, verts=verts, tris=tris, mesh_rec=mesh_rec, labels=labels, sizes=sizes, comp_rec=comp_rec,
                records=records, images=images, points=points, points32=points.to(F32).contiguous(),
                ident=np.asarray(eng._IDENTITY_AFFINE, np.float64))


class Case:
    """One wrapper: `outputs` name -> (dtype, shape) of the buffers it allocates unless they are passed, `inputs` name -> (dtype, shape,
    the valid tensor) of the caller buffers it only reads, `workspace` the size query, `call(bufs)` -> name -> tensor for every output."""
    outputs, inputs = {}, {}

    def workspace(self):
        return None

    def specified(self, res):
        return res


class SurfaceMetrics(Case):
    outputs = {"record": (I64, (16,))}

    def workspace(self):
        return _lib().afx_surface_metrics_3d_workspace_bytes(*SHAPE)

    def call(self, b):
        x = _inputs()["ramp"]
        return {"record": _eng().surface_metrics_record(x, x + 0.1, ISO, ISO, record=b.get("record"), workspace=b.get("workspace"))}


class Components(Case):
    outputs = {"labels": (I32, SHAPE), "sizes": (I32, (N,)), "record": (I64, (8,))}

    def workspace(self):
        return _lib().afx_label_components_3d_workspace_bytes(*SHAPE)

    def call(self, b):
        return dict(zip(("labels", "sizes", "record"), _eng().components_record(_inputs()["mask"], 3, b.get("labels"), b.get("sizes"), b.get("record"),
                                                                               b.get("workspace"))))


class ComponentsFilter(Case):
    outputs = {"out": (U8, SHAPE)}

    @property
    def inputs(self):
        return {"sizes": (I32, (N,), _inputs()["sizes"]), "record": (I64, (8,), _inputs()["comp_rec"])}

    def call(self, b):
        inp = _inputs()
        return {"out": _eng().components_filter(inp["labels"], b.get("sizes", inp["sizes"]), b.get("record", inp["comp_rec"]), True, 1, out=b.get("out"))}


class Skeleton(Case):
    outputs = {"skel": (U8, SHAPE), "record": (I64, (8,))}

    def workspace(self):
        return _lib().afx_skeletonize_3d_workspace_bytes(*SHAPE)

    def call(self, b):
        return dict(zip(("skel", "record"), _eng().skeleton_record(_inputs()["mask"], PASSES, 0, b.get("skel"), b.get("record"), b.get("workspace"))))


class Isosurface(Case):
    @property
    def outputs(self):
        return {"vertices": (F32, (_inputs()["V"], 3)), "triangles": (I32, (_inputs()["T"], 3)), "record": (I64, (8,))}

    def workspace(self):
        return _lib().afx_isosurface_3d_workspace_bytes(*SHAPE)

    def call(self, b):
        inp = _inputs()
        return dict(zip(("vertices", "triangles", "record"),
                        _eng().isosurface_record(inp["ramp"], ISO, None, inp["V"], inp["T"], b.get("vertices"), b.get("triangles"), b.get("record"),
                                                 b.get("workspace"))))


class MeshMeasures(Case):
    outputs = {"out": (F64, (2,))}

    @property
    def inputs(self):
        return {"record": (I64, (8,), _inputs()["mesh_rec"])}

    def workspace(self):
        return _lib().afx_mesh_measures_workspace_bytes()

    def call(self, b):
        inp = _inputs()
        return {"out": _eng().mesh_measures_record(inp["verts"], inp["tris"], b.get("record", inp["mesh_rec"]), None, b.get("out"), b.get("workspace"))}


class MeshSdf(Case):
    outputs = {"sdf": (F32, SHAPE), "record": (I64, (8,))}

    def workspace(self):
        return _lib().afx_mesh_sdf_3d_workspace_bytes(_inputs()["T"])

    def call(self, b):
        inp = _inputs()
        return dict(zip(("sdf", "record"), _eng().mesh_sdf_record(inp["verts"], inp["tris"], SHAPE, sdf=b.get("sdf"), record=b.get("record"),
                                                                  workspace=b.get("workspace"))))

    def specified(self, res):
        return dict(res, record=res["record"][:4])            # the four slots include/afx.h names


class MeshPointDistance(Case):
    outputs = {"dist": (F32, (5,)), "record": (I64, (8,))}

    def call(self, b):
        inp = _inputs()
        return dict(zip(("dist", "record"), _eng().mesh_point_distance_record(inp["points32"], inp["verts"], inp["tris"], dist=b.get("dist"),
                                                                              record=b.get("record"))))

    specified = MeshSdf.specified


class CentrelineGraph(Case):
    outputs = {"node_labels": (I32, SHAPE), "branch_labels": (I32, SHAPE), "path_voxels": (I32, (N,)), "branches": (I64, (CAP, 16)),
               "record": (I64, (16,))}

    def workspace(self):
        return _lib().afx_centreline_graph_workspace_bytes(*SHAPE)

    def call(self, b):
        inp = _inputs()
        return dict(zip(self.outputs, _eng().centreline_graph_record(inp["mask"], inp["d2"], None, CAP, b.get("node_labels"), b.get("branch_labels"),
                                                                     b.get("path_voxels"), b.get("branches"), b.get("record"), b.get("workspace"))))

    def specified(self, res):
        rec = res["record"].tolist()                        # path_voxels up to record[2], rows up to min(B, max_branches) (include/afx.h)
        return dict(res, path_voxels=res["path_voxels"][:rec[2]], branches=res["branches"][:min(rec[4], CAP)])


class Prune(Case):
    outputs = {"out": (U8, SHAPE), "record": (I64, (8,))}

    def workspace(self):
        return _lib().afx_prune_spurs_workspace_bytes(*SHAPE)

    def call(self, b):
        inp = _inputs()
        return dict(zip(("out", "record"), _eng().prune_record(inp["mask"], inp["d2"], 1.0, 2, 0, b.get("out"), b.get("record"), b.get("workspace"))))


class Frangi3D(Case):
    outputs = {"out": (F64, SHAPE), "scale_index": (U8, SHAPE)}

    def workspace(self):
        return _lib().afx_frangi_3d_workspace_bytes(*SHAPE, 1)

    def call(self, b):
        return dict(zip(("out", "scale_index"), _eng().frangi_3d_record(_inputs()["ramp"], (1.0,), out=b.get("out"), scale_index=b.get("scale_index"),
                                                                        workspace=b.get("workspace"))))


CASES = {"surface_metrics_record": SurfaceMetrics(), "components_record": Components(), "components_filter": ComponentsFilter(),
         "skeleton_record": Skeleton(), "isosurface_record": Isosurface(), "mesh_measures_record": MeshMeasures(), "mesh_sdf_record": MeshSdf(),
         "mesh_point_distance_record": MeshPointDistance(), "centreline_graph_record": CentrelineGraph(), "prune_record": Prune(),
         "frangi_3d_record": Frangi3D()}


def _bytes(t):
    return t.reshape(-1).view(U8)


def _painted(dtype, shape):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    _bytes(t).fill_(0xA5)
    return t


def _count(shape):
    return int(np.prod(shape))


def _violations(dtype, shape):
    """what -> a malformed stand-in for a (dtype, shape) buffer, each a view into an allocation at least as large as the right buffer"""
    n = _count(shape)
    assert n >= 2
    return {"dtype": torch.empty(shape, dtype=SAME_SIZE[dtype], device=DEV),
            "strided": torch.empty(2 * n, dtype=dtype, device=DEV)[::2],
            "short": torch.empty(n, dtype=dtype, device=DEV)[:n - 1]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_passed_buffers_are_returned_and_hold_what_an_allocating_call_returns(name):
    case = CASES[name]
    auto = case.call({})
    given = {k: _painted(dtype, shape) for k, (dtype, shape) in case.outputs.items()}
    need = case.workspace()
    if need is not None:
        given["workspace"] = _painted(U8, (int(need),))
    res = case.call(given)
    torch.cuda.synchronize()
    assert res.keys() == case.outputs.keys() == auto.keys()
    for k in res:
        assert res[k] is given[k], (name, k)
    want, got = case.specified(auto), case.specified(res)
    for k in want:
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape and torch.equal(_bytes(want[k]), _bytes(got[k])), (name, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_malformed_buffer_is_refused_by_name_before_any_launch(name):
    case = CASES[name]
    specs = dict(case.outputs)
    specs.update({k: (dtype, shape) for k, (dtype, shape, _) in case.inputs.items()})
    for bad_name, (dtype, shape) in specs.items():
        for what, bad in _violations(dtype, shape).items():
            bufs = {k: _painted(d, s) for k, (d, s) in case.outputs.items()}
            before = {k: v.clone() for k, v in bufs.items() if k != bad_name}
            bufs[bad_name] = bad
            with pytest.raises(ValueError, match=rf"\b{bad_name} must be "):
                case.call(bufs)
            torch.cuda.synchronize()
            for k, v in before.items():
                assert torch.equal(_bytes(bufs[k]), _bytes(v)), (name, bad_name, what, "a refused call wrote to", k)


@pytest.mark.parametrize("name", sorted(set(CASES) - {"components_filter", "mesh_point_distance_record"}))      # (these two take no workspace)
def test_a_strided_workspace_is_refused(name):
    case = CASES[name]
    assert case.workspace() is not None
    bufs = {k: _painted(d, s) for k, (d, s) in case.outputs.items()}
    before = {k: v.clone() for k, v in bufs.items()}
    bufs["workspace"] = torch.empty(2 * int(case.workspace()), dtype=U8, device=DEV)[::2]
    with pytest.raises(ValueError, match="workspace"):
        case.call(bufs)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(_bytes(bufs[k]), _bytes(v)), (name, "a refused call wrote to", k)


# ---- the families that checked their buffers before the shared helper: one wrapper and one buffer of each ----
def _family_calls():
    eng, inp = _eng(), _inputs()
    hull = dict(records=inp["records"], dist=inp["images"], n_views=2, width=8, height=8, margin_px=1.0)
    xray = dict(records=inp["records"], n_views=2, width=8, height=8, near=40.0, far=60.0, n_samples=4)
    first, last = torch.zeros(5, dtype=I32, device=DEV), torch.full((5,), 4, dtype=I32, device=DEV)
    seg = torch.zeros(2, eng.VIEWMAP_SEGMENT_DOUBLES, dtype=F64, device=DEV)
    seg_branch = torch.ones(2, dtype=I32, device=DEV)
    planes, table = torch.zeros(2, 9, dtype=F64, device=DEV), torch.zeros(3, 4, dtype=F64, device=DEV)
    return {
        "pose": ("out", F64, (2, 16), lambda t: eng.pose_compose(inp["records"], torch.zeros(2, 6, dtype=F64, device=DEV), out=t)),
        "territory": ("d2", I32, SHAPE, lambda t: eng.feature_transform_record(inp["mask"], d2=t)),
        "hull": ("seen", U16, SHAPE, lambda t: eng.visual_hull_record(hull, SHAPE, None, 1.0, seen=t)),
        "x-ray": ("acc", F64, SHAPE, lambda t: eng.xray_backproject(inp["images"], xray, SHAPE, acc=t)),
        "lumen": ("profile", F64, (5, 8), lambda t: eng.lumen_profile_record(inp["ramp"], inp["points"], first, last, inp["ident"], ISO, 8, 0.5, 4,
                                                                             profile=t)),
        "reformat": ("out", F64, (2, 3), lambda t: eng.reformat_planes_record(inp["ramp"], planes, table, inp["ident"], out=t)),
        "view map": ("count", U16, (2, 8, 8), lambda t: eng.view_map_record(seg, seg_branch, inp["records"], 8, 8, n_branches=1, out={"count": t})),
        "mesh SDF": ("sdf", F32, SHAPE, lambda t: eng.mesh_sdf_record(inp["verts"], inp["tris"], SHAPE, sdf=t)),
        "TV": ("out", F64, SHAPE, lambda t: eng.tv_denoise_3d(inp["ramp"].double(), 0.1, 2, out=t)),
    }


@pytest.mark.parametrize("family", ["pose", "territory", "hull", "x-ray", "lumen", "reformat", "view map", "mesh SDF", "TV"])
def test_the_families_that_already_checked_still_do(family):
    name, dtype, shape, call = _family_calls()[family]
    for what, bad in _violations(dtype, shape).items():
        with pytest.raises(ValueError, match=rf": {name} must be "):
            call(bad)
    torch.cuda.synchronize()
