"""The host side of the wrappers of nerf_for_angiography_amd/engine.py, without a device: the buffer vocabulary (_on_gpu, _buffer, _out,
_scratch, _volume_side_ok) on CPU tensors, and one table over every public wrapper that takes a tensor - the analysis wrappers and the
training, grid, march and sampler wrappers (Engine's methods on the smallest model the library admits) - called with CPU tensors of
otherwise valid dtype and shape, each refuses with AfxError "... there is no CPU path" before anything else happens."""
import functools

import numpy as np
import pytest
import torch

from nerf_for_angiography_amd import engine
from nerf_for_angiography_amd.engine import AfxError

CPU = torch.device("cpu")
SHAPE = (3, 4, 5)


def _inputs():
    f64, i32 = torch.float64, torch.int32
    vol = torch.rand(SHAPE, dtype=torch.float32)
    mask = torch.ones(SHAPE, dtype=torch.uint8)
    d2 = torch.ones(SHAPE, dtype=i32)
    verts = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=torch.float32)
    tris = torch.tensor([[0, 1, 2]], dtype=i32)
    pts32 = torch.rand(5, 3, dtype=torch.float32)
    pts = torch.rand(5, 3, dtype=f64)
    first, last = torch.zeros(5, dtype=i32), torch.full((5,), 4, dtype=i32)
    ident = np.asarray(engine._IDENTITY_AFFINE, np.float64)
    poses = np.tile(np.eye(4), (2, 1, 1))
    records = torch.from_numpy(engine.hull_view_records(poses, 100.0))
    images = torch.rand(2, 8, 8, dtype=f64)
    hull = dict(records=records, dist=images, n_views=2, width=8, height=8, margin_px=1.0)
    pose = dict(records=records, field=images, n_views=2, width=8, height=8, poses=poses)
    xray = dict(records=records, n_views=2, width=8, height=8, near=1.0, far=2.0, n_samples=4)
    seg = torch.zeros(2, engine.VIEWMAP_SEGMENT_DOUBLES, dtype=f64)
    seg_branch = torch.ones(2, dtype=i32)
    graph = dict(branch_labels=d2, node_labels=torch.zeros(SHAPE, dtype=i32), n_branches=1, n_nodes=0, shape=SHAPE,
                 path_voxels=torch.arange(5), branch_size=torch.tensor([5]))
    rec8 = torch.zeros(8, dtype=torch.int64)
    return locals()


I = _inputs()
e = engine

# name -> the call; every tensor lives on the CPU and has the dtype and shape the wrapper documents
NO_CPU_PATH = {
    "frangi": lambda: e.frangi(I["images"]),
    "distance_transform_edt": lambda: e.distance_transform_edt(I["images"]),
    "sampling_weights": lambda: e.sampling_weights(I["images"]),
    "ssim": lambda: e.ssim(I["images"], I["images"]),
    "distance_transform_edt_3d": lambda: e.distance_transform_edt_3d(I["mask"]),
    "surface_metrics_record": lambda: e.surface_metrics_record(I["vol"], I["vol"], 0.5, 0.5),
    "surface_metrics_3d": lambda: e.surface_metrics_3d(I["vol"], I["vol"], 0.5, 0.5),
    "components_record": lambda: e.components_record(I["mask"]),
    "label_components_3d": lambda: e.label_components_3d(I["mask"]),
    "filter_components_3d": lambda: e.filter_components_3d(I["mask"]),
    "components_filter": lambda: e.components_filter(I["d2"], I["d2"].reshape(-1), I["rec8"]),
    "skeleton_record": lambda: e.skeleton_record(I["mask"], 3),
    "skeletonize_3d": lambda: e.skeletonize_3d(I["mask"]),
    "isosurface_record": lambda: e.isosurface_record(I["vol"], 0.5),
    "extract_isosurface": lambda: e.extract_isosurface(I["vol"], 0.5),
    "mesh_measures_record": lambda: e.mesh_measures_record(I["verts"], I["tris"], I["rec8"]),
    "mesh_measures": lambda: e.mesh_measures(I["verts"], I["tris"]),
    "mesh_sdf_record": lambda: e.mesh_sdf_record(I["verts"], I["tris"], (2, 2, 2)),
    "mesh_signed_distance": lambda: e.mesh_signed_distance(I["verts"], I["tris"], (2, 2, 2)),
    "mesh_point_distance_record": lambda: e.mesh_point_distance_record(I["pts32"], I["verts"], I["tris"]),
    "mesh_point_distance": lambda: e.mesh_point_distance(I["pts32"], I["verts"], I["tris"]),
    "centreline_graph_record": lambda: e.centreline_graph_record(I["mask"], I["d2"]),
    "centreline_graph": lambda: e.centreline_graph(I["mask"], I["d2"]),
    "prune_record": lambda: e.prune_record(I["mask"], I["d2"], 1.0, 2),
    "prune_spurs": lambda: e.prune_spurs(I["mask"], I["d2"]),
    "lumen_profile_record": lambda: e.lumen_profile_record(I["vol"], I["pts"], I["first"], I["last"], I["ident"], 0.5, 8, 0.5, 4),
    "lumen_profile": lambda: e.lumen_profile(I["vol"], I["pts"], I["first"], I["last"]),
    "centreline_lumen_profile": lambda: e.centreline_lumen_profile(I["graph"], I["vol"], I["ident"], 0.5),
    "reformat_planes_record": lambda: e.reformat_planes_record(I["vol"], torch.zeros(2, 9, dtype=torch.float64),
                                                               torch.zeros(3, 4, dtype=torch.float64), I["ident"]),
    "straighten_volume": lambda: e.straighten_volume(I["vol"], I["pts"]),
    "cpr_images": lambda: e.cpr_images(I["vol"], I["pts"]),
    "centreline_cpr": lambda: e.centreline_cpr(I["graph"], I["vol"], I["ident"]),
    "frangi_3d_record": lambda: e.frangi_3d_record(I["vol"]),
    "frangi_3d": lambda: e.frangi_3d(I["vol"]),
    "visual_hull_views": lambda: e.visual_hull_views(I["poses"], torch.ones(2, 8, 8, dtype=torch.uint8), 100.0),
    "visual_hull_record": lambda: e.visual_hull_record(I["hull"], SHAPE, None, 1.0),
    "visual_hull": lambda: e.visual_hull(I["hull"], SHAPE),
    "view_map_record": lambda: e.view_map_record(I["seg"], I["seg_branch"], I["records"], 8, 8, n_branches=1),
    "view_map": lambda: e.view_map((I["seg"], I["seg_branch"]), I["records"], 8, 8),
    "pose_views": lambda: e.pose_views(I["poses"], torch.ones(2, 8, 8, dtype=torch.uint8), 100.0),
    "pose_compose": lambda: e.pose_compose(I["records"], torch.zeros(2, 6, dtype=torch.float64)),
    "pose_chamfer_record": lambda: e.pose_chamfer_record(I["pose"], I["pts"], None, None, I["records"], torch.arange(2, dtype=torch.int32), 8.0),
    "pose_chamfer": lambda: e.pose_chamfer(I["pts"], None, I["pose"]),
    "register_poses_record": lambda: e.register_poses_record(I["pose"], I["pts"], None, None, I["records"]),
    "register_poses": lambda: e.register_poses(I["pts"], None, I["pose"]),
    "centreline_register_poses": lambda: e.centreline_register_poses(I["graph"], I["pose"]),
    "feature_transform_record": lambda: e.feature_transform_record(I["mask"]),
    "feature_transform_3d": lambda: e.feature_transform_3d(I["mask"]),
    "label_overlap_record": lambda: e.label_overlap_record(I["d2"], I["mask"], 3),
    "label_overlap_3d": lambda: e.label_overlap_3d(I["d2"], I["mask"]),
    "branch_territories": lambda: e.branch_territories(I["graph"]),
    "xray_views": lambda: e.xray_views(I["poses"], 100.0, 8, 8, 1.0, 2.0, 4, device="cpu"),
    "xray_project": lambda: e.xray_project(I["vol"].double(), I["xray"]),
    "xray_backproject": lambda: e.xray_backproject(I["images"], I["xray"], SHAPE),
    "tv_denoise_3d": lambda: e.tv_denoise_3d(I["vol"].double(), 0.1),
    "sirt_reconstruct": lambda: e.sirt_reconstruct(I["xray"], I["images"], SHAPE),
}


# ---- the training, grid, march and sampler wrappers: 9 rays of 6 samples, 3 groups, a 5 x 3 x 7 grid (105 cells, 4 words), n_draw 4, 2 batches of 3 ----
R, S, G, NF, RES, NC, BOX = 9, 6, 3, 2, (5, 3, 7), 105, [0.0, 0.0, 0.0, 5.0, 3.0, 7.0]
F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8


@functools.lru_cache(maxsize=None)
def _model():
    """The smallest model the library admits, with CPU stand-ins for its buffers."""
    eng = e.Engine(64, 1)
    return eng, torch.zeros(eng.param_count), torch.zeros(eng.param_count)


def _prep(prec):
    """CPU bytes of the size Engine.prepare allocates at `prec`."""
    from nerf_for_angiography_amd import _lib
    eng = _model()[0]
    return torch.zeros(int(eng.lib.afx_query(eng.h, _lib.Q_PREPARED_BYTES, _lib.PREC[prec], 0, 0)), dtype=U8)


def _t():
    o, d = torch.zeros(R, 3), torch.ones(R, 3)
    return dict(o=o, d=d, tgt=torch.zeros(R), pix=torch.zeros(R), pts=torch.zeros(R, 3), z=torch.linspace(0.1, 0.9, S), u=torch.rand(R, NF),
                raw=torch.zeros(R, S), bits=torch.zeros(4, dtype=I32), occs=torch.zeros(NC), b8=torch.zeros(NC, dtype=U8),
                acc=e.RenderSpec(R, S, origins=o, dirs=d, mode="acc", t_near=0.0, t_far=1.0),
                dense=e.RenderSpec(R, S, origins=o, dirs=d, mode="dense", z=torch.linspace(0.1, 0.9, S)),
                packed=e.PackedGroups(R, G, torch.zeros(R + 1, dtype=I64), torch.zeros(G, dtype=I32), torch.zeros(32 * G), torch.zeros(32 * G)),
                march=dict(grid_bits=torch.zeros(4, dtype=I32), grid_aabb=BOX, grid_res=RES),
                ri=torch.zeros(R * S, dtype=I32), n=torch.zeros(R * S), off=torch.arange(R + 1) * S, step=torch.zeros((), dtype=I64),
                one=torch.zeros(1), one64=torch.zeros(1, dtype=I64), three64=torch.zeros(3, dtype=I64))


T = _t()
NO_CPU_PATH.update({
    "Engine.prepare": lambda: _model()[0].prepare(_model()[1], None, "f32"),
    "Engine.infer": lambda: _model()[0].infer(_prep("f32"), T["pts"], "f32"),
    "Engine.encoding_grad": lambda: _model()[0].encoding_grad(_model()[1], torch.zeros(3)).__enter__(),
    "Engine.mlp_backward": lambda: _model()[0].mlp_backward(_prep("f32"), T["pts"], T["tgt"], _model()[2], "f32"),
    "Engine.mlp_backward_inputs": lambda: _model()[0].mlp_backward_inputs(_prep("f32"), T["pts"], T["tgt"], None, torch.zeros(R, 3), "f32"),
    "Engine.render_forward": lambda: _model()[0].render_forward(_prep("f32"), T["acc"], "f32"),
    "Engine.render_backward": lambda: _model()[0].render_backward(_prep("f32"), T["acc"], T["pix"], T["tgt"], _model()[2], "f32"),
    "Engine.render_backward_inputs": lambda: _model()[0].render_backward_inputs(_prep("f32"), T["acc"], T["pix"], T["tgt"], None, torch.zeros(R, 3),
                                                                               torch.zeros(R, 3), "f32"),
    "Engine.train_step_mse": lambda: _model()[0].train_step_mse(_prep("f16s8"), T["acc"], T["tgt"], 1.0 / R, _model()[2], "f16s8"),
    "Engine.hier_train_step_mse": lambda: _model()[0].hier_train_step_mse(_prep("f16s8"), T["dense"], NF, T["u"], T["tgt"], 1.0 / R, _model()[2], "f16s8"),
    "Engine.train_step_packed_mse": lambda: _model()[0].train_step_packed_mse(_prep("f16s8"), T["o"], T["d"], T["packed"], T["tgt"], 1.0 / R, _model()[2],
                                                                             "f16s8"),
    "Engine.march_train_step_mse": lambda: _model()[0].march_train_step_mse(_prep("f16s8"), T["o"], T["d"], T["tgt"], 1.0 / R, _model()[2], "f16s8", BOX,
                                                                           0.0, 9.0, 0.5, 1e-4, 1e-2, **T["march"]),
    "Engine.march_train_step_mse_capturable": lambda: _model()[0].march_train_step_mse_capturable(
        _prep("f16s8"), T["o"], T["d"], T["tgt"], 1.0 / R, _model()[2], "f16s8", BOX, 0.0, 9.0, 0.5, 1e-4, 1e-2, pixel=torch.zeros(R),
        counts=torch.zeros(3, dtype=I64), skip=torch.zeros(1), **T["march"]),
    "Engine.march_train_step_mse_single_eval": lambda: _model()[0].march_train_step_mse_single_eval(
        _prep("f16s8"), T["o"], T["d"], T["tgt"], 1.0 / R, _model()[2], "f16s8", BOX, 0.0, 9.0, 0.5, 1e-4, 1e-2, **T["march"]),
    "Engine.march_render": lambda: _model()[0].march_render(_prep("f16s8"), "f16s8", BOX, 0.0, 9.0, 0.5, 1e-4, 1e-2, origins=T["o"], dirs=T["d"],
                                                           **T["march"]),
    "pack_groups": lambda: e.pack_groups(T["off"], T["n"], T["n"]),
    "composite_dense": lambda: e.composite_dense(T["raw"], T["d"], T["z"]),
    "composite_dense_backward": lambda: e.composite_dense_backward(T["raw"], T["d"], T["z"], T["pix"], T["tgt"]),
    "composite_packed": lambda: e.composite_packed(T["n"], T["ri"], T["n"], T["n"], R),
    "composite_packed_backward": lambda: e.composite_packed_backward(T["n"], T["ri"], T["n"], T["n"], R, T["pix"], T["tgt"]),
    "ray_entropy_packed": lambda: e.ray_entropy_packed(T["n"], T["ri"], T["pix"], R),
    "ray_entropy_packed_backward": lambda: e.ray_entropy_packed_backward(T["n"], T["ri"], T["pix"], torch.ones(R, 2), T["tgt"], out=torch.zeros(R * S)),
    "ray_entropy_dense": lambda: e.ray_entropy_dense(T["raw"], T["pix"]),
    "ray_entropy_dense_backward": lambda: e.ray_entropy_dense_backward(T["raw"], T["pix"], torch.ones(R, 2), T["tgt"], out=torch.zeros(R, S)),
    "project_volume": lambda: e.project_volume(I["vol"], (0, 0, 0), (1, 1, 1), 0.0, T["z"], origins=T["o"], dirs=T["d"]),
    "fine_depths": lambda: e.fine_depths(T["z"], T["raw"], T["u"]),
    "fine_depths_from_tau": lambda: e.fine_depths_from_tau(T["raw"], T["raw"], T["u"]),
    "volume_grid": lambda: e.volume_grid(I["vol"], (0, 0, 0), (1, 1, 1), 0.0, -1.0, 1.0, 4),
    "grid_points": lambda: e.grid_points(BOX, RES, torch.zeros(4, dtype=I32), 4, jitter=torch.zeros(4, 3)),
    "grid_update": lambda: e.grid_update(BOX, RES, T["occs"], torch.zeros(4, dtype=I32), torch.zeros(4), 0.95, torch.zeros(NC)),
    "grid_binarize": lambda: e.grid_binarize(BOX, RES, T["occs"], 1e-2, T["b8"], T["bits"], torch.zeros(256, dtype=torch.float64)),
    "grid_pack": lambda: e.grid_pack(BOX, RES, T["b8"], T["bits"]),
    "grid_select_cells": lambda: e.grid_select_cells(BOX, RES, T["bits"], 4, 1, T["step"], cells=torch.zeros(8, dtype=I32), count=T["one64"],
                                                     workspace=torch.zeros(64, dtype=U8)),
    "grid_refresh": lambda: e.grid_refresh(_model()[0], _prep("f16s8"), "f16s8", BOX, RES, T["occs"], T["b8"], T["bits"], 4, False, 1, T["step"], 1e-2, 0.95,
                                           torch.zeros(64, dtype=U8)),
    "march": lambda: e.march(T["o"], T["d"], BOX, 0.0, 9.0, 0.5, **T["march"]),
    "march_visibility": lambda: e.march_visibility(T["n"], T["n"], T["n"], T["off"], 1e-4, 1e-2),
    "topk_indices": lambda: e.topk_indices(T["n"], 3),
    "RayBatchSampler": lambda: e.RayBatchSampler(T["o"], T["d"], T["pix"], torch.ones(R), 3),
    "sample_batches_dev": lambda: e.sample_batches_dev(torch.ones(R), 1, T["step"], 2, 3, out_idx=torch.zeros(2, 3, dtype=I64),
                                                       workspace=torch.zeros(64, dtype=U8)),
    "gather_rays": lambda: e.gather_rays(T["o"], T["d"], T["pix"], torch.zeros(3, dtype=I64), torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3)),
    "train_round_advance": lambda: e.train_round_advance(T["one64"], torch.zeros(5), T["one"], T["one"], T["one"], T["three64"], torch.zeros(2),
                                                         torch.zeros(2, 3, dtype=I64), torch.zeros(2), T["one"], T["one64"]),
    "sample_rays": lambda: e.sample_rays(T["o"], T["d"], T["pix"], torch.ones(R), 3, u=torch.rand(R)),
})


@pytest.mark.parametrize("name", sorted(NO_CPU_PATH))
def test_analysis_wrappers_have_no_cpu_path(name):
    with pytest.raises(AfxError, match="no CPU path"):
        NO_CPU_PATH[name]()


def test_on_gpu_is_the_one_sentence():
    for bad in (torch.zeros(3), np.zeros(3), None):
        with pytest.raises(AfxError, match=r"^unit: the thing must be a tensor on a GPU; there is no CPU path$"):
            engine._on_gpu(bad, "the thing", "unit")


def _violations(shape):
    """name of the violation -> a tensor that commits exactly that one against (float32, shape, cpu)"""
    n = int(np.prod(shape))
    return {"not a tensor": np.zeros(shape, np.float32), "dtype": torch.zeros(shape, dtype=torch.int32),
            "transposed": torch.zeros(shape[::-1], dtype=torch.float32).permute(*range(len(shape) - 1, -1, -1)),
            "short": torch.zeros(n - 1, dtype=torch.float32), "long": torch.zeros(n + 1, dtype=torch.float32)}


def test_buffer_accepts_the_right_tensor_and_names_every_violation():
    good = torch.zeros(SHAPE, dtype=torch.float32)
    assert engine._buffer(good, "buf", torch.float32, SHAPE, CPU, "unit") is good
    assert engine._buffer(good.reshape(-1), "buf", torch.float32, SHAPE, CPU, "unit") is not None      # the count, not the shape
    assert engine._buffer(good, "buf", (torch.float32, torch.float64), SHAPE, CPU, "unit") is good
    assert engine._buffer(good.double(), "buf", (torch.float32, torch.float64), SHAPE, CPU, "unit") is not None
    assert engine._buffer(good, "buf", torch.float32, good.numel(), CPU, "unit") is good                  # a count alone
    assert not _violations(SHAPE)["transposed"].is_contiguous() and _violations(SHAPE)["transposed"].shape == SHAPE
    for what, bad in _violations(SHAPE).items():
        with pytest.raises(ValueError, match=r"^unit: buf must be a contiguous torch\.float32 tensor of 60 elements") as err:
            engine._buffer(bad, "buf", torch.float32, SHAPE, CPU, "unit")
        assert "on cpu" in str(err.value) and "got" in str(err.value), what
    with pytest.raises(ValueError, match="buf.*float32 or torch.float64"):
        engine._buffer(good.int(), "buf", (torch.float32, torch.float64), SHAPE, CPU, "unit")
    with pytest.raises(ValueError, match=r"buf .*shape \(3, 4, 5\).*got torch\.float32 \(60,\)"):        # the right count, the wrong shape
        engine._buffer(good.reshape(-1), "buf", torch.float32, SHAPE, CPU, "unit", exact_shape=True)
    assert engine._buffer(good, "buf", torch.float32, SHAPE, CPU, "unit", exact_shape=True) is good
    with pytest.raises(ValueError, match="buf"):                                                          # another device
        engine._buffer(good, "buf", torch.float32, SHAPE, torch.device("meta"), "unit")


def test_buffer_copy_makes_a_strided_input_contiguous_and_converts_nothing_else():
    table = torch.arange(15, dtype=torch.float32).reshape(3, 5).t()                 # a column-major [5, 3] table
    assert not table.is_contiguous()
    with pytest.raises(ValueError, match="unit: rays must be a contiguous"):       # without the keyword a strided tensor is refused
        engine._buffer(table, "rays", torch.float32, (5, 3), CPU, "unit")
    got = engine._buffer(table, "rays", torch.float32, (5, 3), CPU, "unit", exact_shape=True, copy=True)
    assert got.is_contiguous() and got.shape == table.shape and torch.equal(got, table) and got.data_ptr() != table.data_ptr()
    view = torch.arange(4.0)[:, None].expand(4, 3)                                  # a broadcast view
    assert torch.equal(engine._buffer(view, "rays", torch.float32, 12, CPU, "unit", copy=True), view.contiguous())
    good = torch.zeros(5, 3)
    assert engine._buffer(good, "rays", torch.float32, (5, 3), CPU, "unit", copy=True) is good      # a contiguous one is not copied
    for what, bad in _violations((5, 3)).items():
        if what != "transposed":
            with pytest.raises(ValueError, match=r"^unit: rays must be a torch\.float32 tensor of 15 elements"):
                engine._buffer(bad, "rays", torch.float32, (5, 3), CPU, "unit", copy=True)
    with pytest.raises(ValueError, match="unit: rays"):                            # another device: refused, not moved
        engine._buffer(good, "rays", torch.float32, (5, 3), torch.device("meta"), "unit", copy=True)
    with pytest.raises(ValueError, match=r"rays .*shape \(5, 3\)"):                # the count but not the shape
        engine._buffer(table.t(), "rays", torch.float32, (5, 3), CPU, "unit", exact_shape=True, copy=True)


def test_buffer_at_least_admits_a_longer_buffer_only():
    long, short = torch.zeros(7, 3), torch.zeros(4, 3)
    assert engine._buffer(long, "rows", torch.float32, (5, 3), CPU, "unit", at_least=True) is long
    with pytest.raises(ValueError, match="rows .*at least 15 elements"):
        engine._buffer(short, "rows", torch.float32, (5, 3), CPU, "unit", at_least=True)
    with pytest.raises(ValueError, match="rows"):
        engine._buffer(long, "rows", torch.float32, (5, 3), CPU, "unit")


def test_out_allocates_or_checks():
    t = engine._out(None, "buf", torch.int32, SHAPE, CPU, "unit")
    assert t.shape == SHAPE and t.dtype == torch.int32 and t.device == CPU
    one = engine._out(None, "buf", torch.int32, SHAPE, CPU, "unit", ok=False)
    assert one.shape == (1,) and one.dtype == torch.int32
    assert engine._out(None, "buf", torch.int64, 8, CPU, "unit").shape == (8,)
    assert engine._out(t, "buf", torch.int32, SHAPE, CPU, "unit") is t
    for what, bad in _violations(SHAPE).items():
        with pytest.raises(ValueError, match="unit: buf"):
            engine._out(bad, "buf", torch.float32, SHAPE, CPU, "unit")
    # a refused shape: the library reports the limits, so the count is not the wrapper's to judge - dtype and contiguity still are
    assert engine._out(t, "buf", torch.int32, (2000, 1, 1), CPU, "unit", ok=False) is t
    with pytest.raises(ValueError, match="unit: buf"):
        engine._out(t.float(), "buf", torch.int32, (2000, 1, 1), CPU, "unit", ok=False)


def test_scratch_reports_bytes():
    ws, nbytes = engine._scratch(None, 0, CPU, "unit")
    assert ws.dtype == torch.uint8 and ws.numel() == 1 and nbytes == 1
    ws, nbytes = engine._scratch(None, 100, CPU, "unit")
    assert ws.numel() == 100 and nbytes == 100
    mine = torch.zeros(5, dtype=torch.float32)
    assert engine._scratch(mine, 100, CPU, "unit") == (mine, 20)                  # numel x element_size; the size check is the library's
    for bad in (torch.zeros(4, 6)[:, ::2], np.zeros(8, np.uint8)):
        with pytest.raises(ValueError, match="unit: workspace"):
            engine._scratch(bad, 4, CPU, "unit")
    with pytest.raises(ValueError, match="unit: workspace"):
        engine._scratch(mine, 4, torch.device("meta"), "unit")


def test_volume_side_ok_is_the_library_limit():
    assert engine.EDT3D_MAX_SIDE == 1024
    assert engine._volume_side_ok((1, 1024, 7)) and engine._volume_side_ok(torch.Size((2, 3, 4)))
    for bad in ((0, 4, 4), (4, 1025, 4), (4, 4, -1)):
        assert not engine._volume_side_ok(bad)
