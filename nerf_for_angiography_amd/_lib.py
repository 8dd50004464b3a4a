"""ctypes binding of libafx.so (include/afx.h).  There is NO fallback: if the HIP library is
missing or a call fails, an exception is raised."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libafx.so")

ACT = {"relu": 0, "tanh": 1, "sine": 2}
ENC = {"none": 0, "barf": 1, "fourier": 2}
PREC = {"f32": 0, "bf16x3": 1, "bf16": 2, "f16": 3, "f16s8": 4}
RAYS_ARRAYS, RAYS_POSE = 0, 1
DEPTH_UNIFORM_MID, DEPTH_SHARED_Z, DEPTH_PER_RAY_Z, DEPTH_STRATIFIED = 0, 1, 2, 3
(Q_PARAM_COUNT, Q_K0, Q_PREPARED_BYTES, Q_FWD_WORKSPACE, Q_BWD_WORKSPACE_MIN, Q_BWD_WORKSPACE_FULL, Q_BWD_INPUTS_WORKSPACE_MIN,
 Q_BWD_INPUTS_WORKSPACE_FULL) = range(8)
SAMPLING = {"frangi": 0, "segmentation": 1}                                 # AFX_SAMPLING_* (include/afx.h)
GRID_JITTER_TAG, GRID_SELECT_TAG = 0x47524944 << 32, 0x53454C43 << 32      # Philox stream tags of the grid refresh (include/afx.h)


class AfxError(RuntimeError):
    pass


class ModelDesc(C.Structure):
    _fields_ = [("n_in", C.c_int32), ("enc", C.c_int32), ("n_freq", C.c_int32), ("width", C.c_int32),
                ("n_hidden", C.c_int32), ("act", C.c_int32), ("act_w0", C.c_float)]


class RenderArgs(C.Structure):
    _fields_ = [("n_rays", C.c_int64), ("n_samples", C.c_int32), ("ray_mode", C.c_int32),
                ("origins", C.c_void_p), ("dirs", C.c_void_p), ("poses", C.c_void_p), ("ray_ids", C.c_void_p),
                ("ray_id0", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("focal", C.c_double),
                ("depth_mode", C.c_int32), ("t_near", C.c_float), ("t_far", C.c_float), ("z", C.c_void_p),
                ("pixel", C.c_void_p), ("sigma", C.c_void_p), ("tau", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("jitter_seed", C.c_uint64), ("jitter_stream", C.c_uint64)]


class GridDesc(C.Structure):
    _fields_ = [("roi_aabb", C.c_float * 6), ("resolution", C.c_int32 * 3)]


class GridRefreshArgs(C.Structure):
    _fields_ = [("grid", GridDesc), ("occs", C.c_void_p), ("binary", C.c_void_p), ("bits", C.c_void_p), ("all_cells", C.c_int32),
                ("n_draw", C.c_int64), ("seed", C.c_uint64), ("step", C.c_int64), ("step_dev", C.c_void_p), ("occ_thre", C.c_float),
                ("ema_decay", C.c_float), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class MarchArgs(C.Structure):
    _fields_ = [("origins", C.c_void_p), ("dirs", C.c_void_p), ("n_rays", C.c_int64), ("has_aabb", C.c_int32),
                ("scene_aabb", C.c_float * 6), ("has_near", C.c_int32), ("has_far", C.c_int32), ("near_plane", C.c_float),
                ("far_plane", C.c_float), ("step", C.c_float), ("grid_bits", C.c_void_p), ("grid", GridDesc)]


class MarchTrainArgs(C.Structure):
    _fields_ = [("march", MarchArgs), ("early_stop_eps", C.c_float), ("alpha_thre", C.c_float), ("target", C.c_void_p), ("inv_n", C.c_float),
                ("pixel", C.c_void_p), ("grad_flat", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("n_candidates", C.c_int64), ("n_kept", C.c_int64), ("n_groups", C.c_int64), ("workspace_needed", C.c_size_t)]


class MarchRenderArgs(C.Structure):
    _fields_ = [("march", MarchArgs), ("ray_mode", C.c_int32), ("poses", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("focal", C.c_double), ("ray_id0", C.c_int64), ("n_rays", C.c_int64), ("early_stop_eps", C.c_float), ("alpha_thre", C.c_float),
                ("pixel", C.c_void_p), ("binary_pixel", C.c_void_p), ("binary_thresh", C.c_float), ("kept_counts", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("n_candidates", C.c_int64), ("workspace_needed", C.c_size_t)]


class TrainRoundArgs(C.Structure):
    _fields_ = [("step_dev", C.c_void_p), ("lr_table", C.c_void_p), ("n_table", C.c_int64), ("lr_dev", C.c_void_p), ("skip", C.c_void_p),
                ("loss", C.c_void_p), ("counts", C.c_void_p), ("round_len", C.c_int64), ("loss_hist", C.c_void_p), ("counts_hist", C.c_void_p),
                ("skip_hist", C.c_void_p), ("last_loss", C.c_void_p), ("n_marched", C.c_void_p)]


_SIGS = {
    "afx_create": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(C.c_void_p)]),
    "afx_destroy": (None, [C.c_void_p]),
    "afx_last_error": (C.c_char_p, []),
    "afx_query": (C.c_int64, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64]),
    "afx_param_layout": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "afx_prepare_weights": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "afx_mlp_infer": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
    "afx_mlp_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "afx_mlp_backward_inputs": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p]),
    "afx_render_backward_inputs": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(RenderArgs), C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "afx_render_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(RenderArgs), C.c_void_p]),
    "afx_render_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(RenderArgs), C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "afx_train_step_mse": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(RenderArgs), C.c_void_p, C.c_float, C.c_void_p,
                                     C.c_void_p]),
    "afx_composite_dense": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_composite_dense_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_composite_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                       C.c_void_p]),
    "afx_composite_packed_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_ray_entropy_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_ray_entropy_packed_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                                  C.c_void_p, C.c_void_p]),
    "afx_ray_entropy_dense": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_ray_entropy_dense_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p]),
    "afx_project_volume": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.c_float, C.POINTER(RenderArgs), C.c_int, C.c_void_p]),
    "afx_topk_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "afx_topk_indices": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "afx_sample_batches_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "afx_sample_batches": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "afx_sample_batches_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    "afx_train_round_advance": (C.c_int, [C.POINTER(TrainRoundArgs), C.c_void_p]),
    "afx_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "afx_set_encoding_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_profile_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "afx_fine_depths": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                  C.c_void_p, C.c_void_p]),
    "afx_fine_depths_from_tau": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p]),
    "afx_grid_points": (C.c_int, [C.POINTER(GridDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "afx_grid_update": (C.c_int, [C.POINTER(GridDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p]),
    "afx_grid_binarize": (C.c_int, [C.POINTER(GridDesc), C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_grid_pack": (C.c_int, [C.POINTER(GridDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_grid_select_workspace_bytes": (C.c_size_t, [C.POINTER(GridDesc)]),
    "afx_grid_select_cells": (C.c_int, [C.POINTER(GridDesc), C.c_void_p, C.c_int64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "afx_grid_refresh_workspace_bytes": (C.c_int64, [C.POINTER(GridDesc), C.c_int64, C.c_int32]),
    "afx_grid_refresh": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(GridRefreshArgs), C.c_void_p]),
    "afx_hier_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "afx_hier_train_step_mse": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(RenderArgs), C.c_int32, C.c_void_p, C.c_void_p, C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_pack_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_train_step_packed_mse": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "afx_march_count": (C.c_int, [C.POINTER(MarchArgs), C.c_void_p, C.c_void_p]),
    "afx_march_write": (C.c_int, [C.POINTER(MarchArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_march_visibility": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_march_train_step_mse": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(MarchTrainArgs), C.c_void_p]),
    "afx_march_max_steps": (C.c_int64, [C.POINTER(MarchArgs)]),
    "afx_march_train_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int64, C.c_int64]),
    "afx_march_train_step_mse_capturable": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(MarchTrainArgs), C.c_void_p, C.c_void_p,
                                                      C.c_void_p]),
    "afx_march_single_eval_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int64, C.c_int64]),
    "afx_march_train_step_mse_single_eval": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(MarchTrainArgs), C.c_void_p, C.c_void_p,
                                                       C.c_void_p]),
    "afx_march_render_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64, C.c_int64]),
    "afx_march_render": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(MarchRenderArgs), C.c_void_p]),
    "afx_ray_offsets": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_march_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_sample_keys": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "afx_gather_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "afx_philox_uniform": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p]),
    "afx_frangi_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "afx_frangi": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_int32, C.c_double, C.c_double, C.c_int32,
                             C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_distance_transform_edt_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "afx_distance_transform_edt": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_sampling_weights_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "afx_sampling_weights": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_int32,
                                       C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_ssim_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "afx_ssim": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                           C.c_void_p]),
    "afx_volume_grid": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_float,
                                  C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]),
    "afx_distance_transform_edt_3d_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "afx_distance_transform_edt_3d": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_surface_metrics_3d_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "afx_surface_metrics_3d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_double, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_label_components_3d_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "afx_label_components_3d": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_filter_components_3d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32,
                                           C.c_void_p, C.c_void_p]),
    "afx_skeletonize_3d_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "afx_skeletonize_3d": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    "afx_simple_point_26": (C.c_int, [C.c_uint32]),
    "afx_isosurface_3d_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "afx_isosurface_3d": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.POINTER(C.c_double), C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_mesh_measures_workspace_bytes": (C.c_size_t, []),
    "afx_mesh_measures": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p,
                                    C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_mesh_sdf_3d_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "afx_mesh_sdf_3d": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_mesh_point_distance": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "afx_centreline_graph_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "afx_centreline_graph": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_prune_spurs_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "afx_prune_spurs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_frangi_3d_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "afx_frangi_3d": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_int32, C.c_double, C.c_double,
                                C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "afx_lumen_profile": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_visual_hull": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_grid_apply_mask": (C.c_int, [C.POINTER(GridDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_xray_project": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_xray_backproject": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]),
    "afx_tv_denoise_3d_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "afx_tv_denoise_3d": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "afx_view_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_reformat_planes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "afx_pose_chamfer": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_pose_compose": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "afx_pose_select": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_pose_lm_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "afx_feature_transform_3d": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afx_label_overlap_3d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
}

_libs = {}


def exported_symbols():
    """Every entry point include/afx.h declares."""
    return sorted(_SIGS)


def load(variant: str = ""):
    """Load libafx.so (or a build variant such as the race-detector build "safe" = libafx_safe.so); raise loudly when
    it has not been built."""
    if variant in _libs:
        return _libs[variant]
    # torch first: it ships its own libamdhip64.so.7; libafx.so must bind to THAT runtime (the one torch's
    # allocator and streams live in), not to a second copy pulled in through its RUNPATH.
    import torch  # noqa: F401
    path = LIB_PATH if not variant else os.path.join(_HERE, "csrc", f"libafx_{variant}.so")
    if not os.path.exists(path):
        raise AfxError(f"HIP library not built: {path} is missing. Run `python -m nerf_for_angiography_amd.build` "
                       "(needs hipcc, --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _libs[variant] = lib
    return lib


def check(rc, what="afx call", lib=None):
    if rc != 0:
        msg = (lib or load()).afx_last_error()
        raise AfxError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
