"""Training driver — mirror of the reference's nerf/run_nerf_acc.py (flags :25-47, hyper-parameters :126-183,
loop :263-441) on the MI355X hot path.

Same command-line flags, model dictionary, ray sampling (`sample_pixel_rays` with `distance_pixel_value`
weights), BARF schedule, learning-rate decay, evaluation cadence, best-PSNR / vessel-PSNR checkpointing and
early stopping.  Differences: the dataset comes from `load_data` (which the reference calls but never defines) or
is synthesised in memory; TensorBoard/pyvista outputs are replaced by a JSONL log.

Three iteration bodies (--march): `dense` (default) is ONE fused launch per ray chunk (`train_step_mse`: ray -> samples ->
MLP -> Beer-Lambert -> MSE -> backward; render + autograd with --precision f32); `grid` is the reference's own body,
run_nerf_acc.py:284-306 - acc_update_n_step for both grids, acc_ray_marching with the occupancy grid (HIP march / visibility
kernels, nerf/occupancy.py), then positions / get_predictions / acc_render_volume_density / mse_loss / backward as ONE fused pass
over the march's packed samples, march included, in one library call (`march_train_step_mse`; f16s8); `grid_ops` is the same body call for call through
the mirrored functions (also what `grid` does at the other precisions).  `--graph` (with `grid`, f16s8) replays that iteration, Adam
included, from a HIP graph captured once (`render.GridTrainGraph`): the sizes stay on the device and the host never waits for the GPU.
`--graph-grid-update` (with `--graph`) also replays the refresh of both occupancy grids every 16th iteration from HIP graphs
(`render.GridUpdateGraph`: the cells drawn on the device, no host synchronisation); without it the refresh stays eager.
`--graph-rounds` (with both) replays a whole refresh period - both refreshes, the draw of the 16 batches from a device step counter, 16
iterations with Adam and the learning-rate update - from one graph launch (`render.GridTrainRoundGraph`); same numbers, opt-in.
`--single-eval` (with `grid`, f16s8, with or without `--graph`) evaluates the model once per iteration: the training step's forward half over
the march's candidates doubles as the alpha pass.
`--entropy_weight LAMBDA` (with `grid_ops`) adds LAMBDA times the batch's mean ray entropy (`acc_ray_entropy`) to the loss.
`--grid_init hull` (with `grid` or `grid_ops`, `--binary True`) carves both occupancy grids with the visual hull of the training views
before training and keeps it as the ceiling of every grid update (`OccupancyGrid.carve_from_views`, `afx_visual_hull`).
`--save_sirt PATH.npy` (`--binary True` or CT-type data) writes, at the end of the run, the classical baseline: the SIRT reconstruction
of the attenuation volume from the training views on the 128^3 lattice of the occupancy grid's cell centres (`engine.sirt_reconstruct`);
`--sirt_tv_weight W` makes it SIRT-TV, a total-variation denoising step after every update (`engine.tv_denoise_3d`, `afx_tv_denoise_3d`).
`--save_poses PATH.csv` (`--binary True`) registers, at the end of the run, the pose of every training view to its vessel silhouette by
2D-3D chamfer registration of the final model's centreline (`engine.register_poses`, `afx_pose_chamfer`, `afx_pose_lm_step`) and writes
the given and the refined poses; `--pose_noise DEG UNITS` (`--synthetic`) hands training perturbed poses of images rendered at the true ones.
The training rays live on the GPU: one table (origins, directions, pixel, weight) built once, and every iteration's
batch is drawn there (weighted sampling without replacement, `engine.sample_rays`); --host_sampler restores the
reference's per-iteration pandas draw (`sample_pixel_rays`).

    python -m nerf_for_angiography_amd.nerf.run_nerf_acc --synthetic --n_iters 2000 --num_layers 4 --num_hidden_units 128
"""
from __future__ import annotations

import argparse
import ast
import json
import os
import time

import numpy as np
import torch

from ..engine import RenderSpec
from ..model.CPPN import CPPN
from ..phantomdata import dataset as ds
from .. import engine as _engine
from ..render import (render_rays, train_step_mse, march_train_step_mse, march_render, GridTrainGraph, GridUpdateGraph, GridTrainRoundGraph,
                      lr_decay_table)
from .nerf_helpers import sample_pixel_rays, get_predictions
from .nerf_helpers_acc import acc_ray_marching, acc_render_volume_density, acc_ray_entropy, acc_update_n_step
from .occupancy import OccupancyGrid, ContractionType
from . import checkpoint as _ckpt


def build_parser():
    p = argparse.ArgumentParser()
    # the reference's flags (nerf/run_nerf_acc.py:27-34), parsed as strings and cast the same way
    p.add_argument('--limited_size', help='Angle range to sample the projections in')
    p.add_argument('--number_angles', help='Number of projections to sample per axis')
    p.add_argument('--center_point', help='Center point for the angle sampling')
    p.add_argument('--binary', help='Whether images are binary or not')
    p.add_argument('--sampling_strategy', help='What sampling strategy to use, options: frangi, segmentation or random')
    p.add_argument('--data_name', help='Either CT data or LCA data')
    p.add_argument('--num_layers', help='Number of layers for MLP')
    p.add_argument('--num_hidden_units', help='Number of hidden units for MLP')
    # extensions
    p.add_argument('--synthetic', action='store_true', help='synthesise the dataset in memory instead of load_data')
    p.add_argument('--data_root', default='data')
    p.add_argument('--img_size', type=int, default=64)
    p.add_argument('--n_iters', type=int, default=500000)
    p.add_argument('--display_every', type=int, default=500)
    p.add_argument('--sample_size', type=int, default=75, help='rays per dimension per iteration (75^2 = 5625)')
    p.add_argument('--depth_samples', type=int, default=300)
    p.add_argument('--pos_enc', default='none', choices=['none', 'barf', 'fourier'])
    p.add_argument('--precision', default='f16s8', choices=['f32', 'bf16x3', 'bf16', 'f16', 'f16s8'],
                   help='arithmetic of the training step (include/afx.h); f16s8 = f16 with the backward stash kept as bf8')
    p.add_argument('--eval_precision', default='f16', choices=['f32', 'bf16x3', 'bf16', 'f16'])
    p.add_argument('--march', default='dense', choices=['dense', 'grid', 'grid_ops'],
                   help='dense: fused fixed-step march (one launch per ray chunk); grid: the reference loop with the occupancy grid, its body behind '
                        'the march (positions, get_predictions, acc_render_volume_density, mse, backward) as ONE fused packed step at the f16s8 '
                        'precision; grid_ops: the same loop call for call through the mirrored functions')
    p.add_argument('--graph', action='store_true',
                   help='--march grid --precision f16s8: capture the whole iteration (re-tiling, march, alpha pass, visibility, packed step, loss, '
                        'Adam) once into a HIP graph and replay it; sizes stay on the device and the host never waits for the GPU (the '
                        'occupancy-grid update every 16 iterations stays eager unless --graph-grid-update; counts and loss are read at the display '
                        'cadence only)')
    p.add_argument('--graph-grid-update', dest='graph_grid_update', action='store_true',
                   help='with --graph: refresh both occupancy grids every 16th iteration from HIP graphs too (render.GridUpdateGraph: the cells '
                        'are drawn on the device, afx_grid_refresh), so the host never waits for the GPU; the draw differs from the eager '
                        'refresh\'s torch draw')
    p.add_argument('--graph-rounds', dest='graph_rounds', action='store_true',
                   help='with --graph --graph-grid-update: one graph launch per 16 iterations (render.GridTrainRoundGraph) - both grid refreshes, '
                        'the draw of the 16 batches from a device step counter (afx_sample_batches_dev), then 16 times gather, step, Adam and the '
                        'learning-rate update (afx_train_round_advance); the host launches up to the next display point and reads nothing back '
                        'in between; same numbers as without the flag')
    p.add_argument('--single-eval', dest='single_eval', action='store_true',
                   help='--march grid --precision f16s8 --pos_enc none (with or without --graph): evaluate the model ONCE per iteration - the '
                        'training step\'s forward half over the march\'s candidates doubles as the alpha pass (afx_march_train_step_mse_single_eval)')
    p.add_argument('--adam', default='fused', choices=['fused', 'foreach'], help="PyTorch Adam implementation (same update rule)")
    p.add_argument('--host_sampler', action='store_true', help="draw each batch with pandas on the host (the reference's sample_pixel_rays)")
    p.add_argument('--barf_start', type=int, default=8000, help='--pos_enc barf: first iteration of the coarse-to-fine schedule')
    p.add_argument('--barf_stop', type=int, default=250000, help='--pos_enc barf: iteration at which every frequency band is open')
    p.add_argument('--checkpoint_every', type=int, default=0,
                   help='write the full training state (LOG_DIR/trainstate.pt: parameters, Adam state, both occupancy grids, counters, history, '
                        'RNG states; nerf/checkpoint.py) every N iterations, atomically; 0 (default) never writes one.  With --graph-rounds a '
                        'state can only be taken between rounds: N is rounded up to a multiple of the 16-iteration round.  A save waits for the '
                        'GPU, reads the state back and writes 27 MB with the two 128^3 grids (55-75 ms for the host half alone, '
                        'profiles/r10_resume.md: a hundred iterations of the grid loop) - keep N in the thousands.  A state whose loss or parameters are not finite is not written; when the run stops on a '
                        'non-finite loss the last state written is kept as LOG_DIR/trainstate-before-nonfinite.pt')
    p.add_argument('--resume', default=None, metavar='PATH',
                   help='continue from a training-state file (or the trainstate.pt in a directory) at its iteration, bit for bit; every '
                        'argument that changes the arithmetic must equal the saved run\'s (a mismatch names the fields)')
    p.add_argument('--entropy_weight', type=float, default=0.0, metavar='LAMBDA',
                   help='--march grid_ops: add LAMBDA * mean over the batch\'s rays of the per-ray entropy of the density profile to the loss '
                        '(get_ray_entropy of the reference, the sparse-view regulariser its packed loop leaves out; acc_ray_entropy, '
                        'afx_ray_entropy_packed); 0 (default): the MSE-only loop, and no `entropy` field in the log')
    p.add_argument('--save_mesh', default=None, metavar='PATH',
                   help='after training, write the final model\'s vessel surface to PATH (.stl: binary STL, .vtk: legacy VTK POLYDATA): the '
                        'density grid at depth_samples + 1 points per axis, meshed at --mesh_threshold by marching tetrahedra on the GPU '
                        '(afx_isosurface_3d), capped where it leaves the grid, in world coordinates; without the flag nothing changes')
    p.add_argument('--mesh_threshold', type=float, default=0.05, metavar='SIGMA',
                   help='--save_mesh: the density at which the surface is taken (default: the evaluation sweep\'s binary_thresh)')
    p.add_argument('--save_centreline', default=None, metavar='PATH',
                   help='after training, write the final model\'s vessel centreline to PATH (.vtk: legacy VTK POLYDATA LINES with the radius '
                        'per point): the density grid at depth_samples + 1 points per axis, thresholded at --mesh_threshold, thinned '
                        '(afx_skeletonize_3d), its spurs pruned (afx_prune_spurs, factor 1) and read as a graph (afx_centreline_graph), one '
                        'polyline per branch in world coordinates; without the flag nothing changes')
    p.add_argument('--save_lumen', default=None, metavar='PATH',
                   help='after training, write the lumen cross-sections along the final model\'s vessel centreline to PATH (.csv): the pruned '
                        'centreline of --save_centreline at --mesh_threshold, and at each of its points the area and the diameters of the '
                        'cross-section of the density grid at that level (afx_lumen_profile: 64 rays in the plane normal to the centreline, '
                        'crossings interpolated below the voxel), one row per point; without the flag nothing changes')
    p.add_argument('--save_branches', default=None, metavar='PATH',
                   help='after training, write one row per branch and junction of the final model\'s vessel centreline to PATH (.csv): the '
                        'pruned centreline of --save_centreline at --mesh_threshold, every vessel voxel given to the branch or junction it '
                        'lies nearest to (afx_feature_transform_3d, afx_label_overlap_3d): territory voxels and volume in world units, '
                        'length, mean, minimum and maximum radius, attached nodes; needs no ground truth; without the flag nothing changes')
    p.add_argument('--save_cpr', default=None, metavar='PATH',
                   help='after training, write the curved-planar reformation of the final model\'s vessel to PATH (.npy, float64 [A, P, K]): the '
                        'main path of the pruned centreline of --save_centreline at --mesh_threshold (from the widest free end to the farthest '
                        'one), smoothed and resampled at the grid step, and along it the longitudinal images of the density grid at the '
                        'in-plane angles --cpr_angles, K = 2 --cpr_half_width + 1 samples half a grid step apart (afx_reformat_planes on '
                        'rotation-minimising frames); without the flag nothing changes')
    p.add_argument('--cpr_angles', type=float, nargs='+', default=[0.0, 45.0, 90.0, 135.0], metavar='DEGREES',
                   help='--save_cpr: the in-plane angles of the longitudinal images')
    p.add_argument('--cpr_half_width', type=int, default=16, metavar='K', help='--save_cpr: samples on either side of the centreline')
    p.add_argument('--save_view_map', default=None, metavar='PATH',
                   help='after training, write the foreshortening and overlap map of the final model\'s vessel centreline to PATH (.csv): the '
                        'pruned centreline of --save_centreline at --mesh_threshold with its radii, scored over the evaluation sweep\'s angles '
                        '(--limited_size, --view_map_step) on the test view\'s detector (afx_view_map), one row per angle: theta, phi, '
                        'tree_foreshortening, tree_overlap, then foreshortening and overlap of every branch; the five best whole-tree views are '
                        'printed; without the flag nothing changes')
    p.add_argument('--view_map_step', type=float, default=5.0, metavar='DEGREES', help='--save_view_map: the step of the angle grid')
    p.add_argument('--save_poses', default=None, metavar='PATH',
                   help='after training, register the pose of every training view to its vessel silhouette and write the result to PATH '
                        '(.csv): the pruned centreline of --save_centreline at --mesh_threshold with its radii against the signed distance '
                        'images of the silhouettes (pixel_value < --hull_threshold), by Levenberg-Marquardt on the 2D-3D chamfer residual '
                        '(afx_pose_chamfer, afx_pose_lm_step); one row per view: the id, the given and the refined cam2world, the chamfer '
                        'before and after, the shift in pixels and the accepted steps.  Needs --binary True.  The refined poses are written, '
                        'not trained with; without the flag nothing changes')
    p.add_argument('--pose_dof', default='all', choices=['all', 'translation', 'rotation', 'inplane'],
                   help='--save_poses: the degrees of freedom that move (inplane: the rotation about the view axis and the two detector shifts)')
    p.add_argument('--pose_trunc', type=float, default=8.0, metavar='PIXELS',
                   help='--save_poses: the residual is truncated at PIXELS (a point further from the silhouette pulls no more)')
    p.add_argument('--pose_search', type=float, nargs=3, default=None, metavar=('DEGREES', 'UNITS', 'STEPS'),
                   help='--save_poses: before the refinement, score an in-plane grid of STEPS^3 poses (STEPS odd) within +-DEGREES about the '
                        'view axis and +-UNITS along the two detector axes, and start from the best')
    p.add_argument('--pose_noise', type=float, nargs=2, default=None, metavar=('DEG', 'UNITS'),
                   help='--synthetic: the images are rendered at the true poses, but the poses and rays handed to training are perturbed by a '
                        'seeded rigid increment of up to +-DEG about each camera axis and +-UNITS along each (make_synthetic_dataset '
                        'pose_noise); unshifted_tform_cam2world keeps the true poses')
    p.add_argument('--grid_init', default=None, choices=['hull'],
                   help='hull (--march grid or grid_ops, --binary True): before training, carve both occupancy grids with the visual hull of '
                        'the training views - a cell stays only where no training view\'s vessel silhouette (pixel_value < --hull_threshold) '
                        'rules it out and at least one view sees it (afx_visual_hull over the cell centres) - and keep that mask as the '
                        'ceiling of every later grid update (OccupancyGrid.carve).  On data with background the tissue outside the vessel '
                        'attenuates too, so the flag is refused there.  Without the flag nothing changes')
    p.add_argument('--hull_margin', type=float, default=1.0, metavar='PIXELS',
                   help='--grid_init hull: pixels added to every view\'s tolerance (1: a vessel point may project up to one pixel from the '
                        'nearest silhouette pixel centre)')
    p.add_argument('--hull_max_rejects', type=int, default=0, metavar='N', help='--grid_init hull: a cell stays when at most N views reject it')
    p.add_argument('--hull_threshold', type=float, default=1.0, metavar='T',
                   help='--grid_init hull: a training pixel belongs to the silhouette when pixel_value < T (1.0: any attenuation at all)')
    p.add_argument('--save_hull', default=None, metavar='PATH',
                   help='--grid_init hull: write the vote volumes to PATH (.npy): uint16 [2, 128, 128, 128], the views that see each cell and '
                        'the views that reject it')
    p.add_argument('--save_sirt', default=None, metavar='PATH',
                   help='after training, write the algebraic reconstruction (SIRT) of the attenuation volume from the training views to PATH '
                        '(.npy): float64 [128, 128, 128] on the cell centres of the occupancy grid\'s box (afx_xray_project, '
                        'afx_xray_backproject); needs --binary True or CT-type data (pixel values exp(-line integral)); with --grid_init '
                        'hull the hull is the support mask')
    p.add_argument('--sirt_iterations', type=int, default=50, metavar='N', help='--save_sirt: SIRT iterations (default 50)')
    p.add_argument('--sirt_relax', type=float, default=1.0, metavar='LAMBDA', help='--save_sirt: the relaxation factor (default 1.0)')
    p.add_argument('--sirt_tv_weight', type=float, default=0.0, metavar='W',
                   help='--save_sirt: SIRT-TV - after every SIRT update the volume is denoised by the proximal operator of the total variation '
                        'at the weight W (afx_tv_denoise_3d); 0 (the default): plain SIRT')
    p.add_argument('--sirt_tv_iterations', type=int, default=10, metavar='N',
                   help='--sirt_tv_weight: iterations of the denoising step after every SIRT update (default 10)')
    p.add_argument('--phantom_mesh', default=None, metavar='PATH',
                   help='--synthetic: the phantom is the vessel surface in PATH (.stl or .vtk) instead of the capsule tree: its signed distance '
                        'field on the GPU (afx_mesh_sdf_3d), passed through rev_sigmoid(., 2) and projected with type=\'sdf\' as the '
                        'reference\'s sdftoray.py does; the mesh is centred and scaled to fill the scene.  Without the flag nothing changes')
    p.add_argument('--phantom_points', type=int, default=201, metavar='N',
                   help='--phantom_mesh: grid points along the longest side of the mesh (default 201)')
    p.add_argument('--log_dir', default='runs/afx')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--out_bias_init', type=float, default=-5.0,
                   help='initial output bias. Dense marching has no nerfacc early termination: with the default '
                        'nn.Linear init sigma ~ 0.5 everywhere, the transmittance underflows to 0 and so does its '
                        'gradient; starting from near-empty space (sigmoid(-5) ~ 0.007) keeps training well-posed')
    return p


def check_args(args):
    """The flag combinations the driver refuses (before any device work)."""
    if args.single_eval and (args.march != 'grid' or args.precision != 'f16s8' or args.pos_enc != 'none'):
        raise ValueError("--single-eval: needs --march grid --precision f16s8 --pos_enc none (the single-evaluation grid step is f16s8, ReLU, "
                         "without an input encoding)")
    if args.graph_grid_update and not args.graph:
        raise ValueError("--graph-grid-update: needs --graph")
    if args.graph_rounds and not (args.graph and args.graph_grid_update):
        raise ValueError("--graph-rounds: needs --graph --graph-grid-update")
    if args.graph_rounds and args.host_sampler:
        raise ValueError("--graph-rounds: the batches are drawn inside the graph; --host_sampler draws them on the host")


    if args.entropy_weight < 0:
        raise ValueError("--entropy_weight: needs LAMBDA >= 0")
    if args.entropy_weight > 0 and (args.march != 'grid_ops' or args.graph or args.graph_grid_update or args.graph_rounds or args.single_eval):
        raise ValueError("--entropy_weight: needs --march grid_ops without the graph flags (the operator-sequence body, where the loss is built "
                         "under autograd; --march dense, --march grid and the graphs are fused MSE steps)")
    if args.checkpoint_every < 0:
        raise ValueError("--checkpoint_every: needs N >= 0")
    if getattr(args, 'grid_init', None) == 'hull':
        if args.binary != 'True':
            raise ValueError("--grid_init hull: needs --binary True (vessel-only data: on data with background the tissue outside the vessel "
                             "attenuates too, every pixel would belong to the silhouette, and carving by it would be wrong)")
        if args.march == 'dense':
            raise ValueError("--grid_init hull: needs --march grid or grid_ops (the dense march has no occupancy grid to carve)")
        if not (args.hull_margin >= 0 and np.isfinite(args.hull_margin)):
            raise ValueError("--hull_margin: needs PIXELS >= 0")
        if args.hull_max_rejects < 0:
            raise ValueError("--hull_max_rejects: needs N >= 0")
    if getattr(args, 'save_hull', None) is not None:
        if getattr(args, 'grid_init', None) != 'hull':
            raise ValueError("--save_hull: needs --grid_init hull")
        if os.path.splitext(args.save_hull)[1].lower() != '.npy':
            raise ValueError("--save_hull: PATH must end in .npy")
    if getattr(args, 'save_sirt', None) is not None:
        if args.binary != 'True' and (args.data_name or 'ct') != 'ct':
            raise ValueError("--save_sirt: needs --binary True or CT-type data (--data_name ct): the pixel values must be transmissions "
                             "exp(-line integral)")
        if os.path.splitext(args.save_sirt)[1].lower() != '.npy':
            raise ValueError("--save_sirt: PATH must end in .npy")
        if args.sirt_iterations < 1:
            raise ValueError("--sirt_iterations: needs N >= 1")
        if not (np.isfinite(args.sirt_relax) and 0 < args.sirt_relax < 2):
            raise ValueError("--sirt_relax: needs 0 < LAMBDA < 2")
    tv_weight = getattr(args, 'sirt_tv_weight', 0.0)
    if not (np.isfinite(tv_weight) and tv_weight >= 0):
        raise ValueError("--sirt_tv_weight: needs a finite W >= 0")
    if tv_weight > 0 and getattr(args, 'save_sirt', None) is None:
        raise ValueError("--sirt_tv_weight: needs --save_sirt")
    if getattr(args, 'sirt_tv_iterations', 10) < 0:
        raise ValueError("--sirt_tv_iterations: needs N >= 0")
    if args.phantom_mesh is not None:
        if not args.synthetic:
            raise ValueError("--phantom_mesh: needs --synthetic (the phantom replaces the capsule tree of the synthetic dataset)")
        if os.path.splitext(args.phantom_mesh)[1].lower() not in ('.stl', '.vtk'):
            raise ValueError("--phantom_mesh: PATH must end in .stl or .vtk")
        if args.phantom_points < 2:
            raise ValueError("--phantom_points: needs N >= 2")
    if args.save_mesh is not None:
        if os.path.splitext(args.save_mesh)[1].lower() not in ('.stl', '.vtk'):
            raise ValueError("--save_mesh: PATH must end in .stl or .vtk")
        if not args.mesh_threshold > 0:
            raise ValueError("--mesh_threshold: needs SIGMA > 0 (the surface is capped with zero density around the grid)")
    if args.save_centreline is not None:
        if os.path.splitext(args.save_centreline)[1].lower() != '.vtk':
            raise ValueError("--save_centreline: PATH must end in .vtk")
        if not args.mesh_threshold > 0:
            raise ValueError("--mesh_threshold: needs SIGMA > 0")
    if args.save_lumen is not None:
        if os.path.splitext(args.save_lumen)[1].lower() != '.csv':
            raise ValueError("--save_lumen: PATH must end in .csv")
        if not args.mesh_threshold > 0:
            raise ValueError("--mesh_threshold: needs SIGMA > 0")
    if getattr(args, 'save_branches', None) is not None:
        if os.path.splitext(args.save_branches)[1].lower() != '.csv':
            raise ValueError("--save_branches: PATH must end in .csv")
        if not args.mesh_threshold > 0:
            raise ValueError("--mesh_threshold: needs SIGMA > 0")
    if args.save_cpr is not None:
        if os.path.splitext(args.save_cpr)[1].lower() != '.npy':
            raise ValueError("--save_cpr: PATH must end in .npy")
        if not args.mesh_threshold > 0:
            raise ValueError("--mesh_threshold: needs SIGMA > 0")
        if not args.cpr_angles or not all(np.isfinite(a) for a in args.cpr_angles):
            raise ValueError("--cpr_angles: needs at least one finite angle")
        if not 0 <= args.cpr_half_width <= 511:
            raise ValueError("--cpr_half_width: needs K in 0..511")
    if args.save_view_map is not None:
        if os.path.splitext(args.save_view_map)[1].lower() != '.csv':
            raise ValueError("--save_view_map: PATH must end in .csv")
        if not args.mesh_threshold > 0:
            raise ValueError("--mesh_threshold: needs SIGMA > 0")
        if not (args.view_map_step > 0 and np.isfinite(args.view_map_step)):
            raise ValueError("--view_map_step: needs DEGREES > 0")
    if getattr(args, 'save_poses', None) is not None:
        if args.binary != 'True':
            raise ValueError("--save_poses: needs --binary True (vessel-only data: on data with background every pixel attenuates, and "
                             "there is no vessel silhouette to register a pose to)")
        if os.path.splitext(args.save_poses)[1].lower() != '.csv':
            raise ValueError("--save_poses: PATH must end in .csv")
        if not args.mesh_threshold > 0:
            raise ValueError("--mesh_threshold: needs SIGMA > 0")
        if not (args.pose_trunc > 0 and np.isfinite(args.pose_trunc)):
            raise ValueError("--pose_trunc: needs a finite PIXELS > 0")
        if args.pose_search is not None:
            deg, units, steps = args.pose_search
            if not (0 <= deg < 180 and units >= 0 and np.isfinite(units) and steps == int(steps) and steps >= 1 and int(steps) % 2 == 1):
                raise ValueError("--pose_search: needs 0 <= DEGREES < 180, UNITS >= 0 and an odd STEPS >= 1")
    elif getattr(args, 'pose_search', None) is not None:
        raise ValueError("--pose_search: needs --save_poses")
    if getattr(args, 'pose_noise', None) is not None:
        if not args.synthetic:
            raise ValueError("--pose_noise: needs --synthetic (the poses of the synthetic dataset are perturbed)")
        if not all(np.isfinite(x) and x >= 0 for x in args.pose_noise):
            raise ValueError("--pose_noise: needs DEG >= 0 and UNITS >= 0")


def checkpoint_interval(checkpoint_every: int, graph_rounds: bool, round_len: int = 16) -> int:
    """Iterations between two state files: --checkpoint_every, rounded up to whole rounds with --graph-rounds (0: none)."""
    n = int(checkpoint_every)
    return -(-n // round_len) * round_len if graph_rounds else n


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    if device.type != "cuda":
        raise SystemExit("run_nerf_acc: needs an MI355X; there is no CPU fallback")
    limited_size = float(args.limited_size) if args.limited_size is not None else 180.0
    number_angles = float(args.number_angles) if args.number_angles is not None else 4.0
    center_point = ast.literal_eval(args.center_point) if args.center_point is not None else [90, 0]
    binary = args.binary == 'True' if args.binary is not None else False
    sampling_strategy = args.sampling_strategy if args.sampling_strategy is not None else 'segmentation'
    data_name = args.data_name if args.data_name else 'ct'
    num_layers = int(args.num_layers) if args.num_layers else 4
    num_hidden_units = int(args.num_hidden_units) if args.num_hidden_units else 128
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)

    outside = 100
    file_name = f'limited-sparse-{limited_size}-{number_angles}-{center_point}' if binary else \
        f'background-{limited_size}-{number_angles}-{center_point}'
    if args.synthetic and args.phantom_mesh is not None:
        proj_df, ray_df = ds.make_synthetic_dataset(ds.angle_grid(limited_size, int(number_angles), center_point),
                                                    img_size=args.img_size, sampling_strategy=sampling_strategy,
                                                    device=device, seed=args.seed, binary=binary,
                                                    phantom=mesh_phantom(args.phantom_mesh, args.phantom_points, outside, device),
                                                    projection_type='sdf', pose_noise=args.pose_noise)
    elif args.synthetic:
        proj_df, ray_df = ds.make_synthetic_dataset(ds.angle_grid(limited_size, int(number_angles), center_point),
                                                    img_size=args.img_size, sampling_strategy=sampling_strategy,
                                                    device=device, seed=args.seed, binary=binary, pose_noise=args.pose_noise)
    else:
        step_size = limited_size / number_angles if number_angles > 0 else limited_size
        proj_df, ray_df, _, _ = ds.load_data(data_name, file_name, False, binary, args.img_size, step_size, args.data_root)

    # held-out projection = last one (run_nerf_acc.py:85-99); [W,H] image indexing as upstream
    test_proj_id = proj_df.index[-1]
    test_ray_df = ray_df[ray_df['image_id'] == test_proj_id].copy()
    # (np.ascontiguousarray: a frame's multi-column to_numpy() is column-major, and .float().to(device) would keep those strides)
    cols = lambda df, stem: torch.from_numpy(np.ascontiguousarray(df[[f'{stem}_x', f'{stem}_y', f'{stem}_z']].to_numpy(), dtype=np.float32)).to(device)
    test_origins, test_directions = cols(test_ray_df, 'ray_origins'), cols(test_ray_df, 'ray_directions')
    test_x = torch.from_numpy(test_ray_df['x_position'].to_numpy().astype('int64')).to(device)
    test_y = torch.from_numpy(test_ray_df['y_position'].to_numpy().astype('int64')).to(device)
    img_width, img_height = int(test_x.max()) + 1, int(test_y.max()) + 1
    test_img = torch.zeros((img_width, img_height), device=device)
    test_img[test_x, test_y] = torch.from_numpy(test_ray_df['pixel_value'].to_numpy()).to(device).float()
    vessel = torch.from_numpy((test_ray_df['distance_pixel_value'] > test_ray_df['distance_pixel_value'].mean()).to_numpy()).to(device)

    train_ray_df = ray_df[ray_df['image_id'] != test_proj_id].copy()
    train_ray_df['ray_origins'] = train_ray_df[['ray_origins_x', 'ray_origins_y', 'ray_origins_z']].to_numpy().tolist()
    train_ray_df['ray_directions'] = train_ray_df[['ray_directions_x', 'ray_directions_y', 'ray_directions_z']].to_numpy().tolist()

    src_pt_z = float(proj_df['src_pt_z'].iloc[0])
    depth_samples_per_ray_coarse = args.depth_samples
    near_thresh, far_thresh = src_pt_z - outside, src_pt_z + outside

    n_iters, early_stop_iters = args.n_iters, 50000
    display_every, save_every = args.display_every, args.display_every * 100
    coarse_lr, decay_rate, decay_steps = 1e-4, 0.1, 500 * 1000
    img_sample_size = args.sample_size ** 2
    start_pos_enc_basis, pos_enc_basis, fourier_sigma = 0, 5, 5
    barf_start, barf_stop = args.barf_start, args.barf_stop
    barf_step_size = pos_enc_basis / (barf_stop - barf_start)
    params = {'num_early_layers': num_layers, 'num_late_layers': 0, 'num_filters': num_hidden_units,
              'num_input_channels': 3, 'num_output_channels': 1, 'num_input_channels_views': 0, 'use_bias': True,
              'pos_enc': args.pos_enc, 'pos_enc_basis': pos_enc_basis, 'act_func': 'relu', 'fourier_sigma': fourier_sigma,
              'num_img': 1, 'device': device, 'precision': args.precision}
    coarse_model = CPPN(dict(params)).to(device)
    if coarse_model.use_pos_enc == 'barf':
        coarse_model.update_barf_alpha(start_pos_enc_basis, 'pts')
    if coarse_model.use_pos_enc == 'fourier' and args.precision == 'f32':
        coarse_model.fourier_coefficients.requires_grad_(False)     # the f32 kernels take them as constants; the 16-bit ones train them
    with torch.no_grad():
        coarse_model.output_linear[0].bias.fill_(args.out_bias_init)
    # run_nerf_acc.py:206.  fused=True: PyTorch's single multi-tensor Adam kernel instead of its foreach sequence of ~7 launches - same
    # update, and on the reference's 1.3 ms iteration the difference is 10 % (host-side dispatch: 0.95 -> 0.55 ms with the grid march)
    if args.graph and (args.march != 'grid' or args.precision != 'f16s8' or args.adam != 'fused' or args.pos_enc != 'none'):
        raise ValueError("--graph: needs --march grid --precision f16s8 --adam fused --pos_enc none (the capturable grid step is f16s8; "
                         "the captured optimizer is the fused, capturable Adam; the encodings' schedules and coefficients are not captured)")
    # --graph: a device-resident lr (changed with fill_ between replays) and an Adam whose step can be captured
    coarse_optimizer = torch.optim.Adam(list(coarse_model.parameters()), lr=torch.tensor(coarse_lr, device=device) if args.graph else coarse_lr,
                                        fused=(args.adam == 'fused'), capturable=args.graph)

    # device-resident ray table (R13): built once; every batch is drawn and gathered on the GPU
    tab_o, tab_d = cols(train_ray_df, 'ray_origins'), cols(train_ray_df, 'ray_directions')
    tab_pix = torch.from_numpy(train_ray_df['pixel_value'].to_numpy()).float().to(device)
    tab_w = torch.from_numpy(train_ray_df['distance_pixel_value'].to_numpy()).float().to(device)

    # occupancy grid of the reference loop (run_nerf_acc.py:196-198); thresholds :68-70
    early_stop_eps, alpha_thre, vessel_alpha_thre = 1e-2, 1e-4, 5e-2
    scene_aabb = torch.tensor([-outside, -outside, -outside, outside, outside, outside], dtype=torch.float32, device=device)
    acc_grid = OccupancyGrid(roi_aabb=scene_aabb, resolution=128, contraction_type=ContractionType.AABB, seed=args.seed).to(device) \
        if args.march != 'dense' else None
    # the reference's second grid (:198,286): same updates at the vessel threshold; it only feeds the exported occupancy volumes (:362-367)
    vessel_acc_grid = OccupancyGrid(roi_aabb=scene_aabb, resolution=128, contraction_type=ContractionType.AABB, seed=args.seed + 1).to(device) \
        if args.march != 'dense' else None
    packed_step = args.march == 'grid' and args.precision == 'f16s8'      # else the operator sequence
    batch_size = 131072
    hull_info = None
    if args.grid_init == 'hull':      # before any graph is captured over the grids: a carved grid ends every update with the mask's launch
        hull_info = carve_grids_with_hull([acc_grid, vessel_acc_grid], proj_df, train_ray_df, test_proj_id, args.hull_threshold,
                                          args.hull_margin, args.hull_max_rejects, device, save_path=args.save_hull, log_dir=args.log_dir)

    os.makedirs(args.log_dir, exist_ok=True)
    log = open(os.path.join(args.log_dir, 'train_log.jsonl'), 'a')
    highest_psnr, highest_iter, history = 0.0, 0, []
    if not args.host_sampler and not args.graph_rounds:      # the batches of 16 iterations per launch sequence
        ray_batches = _engine.RayBatchSampler(tab_o, tab_d, tab_pix, tab_w, img_sample_size, seed=args.seed, prefetch=16)
    new_lr_coarse = coarse_lr
    loss_coarse = torch.tensor(float('nan'), device=device)
    n_marched = 0
    entropy_mean = torch.tensor(float('nan'), device=device)      # (--entropy_weight: until the first iteration whose march keeps samples)
    train_graph = None
    round_graph = None
    if args.graph_rounds:      # whole refresh periods per graph launch: draw, refreshes, 16 iterations and their bookkeeping on the device
        if acc_grid is None:
            raise ValueError("--graph-rounds: needs --march grid")      # (--graph has checked the rest)
        round_graph = GridTrainRoundGraph(coarse_model, coarse_optimizer, [(acc_grid, alpha_thre), (vessel_acc_grid, vessel_alpha_thre)],
                                          (tab_o, tab_d, tab_pix, tab_w), scene_aabb, img_sample_size, depth_samples_per_ray_coarse, near_thresh,
                                          far_thresh, early_stop_eps, alpha_thre, seed=args.seed,
                                          lr_table=lr_decay_table(coarse_lr, decay_rate, decay_steps, n_iters + 1), single_eval=args.single_eval)
    elif args.graph:      # captured once; every iteration then copies its batch into the graph's static tensors and replays
        train_graph = GridTrainGraph(coarse_model, coarse_optimizer, acc_grid, scene_aabb, img_sample_size, depth_samples_per_ray_coarse, near_thresh,
                                     far_thresh, early_stop_eps, alpha_thre, single_eval=args.single_eval)
        n_marched = torch.zeros((), dtype=torch.int64, device=device)
    update_graph = None
    if args.graph_grid_update and round_graph is None:      # both grids' refresh (:285-286) in graphs captured on first use; replayed before the training step
        update_graph = GridUpdateGraph(coarse_model, [(acc_grid, alpha_thre), (vessel_acc_grid, vessel_alpha_thre)])
    # training state (--checkpoint_every / --resume, nerf/checkpoint.py).  Everything above is built as in a fresh run, graphs captured
    # included; a restored state is then copied INTO the live tensors
    start_iter, state_file, last_state = 0, os.path.join(args.log_dir, _ckpt.STATE_FILE), None
    ckpt_every = checkpoint_interval(args.checkpoint_every, args.graph_rounds)
    if ckpt_every or args.resume:
        fingerprint = _ckpt.config_fingerprint(args, params, (tab_o, tab_d, tab_pix, tab_w))
        live = dict(model=coarse_model, optimizer=coarse_optimizer, grids=[g for g in (acc_grid, vessel_acc_grid) if g is not None],
                    graphs={k: g for k, g in (('train', train_graph), ('update', update_graph), ('round', round_graph)) if g is not None})
        if ckpt_every != args.checkpoint_every:
            print(f'--checkpoint_every {args.checkpoint_every}: rounded up to {ckpt_every} (whole rounds of --graph-rounds)')
    if args.resume:
        state = _ckpt.load_training_state(args.resume, fingerprint=fingerprint, **live)
        start_iter, history, kept = state['n_iter'], list(state['history']), state['counters']
        highest_psnr, highest_iter, new_lr_coarse = kept['highest_psnr'], kept['highest_iter'], kept['lr']
        if round_graph is None:      # (--graph-rounds keeps both on the device: restored with the round graph)
            loss_coarse = kept['loss'].to(device)
            n_marched = kept['n_marched'] if train_graph is None else n_marched.fill_(kept['n_marched'])
        last_state = _ckpt.state_path(args.resume)
        print(f'resumed from {last_state} at iteration {start_iter}')

    def write_state(next_iter):
        """trainstate.pt after iteration next_iter - 1, unless the loss or a parameter is not finite (the file then stays the last good one)."""
        loss_now = (round_graph.last_loss if round_graph is not None else loss_coarse).detach()
        if not (bool(torch.isfinite(loss_now)) and bool(torch.isfinite(coarse_model.flat_params).all())):
            print(f'iteration {next_iter - 1}: non-finite loss or parameters, no state written')
            return last_state
        return _ckpt.save_training_state(state_file, fingerprint=fingerprint, n_iter=next_iter, history=history,
                                         counters=dict(highest_psnr=highest_psnr, highest_iter=highest_iter, lr=new_lr_coarse,
                                                       loss=loss_now.float(), n_marched=int(n_marched)), **live)

    t_last = time.time()
    # --graph-rounds: the loop visits the display points (and the last iteration) only; run() replays every iteration up to each of them
    # (and up to the last iteration of every round after which a state is written)
    stops = range(start_iter, n_iters + 1) if round_graph is None else \
        [s for s in sorted(set(range(0, n_iters + 1, display_every)) | {n_iters} |
                           (set(range(ckpt_every - 1, n_iters + 1, ckpt_every)) if ckpt_every else set())) if s >= start_iter]
    for n_iter in stops:
        coarse_model.train()
        if round_graph is not None:
            round_graph.run(n_iter + 1 - round_graph.iter)      # iterations round_graph.iter .. n_iter; nothing is read back
            loss_coarse, n_marched = round_graph.last_loss, round_graph.n_marched      # (device tensors, read at the display point below)
            new_lr_coarse = coarse_lr * (decay_rate ** (n_iter / decay_steps))
        else:
            if coarse_model.use_pos_enc == 'barf' and barf_start <= n_iter < barf_stop:
                coarse_model.update_barf_alpha(coarse_model.barf_alpha + barf_step_size, 'pts')
            if args.host_sampler:
                batch_origins, batch_directions, batch_pix_vals = sample_pixel_rays(train_ray_df, img_sample_size, device,
                                                                                   weights='distance_pixel_value')
            else:
                batch_origins, batch_directions, batch_pix_vals, _ = ray_batches.draw(n_iter)      # == sample_rays(..., seed, stream_id=n_iter)
            if train_graph is None:
                coarse_optimizer.zero_grad()      # (--graph: the captured step zeroes the gradient buffer it accumulates into)
            if args.march != 'dense':
                # the reference's iteration body, run_nerf_acc.py:284-306
                with torch.no_grad():
                    acc_grid.train()
                    vessel_acc_grid.train()
                    if update_graph is not None:
                        update_graph.step(n_iter)
                    else:
                        acc_grid = acc_update_n_step(acc_grid, coarse_model, n_iter, occ_thre=alpha_thre)
                        vessel_acc_grid = acc_update_n_step(vessel_acc_grid, coarse_model, n_iter, occ_thre=vessel_alpha_thre)
                if train_graph is not None:
                    # the same iteration replayed from the graph: no host read-back; an empty march skips the Adam step on the device
                    loss_k, pred, counts = train_graph.step(batch_origins, batch_directions, batch_pix_vals)
                    loss_coarse = torch.where(train_graph.skip[0] > 0, loss_coarse, loss_k)      # (the last step that kept samples, as below)
                    n_marched += counts[1]
                    ray_indices = ()      # (the optimizer step is part of the graph)
                elif packed_step:
                    # :287-306 - march, alpha pass, visibility and the fused packed step - as ONE library call (the entry points of the
                    # operator branch below, in the same order: ~30 launches that a Python loop issues slower than the GPU runs them)
                    loss_k, pred_k, n_kept = march_train_step_mse(coarse_model, acc_grid, scene_aabb, batch_origins, batch_directions,
                                                                  depth_samples_per_ray_coarse, near_thresh, far_thresh, early_stop_eps,
                                                                  alpha_thre, batch_pix_vals, single_eval=args.single_eval)
                    ray_indices = range(n_kept)      # (only its length is used below: the reference steps when the march kept samples)
                    if n_kept:
                        loss_coarse, pred = loss_k, pred_k
                        n_marched += n_kept
                else:
                    with torch.no_grad():
                        ray_indices, t_starts, t_ends = acc_ray_marching(coarse_model, acc_grid, scene_aabb, batch_origins, batch_directions,
                                                                         depth_samples_per_ray_coarse, near_thresh, far_thresh, early_stop_eps,
                                                                         alpha_thre)
                    if len(ray_indices) > 0:
                        positions = batch_origins[ray_indices.long()] + batch_directions[ray_indices.long()] * (t_starts + t_ends) / 2.0
                        predictions = get_predictions(coarse_model, positions, batch_size)
                        pred, _ = acc_render_volume_density(predictions, ray_indices, t_starts, t_ends, img_sample_size,
                                                            depth_samples_per_ray_coarse)
                        loss_coarse = torch.nn.functional.mse_loss(pred, batch_pix_vals)
                        if args.entropy_weight > 0:      # mse + lambda * mean entropy of the batch's rays (rays the march left empty count as 0)
                            entropy_mean = acc_ray_entropy(predictions, ray_indices, pred, img_sample_size).mean()
                            loss_coarse = loss_coarse + args.entropy_weight * entropy_mean
                        loss_coarse.backward()
                        n_marched += int(len(ray_indices))
            elif args.precision == 'f32':
                pred = render_rays(coarse_model, batch_origins, batch_directions, depth_samples_per_ray_coarse, near_thresh,
                                   far_thresh, mode='acc').rgb_map
                loss_coarse = torch.nn.functional.mse_loss(pred, batch_pix_vals)
                loss_coarse.backward()
            else:
                loss_coarse, pred = train_step_mse(coarse_model, RenderSpec(
                    n_rays=img_sample_size, n_samples=depth_samples_per_ray_coarse, origins=batch_origins,
                    dirs=batch_directions, mode='acc', t_near=near_thresh, t_far=far_thresh), batch_pix_vals)
            if args.march == 'dense' or len(ray_indices) > 0:      # (the reference steps only when the march kept samples, :293)
                coarse_optimizer.step()
            new_lr_coarse = coarse_lr * (decay_rate ** (n_iter / decay_steps))
            for param_group in coarse_optimizer.param_groups:
                if train_graph is not None:
                    param_group['lr'].fill_(new_lr_coarse)
                else:
                    param_group['lr'] = new_lr_coarse

        if n_iter % display_every == 0:
            coarse_model.eval()
            keep, coarse_model.precision = coarse_model.precision, args.eval_precision
            eval_counts = None
            with torch.no_grad():
                if args.march == 'grid':           # run_nerf_acc.py:338-349 with ONE evaluation of the model: the alpha pass's raw output is
                    # the one compositing uses - the operator sequence below (the `grid_ops` body) bit for bit
                    test_pred, eval_counts = march_render(coarse_model, acc_grid, scene_aabb, test_origins, test_directions,
                                                          depth_samples_per_ray_coarse, near_thresh, far_thresh, early_stop_eps, alpha_thre)
                elif args.march != 'dense':        # run_nerf_acc.py:338-349
                    ri_t, ts_t, te_t = acc_ray_marching(coarse_model, acc_grid, scene_aabb, test_origins, test_directions,
                                                        depth_samples_per_ray_coarse, near_thresh, far_thresh, early_stop_eps, alpha_thre)
                    pos_t = test_origins[ri_t.long()] + test_directions[ri_t.long()] * (ts_t + te_t) / 2.0
                    test_pred, _ = acc_render_volume_density(get_predictions(coarse_model, pos_t, batch_size) if len(ri_t) else pos_t[:, :1],
                                                             ri_t, ts_t, te_t, test_origins.shape[0], depth_samples_per_ray_coarse)
                else:
                    test_pred = render_rays(coarse_model, test_origins, test_directions, depth_samples_per_ray_coarse,
                                            near_thresh, far_thresh, mode='acc').rgb_map
            coarse_model.precision = keep
            pred_img = torch.zeros_like(test_img)
            pred_img[test_x, test_y] = test_pred
            mse = torch.nn.functional.mse_loss(pred_img, test_img)
            psnr = float(-10. * torch.log10(mse))
            vessel_psnr = float(-10. * torch.log10(torch.nn.functional.mse_loss(test_pred[vessel], test_img[test_x, test_y][vessel])))
            rec = dict(iter=n_iter, train_loss=float(loss_coarse.detach()), train_psnr=float(-10. * torch.log10(loss_coarse.detach())),
                       test_psnr=psnr, test_vessel_psnr=vessel_psnr, lr=new_lr_coarse,
                       barf_alpha=float(getattr(coarse_model, 'barf_alpha', 0.0)), sec=round(time.time() - t_last, 3),
                       it_per_s=round(display_every / max(time.time() - t_last, 1e-9), 1) if n_iter else 0.0,
                       marched_samples_per_iter=(int(n_marched) // max(display_every, 1)) if args.march != 'dense' else
                       img_sample_size * depth_samples_per_ray_coarse)
            if args.entropy_weight > 0:      # the last training batch's mean ray entropy (train_loss includes lambda times it)
                rec['entropy'] = float(entropy_mean.detach())
            if hull_info is not None:      # --grid_init hull: the hull's share of the grid and the fewest views that see a kept cell
                rec['hull'] = dict(share=hull_info['share'], min_seen=hull_info['min_seen'], n_views=hull_info['n_views'])
            if eval_counts is not None:      # candidates : kept samples of the test-view march
                rec['eval_candidates_per_kept'] = eval_counts[0] / eval_counts[1] if eval_counts[1] else None
            n_marched = 0 if train_graph is None and round_graph is None else n_marched.zero_()
            t_last = time.time()
            history.append(rec)
            log.write(json.dumps(rec) + "\n")
            log.flush()
            print(rec, flush=True)
            if not np.isfinite(rec['train_loss']):
                if last_state is not None:      # the last finite state, under its own name: resume it by hand, e.g. at another precision
                    import shutil
                    shutil.copyfile(last_state, os.path.join(args.log_dir, _ckpt.NONFINITE_FILE))
                    print('kept', os.path.join(args.log_dir, _ckpt.NONFINITE_FILE))
                raise FloatingPointError(
                    f"non-finite training loss at iteration {n_iter} (precision {args.precision}): the f16 precisions hold hidden "
                    "activations up to 65504 (include/afx.h); re-run with --precision bf16 (fp32 exponent range) or bf16x3")
            if psnr > highest_psnr:
                highest_psnr, highest_iter = psnr, n_iter
                coarse_model.save(os.path.join(args.log_dir, 'coarsemodel.pth'),
                                  {'epochs': n_iter, 'psnr': psnr, 'vessel_psnr': vessel_psnr})
                if acc_grid is not None:      # the occupancy volumes the reference writes as VTK next to the best model (:362-367,384-385)
                    np.save(os.path.join(args.log_dir, 'acc_grid_binary.npy'), acc_grid.binary.cpu().numpy())
                    np.save(os.path.join(args.log_dir, 'vessel_acc_grid_binary.npy'), vessel_acc_grid.binary.cpu().numpy())
            if n_iter % save_every == 0 and n_iter > 0:
                coarse_model.save(os.path.join(args.log_dir, f'coarsemodel-{n_iter}.pth'), {'epochs': n_iter})
            if n_iter - highest_iter > early_stop_iters:
                print('early stopping at', n_iter)
                break
        if ckpt_every and (n_iter + 1) % ckpt_every == 0:
            last_state = write_state(n_iter + 1)
    log.close()
    result = dict(history=history, best_psnr=highest_psnr, best_iter=highest_iter, model=coarse_model,
                  optimizer=coarse_optimizer, test_image=test_img, log_dir=args.log_dir, acc_grid=acc_grid,
                  vessel_acc_grid=vessel_acc_grid)
    if hull_info is not None:
        result['hull_info'] = hull_info
    exports = (('mesh_info', save_mesh, args.save_mesh), ('centreline_info', save_centreline, args.save_centreline),
               ('lumen_info', save_lumen, args.save_lumen), ('branches_info', save_branches, args.save_branches))
    exports = [e for e in exports if e[2] is not None]
    if exports or args.save_view_map is not None or args.save_cpr is not None or args.save_poses is not None:      # the density grid the exports read, evaluated once
        from ..render import density_grid
        grid = density_grid(coarse_model, outside, depth_samples_per_ray_coarse)
    for key, save, path in exports:
        result[key] = save(coarse_model, outside, depth_samples_per_ray_coarse + 1, args.mesh_threshold, path, grid=grid)
    if args.save_view_map is not None:
        from ..visualization.sweep import sweep_angles
        result['view_map_info'] = save_view_map(coarse_model, outside, depth_samples_per_ray_coarse + 1, args.mesh_threshold, args.save_view_map,
                                                sweep_angles(limited_size, args.view_map_step), img_width, img_height,
                                                float(proj_df['focal_length'].iloc[0]), (0.0, 0.0, src_pt_z), grid=grid)
    if args.save_poses is not None:
        result['pose_info'] = save_poses(coarse_model, outside, depth_samples_per_ray_coarse + 1, args.mesh_threshold, args.save_poses, proj_df,
                                         train_ray_df, test_proj_id, args.hull_threshold, device, dof=args.pose_dof, trunc=args.pose_trunc,
                                         search=args.pose_search, grid=grid)
    if args.save_cpr is not None:
        result['cpr_info'] = save_cpr(coarse_model, outside, depth_samples_per_ray_coarse + 1, args.mesh_threshold, args.save_cpr, args.cpr_angles,
                                      args.cpr_half_width, grid=grid)
    if args.save_sirt is not None:
        mask = acc_grid._carve_u8 if acc_grid is not None and args.grid_init == 'hull' else None      # the hull the grids were carved with
        result['sirt_info'] = save_sirt(proj_df, train_ray_df, test_proj_id, [-outside] * 3 + [outside] * 3, 128, near_thresh, far_thresh,
                                        depth_samples_per_ray_coarse, args.sirt_iterations, args.sirt_relax, device, args.save_sirt, mask=mask,
                                        tv_weight=args.sirt_tv_weight if args.sirt_tv_weight > 0 else None, tv_iterations=args.sirt_tv_iterations)
    return result


def training_view_images(proj_df, train_ray_df, test_proj_id, device):
    """The training views' images from the training rays alone, as `training_view_masks` gathers their silhouettes: pixel (y_position,
    x_position) of view image_id holds pixel_value; a pixel no ray covers holds 1 (no attenuation) -> (poses float64 [V, 4, 4], images
    float64 [V, H, W] on `device`, focal float64 [V]), the views in the order of proj_df."""
    ids = [i for i in proj_df.index if i != test_proj_id]
    if not ids:
        raise ValueError("--save_sirt: there is no training view")
    w, h = int(proj_df['org_img_width'].iloc[0]), int(proj_df['org_img_height'].iloc[0])
    slot = {image_id: v for v, image_id in enumerate(ids)}
    image = train_ray_df['image_id'].map(slot)
    if image.isna().any():
        raise ValueError("--save_sirt: a training ray belongs to no training view of the projection frame")
    images = torch.ones((len(ids), h, w), dtype=torch.float64)
    images[torch.from_numpy(image.to_numpy().astype('int64')), torch.from_numpy(train_ray_df['y_position'].to_numpy().astype('int64')),
           torch.from_numpy(train_ray_df['x_position'].to_numpy().astype('int64'))] = torch.from_numpy(
               train_ray_df['pixel_value'].to_numpy().astype('float64'))
    poses = np.asarray([proj_df.loc[i, 'tform_cam2world'] for i in ids], dtype=np.float64)
    focal = np.asarray([proj_df.loc[i, 'focal_length'] for i in ids], dtype=np.float64)
    return poses, images.to(device), focal


def save_sirt(proj_df, train_ray_df, test_proj_id, roi_aabb, resolution, near, far, n_samples, iterations, relax, device, path, mask=None,
              tv_weight=None, tv_iterations=10):
    """--save_sirt: the SIRT reconstruction of the attenuation volume from the training views (`engine.sirt_reconstruct`, from zero,
    clamped at zero) on the cell centres of the resolution^3 grid over `roi_aabb`, the line integrals -log(pixel_value) sampled as the
    training rays are (n_samples between near and far); mask: a support constraint of that shape (the hull the grids were carved with)
    -> its info (shape, iterations, relax, masked, n_views, the first and last residual norm, the volume's maximum and sum, path).
    tv_weight (--sirt_tv_weight; None: plain SIRT): SIRT-TV, `engine.tv_denoise_3d` at tv_weight and tv_iterations after every update;
    the info gains tv_weight, tv_iterations and total_variation (`engine.total_variation_3d` of the volume)."""
    poses, images, focal = training_view_images(proj_df, train_ray_df, test_proj_id, device)
    views = _engine.xray_views(poses, focal, images.shape[2], images.shape[1], near, far, n_samples, device=device)
    shape = (int(resolution),) * 3
    a12, _ = _engine.grid_cell_lattice(roi_aabb, shape)
    tv = {} if tv_weight is None else dict(tv_weight=float(tv_weight), tv_iterations=int(tv_iterations))
    x, history = _engine.sirt_reconstruct(views, _engine.line_integrals(images), shape, a12, iterations=iterations, relax=relax,
                                          mask=None if mask is None else mask.reshape(shape), return_history=True, **tv)
    np.save(path, x.cpu().numpy())
    info = dict(shape=shape, iterations=int(iterations), relax=float(relax), masked=mask is not None, n_views=int(views['n_views']),
                residual_first=float(history[0]), residual_last=float(history[-1]), max=float(x.max()), sum=float(x.sum()), path=str(path))
    if tv:
        info.update(tv, total_variation=float(_engine.total_variation_3d(x)))
    print('sirt', {k: info[k] for k in ('iterations', 'masked', 'n_views', 'residual_first', 'residual_last', 'max', 'path') + tuple(tv)}, flush=True)
    return info


def training_view_masks(proj_df, train_ray_df, test_proj_id, threshold, device):
    """The vessel silhouettes of the training views from the training rays alone: pixel (y_position, x_position) of view image_id belongs
    to the silhouette when pixel_value < threshold; the held-out view is left out -> (poses float64 [V, 4, 4], masks bool [V, H, W] on
    `device`, focal float64 [V]), the views in the order of proj_df."""
    ids = [i for i in proj_df.index if i != test_proj_id]
    if not ids:
        raise ValueError("--grid_init hull: there is no training view")
    w, h = int(proj_df['org_img_width'].iloc[0]), int(proj_df['org_img_height'].iloc[0])
    slot = {image_id: v for v, image_id in enumerate(ids)}
    image = train_ray_df['image_id'].map(slot)
    if image.isna().any():
        raise ValueError("--grid_init hull: a training ray belongs to no training view of the projection frame")
    inside = torch.from_numpy((train_ray_df['pixel_value'].to_numpy() < float(threshold)))
    masks = torch.zeros((len(ids), h, w), dtype=torch.bool)
    masks[torch.from_numpy(image.to_numpy().astype('int64')), torch.from_numpy(train_ray_df['y_position'].to_numpy().astype('int64')),
          torch.from_numpy(train_ray_df['x_position'].to_numpy().astype('int64'))] = inside
    poses = np.asarray([proj_df.loc[i, 'tform_cam2world'] for i in ids], dtype=np.float64)
    focal = np.asarray([proj_df.loc[i, 'focal_length'] for i in ids], dtype=np.float64)
    return poses, masks.to(device), focal


def carve_grids_with_hull(grids, proj_df, train_ray_df, test_proj_id, threshold, margin, max_rejects, device, save_path=None, log_dir=None):
    """--grid_init hull: the visual hull of the training views over the cell centres of each grid (the grids share their box: computed
    once per distinct shape), installed as the grids' persistent mask -> its info (share of the grid, fewest views that see a kept cell,
    views, margin); LOG_DIR/hull.npy keeps the hull as the grid masks are kept, --save_hull the two vote volumes."""
    poses, masks, focal = training_view_masks(proj_df, train_ray_df, test_proj_id, threshold, device)
    views = _engine.visual_hull_views(poses, masks, focal, margin_px=margin)
    hull, seen, rejects = grids[0].carve_from_views(views, max_rejects=max_rejects, min_seen=1, return_counts=True)
    for g in grids[1:]:
        if g._res_host == grids[0]._res_host and g._aabb_host == grids[0]._aabb_host:
            g.carve(hull)
        else:
            g.carve_from_views(views, max_rejects=max_rejects, min_seen=1)
    n_kept = int(hull.sum())
    info = dict(share=n_kept / hull.numel(), cells=n_kept, n_views=int(views['n_views']), margin=float(margin), max_rejects=int(max_rejects),
                min_seen=int(seen.to(torch.int32)[hull].min()) if n_kept else 0)
    if log_dir is not None:
        os.makedirs(log_dir, exist_ok=True)
        np.save(os.path.join(log_dir, 'hull.npy'), hull.cpu().numpy())
    if save_path is not None:
        np.save(save_path, np.stack([seen.cpu().numpy(), rejects.cpu().numpy()]))
        info['path'] = str(save_path)
    print('hull', {k: info[k] for k in ('share', 'cells', 'n_views', 'min_seen', 'margin')}, flush=True)
    return info


def mesh_phantom(path, n, outside, device):
    """--phantom_mesh: the mesh in `path` as a VoxelVolume - centred, scaled so that its longest side takes three quarters of the scene
    [-outside, outside]^3, its signed distance field on n points along that side passed through rev_sigmoid(., 2)."""
    from ..phantomdata.helpers import voxel_volume_from_mesh
    from ..visualization.mesh_io import read_mesh
    vertices, triangles = read_mesh(path)
    if len(triangles) == 0:
        raise ValueError(f"--phantom_mesh: {path} holds no triangle")
    longest = float((vertices.max(axis=0).astype(np.float64) - vertices.min(axis=0)).max())
    if not longest > 0:
        raise ValueError(f"--phantom_mesh: {path}: the mesh is a single point")
    return voxel_volume_from_mesh(vertices, triangles, n=n, margin=0.1, vol_scale=1.5 * float(outside) / longest, device=device)


def _export_grid(model, outside, n, grid):
    """The density grid the --save_* exports read (n points per axis over [-outside, outside]^3): `grid` when the caller has evaluated it."""
    from ..render import density_grid
    return density_grid(model, outside, int(n) - 1) if grid is None else grid


def _export_tree(grid, outside, n, threshold, prune_factor):
    """The pruned centreline of {grid >= threshold}, the level rounded to fp32 as the grid is -> (`sweep.centreline_tree`'s result, the
    grid's index_to_world)."""
    from ..visualization.sweep import centreline_tree, grid_index_to_world
    a = grid_index_to_world(outside, n)
    return centreline_tree(grid >= torch.tensor(float(threshold), dtype=torch.float32, device=grid.device), a, prune_factor), a


def save_mesh(model, outside, n, threshold, path, grid=None):
    """--save_mesh: the surface {sigma = threshold} of the model's density grid (n points per axis over [-outside, outside]^3), capped, in
    world coordinates, written by the file name's extension -> its info (V, T, E, B, euler, area, volume, threshold, path).  grid: that
    density grid, when it has been evaluated already."""
    from ..visualization.mesh_io import write_mesh
    from ..visualization.sweep import _grid_mesh
    vertices, triangles, info = _grid_mesh(_export_grid(model, outside, n, grid), float(threshold), outside, n)
    info.update(threshold=float(threshold), path=write_mesh(path, vertices, triangles))
    print('mesh', {k: info[k] for k in ('V', 'T', 'euler', 'area', 'volume', 'path')}, flush=True)
    return info


def save_centreline(model, outside, n, threshold, path, prune_factor=1.0, grid=None):
    """--save_centreline: the pruned centreline of {sigma >= threshold} on the model's density grid (n points per axis over [-outside,
    outside]^3), one polyline per branch in world coordinates with the radius per point -> its info (branches, nodes, free ends, spurs
    removed, length, threshold, path).  An empty mask writes a file without lines.  grid: as in `save_mesh`."""
    from ..visualization.mesh_io import write_vtk_polylines
    from ..visualization.sweep import centreline_polylines
    tree, a = _export_tree(_export_grid(model, outside, n, grid), outside, n, threshold, prune_factor)
    graph = tree['graph']
    points, offsets, radius = centreline_polylines(graph, tree['d2'], a, 2.0 * float(outside) / (int(n) - 1))
    info = dict(n_branches=graph['n_branches'], n_nodes=graph['n_nodes'], n_free_ends=graph['n_free_ends'],
                n_spurs_removed=tree['prune_record']['branches'], length=graph['total_length'], threshold=float(threshold),
                path=write_vtk_polylines(path, points, offsets, {'radius': radius}))
    print('centreline', info, flush=True)
    return info


LUMEN_CSV_COLUMNS = ('branch', 'index', 'x', 'y', 'z', 'arc_length', 'area', 'd_min', 'd_max', 'r_mean', 'flags')


def save_lumen(model, outside, n, threshold, path, prune_factor=1.0, grid=None):
    """--save_lumen: the cross-sections of the model's density grid (n points per axis over [-outside, outside]^3) at the level `threshold`
    along the pruned centreline of {sigma >= threshold} (that of --save_centreline), one CSV row per centreline point (LUMEN_CSV_COLUMNS;
    index = the point's position within its branch, lengths in world units, numbers written with repr) -> its info (path, n_points,
    n_valid, max_area_stenosis and its branch - NaN and -1 without a branch of 5 valid points - and threshold).  An empty mask writes the
    header alone.  grid: as in `save_mesh`."""
    from ..engine import centreline_lumen_profile, lumen_branch_summary
    grid = _export_grid(model, outside, n, grid)
    threshold = float(torch.tensor(float(threshold), dtype=torch.float32))      # the level the mask is cut at is the level the rays look for
    tree, a = _export_tree(grid, outside, n, threshold, prune_factor)
    prof = centreline_lumen_profile(tree['graph'], grid, a, threshold)
    host = {k: v.cpu().numpy() for k, v in prof.items() if isinstance(v, torch.Tensor)}
    n_points = int(host['flags'].size)
    summary = lumen_branch_summary(host)
    worst = float('nan'), -1
    known = ~np.isnan(summary['area_stenosis'])
    if known.any():
        q = int(np.flatnonzero(known)[np.argmax(summary['area_stenosis'][known])])
        worst = float(summary['area_stenosis'][q]), int(summary['branch'][q])
    first = {}
    tmp = f'{path}.tmp.{os.getpid()}'
    with open(tmp, 'w') as f:
        f.write(','.join(LUMEN_CSV_COLUMNS) + '\n')
        for k in range(n_points):
            b = int(host['branch'][k])
            first.setdefault(b, k)
            row = [b, k - first[b]] + [repr(float(v)) for v in host['points'][k]] + \
                  [repr(float(host[name][k])) for name in ('arc_length', 'area', 'd_min', 'd_max', 'r_mean')] + [int(host['flags'][k])]
            f.write(','.join(str(v) for v in row) + '\n')
    os.replace(tmp, path)
    info = dict(path=str(path), n_points=n_points, n_valid=int((host['flags'] == 0).sum()), max_area_stenosis=worst[0], branch=worst[1],
                threshold=float(threshold))
    print('lumen', info, flush=True)
    return info


BRANCH_CSV_COLUMNS = ('label', 'kind', 'territory_voxels', 'territory_volume', 'centreline_voxels', 'length', 'r_mean', 'r_min', 'r_max',
                      'node_start', 'node_end')


def save_branches(model, outside, n, threshold, path, prune_factor=1.0, grid=None):
    """--save_branches: one CSV row (BRANCH_CSV_COLUMNS, numbers written with repr) per branch, then per junction, of the pruned
    centreline of {sigma >= threshold} on the model's density grid (that of --save_centreline): territory_voxels = the voxels of the
    mask that lie nearest to that branch or junction (`engine.branch_territories`), territory_volume the same in world units, length
    (world units; 0 for a junction), the mean, minimum and maximum of the radius voxel x sqrt(d2) over its own centreline voxels, and the
    junction nodes its two ends are attached to (0: a free end; a junction row repeats its own number) -> its info (path, n_branches,
    n_nodes, n_rows, n_voxels, n_assigned, threshold).  No ground truth is read.  An empty mask writes the header alone.  grid: as in
    `save_mesh`."""
    from ..engine import branch_territories, territory_overlap
    if os.path.splitext(str(path))[1].lower() != '.csv':
        raise ValueError("--save_branches: PATH must end in .csv")
    grid = _export_grid(model, outside, n, grid)
    tree, _ = _export_tree(grid, outside, n, threshold, prune_factor)
    mask = grid >= torch.tensor(float(threshold), dtype=torch.float32, device=grid.device)
    graph = tree['graph']
    terr = branch_territories(graph)
    counts = territory_overlap(terr, mask).cpu().numpy()
    voxel = 2.0 * float(outside) / (int(n) - 1)
    labels = terr['labels'].reshape(-1)
    vox = torch.nonzero(labels, as_tuple=False).reshape(-1)
    lab = labels[vox].cpu().numpy()
    radius = np.sqrt((tree['d2'].reshape(-1)[vox].to(torch.int64) & 0xffffffff).cpu().numpy().astype(np.float64)) * voxel
    nb, nk = terr['n_branches'], terr['n_nodes']
    length = graph['length'].cpu().numpy()
    ends = np.stack([graph['node_start'].cpu().numpy(), graph['node_end'].cpu().numpy()], axis=1).reshape(nb, 2)
    tmp = f'{path}.tmp.{os.getpid()}'
    with open(tmp, 'w') as f:
        f.write(','.join(BRANCH_CSV_COLUMNS) + '\n')
        for l in range(1, nb + nk + 1):
            r = radius[lab == l]
            branch = l <= nb
            row = [l, 'branch' if branch else 'junction', int(counts[l, 1]), repr(float(counts[l, 1]) * voxel ** 3), int(r.size),
                   repr(float(length[l - 1]) if branch else 0.0), repr(float(r.mean())), repr(float(r.min())), repr(float(r.max())),
                   int(ends[l - 1, 0]) if branch else l - nb, int(ends[l - 1, 1]) if branch else l - nb]
            f.write(','.join(str(v) for v in row) + '\n')
    os.replace(tmp, path)
    info = dict(path=str(path), n_branches=nb, n_nodes=nk, n_rows=nb + nk, n_voxels=int(counts[:, 1].sum()), n_assigned=int(counts[1:, 1].sum()),
                threshold=float(threshold))
    print('branches', info, flush=True)
    return info


def save_cpr(model, outside, n, threshold, path, angles, half_width=16, prune_factor=1.0, smooth_passes=8, grid=None):
    """--save_cpr: the longitudinal images (`engine.centreline_cpr`: afx_reformat_planes) of the model's density grid (n points per axis
    over [-outside, outside]^3) along the main path of the pruned centreline of {sigma >= threshold} (that of --save_centreline), smoothed
    and resampled at the grid step, written as a float64 [A, P, K] array -> its info (path, shape, angles, step, n_rows, rows_flagged,
    branches, path_length, threshold).  A centreline without a free end (an empty mask among them) writes an array of no rows.  grid: as
    in `save_mesh`."""
    from ..engine import centreline_cpr
    grid = _export_grid(model, outside, n, grid)
    tree, a = _export_tree(grid, outside, n, threshold, prune_factor)
    angles = [float(x) for x in angles]
    step = float(outside) / (int(n) - 1)                  # half the grid step
    info = dict(branches=[], path_length=0.0, rows_flagged=0)
    images = np.zeros((len(angles), 0, 2 * int(half_width) + 1), np.float64)
    try:
        cpr = centreline_cpr(tree['graph'], grid, a, d2=tree['d2'], smooth_passes=smooth_passes, angles=angles, half_width=half_width, step=step)
    except ValueError as e:
        if 'centreline_main_path' not in str(e):
            raise
        info['reason'] = str(e)
    else:
        images = cpr['images'].cpu().numpy()
        info.update(branches=cpr['path']['branches'], path_length=cpr['path']['length'], rows_flagged=int((cpr['flags'] != 0).sum()))
    tmp = f'{path}.tmp.{os.getpid()}'
    with open(tmp, 'wb') as f:
        np.save(f, images)
    os.replace(tmp, path)
    info.update(path=str(path), shape=tuple(images.shape), angles=angles, step=step, n_rows=int(images.shape[1]), threshold=float(threshold))
    print('cpr', info, flush=True)
    return info


def save_view_map(model, outside, n, threshold, path, angles, width, height, focal, src_pt, prune_factor=1.0, grid=None, k=5):
    """--save_view_map: the foreshortening and overlap (`engine.view_map`: afx_view_map) of the pruned centreline of {sigma >= threshold} on
    the model's density grid (that of --save_centreline, radii voxel x sqrt(d2)) over `angles` [V, 2] posed as the evaluation sweep poses
    them, on a width x height detector; one CSV row per angle (theta, phi, tree_foreshortening, tree_overlap, then
    foreshortening_b and overlap_b of every branch b; numbers written with repr) -> its info (path, n_views, n_branches, n_segments,
    threshold, best: the k best whole-tree views as (theta, phi, score) by `engine.optimal_views`).  A centreline without a point writes
    NaN in the two whole-tree columns.  grid: as in `save_mesh`."""
    from ..engine import optimal_views, view_angles_records, view_map
    tree, a = _export_tree(_export_grid(model, outside, n, grid), outside, n, threshold, prune_factor)
    angles = np.asarray(angles, np.float64).reshape(-1, 2)
    nb = int(tree['graph']['n_branches']) if int(tree['graph']['path_voxels'].numel()) else 0
    vm = None
    if nb:
        vm = view_map(tree['graph'], view_angles_records(angles, src_pt, focal), int(width), int(height), index_to_world=a, d2=tree['d2'],
                      voxel_size=2.0 * float(outside) / (int(n) - 1))
    header = ['theta', 'phi', 'tree_foreshortening', 'tree_overlap']
    header += [f'{name}_{b + 1}' for b in range(nb) for name in ('foreshortening', 'overlap')]
    tmp = f'{path}.tmp.{os.getpid()}'
    with open(tmp, 'w') as f:
        f.write(','.join(header) + '\n')
        for v in range(angles.shape[0]):
            row = [repr(float(angles[v, 0])), repr(float(angles[v, 1])), repr(float(vm['tree_foreshortening'][v]) if nb else float('nan')),
                   repr(float(vm['tree_overlap'][v]) if nb else float('nan'))]
            for b in range(nb):
                row += [repr(float(vm['foreshortening'][v, b])), repr(float(vm['overlap'][v, b]))]
            f.write(','.join(str(x) for x in row) + '\n')
    os.replace(tmp, path)
    best = []
    if nb:
        idx, score = optimal_views(vm, k=k)
        best = [(float(angles[i, 0]), float(angles[i, 1]), float(s)) for i, s in zip(idx, score)]
    info = dict(path=str(path), n_views=int(angles.shape[0]), n_branches=nb, n_segments=vm['n_segments'] if nb else 0, threshold=float(threshold),
                best=best)
    print('view map', info, flush=True)
    return info


POSE_CSV_COLUMNS = ('image_id',) + tuple(f'given_{r}{c}' for r in range(3) for c in range(4)) + \
    tuple(f'refined_{r}{c}' for r in range(3) for c in range(4)) + ('chamfer_before', 'chamfer_after', 'rms_before', 'rms_after', 'shift_px', 'accepted', 'selected')


def save_poses(model, outside, n, threshold, path, proj_df, train_ray_df, test_proj_id, mask_threshold, device, dof='all', trunc=8.0,
               search=None, iterations=20, prune_factor=1.0, grid=None):
    """--save_poses: every training view's pose registered (`engine.centreline_register_poses`: afx_pose_chamfer, afx_pose_lm_step) to its
    silhouette (`training_view_masks` at mask_threshold): the points are the pruned centreline of {sigma >= threshold} on the model's
    density grid (that of --save_centreline, radii voxel x sqrt(d2)).  One CSV row per view (POSE_CSV_COLUMNS: the first three rows of the
    given and the refined cam2world, the mean chamfer residual in pixels before and after, its root mean square before and after (the
    figure the registration minimises, so it never rises), the mean shift of the points' projections,
    the accepted steps and the search's candidate; numbers written with repr) -> its info (path, n_views, n_points, dof, trunc,
    chamfer_before, chamfer_after, shift_px: the means over the views).  A centreline without a point writes the header alone."""
    tree, a = _export_tree(_export_grid(model, outside, n, grid), outside, n, threshold, prune_factor)
    poses, masks, focal = training_view_masks(proj_df, train_ray_df, test_proj_id, mask_threshold, device)
    ids = [i for i in proj_df.index if i != test_proj_id]
    n_points = int(tree['graph']['path_voxels'].numel())
    reg = None
    if n_points:
        views = _engine.pose_views(poses, masks, focal)
        reg = _engine.centreline_register_poses(tree['graph'], views, index_to_world=a, d2=tree['d2'],
                                                voxel_size=2.0 * float(outside) / (int(n) - 1), iterations=iterations, trunc=float(trunc),
                                                dof=dof, search=None if search is None else (float(search[0]), float(search[1]), int(search[2])))
    tmp = f'{path}.tmp.{os.getpid()}'
    with open(tmp, 'w') as f:
        f.write(','.join(POSE_CSV_COLUMNS) + '\n')
        for v in range(len(ids) if reg is not None else 0):
            row = [ids[v]] + [repr(float(x)) for x in np.asarray(poses[v], np.float64)[:3].reshape(-1)] + \
                  [repr(float(x)) for x in reg['poses'][v, :3].reshape(-1)] + \
                  [repr(float(reg[k][v])) for k in ('mean_residual_before', 'mean_residual_after', 'rms_residual_before', 'rms_residual_after')] + \
                  [repr(float(reg['shift_px'][v])),
                   int(reg['accepted'][v]), int(reg['selected'][v])]
            f.write(','.join(str(x) for x in row) + '\n')
    os.replace(tmp, path)
    mean = lambda key: float(np.mean(reg[key])) if reg is not None else float('nan')
    info = dict(path=str(path), n_views=len(ids), n_points=n_points, dof=str(dof), trunc=float(trunc), chamfer_before=mean('mean_residual_before'),
                chamfer_after=mean('mean_residual_after'), shift_px=mean('shift_px'))
    print('poses', info, flush=True)
    return info


if __name__ == "__main__":
    main()
