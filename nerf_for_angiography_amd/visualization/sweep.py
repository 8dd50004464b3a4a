"""Evaluation sweep — the metric loop of the reference's visualization/visualization.py:188-191,277-505: render the model
from a grid of C-arm angles (th x ph, the "37 x 37" sweep at limited_size_vis = 180, angle_step_vis = 5), compare every
projection with the ground truth and tabulate per-view metrics, and compare the reconstructed density grid with the ground-truth volume.

What differs from upstream is where the work happens: ALL views of the sweep are ONE fused launch (rays of every pose are
generated in the kernel from the [n_views, 3, 4] pose table, `render_projection`), the ground truth of a voxel phantom is one
`afx_project_volume` launch over the same poses, and the metrics are reductions on the GPU.  Metrics: PSNR (:406-409,
data range 1), SSIM (:411-417: torchmetrics' StructuralSimilarityIndexMeasure(data_range=1.0), a fixed 11-tap Gaussian window with
no network - every view in one `afx_ssim` call, in fp64), normalised DOT 2D (:440-450), DICE 2D on the binarised projections
(:433-438; prediction binarised by zeroing densities below `binary_thresh`, :172,349-352), and the two whole-volume scores DICE 3D and
DOT 3D (:480-495) of `reconstruction_metrics`: the model's density grid against the ground-truth volume sampled at the same points
(`afx_volume_grid`).  LPIPS and DISTS upstream are pretrained networks whose weights this project does not ship: out of scope.

Beyond the reference: eleven more families of whole-volume scores on the same two grids, each a reconstruction_* function with a tuple of
column names, listed in table order in _VOLUME_FAMILIES at the end of this file; what a family scores is in its function's docstring.
The surface distances between the two thresholded grids (`afx_surface_metrics_3d`), the connected pieces of the reconstruction
(`afx_label_components_3d`), clDice on the medial curves (`afx_skeletonize_3d`), the vessel as a capped triangle mesh
(`reconstruction_mesh`, `afx_isosurface_3d`; visualization/mesh_io.py writes it) with its measures and the distance between the two
meshes (`afx_mesh_point_distance`), the pruned centreline read as a graph (`afx_prune_spurs`, `afx_centreline_graph`), the tubular
share by the 3-D Frangi filter (`afx_frangi_3d`), the lumen's cross-sections along the true centreline (`afx_lumen_profile`), the
visual hull of the training views (`afx_visual_hull`) and the classical baseline, the algebraic reconstruction (SIRT) of the attenuation
volume from the same views (`afx_xray_project`, `afx_xray_backproject`), plain and with a total-variation step (`afx_tv_denoise_3d`).  The families share what they derive from the grids through one `GridAnalysis`;
the chain mask -> distance transform -> skeleton -> pruned skeleton -> graph is `centreline_tree`."""
from __future__ import annotations

import itertools

import numpy as np
import pandas as pd
import torch

from ..phantomdata.proj_helpers import source_matrix
from ..render import density_grid, march_render_projection, render_projection

# the reference's metric columns in its order (visualization.py:455-495); LPIPS and DISTS need pretrained networks
METRICS = ("PSNR", "SSIM", "LPIPS", "DISTS", "DICE 2D", "DOT 2D", "DICE 3D", "DOT 3D")
_NETWORK_METRICS = ("LPIPS", "DISTS")
# not in the reference: one tuple of columns per family of whole-volume scores, tabulated behind the reference's columns in this order
# (_VOLUME_FAMILIES pairs each with its reconstruction_* function); all need the ground-truth volume
SURFACE_METRICS = ("DICE 3D VESSEL", "ASSD 3D", "HD 3D", "HD95 3D")                  # how far the two vessel surfaces lie apart, on the grid
TOPOLOGY_METRICS = ("COMPONENTS 3D", "LCC FRACTION 3D", "DICE 3D LCC")               # one vessel tree, or a tree plus floaters
CENTRELINE_METRICS = ("CLDICE 3D", "TPREC 3D", "TSENS 3D")                           # clDice (Shit et al. 2021)
MESH_METRICS = ("VOLUME RATIO 3D", "AREA RATIO 3D", "EULER 3D")                      # the vessel measured as a surface
_EXTRA_METRICS = SURFACE_METRICS + TOPOLOGY_METRICS + CENTRELINE_METRICS + MESH_METRICS
MESH_DISTANCE_METRICS = ("ASSD MESH", "HD MESH", "HD95 MESH")                        # how far the two meshes lie apart, below the voxel
GRAPH_METRICS = ("BRANCHES 3D", "JUNCTIONS 3D", "LENGTH RATIO 3D")                   # the pruned centreline read as a graph
_VOLUME_METRICS = _EXTRA_METRICS + MESH_DISTANCE_METRICS + GRAPH_METRICS
VESSELNESS_METRICS = ("TUBULAR FRACTION 3D", "DICE 3D TUBULAR", "SCALE RATIO 3D")    # is the thresholded reconstruction tube-shaped at all
LUMEN_METRICS = ("LUMEN AREA ERR 3D", "MLA RATIO 3D", "STENOSIS ERR 3D")             # the lumen's width along the TRUE centreline
_ALL_VOLUME_METRICS = _VOLUME_METRICS + VESSELNESS_METRICS + LUMEN_METRICS
# against the visual hull of the training views: needs the views (hull_views=engine.visual_hull_views(...)) besides the volume
HULL_METRICS = ("OUTSIDE HULL 3D", "DICE 3D HULL", "HULL RATIO 3D")
# and how it stands against the classical baseline, the algebraic reconstruction (SIRT) of the attenuation volume from the same training
# views (reconstruction_sirt_metrics: afx_xray_project, afx_xray_backproject), a tuple of its own, tabulated behind the hull columns; it
# needs the views with their line integrals (sirt_views=(engine.xray_views(...), line integrals)) and the ground-truth volume
SIRT_METRICS = ("DICE 3D SIRT", "DICE GAIN 3D", "CORR 3D SIRT")
# and SIRT-TV, the same reconstruction with a total-variation denoising step (afx_tv_denoise_3d) after every update, against plain SIRT;
# it needs sirt_views, the ground-truth volume and a weight (sirt_tv_weight)
SIRT_TV_METRICS = ("DICE 3D SIRT-TV", "TV GAIN 3D", "CORR 3D SIRT-TV")
# and whether the reconstruction would send the C-arm where the truth would: the foreshortening and overlap map (engine.view_map:
# afx_view_map) of the two pruned centrelines over the sweep's own angles, a tuple of its own behind all the families above; it needs
# the ground-truth volume
VIEW_METRICS = ("FORESHORTENING ERR 3D", "OVERLAP ERR 3D", "VIEW REGRET 3D")
# and the picture behind the lumen numbers: the longitudinal (curved-planar reformation) images of the two grids along the main path of
# the TRUE centreline (engine.cpr_images: afx_reformat_planes), compared as images; a tuple of its own behind the view columns; it needs
# the ground-truth volume
CPR_METRICS = ("CPR PSNR 3D", "CPR SSIM 3D", "CPR CORR 3D")
# and whether the poses the model was trained with fit the silhouettes of its training views: the 2D-3D chamfer of the pruned predicted
# centreline against the views' signed distance images before and after a rigid registration of every pose (engine.register_poses:
# afx_pose_chamfer, afx_pose_lm_step); a tuple of its own behind the CPR columns.  It needs the training views
# (pose_views=engine.pose_views(poses, masks, focal)) and NO ground truth: volume=None works, with a threshold
POSE_METRICS = ("CHAMFER 2D", "CHAMFER 2D REFINED", "POSE SHIFT 2D")
# and WHICH branch was lost, thinned or doubled: every vessel voxel of either mask goes to the branch of the TRUE pruned centreline it
# lies nearest to (engine.branch_territories: afx_feature_transform_3d, afx_label_overlap_3d), scored branch by branch
# (reconstruction_branch_metrics); a tuple of its own behind the pose columns; it needs the ground-truth volume
BRANCH_METRICS = ("BRANCH RECALL 3D", "WORST BRANCH DICE 3D", "BRANCH RADIUS ERR 3D")
CPR_MIN_ROWS = 11                    # afx_ssim takes images of at least 11 x 11


def sweep_angles(limited_size_vis: float = 180.0, angle_step_vis: float = 5.0):
    """visualization.py:188-191: th, ph in arange(-L//2, L//2 + 1, step), all pairs."""
    a = np.arange(-limited_size_vis // 2, limited_size_vis // 2 + 1, angle_step_vis).astype("float64")
    return np.array([np.array(v) for v in itertools.product(a, a)])


def _poses(angles, src_pt, translation, device):
    mats = []
    for theta, phi in angles:
        th = theta if theta >= 0 else 360 + theta            # :280-281
        ph = phi if phi >= 0 else 360 + phi
        mats.append(source_matrix(np.asarray(src_pt, dtype=np.float64), th, ph, 0.0, np.asarray(translation, dtype=np.float64)))
    return torch.from_numpy(np.stack(mats)).to(device)


@torch.no_grad()
def evaluation_sweep(model, targets, angles, img_width, img_height, focal_length, src_pt, near_thresh, far_thresh,
                     depth_samples_per_ray, translation=(0.0, 0.0, 0.0), binary_thresh=0.05, binary_targets=None,
                     views_per_launch=512, grid=None, scene_aabb=None, early_stop_eps=1e-2, alpha_thre=1e-3, metrics=None, volume=None,
                     volume_outside=100.0, volume_points=None, hull_views=None, sirt_views=None, sirt_iterations=50, sirt_relax=1.0,
                     sirt_tv_weight=None, sirt_tv_iterations=10, pose_views=None, pose_threshold=None):
    """Per-view metrics of `model` over `angles` [n,2] (theta, phi in degrees).

    grid: an occupancy grid (nerf.occupancy.OccupancyGrid, e.g. restored with `grid._binary = mask` as visualization.py:162 does) - the views
    are then rendered as the reference renders CT models (:335-352): acc_ray_marching through the grid and `scene_aabb` with
    (early_stop_eps, alpha_thre), the kept samples composited, the binary image from the same samples with sigma < binary_thresh zeroed -
    each chunk of views ONE `march_render_projection` call (one evaluation of the model).  grid=None: the dense fixed-step render.

    targets: [n, H, W] ground-truth projections on the model's device (e.g. `ground_truth_sweep`), binary_targets likewise
    (optional; DICE 2D needs them).  Returns a DataFrame with the reference's columns (image_id, theta, phi, larm,
    theta_360, phi_360, cam_pose_x/y/z, then the metrics) and the predicted images [n, H, W].

    metrics=None: the metric columns PSNR, DOT 2D[, DICE 2D when binary_targets are given].  Otherwise a list drawn from METRICS, tabulated
    in the reference's order (PSNR, SSIM, DICE 2D, DOT 2D, DICE 3D, DOT 3D); LPIPS and DISTS raise NotImplementedError.  DICE 2D needs
    binary_targets.

    The whole-volume columns - DICE 3D, DOT 3D and the families of _VOLUME_FAMILIES, tabulated in that table's order behind the reference's
    columns - need `volume` (a VoxelVolume), the hull columns `hull_views` = engine.visual_hull_views(...) of the training views as well.
    Each family is one call of the table's function at its defaults (threshold mean(gt)) on volume_points points per axis over
    [-volume_outside, volume_outside]^3 (default depth_samples_per_ray + 1 as upstream, :102), its scores repeated on every row (:490,
    :495).  All families share one `GridAnalysis`: the two grids are evaluated once, and so is every mask, skeleton, centreline, mesh and
    filter response more than one family reads.  The SIRT columns need `sirt_views` = (engine.xray_views(...) of the training views,
    their line integrals [V, H, W]) besides `volume`: one `reconstruction_sirt_metrics` call at sirt_iterations and sirt_relax; when
    `hull_views` is given as well, the hull - taken once, whoever asks first - is the support mask of the reconstruction.  The SIRT-TV
    columns need sirt_tv_weight as well: the same call with tv_weight = sirt_tv_weight and tv_iterations = sirt_tv_iterations; plain
    SIRT, which both families read, runs once.  The VIEW_METRICS columns stand behind all of these and need `volume` alone: one
    `reconstruction_view_metrics` call over the sweep's own angles, detector, focal length and source, on the pruned centrelines the
    shared analysis holds.  The POSE_METRICS columns stand behind the CPR columns and need `pose_views` = engine.pose_views(...) of the training views
    and no ground truth: one `reconstruction_pose_metrics` call at pose_threshold (None: mean(gt), which needs `volume`).  The BRANCH_METRICS
    columns stand behind those and need `volume` alone: one `reconstruction_branch_metrics` call at its defaults on the pruned
    centrelines the shared analysis holds.  The arguments are checked before any work on the GPU."""
    from ..engine import ssim
    want = _check_metrics(metrics, binary_targets, volume, hull_views, sirt_views, sirt_tv_weight, pose_views, pose_threshold)
    dev = model.flat_params.device
    n = len(angles)
    poses = _poses(angles, src_pt, translation, dev)
    hw = int(img_width) * int(img_height)
    preds = torch.empty(n, hw, device=dev)
    bin_preds = torch.empty(n, hw, device=dev) if "DICE 2D" in want else None
    for v0 in range(0, n, views_per_launch):
        v1 = min(n, v0 + views_per_launch)
        if grid is not None:
            res = march_render_projection(model, grid, scene_aabb, poses[v0:v1], img_width, img_height, focal_length, depth_samples_per_ray,
                                          near_thresh, far_thresh, early_stop_eps, alpha_thre,
                                          binary_thresh=binary_thresh if bin_preds is not None else None)
            preds[v0:v1] = res[0].view(v1 - v0, hw)
            if bin_preds is not None:
                bin_preds[v0:v1] = res[1].view(v1 - v0, hw)
            continue
        out = render_projection(model, poses[v0:v1], img_width, img_height, focal_length, depth_samples_per_ray, near_thresh,
                                far_thresh, want_aux=bin_preds is not None)
        preds[v0:v1] = out.rgb_map.view(v1 - v0, hw)
        if bin_preds is not None:
            # densities below the threshold are zeroed before compositing (zero_idx of acc_render_volume_density)
            step = (far_thresh - near_thresh) / depth_samples_per_ray
            tau = out.sigma * (out.sigma >= binary_thresh) * step
            bin_preds[v0:v1] = torch.exp(-tau.sum(-1)).view(v1 - v0, hw)
    tgt = targets.reshape(n, hw).to(dev, torch.float32)
    mse = ((preds - tgt) ** 2).mean(-1)
    psnr = -10.0 * torch.log10(mse)
    def norm01(x):
        x = x - x.min(-1, keepdim=True).values
        return x / x.max(-1, keepdim=True).values
    dot2d = (norm01(preds) * norm01(tgt)).mean(-1)
    cols = {"image_id": [f"{t}-{p}".replace(".", ",") for t, p in angles], "theta": [float(a[0]) for a in angles],
            "phi": [float(a[1]) for a in angles], "larm": [0] * n,
            "theta_360": [float(a[0] if a[0] >= 0 else 360 + a[0]) for a in angles],
            "phi_360": [float(a[1] if a[1] >= 0 else 360 + a[1]) for a in angles],
            "cam_pose_x": poses[:, 0, 3].cpu().tolist(), "cam_pose_y": poses[:, 1, 3].cpu().tolist(),
            "cam_pose_z": poses[:, 2, 3].cpu().tolist()}
    scores = {"PSNR": psnr.cpu().tolist(), "DOT 2D": dot2d.cpu().tolist()}
    if bin_preds is not None:
        bp = (bin_preds >= 1).to(torch.int64)               # :434-435: everything below 1 is vessel -> 0
        bt = (binary_targets.reshape(n, hw).to(dev) >= 1).to(torch.int64)
        # Dice(average='micro') over the two classes of a binary image = pixel accuracy
        scores["DICE 2D"] = (bp == bt).float().mean(-1).cpu().tolist()
    if "SSIM" in want:
        scores["SSIM"] = ssim(preds.view(n, int(img_height), int(img_width)), tgt.view(n, int(img_height), int(img_width))).cpu().tolist()
    analysis = None
    for names, score, keys in _VOLUME_FAMILIES:
        if not any(m in want for m in names):
            continue
        if analysis is None:                                  # the two n^3 grids, evaluated once for every family
            pts = int(volume_points) if volume_points is not None else int(depth_samples_per_ray) + 1
            analysis = GridAnalysis(*_reconstruction_grids(model, volume, volume_outside, pts), volume_outside, pts)
        views, kw = ((hull_views,), {}) if names is HULL_METRICS else ((), {})
        if names is SIRT_METRICS or names is SIRT_TV_METRICS:
            views, kw = tuple(sirt_views), dict(iterations=sirt_iterations, relax=sirt_relax, hull_views=hull_views)
        if names is SIRT_TV_METRICS:
            kw.update(tv_weight=sirt_tv_weight, tv_iterations=sirt_tv_iterations)
        got = score(model, volume, volume_outside, pts, *views, grids=analysis, **kw)[0]
        for name, key in zip(names, keys):
            scores[name] = [got[key]] * n
    if any(m in want for m in VIEW_METRICS):                  # behind the families: its views are the sweep's own angles
        if analysis is None:
            pts = int(volume_points) if volume_points is not None else int(depth_samples_per_ray) + 1
            analysis = GridAnalysis(*_reconstruction_grids(model, volume, volume_outside, pts), volume_outside, pts)
        got = reconstruction_view_metrics(model, volume, volume_outside, pts, angles, img_width, img_height, focal_length, src_pt, translation,
                                          grids=analysis)[0]
        for name, key in zip(VIEW_METRICS, ("foreshortening_err", "overlap_err", "view_regret")):
            scores[name] = [got[key]] * n
    if any(m in want for m in CPR_METRICS):                   # behind the view columns
        if analysis is None:
            pts = int(volume_points) if volume_points is not None else int(depth_samples_per_ray) + 1
            analysis = GridAnalysis(*_reconstruction_grids(model, volume, volume_outside, pts), volume_outside, pts)
        got = reconstruction_cpr_metrics(model, volume, volume_outside, pts, grids=analysis)[0]
        for name, key in zip(CPR_METRICS, ("cpr_psnr", "cpr_ssim", "cpr_corr")):
            scores[name] = [got[key]] * n
    if any(m in want for m in POSE_METRICS):                  # behind the CPR columns; the one family that needs no truth
        pts = int(volume_points) if volume_points is not None else int(depth_samples_per_ray) + 1
        got = reconstruction_pose_metrics(model, volume, volume_outside, pts, pose_views, threshold=pose_threshold, grids=analysis)[0]
        for name, key in zip(POSE_METRICS, ("chamfer", "chamfer_refined", "pose_shift")):
            scores[name] = [got[key]] * n
    if any(m in want for m in BRANCH_METRICS):                # behind the pose columns
        pts = int(volume_points) if volume_points is not None else int(depth_samples_per_ray) + 1
        if analysis is None:
            analysis = GridAnalysis(*_reconstruction_grids(model, volume, volume_outside, pts), volume_outside, pts)
        got = reconstruction_branch_metrics(model, volume, volume_outside, pts, grids=analysis)[0]
        for name, key in zip(BRANCH_METRICS, ("branch_recall", "worst_branch_dice", "branch_radius_err")):
            scores[name] = [got[key]] * n
    for name in want:
        cols[name] = scores[name]
    return pd.DataFrame(cols), preds.view(n, int(img_height), int(img_width))


def _check_metrics(metrics, binary_targets, volume, hull_views=None, sirt_views=None, sirt_tv_weight=None, pose_views=None, pose_threshold=None):
    """The metric columns evaluation_sweep fills, in order; raises on a request it cannot serve (before any GPU work)."""
    if metrics is None:
        return ["PSNR", "DOT 2D"] + (["DICE 2D"] if binary_targets is not None else [])
    metrics = [metrics] if isinstance(metrics, str) else list(metrics)
    known = METRICS + _ALL_VOLUME_METRICS + HULL_METRICS + SIRT_METRICS + SIRT_TV_METRICS + VIEW_METRICS + CPR_METRICS + POSE_METRICS + \
        BRANCH_METRICS
    unknown = [m for m in metrics if m not in known]
    if unknown:
        raise ValueError(f"evaluation_sweep: unknown metrics {unknown}; choose from {list(known)}")
    nets = [m for m in metrics if m in _NETWORK_METRICS]
    if nets:
        raise NotImplementedError(f"evaluation_sweep: {nets} need pretrained networks (LPIPS: AlexNet/VGG features, DISTS: VGG16 "
                                  "with learned weights) whose weights this project does not ship")
    if "DICE 2D" in metrics and binary_targets is None:
        raise ValueError("evaluation_sweep: DICE 2D needs binary_targets")
    if ("DICE 3D" in metrics or "DOT 3D" in metrics) and volume is None:
        raise ValueError("evaluation_sweep: DICE 3D and DOT 3D need the ground-truth volume (volume=VoxelVolume)")
    if any(m in metrics for m in _ALL_VOLUME_METRICS) and volume is None:
        raise ValueError(f"evaluation_sweep: {[m for m in metrics if m in _ALL_VOLUME_METRICS]} need the ground-truth volume (volume=VoxelVolume)")
    hull = [m for m in metrics if m in HULL_METRICS]
    if hull and hull_views is None:
        raise ValueError(f"evaluation_sweep: {hull} need the training views (hull_views=engine.visual_hull_views(poses, masks, focal))")
    if hull and volume is None:
        raise ValueError(f"evaluation_sweep: {hull} need the ground-truth volume (volume=VoxelVolume)")
    sirt = [m for m in metrics if m in SIRT_METRICS + SIRT_TV_METRICS]
    if sirt and sirt_views is None:
        raise ValueError(f"evaluation_sweep: {sirt} need the training views and their line integrals "
                         "(sirt_views=(engine.xray_views(...), engine.line_integrals(images)))")
    if sirt and volume is None:
        raise ValueError(f"evaluation_sweep: {sirt} need the ground-truth volume (volume=VoxelVolume)")
    tv = [m for m in metrics if m in SIRT_TV_METRICS]
    if tv and sirt_tv_weight is None:
        raise ValueError(f"evaluation_sweep: {tv} need the weight of the total variation (sirt_tv_weight=W)")
    view = [m for m in metrics if m in VIEW_METRICS + CPR_METRICS + BRANCH_METRICS]
    if view and volume is None:
        raise ValueError(f"evaluation_sweep: {view} need the ground-truth volume (volume=VoxelVolume)")
    pose = [m for m in metrics if m in POSE_METRICS]
    if pose and pose_views is None:
        raise ValueError(f"evaluation_sweep: {pose} need the training views (pose_views=engine.pose_views(poses, masks, focal))")
    if pose and volume is None and pose_threshold is None:
        raise ValueError(f"evaluation_sweep: {pose} without a ground-truth volume need the level the prediction is cut at (pose_threshold=T)")
    return [m for m in known if m in metrics]


@torch.no_grad()
def ground_truth_grid(volume, outside, n):
    """The ground-truth density of a `VoxelVolume` at np.meshgrid(t, t, t), t = linspace(-outside, outside, n) (visualization.py:100-102,
    229: gt_interpolator(query_pts)): one afx_volume_grid launch, float32 [n, n, n] in density_grid's layout."""
    from ..engine import volume_grid
    return volume_grid(volume.values, volume.origin, volume.spacing, volume.fill_value, -float(outside), float(outside), int(n))


@torch.no_grad()
def _reconstruction_grids(model, volume, outside, n, grids=None):
    """(predicted grid, ground-truth grid) at the n^3 points of the whole-volume scores; `grids`, when given, is that pair already
    evaluated (both are bit-reproducible, so sharing them between the scores changes nothing)."""
    if grids is not None:
        return grids
    return density_grid(model, outside, int(n) - 1), ground_truth_grid(volume, outside, n)


def centreline_skeleton(mask):
    """The unpruned half of `centreline_tree` -> {"dist", "d2", "skeleton", "skeleton_record"}: the exact distance transform of a bool
    device mask with its integer square (one `engine.distance_transform_edt_3d` call), its medial curves and their thinning record."""
    from ..engine import distance_transform_edt_3d, skeletonize_3d
    dist, d2 = distance_transform_edt_3d(mask, return_squared=True)
    skeleton, record = skeletonize_3d(mask, return_record=True)
    return {"dist": dist, "d2": d2, "skeleton": skeleton, "skeleton_record": record}


def centreline_tree(mask, index_to_world, prune_factor=1.0, skeleton=None):
    """The centreline of a bool device mask, from the mask to the graph -> `centreline_skeleton(mask)` (or `skeleton`, that result computed
    earlier: the mask is not read then) plus "pruned" and "prune_record" (`engine.prune_spurs` at `prune_factor` with d2: a spur no longer
    than prune_factor x the vessel radius at its junction is a thinning artefact) and "graph" (`engine.centreline_graph` of pruned)."""
    from ..engine import centreline_graph, prune_spurs
    tree = dict(centreline_skeleton(mask) if skeleton is None else skeleton)
    tree["pruned"], tree["prune_record"] = prune_spurs(tree["skeleton"], tree["d2"], prune_factor, return_record=True)
    tree["graph"] = centreline_graph(tree["pruned"], tree["d2"], index_to_world)
    return tree


class GridAnalysis:
    """The predicted and the ground-truth grid of the whole-volume scores (n^3 points over [-outside, outside]^3; gt None where there is no
    truth) and what more than one family of scores derives from them.  Each method computes its result once per set of the arguments it
    depends on and keeps it in `cache`; everything kept is bit-reproducible, so sharing changes no number.  Every reconstruction_* function
    takes one as `grids=`; whoever holds one leaves the tensors it hands out unchanged."""

    def __init__(self, pred, gt, outside, n):
        self.pred, self.gt, self.outside, self.n, self.cache = pred, gt, float(outside), int(n), {}
        self.voxel, self.index_to_world = 2.0 * self.outside / (self.n - 1), grid_index_to_world(outside, n)      # voxel: the grid step

    def _once(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def threshold(self, threshold=None):
        """The level both grids are cut at, as a float: `threshold`, or mean(gt) in fp32 - the rule DICE 3D uses."""
        return self._once("mean(gt)", lambda: float(torch.mean(self.gt))) if threshold is None else float(threshold)

    def masks(self, thr):
        """(A = pred >= thr, B = gt >= thr, |A|, |B|), thr rounded to fp32 as the grids are; without a ground truth B is None and |B| 0."""
        def cut():
            t32 = torch.tensor(thr, dtype=torch.float32, device=self.pred.device)
            a, b = self.pred >= t32, None if self.gt is None else self.gt >= t32
            return a, b, int(a.sum()), 0 if b is None else int(b.sum())
        return self._once(("masks", thr), cut)

    def body(self, thr, largest_component=False, connectivity=3):
        """A, or with largest_component its largest connected piece alone (`connectivity` 1, 2, 3 = 6, 18, 26 neighbours)."""
        from ..engine import filter_components_3d
        if not largest_component:
            return self.masks(thr)[0]
        return self._once(("body", thr, int(connectivity)), lambda: filter_components_3d(self.masks(thr)[0], connectivity, largest_only=True))

    def skeleton(self, side, thr, largest_component=False):
        """`centreline_skeleton` of `side`: "gt" is B, "pred" body(thr, largest_component) at 26 neighbours - the truth is never filtered."""
        lc = side == "pred" and bool(largest_component)
        return self._once(("skeleton", side, thr, lc), lambda: centreline_skeleton(self.body(thr, lc) if side == "pred" else self.masks(thr)[1]))

    def tree(self, side, thr, largest_component=False, prune_factor=1.0):
        """`centreline_tree` of the same mask at the grid's index_to_world, grown from the shared skeleton."""
        lc = side == "pred" and bool(largest_component)
        return self._once(("tree", side, thr, lc, float(prune_factor)),
                          lambda: centreline_tree(None, self.index_to_world, prune_factor, self.skeleton(side, thr, lc)))

    def mesh(self, side, thr, largest_component=False, connectivity=3):
        """(vertices, triangles, info) of `_grid_mesh`: the capped surface of `side` at the level thr in world coordinates; the largest
        component of the prediction is meshed at 0.5 - its surface runs half-way between the voxels."""
        if side == "pred" and largest_component:
            return self._once(("mesh", side, thr, int(connectivity)),
                              lambda: _grid_mesh(self.body(thr, True, connectivity).float(), 0.5, self.outside, self.n))
        return self._once(("mesh", side, thr), lambda: _grid_mesh(self.pred if side == "pred" else self.gt, thr, self.outside, self.n))

    def frangi(self, side, sigmas):
        """(vesselness float64, index of the selected scale uint8) of `engine.frangi_3d` over the grid of `side`."""
        from ..engine import frangi_3d
        return self._once(("frangi", side, tuple(float(s) for s in sigmas)),
                          lambda: frangi_3d(self.pred if side == "pred" else self.gt, sigmas, return_scale=True))

    def hull(self, views):
        """`engine.visual_hull` of `views` (engine.visual_hull_views) over the grid's points, each speaking for its voxel: bool [n^3].
        Kept per views object (which the cache holds on to)."""
        from ..engine import visual_hull
        return self._once(("hull", id(views)), lambda: (visual_hull(views, tuple(self.pred.shape), self.index_to_world), views))[0]

    def sirt(self, views, images, iterations, relax, support=None, tv_weight=None, tv_iterations=10):
        """(volume, residual history) of `engine.sirt_reconstruct` on the grid's points with `support` (None, or a mask this analysis or
        the caller made) as its mask.  Kept per views, images and support object (which the cache holds on to) and per setting, so plain
        SIRT runs once for every family that reads it."""
        from ..engine import sirt_reconstruct
        tv = None if tv_weight is None else (float(tv_weight), int(tv_iterations))
        key = ("sirt", id(views), id(images), id(support), int(iterations), float(relax), tv)
        def run():
            kw = {} if tv is None else dict(tv_weight=tv[0], tv_iterations=tv[1])
            return sirt_reconstruct(views, images, tuple(self.pred.shape), self.index_to_world, iterations=iterations, relax=relax, mask=support,
                                    return_history=True, **kw), (views, images, support)
        return self._once(key, run)[0]


def _analysis(model, volume, outside, n, grids, threshold):
    """(the GridAnalysis a reconstruction_* function works on, its threshold): `grids` itself when it is one, else a fresh one around the
    (predicted, ground-truth) pair `grids`, or around the two grids evaluated here."""
    if not isinstance(grids, GridAnalysis):
        grids = GridAnalysis(*_reconstruction_grids(model, volume, outside, n, grids), outside, n)
    if (grids.outside, grids.n) != (float(outside), int(n)):
        raise ValueError(f"grids= holds {grids.n} points per axis over +-{grids.outside}, the call asks for {int(n)} over +-{float(outside)}")
    return grids, grids.threshold(threshold)


def _refuse_empty(who, n_pred, n_gt, what):
    """The ValueError every family raises, under its own name, when its threshold leaves the prediction or the truth with nothing."""
    empty = [name for cnt, name in ((n_pred, "pred"), (n_gt, "gt")) if cnt == 0]
    if empty:
        raise ValueError(f"{who}: no voxel of {' or '.join(empty)} reaches its threshold: an empty {what}")


@torch.no_grad()
def reconstruction_metrics(model, volume, outside, n, grids=None):
    """DICE 3D and DOT 3D of visualization.py:480-495 for 'ct' data -> (dice_3d, dot_3d, predicted grid, ground-truth grid).

    The predicted grid is the model's density at every one of the n^3 points (query_occ masks nothing there: `occ_pts >= 0` keeps them all,
    :216-219), `density_grid(model, outside, n - 1)`; the ground truth `ground_truth_grid(volume, outside, n)`.  thr = mean(gt) in fp32 as
    torch.mean gives it; DICE 3D is the fraction of points where (pred >= thr) == (gt >= thr) (Dice(average='micro') over both classes of a
    0/1 volume, as DICE 2D); DOT 3D = mean(pred * gt), the products in fp32, their mean accumulated in fp64."""
    pred, gt = (grids.pred, grids.gt) if isinstance(grids, GridAnalysis) else _reconstruction_grids(model, volume, outside, n, grids)
    thr = torch.mean(gt)
    agree = ((pred >= thr) == (gt >= thr)).sum()
    dice = agree.double() / gt.numel()
    dot = torch.mean(pred * gt, dtype=torch.float64)
    return float(dice), float(dot), pred, gt


@torch.no_grad()
def reconstruction_surface_metrics(model, volume, outside, n, threshold=None, q=95.0, largest_component=False, connectivity=3, grids=None):
    """How far the reconstructed vessel lies from the true one -> (scores, predicted grid, ground-truth grid).

    The two grids are those of `reconstruction_metrics` (n^3 points over [-outside, outside]^3); both are thresholded at `threshold`,
    which defaults to mean(gt) in fp32 - the rule DICE 3D uses; pass e.g. the sweep's binary_thresh instead.  scores
    (`engine.surface_metrics_3d`; medpy.metric.binary's dc / assd / hd / hd95 definitions): dice_vessel, the Dice of the vessel class
    alone (DICE 3D counts the background, more than 99 % of the grid, as well); assd, hd and hd_percentile (the q-th percentile of the
    surface distances of both directions) in WORLD units - the voxel distances times the grid step 2 outside / (n - 1), multiplied in fp64;
    voxel_size, threshold, q and the counts.  ValueError when the threshold leaves either grid empty.  largest_component: the scores of
    the largest connected component of pred >= threshold alone (`connectivity` 1, 2, 3 = 6, 18, 26 neighbours) - the surface distances
    without the floaters, one stray voxel of which sets HD; the returned predicted grid is the unfiltered one.  grids: the (predicted,
    ground-truth) pair another of the reconstruction_* functions returned for the same points, to save evaluating them again, or a
    `GridAnalysis` of that pair, to share what the families derive from it as well."""
    from ..engine import surface_metrics_3d
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    if largest_component:
        scores = surface_metrics_3d(an.body(thr, True, connectivity).float(), an.gt, 0.5, thr, q)
    else:
        scores = surface_metrics_3d(an.pred, an.gt, thr, thr, q)
    for key in ("assd", "hd", "hd_percentile"):
        scores[key] = scores[key] * an.voxel
    scores["voxel_size"], scores["threshold"] = an.voxel, thr
    return scores, an.pred, an.gt


@torch.no_grad()
def reconstruction_topology_metrics(model, volume, outside, n, threshold=None, connectivity=3, grids=None):
    """Is the reconstruction one vessel tree, or a tree plus debris -> (scores, predicted grid, ground-truth grid, mask of the largest
    component of the prediction [bool, n^3]).

    A = pred >= threshold, B = gt >= threshold on the grids of `reconstruction_surface_metrics` (threshold: mean(gt) in fp32 unless
    given); L = the largest connected component of A (`connectivity` 1, 2, 3 = 6, 18, 26 neighbours; of equal sizes the first in raster
    order).  scores: n_components = K(A) and n_components_gt = K(B), the number of connected components (`engine.label_components_3d`:
    scipy.ndimage.label's result); n_pred = |A|, n_gt = |B|, n_largest = |L|; lcc_fraction = |L| / |A|, the share of the predicted vessel
    class that hangs together; dice_lcc = 2 |L & B| / (|L| + |B|), the vessel Dice after the floaters are dropped; connectivity and
    threshold.  Both ratios are formed in fp64 from integer counts.  ValueError when the threshold leaves either grid empty.  grids: as
    in `reconstruction_surface_metrics`."""
    from ..engine import components_filter, components_record
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    a, b, n_a, n_b = an.masks(thr)
    _refuse_empty("reconstruction_topology_metrics", n_a, n_b, "volume has no components")
    labels, sizes, rec_a = components_record(a.to(torch.uint8).contiguous(), connectivity)
    lcc = components_filter(labels, sizes, rec_a, largest_only=True).bool()
    rec_b = components_record(b.to(torch.uint8).contiguous(), connectivity)[2]
    k_a, n_l = (int(v) for v in rec_a[1:3].cpu())
    n_lb = int((lcc & b).sum())
    scores = {"n_components": k_a, "n_components_gt": int(rec_b[1]), "n_pred": n_a, "n_gt": n_b, "n_largest": n_l, "lcc_fraction": n_l / n_a,
              "dice_lcc": 2.0 * n_lb / (n_l + n_b), "connectivity": int(connectivity), "threshold": thr}
    return scores, an.pred, an.gt, lcc


def cldice_scores(vp, vl, sp, sl):
    """clDice (Shit et al. 2021) of two bool masks V_P, V_L and their skeletons S_P, S_L (tensors of one shape, on any device) ->
    {"cldice", "tprec", "tsens", "n_skeleton", "n_skeleton_gt"}: tprec = |S_P & V_L| / |S_P|, tsens = |S_L & V_P| / |S_L|, cldice their
    harmonic mean (0 when both are 0); integer counts, the ratios in fp64.  ValueError on an empty skeleton."""
    n_sp, n_sl = int(sp.sum()), int(sl.sum())
    if n_sp == 0 or n_sl == 0:
        empty = [name for cnt, name in ((n_sp, "pred"), (n_sl, "gt")) if cnt == 0]
        raise ValueError(f"cldice_scores: the skeleton of {' or '.join(empty)} is empty")
    tprec, tsens = int((sp & vl).sum()) / n_sp, int((sl & vp).sum()) / n_sl
    return {"cldice": 2.0 * tprec * tsens / (tprec + tsens) if tprec + tsens > 0 else 0.0, "tprec": tprec, "tsens": tsens,
            "n_skeleton": n_sp, "n_skeleton_gt": n_sl}


@torch.no_grad()
def reconstruction_centreline_metrics(model, volume, outside, n, threshold=None, largest_component=False, grids=None):
    """Does the reconstruction follow the centrelines of the true vessel tree -> (scores, predicted grid, ground-truth grid, skeleton of
    the prediction, skeleton of the ground truth [bool, n^3 each]).

    V_P = pred >= threshold, V_L = gt >= threshold on the grids of `reconstruction_topology_metrics` (threshold: mean(gt) in fp32 unless
    given); S_P, S_L = their medial curves (`engine.skeletonize_3d`; largest_component: S_P is thinned from the largest 26-connected
    component of V_P alone, `filter_components_3d(..., largest_only=True)`, the skeleton without the floaters; V_P itself stays whole).
    clDice of Shit et al. (2021): tprec = |S_P & V_L| / |S_P|, tsens = |S_L & V_P| / |S_L|, cldice = 2 tprec tsens / (tprec + tsens)
    (0 when both are 0), formed in fp64 from integer counts.  A thin branch the reconstruction loses costs tsens its whole length,
    however few voxels it had.  Also: n_skeleton, n_skeleton_gt = |S_P|, |S_L|; n_end_points, n_end_points_gt, the skeleton voxels
    with exactly one 26-neighbour in the skeleton; mean_radius, mean_radius_gt, the mean over the skeleton voxels of the mask's exact
    distance transform (`engine.distance_transform_edt_3d` of the mask that was thinned: the vessel radius along the centreline), in
    WORLD units - voxels times the grid step 2 outside / (n - 1), summed and multiplied in fp64; n_pred, n_gt, passes, passes_gt,
    voxel_size and threshold.  ValueError when the threshold leaves either mask, or either skeleton, empty.  grids: as in
    `reconstruction_surface_metrics`."""
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    vp, vl, n_p, n_l = an.masks(thr)
    _refuse_empty("reconstruction_centreline_metrics", n_p, n_l, "volume has no centreline")
    line_p, line_l = an.skeleton("pred", thr, largest_component), an.skeleton("gt", thr)
    sp, sl = line_p["skeleton"], line_l["skeleton"]
    scores = cldice_scores(vp, vl, sp, sl)                      # (thinning keeps every component: only an empty mask has an empty skeleton)
    n_sp, n_sl = scores["n_skeleton"], scores["n_skeleton_gt"]

    def ends(s):                                              # skeleton voxels with exactly one 26-neighbour: 2 voxels in their 3 x 3 x 3 box
        p = torch.nn.functional.pad(s.to(torch.int32), (1, 1, 1, 1, 1, 1))
        box = sum(p[a:a + s.shape[0], b:b + s.shape[1], c:c + s.shape[2]] for a, b, c in itertools.product(range(3), repeat=3))
        return int((s & (box == 2)).sum())

    scores.update({"n_end_points": ends(sp), "n_end_points_gt": ends(sl),
                   "mean_radius": float(line_p["dist"][sp].sum()) / n_sp * an.voxel,
                   "mean_radius_gt": float(line_l["dist"][sl].sum()) / n_sl * an.voxel,
                   "n_pred": n_p, "n_gt": n_l, "passes": line_p["skeleton_record"]["passes"], "passes_gt": line_l["skeleton_record"]["passes"],
                   "voxel_size": an.voxel, "threshold": thr})
    return scores, an.pred, an.gt, sp, sl


def graph_scores(graph_p, graph_l, rec_p, rec_l, voxel):
    """The scores of `reconstruction_graph_metrics` from two `engine.centreline_graph` results of the pruned centrelines (lengths in world
    units), the two pruning records and the voxel size: plain Python on integers and fp64."""
    out = {}
    for sfx, g, r in (("", graph_p, rec_p), ("_gt", graph_l, rec_l)):
        out.update({"n_branches" + sfx: g["n_branches"], "n_nodes" + sfx: g["n_nodes"], "n_free_ends" + sfx: g["n_free_ends"],
                    "n_spurs_removed" + sfx: r["branches"], "prune_rounds" + sfx: r["rounds"], "length" + sfx: g["total_length"],
                    "min_radius" + sfx: float("nan") if g["d2_min_all"] is None else float(g["d2_min_all"]) ** 0.5 * voxel})
    out["length_ratio"] = out["length"] / out["length_gt"] if out["length_gt"] > 0 else float("nan")
    return out


@torch.no_grad()
def reconstruction_graph_metrics(model, volume, outside, n, threshold=None, largest_component=False, prune_factor=1.0, grids=None):
    """The two centrelines read as graphs -> (scores, pruned predicted centreline, pruned true centreline, graph of the prediction, graph of
    the ground truth).

    The masks and skeletons are those of `reconstruction_centreline_metrics` (same threshold, same largest_component); `centreline_tree`
    prunes both skeletons at `prune_factor` and reads them as graphs at the grid's index_to_world.  Scores, for the prediction and with
    the suffix _gt for the ground truth, AFTER pruning: n_branches, n_nodes
    (junction nodes), n_free_ends, n_spurs_removed, prune_rounds, length (the total centreline length in WORLD units) and min_radius
    (the smallest radius along any branch, world units: voxels times the grid step; NaN without a branch); length_ratio = length /
    length_gt in fp64 (NaN when the true centreline has no step); voxel_size and threshold.  ValueError when the threshold leaves either
    mask empty."""
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    _refuse_empty("reconstruction_graph_metrics", *an.masks(thr)[2:], "volume has no centreline")
    tree_p, tree_l = an.tree("pred", thr, largest_component, prune_factor), an.tree("gt", thr, prune_factor=prune_factor)
    scores = graph_scores(tree_p["graph"], tree_l["graph"], tree_p["prune_record"], tree_l["prune_record"], an.voxel)
    scores.update(voxel_size=an.voxel, threshold=thr)
    return scores, tree_p["pruned"], tree_l["pruned"], tree_p["graph"], tree_l["graph"]


def vesselness_scores(a, b, vp, vg, ip, ig, sigmas, v_min):
    """The scores of `reconstruction_vesselness_metrics` from the two thresholded masks A, B (bool), the two vesselness volumes (float64),
    the two scale-index volumes (uint8) - tensors of one shape on any device - the sigmas and v_min -> (scores, A' = A & (Vp >= v_min)).
    Integer counts and fp64 sums; a ratio whose divisor is 0 is NaN."""
    ta, tb = a & (vp >= v_min), b & (vg >= v_min)
    n_a, n_b, n_ta, n_tb, n_both = (int(v) for v in (a.sum(), b.sum(), ta.sum(), tb.sum(), (ta & tb).sum()))
    sg = torch.tensor([float(v) for v in sigmas], dtype=torch.float64, device=a.device)
    sum_a, sum_b = float(sg[ip[ta].long()].sum()), float(sg[ig[tb].long()].sum())
    nan = float("nan")
    mean_a, mean_b = (sum_a / n_ta if n_ta else nan), (sum_b / n_tb if n_tb else nan)
    scores = {"tubular_fraction": n_ta / n_a if n_a else nan, "tubular_fraction_gt": n_tb / n_b if n_b else nan,
              "dice_tubular": 2.0 * n_both / (n_ta + n_tb) if n_ta + n_tb else nan,
              "scale_ratio": mean_a / mean_b if n_ta and n_tb and mean_b != 0 else nan, "mean_scale": mean_a, "mean_scale_gt": mean_b,
              "n_pred": n_a, "n_gt": n_b, "n_tubular": n_ta, "n_tubular_gt": n_tb, "n_tubular_both": n_both,
              "sigmas": tuple(float(v) for v in sigmas), "v_min": float(v_min)}
    return scores, ta


@torch.no_grad()
def reconstruction_vesselness_metrics(model, volume, outside, n, threshold=None, sigmas=(1, 2, 3), v_min=0.1, grids=None):
    """Are the bright voxels of the reconstruction tube-shaped -> (scores, predicted grid, ground-truth grid, tubular mask of the prediction
    [bool, n^3]).

    A = pred >= threshold, B = gt >= threshold on the grids of `reconstruction_topology_metrics` (threshold: mean(gt) in fp32 unless
    given).  Vp, Vg = `engine.frangi_3d` of the two grids (the 3-D Frangi vesselness of include/afx.h: bright ridges, `sigmas` in voxels,
    gamma per scale, so neither depends on the density scale) with the index of the scale each voxel selects.  A' = A & (Vp >= v_min),
    B' = B & (Vg >= v_min): a floater is blob-like and back-projection haze plate-like - both pass the threshold and fail the filter.
    scores: tubular_fraction = |A'| / |A|; tubular_fraction_gt = |B'| / |B|, what a perfect reconstruction would score (the wall voxels
    of a true tube fail the filter as well); dice_tubular = 2 |A' & B'| / (|A'| + |B'|); scale_ratio = the mean selected sigma over A'
    divided by the mean over B', a coarse ratio of the vessel radii (mean_scale, mean_scale_gt); the counts n_pred, n_gt, n_tubular,
    n_tubular_gt, n_tubular_both; sigmas, v_min and threshold.  The ratios are formed in fp64 from integer counts and fp64 sums; an
    empty A' or B' gives NaN for the ratios that divide by it.  ValueError when the threshold leaves A or B empty.  v_min = 0.1 is a
    default, not a validated operating point.  The mask can be fed to the component, skeleton and surface functions.
    grids: as in `reconstruction_surface_metrics`."""
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    a, b, n_a, n_b = an.masks(thr)
    _refuse_empty("reconstruction_vesselness_metrics", n_a, n_b, "volume has no tubular share")
    (vp, ip), (vg, ig) = an.frangi("pred", sigmas), an.frangi("gt", sigmas)
    scores, tubular = vesselness_scores(a, b, vp, vg, ip, ig, sigmas, v_min)
    scores["threshold"] = thr
    return scores, an.pred, an.gt, tubular


def lumen_scores(prof_p, prof_g, sum_p, sum_g):
    """The scores of `reconstruction_lumen_metrics` from the two profiles along one centreline (read back: NumPy arrays `area` and `flags`
    of P points each) and their `engine.lumen_branch_summary` results: NumPy fp64 on the host, NaN where a divisor or a set is empty."""
    nan = float("nan")
    ap, ag = np.asarray(prof_p["area"], np.float64), np.asarray(prof_g["area"], np.float64)
    ok_g = np.asarray(prof_g["flags"]) == 0
    both = ok_g & (np.asarray(prof_p["flags"]) == 0)
    n_g, n_b = int(ok_g.sum()), int(both.sum())
    out = {"n_points": int(ag.size), "n_valid_gt": n_g, "n_valid_both": n_b, "centreline_coverage": n_b / n_g if n_g else nan}
    out["lumen_area_err"] = float(np.mean(np.abs(ap[both] - ag[both]) / ag[both])) if n_b else nan
    out["mla"], out["mla_gt"] = (float(ap[both].min()), float(ag[both].min())) if n_b else (nan, nan)
    out["mla_ratio"] = out["mla"] / out["mla_gt"] if n_b and out["mla_gt"] != 0 else nan
    sp, sg = np.asarray(sum_p["area_stenosis"], np.float64), np.asarray(sum_g["area_stenosis"], np.float64)
    out["max_stenosis"] = float(sp[~np.isnan(sp)].max()) if (~np.isnan(sp)).any() else nan
    out["max_stenosis_gt"] = float(sg[~np.isnan(sg)].max()) if (~np.isnan(sg)).any() else nan
    pair = ~np.isnan(sp) & ~np.isnan(sg)
    out["stenosis_err"] = float(np.abs(sp[pair] - sg[pair]).max()) if pair.any() else nan
    return out


@torch.no_grad()
def reconstruction_lumen_metrics(model, volume, outside, n, threshold=None, prune_factor=1.0, grids=None, **profile_kw):
    """How wide is the reconstructed lumen along the TRUE centreline -> (scores, profile of the prediction, profile of the ground truth).

    The centreline is the pruned true one of `reconstruction_graph_metrics` (same threshold, prune_factor), so no branch of one graph has
    to be matched with a branch of the other.  `engine.centreline_lumen_profile` (afx_lumen_profile: include/afx.h) measures the
    ground-truth grid and the predicted grid along it at iso = threshold with `grid_index_to_world(outside, n)`; profile_kw goes to it
    (n_rays, step, r_max, half_window).  Both profiles are read back (NumPy arrays per key) and scored on the host in fp64
    (`lumen_scores`): n_points, n_valid_gt, n_valid_both (points whose cross-section is closed in both grids),
    centreline_coverage = n_valid_both / n_valid_gt, the share of the true centreline that lies inside the predicted lumen;
    lumen_area_err = the mean over the both-valid points of |A_p - A_g| / A_g; mla, mla_gt, mla_ratio: the minimal lumen areas over those
    points and their ratio; max_stenosis, max_stenosis_gt: the largest area_stenosis of `engine.lumen_branch_summary` over the branches;
    stenosis_err = the largest |S_p,b - S_g,b| over the branches with a summary on both sides; threshold.  NaN where a divisor or a set
    is empty; ValueError when either mask is empty or the true centreline has no point.  Near a bifurcation rays leak into the sibling branch: the median
    and the minimum are robust to it.  grids: as in `reconstruction_surface_metrics`."""
    from ..engine import centreline_lumen_profile, lumen_branch_summary
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    _refuse_empty("reconstruction_lumen_metrics", *an.masks(thr)[2:], "volume has no centreline")
    graph_l = an.tree("gt", thr, prune_factor=prune_factor)["graph"]
    if int(graph_l["path_voxels"].numel()) == 0:
        raise ValueError("reconstruction_lumen_metrics: the true centreline has no point at this threshold")
    profiles = []
    for x in (an.pred, an.gt):
        prof = centreline_lumen_profile(graph_l, x, an.index_to_world, thr, **profile_kw)
        profiles.append({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in prof.items()})
    scores = lumen_scores(profiles[0], profiles[1], lumen_branch_summary(profiles[0]), lumen_branch_summary(profiles[1]))
    scores["threshold"] = thr
    return scores, profiles[0], profiles[1]


def hull_scores(n_pred, n_pred_outside, n_hull, n_gt, n_both):
    """The scores of `reconstruction_hull_metrics` from five voxel counts, fp64 on the host, NaN where a divisor is 0: outside_hull =
    n_pred_outside / n_pred; dice_hull = 2 n_both / (n_hull + n_gt); hull_ratio = n_hull / n_gt."""
    nan = float("nan")
    return dict(outside_hull=float(n_pred_outside) / float(n_pred) if n_pred else nan,
                dice_hull=2.0 * float(n_both) / float(n_hull + n_gt) if n_hull + n_gt else nan,
                hull_ratio=float(n_hull) / float(n_gt) if n_gt else nan)


@torch.no_grad()
def reconstruction_hull_metrics(model, volume, outside, n, views, threshold=None, grids=None):
    """How the reconstruction stands against the visual hull of the training views -> (scores, hull mask [bool, n^3], predicted grid,
    ground-truth grid).

    The hull (`engine.visual_hull`: include/afx.h, afx_visual_hull) is taken over the n^3 points of the evaluation grids
    (`grid_index_to_world(outside, n)`), each point speaking for its voxel (radius: half the voxel diagonal), from `views` =
    engine.visual_hull_views(poses, masks, focal) of the TRAINING views.  A = pred >= threshold, B = gt >= threshold (threshold: mean(gt)
    in fp32 unless given), H = the hull.  scores (`hull_scores`, fp64 on the host from device counts): outside_hull = |A and not H| / |A|, the
    share of the reconstructed vessel that contradicts a training image - it needs no ground truth (volume=None with `threshold` given
    leaves the other two NaN); dice_hull = the vessel Dice of H against B, what silhouettes alone achieve - the reconstruction should
    beat it; hull_ratio = |H| / |B|; and the counts n_pred, n_pred_outside, n_hull, n_gt, n_hull_gt, threshold."""
    if volume is None and grids is None:
        if threshold is None:
            raise ValueError("reconstruction_hull_metrics: without the ground-truth volume the threshold must be given")
        grids = density_grid(model, outside, int(n) - 1), None
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    hull = an.hull(views)                                 # taken once per analysis, whoever asks first
    a, b, n_pred, n_gt = an.masks(thr)
    n_out, n_hull = int((a & ~hull).sum()), int(hull.sum())
    n_both = int((b & hull).sum()) if b is not None else 0
    scores = hull_scores(n_pred, n_out, n_hull if b is not None else 0, n_gt, n_both)
    scores.update(n_pred=n_pred, n_pred_outside=n_out, n_hull=n_hull, n_gt=n_gt, n_hull_gt=n_both, threshold=thr)
    return scores, hull, an.pred, an.gt


def sirt_scores(n_sirt, n_pred, n_gt, n_sirt_gt, n_pred_gt, n, sx, sg, sxx, sgg, sxg):
    """The scores of `reconstruction_sirt_metrics` from five voxel counts, the number of grid points and five fp64 sums over them (x the
    SIRT volume, g the truth: sum x, sum g, sum x x, sum g g, sum x g), fp64 on the host, NaN where a divisor is 0: dice_sirt =
    2 n_sirt_gt / (n_sirt + n_gt); dice_model = 2 n_pred_gt / (n_pred + n_gt); dice_gain = dice_model - dice_sirt; corr_sirt =
    (n sxg - sx sg) / sqrt((n sxx - sx sx) (n sgg - sg sg)), Pearson's correlation."""
    nan = float("nan")
    dice_sirt = 2.0 * float(n_sirt_gt) / float(n_sirt + n_gt) if n_sirt + n_gt else nan
    dice_model = 2.0 * float(n_pred_gt) / float(n_pred + n_gt) if n_pred + n_gt else nan
    var = (float(n) * sxx - sx * sx) * (float(n) * sgg - sg * sg)
    return dict(dice_sirt=dice_sirt, dice_model=dice_model, dice_gain=dice_model - dice_sirt,
                corr_sirt=(float(n) * sxg - sx * sg) / float(np.sqrt(var)) if var > 0 else nan)


@torch.no_grad()
def reconstruction_sirt_metrics(model, volume, outside, n, views, images, iterations=50, relax=1.0, mask=None, threshold=None, grids=None,
                                hull_views=None, tv_weight=None, tv_iterations=10):
    """How the reconstruction stands against the classical baseline, the algebraic reconstruction of the attenuation volume from the same
    training views -> (scores, SIRT volume [float64, n^3], predicted grid, ground-truth grid).

    `engine.sirt_reconstruct` (include/afx.h: afx_xray_project, afx_xray_backproject) runs `iterations` SIRT iterations at `relax`, from
    zero and clamped at zero, on the n^3 points of the evaluation grids (`grid_index_to_world(outside, n)`) from `views` =
    engine.xray_views(poses, focal, width, height, near, far, n_samples) of the TRAINING views and `images`, their line integrals
    [V, H, W] (`engine.line_integrals(I)` of transmission images).  mask: a support constraint (bool, n^3); hull_views =
    engine.visual_hull_views(...): the visual hull of these views is the mask (taken once per `GridAnalysis`; with `mask` as well,
    their intersection).  S = sirt >= threshold, A = pred >= threshold, B = gt >= threshold (threshold: mean(gt) in fp32 unless given).
    scores (`sirt_scores`, fp64 on the host from device counts and device sums): dice_sirt, the vessel Dice of S against B - what a
    classical method achieves from these views; dice_model, that of A; dice_gain = dice_model - dice_sirt; corr_sirt, Pearson's
    correlation of the SIRT volume with the truth over all grid points; and the counts n_sirt, n_pred, n_gt, n_sirt_gt, n_pred_gt,
    residual (`engine.sirt_residual_norm` of the last iteration), iterations, relax, masked (whether a mask was used), threshold.

    tv_weight (default None: plain SIRT): the reconstruction is SIRT-TV, `engine.tv_denoise_3d` (afx_tv_denoise_3d) at tv_weight and
    tv_iterations after every update, and the scores gain dice_sirt_tv and corr_sirt_tv, the two scores above of the SIRT-TV volume -
    which is the volume returned -, tv_gain = dice_sirt_tv - dice_sirt, and tv_weight, tv_iterations; dice_sirt, corr_sirt and the
    rest stay those of plain SIRT from the same views with the same mask (kept on the `GridAnalysis`: it runs once)."""
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    support = mask
    if hull_views is not None:
        support = an.hull(hull_views) if mask is None else an.hull(hull_views) & (mask != 0)
    x, history = an.sirt(views, images, iterations, relax, support)
    a, b, n_a, n_b = an.masks(thr)
    s = x >= thr
    g = an.gt.double()
    sums = torch.stack([x.sum(), g.sum(), (x * x).sum(), (g * g).sum(), (x * g).sum()]).cpu().tolist()
    n_s, n_sb, n_ab = int(s.sum()), int((s & b).sum()), int((a & b).sum())
    scores = sirt_scores(n_s, n_a, n_b, n_sb, n_ab, x.numel(), *sums)
    scores.update(n_sirt=n_s, n_pred=n_a, n_gt=n_b, n_sirt_gt=n_sb, n_pred_gt=n_ab, residual=float(history[-1]) if len(history) else float("nan"),
                  iterations=int(iterations), relax=float(relax), masked=support is not None, threshold=thr)
    if tv_weight is not None:
        x = an.sirt(views, images, iterations, relax, support, tv_weight, tv_iterations)[0]
        s = x >= thr
        sums[0], sums[2], sums[4] = torch.stack([x.sum(), (x * x).sum(), (x * g).sum()]).cpu().tolist()
        n_s, n_sb = int(s.sum()), int((s & b).sum())
        tv = sirt_scores(n_s, n_a, n_b, n_sb, n_ab, x.numel(), *sums)
        scores.update(dice_sirt_tv=tv["dice_sirt"], corr_sirt_tv=tv["corr_sirt"], tv_gain=tv["dice_sirt"] - scores["dice_sirt"],
                      n_sirt_tv=n_s, n_sirt_tv_gt=n_sb, tv_weight=float(tv_weight), tv_iterations=int(tv_iterations))
    return scores, x, an.pred, an.gt


def view_scores(vm_p, vm_g, overlap_weight=1.0):
    """The scores of `reconstruction_view_metrics` from two `engine.view_map` results over the same views, fp64 on the host:
    foreshortening_err = the mean over the views of |tree_foreshortening_p - tree_foreshortening_g|; overlap_err = the same of
    tree_overlap over the views where both are numbers (NaN without one); view_regret = the truth's whole-tree score (foreshortening +
    overlap_weight x overlap) at the prediction's best view (`engine.optimal_views`, k = 1) minus the truth's best score: >= 0, and 0
    when the reconstruction recommends the view the truth would; best_view, best_view_gt: the two indices (-1 without a view)."""
    from ..engine import optimal_views
    fp, fg = np.asarray(vm_p["tree_foreshortening"], np.float64), np.asarray(vm_g["tree_foreshortening"], np.float64)
    op, og = np.asarray(vm_p["tree_overlap"], np.float64), np.asarray(vm_g["tree_overlap"], np.float64)
    both = np.isfinite(op) & np.isfinite(og)
    best_p, _ = optimal_views(vm_p, overlap_weight=overlap_weight, k=1)
    best_g, score_g = optimal_views(vm_g, overlap_weight=overlap_weight, k=1)
    with np.errstate(invalid="ignore"):
        truth_at = fg + float(overlap_weight) * og
    nan = float("nan")
    regret = float(truth_at[best_p[0]] - score_g[0]) if best_p.size and best_g.size else nan
    return dict(foreshortening_err=float(np.abs(fp - fg).mean()) if fp.size else nan,
                overlap_err=float(np.abs(op[both] - og[both]).mean()) if both.any() else nan, view_regret=regret,
                best_view=int(best_p[0]) if best_p.size else -1, best_view_gt=int(best_g[0]) if best_g.size else -1)


@torch.no_grad()
def reconstruction_view_metrics(model, volume, outside, n, angles, img_width=100, img_height=100, focal_length=1300.0, src_pt=(0.0, 0.0, 1500.0),
                                translation=(0.0, 0.0, 0.0), threshold=None, largest_component=False, prune_factor=1.0, overlap_weight=1.0,
                                grids=None):
    """Would the reconstruction send the C-arm where the truth would -> (scores, view map of the prediction, view map of the truth).

    The two trees are the pruned centrelines of `reconstruction_graph_metrics` (same threshold, largest_component, prune_factor: with
    `grids=` a GridAnalysis nothing is thinned twice) with the radii voxel x sqrt(d2) of their own masks; the views are `angles` [V, 2]
    (theta, phi in degrees) as the evaluation sweep poses them (`engine.view_angles_records` with src_pt, focal_length, translation) on a
    detector of img_width x img_height; `engine.view_map` (afx_view_map: include/afx.h) takes both maps.  Scores: `view_scores` plus
    threshold.  A predicted centreline without a point scores NaN (its map is None); ValueError when either mask is empty or the true
    centreline has no point."""
    from ..engine import view_angles_records, view_map
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    _refuse_empty("reconstruction_view_metrics", *an.masks(thr)[2:], "volume has no centreline")
    rec = view_angles_records(angles, src_pt, float(focal_length), translation)
    maps = []
    for side, lc in (("gt", False), ("pred", largest_component)):
        tree = an.tree(side, thr, lc, prune_factor)
        if int(tree["graph"]["path_voxels"].numel()) == 0:
            if side == "gt":
                raise ValueError("reconstruction_view_metrics: the true centreline has no point at this threshold")
            maps.append(None)
            continue
        maps.append(view_map(tree["graph"], rec, int(img_width), int(img_height), index_to_world=an.index_to_world, d2=tree["d2"],
                             voxel_size=an.voxel))
    maps.reverse()
    nan = float("nan")
    scores = dict(foreshortening_err=nan, overlap_err=nan, view_regret=nan, best_view=-1, best_view_gt=-1) if maps[0] is None else \
        view_scores(maps[0], maps[1], overlap_weight)
    scores["threshold"] = thr
    return scores, maps[0], maps[1]


@torch.no_grad()
def reconstruction_pose_metrics(model, volume, outside, n, views, threshold=None, largest_component=False, prune_factor=1.0, iterations=20,
                                trunc=8.0, dof="all", search=None, grids=None):
    """Do the training poses fit the silhouettes of their views, judged by the reconstruction alone -> (scores, `engine.register_poses`'
    result or None).

    The points are the pruned predicted centreline of `reconstruction_graph_metrics` (same threshold, largest_component, prune_factor:
    with `grids=` a GridAnalysis nothing is thinned twice) with the radii voxel x sqrt(d2) of its mask; `views` = engine.pose_views(poses,
    masks, focal) of the training views.  Scores: chamfer = the mean over the views of sum w r / sum w in pixels (the one-sided residual
    truncated at `trunc`: a point inside its silhouette costs nothing), chamfer_refined the same after `engine.register_poses`
    (iterations, trunc, dof, search), pose_shift the mean pixel displacement of the points between the given and the refined poses,
    plus threshold and n_points.  No ground truth is read: volume=None works, and then needs `threshold` (None is mean(gt)).  A
    predicted centreline without a point scores NaN."""
    from ..engine import centreline_register_poses
    if volume is None and not isinstance(grids, GridAnalysis):
        if threshold is None:
            raise ValueError("reconstruction_pose_metrics: without a ground-truth volume the threshold must be given")
        grids = GridAnalysis(density_grid(model, outside, int(n) - 1) if grids is None else grids[0], None, outside, n)
    if isinstance(grids, GridAnalysis) and grids.gt is None and threshold is None:
        raise ValueError("reconstruction_pose_metrics: without a ground-truth volume the threshold must be given")
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    tree = an.tree("pred", thr, largest_component, prune_factor)
    n_points = int(tree["graph"]["path_voxels"].numel())
    nan = float("nan")
    if n_points == 0:
        return dict(chamfer=nan, chamfer_refined=nan, pose_shift=nan, threshold=thr, n_points=0), None
    reg = centreline_register_poses(tree["graph"], views, index_to_world=an.index_to_world, d2=tree["d2"], voxel_size=an.voxel,
                                    iterations=iterations, trunc=trunc, dof=dof, search=search)
    scores = dict(chamfer=float(np.mean(reg["mean_residual_before"])), chamfer_refined=float(np.mean(reg["mean_residual_after"])),
                  pose_shift=float(np.mean(reg["shift_px"])), threshold=thr, n_points=n_points)
    return scores, reg


def branch_scores(counts, cover, n_branches, lengths, site_label, d2_offset, d2_true, d2_pred, found_at=0.5):
    """The table and the scores of `reconstruction_branch_metrics` from what the device counted, fp64 NumPy on the host -> (scores,
    table).  counts, cover: integer [B + K + 1, 4] rows of afx_label_overlap_3d (cover: the call without an index, so its column 0 is
    the label's own centreline voxels and column 1 those of them in A); lengths [B]; site_label, d2_offset, d2_true, d2_pred: one entry
    per voxel of the true centreline in raster order - its label, the squared distance to the predicted centreline, the true mask's
    squared EDT there, and the predicted mask's squared EDT at the nearest predicted centreline voxel (d2_offset 0xffffffff: there is
    no predicted centreline, the three means are NaN).  A ratio whose divisor is 0 is NaN."""
    nan = float("nan")
    counts, cover = np.asarray(counts, np.int64), np.asarray(cover, np.int64)
    rows, nb = counts.shape[0] - 1, int(n_branches)
    n_pred, n_gt, n_both = (counts[1:, c].astype(np.float64) for c in (1, 2, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        table = {"label": np.arange(1, rows + 1), "kind": np.array(["branch"] * nb + ["junction"] * (rows - nb), dtype=object),
                 "n_pred": counts[1:, 1].copy(), "n_gt": counts[1:, 2].copy(), "n_both": counts[1:, 3].copy(),
                 "dice": np.where(n_pred + n_gt > 0, 2.0 * n_both / (n_pred + n_gt), nan),
                 "sensitivity": np.where(n_gt > 0, n_both / n_gt, nan), "precision": np.where(n_pred > 0, n_both / n_pred, nan),
                 "coverage": np.where(cover[1:, 0] > 0, cover[1:, 1].astype(np.float64) / cover[1:, 0].astype(np.float64), nan),
                 "length": np.concatenate([np.asarray(lengths, np.float64).reshape(-1)[:nb], np.zeros(rows - nb)])}
    site_label = np.asarray(site_label, np.int64)
    have_pred = site_label.size > 0 and not (np.asarray(d2_offset, np.int64) == 0xffffffff).any()
    means = {"offset": d2_offset, "radius_true": d2_true, "radius_pred": d2_pred}
    for key, d2 in means.items():
        col = np.full(rows, nan)
        if have_pred or key == "radius_true":
            root = np.sqrt(np.asarray(d2, np.int64).astype(np.float64))
            for l in range(1, rows + 1):
                sel = site_label == l
                if sel.any():
                    col[l - 1] = float(np.mean(root[sel]))
        table[key] = col
    found = np.zeros(rows, bool)
    found[:nb] = table["coverage"][:nb] >= float(found_at)
    table["found"] = found
    union = counts[:, 1] + counts[:, 2] - counts[:, 3]
    length, f = table["length"][:nb], found[:nb]
    rt, rp = table["radius_true"][:nb][f], table["radius_pred"][:nb][f]
    ok = rt > 0
    total = found_length = 0.0                                # added up branch after branch
    for x, hit in zip(length.tolist(), f.tolist()):
        total, found_length = total + x, found_length + (x if hit else 0.0)
    scores = dict(branch_recall=float(f.sum()) / nb if nb else nan,
                  branch_recall_length=found_length / total if nb and total > 0 else nan,
                  worst_branch_dice=float(np.min(table["dice"][:nb])) if nb else nan,
                  branch_radius_err=float(np.mean(np.abs(rp[ok] - rt[ok]) / rt[ok])) if ok.any() else nan,
                  unassigned=float(union[0]) / float(union.sum()) if union.sum() > 0 else nan,
                  n_branches=nb, n_junctions=rows - nb, n_found=int(f.sum()))
    return scores, table


@torch.no_grad()
def reconstruction_branch_metrics(model, volume, outside, n, threshold=None, largest_component=False, prune_factor=1.0, max_distance=None,
                                  found_at=0.5, grids=None):
    """Which branch was lost, which is too thin -> (scores, table, territories).

    The masks and both pruned centrelines are those of `reconstruction_graph_metrics` (same threshold, largest_component, prune_factor:
    with `grids=` a GridAnalysis nothing is computed twice).  The voxels of the TRUE pruned centreline are the sites of a feature
    transform (`engine.branch_territories`: branch b carries label b, junction node k label B + k); every voxel of A (the prediction's
    mask) or B (the truth's) belongs to the territory of the site nearest to it (ties to the lowest index), a voxel farther than
    `max_distance` voxels from the true centreline to row 0.  One counting call (afx_label_overlap_3d) gives n_pred, n_gt and n_both per
    territory, from which the host takes dice, sensitivity and precision in fp64; a second one without an index gives coverage, the
    share of a branch's own centreline voxels that lie in A; length is the graph's (world units; 0 for a junction row).  A second
    feature transform, of the PREDICTED pruned centreline, read at the true centreline's voxels, gives per row offset (the mean
    distance to the predicted centreline, voxels), radius_true (the mean sqrt(d2) of B along the row) and radius_pred (the mean sqrt(d2)
    of A at the nearest predicted centreline voxel); NaN without a predicted centreline.  table: one entry per branch, then per junction
    (`branch_scores`).  scores: branch_recall = the share of true branches with coverage >= found_at, branch_recall_length the same
    weighted by length, worst_branch_dice = the minimum over the true branches, branch_radius_err = the mean over the found branches of
    |radius_pred - radius_true| / radius_true (NaN when none is found), unassigned = row 0's share of A or B, n_branches, n_junctions,
    n_found, threshold, voxel_size, found_at.  ValueError when the threshold leaves either mask empty."""
    from ..engine import branch_territories, feature_transform_record, territory_overlap
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    a_all, b, n_pred, n_gt = an.masks(thr)
    _refuse_empty("reconstruction_branch_metrics", n_pred, n_gt, "volume has no centreline")
    a = an.body(thr, largest_component)
    tree_p, tree_l = an.tree("pred", thr, largest_component, prune_factor), an.tree("gt", thr, prune_factor=prune_factor)
    graph = tree_l["graph"]
    terr = branch_territories(graph, max_distance)
    counts = territory_overlap(terr, a, b)
    cover = territory_overlap(terr, a, sites_only=True)
    d2_off, nearest_p = feature_transform_record((tree_p["pruned"] != 0).to(torch.uint8).contiguous())
    labels = terr["labels"].reshape(-1)
    vox = torch.nonzero(labels, as_tuple=False).reshape(-1)                         # the true centreline's voxels in raster order
    near = nearest_p.reshape(-1)[vox].to(torch.int64)
    u32 = lambda t: (t.to(torch.int64) & 0xffffffff).cpu().numpy()
    d2_pred_at = tree_p["d2"].reshape(-1)[near.clamp(min=0)]
    scores, table = branch_scores(counts.cpu().numpy(), cover.cpu().numpy(), terr["n_branches"], graph["length"].cpu().numpy(),
                                  labels[vox].cpu().numpy(), u32(d2_off.reshape(-1)[vox]), u32(tree_l["d2"].reshape(-1)[vox]), u32(d2_pred_at),
                                  found_at)
    scores.update(threshold=thr, voxel_size=an.voxel, found_at=float(found_at))
    return scores, table, terr


def cpr_scores(images_p, images_g):
    """The scores of `reconstruction_cpr_metrics` from the two image stacks [A, P, K] (read back: NumPy fp64) but for the SSIM, NumPy fp64
    on the host -> (scores, the two stacks as they are compared).  Both stacks are divided by the largest value of the truth's and
    clamped to [0, 1]; cpr_psnr = -10 log10(mean((p - g)^2)) over all angles (data range 1; inf when the stacks agree); cpr_corr =
    Pearson's correlation over all pixels (NaN when either stack is constant).  A truth without a positive value scores NaN."""
    nan = float("nan")
    # C-contiguous copies: NumPy's sums run pairwise over the memory order, so a transposed view of the same numbers may round differently
    p, g = np.ascontiguousarray(images_p, np.float64), np.ascontiguousarray(images_g, np.float64)
    top = float(g.max()) if g.size else 0.0
    if not top > 0.0:
        return {"cpr_psnr": nan, "cpr_corr": nan}, p, g
    p, g = np.clip(p / top, 0.0, 1.0), np.clip(g / top, 0.0, 1.0)
    mse = float(np.mean((p - g) ** 2))
    dp, dg = p - p.mean(), g - g.mean()
    den = float(np.sqrt((dp * dp).sum() * (dg * dg).sum()))
    with np.errstate(divide="ignore"):
        return {"cpr_psnr": float(-10.0 * np.log10(mse)), "cpr_corr": float((dp * dg).sum() / den) if den > 0 else nan}, p, g


@torch.no_grad()
def reconstruction_cpr_metrics(model, volume, outside, n, threshold=None, angles=(0.0, 45.0, 90.0, 135.0), half_width=16, prune_factor=1.0,
                               smooth_passes=8, grids=None):
    """Does the straightened vessel look like the true one -> (scores, image stack of the prediction, of the truth, the path).

    The path is the main path (`engine.centreline_main_path`: from the ostium side to the farthest end) of the pruned TRUE centreline of
    `reconstruction_graph_metrics` (same threshold, prune_factor), so no branch of one graph has to be matched with a branch of the
    other; it is smoothed (`engine.polyline_smooth`, smooth_passes) and resampled at the grid step (`engine.polyline_resample`).
    `engine.cpr_images` (afx_reformat_planes: include/afx.h) takes the longitudinal images of the predicted and of the true grid along it
    at `angles` (degrees), K = 2 half_width + 1 samples half a grid step apart.  Both stacks [A, P, K] are read back and scored on the
    host (`cpr_scores`): cpr_psnr, cpr_corr, and cpr_ssim = the mean over the angles of `engine.ssim` of the normalised images; n_rows =
    P, path_length (the graph length of the path, world units), path_share = path_length / the total centreline length, threshold.
    NaN where a divisor is empty.  ValueError when either mask is empty, the true centreline has no free end, or the path has fewer
    than CPR_MIN_ROWS rows (or K is below it).  grids: as in `reconstruction_surface_metrics`."""
    from ..engine import cpr_images, centreline_main_path, polyline_resample, polyline_smooth, ssim
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    _refuse_empty("reconstruction_cpr_metrics", *an.masks(thr)[2:], "volume has no centreline")
    if 2 * int(half_width) + 1 < CPR_MIN_ROWS:
        raise ValueError(f"reconstruction_cpr_metrics: half_width = {half_width} gives images narrower than {CPR_MIN_ROWS} samples")
    tree = an.tree("gt", thr, prune_factor=prune_factor)
    path = centreline_main_path(tree["graph"], an.index_to_world, d2=tree["d2"])
    points = polyline_resample(polyline_smooth(path["points"], smooth_passes), an.voxel)
    if len(points) < CPR_MIN_ROWS:
        raise ValueError(f"reconstruction_cpr_metrics: the main path has {len(points)} rows, the SSIM needs {CPR_MIN_ROWS}")
    stacks = [cpr_images(x, points, an.index_to_world, angles, half_width)["images"].cpu().numpy() for x in (an.pred, an.gt)]
    scores, p, g = cpr_scores(*stacks)
    scores["cpr_ssim"] = float("nan")
    if scores["cpr_psnr"] == scores["cpr_psnr"]:
        dev = an.pred.device
        scores["cpr_ssim"] = float(ssim(torch.from_numpy(p).to(dev), torch.from_numpy(g).to(dev)).mean())
    total = float(tree["graph"]["total_length"])
    scores.update(n_rows=len(points), path_length=path["length"], path_share=path["length"] / total if total > 0 else float("nan"), threshold=thr)
    return scores, stacks[0], stacks[1], dict(path, resampled=points)


def centreline_polylines(graph, d2, index_to_world, voxel_size=1.0):
    """An `engine.centreline_graph` result as polylines -> (points float64 [P, 3] in world coordinates, offsets int64 [B + 1], radius
    float64 [P] = voxel_size x sqrt(d2)): branch b is points[offsets[b]:offsets[b + 1]] in path order; what `mesh_io.write_vtk_polylines`
    takes.  Junction voxels belong to no branch and are not listed.  Host arithmetic in fp64."""
    from ..engine import centreline_world_points
    points, offsets = centreline_world_points(graph, index_to_world)
    vox = graph["path_voxels"].cpu().numpy().astype(np.int64)
    dd = (d2.reshape(-1).cpu().numpy().astype(np.int64) & 0xffffffff)[vox]
    return points, offsets, np.sqrt(dd.astype(np.float64)) * float(voxel_size)


def grid_index_to_world(outside, n):
    """The index-to-world map of the n^3 evaluation grids (density_grid, ground_truth_grid) as afx_isosurface_3d takes it, 12 numbers
    (rows m[r][0..2], o[r]): index (i0, i1, i2) lies at (t[i1], t[i0], t[i2]), t[m] = m * (2 outside / (n - 1)) - outside (np.meshgrid's
    'xy' order).  The first two axes are exchanged: det(m) < 0."""
    step, lo = 2.0 * float(outside) / (int(n) - 1), -float(outside)
    return (0.0, step, 0.0, lo, step, 0.0, 0.0, lo, 0.0, 0.0, step, lo)


def _grid_mesh(x, iso, outside, n):
    """(vertices, triangles, info) of the capped surface {x = iso} of an n^3 evaluation grid in world coordinates; info with its area
    and enclosed volume (fp64, about the middle of the mesh's bounding box)."""
    from ..engine import extract_isosurface, mesh_measures
    vertices, triangles, info = extract_isosurface(x, iso, grid_index_to_world(outside, n), cap=True, fill=0.0)
    if info["T"]:
        info.update(mesh_measures(vertices, triangles))
    else:
        info.update(area=0.0, volume=0.0)
    return vertices, triangles, info


@torch.no_grad()
def reconstruction_mesh(model, volume, outside, n, threshold=None, largest_component=False, connectivity=3, grids=None):
    """The reconstructed vessel as a surface -> (vertices float32 [V, 3], triangles int32 [T, 3], info, predicted grid, ground-truth grid).

    The mesh of {pred >= threshold} on the n^3 grid of `reconstruction_metrics`, in WORLD coordinates (`grid_index_to_world`), welded,
    canonically numbered and wound so that the normals point out of the vessel (`engine.extract_isosurface`: marching tetrahedra on
    the Kuhn split).  threshold: mean(gt) in fp32 unless given; it must be positive - the surface is capped with one layer of zero
    density around the grid, so it is closed where the vessel leaves the grid.  largest_component: the mesh of the largest connected
    component alone (`filter_components_3d`'s mask, `connectivity` 1, 2, 3 = 6, 18, 26 neighbours, meshed at 0.5: its surface runs
    half-way between the voxels).  info: V, T, E, B, n22, euler = V - E + T, area and volume (world units, fp64), threshold.  The surface
    is that of the piecewise-linear interpolant, which joins a voxel to 14 neighbours: euler is not the Euler number of the
    26-connected mask.  An empty mesh (nothing reaches the threshold) has V = T = 0.  grids: as in `reconstruction_surface_metrics`."""
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    vertices, triangles, info = an.mesh("pred", thr, largest_component, connectivity)
    return vertices, triangles, dict(info, threshold=thr), an.pred, an.gt


@torch.no_grad()
def reconstruction_mesh_metrics(model, volume, outside, n, threshold=None, largest_component=False, connectivity=3, grids=None):
    """The reconstruction and the truth measured as surfaces -> (scores, predicted grid, ground-truth grid).

    Both grids are meshed at `threshold` as in `reconstruction_mesh` (largest_component filters the prediction only).  scores: area,
    volume (world units, fp64), euler, n_vertices, n_triangles, n_edges of the prediction, the same with the suffix _gt of the truth,
    volume_ratio = volume / volume_gt and area_ratio = area / area_gt (fp64), threshold and voxel_size.  ValueError when either mesh
    is empty."""
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    info, info_gt = an.mesh("pred", thr, largest_component, connectivity)[2], an.mesh("gt", thr)[2]
    _refuse_empty("reconstruction_mesh_metrics", info["T"], info_gt["T"], "mesh has no measures")
    scores = {}
    for suffix, i in (("", info), ("_gt", info_gt)):
        scores.update({"area" + suffix: i["area"], "volume" + suffix: i["volume"], "euler" + suffix: i["euler"], "n_vertices" + suffix: i["V"],
                       "n_triangles" + suffix: i["T"], "n_edges" + suffix: i["E"]})
    scores.update(volume_ratio=scores["volume"] / scores["volume_gt"], area_ratio=scores["area"] / scores["area_gt"], threshold=thr,
                  voxel_size=an.voxel)
    return scores, an.pred, an.gt


@torch.no_grad()
def reconstruction_mesh_distance_metrics(model, volume, outside, n, threshold=None, q=95.0, largest_component=False, grids=None):
    """How far the reconstructed surface lies from the true one, measured on the meshes -> (scores, predicted grid, ground-truth grid).

    Both grids are meshed as `reconstruction_mesh` meshes them, the truth at the same threshold (largest_component filters the
    prediction only); each mesh's vertices are measured against the other's triangles (`engine.mesh_point_distance`: the exact
    point-to-triangle distance, fp32 in world units).  scores, by medpy's formulas: assd = the mean of the two directed means, hd =
    the maximum of the two directed maxima, hd_percentile = the q-th percentile of the two directed sets together (sums and the
    percentile in fp64); n_vertices, n_vertices_gt, threshold, q.  An empty mesh on either side gives NaN scores, as the voxel scores
    do."""
    from ..engine import mesh_point_distance
    if not 0.0 <= float(q) <= 100.0:
        raise ValueError(f"reconstruction_mesh_distance_metrics: q = {q} must lie in [0, 100]")
    an, thr = _analysis(model, volume, outside, n, grids, threshold)
    vertices, triangles, info = an.mesh("pred", thr, largest_component)
    vertices_gt, triangles_gt, info_gt = an.mesh("gt", thr)
    scores = {"assd": float("nan"), "hd": float("nan"), "hd_percentile": float("nan"), "n_vertices": info["V"], "n_vertices_gt": info_gt["V"],
              "threshold": thr, "q": float(q)}
    if info["T"] and info_gt["T"]:
        there = mesh_point_distance(vertices, vertices_gt, triangles_gt).double()
        back = mesh_point_distance(vertices_gt, vertices, triangles).double()
        scores["assd"] = float((there.mean() + back.mean()) / 2.0)
        scores["hd"] = float(torch.maximum(there.max(), back.max()))
        scores["hd_percentile"] = float(torch.quantile(torch.cat([there, back]), float(q) / 100.0))
    return scores, an.pred, an.gt


def _reference_scores(*args, **kw):
    dice, dot = reconstruction_metrics(*args, **kw)[:2]
    return ({"dice_3d": dice, "dot_3d": dot},)


# the whole-volume columns of evaluation_sweep in table order: (column names, the function whose first result holds the scores, the
# score behind each column); the hull family takes the training views as a fifth argument
_VOLUME_FAMILIES = (
    (METRICS[-2:], _reference_scores, ("dice_3d", "dot_3d")),
    (SURFACE_METRICS, reconstruction_surface_metrics, ("dice_vessel", "assd", "hd", "hd_percentile")),
    (TOPOLOGY_METRICS, reconstruction_topology_metrics, ("n_components", "lcc_fraction", "dice_lcc")),
    (CENTRELINE_METRICS, reconstruction_centreline_metrics, ("cldice", "tprec", "tsens")),
    (MESH_METRICS, reconstruction_mesh_metrics, ("volume_ratio", "area_ratio", "euler")),
    (MESH_DISTANCE_METRICS, reconstruction_mesh_distance_metrics, ("assd", "hd", "hd_percentile")),
    (GRAPH_METRICS, reconstruction_graph_metrics, ("n_branches", "n_nodes", "length_ratio")),
    (VESSELNESS_METRICS, reconstruction_vesselness_metrics, ("tubular_fraction", "dice_tubular", "scale_ratio")),
    (LUMEN_METRICS, reconstruction_lumen_metrics, ("lumen_area_err", "mla_ratio", "stenosis_err")),
    (HULL_METRICS, reconstruction_hull_metrics, ("outside_hull", "dice_hull", "hull_ratio")),
    (SIRT_METRICS, reconstruction_sirt_metrics, ("dice_sirt", "dice_gain", "corr_sirt")),
    (SIRT_TV_METRICS, reconstruction_sirt_metrics, ("dice_sirt_tv", "tv_gain", "corr_sirt_tv")),
)


@torch.no_grad()
def ground_truth_sweep(volume, angles, img_width, img_height, focal_length, src_pt, depth_values, translation=(0.0, 0.0, 0.0),
                       type_ct=True):
    """Ground-truth projections of a `VoxelVolume` for every view of the sweep: one afx_project_volume launch, rays generated
    in the kernel from the poses (helpers.py:192-224 per view upstream)."""
    from ..engine import project_volume
    dev = volume.values.device
    poses = _poses(angles, src_pt, translation, dev)
    img = project_volume(volume.values, volume.origin, volume.spacing, volume.fill_value, depth_values.to(dev, torch.float32),
                         poses=poses, width=int(img_width), height=int(img_height), focal=float(focal_length), type_ct=type_ct)
    return img.view(len(angles), int(img_height), int(img_width))
