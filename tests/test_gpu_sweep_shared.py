"""The shared analysis of the evaluation sweep (sweep.GridAnalysis, sweep.centreline_tree): one sweep that asks for every family of
whole-volume scores gives, column by column, what each family's stand-alone function gives, evaluates the two grids once and runs every
shared stage once per grid; the cache follows the arguments; the driver's exports do not depend on who evaluated the density grid.  The
numbers themselves are pinned against NumPy in each family's own test file (run with -m gpu on an MI355X)."""
import math

import pytest
import torch

from test_gpu_sweep_metrics import DEV, _sweep_setup

pytestmark = pytest.mark.gpu
N, OUTSIDE = 33, 100.0
# column -> (family, key of its scores), written out here so that the sweep's own table is what is under test
COLUMNS = {"DICE 3D": ("metrics", "dice_3d"), "DOT 3D": ("metrics", "dot_3d"),
           "DICE 3D VESSEL": ("surface", "dice_vessel"), "ASSD 3D": ("surface", "assd"), "HD 3D": ("surface", "hd"),
           "HD95 3D": ("surface", "hd_percentile"),
           "COMPONENTS 3D": ("topology", "n_components"), "LCC FRACTION 3D": ("topology", "lcc_fraction"), "DICE 3D LCC": ("topology", "dice_lcc"),
           "CLDICE 3D": ("centreline", "cldice"), "TPREC 3D": ("centreline", "tprec"), "TSENS 3D": ("centreline", "tsens"),
           "VOLUME RATIO 3D": ("mesh", "volume_ratio"), "AREA RATIO 3D": ("mesh", "area_ratio"), "EULER 3D": ("mesh", "euler"),
           "ASSD MESH": ("mesh_distance", "assd"), "HD MESH": ("mesh_distance", "hd"), "HD95 MESH": ("mesh_distance", "hd_percentile"),
           "BRANCHES 3D": ("graph", "n_branches"), "JUNCTIONS 3D": ("graph", "n_nodes"), "LENGTH RATIO 3D": ("graph", "length_ratio"),
           "TUBULAR FRACTION 3D": ("vesselness", "tubular_fraction"), "DICE 3D TUBULAR": ("vesselness", "dice_tubular"),
           "SCALE RATIO 3D": ("vesselness", "scale_ratio"),
           "LUMEN AREA ERR 3D": ("lumen", "lumen_area_err"), "MLA RATIO 3D": ("lumen", "mla_ratio"), "STENOSIS ERR 3D": ("lumen", "stenosis_err"),
           "OUTSIDE HULL 3D": ("hull", "outside_hull"), "DICE 3D HULL": ("hull", "dice_hull"), "HULL RATIO 3D": ("hull", "hull_ratio")}


def _same(a, b):
    """== with NaN equal to NaN, through dicts and sequences."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _families(sweep, m, vol, views, grids=None, order=None):
    """The scores dict of every family, the families called in `order`."""
    def two(*args, **kw):
        dice, dot = sweep.reconstruction_metrics(*args, **kw)[:2]
        return ({"dice_3d": dice, "dot_3d": dot},)
    calls = {"metrics": two, "surface": sweep.reconstruction_surface_metrics, "topology": sweep.reconstruction_topology_metrics,
             "centreline": sweep.reconstruction_centreline_metrics, "mesh": sweep.reconstruction_mesh_metrics,
             "mesh_distance": sweep.reconstruction_mesh_distance_metrics, "graph": sweep.reconstruction_graph_metrics,
             "vesselness": sweep.reconstruction_vesselness_metrics, "lumen": sweep.reconstruction_lumen_metrics,
             "hull": lambda *a, **kw: sweep.reconstruction_hull_metrics(*a, views, **kw)}
    return {name: calls[name](m, vol, OUTSIDE, N, grids=grids)[0] for name in (order or calls)}


@pytest.fixture(scope="module")
def shared(golden):
    """The 3 x 3 sweep over the G10 volume, the views of test_gpu_visual_hull.py::test_hull_metrics and every family's stand-alone scores."""
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd.visualization import sweep
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    poses = sweep._poses(angles, geo[3], (0.0, 0.0, 0.0), DEV)
    views = engine.visual_hull_views(poses, torch.ones(len(angles), geo[1], geo[0], dtype=torch.bool, device=DEV), geo[2])
    alone = _families(sweep, m, vol, views)
    assert alone["centreline"]["n_skeleton"] > 0 and alone["lumen"]["n_points"] > 0 and alone["graph"]["n_spurs_removed"] > 0
    return dict(sweep=sweep, engine=engine, vol=vol, m=m, gt=gt, angles=angles, geo=geo, views=views, alone=alone)


def _counted(monkeypatch, owner, names, calls):
    for name in names:
        def counting(*args, _real=getattr(owner, name), _name=name, **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*args, **kw)
        monkeypatch.setattr(owner, name, counting)


def test_one_sweep_serves_every_family_from_one_analysis(shared, monkeypatch):
    sweep, s = shared["sweep"], shared
    calls = {}
    _counted(monkeypatch, sweep, ["density_grid"], calls)
    _counted(monkeypatch, s["engine"], ["volume_grid", "skeletonize_3d", "distance_transform_edt_3d", "prune_spurs", "centreline_graph",
                                        "extract_isosurface", "frangi_3d", "visual_hull"], calls)
    df, _ = sweep.evaluation_sweep(s["m"], s["gt"], s["angles"], *s["geo"], metrics=["PSNR"] + list(COLUMNS), volume=s["vol"],
                                   volume_outside=OUTSIDE, volume_points=N, hull_views=s["views"])
    monkeypatch.undo()
    assert set(COLUMNS) == set(sweep.METRICS[-2:] + sweep._ALL_VOLUME_METRICS + sweep.HULL_METRICS)      # every whole-volume column there is
    assert list(df.columns[-len(COLUMNS):]) == list(COLUMNS)
    for col, (family, key) in COLUMNS.items():
        want = s["alone"][family][key]
        assert len(df[col]) == len(s["angles"]) and all(_same(v, want) for v in df[col].tolist()), (col, df[col][0], want)
    print(f"calls of one sweep: {calls}")
    assert calls == {"density_grid": 1, "volume_grid": 1, "skeletonize_3d": 2, "distance_transform_edt_3d": 2, "prune_spurs": 2,
                     "centreline_graph": 2, "extract_isosurface": 2, "frangi_3d": 2, "visual_hull": 1}


def test_shared_analysis_does_not_depend_on_the_order_of_calls(shared):
    sweep, s = shared["sweep"], shared
    for order in (list(reversed(list(s["alone"]))), ["lumen", "mesh_distance", "centreline", "hull", "graph", "metrics", "mesh", "vesselness",
                                                     "surface", "topology"]):
        an = sweep.GridAnalysis(*sweep._reconstruction_grids(s["m"], s["vol"], OUTSIDE, N), OUTSIDE, N)
        got = _families(sweep, s["m"], s["vol"], s["views"], grids=an, order=order)
        for name in order:
            assert _same(got[name], s["alone"][name]), (name, got[name], s["alone"][name])


def test_cache_keys_follow_the_arguments(shared):
    sweep, s = shared["sweep"], shared
    grids = sweep._reconstruction_grids(s["m"], s["vol"], OUTSIDE, N)
    thr = float(torch.mean(grids[1]))
    other = dict(largest_component=True, prune_factor=2.0, threshold=thr * 0.5)
    an = sweep.GridAnalysis(*grids, OUTSIDE, N)
    first = sweep.reconstruction_graph_metrics(s["m"], s["vol"], OUTSIDE, N, grids=an)
    after = sweep.reconstruction_graph_metrics(s["m"], s["vol"], OUTSIDE, N, grids=an, **other)
    fresh = sweep.reconstruction_graph_metrics(s["m"], s["vol"], OUTSIDE, N, grids=sweep.GridAnalysis(*grids, OUTSIDE, N), **other)
    assert _same(first[0], s["alone"]["graph"])
    assert _same(after[0], fresh[0]) and not _same(after[0], first[0])
    assert torch.equal(after[1], fresh[1]) and torch.equal(after[2], fresh[2]) and not torch.equal(after[1], first[1])
    again = sweep.reconstruction_graph_metrics(s["m"], s["vol"], OUTSIDE, N, grids=an)      # and the first entry is still the first
    assert _same(again[0], first[0]) and torch.equal(again[1], first[1])
    with pytest.raises(ValueError, match="points per axis"):
        sweep.reconstruction_graph_metrics(s["m"], s["vol"], OUTSIDE, N - 8, grids=an)


def test_driver_exports_take_an_evaluated_grid(shared, tmp_path):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import save_centreline, save_lumen, save_mesh
    from nerf_for_angiography_amd.render import density_grid
    s = shared
    thr = s["alone"]["graph"]["threshold"]
    grid = density_grid(s["m"], OUTSIDE, N - 1)
    for save, name in ((save_centreline, "centreline.vtk"), (save_lumen, "lumen.csv"), (save_mesh, "mesh.stl")):
        path = tmp_path / name
        info = save(s["m"], OUTSIDE, N, thr, str(path))
        written = path.read_bytes()
        path.unlink()
        info_grid = save(s["m"], OUTSIDE, N, thr, str(path), grid=grid)
        assert path.read_bytes() == written and len(written) > 200, name
        assert _same(info_grid, info), (name, info_grid, info)
