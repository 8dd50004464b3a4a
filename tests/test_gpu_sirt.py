"""afx_xray_project, afx_xray_backproject and engine.sirt_reconstruct against the NumPy restatement tests/sirt_reference.py: every comparison
is on the fp64 bits.  Also the sweep's SIRT columns and the driver's --save_sirt (run with -m gpu on an MI355X)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sirt_reference as sr
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


def _engine():
    from nerf_for_angiography_amd import engine
    return engine


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same_bits(device_tensor, array):
    """fp64 bits equal (NaN patterns and the sign of zero included)."""
    return np.array_equal(device_tensor.cpu().numpy().view(np.int64), np.ascontiguousarray(array, dtype=np.float64).view(np.int64))


# ---- the two lattices ----
# general: anisotropic, sheared, offset; 9 x 12 x 7 = 756 points and 3 x 10 x 13 = 390 rays: no multiple of 64 or 256
GENERAL = dict(shape=(9, 12, 7), a12=np.array([2.0, 0.3, 0.0, -9.0, 0.0, 1.5, 0.2, -8.0, 0.1, 0.0, 2.5, -7.0]), width=13, height=10,
               near=38.0, far=83.0, n_samples=17)
# aligned: the identity lattice, points at the integers
ALIGNED = dict(shape=(6, 8, 5), a12=np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]), width=12, height=8, near=40.0, far=75.0, n_samples=35)


def _general_poses():
    """(poses, focal): an oblique view of the whole lattice; a view from close by that looks past a corner, so that many rays miss the
    lattice; a view whose source lies in the plane of the lattice face i = 0 with the camera's y axis normal to it - the detector row
    iw = H / 2 runs inside that face (to rounding: the samples flip in and out of 0 <= g_0 by the last bits) and crosses its edges."""
    a = GENERAL["a12"].reshape(3, 4)
    centre = a[:, :3] @ ((np.asarray(GENERAL["shape"]) - 1) / 2.0) + a[:, 3]
    oblique = sr.look_at_pose(centre + 60.0 * np.array([0.5, 0.35, 0.79]) / np.linalg.norm([0.5, 0.35, 0.79]), target=centre)
    corner = a[:, :3] @ np.array([8.0, 11.0, 6.0]) + a[:, 3]
    close = sr.look_at_pose(corner + np.array([18.0, 22.0, 30.0]), target=corner + np.array([9.0, -2.0, 1.0]))
    col1, col2 = a[:, 1], a[:, 2]
    normal = np.cross(col1, col2) / np.linalg.norm(np.cross(col1, col2))
    face_centre = a[:, :3] @ np.array([0.0, 5.5, 3.0]) + a[:, 3]
    along = (0.6 * col1 + 0.4 * col2) / np.linalg.norm(0.6 * col1 + 0.4 * col2)
    graze = sr.look_at_pose(face_centre + 60.0 * along, target=face_centre, up=normal)
    return np.stack([oblique, close, graze]), np.array([40.0, 25.0, 45.0])


def _aligned_poses():
    """(poses, focal): a source over the LAST lattice line of axis 0 (x = 5 = n0 - 1, y = 3) at z = 60.5, the camera axes the world's: the
    central ray (iu = W / 2, iw = H / 2) runs along that line, g_0 = n_0 - 1 exactly, and its samples t = 40.5 + s land on z = 20 - s,
    the integers, the faces z = 4 and z = 0 among them.  And a source on the last line of axis 1 (y = 7 = n1 - 1, z = 2) at x = -55.5
    looking along +x (a rotation of 0 and +-1 entries)."""
    down = np.eye(4)
    down[:3, 3] = (5.0, 3.0, 60.5)
    side = sr.look_at_pose((-55.5, 7.0, 2.0), target=(0.0, 7.0, 2.0), up=(0.0, 0.0, 1.0))
    assert set(np.unique(np.abs(side[:3, :3]))) == {0.0, 1.0}
    return np.stack([down, side]), np.array([200.0, 150.0])


CASES = {"general": (GENERAL, _general_poses), "aligned": (ALIGNED, _aligned_poses)}


@pytest.fixture(scope="module")
def setups():
    """Per case: the lattice, a random volume with negative entries, the views on the device, the restatement's plain projection and the
    fused residual's inputs; made once, left unchanged."""
    eng = _engine()
    out = {}
    for k, (name, (lat, make)) in enumerate(CASES.items()):
        poses, focal = make()
        rng = np.random.RandomState(10 + k)
        vol = rng.normal(0.3, 1.0, lat["shape"])
        geo = {key: lat[key] for key in ("width", "height", "near", "far", "n_samples")}
        views = eng.xray_views(poses, focal, device=DEV, **geo)
        rec = views["records"].cpu().numpy()
        assert np.array_equal(rec, sr.view_records(poses, focal))
        b12 = eng.lumen_world_to_index(lat["a12"])      # the library and the restatement get this array alike
        shape_img = (len(poses), lat["height"], lat["width"])
        out[name] = dict(lat=lat, geo=geo, poses=poses, focal=focal, vol=vol, views=views, rec=rec, b12=b12, want=sr.project(vol, b12, rec, **geo),
                         target=rng.normal(0.0, 2.0, shape_img), weight=rng.uniform(0.0, 1.5, shape_img))
    return out


def _chords(s):
    """The restatement's projection of a volume of ones: 0 exactly where no sample of the ray lies inside the lattice."""
    return sr.project(np.ones(s["lat"]["shape"]), s["b12"], s["rec"], **s["geo"])


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("name", list(CASES))
def test_projector_equals_the_restatement(setups, name, fused):
    eng, s = _engine(), setups[name]
    vol = torch.from_numpy(s["vol"]).to(DEV)
    if fused:
        target, weight = torch.from_numpy(s["target"]).to(DEV), torch.from_numpy(s["weight"]).to(DEV)
        got = eng.xray_project(vol, s["views"], s["lat"]["a12"], target=target, weight=weight)
        want = sr.project(s["vol"], s["b12"], s["rec"], target=s["target"], weight=s["weight"], **s["geo"])
        assert np.array_equal(want, s["weight"] * (s["target"] - s["want"]))
    else:
        got = eng.xray_project(vol, s["views"], s["lat"]["a12"])
        want = s["want"]
    chord = _chords(s)
    miss = (chord == 0).reshape(chord.shape[0], -1).mean(axis=1)
    print(f"{name} {'residual' if fused else 'plain'}: rays that miss the lattice per view {np.round(miss, 3).tolist()}, "
          f"max |device - restatement| {np.abs(got.cpu().numpy() - want).max():.3g}")
    assert _same_bits(got, want)
    # the case is what it claims to be
    if name == "general":
        assert miss[0] < 0.35 and miss[1] > 0.4 and 0.0 < miss[2] < 1.0
        assert (chord[2, s["lat"]["height"] // 2] > 0).any()      # the row inside the face i = 0 does meet the lattice
    else:
        lat = s["lat"]
        assert chord[0, lat["height"] // 2, lat["width"] // 2] > 0 and chord[0, lat["height"] // 2, lat["width"] // 2 + 1] == 0
        # the central ray of view 0: unit lattice, unit steps, 5 samples on z = 4 .. 0 at x = 5 = n0 - 1, y = 3: the sum of those voxels
        # (to rounding: a lerp at phi = 1, p + (q - p), is q only to an ulp) - the upper faces of axes 0 and 2 count as inside
        assert abs(s["want"][0, lat["height"] // 2, lat["width"] // 2] - s["vol"][5, 3, :].sum()) <= 1e-12
        assert chord[0, lat["height"] // 2, lat["width"] // 2] == 5.0 and chord[1, lat["height"] // 2, lat["width"] // 2] == 6.0
        assert chord[1, lat["height"] // 2, lat["width"] // 2] > 0


BP_GENERAL_VIEWS = dict(width=9, height=11)
BP_ALIGNED_VIEWS = dict(width=6, height=7)


def _backprojector_setup(name):
    """Views for the backprojector on the lattice of `name`: long focal lengths, so that each detector is smaller than the lattice's
    shadow, one view that looks past the lattice, and one source inside the lattice's bounding box, so that points lie behind it."""
    lat = CASES[name][0]
    a = lat["a12"].reshape(3, 4)
    centre = a[:, :3] @ ((np.asarray(lat["shape"]) - 1) / 2.0) + a[:, 3]
    if name == "general":
        poses = np.stack([sr.look_at_pose(centre + np.array([30.0, 20.0, 48.0]), target=centre + np.array([3.0, 0.0, -2.0])),
                          sr.look_at_pose(centre + np.array([-50.0, 10.0, 5.0]), target=centre + np.array([0.0, 6.0, 0.0])),
                          sr.look_at_pose(centre + np.array([1.0, 0.5, 2.0]), target=centre + np.array([-3.0, -5.0, -9.0])),
                          sr.look_at_pose(centre + np.array([0.0, -70.0, 10.0]), target=centre + np.array([25.0, 0.0, 0.0]))])
        focal, size = np.array([55.0, 60.0, 6.0, 50.0]), BP_GENERAL_VIEWS
    else:
        down = np.eye(4)
        down[:3, 3] = (2.0, 3.0, 30.0)                      # over the lattice line x = 2, y = 3: u = W / 2 and w = H / 2 exactly there
        inside = np.eye(4)
        inside[:3, 3] = (2.5, 3.5, 2.0)                     # inside the lattice: the points with z >= 2 have d <= 0, those at z = 2 have d = 0
        side = sr.look_at_pose((-40.0, 7.0, 2.0), target=(0.0, 7.0, 2.0), up=(0.0, 0.0, 1.0))
        poses, focal, size = np.stack([down, inside, side]), np.array([40.0, 2.0, 30.0]), BP_ALIGNED_VIEWS
    return lat, poses, focal, size


@pytest.fixture(scope="module")
def bp_setups():
    eng = _engine()
    out = {}
    for k, name in enumerate(CASES):
        lat, poses, focal, size = _backprojector_setup(name)
        rng = np.random.RandomState(20 + k)
        images = rng.normal(0.0, 1.0, (len(poses), size["height"], size["width"]))
        views = eng.xray_views(poses, focal, size["width"], size["height"], 1.0, 2.0, 1, device=DEV)
        rec = views["records"].cpu().numpy()
        acc, cnt = sr.backproject(images, rec, lat["shape"], lat["a12"])
        x = sr.lattice_points(lat["shape"], lat["a12"])
        depth = np.stack([-((r[2] * (x[:, 0] - r[9]) + r[5] * (x[:, 1] - r[10])) + r[8] * (x[:, 2] - r[11])) for r in rec])
        out[name] = dict(lat=lat, views=views, rec=rec, images=images, acc=acc, cnt=cnt, depth=depth, x0=rng.uniform(-0.6, 0.8, lat["shape"]),
                         mask=(rng.uniform(size=lat["shape"]) < 0.6).astype(np.uint8))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_backprojector_equals_the_restatement(bp_setups, name):
    eng, s = _engine(), bp_setups[name]
    n_views = s["rec"].shape[0]
    counts = np.bincount(s["cnt"].reshape(-1), minlength=n_views + 1)
    print(f"{name}: points seen by 0..{n_views} views {counts.tolist()}, points with d <= 0 per view {(s['depth'] <= 0).sum(axis=1).tolist()}")
    assert counts[0] > 0 and (counts[1:n_views] > 0).any() and (s["depth"] <= 0).any() and (s["cnt"] > 0).any()
    if name == "aligned":
        assert (s["depth"][1] == 0).any()                   # d = 0 exactly: !(d > 0)
    images = torch.from_numpy(s["images"]).to(DEV)
    acc, seen = eng.xray_backproject(images, s["views"], s["lat"]["shape"], s["lat"]["a12"])
    assert tuple(acc.shape) == s["lat"]["shape"] and seen.dtype == torch.uint16
    assert np.array_equal(seen.cpu().view(torch.int16).numpy().view(np.uint16), s["cnt"])
    assert _same_bits(acc, s["acc"])
    # each output alone
    only_acc = torch.full(s["lat"]["shape"], 7.0, dtype=torch.float64, device=DEV)
    lib_rc = _raw_backproject(images, s["views"], s["lat"], acc=only_acc)
    assert lib_rc[0] == 0 and torch.equal(_bits(only_acc), _bits(acc))
    only_seen = torch.full(s["lat"]["shape"], 7, dtype=torch.int16, device=DEV)
    lib_rc = _raw_backproject(images, s["views"], s["lat"], seen=only_seen)
    assert lib_rc[0] == 0 and torch.equal(only_seen, seen.view(torch.int16))


@pytest.mark.parametrize("masked", [False, True], ids=["no mask", "mask"])
@pytest.mark.parametrize("nonneg", [False, True], ids=["signed", "nonneg"])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_update_equals_the_restatement(bp_setups, name, nonneg, masked):
    eng, s = _engine(), bp_setups[name]
    images = torch.from_numpy(s["images"]).to(DEV)
    x = torch.from_numpy(s["x0"]).to(DEV)
    mask = torch.from_numpy(s["mask"]).to(DEV) if masked else None
    got = eng.xray_backproject(images, s["views"], s["lat"]["shape"], s["lat"]["a12"], x_inout=x, relax=1.9, nonneg=nonneg, mask=mask)
    assert got is x
    want = sr.update(s["x0"], s["acc"], s["cnt"], 1.9, nonneg, s["mask"] if masked else None)
    assert (s["x0"] < 0).any() and (want < 0).any() != nonneg and (want != s["x0"]).any()
    assert _same_bits(x, want)
    if masked:
        assert not want[s["mask"] == 0].any()


def _raw_backproject(image_stack, view_set, lat, **pointers):
    """afx_xray_backproject as C sees it, relax 1, signed -> (return code, afx_last_error); pointers: tensors or addresses for images,
    views, acc, seen, x, mask."""
    from nerf_for_angiography_amd import _lib
    lib = _lib.load()
    ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    a = dict(images=image_stack, views=view_set["records"], acc=None, seen=None, x=None, mask=None)
    a.update(pointers)
    n0, n1, n2 = lat["shape"]
    rc = lib.afx_xray_backproject(ptr(a["images"]), ptr(a["views"]), view_set["n_views"], view_set["width"], view_set["height"], n0, n1, n2,
                                  (C.c_double * 12)(*lat["a12"]), ptr(a["acc"]), ptr(a["seen"]), ptr(a["x"]), 1.0, 0, ptr(a["mask"]), None)
    return rc, (lib.afx_last_error() or b"").decode()


def test_host_memory_is_refused_by_name(setups, bp_setups):
    """A pointer that is not memory of the current device: AFX_E_INVALID before any launch, naming the argument."""
    from nerf_for_angiography_amd import _lib
    lib = _lib.load()
    s = bp_setups["general"]
    host = np.zeros(4096, np.float64)                       # large enough for every role below; never written: the call is refused
    images = torch.from_numpy(s["images"]).to(DEV)
    acc = torch.zeros(s["lat"]["shape"], dtype=torch.float64, device=DEV)
    for change, word in ((dict(images=host.ctypes.data), "images"), (dict(views=host.ctypes.data), "views"), (dict(acc=host.ctypes.data), "acc"),
                         (dict(seen=host.ctypes.data), "seen"), (dict(x=host.ctypes.data), "x_inout"),
                         (dict(x=acc.data_ptr(), mask=host.ctypes.data), "mask")):
        rc, msg = _raw_backproject(images, s["views"], s["lat"], **dict(dict(acc=acc), **change))
        assert rc == -1 and msg.startswith("afx_xray_backproject: ") and word in msg and "not memory" in msg, (change, rc, msg)
    p = setups["general"]
    vol, out = torch.from_numpy(p["vol"]).to(DEV), torch.zeros(3, 10, 13, dtype=torch.float64, device=DEV)
    ptr = lambda t: C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    good = dict(volume=vol, views=p["views"]["records"], target=out, weight=out, out=out)
    for key in good:
        a = dict(good, **{key: host.ctypes.data})
        rc = lib.afx_xray_project(ptr(a["volume"]), 9, 12, 7, (C.c_double * 12)(*p["b12"]), ptr(a["views"]), 3, 13, 10, 38.0, 83.0, 17,
                                  ptr(a["target"]), ptr(a["weight"]), ptr(a["out"]), None)
        msg = lib.afx_last_error().decode()
        assert rc == -1 and msg.startswith("afx_xray_project: ") and key in msg and "not memory" in msg, (key, rc, msg)
    torch.cuda.synchronize()
    assert not out.any() and not acc.any()                  # nothing was launched


# ---- the iteration ----
@pytest.fixture(scope="module")
def scene():
    """sirt_reference.scene() and five iterations of the restatement with the mask, relax = 1; made once."""
    sc = sr.scene()
    sc["x"], sc["residuals"] = sr.sirt(sc["line_integrals"], sr.SCENE_SHAPE, sc["a12"], sc["records"], iterations=5, relax=1.0, mask=sc["mask"],
                                       **sr.SCENE_VIEW)
    return sc


def test_sirt_reconstruct_equals_the_restatement(scene):
    """Volume and residual history, bit for bit.  The history entry is engine.sirt_residual_norm - one torch sum - of an iteration's
    residual images: the images themselves equal the restatement's bits (checked here launch by launch), and the entry equals that sum of
    the restatement's images taken on the same device; NumPy's own sum of them, in another order, agrees to a few ulps."""
    eng = _engine()
    views = eng.xray_views(scene["poses"], sr.SCENE_FOCAL, device=DEV, **sr.SCENE_VIEW)
    b = torch.from_numpy(scene["line_integrals"]).to(DEV)
    mask = torch.from_numpy(scene["mask"]).to(DEV)
    x, history = eng.sirt_reconstruct(views, b, sr.SCENE_SHAPE, scene["a12"], iterations=5, relax=1.0, mask=mask, return_history=True)
    assert _same_bits(x, scene["x"]) and float(x.max()) > 0 and float(x.min()) >= 0
    want = torch.stack([eng.sirt_residual_norm(torch.from_numpy(r).to(DEV)) for r in scene["residuals"]]).cpu()
    print(f"residual history {history.tolist()}")
    assert history.dtype == torch.float64 and torch.equal(_bits(history), _bits(want))
    assert np.allclose(history.numpy(), sr.residual_norms(scene["residuals"]), rtol=1e-14, atol=0) and np.all(np.diff(history.numpy()) < 0)
    # the same iteration, launch by launch
    b12 = eng.lumen_world_to_index(scene["a12"])
    weight = torch.from_numpy(sr.sirt_weight(sr.SCENE_SHAPE, b12, scene["records"], **sr.SCENE_VIEW)).to(DEV)
    ell = eng.xray_project(torch.ones(sr.SCENE_SHAPE, dtype=torch.float64, device=DEV), views, scene["a12"])
    assert torch.equal(_bits(torch.where(ell > 0, 1.0 / ell, torch.zeros_like(ell))), _bits(weight))      # torch's quotient is NumPy's
    y = torch.zeros(sr.SCENE_SHAPE, dtype=torch.float64, device=DEV)
    for it in range(5):
        r = eng.xray_project(y, views, scene["a12"], target=b, weight=weight)
        assert _same_bits(r, scene["residuals"][it]), it
        eng.xray_backproject(r, views, sr.SCENE_SHAPE, scene["a12"], x_inout=y, relax=1.0, nonneg=True, mask=mask)
    assert torch.equal(_bits(y), _bits(x))
    # without history and from a start volume: the same bits, the start volume unchanged
    x4 = eng.sirt_reconstruct(views, b, sr.SCENE_SHAPE, scene["a12"], iterations=4, relax=1.0, mask=mask)
    keep = x4.clone()
    x5 = eng.sirt_reconstruct(views, b, sr.SCENE_SHAPE, scene["a12"], iterations=1, relax=1.0, mask=mask, x0=x4)
    assert torch.equal(_bits(x5), _bits(x)) and torch.equal(_bits(x4), _bits(keep)) and not torch.equal(_bits(x4), _bits(x))


def test_one_captured_iteration_replays_the_same_bits(scene):
    """Both launches of an iteration captured once through torch.cuda.graph; five replays from zero give the volume of five eager
    iterations."""
    eng = _engine()
    views = eng.xray_views(scene["poses"], sr.SCENE_FOCAL, device=DEV, **sr.SCENE_VIEW)
    b = torch.from_numpy(scene["line_integrals"]).to(DEV)
    mask = torch.from_numpy(scene["mask"]).to(DEV)
    weight = torch.from_numpy(sr.sirt_weight(sr.SCENE_SHAPE, eng.lumen_world_to_index(scene["a12"]), scene["records"], **sr.SCENE_VIEW)).to(DEV)
    x = torch.full(sr.SCENE_SHAPE, 3.0, dtype=torch.float64, device=DEV)
    r = torch.zeros_like(b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            eng.xray_project(x, views, scene["a12"], target=b, weight=weight, out=r)
            eng.xray_backproject(r, views, sr.SCENE_SHAPE, scene["a12"], x_inout=x, relax=1.0, nonneg=True, mask=mask)
    torch.cuda.current_stream().wait_stream(side)
    x.zero_()
    for it in range(5):
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(r, scene["residuals"][it]), it
    assert _same_bits(x, scene["x"])


# ---- the sweep's columns ----
def test_sweep_columns_equal_the_stand_alone_scores(golden, monkeypatch):
    """On the G10 setup of test_gpu_sweep_shared.py: the three columns are reconstruction_sirt_metrics' scores, with and without the hull
    as the mask; asked for together with the hull columns, the hull is taken once."""
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from test_gpu_sweep_shared import N, OUTSIDE, _counted, _same
    from nerf_for_angiography_amd.visualization import sweep
    eng = _engine()
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    w, h, focal, src, near, far, s = geo
    poses = sweep._poses(angles, src, (0.0, 0.0, 0.0), DEV)
    hull_views = eng.visual_hull_views(poses, gt.reshape(len(angles), h, w) < 1.0, focal)
    views = eng.xray_views(poses, focal, w, h, near, far, s)
    images = eng.line_integrals(gt.reshape(len(angles), h, w))
    keys = ("dice_sirt", "dice_gain", "corr_sirt")
    alone = sweep.reconstruction_sirt_metrics(m, vol, OUTSIDE, N, views, images, iterations=8)
    print(f"SIRT alone: { {k: alone[0][k] for k in keys + ('dice_model', 'n_sirt', 'n_gt', 'residual')} }")
    assert tuple(alone[1].shape) == (N, N, N) and alone[1].dtype == torch.float64 and float(alone[1].min()) >= 0 and float(alone[1].max()) > 0
    assert all(np.isfinite(alone[0][k]) for k in keys) and alone[0]["corr_sirt"] > 0.2 and not alone[0]["masked"]
    df, _ = sweep.evaluation_sweep(m, gt, angles, *geo, metrics=["CORR 3D SIRT", "PSNR", "DICE 3D SIRT", "DICE GAIN 3D"], volume=vol,
                                   volume_outside=OUTSIDE, volume_points=N, sirt_views=(views, images), sirt_iterations=8)
    assert list(df.columns) == BASE + ["PSNR"] + list(sweep.SIRT_METRICS)
    for col, key in zip(sweep.SIRT_METRICS, keys):
        assert len(df[col]) == len(angles) and all(_same(v, alone[0][key]) for v in df[col].tolist()), (col, df[col][0], alone[0][key])
    # with the hull: the mask of the reconstruction, and one visual_hull call for both families
    masked = sweep.reconstruction_sirt_metrics(m, vol, OUTSIDE, N, views, images, iterations=8, hull_views=hull_views)
    hull = sweep.reconstruction_hull_metrics(m, vol, OUTSIDE, N, hull_views)
    assert masked[0]["masked"] and not masked[1][~hull[1]].any() and masked[1][hull[1]].any()
    calls = {}
    _counted(monkeypatch, eng, ["visual_hull", "sirt_reconstruct"], calls)
    df, _ = sweep.evaluation_sweep(m, gt, angles, *geo, metrics=list(sweep.SIRT_METRICS) + list(sweep.HULL_METRICS), volume=vol,
                                   volume_outside=OUTSIDE, volume_points=N, hull_views=hull_views, sirt_views=(views, images), sirt_iterations=8)
    monkeypatch.undo()
    assert calls == {"visual_hull": 1, "sirt_reconstruct": 1}
    assert list(df.columns) == BASE + list(sweep.HULL_METRICS) + list(sweep.SIRT_METRICS)
    for col, key in zip(sweep.SIRT_METRICS, keys):
        assert all(_same(v, masked[0][key]) for v in df[col].tolist()), (col, df[col][0], masked[0][key])
    for col, key in zip(sweep.HULL_METRICS, ("outside_hull", "dice_hull", "hull_ratio")):
        assert all(_same(v, hull[0][key]) for v in df[col].tolist()), col
    with pytest.raises(ValueError, match="sirt_views"):
        sweep.evaluation_sweep(m, gt, angles, *geo, metrics=["DICE 3D SIRT"], volume=vol)


# ---- the driver ----
@pytest.mark.parametrize("flags", [[], ["--march", "grid", "--grid_init", "hull"]], ids=["plain", "hull mask"])
def test_driver_saves_the_sirt_volume(tmp_path, flags):
    """--save_sirt on the tiny synthetic run: a finite, non-negative, non-zero float64 volume on the 128^3 lattice; with --grid_init hull
    it is zero outside the hull the grids were carved with."""
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    path = tmp_path / "sirt.npy"
    out = main(["--synthetic", "--binary", "True", "--img_size", "32", "--number_angles", "2", "--n_iters", "16", "--display_every", "16",
                "--sample_size", "24", "--depth_samples", "100", "--num_layers", "4", "--num_hidden_units", "64", "--save_sirt", str(path),
                "--sirt_iterations", "10", "--log_dir", str(tmp_path / "run")] + flags)
    x = np.load(path)
    info = out["sirt_info"]
    print(f"sirt info {info}")
    assert x.shape == (128, 128, 128) and x.dtype == np.float64
    assert np.isfinite(x).all() and x.min() >= 0 and x.max() > 0
    assert info["n_views"] == 9 and info["iterations"] == 10 and info["residual_last"] < info["residual_first"] and info["max"] == x.max()
    assert info["masked"] == bool(flags)
    if flags:
        hull = np.load(tmp_path / "run" / "hull.npy")
        assert not x[~hull].any() and x[hull].any()
