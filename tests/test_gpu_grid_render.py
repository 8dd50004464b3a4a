"""The forward-only grid render with one evaluation of the model (afx_march_render, render.march_render / march_render_projection,
evaluation_sweep(grid=...), the driver's --march grid test render): bit for bit against the operator sequence it replaces -
acc_ray_marching -> get_predictions over the kept samples -> acc_render_volume_density - at every precision, against the oracle at f32, over
both ray modes, chunkings and the edge cases of the per-ray kernel (run with -m gpu on an MI355X)."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_gpu_parity import DEV
from test_gpu_grid_graph import AABB, _mask, _grid, _rays

pytestmark = pytest.mark.gpu

NEAR, FAR, SPR, EPS, THRE = 1400.0, 1600.0, 300, 1e-2, 1e-3


def _model(layers, width, enc="none", act="relu", prec="f32", seed=8, bias=-3.0):
    from nerf_for_angiography_amd.model.CPPN import CPPN
    torch.manual_seed(seed)
    md = dict(num_early_layers=layers, num_late_layers=0, num_filters=width, num_input_channels=3, num_output_channels=1,
              num_input_channels_views=0, use_bias=True, pos_enc=enc, pos_enc_basis=5, act_func=act, fourier_sigma=5, num_img=1,
              device=torch.device(DEV), precision=prec)
    m = CPPN(md).to(DEV)
    if enc == "barf":
        m.update_barf_alpha(2.5, "pts")
    with torch.no_grad():
        m.output_linear[0].weight.mul_(4.0)
        m.output_linear[0].bias.fill_(bias)
    return m


def _aabb():
    return torch.tensor(AABB, dtype=torch.float32, device=DEV)


def _op_sequence(m, grid, o, d, spr=SPR, near=NEAR, far=FAR, eps=EPS, thre=THRE, aabb=None):
    """The reference's evaluation render (nerf/run_nerf_acc.py:338-349): march + alpha pass + visibility, then the kept samples evaluated
    again and composited.  -> (pixels, ray_indices, t_starts, t_ends, raw of the kept samples)"""
    from nerf_for_angiography_amd.nerf.nerf_helpers import get_predictions
    from nerf_for_angiography_amd.nerf.nerf_helpers_acc import acc_ray_marching, acc_render_volume_density
    ri, ts, te = acc_ray_marching(m, grid, _aabb() if aabb is None else aabb, o, d, spr, near, far, eps, thre)
    pos = o[ri.long()] + d[ri.long()] * (ts + te) / 2.0
    raw = get_predictions(m, pos, 8192) if len(ri) else pos[:, :1]
    pix, _ = acc_render_volume_density(raw, ri, ts, te, o.shape[0], spr)
    return pix, ri, ts, te, raw.reshape(-1)


def _render(m, grid, o, d, spr=SPR, near=NEAR, far=FAR, eps=EPS, thre=THRE, binary_thresh=None):
    from nerf_for_angiography_amd.render import march_render
    return march_render(m, grid, _aabb(), o, d, spr, near, far, eps, thre, binary_thresh=binary_thresh)


def _n_candidates(grid, o, d, spr=SPR, near=NEAR, far=FAR):
    from nerf_for_angiography_amd import engine
    ri, *_ = engine.march(o, d, AABB, near, far, (far - near) / spr, grid_bits=None if grid is None else grid.bits,
                          grid_aabb=None if grid is None else grid._aabb_host, grid_res=None if grid is None else grid._res_host,
                          want_points=False)
    return ri.numel()


def _check_equal(m, grid, o, d, **kw):
    with torch.no_grad():
        want, ri, *_ = _op_sequence(m, grid, o, d, **kw)
        pix, (n_cand, n_kept) = _render(m, grid, o, d, **kw)
    kept = m.engine.last_kept_counts
    assert torch.equal(pix, want)
    assert torch.equal(kept.long(), torch.bincount(ri.long(), minlength=o.shape[0]))
    assert n_kept == ri.numel() and n_cand == _n_candidates(grid, o, d, **{k: v for k, v in kw.items() if k in ("spr", "near", "far")})
    return pix, kept, n_cand, n_kept


MODELS = {"relu4x64": (4, 64, "none", "relu"), "relu4x128": (4, 128, "none", "relu"), "relu8x256": (8, 256, "none", "relu"),
          "barf4x128": (4, 128, "barf", "relu"), "tanh4x128": (4, 128, "none", "tanh")}


@pytest.mark.parametrize("kind", ["sphere", "sparse"])
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16", "f16"])
def test_equals_the_operator_sequence(prec, model, kind):
    """Pixels bit for bit and kept counts equal to the per-ray counts of the operator sequence's ray_indices: each sample's raw output is a
    function of its own point, so the alpha pass's raw output is the one the second evaluation gives."""
    layers, width, enc, act = MODELS[model]
    m = _model(layers, width, enc, act, prec)
    o, d, _ = _rays(1500, 17)
    _, kept, n_cand, n_kept = _check_equal(m, _grid(kind), o, d)
    assert n_cand >= n_kept > 0
    assert int((kept == 0).sum()) > 0 or kind == "sphere"


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_binary_pixel(prec):
    """The binary image (visualization.py:349-352): the kept samples composited again with sigma forced to 0 where sigmoid(raw) < thresh."""
    from nerf_for_angiography_amd.nerf.nerf_helpers_acc import acc_render_volume_density
    m = _model(4, 128, prec=prec, bias=-2.5)
    o, d, _ = _rays(400, 5)
    grid = _grid("sphere")
    with torch.no_grad():
        want, ri, ts, te, raw = _op_sequence(m, grid, o, d)
        sg = torch.sigmoid(raw).sort().values
        # the threshold: mid-way across the widest gap between the kept samples' sigmoids (outside the extreme tenths), so that torch's and
        # the kernel's sigmoid cannot disagree at the boundary
        lo, hi = len(sg) // 10, len(sg) - len(sg) // 10
        j = lo + int(torch.argmax(sg[lo + 1:hi] - sg[lo:hi - 1]))
        thresh = float((sg[j] + sg[j + 1]) / 2)
        assert float((torch.sigmoid(raw) - thresh).abs().min()) > 1e-6
        zero_idx = torch.where(torch.sigmoid(raw) < thresh)[0]
        assert 0 < zero_idx.numel() < raw.numel()
        want_bin, _ = acc_render_volume_density(raw, ri, ts, te, o.shape[0], SPR, zero_idx=zero_idx)
        pix, binary, (n_cand, n_kept) = _render(m, grid, o, d, binary_thresh=thresh)
    assert torch.equal(pix, want) and torch.equal(binary, want_bin)
    assert not torch.equal(binary, pix) and bool((binary >= pix).all())


def test_against_the_oracle_f32():
    """oracle.march_grid + render_visibility + acc_render_volume_density (plain PyTorch-CPU loops): kept counts equal, pixels to 1e-5."""
    from oracle import angio_oracle as orc
    m = _model(4, 64, prec="f32", bias=-2.5)
    o, d, _ = _rays(40, 23)
    grid = _grid("sphere")
    with torch.no_grad():
        pix, (n_cand, n_kept) = _render(m, grid, o, d)
    kept = m.engine.last_kept_counts.cpu().long()
    oc, dc, box = o.cpu(), d.cpu(), torch.tensor(AABB)
    ri, ts, te = orc.march_grid(oc, dc, box, NEAR, FAR, (FAR - NEAR) / SPR, binary=_mask("sphere"), grid_aabb=box)
    mid = oc[ri] + dc[ri] * ((ts + te) * 0.5)[:, None]
    params = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    raw = orc.cppn_forward(mid, dict(num_early_layers=4, num_filters=64, pos_enc="none", pos_enc_basis=5), params).reshape(-1).float()
    alpha = 1 - torch.exp(-torch.sigmoid(raw) * (te - ts))
    keep = orc.render_visibility(alpha, ri, EPS, THRE)
    want = orc.acc_render_volume_density(raw[keep][:, None], ri[keep], ts[keep][:, None], te[keep][:, None], o.shape[0])
    assert n_cand == ri.numel() and n_kept == int(keep.sum()) > 0
    assert torch.equal(kept, torch.bincount(ri[keep], minlength=o.shape[0]))
    assert rel_l2(pix.cpu().numpy(), want.numpy()) < 1e-5


def _port_rays(th, ph, w, h, f, src):
    """The port's get_ray_values on the host (float64, pinned against the kernel's ray generation by G2), cast as the reference batches them."""
    from nerf_for_angiography_amd.phantomdata.helpers import get_ray_values
    o, d = get_ray_values(th, ph, 0.0, np.asarray(src, dtype=np.float64), w, h, f, "cpu")[:2]
    return o.reshape(-1, 3).float().to(DEV), d.reshape(-1, 3).float().to(DEV)


def test_pose_mode_equals_arrays_mode_and_chunking_changes_nothing(golden):
    from nerf_for_angiography_amd.render import march_render, march_render_projection
    from nerf_for_angiography_amd.visualization.sweep import _poses, sweep_angles
    m = _model(4, 128, prec="f16")
    grid = _grid("sphere")
    g2 = golden("g2_rays")
    with torch.no_grad():
        for tag in ("a", "b", "c"):      # G2's views: the rays the dense fused kernels generate
            w, h, f = g2[f"{tag}_whf"]
            w, h, f = int(w), int(h), float(f)
            o = torch.from_numpy(g2[f"{tag}_o"].reshape(-1, 3).astype(np.float32)).to(DEV)
            d = torch.from_numpy(g2[f"{tag}_d"].reshape(-1, 3).astype(np.float32)).to(DEV)
            pose = torch.from_numpy(g2[f"{tag}_pose"][None]).to(DEV)
            near, far = f + 50.0, f + 350.0
            a, ca = march_render(m, grid, _aabb(), o, d, SPR, near, far)
            b, cb = march_render_projection(m, grid, _aabb(), pose, w, h, f, SPR, near, far)
            assert torch.equal(a, b) and ca == cb and ca[1] > 0, tag
        # nine views of the sweep in one call, against the port's rays; then chunked so that calls split views
        angles = sweep_angles(40, 20)
        w, h, f, src = 24, 20, 13.0 * 24, [0, 0, 1500.0]
        poses = _poses(angles, src, (0.0, 0.0, 0.0), DEV)
        rays = [_port_rays(th if th >= 0 else 360 + th, ph if ph >= 0 else 360 + ph, w, h, f, src) for th, ph in angles]
        o, d = torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays])
        a, abin, ca = march_render(m, grid, _aabb(), o, d, SPR, NEAR, FAR, binary_thresh=0.05)
        b, bb, cb = march_render_projection(m, grid, _aabb(), poses, w, h, f, SPR, NEAR, FAR, binary_thresh=0.05)
        assert torch.equal(a, b) and torch.equal(abin, bb) and ca == cb and cb[1] > 0
        kept = m.engine.last_kept_counts.clone()
        eng = m.engine
        full = eng.max_workspace_bytes
        try:
            eng.max_workspace_bytes = int(eng.lib.afx_march_render_workspace_bytes(1, 700, 302))      # ~700 rays per call: 480-ray views split
            c, cbin, cc = march_render_projection(m, grid, _aabb(), poses, w, h, f, SPR, NEAR, FAR, binary_thresh=0.05)
            kept_c = eng.last_kept_counts.clone()
            e, ce = march_render(m, grid, _aabb(), o, d, SPR, NEAR, FAR)
        finally:
            eng.max_workspace_bytes = full
        assert torch.equal(b, c) and torch.equal(bb, cbin) and cb == cc and torch.equal(kept, kept_c)
        assert torch.equal(a, e) and ce == cb
        # a window of the table (ray_id0 / n_rays)
        part, _ = march_render_projection(m, grid, _aabb(), poses, w, h, f, SPR, NEAR, FAR, ray_id0=1000, n_rays=1500)
        assert torch.equal(part, b[1000:2500])


def test_edges():
    m = _model(4, 128, prec="f16")
    o, d, _ = _rays(256, 31)
    with torch.no_grad():
        # an empty grid: no candidates, every pixel 1
        pix, (n_cand, n_kept) = _render(m, _grid("empty"), o, d)
        assert n_cand == 0 and n_kept == 0 and bool((pix == 1).all()) and int(m.engine.last_kept_counts.abs().sum()) == 0
        # rays that miss the box, mixed with rays that hit it
        o2 = o.clone()
        o2[::2, 0] += 400.0
        pix, kept, n_cand, n_kept = _check_equal(m, _grid("sphere"), o2, d)
        assert bool((pix[::2] == 1).all()) and int(kept[::2].sum()) == 0 and int(kept[1::2].sum()) > 0
        # exactly 64 and 65 candidates per ray (no grid; planes inside the box), alpha_thre = early_stop_eps = 0: every candidate kept
        oz = torch.tensor([[0.0, 0.0, 1500.0]], device=DEV).repeat(8, 1) + torch.randn(8, 3, device=DEV)
        dz = torch.tensor([[0.0, 0.0, -1.0]], device=DEV).repeat(8, 1)
        for n in (64, 65):
            pix, kept, n_cand, n_kept = _check_equal(m, None, oz, dz, spr=n, near=1450.0, far=1450.0 + n, eps=0.0, thre=0.0)
            assert n_cand == n_kept == 8 * n and bool((kept == n).all())
        # early stop in the middle of a chunk: dense samples, T < early_stop_eps after a handful of them
        md = _model(4, 128, prec="f16", bias=2.0)
        pix, kept, n_cand, n_kept = _check_equal(md, None, oz, dz, spr=130, near=1450.0, far=1580.0)
        assert n_cand == 8 * 130 and bool((kept > 0).all()) and int(kept.min()) < 64 and int(kept.max()) < 130
        pix, kept, *_ = _check_equal(md, None, oz, dz, spr=130, near=1450.0, far=1580.0, eps=0.0, thre=0.0)
        assert bool((kept == 130).all())


def test_evaluation_sweep_with_a_grid():
    """evaluation_sweep(grid=...) on 3 x 3 views against a per-view loop of the reference's CT sweep (visualization.py:335-352): the operator
    sequence and the binary render.  Images equal, PSNR to 1e-4, DICE 2D exactly."""
    from nerf_for_angiography_amd.nerf.nerf_helpers_acc import acc_render_volume_density
    from nerf_for_angiography_amd.visualization.sweep import evaluation_sweep, sweep_angles
    m = _model(4, 64, prec="f16", bias=-5.0)
    with torch.no_grad():
        m.output_linear[0].weight.mul_(2.0)
    grid = _grid("sphere")
    angles = sweep_angles(40, 20)
    w, h, f, src, spr, bt = 24, 20, 13.0 * 24, [0, 0, 1500.0], 400, 0.05
    g = torch.Generator().manual_seed(3)
    targets = torch.rand(9, h, w, generator=g).to(DEV)
    bin_targets = (targets > 0.5).float()
    df, preds = evaluation_sweep(m, targets, angles, w, h, f, np.array(src), NEAR, FAR, spr, binary_thresh=bt, binary_targets=bin_targets,
                                 views_per_launch=4, grid=grid, scene_aabb=_aabb())
    with torch.no_grad():
        for i, (th, ph) in enumerate(angles):
            o, d = _port_rays(th if th >= 0 else 360 + th, ph if ph >= 0 else 360 + ph, w, h, f, src)
            pix, ri, ts, te, raw = _op_sequence(m, grid, o, d, spr=spr)
            zero_idx = torch.where(torch.sigmoid(raw) < bt)[0]
            bpix, _ = acc_render_volume_density(raw, ri, ts, te, o.shape[0], spr, zero_idx=zero_idx)
            assert torch.equal(preds[i].reshape(-1), pix), i
            psnr = float(-10.0 * torch.log10(((pix - targets[i].reshape(-1)) ** 2).mean()))
            assert abs(df["PSNR"][i] - psnr) < 1e-4, i
            dice = float(((bpix >= 1).long() == (bin_targets[i].reshape(-1) >= 1).long()).float().mean())
            assert df["DICE 2D"][i] == dice, i
    assert not math.isclose(float(preds.min()), 1.0)


def test_driver_grid_test_render(tmp_path):
    """--march grid renders its test view with march_render: a finite test PSNR and the candidates : kept ratio in every record."""
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    base = ["--synthetic", "--img_size", "20", "--number_angles", "1", "--limited_size", "90", "--n_iters", "48", "--display_every", "16",
            "--sample_size", "16", "--depth_samples", "100", "--num_layers", "4", "--num_hidden_units", "64", "--sampling_strategy", "segmentation",
            "--march", "grid", "--precision", "f16s8", "--log_dir", str(tmp_path / "grid")]
    h = main(base)["history"]
    assert len(h) == 4
    for r in h:
        assert math.isfinite(r["test_psnr"]) and r["eval_candidates_per_kept"] is not None and r["eval_candidates_per_kept"] >= 1.0, r
