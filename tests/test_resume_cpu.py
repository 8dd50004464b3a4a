"""The training-state file (nerf/checkpoint.py) and the driver's --checkpoint_every / --resume flags, without a GPU: parsing, the host-side
round trip, the fingerprint, the format version, atomic replacement, and the model file's unchanged layout."""
import os
import random

import numpy as np
import pytest
import torch

from nerf_for_angiography_amd.nerf import checkpoint as ck
from nerf_for_angiography_amd.nerf import run_nerf_acc as drv


def _args(*argv):
    return drv.build_parser().parse_args(list(argv))


def _table(n=50, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g), torch.rand(n, generator=g), torch.rand(n, generator=g))


def _model_definition(width=64):
    return {'num_early_layers': 4, 'num_late_layers': 0, 'num_filters': width, 'num_input_channels': 3, 'num_output_channels': 1,
            'num_input_channels_views': 0, 'use_bias': True, 'pos_enc': 'none', 'pos_enc_basis': 5, 'act_func': 'relu', 'fourier_sigma': 5,
            'num_img': 1, 'device': torch.device('cpu'), 'precision': 'f16s8'}


def _trained_adam(seed=0, steps=3):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(3, 8), torch.nn.ReLU(), torch.nn.Linear(8, 1))
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    for _ in range(steps):
        opt.zero_grad()
        net(torch.randn(16, 3)).square().mean().backward()
        opt.step()
    return net, opt


def test_flags_parse():
    a = _args('--resume', 'runs/x', '--checkpoint_every', '500')
    assert a.resume == 'runs/x' and a.checkpoint_every == 500
    d = _args()
    assert d.resume is None and d.checkpoint_every == 0      # the defaults: no state is read or written
    assert (d.barf_start, d.barf_stop) == (8000, 250000)      # the reference's schedule


def test_main_accepts_the_flags(tmp_path):
    """main() gets past argparse with both flags (an unknown flag is exit status 2); what stops it here is the missing GPU, or - on a GPU
    box - the missing state file."""
    try:
        drv.main(['--synthetic', '--img_size', '16', '--resume', str(tmp_path / 'absent.pt'), '--checkpoint_every', '10',
                  '--log_dir', str(tmp_path / 'log')])
    except SystemExit as exc:
        assert exc.code != 2, "argparse refused --resume / --checkpoint_every"
    except FileNotFoundError:
        pass


def test_checkpoint_interval_rounds_up_to_whole_rounds():
    assert drv.checkpoint_interval(20, True) == 32
    assert drv.checkpoint_interval(32, True) == 32
    assert drv.checkpoint_interval(33, True) == 48
    assert drv.checkpoint_interval(20, False) == 20
    assert drv.checkpoint_interval(0, True) == 0 and drv.checkpoint_interval(0, False) == 0
    with pytest.raises(ValueError):
        drv.check_args(_args('--checkpoint_every', '-1'))


def test_host_side_round_trip(tmp_path):
    """Optimizer state of a CPU Adam, history, counters, RNG states and the fingerprint: saved, loaded into a second set of live objects,
    equal tensor for tensor - and the moments are copied INTO the second optimizer's tensors, not rebound."""
    net, opt = _trained_adam(seed=0)
    fp = ck.config_fingerprint(_args('--seed', '4'), _model_definition(), _table())
    history = [dict(iter=0, train_loss=0.25, test_psnr=11.5, eval_candidates_per_kept=None), dict(iter=10, train_loss=0.125, test_psnr=12.75)]
    counters = dict(highest_psnr=12.75, highest_iter=10, lr=9.5e-5, loss=torch.tensor(0.125), n_marched=1234)
    random.seed(5), np.random.seed(6), torch.manual_seed(7)
    random.random(), np.random.rand(3), torch.rand(3)
    path = ck.save_training_state(tmp_path / ck.STATE_FILE, fingerprint=fp, n_iter=11, model=net, optimizer=opt, history=history,
                                  counters=counters)
    expect = (random.random(), np.random.rand(4), torch.rand(4))      # what the saved generators produce next

    net2, opt2 = _trained_adam(seed=1, steps=1)
    live = {id(p): dict(opt2.state[p]) for p in opt2.state}
    random.seed(50), np.random.seed(60), torch.manual_seed(70)
    state = ck.load_training_state(tmp_path, fingerprint=fp, model=net2, optimizer=opt2)      # (a directory: its trainstate.pt)
    assert path == str(tmp_path / ck.STATE_FILE)
    assert state['n_iter'] == 11 and state['format_version'] == ck.FORMAT_VERSION
    assert state['history'] == history
    assert state['fingerprint'] == fp
    c = state['counters']
    assert (c['highest_psnr'], c['highest_iter'], c['lr'], c['n_marched']) == (12.75, 10, 9.5e-5, 1234)
    assert torch.equal(c['loss'], torch.tensor(0.125))
    for a, b in zip(net.parameters(), net2.parameters()):
        assert torch.equal(a, b)
    for a, b in zip(opt.param_groups[0]['params'], opt2.param_groups[0]['params']):
        for k in ('exp_avg', 'exp_avg_sq', 'step'):
            assert torch.equal(opt.state[a][k], opt2.state[b][k]), k
            assert opt2.state[b][k] is live[id(b)][k], f"{k} was rebound"
    assert opt2.param_groups[0]['lr'] == opt.param_groups[0]['lr'] and tuple(opt2.param_groups[0]['betas']) == (0.9, 0.999)
    got = (random.random(), np.random.rand(4), torch.rand(4))
    assert got[0] == expect[0] and np.array_equal(got[1], expect[1]) and torch.equal(got[2], expect[2])

    # both optimizers now take the same step
    for n, o in ((net, opt), (net2, opt2)):
        o.zero_grad()
        n(torch.ones(4, 3)).square().mean().backward()
        o.step()
    for a, b in zip(net.parameters(), net2.parameters()):
        assert torch.equal(a, b)


def test_optimizer_state_is_created_when_the_live_optimizer_has_none(tmp_path):
    net, opt = _trained_adam(seed=0)
    ck.save_training_state(tmp_path / 's.pt', fingerprint={}, n_iter=3, optimizer=opt)
    net2, opt2 = _trained_adam(seed=0, steps=0)
    ck.load_training_state(tmp_path / 's.pt', optimizer=opt2, rng=False)
    for a, b in zip(opt.param_groups[0]['params'], opt2.param_groups[0]['params']):
        for k in ('exp_avg', 'exp_avg_sq', 'step'):
            assert torch.equal(opt.state[a][k], opt2.state[b][k]), k


@pytest.mark.parametrize("field,argv,width", [("precision", ['--precision', 'f16'], 64), ("seed", ['--seed', '1'], 64),
                                              ("model.num_filters", [], 128), ("march", ['--march', 'grid'], 64),
                                              ("graph_rounds", ['--graph-rounds'], 64), ("sample_size", ['--sample_size', '9'], 64)])
def test_fingerprint_mismatch_names_the_field(tmp_path, field, argv, width):
    table = _table()
    saved = ck.config_fingerprint(_args(), _model_definition(), table)
    ck.save_training_state(tmp_path / 's.pt', fingerprint=saved, n_iter=1)
    now = ck.config_fingerprint(_args(*argv), _model_definition(width), table)
    with pytest.raises(ValueError) as exc:
        ck.load_training_state(tmp_path / 's.pt', fingerprint=now)
    assert field in str(exc.value)
    others = {"precision", "seed", "model.num_filters", "march", "graph_rounds", "sample_size"} - {field}
    assert not any(f"{o} (" in str(exc.value) for o in others), "a field that did not change is named"


def test_fingerprint_covers_the_ray_table_and_ignores_the_run_length(tmp_path):
    saved = ck.config_fingerprint(_args('--n_iters', '100', '--log_dir', 'a'), _model_definition(), _table())
    assert saved == ck.config_fingerprint(_args('--n_iters', '900', '--log_dir', 'b', '--checkpoint_every', '7'), _model_definition(), _table())
    other = list(_table())
    other[2] = other[2].clone()
    other[2][17] += 1e-3
    with pytest.raises(ValueError, match="ray_table_sha256"):
        ck.compare_fingerprints(saved, ck.config_fingerprint(_args(), _model_definition(), other))
    with pytest.raises(ValueError, match="n_rays"):
        ck.compare_fingerprints(saved, ck.config_fingerprint(_args(), _model_definition(), _table(n=51)))


def test_future_format_version_is_refused(tmp_path, monkeypatch):
    monkeypatch.setattr(ck, "FORMAT_VERSION", ck.FORMAT_VERSION + 1)
    ck.save_training_state(tmp_path / 's.pt', fingerprint={}, n_iter=1)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="format version"):
        ck.read_training_state(tmp_path / 's.pt')
    torch.save({'model': {}}, tmp_path / 'm.pt')
    with pytest.raises(ValueError, match="not a training-state file"):
        ck.read_training_state(tmp_path / 'm.pt')


def test_interrupted_save_leaves_the_previous_file(tmp_path, monkeypatch):
    path = tmp_path / ck.STATE_FILE
    ck.save_training_state(path, fingerprint={'seed': 0}, n_iter=5, history=[dict(iter=0, test_psnr=1.5)])
    before = path.read_bytes()

    def fail(src, dst):
        raise OSError("interrupted")
    monkeypatch.setattr(os, "replace", fail)
    with pytest.raises(OSError, match="interrupted"):
        ck.save_training_state(path, fingerprint={'seed': 0}, n_iter=9, history=[dict(iter=0, test_psnr=1.5), dict(iter=8, test_psnr=2.5)])
    monkeypatch.undo()
    assert path.read_bytes() == before
    state = ck.read_training_state(path)
    assert state['n_iter'] == 5 and state['history'] == [dict(iter=0, test_psnr=1.5)]
    assert sorted(os.listdir(tmp_path)) == [ck.STATE_FILE], "the temporary file was left behind"


def test_missing_piece_is_an_error_unless_not_strict(tmp_path):
    net, opt = _trained_adam()
    ck.save_training_state(tmp_path / 's.pt', fingerprint={}, n_iter=2, model=net)
    with pytest.raises(ValueError, match="optimizer"):
        ck.load_training_state(tmp_path / 's.pt', model=net, optimizer=opt)
    ck.load_training_state(tmp_path / 's.pt', model=net, optimizer=opt, strict=False)


def test_model_file_next_to_the_state_keeps_the_reference_layout(tmp_path):
    from nerf_for_angiography_amd.model.CPPN import CPPN
    definition = _model_definition()
    model = CPPN(dict(definition))
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    model.save(str(tmp_path / 'coarsemodel.pth'), {'epochs': 3, 'psnr': 20.0})
    ck.save_training_state(tmp_path / ck.STATE_FILE, fingerprint=ck.config_fingerprint(_args(), definition, _table()), n_iter=4, model=model,
                           optimizer=opt)
    saved = torch.load(tmp_path / 'coarsemodel.pth', weights_only=False)
    assert set(saved) == {'version', 'parameters', 'training_information', 'model'}
    assert saved['training_information'] == {'epochs': 3, 'psnr': 20.0}
    assert set(saved['model']) == set(model.state_dict())
    state = ck.read_training_state(tmp_path)
    for k, v in model.state_dict().items():
        assert torch.equal(state['model']['state_dict'][k], v), k


def test_grid_training_state_is_copied_into_the_live_buffers():
    """On the host (the bitfield is packed once the grid reaches the GPU): occs and the mask are copied in, not rebound; another seed or
    resolution is refused; nn.Module's own state_dict keeps its keys."""
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    aabb = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    g = OccupancyGrid(aabb, resolution=8, seed=3)
    g.occs.copy_(torch.rand(g.num_cells, generator=torch.Generator().manual_seed(1)))
    g.set_binary(g.occs > 0.5)
    state = g.training_state()
    h = OccupancyGrid(aabb, resolution=8, seed=3)
    occs, mask = h.occs, h._binary_u8
    h.load_training_state(state)
    assert h.occs is occs and h._binary_u8 is mask
    assert torch.equal(h.occs, g.occs) and torch.equal(h.binary, g.binary) and bool(h.binary.any())
    with pytest.raises(ValueError, match="seed"):
        OccupancyGrid(aabb, resolution=8, seed=4).load_training_state(state)
    with pytest.raises(ValueError, match="resolution"):
        OccupancyGrid(aabb, resolution=4, seed=3).load_training_state(state)
    assert set(g.state_dict()) == {"_roi_aabb", "resolution", "occs", "_binary_u8", "_bits", "_scratch", "_partial"}
