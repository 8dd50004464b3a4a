"""What --checkpoint_every / --resume cost (run on the GPU box; profiles/r10_resume.md).

    python tools/resume_cost.py rate [PACKAGE_ROOT]   the grid loop of tools/prof_driver.py through main() with --checkpoint_every 0: the driver's
                                                      own it_per_s records.  PACKAGE_ROOT: a directory that holds another checkout's
                                                      nerf_for_angiography_amd (the parent commit), to interleave the two.
    python tools/resume_cost.py save                  wall time and file size of one save_training_state at 8x256 with two 128^3 grids
                                                      (fused capturable Adam with state), and of the load into the live objects.
    python tools/resume_cost.py save-host             the same objects in host memory: serialisation, fsync and rename without the read-back.
"""
import json, os, sys, tempfile, time

root = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.abspath(root))
import torch

if sys.argv[1] == "rate":
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    with tempfile.TemporaryDirectory() as tmp:
        r = main(["--synthetic", "--img_size", "100", "--number_angles", "9", "--limited_size", "180", "--n_iters", "2000", "--display_every", "500",
                  "--sample_size", "75", "--depth_samples", "300", "--num_layers", "4", "--num_hidden_units", "128", "--sampling_strategy",
                  "segmentation", "--march", "grid", "--log_dir", tmp])
    print(json.dumps(dict(root=os.path.abspath(root), it_per_s=[h["it_per_s"] for h in r["history"][1:]])))
else:
    from nerf_for_angiography_amd.model.CPPN import CPPN
    from nerf_for_angiography_amd.nerf import checkpoint as ck
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    on_gpu = sys.argv[1] == "save"
    dev = torch.device("cuda:0" if on_gpu else "cpu")
    sync = torch.cuda.synchronize if on_gpu else (lambda: None)
    model = CPPN(dict(num_early_layers=8, num_late_layers=0, num_filters=256, num_input_channels=3, num_output_channels=1,
                      num_input_channels_views=0, use_bias=True, pos_enc="none", pos_enc_basis=5, act_func="relu", fourier_sigma=5, num_img=1,
                      device=dev, precision="f16s8")).to(dev)
    opt = torch.optim.Adam(list(model.parameters()), lr=torch.tensor(1e-4, device=dev), fused=on_gpu, capturable=on_gpu)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    opt.step()
    aabb = torch.tensor([-100.0] * 3 + [100.0] * 3, device=dev)
    grids = [OccupancyGrid(roi_aabb=aabb, resolution=128, seed=s).to(dev) for s in (0, 1)]
    for g in grids:
        g.occs.uniform_()
        g.set_binary(g.occs > 0.5)
    history = [dict(iter=i, train_loss=0.1, test_psnr=20.0) for i in range(0, 500000, 500)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, ck.STATE_FILE)
        save, load = [], []
        for _ in range(6):
            sync()
            t = time.perf_counter()
            ck.save_training_state(path, fingerprint={}, n_iter=1, model=model, optimizer=opt, grids=grids, history=history, counters={})
            save.append(time.perf_counter() - t)
            t = time.perf_counter()
            ck.load_training_state(path, model=model, optimizer=opt, grids=grids)
            sync()
            load.append(time.perf_counter() - t)
        print(json.dumps(dict(save_ms=[round(1e3 * x, 1) for x in save], load_ms=[round(1e3 * x, 1) for x in load],
                              file_MB=round(os.path.getsize(path) / 1e6, 1))))
