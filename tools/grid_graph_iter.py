#!/usr/bin/env python3
"""ms per grid training iteration (nerf/run_nerf_acc.py:284-306, with the Adam step) at the reference's 5 625 rays x 300 steps, five ways:
  one      - render.march_train_step_mse (afx_march_train_step_mse: two polled size read-backs per iteration) + Adam(fused)
  capt     - afx_march_train_step_mse_capturable issued eagerly (re-tiling, step, loss, Adam(fused, capturable) with found_inf = skip)
  graph    - render.GridTrainGraph: the same iteration captured once and replayed
  se       - afx_march_train_step_mse_single_eval issued eagerly like `capt` (one evaluation of the model per iteration)
  se_graph - render.GridTrainGraph(single_eval=True)
on a trained-like occupancy grid (cells within 4 units of a capsule vessel tree) and on a full grid, for 4x128 and 8x256.  Prints a
markdown table (and writes it to the path given as the first argument).  usage: grid_graph_iter.py [out.md [iters]]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from nerf_for_angiography_amd.model.CPPN import CPPN
from nerf_for_angiography_amd.render import march_train_step_mse, GridTrainGraph
from nerf_for_angiography_amd.engine import RayBatchSampler
from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
from nerf_for_angiography_amd.phantomdata.helpers import capsule_tree, capsule_mu

dev = torch.device("cuda:0")
out_path = sys.argv[1] if len(sys.argv) > 1 else None
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
R, S, near, far, eps, thre = 5625, 300, 1400.0, 1600.0, 1e-2, 1e-4
aabb = [-100.0, -100, -100, 100, 100, 100]
torch.manual_seed(0)
NT = 90 * 100 * 100
tab_o = torch.randn(NT, 3, device=dev) * 3 + torch.tensor([0, 0, 1500.0], device=dev)
tab_d = torch.nn.functional.normalize(torch.randn(NT, 3, device=dev) * 0.03 + torch.tensor([0, 0, -1.0], device=dev), dim=-1)
tab_p, tab_w = torch.rand(NT, device=dev), torch.rand(NT, device=dev) + 0.05
sampler = RayBatchSampler(tab_o, tab_d, tab_p, tab_w, R, seed=0, prefetch=16)
batches = [tuple(t.clone() for t in sampler.draw(i)[:3]) for i in range(16)]      # drawn once: every path trains on the same 16 batches

res = 128
c = (torch.stack(torch.meshgrid(*[torch.arange(res, device=dev)] * 3, indexing="ij"), -1).float() + 0.5) / res * 200 - 100
caps = capsule_tree(levels=5, seed=0)
caps[:, 6] += 4.0
masks = {"trained-like": torch.cat([capsule_mu(c[i:i + 8].reshape(-1, 3), caps) > 0 for i in range(0, res, 8)]).reshape(res, res, res),
         "full": torch.ones(res, res, res, dtype=torch.bool, device=dev)}


def model(layers, width):
    torch.manual_seed(1)
    md = dict(num_early_layers=layers, num_late_layers=0, num_filters=width, num_input_channels=3, num_output_channels=1, num_input_channels_views=0,
              use_bias=True, pos_enc="none", pos_enc_basis=5, act_func="relu", fourier_sigma=5, num_img=1, device=dev, precision="f16s8")
    m = CPPN(md).to(dev)
    with torch.no_grad():
        m.output_linear[0].bias.fill_(-3.0)
    return m


def run(path, layers, width, grid):
    m = model(layers, width)
    kept = torch.zeros((), dtype=torch.int64, device=dev)
    cand = torch.zeros((), dtype=torch.int64, device=dev)
    if path == "one":
        opt = torch.optim.Adam(m.parameters(), lr=1e-4, fused=True)

        def it(o, d, t):
            opt.zero_grad(set_to_none=True)
            _, _, k = march_train_step_mse(m, grid, aabb, o, d, S, near, far, eps, thre, t)
            kept.add_(k)
            if k:
                opt.step()
    elif path in ("capt", "se"):
        opt = torch.optim.Adam(m.parameters(), lr=torch.tensor(1e-4, device=dev), fused=True, capturable=True)
        eng = m.engine
        flat_grad = torch.zeros(eng.param_count, device=dev)
        for p, g in zip(m._hip_params(), m._split_grad(flat_grad)):
            p.grad = g
        pixel, counts, skip = torch.ones(R, device=dev), torch.zeros(3, dtype=torch.int64, device=dev), torch.ones(1, device=dev)
        opt.found_inf = skip.view(())
        step = (far - near) / S

        def it(o, d, t):
            prepared = eng.prepare(m.flat_params, None, "f16s8")
            flat_grad.zero_()
            fn = eng.march_train_step_mse_capturable if path == "capt" else eng.march_train_step_mse_single_eval
            fn(prepared, o, d, t, 1.0 / R, flat_grad, "f16s8", aabb, near, far, step, eps, thre, grid_bits=grid.bits, grid_aabb=grid._aabb_host,
               grid_res=grid._res_host, pixel=pixel, counts=counts, skip=skip)
            torch.nn.functional.mse_loss(pixel, t)
            opt.step()
            kept.add_(counts[1])
            cand.add_(counts[0])
    else:
        opt = torch.optim.Adam(m.parameters(), lr=torch.tensor(1e-4, device=dev), fused=True, capturable=True)
        gtg = GridTrainGraph(m, opt, grid, aabb, R, S, near, far, eps, thre, single_eval=path == "se_graph")

        def it(o, d, t):
            _, _, counts = gtg.step(o, d, t)
            kept.add_(counts[1])
            cand.add_(counts[0])
    for i in range(20):
        it(*batches[i % 16])
    kept.zero_()
    cand.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        it(*batches[i % 16])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    return ms, int(kept) / iters, int(cand) / iters


rows = []
for layers, width in [(4, 128), (8, 256)]:
    for gname, mask in masks.items():
        grid = OccupancyGrid(roi_aabb=torch.tensor(aabb, device=dev), resolution=res).to(dev)
        grid._binary = mask
        occ = float(mask.float().mean()) * 100
        res_ = {p: run(p, layers, width, grid) for p in ("one", "capt", "graph", "se", "se_graph")}
        rows.append((f"{layers}x{width}", f"{gname} ({occ:.2f} % of cells)", res_))
        print(rows[-1], flush=True)
lines = ["| model | grid | candidates / it | kept samples / it | candidates : kept | one call (ms) | capturable, eager (ms) | graph replay (ms) "
         "| single eval, eager (ms) | single eval, graph (ms) | single eval vs capturable |", "|---|---|---|---|---|---|---|---|---|---|---|"]
for mdl, g, r in rows:
    nc, nk = r['se'][2], r['se'][1]
    lines.append(f"| {mdl} | {g} | {nc:.0f} | {nk:.0f} | {nc / max(nk, 1):.1f} | {r['one'][0]:.3f} | {r['capt'][0]:.3f} | {r['graph'][0]:.3f} | "
                 f"{r['se'][0]:.3f} | {r['se_graph'][0]:.3f} | {(1 - r['se'][0] / r['capt'][0]) * 100:+.1f} % |")
table = "\n".join(lines)
print(table)
if out_path:
    with open(out_path, "w") as f:
        f.write(f"# Grid training iteration: one call vs capturable vs graph replay vs single evaluation\n\n`python tools/grid_graph_iter.py <out.md> {iters}` on one MI355X: "
                f"{R} rays x {S} steps, Adam step included, {iters} timed iterations after 20 warm-up ones (wall time / iteration, the host "
                "synchronised only at both ends).\n\n" + table + "\n")
