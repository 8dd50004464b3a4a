#!/usr/bin/env python3
"""ms per refresh of BOTH occupancy grids (nerf/run_nerf_acc.py:285-286, acc_update_n_step for the grid and the vessel grid) at 128^3, three ways:
  eager   - OccupancyGrid.every_n_step (torch draw: torch.nonzero + len() synchronise the host; sigmoid(model) through the module)
  refresh - OccupancyGrid.refresh issued eagerly (afx_grid_refresh: the cells drawn on the device, no host synchronisation)
  graph   - render.GridUpdateGraph: re-tiling + both refreshes captured once and replayed
in the warm-up phase (every cell) and after it (num_cells/4 uniform + num_cells/4 occupied cells), on a trained-like grid (~0.5 % of the
cells occupied) and on a full grid, for 4x128 and 8x256 (f16s8).  Each update is timed on its own by device events around it (a host wait
inside it shows as GPU idle time between them); the grid state is restored before every update, outside the events.  Prints a markdown table
(and writes it to the path given as the first argument).  usage: grid_refresh_iter.py [out.md [updates]]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from nerf_for_angiography_amd.model.CPPN import CPPN
from nerf_for_angiography_amd.render import GridUpdateGraph
from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid

dev = torch.device("cuda:0")
out_path = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None
updates = int(sys.argv[2]) if len(sys.argv) > 2 else 200
res, aabb = 128, [-100.0, -100, -100, 100, 100, 100]
THRE = (1e-4, 5e-2)      # the driver's two grids

g = torch.Generator(device=dev).manual_seed(0)
masks = {"trained-like": torch.rand(res ** 3, device=dev, generator=g) < 0.005, "full": torch.ones(res ** 3, dtype=torch.bool, device=dev)}


def model(layers, width):
    torch.manual_seed(0)
    md = dict(num_early_layers=layers, num_late_layers=0, num_filters=width, num_input_channels=3, num_output_channels=1,
              num_input_channels_views=0, use_bias=True, pos_enc="none", pos_enc_basis=5, act_func="relu", fourier_sigma=5, num_img=1,
              device=dev, precision="f16s8")
    m = CPPN(md).to(dev)
    with torch.no_grad():
        m.output_linear[0].bias.fill_(-5.0)
    return m


def grids(mask):
    out = []
    for s in (0, 1):
        gr = OccupancyGrid(roi_aabb=torch.tensor(aabb, device=dev), resolution=res, seed=s).to(dev)
        gr.train()
        gr.occs.copy_(mask.float() * 0.5)
        gr._binary = mask
        out.append(gr)
    return out


def snapshot(gs):
    return [(gr.occs.clone(), gr._binary_u8.clone(), gr._bits.clone()) for gr in gs]


def restore(gs, snap):
    for gr, (o, b, w) in zip(gs, snap):
        gr.occs.copy_(o); gr._binary_u8.copy_(b); gr._bits.copy_(w)


def time_updates(fn, gs, snap, steps):
    ms = []
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in steps]
    for (a, b), step in zip(ev, steps):
        restore(gs, snap)
        torch.cuda.synchronize()
        a.record()
        fn(step)
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]


rows = []
for layers, width in ((4, 128), (8, 256)):
    m = model(layers, width)
    for kind, mask in masks.items():
        gs = grids(mask)
        snap = snapshot(gs)
        upd = GridUpdateGraph(m, list(zip(gs, THRE)))
        for phase, steps in (("warm-up", [16 * k for k in range(1, 16)]), ("post-warm-up", [256 + 16 * k for k in range(updates)])):
            if phase == "warm-up":
                steps = (steps * (updates // len(steps) + 1))[:updates]

            def eager(step):
                for gr, t in zip(gs, THRE):
                    gr.every_n_step(step, lambda x: torch.sigmoid(m(x)), occ_thre=t)

            def refresh(step):
                for gr, t in zip(gs, THRE):
                    gr.refresh(m, step, occ_thre=t)

            res_ms = {}
            for name, fn in (("eager every_n_step", eager), ("eager refresh", refresh), ("graph replay", upd.step)):
                fn(steps[0]); torch.cuda.synchronize()      # warm-up of the path (captures the graph)
                res_ms[name] = time_updates(fn, gs, snap, steps)
            restore(gs, snap)
            n_occ = int(mask.sum())
            for name, (med, p10, p90) in res_ms.items():
                rows.append(f"| {layers}x{width} | {kind} ({n_occ} occupied) | {phase} | {name} | {med:.3f} | {p10:.3f} - {p90:.3f} |")
            print("\n".join(rows[-3:]), flush=True)

table = ["| model | grid | phase | path | median ms per update of both grids | p10 - p90 |", "|---|---|---|---|---|---|"] + rows
print("\n".join(table))
if out_path:
    with open(out_path, "w") as f:
        f.write(f"{updates} updates per row, device events around each update (grid state restored before each, outside the events)\n\n")
        f.write("\n".join(table) + "\n")
