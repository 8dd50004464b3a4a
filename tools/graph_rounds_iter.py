#!/usr/bin/env python3
"""Iterations per second and host-side issue time per iteration of the training driver's grid loop (nerf/run_nerf_acc.py) at the
reference's 5 625 rays x 300 steps, 4x128, f16s8, on the trained-like and the full 128^3 grid of tools/grid_graph_iter.py, two ways:
  loop   - what --graph --graph-grid-update runs per iteration: RayBatchSampler.draw, GridUpdateGraph.step, GridTrainGraph.step, the
           torch.where on the loss, the sample total, lr.fill_
  rounds - what --graph-rounds runs: render.GridTrainRoundGraph.run (one graph launch per 16 iterations)
Both start at iteration 256 (past the warm-up of the grids: the steady state of a long run) and compute the same numbers.  The refresh
threshold is set above a fresh model's occupancy and the occupied cells start at a large occupancy, so every refresh does its full work
(draw, evaluation, decay / EMA, threshold) but leaves the grid as it is - the march sees the same grid for the whole run.

Per run and grid: wall time per iteration with the host synchronised at both ends only, and the part of it the host spends issuing work
(the time at which the Python loop has issued everything, before the final synchronisation).

usage: graph_rounds_iter.py --mode loop|rounds [--iters N] [--label TEXT] [--append runs.jsonl]
       graph_rounds_iter.py --report runs.jsonl out.md      (label "parent" = the baseline whose min-max spread is the noise band)"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

R, S, near, far, eps, thre = 5625, 300, 1400.0, 1600.0, 1e-2, 1e-4
aabb = [-100.0, -100, -100, 100, 100, 100]
START, WARM = 256, 64
LR0, DECAY, DECAY_STEPS = 1e-4, 0.1, 500 * 1000
KEEP_THRE = 0.5      # refresh threshold: above sigmoid(model) of the fresh model, below the occupied cells' occupancy


def report(src, dst):
    runs = [json.loads(l) for l in open(src)]
    lines = ["| grid | path | runs | it/s: median (min - max) | ms / it: median (min - max) | host issue ms / it: median (min - max) |", "|---|---|---|---|---|---|"]
    verdict = []
    for grid in dict.fromkeys(r["grid"] for r in runs):
        med = {}
        for label in dict.fromkeys(r["label"] for r in runs):
            rs = [r for r in runs if r["grid"] == grid and r["label"] == label]
            if not rs:
                continue
            f = lambda key, fmt: (f"{statistics.median(r[key] for r in rs):{fmt}} ({min(r[key] for r in rs):{fmt}} - {max(r[key] for r in rs):{fmt}})")
            lines.append(f"| {grid} | {label} ({rs[0]['mode']}) | {len(rs)} | {f('it_per_s', '.0f')} | {f('ms_per_it', '.4f')} | {f('issue_ms_per_it', '.4f')} |")
            med[label] = (statistics.median(r["it_per_s"] for r in rs), min(r["it_per_s"] for r in rs), max(r["it_per_s"] for r in rs))
        if "parent" in med:
            p = med["parent"]
            for label, m in med.items():
                if label != "parent":
                    outside = m[0] > p[2] or m[0] < p[1]
                    verdict.append(f"- {grid}: {label} / parent = {m[0] / p[0]:.3f} (medians, it/s); the parent's band is {p[1]:.0f} - {p[2]:.0f} it/s "
                                   f"(+-{(p[2] - p[1]) / 2 / p[0] * 100:.1f} % of its median): the {label} median lies {'OUTSIDE' if outside else 'inside'} it")
    with open(dst, "w") as f:
        f.write("# Grid training loop: one graph launch per iteration vs one per 16 iterations\n\n"
                f"`python tools/graph_rounds_iter.py --mode loop|rounds` on one MI355X, {runs[0]['iters']} timed iterations per run from iteration "
                f"{START} after {WARM} warm-up ones: {R} rays x {S} steps, 4x128, f16s8, both grid refreshes every 16th iteration, Adam and the "
                "learning-rate update included.  `parent (loop)`: the per-iteration loop of `--graph --graph-grid-update` on the parent "
                "commit; `rounds`: `--graph-rounds` (render.GridTrainRoundGraph).  Wall time, the host synchronised at both ends of a run only; "
                "host issue time = the time at which the Python loop has issued everything.\n\n" + "\n".join(lines) + "\n\n" + "\n".join(verdict) + "\n")
    print("\n".join(lines + verdict))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["loop", "rounds"])
    ap.add_argument("--iters", type=int, default=1600)
    ap.add_argument("--label", default=None)
    ap.add_argument("--append", default=None)
    ap.add_argument("--report", nargs=2, default=None)
    args = ap.parse_args()
    if args.report:
        return report(*args.report)
    if args.mode is None:
        ap.error("--mode or --report")
    import torch
    from nerf_for_angiography_amd.model.CPPN import CPPN
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    from nerf_for_angiography_amd.phantomdata.helpers import capsule_tree, capsule_mu
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    NT = 90 * 100 * 100
    tab_o = torch.randn(NT, 3, device=dev) * 3 + torch.tensor([0, 0, 1500.0], device=dev)
    tab_d = torch.nn.functional.normalize(torch.randn(NT, 3, device=dev) * 0.03 + torch.tensor([0, 0, -1.0], device=dev), dim=-1)
    tab_p, tab_w = torch.rand(NT, device=dev), torch.rand(NT, device=dev) + 0.05
    res = 128
    c = (torch.stack(torch.meshgrid(*[torch.arange(res, device=dev)] * 3, indexing="ij"), -1).float() + 0.5) / res * 200 - 100
    caps = capsule_tree(levels=5, seed=0)
    caps[:, 6] += 4.0
    masks = {"trained-like": torch.cat([capsule_mu(c[i:i + 8].reshape(-1, 3), caps) > 0 for i in range(0, res, 8)]).reshape(res, res, res),
             "full": torch.ones(res, res, res, dtype=torch.bool, device=dev)}
    n_all = START + WARM + args.iters
    for gname, mask in masks.items():
        torch.manual_seed(1)
        md = dict(num_early_layers=4, num_late_layers=0, num_filters=128, num_input_channels=3, num_output_channels=1, num_input_channels_views=0,
                  use_bias=True, pos_enc="none", pos_enc_basis=5, act_func="relu", fourier_sigma=5, num_img=1, device=dev, precision="f16s8")
        m = CPPN(md).to(dev)
        with torch.no_grad():
            m.output_linear[0].bias.fill_(-3.0)
        grids = []
        for s in (0, 1):
            g = OccupancyGrid(roi_aabb=torch.tensor(aabb, device=dev), resolution=res, seed=s).to(dev)
            g.train()
            g.occs.copy_(mask.reshape(-1).float() * 1e6)
            g._binary = mask
            grids.append(g)
        lr = torch.tensor(LR0 * DECAY ** ((START - 1) / DECAY_STEPS), device=dev)
        opt = torch.optim.Adam(m.parameters(), lr=lr, fused=True, capturable=True)
        glist = [(grids[0], KEEP_THRE), (grids[1], KEEP_THRE)]
        if args.mode == "rounds":
            from nerf_for_angiography_amd.render import GridTrainRoundGraph, lr_decay_table
            rg = GridTrainRoundGraph(m, opt, glist, (tab_o, tab_d, tab_p, tab_w), aabb, R, S, near, far, eps, thre, seed=0,
                                     lr_table=lr_decay_table(LR0, DECAY, DECAY_STEPS, n_all), start_iter=START)

            def advance(i0, n):
                rg.run(n)

            totals = lambda: (int(rg.n_marched), float(rg.last_loss))
        else:
            from nerf_for_angiography_amd.engine import RayBatchSampler
            from nerf_for_angiography_amd.render import GridTrainGraph, GridUpdateGraph
            sampler = RayBatchSampler(tab_o, tab_d, tab_p, tab_w, R, seed=0, prefetch=16)
            gtg = GridTrainGraph(m, opt, grids[0], aabb, R, S, near, far, eps, thre)
            upd = GridUpdateGraph(m, glist)
            state = dict(loss=torch.tensor(float("nan"), device=dev), n=torch.zeros((), dtype=torch.int64, device=dev))

            def advance(i0, n):
                for i in range(i0, i0 + n):      # the driver's loop body
                    o, d, p, _ = sampler.draw(i)
                    upd.step(i)
                    loss_k, _, counts = gtg.step(o, d, p)
                    state["loss"] = torch.where(gtg.skip[0] > 0, state["loss"], loss_k)
                    state["n"] += counts[1]
                    new_lr = LR0 * (DECAY ** (i / DECAY_STEPS))
                    for group in opt.param_groups:
                        group["lr"].fill_(new_lr)

            totals = lambda: (int(state["n"]), float(state["loss"]))
        advance(START, WARM)
        torch.cuda.synchronize()
        n0 = totals()[0]
        t0 = time.perf_counter()
        advance(START + WARM, args.iters)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        n1, loss = totals()
        rec = dict(label=args.label or args.mode, mode=args.mode, grid=gname, iters=args.iters, ms_per_it=(t2 - t0) / args.iters * 1e3,
                   issue_ms_per_it=(t1 - t0) / args.iters * 1e3, it_per_s=args.iters / (t2 - t0), kept_per_it=(n1 - n0) / args.iters, last_loss=loss,
                   occupied=int(grids[0]._binary_u8.sum()), occupied_at_start=int(mask.sum()))
        print(json.dumps(rec), flush=True)
        if args.append:
            with open(args.append, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
