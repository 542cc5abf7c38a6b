#!/usr/bin/env python
"""Kernel time of the hard schedule (pfsgnn_schedule) beside the loss forward it
is modelled on, at bench.py's shape (16 x 2394 x 128, Fdim 10): the complete
batch (k_schedule<10> / k_loss_fwd<10> with its per-edge time output) and a
30 %-dense general batch on the sliced kernels (ksl_schedule<10> /
ksl_loss_fwd<10>).  Both read the same lazy edge state (40 B/edge) and write
4 B/edge.

Run it under the profiler, in a run of its own, then summarise the trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python tools/hard_schedule_kernels.py [--reps 20]
    python tools/hard_schedule_kernels.py --summarise DIR OUT.csv

The summary has one row per kernel: calls (the first call of each is dropped as
warm-up), mean / median / min / max in microseconds, and the launch-to-launch
spread max - min.
"""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pfs-neural-net_amd")]

G, NF, NC, F = 16, 2394, 128, 10
KERNELS = ("k_loss_fwd<10>", "k_schedule<10>", "ksl_loss_fwd<10>", "ksl_schedule<10>",
           "k_schedule_finish")


def run(reps):
    import torch
    import pfsgnn
    from pfsgnn import config
    from pfsgnn.gnn import backend
    gen = torch.Generator().manual_seed(0)
    be = backend()
    xs = torch.arange(NF, dtype=torch.float).repeat(G).reshape(-1, 1)
    xt = torch.cat([torch.randint(2, 13, (G * NC, 1), generator=gen).float(),
                    torch.randint(1000, 100000, (G * NC, 1), generator=gen).float()], 1)
    for density in (1.0, 0.3):
        if density >= 1.0:
            e = torch.arange(G * NF * NC)
            ei = torch.stack([e // NC, (e // (NF * NC)) * NC + e % NC])
        else:
            keep = torch.rand(G, NF, NC, generator=gen) < density
            g, f, c = torch.nonzero(keep, as_tuple=True)
            p = torch.randperm(g.numel(), generator=gen)
            ei = torch.stack([(g * NF + f)[p], (g * NC + c)[p]])
        xe = 2.0 + 8.0 * torch.rand(ei.shape[1], F, generator=gen)
        torch.manual_seed(0)
        gnn = pfsgnn.GNN(B=1, Fdim=F, T=NC, F_s=1, F_t=2).cuda()
        gnn.eval()
        with torch.no_grad():
            out = gnn(pfsgnn.BipartiteData(ei, xs, xt, xe, torch.zeros(G, F)))
        model, d, lay, _, (y, sc, sh), _ = out._pf
        assert (lay.sp is None) == (density >= 1.0) and (lay.sp is None or lay.sp.sl is not None)
        P = model._flat_params()
        dec = [P["decoder_e.0.weight"], P["decoder_e.0.bias"], P["decoder_e.2.weight"],
               P["decoder_e.2.bias"]]
        ci = xt.cuda().t().contiguous()
        scale = float(config.TOTAL_TIME) / NC
        for _ in range(reps + 1):
            be.loss_fwd(d, y, sc, sh, *dec, ci, scale, 10.0, 0.3, 1, want_time=True)
            be.schedule(d, y, sc, sh, *dec, ci, scale, float(config.TOTAL_TIME),
                        float(config.NFIELDS), rounding=0, mode=lay.mode, perm=lay.perm)
        torch.cuda.synchronize()
        print(f"density {density}: E = {d.E}, {reps + 1} calls of each op")


def summarise(src, dst):
    paths = sorted(glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {src}")
    times = {k: [] for k in KERNELS}
    for path in paths:
        with open(path, newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        for r in rows:
            name = r["Kernel_Name"]
            for k in KERNELS:
                if k in name and (k != "k_schedule<10>" or "ksl_" not in name) and \
                        (k != "k_loss_fwd<10>" or "ksl_" not in name):
                    times[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    with open(dst, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kernel", "calls", "mean_us", "median_us", "min_us", "max_us", "spread_us"])
        for k in KERNELS:
            t = times[k]
            # the first call of each batch is warm-up; k_schedule_finish serves both batches
            nb = 2 if k == "k_schedule_finish" else 1
            if len(t) > nb:
                half = len(t) // nb
                t = [x for b in range(nb) for x in t[b * half + 1:(b + 1) * half]]
            if not t:
                continue
            w.writerow([k, len(t), f"{statistics.mean(t):.2f}", f"{statistics.median(t):.2f}",
                        f"{min(t):.2f}", f"{max(t):.2f}", f"{max(t) - min(t):.2f}"])
    print(open(dst).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--summarise", nargs=2, metavar=("DIR", "OUT"))
    a = ap.parse_args()
    if a.summarise:
        summarise(*a.summarise)
    else:
        run(a.reps)


if __name__ == "__main__":
    main()
