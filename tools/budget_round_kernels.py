#!/usr/bin/env python
"""Kernel time of the budgeted rounding (pfsgnn_schedule_budget) beside the hard
schedule (pfsgnn_schedule) at bench.py's shape (16 x 2394 x 128, Fdim 10): the
complete batch (k_budget_quot<10> + k_budget_select against k_schedule<10>) and
a 30 %-dense general batch on the sliced kernels (ksl_budget_quot<10> +
ksl_budget_select against ksl_schedule<10>); k_schedule_finish serves both ops.
decoder_e's last bias is shifted (--shift, default 3) so that an edge's time
reaches whole visits: on the untrained model every floor at NC = 128 is 0.

Run it under the profiler, in a run of its own, then summarise the trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python tools/budget_round_kernels.py [--reps 20]
    python tools/budget_round_kernels.py --summarise DIR OUT.csv

One row per kernel and batch: calls (the first of each batch dropped as
warm-up), mean / median / min / max in microseconds, max - min.
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
KERNELS = ("k_schedule<10>", "k_budget_quot<10>", "k_budget_select", "ksl_schedule<10>",
           "ksl_budget_quot<10>", "ksl_budget_select", "k_schedule_finish")


def run(reps, shift):
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
            gnn.decoder_e[2].bias += shift
            out = gnn(pfsgnn.BipartiteData(ei, xs, xt, xe, torch.zeros(G, F)))
        model, d, lay, _, (y, sc, sh), _ = out._pf
        assert (lay.sp is None) == (density >= 1.0) and (lay.sp is None or lay.sp.sl is not None)
        P = model._flat_params()
        dec = [P["decoder_e.0.weight"], P["decoder_e.0.bias"], P["decoder_e.2.weight"],
               P["decoder_e.2.bias"]]
        ci = xt.cuda().t().contiguous()
        scale, tt, nf = float(config.TOTAL_TIME) / NC, float(config.TOTAL_TIME), float(config.NFIELDS)
        for _ in range(reps + 1):
            fl = be.schedule(d, y, sc, sh, *dec, ci, scale, tt, nf, rounding=0, mode=lay.mode,
                             perm=lay.perm)
            bu = be.schedule_budget(d, y, sc, sh, *dec, ci, scale, tt, nf, mode=lay.mode,
                                    perm=lay.perm)
        torch.cuda.synchronize()
        ph = bu[8]
        print(f"density {density}: E = {d.E}, {reps + 1} calls of each op; fibers {ph.numel()}: "
              f"down phase {int((ph & 1).bool().sum())}, bumped {int((ph & 2).bool().sum())}, "
              f"refused {int((ph & 4).bool().sum())}; visits per edge floor "
              f"{fl[0].float().mean().item():.3f} budget {bu[0].float().mean().item():.3f}; "
              f"utility floor {fl[4].sum().item():.5g} budget {bu[4].sum().item():.5g}; over-time "
              f"fibers floor {int(fl[5].sum())} budget {int(bu[5].sum())}")


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
                if k in name and (k.startswith("ksl_") or "ksl_" not in name):
                    times[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    with open(dst, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kernel", "batch", "calls", "mean_us", "median_us", "min_us", "max_us",
                    "spread_us"])
        for k in KERNELS:
            t = times[k]
            # k_schedule_finish: per batch, the two ops' launches alternate
            parts = [("both ops, complete", t[:len(t) // 2]), ("both ops, sliced", t[len(t) // 2:])] \
                if k == "k_schedule_finish" else \
                [("sliced 30 %" if k.startswith("ksl_") else "complete", t)]
            for batch, t in parts:
                t = t[2:] if k == "k_schedule_finish" else t[1:]
                if t:
                    w.writerow([k, batch, len(t), f"{statistics.mean(t):.2f}",
                                f"{statistics.median(t):.2f}", f"{min(t):.2f}", f"{max(t):.2f}",
                                f"{max(t) - min(t):.2f}"])
    print(open(dst).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shift", type=float, default=3.0)
    ap.add_argument("--summarise", nargs=2, metavar=("DIR", "OUT"))
    a = ap.parse_args()
    if a.summarise:
        summarise(*a.summarise)
    else:
        run(a.reps, a.shift)


if __name__ == "__main__":
    main()
