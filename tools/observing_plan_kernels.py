#!/usr/bin/env python
"""Kernel time of the observing plan (pfsgnn_schedule_plan) at bench.py's shape
(16 x 2394 x 128, Fdim 10) and at its 30 %-dense general batch, beside the hard
schedule's k_schedule<10> and the budgeted rounding's k_budget_select /
ksl_budget_select from the same run, for scale.  The visits planned are the
budgeted rounding's, with decoder_e's last bias shifted (--shift, default 3) as
tools/budget_round_kernels.py does; N is cut to 60 % of what the schedule asks
on every other class, so that half the classes take the trim.  Every plan call
lists its exposures (seg_cap = the count), so each pass runs once per call.

Run it under the profiler, in a run of its own, then summarise the trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python tools/observing_plan_kernels.py [--reps 20]
    python tools/observing_plan_kernels.py --summarise DIR OUT.csv

One row per kernel and batch: calls (the first of each batch dropped as
warm-up), mean / median / min / max in microseconds, max - min; the rocprim
kernels of the plan-order sort (general batch) and of the seg_ptr scan are summed
per call; the last rows sum the means of the op's passes per batch.
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
SCALE = ("k_schedule<10>", "k_budget_select", "ksl_schedule<10>", "ksl_budget_select")
COMPLETE = ("k_plan_class<false>", "k_plan_fiber<false>", "k_plan_finish", "seg_ptr scan (rocprim)",
            "k_plan_fiber<true>")
GENERAL = ("k_plan_keys", "plan-order sort (rocprim)", "k_plan_class<true>",
           "k_plan_fiber_csr<false>", "k_plan_finish", "seg_ptr scan (rocprim)",
           "k_plan_fiber_csr<true>")


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
        form = dict(sp=lay.sp) if lay.sp is not None else dict(mode=lay.mode, perm=lay.perm)
        bu = be.schedule_budget(d, y, sc, sh, *dec, ci, scale, tt, nf, mode=lay.mode, perm=lay.perm)
        cip = ci.clone()
        # (at least 1: a class the schedule never visits keeps a finite completeness)
        cip[1, ::2] = torch.clamp(torch.floor(0.6 * bu[1][::2].float()), min=1.0) * nf
        plan = be.schedule_plan(d, cip, bu[0], tt, nf, **form)
        count = int(plan[-1][-1])
        seg_edge = torch.empty(count, dtype=torch.int32, device="cuda")
        seg_start = torch.empty(count, device="cuda")
        torch.cuda.synchronize()
        for _ in range(reps + 1):
            be.schedule(d, y, sc, sh, *dec, ci, scale, tt, nf, rounding=0, mode=lay.mode,
                        perm=lay.perm)
            be.schedule_budget(d, y, sc, sh, *dec, ci, scale, tt, nf, mode=lay.mode, perm=lay.perm,
                               out=bu)
            be.schedule_plan(d, cip, bu[0], tt, nf, seg_edge=seg_edge, seg_start=seg_start,
                             out=plan, **form)
        torch.cuda.synchronize()
        cut = plan[9]
        print(f"density {density}: E = {d.E}, {reps + 1} calls of each op; visits per edge "
              f"{bu[0].float().mean().item():.3f} in, {plan[0].float().mean().item():.3f} planned; "
              f"classes trimmed {int((cut > 0).sum())} of {cut.numel()}, visits cut "
              f"{int(cut.sum())}; exposures {count}; utility {bu[4].sum().item():.5g} -> "
              f"{plan[6].sum().item():.5g}; over-time fibers {int(plan[7].sum())}; idle time mean "
              f"{plan[3].mean().item():.3f}")


def summarise(src, dst):
    paths = sorted(glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {src}")
    rows = []
    for path in paths:
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [k for k in dict.fromkeys(COMPLETE + GENERAL) if "rocprim" not in k]
    times = {}
    last, batch = None, "complete"
    for r in rows:
        name = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        plan = next((k for k in names if k in name), None)
        scale = next((k for k in SCALE if k in name and (k.startswith("ksl_") or "ksl_" not in name)),
                     None)
        group = None
        if plan:
            if plan in ("k_plan_keys", "k_plan_class<true>"):
                batch = "general 30 %"
            elif plan == "k_plan_class<false>":
                batch = "complete"
            times.setdefault((plan, batch), []).append(us)
            last = plan
        elif scale:
            times.setdefault((scale, "sliced 30 %" if scale.startswith("ksl_") else "complete"),
                             []).append(us)
            last = None
        elif last in ("k_plan_keys", "plan-order sort (rocprim)"):
            # whatever runs between the keys and the class pass is the sort's (its
            # rocprim launches and the fill of its histogram)
            group = "plan-order sort (rocprim)"
        elif "rocprim" in name and last in ("k_plan_finish", "seg_ptr scan (rocprim)"):
            group = "seg_ptr scan (rocprim)"
        else:
            last = None
        if group:                                  # the launches of one sort / scan, summed
            t = times.setdefault((group, batch), [])
            if last == group:
                t[-1] += us
            else:
                t.append(us)
            last = group
    with open(dst, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kernel", "batch", "calls", "mean_us", "median_us", "min_us", "max_us",
                    "spread_us"])
        order = [(k, "sliced 30 %" if k.startswith("ksl_") else "complete") for k in SCALE]
        order += [(k, "complete") for k in COMPLETE] + [(k, "general 30 %") for k in GENERAL]
        total = {}
        for key in order:
            t = times.get(key, [])
            # the listing pass ran once per loop call: the last reps calls of every kernel
            # (set-up calls and the loop's first dropped)
            fill = ("k_plan_fiber<true>", "complete") if key[1] == "complete" else \
                ("k_plan_fiber_csr<true>", "general 30 %")
            keep = len(times.get(fill, [])) - 1
            t = t[max(0, len(t) - keep):] if keep > 0 else []
            if not t:
                continue
            w.writerow([key[0], key[1], len(t), f"{statistics.mean(t):.2f}",
                        f"{statistics.median(t):.2f}", f"{min(t):.2f}", f"{max(t):.2f}",
                        f"{max(t) - min(t):.2f}"])
            if key[0] not in SCALE:
                total[key[1]] = total.get(key[1], 0.0) + statistics.mean(t)
        for b, us in total.items():
            w.writerow(["pfsgnn_schedule_plan (sum of the means above)", b, "", f"{us:.2f}", "", "",
                        "", ""])
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
