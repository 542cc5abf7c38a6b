#!/usr/bin/env python
"""ms per epoch of the training loop, in one process:

  (a) eager    the loop body train.main had before TrainLoop: eager launches,
               loss_function(finaloutput=True) with its copies to the host,
               float(utility) every epoch, torch.save on every improvement;
  (b) step     the bare captured step of tests/test_gpu_graph.py / bench.py:
               fixed sharpness, no bookkeeping, one graph replay per epoch;
  (c) loop     pfsgnn.train.TrainLoop: the annealed schedule, history,
               best-tracking and best snapshot inside the replayed graph;
  (b') step+t  (b) with the loss forward also writing the per-edge time [E],
               which TrainLoop needs for the best state: (c) - (b') is what
               the three added launches and the device sharpness cost.

  (c+h) loop+h (c) with ``track_hard=True`` (--track-hard): pfsgnn_schedule, the
               hard history row and the second copy_if inside the replayed
               graph; (c+h) - (c) is the epoch cost of tracking the integer
               objective.
  (c+b) loop+b (c) with ``track_hard="budget"`` (--track-hard budget, beside
               (c+h)): pfsgnn_schedule_budget in place of pfsgnn_schedule --
               the best *executable* schedule; (c+b) - (c+h) is what the
               selection pass adds to the floor evaluation.

Runs are interleaved (a, b, c, b', a, b, c, b', ...); each run times EPOCHS epochs
between two device syncs; reported: the median over RUNS runs and their spread.
Shapes: the reference's (1 x 2000 x 12, B = 3) and bench.py's (16 x 2394 x 128,
B = 8).

    python tools/train_loop_bench.py [--shape ref|bench|both] [--runs 5] [--epochs 200]
                                     [--track-hard [floor|budget]]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pfs-neural-net_amd")]

SHAPES = {"ref": (1, 2000, 12, 3), "bench": (16, 2394, 128, 8)}
FDIM, SHARPS, MIN_SHARP, PCLASS, PFIBER, LR = 10, [0.0, 20.0], 5.0, 0.1, 0.1, 5e-4


def make_batch(G, NF, NC):
    import pfsgnn
    gen = torch.Generator().manual_seed(1234)
    Ti = torch.randint(2, 13, (G * NC, 1), generator=gen).float()
    Ni = torch.randint(1000, 100000, (G * NC, 1), generator=gen).float()
    class_info = torch.cat([Ti, Ni], 1)
    x_s = torch.arange(NF, dtype=torch.float).repeat(G).reshape(-1, 1)
    e = torch.arange(G * NF * NC)
    edge_index = torch.stack([e // NC, (e // (NF * NC)) * NC + e % NC])
    x_e = 2.0 + 8.0 * torch.rand(G * NF * NC, FDIM, generator=gen)
    data = pfsgnn.BipartiteData(edge_index, x_s, class_info, x_e, torch.zeros(G, FDIM))
    return data, class_info.cuda()


def make_model(NC, B, capturable):
    import pfsgnn
    torch.manual_seed(0)
    gnn = pfsgnn.GNN(B=B, Fdim=FDIM, T=NC, F_s=1, F_t=2).cuda()
    gnn.train()
    return gnn, pfsgnn.FusedAdam(gnn.parameters(), lr=LR, capturable=capturable)


class Eager:
    """(a): train.main's loop body before TrainLoop."""

    def __init__(self, shape, nepochs):
        from pfsgnn.train import loss_function
        G, NF, NC, B = shape
        self.loss_function, self.nepochs, self.epoch, self.best = loss_function, nepochs, 0, 0.0
        self.data, self.ci = make_batch(G, NF, NC)
        self.gnn, self.opt = make_model(NC, B, False)
        self.tmp = tempfile.TemporaryDirectory()     # removed with the object
        self.path = os.path.join(self.tmp.name, "model_gnn_0.pth")

    def run(self, n):
        gnn, opt = self.gnn, self.opt
        for epoch in range(self.epoch, self.epoch + n):
            gnn.zero_grad()
            out = gnn(self.data)
            sharp = SHARPS[0] + (SHARPS[1] - SHARPS[0]) * epoch / self.nepochs
            loss, utility, comp, _, fiber_time, t, variance = self.loss_function(
                out, self.ci, pclass=PCLASS, pfiber=PFIBER, sharpness=sharp, finaloutput=True)
            loss.backward()
            opt.step()
            if float(utility.detach()) > self.best and sharp > MIN_SHARP:
                self.best = float(utility.detach())
                torch.save({"epoch": epoch, "model_state": gnn.state_dict(),
                            "optim_state": opt.state_dict()}, self.path)
        self.epoch += n


class Step:
    """(b): the bare captured step (fixed sharpness, device seed, capturable Adam)."""

    def __init__(self, shape, nepochs, want_time=False):
        from pfsgnn.train import _loss_apply
        G, NF, NC, B = shape
        data, ci = make_batch(G, NF, NC)
        gnn, opt = make_model(NC, B, True)
        seed = torch.full((), 0, dtype=torch.int64, device="cuda")

        def step():
            seed.add_(1)
            gnn.zero_grad()
            # loss_function(..., finaloutput=False)'s launches; want_time adds the [E] store
            loss = _loss_apply(gnn(data), ci, PCLASS, PFIBER, 10.0, want_time, None, seed, 0.3)[2][0]
            loss.backward()
            opt.step()
            return loss

        step()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = step()
        # the replays read and write the model, the optimizer state, the batch and
        # the seed at their captured addresses: they live as long as the graph.  So
        # do this batch's cached layout and canonical edge tensor, which the other
        # models of the process could evict from gnn's caches (TrainLoop does the same)
        from pfsgnn import gnn as gmod
        self.keep = (gnn, opt, data, ci, seed, step,
                     gmod._LAYOUT_CACHE.d.get(id(data.edge_index)),
                     gmod._EDGE_CACHE.d.get(id(data.x_e)))

    def run(self, n):
        for _ in range(n):
            self.graph.replay()


class Loop:
    """(c): TrainLoop."""

    def __init__(self, shape, nepochs, track_hard=False):
        from pfsgnn.train import TrainLoop
        G, NF, NC, B = shape
        data, ci = make_batch(G, NF, NC)
        gnn, opt = make_model(NC, B, True)
        self.loop = TrainLoop(gnn, opt, data, ci, nepochs, SHARPS, MIN_SHARP, PCLASS, PFIBER, seed=0,
                              track_hard=track_hard)
        self.loop.run(2)            # the eager and the side-stream epoch, and the capture

    def run(self, n):
        self.loop.run(n)


def measure(name, shape, runs, epochs, track_hard=False):
    nepochs = runs * epochs + 8
    variants = [("eager", Eager(shape, nepochs)), ("step", Step(shape, nepochs)),
                ("loop", Loop(shape, nepochs)), ("step+t", Step(shape, nepochs, want_time=True))]
    if track_hard:
        variants.append(("loop+h", Loop(shape, nepochs, track_hard=True)))
    if track_hard == "budget":
        variants.append(("loop+b", Loop(shape, nepochs, track_hard="budget")))
    for _, v in variants:           # one untimed pass each
        v.run(3)
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in variants}
    for _ in range(runs):
        for k, v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v.run(epochs)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / epochs)
    G, NF, NC, B = shape
    print(f"shape {name}: {G} x {NF} x {NC}, B = {B}; {runs} interleaved runs of {epochs} epochs, "
          f"ms per epoch")
    med, tags = {}, {"eager": "a", "step": "b", "loop": "c", "step+t": "b'", "loop+h": "c+h",
                 "loop+b": "c+b"}
    for k, _ in variants:
        med[k] = statistics.median(ms[k])
        print(f"  ({tags[k]:3s}) {k:6s} median {med[k]:8.4f}  min {min(ms[k]):8.4f}  "
              f"max {max(ms[k]):8.4f}  runs {' '.join(f'{x:.4f}' for x in ms[k])}")
    spread = max(ms["step"]) - min(ms["step"])
    print(f"  (c) - (b) = {1e3 * (med['loop'] - med['step']):8.2f} us per epoch; run-to-run spread "
          f"of (b) {1e3 * spread:.2f} us; (c) - (b') = {1e3 * (med['loop'] - med['step+t']):.2f} us; "
          f"(a) / (c) = {med['eager'] / med['loop']:.2f}x")
    if track_hard:
        hl = variants[4][1].loop
        hh, hb = hl.history(), hl.hard_best()
        assert np.isfinite(hh["hard_objective"]).all(), "TrainLoop's hard_objective is not finite"
        print(f"  (c+h) - (c) = {1e3 * (med['loop+h'] - med['loop']):8.2f} us per epoch; run-to-run "
              f"spread of (c) {1e3 * (max(ms['loop']) - min(ms['loop'])):.2f} us; hard objective "
              f"{hh['hard_objective'][2:].min():.6g} .. {hh['hard_objective'][2:].max():.6g}, "
              f"over-time fibers {hh['hard_overtime'][2:].min()} .. {hh['hard_overtime'][2:].max()}, "
              f"best hard epoch {hb['epoch']} utility {hb['utility']:.6g}")
    if track_hard == "budget":
        bl = variants[5][1].loop
        bh, bb = bl.history(), bl.hard_best()
        assert np.isfinite(bh["hard_objective"]).all(), "the budget hard_objective is not finite"
        print(f"  (c+b) - (c) = {1e3 * (med['loop+b'] - med['loop']):8.2f} us per epoch; (c+b) - (c+h) "
              f"= {1e3 * (med['loop+b'] - med['loop+h']):.2f} us; run-to-run spread of (c+b) "
              f"{1e3 * (max(ms['loop+b']) - min(ms['loop+b'])):.2f} us; budget hard objective "
              f"{bh['hard_objective'][2:].min():.6g} .. {bh['hard_objective'][2:].max():.6g}, "
              f"over-time fibers {bh['hard_overtime'][2:].min()} .. {bh['hard_overtime'][2:].max()}, "
              f"best hard epoch {bb['epoch']} utility {bb['utility']:.6g}")
    hist = variants[2][1].loop
    b = hist.best()
    h = hist.history()
    for k in ("losses", "objective", "variances", "completions"):
        assert np.isfinite(h[k]).all(), f"TrainLoop's {k} are not finite"
    for k, v in variants:
        if k.startswith("step"):
            assert torch.isfinite(v.loss).all(), f"the bare step's loss ({k}) is not finite"
    obj = h["objective"][2:]
    print(f"  loop: epochs {hist.epoch}, final sharpness {hist.sharpness():.4f}, objective "
          f"{obj.min():.6g} .. {obj.max():.6g}, best epoch {b['epoch']} utility {b['utility']:.6g}; "
          f"eager: best utility {variants[0][1].best:.6g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["ref", "bench", "both"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--track-hard", nargs="?", const="floor", default=False,
                    choices=["floor", "budget"],
                    help="add (c+h): TrainLoop(track_hard=True), and report (c+h) - (c); "
                         "'budget' also adds (c+b): track_hard='budget'")
    a = ap.parse_args()
    print(f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    for name in (["ref", "bench"] if a.shape == "both" else [a.shape]):
        measure(name, SHAPES[name], a.runs, a.epochs, a.track_hard)


if __name__ == "__main__":
    main()
