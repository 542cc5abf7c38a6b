"""Benchmark: training-step edges/sec on batches of 2394-fiber x 128-class
complete bipartite graphs (BASELINE.json metric); with --full also the HBM
roofline of the dominant kernel and the CPU oracle timed on the host.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--graphs G] [--blocks B]
                    [--fibers NF] [--classes NC] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps, writes the last step's
results if --dump-outputs is given, and prints the JSON line (``roofline`` and
``cpu_baseline`` null).  --full adds every other measurement after the timed
region: the per-kernel in-graph and eager durations and the roofline, the other
edge paths (``alt_paths``), the CPU baseline, and at N > 1 the eager tail
timings and the rank-consistency check.

Default workload: BASELINE.json's metric config (16 graphs of 2394x128 per
GPU, 8 blocks).  configs[2] of BASELINE.json (a batch of 256 synthetic
2394x16 graphs) is ``--classes 16 --graphs 256``.

One process per GPU (torchrun for N > 1).  Each rank trains on its own G
synthetic graphs (weak scaling); gradients are mean-all-reduced over RCCL once
per step.  A step is the reference training step (train.py:133-141):
zero_grad, GNN forward, loss_function (finaloutput=False), backward,
all-reduce, Adam.  Rank 0 prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "pfs-neural-net_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

NF, NC, FDIM = 2394, 128, 10      # overridden by --fibers / --classes
# what each edge path computes in (include/pfsgnn.h).  The
# node level (per-fiber / per-class MLPs, pf::node_x3) runs its forward in fp32
# on every path and its gradient chains and weight gradients in bf16x3 on every
# path but the exact-fp32 ones (mfma32, valu, bf16y); reductions, BatchNorm
# statistics, Adam and the loss are fp32 everywhere.
_NODE_X3 = "; node level: fp32 forward, bf16x3 gradient chains and weight gradients"
_NODE_F32 = "; node level fp32"
PRECISION = {
    "mfma": "fp32 MFMA forward contractions and recompute; backward gradient chains and weight "
            "gradients bf16x3 (~2^-16 relative per product); fp32 accumulation and edge state"
            + _NODE_X3,
    "mfma32": "every per-edge contraction exact fp32 MFMA (v_mfma_f32_16x16x4_f32), the weight "
              "gradients' outer products included; fp32 accumulation and edge state" + _NODE_F32,
    "valu": "fp32 fmaf chains on the vector ALU; weight gradients exact fp32 MFMA "
            "(v_mfma_f32_16x16x4_f32)" + _NODE_F32,
    "bf16y": "mfma32 arithmetic with the edge state rounded to bf16" + _NODE_F32,
    "bf16m": "every per-edge contraction a single bf16 MFMA, fp32 accumulation and edge state"
             + _NODE_X3,
    "bf16": "single-bf16 MFMA contractions and bf16 edge state" + _NODE_X3,
    "bf16x6": "forward contractions and their backward recompute on bf16 MFMAs with three-way "
              "split operands (hi+mid+lo, six products: fp32-class, ~2^-24 relative); backward "
              "gradient chains and weight gradients bf16x3; fp32 accumulation and edge state"
              + _NODE_X3,
    "bf16x3": "every per-edge contraction (forward, backward recompute, gradient chains, weight "
              "gradients) on bf16 MFMAs with split hi+lo operands (bf16x3, ~2^-16 relative per "
              "product); fp32 accumulation, edge state and loss" + _NODE_X3,
}
# Whether a path meets the fp32 parity bar (tests/test_gpu_parity.py: every
# tensor within max(16 x the fp32 oracle's error, TOL_REL x its scale) of the
# fp64 oracle) on EVERY parity case -- the BASELINE configs[4] requirement.
# bf16x3 passes at the bench geometry (0.28 of the bar, profiles/r05i_precision.json)
# but misses it on the small parity graphs (up to 8.3x on encoder gradients,
# profiles/r05a_bf16x3_parity_report.log), so it is not a configs[4] answer.
MEETS_FP32_TOL = {"mfma": True, "mfma32": True, "valu": True, "bf16x6": True, "bf16x3": False,
                  "bf16y": False, "bf16m": False, "bf16": False}
# the arithmetic each edge path computes in (`precision` spells it out): the
# default path's backward products are split-bf16 (bf16x3), its forward fp32
DTYPE = {"mfma": "f32 (bf16x3 backward products)", "mfma32": "f32", "valu": "f32",
         "bf16y": "f32 (bf16 edge state)", "bf16m": "bf16", "bf16": "bf16",
         "bf16x6": "f32 (split-bf16 products: bf16x6 forward, bf16x3 backward)", "bf16x3": "bf16x3"}
HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
F32_MFMA_PEAK_TFS = 157.3  # MI355X_MICROARCH.md: dense fp32-input MFMA (= fp32 vector peak)
BF16_MFMA_PEAK_TFS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (no sparsity)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--graphs", type=int, default=16, help="graphs per GPU")
    ap.add_argument("--fibers", type=int, default=2394)
    ap.add_argument("--classes", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=8, help="message-passing rounds")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--no-graph", action="store_true",
                    help="launch every kernel from Python instead of replaying a captured HIP graph")
    # The headline runs BASELINE configs[4]'s arithmetic: the per-edge GEMMs on
    # bf16 MFMAs at fp32 tolerance -- bf16x6 (three-way split operands, the six
    # products down to ~2^-18: fp32-class forward; gradient chains bf16x3), held
    # to the fp32 parity bar on every parity case (tests/test_gpu_parity.py
    # PATHS).  The library's default, mfma (fp32 MFMA forward), is measured
    # beside it in alt_paths.
    ap.add_argument("--edge-path", default=os.environ.get("PFSGNN_EDGE_PATH", "bf16x6"),
                    help="per-edge kernel precision: bf16x6 (bench default: BASELINE configs[4], "
                         "bf16 MFMA edge GEMMs at fp32 tolerance), mfma (the library default: fp32 "
                         "forward, bf16x3 gradient chains), mfma32, valu, bf16x3, bf16y, bf16m, bf16")
    ap.add_argument("--alt-paths", default="mfma,bf16x3,mfma32",
                    help="other edge paths whose step rate is measured after the headline "
                         "one (N=1, graph replay; reported in alt_paths; '' for none)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the per-kernel durations and the "
                         "roofline, the --alt-paths, the CPU baseline (--no-cpu-baseline, "
                         "--cpu-seconds) and, at N > 1, the eager tail and the rank consistency; "
                         "without it those options have no effect")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (loss, gradients, parameters, "
                         "BatchNorm buffers) to DIR/<name>.npy")
    return ap.parse_args()


def dump_outputs(dirname, loss, gnn):
    """What a caller of the timed step holds after its last call, as
    DIR/<name>.npy: the loss the step returns (float32), the gradients its
    backward left and the parameters its Adam update left (float32, each
    flattened in named_parameters() order), and the BatchNorm buffers its
    forward updated (float64: running statistics and batch counts, in
    named_buffers() order).  A few hundred KB in all; reads only."""
    os.makedirs(dirname, exist_ok=True)
    params = list(gnn.parameters())
    grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in params]
    arrays = {
        "loss": loss.detach().reshape(1).float(),
        "gradients": torch.cat([g.detach().reshape(-1).float() for g in grads]),
        "parameters": torch.cat([p.detach().reshape(-1).float() for p in params]),
        "buffers": torch.cat([b.detach().reshape(-1).double() for b in gnn.buffers()]),
    }
    for name, t in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), t.cpu().numpy())


def make_batch(G, rank, device):
    """G synthetic graphs shaped like train.py's (train.py:88-104)."""
    import pfsgnn
    gen = torch.Generator().manual_seed(1234 + rank)
    Ti = torch.randint(2, 13, (G * NC, 1), generator=gen).float()
    Ni = torch.randint(1000, 100000, (G * NC, 1), generator=gen).float()
    class_info = torch.cat([Ti, Ni], 1)
    x_s = torch.arange(NF, dtype=torch.float).repeat(G).reshape(-1, 1)
    e = torch.arange(G * NF * NC)
    edge_index = torch.stack([e // NC, (e // (NF * NC)) * NC + e % NC])
    x_e = 2.0 + 8.0 * torch.rand(G * NF * NC, FDIM, generator=gen)
    x_u = torch.zeros(G, FDIM)
    data = pfsgnn.BipartiteData(edge_index, x_s, class_info, x_e, x_u)
    return data, class_info.to(device)


# per-edge algorithmic HBM bytes of each main kernel
def kernel_bytes_per_edge(F, first_block_excluded=False):
    f = 4 * F
    m = 4 if 2 * F <= 32 else 0   # TModel's LeakyReLU mask, 1 byte per (edge, lane group)
    return {
        "edge_mlp_fwd": 2 * f,   # read xe, write y
        "source_fwd": f,         # read y
        "target_fwd": f + m,     # read y; write the TModel mask
        "target_bwd": f + m,     # read y, the mask
        "source_bwd": 3 * f + m,  # read y, g_next, the mask; write g_tot
        "edge_mlp_bwd": 4 * f,   # read g_tot, y, xe; write g_xe (blocks > 0)
        "loss_fwd": f,
        "loss_bwd": 2 * f,
    }


# per-edge algorithmic FLOPs (2 per real multiply-add of the unpadded layer
# shapes), split by the arithmetic they run in: "fwd" the
# forward contractions (and a backward kernel's recompute of them), "grad" the
# gradient chains, "wg" the weight gradients (sums over edges of outer
# products), "valu" the elementwise work (activations, moments, BatchNorm
# affines).  H = 4F hidden units of the EdgeModel MLP, C = 2F of the S/T
# message MLPs.  source_bwd includes TModel's input-gradient chain (its
# pre-activation comes from target_fwd's mask, not recomputed); edge_mlp_bwd's
# input-gradient product is absent in block 0.
def kernel_flops_split(F, B):
    H, C = 4 * F, 2 * F
    return {
        "edge_mlp_fwd": {"fwd": 2 * (H * F + F * H), "valu": 4 * H},
        "source_fwd": {"fwd": 2 * (C * F + C * C), "valu": 16 * C},
        "target_fwd": {"fwd": 2 * C * F, "valu": 4 * C},
        "target_bwd": {"wg": 2 * C * F, "valu": 3 * C},
        "source_bwd": {"fwd": 2 * (C * F + C * C), "grad": 2 * (C * C + F * C + F * C),
                       "wg": 2 * (C * C + C * F), "valu": 12 * C},
        "edge_mlp_bwd": {"fwd": 2 * H * F, "grad": 2 * H * F + 2 * (F * H) * (B - 1) / B,
                         "wg": 2 * (F * H + H * F), "valu": 8 * H},
    }


EDGE_KERNELS = ["edge_mlp_fwd", "source_fwd", "target_fwd", "target_bwd", "source_bwd",
                "edge_mlp_bwd"]


def kernel_flops_per_edge(F, B):
    return {k: sum(v.values()) for k, v in kernel_flops_split(F, B).items()}


# how each edge path computes each class of flops (include/pfsgnn.h,
# pfsgnn_mfma_core.h FwdLayer / GradLayer / WgImg): ("f32", 1) exact fp32
# (MFMA or VALU, 157.3 TF/s), ("bf16", k) k bf16 MFMA products per product
# (bf16x3 = 3, bf16x6 = 6, single bf16 = 1; 2.5 PF/s dense)
PATH_ARITH = {
    "mfma":   {"fwd": ("f32", 1), "grad": ("bf16", 3), "wg": ("bf16", 3)},
    "mfma32": {"fwd": ("f32", 1), "grad": ("f32", 1), "wg": ("f32", 1)},
    "valu":   {"fwd": ("f32", 1), "grad": ("f32", 1), "wg": ("f32", 1)},
    "bf16y":  {"fwd": ("f32", 1), "grad": ("f32", 1), "wg": ("f32", 1)},
    "bf16m":  {"fwd": ("bf16", 1), "grad": ("bf16", 1), "wg": ("bf16", 3)},
    "bf16":   {"fwd": ("bf16", 1), "grad": ("bf16", 1), "wg": ("bf16", 3)},
    "bf16x6": {"fwd": ("bf16", 6), "grad": ("bf16", 3), "wg": ("bf16", 3)},
    "bf16x3": {"fwd": ("bf16", 3), "grad": ("bf16", 3), "wg": ("bf16", 3)},
}


def compute_floor_s(kernel, F, B, path, E):
    """The matrix/vector floor of one launch over E edges: fp32 flops at the
    fp32 peak plus bf16 MFMA products at the dense bf16 peak (MI355X_MICROARCH.md)
    -> (seconds, {f32 flops, bf16 product-flops})."""
    ar = PATH_ARITH[path]
    f32 = bf = 0.0
    for cls, fl in kernel_flops_split(F, B)[kernel].items():
        kind, k = ar.get(cls, ("f32", 1))
        if kind == "f32":
            f32 += fl * E
        else:
            bf += k * fl * E
    return f32 / (F32_MFMA_PEAK_TFS * 1e12) + bf / (BF16_MFMA_PEAK_TFS * 1e12), \
        {"f32_flops": int(f32), "bf16_product_flops": int(bf)}


def kernel_roofline(kernel, F, B, path, E, bytes_per_launch, seconds):
    """Both roofs of one launch and the binding one (the larger floor)."""
    t_mm, fl = compute_floor_s(kernel, F, B, path, E)
    t_hbm = bytes_per_launch / (HBM_PEAK_GBS * 1e9)
    hbm = {"achieved": round(bytes_per_launch / seconds / 1e9, 1), "peak": HBM_PEAK_GBS,
           "unit": "GB/s", "frac": round(t_hbm / seconds, 4), "floor_us": round(t_hbm * 1e6, 1)}
    # the compute roof in fp32-equivalent TFLOP/s: bf16 products weighted by
    # the fp32 / bf16 peak ratio, so that achieved / peak = floor / duration
    eq = fl["f32_flops"] + fl["bf16_product_flops"] * F32_MFMA_PEAK_TFS / BF16_MFMA_PEAK_TFS
    mm = {"achieved": round(eq / seconds / 1e12, 2), "peak": F32_MFMA_PEAK_TFS,
          "unit": "TFLOP/s (fp32-equivalent)", "frac": round(t_mm / seconds, 4),
          "floor_us": round(t_mm * 1e6, 1), **fl}
    bound = "hbm" if t_hbm >= t_mm else "mfma"
    return bound, hbm, mm


def pmc_traffic(kernel, E, F):
    """HBM bytes per launch of `kernel` from the latest committed PMC pass
    (profiles/<round>_traffic.json, made by tools/prof_pmc.sh +
    tools/pmc_traffic.py: separate FETCH_SIZE / WRITE_SIZE passes, FETCH
    calibrated on k_edge_bn_sums), or None.  rocprofv3 cannot run inside the
    process it profiles, so bench.py reads the pass rather than measuring it."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_traffic.json")), reverse=True):
        try:
            d = json.load(open(path))
        except (OSError, ValueError):
            continue
        from pfsgnn import native
        pre = "k_" if native.get_edge_path() == "valu" else "km_"
        key = f"{pre}{kernel}<{F}>"
        # (passes without an edge_path field were taken on the mfma path)
        if (d.get("E") == E and d.get("F") == F and key in d.get("kernels", {})
                and d.get("edge_path", "mfma") == native.get_edge_path()):
            return d["kernels"][key]["traffic_bytes"], os.path.basename(path)
    return None


def cpu_share():
    """CPUs this process may actually run on: os.cpu_count() capped by the
    affinity mask and by a cgroup-v2 CPU quota (a container's share of a large
    host).  Threads beyond the share oversubscribe it and slow torch's CPU
    kernels down by orders of magnitude."""
    host = os.cpu_count() or 1
    n = host
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return host, n


def cpu_baseline(blocks, seconds):
    """The CPU oracle (oracle/, torch on the host cores) timed on a bounded sample
    of the same workload: ONE 2394x128 graph, full training step incl. Adam."""
    from harness import make_problem
    from noise_ref import uniform_numpy
    from oracle.ref_train import loss_function as oracle_loss
    # train.py:15-19 sets torch's threads to os.cpu_count(); on a container
    # share of a large host that count is the host's, so the threads are capped
    # at the CPUs this process may use (both numbers are reported)
    host, threads = cpu_share()
    torch.set_num_threads(threads)
    print(f"[bench] cpu baseline: {threads} threads (os.cpu_count() = {host})",
          file=sys.stderr, flush=True)
    model, graph = make_problem(1, NF, NC, B=blocks, seed=0, dtype=torch.float32)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=5e-4)
    uni = torch.as_tensor(uniform_numpy(1, NF * NC))
    steps, t0 = 0, time.perf_counter()
    while True:
        opt.zero_grad()
        out = model(graph)
        loss, _ = oracle_loss(model, out.x_e, graph.x_t, 1, NF, NC, pclass=0.1, pfiber=0.1,
                              sharpness=10.0, uniform=uni)
        loss.backward()
        opt.step()
        steps += 1
        el = time.perf_counter() - t0
        print(f"[bench] cpu baseline step {steps}: {el:.1f}s", file=sys.stderr, flush=True)
        if el >= seconds or steps >= 50:
            break
    return {"value": steps * NF * NC / el, "unit": "edges/s", "cores": threads, "kind": "port",
            "host_cpus": host,
            "sample": f"{steps} training step(s) of one {NF}x{NC} graph, {blocks} blocks, "
                      f"oracle/ (torch CPU fp32, {threads} threads: os.cpu_count() = {host} as "
                      f"train.py:15-19 sets, capped at this process's CPU share), {el:.1f}s"}


def main():
    global NF, NC
    args = parse()
    NF, NC = args.fibers, args.classes
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # rehearsal knobs for the multi-rank path on a one-GPU box (tests only):
    # every rank on cuda:0 and the gloo backend instead of RCCL
    if os.environ.get("PFSGNN_BENCH_SAME_DEVICE") == "1":
        local = 0
        # ranks sharing one GPU cannot promise a co-resident grid to the fused
        # class-side launches (device-wide barrier): use their unfused form
        for knob in ("PFSGNN_FUSED_TAIL", "PFSGNN_CLASS_TAIL", "PFSGNN_CLASS_BWD"):
            os.environ.setdefault(knob, "0")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    # the data-parallel code path (collectives in the step): N > 1, or forced at
    # N = 1 (PFSGNN_DIST_FORCE=1 under torchrun --nproc-per-node 1) to rehearse
    # the RCCL capture on one GPU
    dist_path = world > 1 or os.environ.get("PFSGNN_DIST_FORCE") == "1"
    if dist_path:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("PFSGNN_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    import pfsgnn
    from pfsgnn import config, native
    from pfsgnn.train import loss_function
    from pfsgnn.distributed import allreduce_gradients, broadcast_parameters, sync_buffers
    config.device = device

    G, B = args.graphs, args.blocks
    native.set_edge_path(args.edge_path)
    torch.manual_seed(0)
    gnn = pfsgnn.GNN(B=B, Fdim=FDIM, T=NC, F_s=1, F_t=2).to(device)
    gnn.train()
    broadcast_parameters(gnn)
    use_graph = not args.no_graph
    opt = pfsgnn.FusedAdam(gnn.parameters(), lr=config.lr, capturable=use_graph)
    data, class_info = make_batch(G, rank, device)
    E = G * NF * NC
    # softfloor's noise seed lives on the device and advances every step, so a
    # replayed graph draws fresh noise each step (train.py:22 draws per call)
    seed_t = torch.full((), 1000 * rank, dtype=torch.int64, device=device)

    def fwd_bwd():
        seed_t.add_(1)
        gnn.zero_grad()
        out = gnn(data)
        loss, _ = loss_function(out, class_info, pclass=0.1, pfiber=0.1, sharpness=10.0,
                                seed=seed_t)
        loss.backward()
        return loss

    def step():
        sync_buffers(gnn)          # DDP broadcast_buffers, before the forward (no-op at N=1)
        loss = fwd_bwd()
        allreduce_gradients(gnn)
        opt.step()
        return loss

    for i in range(args.warmup):
        step()
    torch.cuda.synchronize()
    graph = None
    if use_graph:
        # one training step captured as a HIP graph: forward, train.py loss,
        # backward (+ Adam when there is no collective) replayed by the GPU
        # command processor with no per-kernel host launch
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # N > 1: the whole step -- buffer broadcast, forward, loss, backward,
        # the gradient all-reduce and Adam -- is ONE captured graph, as at N = 1
        # (RCCL collectives capture into HIP graphs); if the capture fails the
        # tail (broadcast, all-reduce, Adam) runs eagerly around the replay
        # (PFSGNN_BENCH_EAGER_TAIL=1 forces that form)
        tail_in_graph = not dist_path or (os.environ.get("PFSGNN_BENCH_EAGER_TAIL") != "1" and
                                          dist.get_backend() == "nccl")
        graph = torch.cuda.CUDAGraph()
        if tail_in_graph:
            try:
                with torch.cuda.graph(graph):
                    sync_buffers(gnn)
                    static_loss = fwd_bwd()
                    allreduce_gradients(gnn)
                    opt.step()
            except Exception as exc:  # noqa: BLE001
                if not dist_path:
                    raise
                print(f"[bench] capturing the collectives failed ({exc!r}): eager tail",
                      file=sys.stderr, flush=True)
                tail_in_graph = False
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
        if not tail_in_graph:
            with torch.cuda.graph(graph):
                static_loss = fwd_bwd()
        torch.cuda.synchronize()

        def step():  # noqa: F811
            if not tail_in_graph:
                sync_buffers(gnn)
            graph.replay()
            if not tail_in_graph:
                allreduce_gradients(gnn)
                opt.step()
            return static_loss

        step()
    torch.cuda.synchronize()
    if dist_path:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    if dist_path:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if rank == 0:
        print(f"[bench] {args.steps} timed steps: {elapsed:.2f}s", file=sys.stderr, flush=True)
    if dist_path:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # (PFSGNN_BENCH_ANY_LOSS=1: timing studies of ablation builds, tools/variants.sh)
    assert torch.isfinite(loss).item() or os.environ.get("PFSGNN_BENCH_ANY_LOSS") == "1", \
        "non-finite loss"
    # no device-wide barrier of the fused class-side launches timed out
    sync_faults = native.sync_faults()
    assert sync_faults == 0, f"{sync_faults} device-wide barrier time-outs"
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, gnn)

    def report(roofline=None, cpu=None, tail=None, consistency=None, alt=None):
        """Rank 0 prints the JSON line; the process group is torn down."""
        if rank == 0:
            value = world * E * args.steps / elapsed
            if NC == 16 and G * world == 2048:
                bcfg = (f"BASELINE configs[3]: 2048 synthetic {NF}x{NC} graphs sharded over "
                        f"{world} GPU(s), {G} per GPU, RCCL gradient all-reduce")
            elif NC == 16 and G == 256 and world == 1:
                bcfg = f"BASELINE configs[2]: 256 synthetic {NF}x{NC} graphs on one GPU"
            elif (NF, NC, B) == (2394, 128, 8):
                bcfg = ("BASELINE metric / configs[4] shape (2394x128, 8 message-passing rounds)" +
                        (f", weak-scaled over {world} GPUs (configs[3]'s data-parallel sharding)"
                         if world > 1 else ""))
            else:
                bcfg = None
            metric = "training-step edges/sec on 2394\u00d7128 bipartite batches; % HBM roofline"
            if (NF, NC) != (2394, 128):
                metric = (f"training-step edges/sec on {NF}\u00d7{NC} bipartite batches; "
                          f"% HBM roofline")
            line = {
                "metric": metric,
                "value": value, "unit": "edges/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": DTYPE[args.edge_path],
                "data": "synthetic",
                "precision": PRECISION[args.edge_path],
                "meets_fp32_tolerance": MEETS_FP32_TOL[args.edge_path],
                "config": {"workload": f"{G} complete bipartite {NF}x{NC} graphs per GPU, {B} "
                                       f"message-passing blocks, Fdim {FDIM}; full training step "
                                       f"(GNN fwd + train.py loss + bwd + Adam)",
                           "fibers": NF, "classes": NC, "graphs_per_gpu": G,
                           "global_graphs": G * world, "blocks": B, "fdim": FDIM,
                           "edges_per_gpu_step": E, "parallelism": f"dp{world}",
                           "baseline_config": bcfg},
                "full": args.full,
                "roofline": roofline,
                "cpu_baseline": cpu,
            }
            line["sync_faults"] = sync_faults
            if consistency is not None:
                line["rank_consistency"] = consistency
            if tail is not None:
                line["eager_tail"] = tail
            if alt:
                line["alt_paths"] = alt
            print(json.dumps(line), flush=True)
        if dist_path:
            dist.destroy_process_group()

    # a plain run ends here: everything below measures or checks something
    # other than the headline figure, in runs of its own
    if not args.full:
        report()
        return

    # ---- N > 1: the tail of a step -- the buffer broadcast before the
    # forward, the gradient all-reduce and Adam after the backward -- each run
    # eagerly and timed alone (synchronised) over a few extra steps
    tail = None
    if dist_path and use_graph:
        t_sync, t_red, t_adam = [], [], []
        for i in range(min(args.steps, 10)):
            torch.cuda.synchronize()
            ta = time.perf_counter()
            sync_buffers(gnn)
            torch.cuda.synchronize()
            tb = time.perf_counter()
            graph.replay()
            torch.cuda.synchronize()
            tc = time.perf_counter()
            allreduce_gradients(gnn)
            torch.cuda.synchronize()
            td = time.perf_counter()
            opt.step()
            torch.cuda.synchronize()
            te = time.perf_counter()
            t_sync.append(tb - ta)
            t_red.append(td - tc)
            t_adam.append(te - td)
        med = lambda v: sorted(v)[len(v) // 2] * 1e3  # noqa: E731
        tail = {"sync_buffers_ms": round(med(t_sync), 4), "allreduce_ms": round(med(t_red), 4),
                "adam_ms": round(med(t_adam), 4), "in_graph": tail_in_graph,
                "note": "per step, each part run eagerly and synchronised alone (median of %d "
                        "steps after the timed region); in the timed steps they are %s" %
                        (len(t_sync), "part of the one captured step graph" if tail_in_graph
                         else "launched eagerly around the graph replay")}
        t = torch.tensor([tail["sync_buffers_ms"], tail["allreduce_ms"], tail["adam_ms"]],
                         device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        tail.update(sync_buffers_ms=round(float(t[0]), 4), allreduce_ms=round(float(t[1]), 4),
                    adam_ms=round(float(t[2]), 4), over_ranks="max")
    consistency = None
    if dist_path:
        # every rank must end the K steps with bitwise the same parameters
        # (one all-reduce, the same Adam) and, after the buffer broadcast that
        # opens the next step, the same BatchNorm buffers
        sync_buffers(gnn)
        flat = gnn.flat_parameters()[0]
        bufs = torch.cat([b.detach().double().reshape(-1) for b in gnn.buffers()])
        consistency = {}
        for name, t in (("parameters", flat.double()), ("buffers", bufs)):
            hi, lo = t.clone(), t.clone()
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            consistency[name + "_bitwise_equal"] = bool(torch.equal(hi, lo))
        assert all(consistency.values()), consistency

    # ---- each edge kernel's duration INSIDE the replayed step: the step
    # captured once more with that kernel launched twice back to back
    # (pfsgnn_timing_repeat; the kernel only overwrites its outputs), the two
    # graphs replayed alternately, timed with HIP events on the launch stream;
    # (repeat - plain) / launches per step = the kernel's in-situ time
    in_graph = {}
    if use_graph and native.get_edge_path() != "valu":
        def replay_ms(gx, reps):
            t_a, t_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t_a.record()
            for _ in range(reps):
                gx.replay()
            t_b.record()
            t_b.synchronize()
            return t_a.elapsed_time(t_b) / reps

        reps = max(5, min(args.steps, 30))
        for kname in EDGE_KERNELS:
            native.timing_repeat(kname, 1)
            try:
                g_rep = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_rep):
                    if tail_in_graph:
                        sync_buffers(gnn)
                    fwd_bwd()
                    if tail_in_graph:
                        allreduce_gradients(gnn)
                        opt.step()
            finally:
                native.timing_repeat(kname, 0)
            torch.cuda.synchronize()
            base, rep = [], []
            g_rep.replay()
            for _ in range(3):
                base.append(replay_ms(graph, reps))
                rep.append(replay_ms(g_rep, reps))
            base.sort()
            rep.sort()
            in_graph[kname] = {"plain_ms_per_step": round(base[1], 4),
                               "repeat_ms_per_step": round(rep[1], 4),
                               "extra_ms_per_step": round(rep[1] - base[1], 4)}
            del g_rep
        torch.cuda.synchronize()
        in_graph_method = ("marginal time of one extra back-to-back launch per call in the "
                           "replayed step (median of 3 alternating rounds of %d replays, HIP "
                           "events on the launch stream)" % reps)

    # ---- the same step on the other edge paths (BASELINE configs[4]: the split-
    # bf16 contractions, each flagged meets_fp32_tolerance or not; the exact-fp32
    # one), each captured and replayed like
    # the headline path, N=1 only; the parameters keep training (synthetic data)
    alt = {}
    if world == 1 and use_graph and args.alt_paths:
        for pth in [p for p in args.alt_paths.split(",") if p and p != args.edge_path]:
            native.set_edge_path(pth)
            for i in range(2):
                fwd_bwd()
                opt.step()
            torch.cuda.synchronize()
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                fwd_bwd()
                opt.step()
            g2.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                g2.replay()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            alt[pth] = {"value": E * args.steps / el, "ms_per_step": el / args.steps * 1e3,
                        "precision": PRECISION[pth], "meets_fp32_tolerance": MEETS_FP32_TOL[pth]}
            del g2
        native.set_edge_path(args.edge_path)

    # ---- per-kernel device times: HIP events around each main kernel, on its
    # launch stream, over a few eager steps of the same workload right after
    # the timed region (a replayed graph has no per-kernel host hook).  Each
    # timed kernel is preceded by a short spin kernel (pfsgnn_timing_enable(2))
    # so that the start event is reached only once the kernel is enqueued: the
    # interval is the kernel alone, not the host's launch latency of an eager
    # step (rocprofv3's kernel trace of the graph replays agrees).
    prof_steps = min(args.steps, 5)
    native.timing_enable("spin")
    native.timing_reset()
    for i in range(prof_steps):
        loss_p = fwd_bwd()
        allreduce_gradients(gnn)
        opt.step()
    torch.cuda.synchronize()
    native.timing_enable(False)

    # ---- per-kernel times (HIP events on the launch stream) and rooflines:
    # each edge kernel against both roofs -- algorithmic HBM bytes at 8 TB/s,
    # and its flops by the arithmetic the edge path runs them in (fp32 at the
    # fp32 peak, bf16 MFMA products at the bf16 peak); the binding roof is
    # the one with the larger floor
    per_edge = kernel_bytes_per_edge(FDIM)
    kt = {}
    for k in native.KERNELS:
        ms, n = native.timing_query(k)
        if n:
            kt[k] = (ms, n)
    path = native.get_edge_path()
    kernels = {}
    for k in EDGE_KERNELS:
        if k not in kt:
            continue
        ms, n = kt[k]
        launches = n / prof_steps
        bpl = per_edge[k] * E
        if k == "edge_mlp_bwd":      # block 0 writes no input gradient
            bpl = (per_edge[k] * (B - 1) + 3 * 4 * FDIM) * E / B
        eager_s = ms / n / 1e3
        ig = in_graph.get(k)
        sec = ig["extra_ms_per_step"] / launches / 1e3 if ig and ig["extra_ms_per_step"] > 0 \
            else eager_s
        bound, hbm, mm = kernel_roofline(k, FDIM, B, path, E, bpl, sec)
        kernels[k] = {"bound": bound, "frac": (hbm if bound == "hbm" else mm)["frac"],
                      "avg_launch_us": round(sec * 1e6, 1),
                      "timing": "in_graph" if sec != eager_s else "eager",
                      "eager_avg_launch_us": round(eager_s * 1e6, 1),
                      "launches_per_step": launches, "bytes_per_launch": int(bpl),
                      "hbm": hbm, "mfma": mm}
    dom = max(kernels, key=lambda k: kernels[k]["avg_launch_us"] * kernels[k]["launches_per_step"])
    kd = kernels[dom]
    top = kd["hbm"] if kd["bound"] == "hbm" else kd["mfma"]
    tr = pmc_traffic(dom, E, FDIM)
    roofline = {"bound": kd["bound"], "kernel": dom,
                "achieved": top["achieved"], "peak": top["peak"], "unit": top["unit"],
                "frac": top["frac"],
                "traffic": None if tr is None else int(tr[0]),
                "traffic_source": None if tr is None else f"profiles/{tr[1]} (PMC bytes per launch)",
                "hbm": kd["hbm"], "mfma": kd["mfma"],
                "avg_launch_us": kd["avg_launch_us"], "launches": kd["launches_per_step"],
                "eager_avg_launch_us": kd["eager_avg_launch_us"],
                "bytes_per_launch": kd["bytes_per_launch"],
                "edge_kernels": {k: {kk: v[kk] for kk in ("bound", "frac", "avg_launch_us", "timing")}
                                 | {"hbm_frac": v["hbm"]["frac"], "mfma_frac": v["mfma"]["frac"]}
                                 for k, v in kernels.items()},
                "pricing": "algorithmic bytes / 8 TB/s vs fp32 flops / 157.3 TF/s + bf16 MFMA "
                           "products / 2.5 PF/s (the edge path's arithmetic per flop class: "
                           f"{PATH_ARITH.get(path)}); the binding roof has the larger floor",
                "kernel_ms_per_step": {k: round(v[0] / prof_steps, 3) for k, v in kt.items()},
                "timing": (f"avg_launch_us: {in_graph_method}; " if in_graph else "") +
                          f"kernel_ms_per_step and eager_avg_launch_us: HIP events around each "
                          f"launch behind a lead-in spin kernel, {prof_steps} eager steps after "
                          f"the timed region (eager launches run ~5% slower than replayed ones)"}
    if in_graph:
        roofline["in_graph"] = in_graph

    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(B, args.cpu_seconds)
    report(roofline, cpu, tail, consistency, alt)


if __name__ == "__main__":
    main()
