"""The cases and the reference of tests/test_gpu_sliced_ops.py, checked on the
CPU: every adversarial graph of tests/sliced_ops_case.py reaches the layout
branch it was built for (judged on the torch restatement of the sliced layout,
test_gpu_sparse.sliced_plan_ref), and the reference those GPU tests use --
pfsgnn.sparse.SparseEdgeOps on the float64 emulation -- equals the
complete-graph emulation that test_gpu_ops.test_edge_ops uses, on a complete
graph, on every output of the six edge ops."""
import pytest
import torch

from sliced_ops_case import (CASES, case_edges, emu_complete_run, emu_sparse_run, make_inputs,
                             plan_of, run_ops, step_classes)


def ks_of(G, NF, maxdeg):
    """pfm::sl_geo's step splits: min(ceil(1024 / groups), 8, max(1, maxdeg / 8)),
    groups = G * ceil(NF / 64) blocks of 64 fibers."""
    groups = G * ((NF + 63) // 64)
    return max(1, min(-(-1024 // groups), 8, max(1, maxdeg // 8)))


@pytest.mark.parametrize("ncmax", [128, 124, 96])
def test_hub_case_preconditions(ncmax):
    G, NF, NC, ei = case_edges("hub", ncmax)
    sp, plan = plan_of(ei, G, NF, NC)
    E = ei.shape[1]
    assert (G, NF, NC) == (2, 70, ncmax) and E < 16000
    assert plan["maxdeg"] >= 64 and ks_of(G, NF, plan["maxdeg"]) == 8
    ln = plan["len"].tolist()
    assert ln == [NC, 1, 1, 1, 1, 0, 0, 0, 22, 2, 2, 2, 2, 0, 0, 0]
    assert 0 in ln and 1 in ln
    lanes = plan["fib"].view(-1, 16)
    assert bool(((lanes < 0).any(1) & (lanes >= 0).any(1)).any())     # a slice with an absent fiber
    assert bool((lanes < 0).all(1).any())                             # a slice of absent fibers only
    assert plan["EP"] / E > 3
    deg = sp.fib_ptr[1:] - sp.fib_ptr[:-1]
    assert bool((deg[64:69] == 0).all()) and int(deg[3]) == NC        # edgeless fibers, the hub
    # a block of 64 fibers splits each slice's steps 8 ways ([L ks / 8, L (ks + 1) / 8)):
    # with len 0, 1 or 2 at least six of the eight splits are empty
    for L in (0, 1, 2):
        assert sum(1 for ks in range(8) if (L * ks) // 8 == (L * (ks + 1)) // 8) >= 6
    steps = step_classes(plan)
    # acc_add's row-sum form with a single valid lane (the hub's own steps) ...
    assert any(s == 0 and c.numel() == 1 for s, k, c in steps)
    # ... and the owner rounds at their longest: a tile of graph 1 with 8 lanes on
    # each of two classes
    worst = [c for s, k, c in steps if s >= 8 and c.numel() == 16 and
             sorted(torch.bincount(c).tolist())[-2:] == [8, 8]]
    assert worst and all(set(c.tolist()) == {5, 9} for c in worst)
    # repeated pairs: fiber 0 of graph 1 holds class 5 21 times
    assert int(((ei[0] == NF) & (ei[1] == NC + 5)).sum()) == 21


def test_complete_case_preconditions():
    G, NF, NC, ei = case_edges("complete")
    sp, plan = plan_of(ei, G, NF, NC)
    assert (G, NF, NC) == (2, 40, 12) and ei.shape[1] == G * NF * NC
    assert plan["len"].tolist() == [12, 12, 12, 0] * 2 and plan["EP"] == 2 * 3 * 16 * 12
    valid = [(plan["fib"].view(-1, 16)[s] >= 0).sum().item() for s in range(8)]
    assert valid == [16, 16, 8, 0] * 2
    for s, k, c in step_classes(plan):
        assert c.numel() == valid[s] and bool((c == k).all())       # one class per tile
    assert ks_of(G, NF, plan["maxdeg"]) == 1


def test_other_case_preconditions():
    G, NF, NC, ei = case_edges("one_class")
    sp, plan = plan_of(ei, G, NF, NC)
    assert (G, NF, NC) == (1, 33, 1) and bool((ei[1] == 0).all())
    deg = sp.fib_ptr[1:] - sp.fib_ptr[:-1]
    assert int(deg.min()) == 0 and int(deg.max()) >= 2               # an edgeless fiber, repeated pairs
    G, NF, NC, ei = case_edges("one_fiber_block")
    sp, plan = plan_of(ei, G, NF, NC)
    assert (G, NF, NC) == (3, 65, 7)
    lanes = plan["fib"].view(G, 8, 16)
    deg = sp.fib_ptr[1:] - sp.fib_ptr[:-1]
    for g in range(G):
        blk = lanes[g, 4:].flatten()
        assert int((blk >= 0).sum()) == 1                             # the second block: one fiber
        assert (int(deg[blk[blk >= 0]]) == 0) == (g == 0)             # edgeless in graph 0
    G, NF, NC, ei = case_edges("ragged")
    sp, plan = plan_of(ei, G, NF, NC)
    assert (G, NF, NC) == (3, 130, 40) and ei.shape[1] < 16000
    deg = sp.fib_ptr[1:] - sp.fib_ptr[:-1]
    cdeg = sp.cls_ptr[1:] - sp.cls_ptr[:-1]
    assert int(deg.min()) == 0 and int(cdeg.min()) == 0 and plan["EP"] > ei.shape[1]
    assert ei.shape[1] > torch.unique(ei, dim=1).shape[1]             # repeated pairs


@pytest.mark.parametrize("case", CASES)
def test_case_builders_are_deterministic(case):
    a, b = case_edges(case), case_edges(case)
    assert a[:3] == b[:3] and torch.equal(a[3], b[3])


@pytest.mark.parametrize("F", [8, 10, 16])
def test_sparse_reference_equals_complete_emulation(F):
    """SparseEdgeOps(EmuBackend()) on the complete graph == the complete-graph
    emulation, float64, 1e-12, every output of the six ops after the edge-order
    map: the reference of the sliced op tests is pinned to test_edge_ops's."""
    G, NF, NC, ei = case_edges("complete")
    inp = make_inputs(G, NF, NC, F, ei.shape[1], 77 + F)
    a = run_ops(emu_sparse_run(ei, G, NF, NC, F), inp)
    b = run_ops(emu_complete_run(G, NF, NC, F), inp)
    assert set(a) == set(b) and len(a) >= 30
    for k in a:
        assert a[k].shape == b[k].shape, k
        err = (a[k] - b[k]).abs().max().item()
        assert err <= 1e-12 * max(b[k].abs().max().item(), 1.0), (k, err)
