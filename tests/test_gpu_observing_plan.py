"""The observing plan on the HIP library: pfsgnn_schedule_plan
(csrc/pfsgnn_schedule.hip) at op level and through ``pfsgnn.train.
observing_plan`` / ``TrainLoop.plan``.

Every output must equal tests/observing_plan_ref.py bit for bit: all T here are
integers (or the golden graph's on a 1/4 grid), so every double sum is exact and
the plan is a pure function of (visits, edge_index, ci, total_time, nfields) --
caller orders and the two batch forms compare bitwise.  One case puts T off the
grid (T + 0.3): there the integer outputs must still be exact and the fp32 times
within one fp32 ulp of the reference's sequential sum.

Visits come from two sources: seeded random integers against a class_info
crafted for the case (tests/observing_plan_case.py, which also says which class
was built for which branch; the branch is then asserted on the reference), and
``hard_schedule(..., "budget")`` on the harness model with ``decoder_e.2.bias``
shifted as tests/test_gpu_budget_round.py does.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from harness import canonical_edges, make_problem  # noqa: E402
from observing_plan_case import (BRANCHES, NFIELDS, TOTAL_TIME, assert_branches,  # noqa: E402
                                 craft)
from observing_plan_ref import observing_plan_ref  # noqa: E402
import sliced_ops_case as soc  # noqa: E402
from test_gpu_hard_schedule import _data, _gnn, sliced_layouts  # noqa: E402,F401
from test_sparse_emu import sparse_edges  # noqa: E402

OUT = ("visits", "start", "used", "idle", "n", "completeness", "utility", "over", "worst", "cut",
       "seg_ptr", "seg_edge", "seg_start")
INTS = ("visits", "n", "over", "cut", "seg_ptr", "seg_edge")
ALL = tuple(b for b in BRANCHES if b != "plain")


@pytest.fixture(scope="module")
def hb():
    from pfsgnn.native import HipBackend
    return HipBackend()


def _ref(vis, ei, ci, G, NF, cap=True):
    return observing_plan_ref(np.asarray(vis), np.asarray(ei), np.asarray(ci), TOTAL_TIME, NFIELDS,
                              G * NF, cap=cap, G=G)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(name, plan, r, fields=OUT):
    """Bit for bit (a NaN -- the completeness of a class with N = 0 or NaN --
    must be a NaN in the same place; its payload is not compared)."""
    for k, t in zip(OUT, plan):
        if k not in fields:
            continue
        got, want = t.cpu().numpy(), r[k]
        assert got.dtype == want.dtype and got.shape == want.shape, (name, k, got.dtype, got.shape)
        if got.dtype == np.float32:
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (name, k)
            got, want = np.where(nan, 0, got).astype(np.float32), np.where(nan, 0, want).astype(
                np.float32)
        bad = bits(got) != bits(want)
        assert not bad.any(), (name, k, int(bad.sum()), np.nonzero(bad)[0][:5])


def equal_plans(a, b, name=""):
    for k, x, y in zip(OUT, a, b):
        if x is None or y is None:
            assert x is None and y is None, (name, k)
            continue
        assert x.dtype == y.dtype and torch.equal(bits_t(x), bits_t(y)), (name, k)


def bits_t(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def batch(ei, G, NF, NC):
    import pfsgnn
    return pfsgnn.BipartiteData(torch.as_tensor(ei).cuda(), torch.zeros(G * NF, 1),
                                torch.zeros(G * NC, 2), torch.zeros(ei.shape[1], 10),
                                torch.zeros(G, 10))


def plan_of(ei, G, NF, NC, vis, ci, **kw):
    from pfsgnn.train import observing_plan
    return observing_plan(batch(ei, G, NF, NC), torch.as_tensor(ci), torch.as_tensor(vis), **kw)


def op_plan(hb, d, ci, vis, cap=True, segments=True, out=None, **form):
    """The op itself with its batch form given (``mode`` / ``perm``, or ``sp``)."""
    cid = ci if isinstance(ci, torch.Tensor) else torch.as_tensor(ci).t().contiguous().cuda()
    v = vis if isinstance(vis, torch.Tensor) else torch.as_tensor(vis, dtype=torch.int32).cuda()
    out = hb.schedule_plan(d, cid, v, TOTAL_TIME, NFIELDS, cap=cap, out=out, **form)
    if not segments:
        return tuple(out) + (None, None)
    count = int(out[-1][-1])
    se = torch.full((count,), -7, dtype=torch.int32, device="cuda")
    ss = torch.full((count,), float("nan"), device="cuda")
    hb.schedule_plan(d, cid, v, TOTAL_TIME, NFIELDS, cap=cap, seg_edge=se, seg_start=ss, out=out,
                     **form)
    return tuple(out) + (se, ss)


# ================================================================ complete batches
# (G, NF, NC, the first branch of the crafted class_info): NF = 70 a partial
# 64-fiber group, NF = 33 / 65 a partial block of the fiber pass; NC = 1; NC =
# 192 the budget op's class limit.  2 x 9 and 192 classes hold every branch
DENSE = [(2, 70, 9, 0), (1, 33, 5, 4), (2, 70, 1, 9), (1, 65, 192, 3)]


@pytest.fixture(scope="module")
def dense_cases():
    out = {}
    for case in DENSE:
        G, NF, NC, first = case
        ei = canonical_edges(G, NF, NC).numpy()
        vis, ci, branch, f0 = craft(ei, G * NF, G * NC, 100 + NF + NC, first=first)
        out[case] = (ei, vis, ci, branch, f0, _ref(vis, ei, ci, G, NF))
    return out


@pytest.mark.parametrize("case", DENSE)
def test_dense(dense_cases, case):
    from pfsgnn.gnn import Layout
    G, NF, NC, first = case
    ei, vis, ci, branch, f0, r = dense_cases[case]
    assert_branches(r, ei, vis, branch, f0, need=ALL if G * NC >= 12 else ())
    if NC > 1:
        # a fiber that is over: negative idle, counted in over
        assert (r["total"] > TOTAL_TIME).any() and r["over"].sum() > 0
        assert (r["idle"][r["total"] > TOTAL_TIME] < 0).all()
    data = batch(ei, G, NF, NC)
    from pfsgnn.train import _plan_geometry, observing_plan
    # (with one class per graph the fiber-major order is the canonical one)
    assert _plan_geometry(data)[1].mode == (Layout.FIBER_MAJOR if NC > 1 else Layout.CANONICAL)
    plan = observing_plan(data, torch.as_tensor(ci), torch.as_tensor(vis))
    same(str(case), plan, r)
    equal_plans(plan, observing_plan(data, torch.as_tensor(ci), torch.as_tensor(vis)), "again")
    count = observing_plan(data, torch.as_tensor(ci), torch.as_tensor(vis), segments=False)
    assert count.seg_edge is None and count.seg_start is None
    same(str(case) + " count-only", count, r, OUT[:11])


def _orders(G, NF, NC):
    E = G * NF * NC
    e = torch.arange(E)
    g, f, c = e // (NF * NC), (e // NC) % NF, e % NC
    from pfsgnn.gnn import Layout
    return {Layout.FIBER_MAJOR: e, Layout.CANONICAL: torch.argsort((g * NC + c) * NF + f),
            Layout.PERM: torch.randperm(E, generator=torch.Generator().manual_seed(11))}


def test_edge_orders(dense_cases):
    """One batch fiber-major, canonical and under a seeded permutation: each equals
    the reference of its own order, and the fiber-major plan re-indexed."""
    from pfsgnn.train import _plan_geometry, observing_plan
    case = DENSE[0]
    G, NF, NC, _ = case
    ei, vis, ci, _, _, _ = dense_cases[case]
    res = {}
    for mode, p in _orders(G, NF, NC).items():
        data = batch(ei[:, p.numpy()], G, NF, NC)
        assert _plan_geometry(data)[1].mode == mode
        res[mode] = observing_plan(data, torch.as_tensor(ci), torch.as_tensor(vis[p.numpy()]))
        same(f"order {mode}", res[mode], _ref(vis[p.numpy()], ei[:, p.numpy()], ci, G, NF))
    base = res[1]
    for mode, p in _orders(G, NF, NC).items():
        pc = p.cuda()
        assert torch.equal(res[mode].visits, base.visits[pc]), mode
        assert torch.equal(bits_t(res[mode].start), bits_t(base.start[pc])), mode
        assert torch.equal(pc[res[mode].seg_edge.long()].int(), base.seg_edge), mode
        for k in ("used", "idle", "n", "utility", "over", "worst", "cut", "seg_ptr", "seg_start"):
            assert torch.equal(bits_t(getattr(res[mode], k)), bits_t(getattr(base, k))), (mode, k)


def test_graph0_in_its_own_order():
    from pfsgnn.gnn import Layout
    from pfsgnn.train import _plan_geometry, observing_plan
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "graph0.npz"))
    ei = z["edge_index"].astype(np.int64)
    G, NF, NC = 1, 2000, 12
    vis, ci, branch, f0 = craft(ei, NF, NC, 9, first=0)
    ci[:, 0] = np.round(z["x_t"][:, 0] * 4) / 4           # the file's T on the 1/4 grid
    ci[branch_class(branch, "inert"), 0] = 0.0
    data = batch(ei, G, NF, NC)
    assert _plan_geometry(data)[1].mode == Layout.PERM
    r = _ref(vis, ei, ci, G, NF)
    assert_branches(r, ei, vis, branch, f0, need=ALL)
    same("graph0", observing_plan(data, torch.as_tensor(ci), torch.as_tensor(vis)), r)


def branch_class(branch, name):
    return [c for c, b in branch.items() if b == name]


# ================================================================ general batches
GENERAL = ["hub", "one_class", "one_fiber_block", "ragged", "wide"]


def general_edges(hb, case):
    if case == "wide":                                     # NC above pfsgnn_sliced_max_nc
        G, NF, NC = 1, 40, max(hb.sliced_max_nc(10), hb.sliced_max_nc(8), 128) + 12
        return G, NF, NC, sparse_edges(G, NF, NC, 0.3, torch.Generator().manual_seed(61), dup=6)
    return soc.case_edges(case, min(128, hb.sliced_max_nc(10)))


@pytest.mark.parametrize("case", GENERAL)
def test_general(hb, sliced_layouts, case):
    """tests/sliced_ops_case.py's graphs (the hub fiber on every class, step-less
    slices, repeated pairs, edgeless fibers and classes) and a batch with more
    classes than the sliced kernels take: the op runs on the CSR layout either way."""
    from pfsgnn.train import _plan_geometry, observing_plan
    G, NF, NC, ei = general_edges(hb, case)
    ei = ei.numpy()
    vis, ci, branch, f0 = craft(ei, G * NF, G * NC, 200 + GENERAL.index(case),
                                first=GENERAL.index(case))
    r = _ref(vis, ei, ci, G, NF)
    assert_branches(r, ei, vis, branch, f0, need=ALL if case in ("ragged", "wide") else ())
    data = batch(ei, G, NF, NC)
    lay = _plan_geometry(data)[1]
    assert lay.sp is not None and (lay.sp.sl is None) == (case == "wide")
    if case != "one_class":
        assert (np.bincount(ei[0], minlength=G * NF) == 0).any()     # an edgeless fiber
    if case in ("one_class", "ragged", "hub"):
        assert np.unique(ei[0] * (G * NC) + ei[1]).size < ei.shape[1]  # repeated pairs
    plan = observing_plan(data, torch.as_tensor(ci), torch.as_tensor(vis))
    same(case, plan, r)
    equal_plans(plan, observing_plan(data, torch.as_tensor(ci), torch.as_tensor(vis)), "again")


def test_repeated_pairs_tie_by_position(hb):
    """Fiber 0 holds class 0 four times at 3 visits each, fiber 1 once; cap 11:
    L = 2, rem = 1 -> fiber 0's lowest position keeps 3.  The fiber's plan order
    is (class, position)."""
    from pfsgnn.engine import Dims
    ei = np.array([[0, 1, 0, 0, 0, 1], [0, 0, 1, 0, 0, 1]])
    ei = np.concatenate([ei, [[0], [0]]], 1)               # positions 0, 3, 4, 6 on (0, 0)
    vis = np.array([3, 3, 1, 3, 3, 2, 3], np.int32)
    ci = np.array([[2, 11 * NFIELDS], [5, 1e6]], np.float32)
    r = _ref(vis, ei, ci, 1, 2)
    assert r["visits"].tolist() == [3, 2, 1, 2, 2, 2, 2] and r["L"][0] == 2 and r["rem"][0] == 1
    assert r["seg_edge"].tolist() == [0] * 3 + [3] * 2 + [4] * 2 + [6] * 2 + [2] + [1] * 2 + [5] * 2
    sp = hb.sparse_layout(torch.as_tensor(ei), 1, 2, 2)
    same("pairs", op_plan(hb, Dims(1, 2, 2, 10), ci, vis, sp=sp), r)


def test_both_batch_forms_on_the_complete_graph(hb, dense_cases):
    from pfsgnn.engine import Dims
    for case in (DENSE[0], DENSE[3]):
        G, NF, NC, _ = case
        ei, vis, ci, _, _, r = dense_cases[case]
        d = Dims(G, NF, NC, 10)
        a = op_plan(hb, d, ci, vis, mode=1)
        b = op_plan(hb, d, ci, vis, sp=hb.sparse_layout(torch.as_tensor(ei), G, NF, NC))
        same(f"{case} csr", b, r)
        equal_plans(a, b, str(case))


# ================================================================ budget visits
def test_budget_visits_dense_and_general(sliced_layouts):
    """The plan of ``hard_schedule(..., "budget")``: the harness model with
    decoder_e.2.bias shifted; N cut to 60 % of what the schedule asks on every
    other class, so that caps bite."""
    import test_gpu_sparse_loss as sparse_loss
    from pfsgnn.train import hard_schedule, observing_plan
    runs = []
    for G, NF, NC, F, B, seed, shift in [(2, 70, 9, 10, 2, 5, 1.5), (1, 33, 5, 16, 2, 3, 1.0)]:
        model, graph = make_problem(G, NF, NC, F=F, B=B, seed=seed)
        runs.append((G, NF, NC, F, B, shift, model, graph))
    G, NF, NC, _, B, _, _, _, F, _ = sparse_loss.CASES[1]
    model, graph, _ = sparse_loss.problem(sparse_loss.CASES[1])
    runs.append((G, NF, NC, F, B, 1.0, model, graph))
    for G, NF, NC, F, B, shift, model, graph in runs:
        with torch.no_grad():
            model.decoder_e[2].bias += shift
        out = _gnn(model, B, F)(_data(graph))
        ci = graph.x_t.float().clone()
        hs = hard_schedule(out, ci.cuda(), "budget")
        n = hs.n.cpu().float()
        ci[::2, 1] = torch.floor(0.6 * n[::2]) * NFIELDS
        plan = observing_plan(out, ci.cuda(), hs.visits)
        r = _ref(hs.visits.cpu().numpy(), graph.edge_index.numpy(), ci.numpy(), G, NF)
        assert (r["L"] >= 0).any() and (r["L"] < 0).any() and int(hs.visits.max()) >= 2
        assert r["over"].sum() == 0                        # the budget fits; the trim only removes
        same(f"budget {G}x{NF}x{NC}", plan, r)
        free = observing_plan(out, ci.cuda(), hs.visits, cap=False)
        assert torch.equal(free.visits, hs.visits) and torch.equal(free.n, hs.n)
        assert torch.equal(free.used.double(), hs.fiber_time.double())   # integer T: exact


# ================================================================ segments, cap
def test_seg_cap_prefix_and_count_only(hb, dense_cases):
    from pfsgnn.engine import Dims
    case = DENSE[0]
    G, NF, NC, _ = case
    ei, vis, ci, _, _, r = dense_cases[case]
    d = Dims(G, NF, NC, 10)
    total = int(r["seg_ptr"][-1])
    cid = torch.as_tensor(ci).t().contiguous().cuda()
    v = torch.as_tensor(vis).cuda()
    forms = [dict(mode=1), dict(sp=hb.sparse_layout(torch.as_tensor(ei), G, NF, NC))]
    for form in forms:
        for k in (1, total // 3, total - 1):
            se = torch.full((total,), -7, dtype=torch.int32, device="cuda")
            ss = torch.full((total,), -7.0, device="cuda")
            out = hb.schedule_plan(d, cid, v, TOTAL_TIME, NFIELDS, seg_edge=se[:k],
                                   seg_start=ss[:k], **form)
            same(f"prefix {k}", tuple(out), r, OUT[:11])   # seg_ptr is complete
            assert np.array_equal(se[:k].cpu().numpy(), r["seg_edge"][:k])
            assert np.array_equal(ss[:k].cpu().numpy(), r["seg_start"][:k])
            assert bool((se[k:] == -7).all()) and bool((ss[k:] == -7.0).all())
        # seg_cap = 0 with null arrays
        same("count-only", op_plan(hb, d, ci, vis, segments=False, **form), r, OUT[:11])


def test_cap_false_keeps_sanitised_visits(hb, dense_cases):
    """Visits already in 0 .. 2^24 on live classes come back bit for bit; inert
    classes, negative and huge inputs are sanitised and nothing else changes."""
    from pfsgnn.engine import Dims
    case = DENSE[0]
    G, NF, NC, _ = case
    ei, vis, ci, branch, _, _ = dense_cases[case]
    d = Dims(G, NF, NC, 10)
    clean = np.clip(vis, 0, 4)
    live = np.isfinite(ci[ei[1], 0]) & (ci[ei[1], 0] > 0)
    clean[~live] = 0
    plan = op_plan(hb, d, ci, clean, cap=False, mode=1)
    assert np.array_equal(plan[0].cpu().numpy(), clean) and not bool(plan[9].any())
    same("cap=False", plan, _ref(clean, ei, ci, G, NF, cap=False))
    raw = np.clip(vis, -9, 60)                             # (no 2^24 exposures to list)
    r = _ref(raw, ei, ci, G, NF, cap=False)
    assert (raw < 0).any() and (~live).any() and np.array_equal(r["visits"], r["w"])
    same("cap=False raw", op_plan(hb, d, ci, raw, cap=False, mode=1), r)


# ================================================================ off the grid
@pytest.mark.parametrize("form", ["complete", "general"])
def test_off_grid_T(hb, dense_cases, form):
    """T + 0.3: sums of fp32 T are no longer exact in any order.  The integer
    outputs are exact; every fp32 time is within one fp32 ulp of the reference's
    sequential double sum (reordering a double sum of < 2^24 terms moves it by
    far less than an fp32 rounding step, so at most the rounding flips); two
    runs are bitwise equal."""
    if form == "complete":
        G, NF, NC, _ = DENSE[0]
        ei, vis, ci, _, _, _ = dense_cases[DENSE[0]]
        ci = ci.copy()
    else:
        G, NF, NC, ei = soc.case_edges("hub", min(128, hb.sliced_max_nc(10)))
        ei = ei.numpy()
        vis, ci, _, _ = craft(ei, G * NF, G * NC, 77, first=1)
    ci[:, 0] += np.float32(0.3)
    r = _ref(vis, ei, ci, G, NF)
    plan = plan_of(ei, G, NF, NC, vis, ci)
    same(form, plan, r, INTS)
    assert r["seg_ptr"][-1] > 100 and (r["L"] >= 0).any()
    for k in ("start", "used", "idle", "worst", "seg_start"):
        got = getattr(plan, k).cpu().numpy().astype(np.float64)
        want = r[k].astype(np.float64)
        ulp = np.spacing(np.maximum(np.abs(r[k]), np.abs(getattr(plan, k).cpu().numpy())))
        assert (np.abs(got - want) <= ulp).all(), (form, k, np.abs(got - want).max())
    same(form, plan, r, ("completeness", "utility"))
    equal_plans(plan, plan_of(ei, G, NF, NC, vis, ci), "again")


# ================================================================ capture
def _bufs(d, E):
    i32 = dict(dtype=torch.int32, device="cuda")
    i64 = dict(dtype=torch.int64, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    nan = float("nan")
    return (torch.full((E,), -1, **i32), torch.full((E,), nan, **f32),
            torch.full((d.NS,), nan, **f32), torch.full((d.NS,), nan, **f32),
            torch.full((d.NT,), -1, **i32), torch.full((d.NT,), nan, **f32),
            torch.full((d.G,), nan, **f32), torch.full((d.G,), -1, **i32),
            torch.full((d.G,), nan, **f32), torch.full((d.NT,), -1, **i64),
            torch.full((d.NS + 1,), -1, **i64))


def _poison(bufs):
    for t in bufs:
        t.fill_(float("nan") if t.dtype == torch.float32 else -1)


@pytest.mark.parametrize("form", ["complete", "general"])
def test_capture_of_the_count_only_call(hb, dense_cases, form):
    """``segments=False`` has no host synchronisation: a torch.cuda.graph capture
    of the call replays to the eager result, bit for bit."""
    from pfsgnn.engine import Dims
    if form == "complete":
        G, NF, NC, _ = DENSE[0]
        ei, vis, ci, _, _, r = dense_cases[DENSE[0]]
        kw = dict(mode=1)
    else:
        G, NF, NC, ei = soc.case_edges("ragged")
        ei = ei.numpy()
        vis, ci, _, _ = craft(ei, G * NF, G * NC, 203, first=3)
        r = _ref(vis, ei, ci, G, NF)
        kw = dict(sp=hb.sparse_layout(torch.as_tensor(ei), G, NF, NC))
    d = Dims(G, NF, NC, 10)
    cid = torch.as_tensor(ci).t().contiguous().cuda()
    v = torch.as_tensor(vis).cuda()
    eager = [t.clone() for t in op_plan(hb, d, cid, v, segments=False, **kw)[:11]]
    bufs = _bufs(d, ei.shape[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op_plan(hb, d, cid, v, segments=False, out=bufs, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _poison(bufs)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        op_plan(hb, d, cid, v, segments=False, out=bufs, **kw)
    _poison(bufs)
    g.replay()
    torch.cuda.synchronize()
    equal_plans(eager, bufs, form)
    same(form, tuple(bufs), r, OUT[:11])


# ================================================================ TrainLoop
def test_train_loop_plans_its_best_schedule():
    """tests/test_gpu_hard_schedule.py's loop (1 x 200 x 12, B = 2, T scaled by
    1/16 -- still on the 2^-20 grid -- so that every class gets visits and some
    epoch has a positive hard utility), tracking the budgeted rounding."""
    import pfsgnn
    from pfsgnn.train import ObservingPlan, TrainLoop, observing_plan
    NF = 200
    model, graph = make_problem(1, NF, 12, B=2, seed=3)
    gnn = _gnn(model, 2, 10)
    opt = pfsgnn.FusedAdam(gnn.parameters(), lr=1e-3, capturable=True)
    ci = graph.x_t.float().clone()
    ci[:, 0] *= 0.0625
    loop = TrainLoop(gnn, opt, _data(graph), ci.cuda(), 8, [0, 20], 5.0, 0.1, 0.1, seed=77,
                     capture=True, track_hard="budget").run(7)
    best = loop.hard_best()
    assert best["epoch"] >= 0 and best["visits"].sum() > 0
    plan = loop.plan()
    assert isinstance(plan, ObservingPlan) and plan._fields == OUT
    equal_plans(plan, observing_plan(_data(graph), ci.cuda(), best["visits"]), "hard_best")
    same("loop", plan, _ref(best["visits"], graph.edge_index.numpy(), ci.numpy(), 1, NF))
    assert int(plan.over.sum()) == 0 and bool((plan.idle >= 0).all())
    assert bool((plan.used.double() <= TOTAL_TIME).all())
    assert loop.plan(segments=False).seg_edge is None
    plain = TrainLoop(gnn, opt, _data(graph), ci.cuda(), 8, [0, 20], 5.0, 0.1, 0.1, seed=77,
                      capture=False)
    with pytest.raises(ValueError, match="track_hard=True"):
        plain.plan()
