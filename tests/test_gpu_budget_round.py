"""Budgeted rounding on the HIP library: pfsgnn_schedule_budget
(csrc/pfsgnn_schedule.hip) at op level and through ``pfsgnn.train.
hard_schedule(..., "budget")`` / ``TrainLoop(track_hard="budget")``.

Quotient: ``quot`` against the float64 reference fed the device's own edge
state (tests/hard_schedule_ref.py), ``|quot - v64| <= 16 x err32`` with err32
the error of the same reference in float32.

Rounding: ``visits`` and ``phase`` must equal tests/budget_round_ref.py applied
to the device's own ``quot`` bit for bit, no edge left out; the aggregates
follow by tests/test_gpu_hard_schedule.py's consistency rules; ``over`` is 0 and
the double sum of visits x T is within total_time.  All T are integers or on a
1/4 grid, so every double sum is exact and the result is a pure function of
(quot, edge_index, ci, total_time): orders and layouts compare bitwise.
"""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from budget_round_ref import budget_round_ref, quotient  # noqa: E402
from harness import canonical_edges, make_problem  # noqa: E402
from hard_schedule_ref import hard_schedule_ref  # noqa: E402
import sliced_ops_case as soc  # noqa: E402
from test_gpu_hard_schedule import (_data, _gnn, check_consistency, class_major_edges,  # noqa: E402
                                    op_inputs, op_refs, sliced_layouts)  # noqa: F401

TOTAL_TIME, NFIELDS = 42.0, 10
FIELDS = ("visits", "n", "fiber_time", "completeness", "utility", "over", "worst", "quot", "phase")


@pytest.fixture(scope="module")
def hb():
    from pfsgnn.native import HipBackend
    return HipBackend()


def check_quot(name, quot, r64, r32):
    v64, v32 = r64["v"].double(), r32["v"].double()
    err32 = (v32 - v64).abs().max().item()
    want = v64.clamp(0.0, 2.0 ** 24)
    err = (quot.cpu().double() - want).abs().max().item()
    print(f"{name}: quot err {err:.3e}, err32 {err32:.3e}")
    assert err <= 16 * err32, (name, err, err32)


def check_rounding(name, hs, ei, ci, G, NF, NC, inert=None):
    """``ci`` [G*NC, 2] float32 on the CPU.  -> the reference's result."""
    ei_np = ei.numpy()
    r = budget_round_ref(hs.quot.cpu().numpy(), ei_np, ci.numpy(), TOTAL_TIME, G * NF, inert)
    vis = hs.visits.cpu().numpy()
    print(f"{name}: fibers {G * NF} down {int((r['phase'] & 1).astype(bool).sum())} "
          f"bumped+refused {int((r['phase'] & 6 == 6).sum())} ties {int(r['ties'].sum())} "
          f"visits {vis.min()}..{vis.max()} mismatches {int((vis != r['visits']).sum())}")
    assert vis.shape == r["visits"].shape and np.array_equal(vis, r["visits"]), name
    assert np.array_equal(hs.phase.cpu().numpy(), r["phase"]), name
    assert int(hs.over.sum()) == 0, name
    ft = np.zeros(G * NF)
    live = ~r["dead"]
    np.add.at(ft, ei_np[0][live], vis[live].astype(np.float64) * ci.numpy()[ei_np[1][live], 0])
    assert (ft <= TOTAL_TIME).all() and np.array_equal(ft, r["ft"]), name
    assert np.array_equal(hs.fiber_time.cpu().double().numpy(), ft), name   # exact sums
    if not r["dead"].any():
        check_consistency(name, hs, ei, ci, G, NF, NC)
    return r


# ================================================================ product level
# (G, NF, NC, F, B, seed, shift of decoder_e.2.bias): the harness's integer T
# unscaled.  NF = 70 a partial 64-fiber group; NC = 9 KS = 3 with an idle wave;
# NC = 5 an uneven class split; NC = 1
DENSE = [(2, 70, 9, 10, 2, 5, 1.5), (1, 33, 5, 16, 2, 3, 1.0), (2, 40, 12, 8, 2, 7, 0.0),
         (2, 70, 1, 10, 2, 9, 0.0)]


def _problem(case):
    G, NF, NC, F, B, seed, shift = case
    model, graph = make_problem(G, NF, NC, F=F, B=B, seed=seed)
    with torch.no_grad():
        model.decoder_e[2].bias += shift
    return model, graph, graph.x_t.float().clone()


def _refs(model, x_e, ei, ci, G, NF, NC):
    x = x_e.detach().cpu()
    return (hard_schedule_ref(model, x.double(), ei, ci.double(), G, NF, NC),
            hard_schedule_ref(copy.deepcopy(model).float(), x, ei, ci, G, NF, NC))


@pytest.fixture(scope="module")
def dense_products():
    from pfsgnn.train import BudgetSchedule, hard_schedule
    out = {}
    for case in DENSE:
        G, NF, NC, F, B, seed, shift = case
        model, graph, ci = _problem(case)
        o = _gnn(model, B, F)(_data(graph))
        hs = hard_schedule(o, ci.cuda(), "budget")
        assert isinstance(hs, BudgetSchedule) and o.__dict__.get("_x_e_val") is None
        again = hard_schedule(o, ci.cuda(), "budget")
        out[case] = (model, graph, ci, o, hs, again)
    return out


@pytest.mark.parametrize("case", DENSE)
def test_dense_product(dense_products, case):
    G, NF, NC, F, B, seed, shift = case
    model, graph, ci, o, hs, again = dense_products[case]
    assert not any(t.requires_grad for t in hs)
    r64, r32 = _refs(model, o.x_e, graph.edge_index, ci, G, NF, NC)
    check_quot(str(case), hs.quot, r64, r32)
    check_rounding(str(case), hs, graph.edge_index, ci, G, NF, NC)
    for a, b in zip(hs, again):                            # two runs are bitwise equal
        assert torch.equal(a, b)


def test_dense_cases_reach_every_branch(dense_products):
    """Asserted on the reference: some case has >= 10 % of its fibers in the down
    phase, some case >= 25 % that both bumped and refused, some case an
    exact-budget tie; and without a shift every fiber is up-phase."""
    down, both, ties = [], [], []
    for case, (model, graph, ci, o, hs, _) in dense_products.items():
        G, NF, NC = case[:3]
        r = budget_round_ref(hs.quot.cpu().numpy(), graph.edge_index.numpy(), ci.numpy(),
                             TOTAL_TIME, G * NF)
        down.append(float((r["phase"] & 1).astype(bool).mean()))
        both.append(float((r["phase"] & 6 == 6).mean()))
        ties.append(int(r["ties"].sum()))
        if case[6] == 0.0:
            assert down[-1] == 0.0
    print("down", down, "bumped+refused", both, "ties", ties)
    assert max(down) >= 0.10 and max(both) >= 0.25 and max(ties) >= 1


def test_edge_orders():
    """One batch fiber-major, canonical and under a seeded permutation: quot and
    visits bitwise the fiber-major result re-indexed, every aggregate bitwise equal."""
    from pfsgnn.gnn import Layout
    from pfsgnn.train import hard_schedule
    case = DENSE[0]
    G, NF, NC, F, B, seed, shift = case
    model, graph, ci = _problem(case)
    E = G * NF * NC
    e = torch.arange(E)
    g, f, c = e // (NF * NC), (e // NC) % NF, e % NC
    orders = {Layout.FIBER_MAJOR: e, Layout.CANONICAL: torch.argsort((g * NC + c) * NF + f),
              Layout.PERM: torch.randperm(E, generator=torch.Generator().manual_seed(11))}
    res = {}
    for mode, p in orders.items():
        out = _gnn(model, B, F)(_data(graph, graph.edge_index[:, p].contiguous(),
                                      graph.x_e[p].contiguous()))
        assert out._pf[2].mode == mode
        res[mode] = hard_schedule(out, ci.cuda(), "budget")
        check_rounding(f"order {mode}", res[mode], graph.edge_index[:, p], ci, G, NF, NC)
    base = res[Layout.FIBER_MAJOR]
    assert int((base.phase & 1).sum()) > 0 and int(base.visits.max()) >= 2
    for mode, p in orders.items():
        assert torch.equal(res[mode].visits, base.visits[p.cuda()]), mode
        assert torch.equal(res[mode].quot, base.quot[p.cuda()]), mode
        for k in ("n", "fiber_time", "completeness", "utility", "over", "worst", "phase"):
            assert torch.equal(getattr(res[mode], k), getattr(base, k)), (mode, k)


def test_graph0_in_its_own_order():
    import pfsgnn
    from oracle.ref_gnn import GNN as OracleGNN
    from pfsgnn.gnn import Layout
    from pfsgnn.train import hard_schedule
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "graph0.npz"))
    ei = torch.as_tensor(z["edge_index"].astype(np.int64))
    E, NF, NC = ei.shape[1], 2000, 12
    gen = torch.Generator().manual_seed(3)
    x_t = torch.as_tensor(z["x_t"]).double()
    x_s = 0.1 * torch.randn(NF, 10, generator=gen, dtype=torch.float64)
    x_e = torch.randn(E, 10, generator=gen, dtype=torch.float64)
    torch.manual_seed(5)
    mo = OracleGNN(B=2, Fdim=10, T=12, F_s=10, F_t=10).double()
    with torch.no_grad():
        mo.decoder_e[2].bias += 1.0
    gnn = pfsgnn.GNN(B=2, Fdim=10, T=12, F_s=10, F_t=10).cuda()
    gnn.load_state_dict({k: v.float() for k, v in mo.state_dict().items()})
    out = gnn(pfsgnn.BipartiteData(ei, x_s.float(), x_t.float(), x_e.float(), torch.zeros(1, 10)))
    assert out._pf[2].mode == Layout.PERM
    ci = x_t[:, :2].float().clone()
    ci[:, 0] = torch.round(ci[:, 0] * 4) / 4               # the 1/4 grid: exact sums
    hs = hard_schedule(out, ci.cuda(), "budget")
    r64, r32 = _refs(mo, out.x_e, ei, ci, 1, NF, NC)
    check_quot("graph0", hs.quot, r64, r32)
    check_rounding("graph0", hs, ei, ci, 1, NF, NC)


def test_sliced_product_and_time(sliced_layouts):
    """A general batch through ``hard_schedule``; and ``time=`` (the loop's best
    time vector) rounds to the same schedule as the graph's own edge times."""
    import test_gpu_sparse_loss as sparse_loss
    from pfsgnn.train import hard_schedule
    case = sparse_loss.CASES[1]
    G, NF, NC, density, B, dup, _, ec, F, _ = case
    model, graph, _ = sparse_loss.problem(case)
    ci = graph.x_t.float().clone()
    out = _gnn(model, B, F)(_data(graph))
    assert out._pf[2].sp is not None and out._pf[2].sp.sl is not None
    hs = hard_schedule(out, ci.cuda(), "budget")
    assert out.__dict__.get("_x_e_val") is None
    r64, r32 = _refs(model, out.x_e, graph.edge_index, ci, G, NF, NC)
    check_quot("sliced-product", hs.quot, r64, r32)
    check_rounding("sliced-product", hs, graph.edge_index, ci, G, NF, NC)
    time = hs.quot * ci.cuda()[graph.edge_index[1].cuda(), 0]
    ht = hard_schedule(out, ci.cuda(), "budget", time=time)
    check_rounding("sliced-product time=", ht, graph.edge_index, ci, G, NF, NC)
    with pytest.raises(ValueError, match="budget"):
        hard_schedule(out, ci.cuda(), "floor", time=time)
    with pytest.raises(ValueError, match="rounding"):
        hard_schedule(out, ci.cuda(), "ceil")


# ================================================================ op level
def op_run(hb, d, i, y_dev, mode=2, perm=None, out=None, time_in=None):
    from pfsgnn.train import BudgetSchedule
    dev = i.setdefault("_dev", {})
    for k in ("sc", "sh", "Wd1", "bd1", "Wd2", "bd2"):
        if k not in dev:
            dev[k] = i[k].cuda().contiguous()
    if "ci" not in dev:                                    # (copied once, before any capture)
        dev["ci"] = i["ci"].t().cuda().contiguous()
    cid = dev["ci"]
    if time_in is not None:
        return BudgetSchedule(*hb.schedule_budget(d, None, None, None, None, None, None, None, cid,
                                                  i["scale"], TOTAL_TIME, NFIELDS, mode=mode,
                                                  perm=perm, time_in=time_in, out=out))
    return BudgetSchedule(*hb.schedule_budget(d, y_dev, dev["sc"], dev["sh"], dev["Wd1"], dev["bd1"],
                                              dev["Wd2"], dev["bd2"], cid, i["scale"], TOTAL_TIME,
                                              NFIELDS, mode=mode, perm=perm, out=out))


def op_bufs(d, fill=-1):
    i32 = dict(dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    nan = float("nan")
    return (torch.full((d.E,), fill, **i32), torch.full((d.NT,), fill, **i32),
            torch.full((d.NS,), nan, **f32), torch.full((d.NT,), nan, **f32),
            torch.full((d.G,), nan, **f32), torch.full((d.G,), fill, **i32),
            torch.full((d.G,), nan, **f32), torch.full((d.E,), nan, **f32),
            torch.full((d.NS,), fill, **i32))


def test_dense_op_at_the_class_limit(hb):
    """NC = pfsgnn_schedule_budget_max_nc(): the largest LDS tile; one more class
    is refused before any launch."""
    from pfsgnn.engine import Dims
    NC = hb.schedule_budget_max_nc()
    assert NC >= 128
    G, NF, F = 1, 70, 10
    ei = class_major_edges(G, NF, NC)
    i = op_inputs(G, NF, NC, F, ei, 611)
    d = Dims(G, NF, NC, F)
    hs = op_run(hb, d, i, i["y"].cuda().contiguous(), out=op_bufs(d))
    assert int((hs.visits < 0).sum()) == 0 and int((hs.phase < 0).sum()) == 0
    r64, r32 = op_refs(i, ei, G, NF, NC, F, "floor")
    check_quot("max_nc", hs.quot, r64, r32)
    r = check_rounding("max_nc", hs, ei, i["ci"], G, NF, NC)
    assert (r["phase"] & 1).all()                          # 192 floors never fit 42
    d1 = Dims(G, NF, NC + 1, F)
    with pytest.raises(RuntimeError, match="pfsgnn_schedule_budget_max_nc"):
        hb.schedule_budget(d1, torch.zeros(F, d1.E, device="cuda"), None, None, i["_dev"]["Wd1"],
                           i["_dev"]["bd1"], i["_dev"]["Wd2"], i["_dev"]["bd2"],
                           torch.ones(2, NC + 1, device="cuda"), 1.0, TOTAL_TIME, NFIELDS, mode=2)


SLICED = [("hub", 10), ("hub", 16), ("complete", 10), ("one_class", 10), ("one_fiber_block", 8),
          ("ragged", 10)]


@pytest.mark.parametrize("case,F", SLICED)
def test_sliced_op(hb, case, F):
    """tests/sliced_ops_case.py's graphs: the hub (step-less slices, padding-heavy,
    NC at the sliced limit, absent fibers), NC = 1 with repeated pairs, the block
    whose only fiber is edgeless, ragged with 17 repeated pairs."""
    ncmax = min(128, hb.sliced_max_nc(F))
    G, NF, NC, ei = soc.case_edges(case, ncmax)
    i = op_inputs(G, NF, NC, F, ei, 900 + soc.CASES.index(case) + F)
    R = soc.hip_sliced_run(hb, ei, G, NF, NC, F)
    y = R.edge_in(i["y"])
    hs = op_run(hb, R.d, i, y, out=op_bufs(R.d))
    assert int((hs.visits < 0).sum()) == 0                 # every caller edge written
    r64, r32 = op_refs(i, ei, G, NF, NC, F, "floor")
    check_quot(f"sliced {case} F{F}", hs.quot, r64, r32)
    check_rounding(f"sliced {case} F{F}", hs, ei, i["ci"], G, NF, NC)
    nof = torch.bincount(ei[0], minlength=G * NF) == 0
    assert bool((hs.fiber_time.cpu()[nof] == 0).all()) and bool((hs.phase.cpu()[nof] == 0).all())
    again = op_run(hb, R.d, i, y)
    for a, b in zip(hs, again):
        assert torch.equal(a, b)


def test_sliced_matches_dense_on_the_complete_graph(hb):
    from pfsgnn.engine import Dims
    F = 10
    G, NF, NC, ei = soc.case_edges("complete")
    i = op_inputs(G, NF, NC, F, ei, 77)
    R = soc.hip_sliced_run(hb, ei, G, NF, NC, F)
    a = op_run(hb, R.d, i, R.edge_in(i["y"]))
    yc = i["y"].reshape(F, G, NF, NC).permute(0, 1, 3, 2).reshape(F, -1).contiguous().cuda()
    b = op_run(hb, Dims(G, NF, NC, F), i, yc, mode=1)
    assert int(a.visits.max()) >= 2 and int((a.phase & 2).sum()) > 0
    for k, x, y in zip(FIELDS, a, b):
        assert torch.equal(x, y), k


# ---------------------------------------------------------------- time_in, crafted
def _time_case(hb, ei, G, NF, NC, T, time, sliced, F=10):
    """``time`` [E] and ``T`` [G*NC] given directly -> (schedule, reference)."""
    from pfsgnn.engine import Dims
    ci = torch.stack([torch.as_tensor(T, dtype=torch.float32),
                      torch.full((G * NC,), 500.0)], 1)
    i = dict(scale=1.0, ci=ci, _dev={k: None for k in ("sc", "sh", "Wd1", "bd1", "Wd2", "bd2")})
    time = torch.as_tensor(time, dtype=torch.float32)
    if sliced:
        d, mode = soc.hip_sliced_run(hb, ei, G, NF, NC, F).d, 1
    else:
        d, mode = Dims(G, NF, NC, F), 1                    # ``ei`` fiber-major
    hs = op_run(hb, d, i, None, mode=mode, time_in=time.cuda(), out=op_bufs(d))
    q, inert = quotient(time.numpy(), ci[ei[1], 0].numpy())
    assert np.array_equal(hs.quot.cpu().numpy(), q)        # one IEEE division: bitwise
    r = check_rounding("time_in", hs, ei, ci, G, NF, NC, inert=inert)
    return hs, r


@pytest.mark.parametrize("sliced", [False, True])
def test_time_in_all_fracs_equal(hb, sliced):
    """Pure tie-break: every quotient 0.5, T = 10 -> each fiber bumps its four
    lowest classes (40 <= 42) and refuses the rest."""
    G, NF, NC = 2, 70, 9
    ei = canonical_edges(G, NF, NC)
    hs, r = _time_case(hb, ei, G, NF, NC, [10.0] * (G * NC), torch.full((ei.shape[1],), 5.0), sliced)
    want = (ei[1] % NC < 4).int()
    assert torch.equal(hs.visits.cpu(), want) and bool((hs.phase == 6).all())
    assert torch.equal(hs.n.cpu(), torch.tensor([NF] * 4 + [0] * 5, dtype=torch.int32).repeat(G))


def test_time_in_repeated_pair_on_a_sliced_batch(hb):
    """Fiber 0 holds class 1 three times (positions 1, 4, 6) with equal frac, and
    time for two bumps: the two lower positions get them."""
    G, NF, NC = 1, 3, 3
    ei = torch.tensor([[0, 0, 1, 2, 0, 1, 0, 2], [2, 1, 0, 0, 1, 2, 1, 1]])
    T = [20.0, 20.0, 50.0]
    time = torch.tensor([25.0, 10.0, 30.0, 70.0, 10.0, 10.0, 10.0, 30.0])
    hs, r = _time_case(hb, ei, G, NF, NC, T, time, True)
    # fiber 0: class 2 (T 50) never fits; class 1 x 3 at frac 0.5: positions 1 and 4
    assert hs.visits.cpu().tolist()[:2] == [0, 1] and hs.visits.cpu().tolist()[4] == 1
    assert hs.visits.cpu().tolist()[6] == 0
    # fiber 2: floors 3 x 20 + 1 x 20 = 80 > 42: the down phase takes the class 0 edge
    # (frac 0.5, lower class) to 1 and stops at 40; the class 1 edge keeps its floor
    assert hs.visits.cpu().tolist()[3] == 1 and hs.visits.cpu().tolist()[7] == 1
    assert int(hs.phase[2]) == 1 | 4


def test_time_in_inert_class_nan_time_exact_floor_and_strip(hb):
    """One inert class (T = 0), one NaN time, a fiber whose floor alone equals the
    budget, and a fiber the down phase strips to zero."""
    G, NF, NC = 1, 4, 4
    ei = canonical_edges(G, NF, NC)
    T = [0.0, 21.0, 7.0, 50.0]
    time = torch.tensor([[5.0, 21.0, 7.0, 10.0],            # floors 1 x 21 + 1 x 7 = 28; +7, no +21
                         [5.0, float("nan"), 20.0, 10.0],  # a NaN time: inert edge
                         [5.0, 42.5, 1.0, 10.0],            # floor 2 x 21 = 42: the budget exactly
                         [5.0, 1.0, 1.0, 170.0]]).reshape(-1)   # 3 x 50 > 42: stripped to zero
    hs, r = _time_case(hb, ei, G, NF, NC, T, time, False)
    v = hs.visits.cpu().reshape(NF, NC)
    assert bool((v[:, 0] == 0).all()) and int(v[1, 1]) == 0
    assert v[2].tolist() == [0, 2, 0, 0] and int(hs.phase[2]) == 4
    assert float(hs.fiber_time[2]) == TOTAL_TIME
    assert int(v[3, 3]) == 0 and int(hs.phase[3]) & 1
    assert bool(torch.isfinite(hs.fiber_time).all()) and int(hs.n[0]) == 0


# ================================================================ capture
def test_capture(hb):
    from pfsgnn.engine import Dims
    from test_gpu_hard_schedule import _captured_equals_eager
    G, NF, NC, F = 2, 70, 9, 10
    i = op_inputs(G, NF, NC, F, class_major_edges(G, NF, NC), 31)
    d = Dims(G, NF, NC, F)
    y = i["y"].cuda().contiguous()
    op_run(hb, d, i, y)                                    # (the workspace, before any capture)
    _captured_equals_eager(lambda out: op_run(hb, d, i, y, out=out), op_bufs(d))
    G, NF, NC, ei = soc.case_edges("ragged")
    i = op_inputs(G, NF, NC, F, ei, 32)
    R = soc.hip_sliced_run(hb, ei, G, NF, NC, F)
    ys = R.edge_in(i["y"])
    op_run(hb, R.d, i, ys)
    _captured_equals_eager(lambda out: op_run(hb, R.d, i, ys, out=out), op_bufs(R.d))


# ================================================================ TrainLoop
NEPOCHS, RUN = 8, 6


def _make_loop(prob, capture, track_hard):
    import pfsgnn
    from pfsgnn.train import TrainLoop
    model, graph = prob
    gnn = _gnn(model, 3, 10)
    opt = pfsgnn.FusedAdam(gnn.parameters(), lr=1e-3, capturable=True)
    loop = TrainLoop(gnn, opt, _data(graph), graph.x_t.float().cuda(), NEPOCHS, [0, 20], 5.0, 0.1,
                     0.1, seed=77, capture=capture, track_hard=track_hard)
    return loop.run(RUN)


def test_train_loop_tracks_the_budget_schedule():
    """The reference shape cut to 1 x 64 x 12 (B = 3, Fdim 10)."""
    prob = make_problem(1, 64, 12, B=3, seed=3)
    replay, eager = _make_loop(prob, True, "budget"), _make_loop(prob, False, "budget")
    assert replay._graph is not None                       # the epoch still captures
    floor, named = _make_loop(prob, True, True), _make_loop(prob, True, "floor")
    hr, he, hf, hn = (l.history() for l in (replay, eager, floor, named))
    for k in hr:
        assert np.array_equal(hr[k], he[k]), k             # replay equals eager, bitwise
    br, be = replay.hard_best(), eager.hard_best()
    assert br.keys() == be.keys() == floor.hard_best().keys()
    for k in br:
        assert np.array_equal(br[k], be[k]), k
    assert (hr["hard_overtime"] == 0).all()
    assert (hr["hard_objective"] >= hf["hard_objective"]).all()
    # the same soft training, so the last epoch rounds the same quotients: no fiber is
    # in the down phase here, every count is its floor or one more, and time is used
    hb_, hf_ = replay._hard, floor._hard
    assert int((hb_.phase & 1).sum()) == 0 and int((hb_.phase & 2).sum()) > 0
    assert bool(((hb_.visits - hf_.visits) >= 0).all()) and bool(((hb_.visits - hf_.visits) <= 1).all())
    assert int(hb_.visits.sum()) > int(hf_.visits.sum())
    assert torch.equal(torch.floor(hb_.quot).int(), hf_.visits)
    assert float(hb_.fiber_time.max()) <= TOTAL_TIME and bool((hb_.n >= hf_.n).all())
    assert (br["fiber_time"] <= TOTAL_TIME).all() and br["visits"].dtype == np.int32
    for k in ("losses", "objective", "variances", "completions"):
        assert np.array_equal(hr[k], hf[k]), k             # the soft run is untouched
    # True and "floor" are the floor path: the same history, and the one the
    # epoch-by-epoch floor evaluation gives (tests/test_gpu_hard_schedule.py)
    for k in hf:
        assert np.array_equal(hf[k], hn[k]), k
    from test_gpu_hard_schedule import _host_epoch
    import pfsgnn
    from pfsgnn.train import TrainLoop
    gnn = _gnn(prob[0], 3, 10)
    opt = pfsgnn.FusedAdam(gnn.parameters(), lr=1e-3, capturable=True)
    host = TrainLoop(gnn, opt, _data(prob[1]), prob[1].x_t.float().cuda(), NEPOCHS, [0, 20], 5.0,
                     0.1, 0.1, seed=77, capture=False, track_hard=False)
    rows = [_host_epoch(host) for _ in range(RUN)]
    assert hf["hard_objective"].tolist() == [float(r[4].sum()) for r in rows]   # G = 1
    assert hf["hard_overtime"].tolist() == [int(r[5].sum()) for r in rows]
