"""The hard (integer) schedule on the HIP library: pfsgnn_schedule
(csrc/pfsgnn_schedule.hip) at op level and through ``pfsgnn.train.hard_schedule``
/ ``TrainLoop(track_hard=True)``, against the float64 reference of
tests/hard_schedule_ref.py.

Visits against float64 (hard_schedule_ref.check_visits): the reference is fed
the device's own edge state, so only the decoder arithmetic differs; with err32
the error of the same reference in float32 and delta = 16 x err32, an edge whose
float64 quotient is farther than delta from the nearest integer (floor) or
half-integer (round) must match exactly, any other may differ by 1.  Every case
first asserts on the reference that at most 1 % of its edges are undecided,
that >= 25 % of them have visits >= 1 and that >= 3 distinct counts occur.

Everything else is exact consistency of the device's own outputs: n is the
integer scatter of visits; fiber_time is within (deg(f) - 1) x 2^-24 relative of
the float64 sum of the fp32 terms visits x T (the bound for a sum of
non-negative fp32 terms in any order); completeness within 1 ulp of torch's
fp32 n / (N / NFIELDS); utility bitwise the minimum of the returned
completeness; over and worst exactly those of the returned fiber_time.

With PFSGNN_HARD_SCHEDULE_ERRORS=<file> the module writes err32 and the
undecided counts of every case (profiles/hard_schedule_errors.txt).
"""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hard_schedule_ref import check_visits, hard_schedule_ref  # noqa: E402
from harness import canonical_edges, make_problem  # noqa: E402
from oracle.ref_gnn import GNN as OracleGNN  # noqa: E402
import sliced_ops_case as soc  # noqa: E402

TOTAL_TIME, NFIELDS = 42.0, 10
_TABLE = {}


@pytest.fixture(scope="module")
def hb():
    from pfsgnn.native import HipBackend
    return HipBackend()


@pytest.fixture(scope="module", autouse=True)
def error_table():
    yield
    path = os.environ.get("PFSGNN_HARD_SCHEDULE_ERRORS")
    if path and _TABLE:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_hard_schedule.py: err32 = max |v32 - v64| of the reference's quotient\n"
                    "# time / T, and the edges within 16 x err32 of a rounding boundary (undecided)\n"
                    "# case edges err32 undecided\n")
            for name, (E, err32, undec) in sorted(_TABLE.items()):
                f.write(f"{name} {E} {err32:.3e} {undec}\n")


@pytest.fixture
def sliced_layouts(monkeypatch):
    from pfsgnn import gnn
    monkeypatch.setenv("PFSGNN_SLICED", "1")
    gnn._LAYOUT_CACHE.clear()
    yield
    gnn._LAYOUT_CACHE.clear()


def compare(name, hs, r64, r32, rounding):
    err32, undec = check_visits(name, hs.visits, r64, r32, rounding)
    _TABLE[name + ":" + rounding] = (r64["visits"].numel(), err32, undec)


def check_consistency(name, hs, ei, ci, G, NF, NC):
    """``ci`` [G*NC, 2] float32 on the CPU (what the device read)."""
    src, tgt = ei[0].long(), ei[1].long()
    vis = hs.visits.cpu().long()
    n = torch.zeros(G * NC, dtype=torch.long).index_add_(0, tgt, vis)
    assert torch.equal(hs.n.cpu().long(), n), name
    terms = vis.float() * ci[tgt, 0]                          # the fp32 products
    ft64 = torch.zeros(G * NF, dtype=torch.float64).index_add_(0, src, terms.double())
    deg = torch.bincount(src, minlength=G * NF)
    bound = (deg - 1).clamp(min=0).double() * 2.0 ** -24 * ft64
    err = (hs.fiber_time.cpu().double() - ft64).abs()
    assert bool((err <= bound).all()), (name, float((err - bound).max()))
    assert bool((hs.fiber_time.cpu()[deg == 0] == 0).all()), name
    # torch's fp32 quotient on the host (IEEE divisions); the same expression on
    # the device is printed beside it
    want = hs.n.cpu().float() / (ci[:, 1] / NFIELDS)
    ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
    got = hs.completeness.cpu()
    dev = (hs.n.float() / (ci.cuda()[:, 1] / NFIELDS)).cpu()
    print(f"{name}: completeness vs host torch {float(((got - want).abs() / ulp).max()):.2f} ulp, "
          f"vs device torch {float(((got - dev).abs() / ulp).max()):.2f} ulp")
    assert bool(((got - want).abs() <= ulp).all()), name
    assert torch.equal(hs.utility, hs.completeness.view(G, NC).min(dim=1).values), name
    ft = hs.fiber_time.view(G, NF)
    assert torch.equal(hs.over.long(), (ft > TOTAL_TIME).sum(dim=1)), name
    assert torch.equal(hs.worst, ft.max(dim=1).values), name
    assert hs.visits.dtype == hs.n.dtype == hs.over.dtype == torch.int32


# ================================================================ product level
def _gnn(model, B, F, train=True):
    import pfsgnn
    gnn = pfsgnn.GNN(B=B, Fdim=F, T=12, F_s=1, F_t=2).cuda()
    gnn.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    gnn.train(train)
    return gnn


def _data(graph, ei=None, xe=None):
    import pfsgnn
    return pfsgnn.BipartiteData(graph.edge_index if ei is None else ei, graph.x_s.float(),
                                graph.x_t.float(), (graph.x_e if xe is None else xe).float(),
                                graph.x_u.float())


def _refs(model, x_e, ei, ci, G, NF, NC, rounding):
    """float64 and float32 reference on the device's materialised x_e [E, F]."""
    x = x_e.detach().cpu()
    r64 = hard_schedule_ref(model, x.double(), ei, ci.double(), G, NF, NC, rounding)
    r32 = hard_schedule_ref(copy.deepcopy(model).float(), x, ei, ci, G, NF, NC, rounding)
    return r64, r32


# (G, NF, NC, F, B, seed, T_i scale): NF = 70 a partial 64-fiber group; NC = 9
# KS = 3 with an idle wave; NC = 5 an uneven last split; NC = 1
DENSE = [(2, 70, 9, 10, 2, 5, 0.25), (1, 33, 5, 16, 2, 3, 1.0), (2, 40, 12, 8, 2, 7, 0.125),
         (2, 70, 1, 10, 2, 9, 1.0)]


@pytest.mark.parametrize("rounding", ["floor", "round"])
@pytest.mark.parametrize("case", DENSE)
def test_dense_product(case, rounding):
    from pfsgnn.train import hard_schedule
    G, NF, NC, F, B, seed, tscale = case
    model, graph = make_problem(G, NF, NC, F=F, B=B, seed=seed)
    ci = graph.x_t.float().clone()
    ci[:, 0] *= tscale
    gnn = _gnn(model, B, F)
    out = gnn(_data(graph))
    hs = hard_schedule(out, ci.cuda(), rounding)
    assert out.__dict__.get("_x_e_val") is None            # the lazy state was read
    assert not any(t.requires_grad for t in hs)
    r64, r32 = _refs(model, out.x_e, graph.edge_index, ci, G, NF, NC, rounding)
    compare(f"dense {G}x{NF}x{NC} F{F}", hs, r64, r32, rounding)
    check_consistency(str(case), hs, graph.edge_index, ci, G, NF, NC)


def test_eval_mode_and_no_grad():
    from pfsgnn.train import hard_schedule
    G, NF, NC, F, B, seed, tscale = DENSE[0]
    model, graph = make_problem(G, NF, NC, F=F, B=B, seed=seed)
    ci = graph.x_t.float().clone()
    ci[:, 0] *= tscale
    gnn = _gnn(model, B, F, train=False)
    with torch.no_grad():
        out = gnn(_data(graph))
        hs = hard_schedule(out, ci.cuda(), gnn=gnn)
    r64, r32 = _refs(model, out.x_e, graph.edge_index, ci, G, NF, NC, "floor")
    check_visits("eval", hs.visits, r64, r32, "floor")
    check_consistency("eval", hs, graph.edge_index, ci, G, NF, NC)


def test_edge_orders():
    """One batch fiber-major, canonical (class-major) and under a seeded random
    permutation: visits bitwise the fiber-major result re-indexed; n,
    fiber_time, utility bitwise equal."""
    from pfsgnn.gnn import Layout
    from pfsgnn.train import hard_schedule
    G, NF, NC, F, B, seed, tscale = DENSE[0]
    model, graph = make_problem(G, NF, NC, F=F, B=B, seed=seed)
    ci = graph.x_t.float().clone()
    ci[:, 0] *= tscale
    E = G * NF * NC
    e = torch.arange(E)
    g, f, c = e // (NF * NC), (e // NC) % NF, e % NC
    orders = {Layout.FIBER_MAJOR: e, Layout.CANONICAL: torch.argsort((g * NC + c) * NF + f),
              Layout.PERM: torch.randperm(E, generator=torch.Generator().manual_seed(11))}
    res = {}
    for mode, p in orders.items():
        gnn = _gnn(model, B, F)
        out = gnn(_data(graph, graph.edge_index[:, p].contiguous(), graph.x_e[p].contiguous()))
        assert out._pf[2].mode == mode
        res[mode] = hard_schedule(out, ci.cuda())
        check_consistency(f"order {mode}", res[mode], graph.edge_index[:, p], ci, G, NF, NC)
    base = res[Layout.FIBER_MAJOR]
    assert int(base.visits.max()) >= 2
    for mode, p in orders.items():
        assert torch.equal(res[mode].visits, base.visits[p.cuda()]), mode
        for k in ("n", "fiber_time", "completeness", "utility", "over", "worst"):
            assert torch.equal(getattr(res[mode], k), getattr(base, k)), (mode, k)


def test_graph0_in_its_own_order():
    """graphs/graph-0.pt's edge_index (each fiber's classes in argsort order: a
    permutation layout, on which loss_function refuses) against the reference;
    its T_i column x 0.25 so that the counts spread."""
    import pfsgnn
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
    gnn = pfsgnn.GNN(B=2, Fdim=10, T=12, F_s=10, F_t=10).cuda()
    gnn.load_state_dict({k: v.float() for k, v in mo.state_dict().items()})
    out = gnn(pfsgnn.BipartiteData(ei, x_s.float(), x_t.float(), x_e.float(), torch.zeros(1, 10)))
    assert out._pf[2].mode == Layout.PERM
    ci = x_t[:, :2].float().clone()
    ci[:, 0] *= 0.25
    for rounding in ("floor", "round"):
        hs = hard_schedule(out, ci.cuda(), rounding)
        r64, r32 = _refs(mo, out.x_e, ei, ci, 1, NF, NC, rounding)
        compare("graph0", hs, r64, r32, rounding)
        check_consistency("graph0", hs, ei, ci, 1, NF, NC)


def test_refusals(sliced_layouts, monkeypatch):
    import pfsgnn
    from pfsgnn import gnn as gnn_mod
    from pfsgnn.train import hard_schedule
    import test_gpu_sparse_loss as sparse_loss
    model, graph = make_problem(1, 8, 3, B=1, seed=1)
    gnn = _gnn(model, 1, 10)
    ci = graph.x_t.float().cuda()
    out = gnn(_data(graph))
    with pytest.raises(NotImplementedError, match="different GNN"):
        hard_schedule(out, ci, gnn=_gnn(model, 1, 10))
    out.x_e = out.x_e + 1
    with pytest.raises(NotImplementedError, match="x_e"):
        hard_schedule(out, ci)
    with pytest.raises(NotImplementedError, match="GNN.forward"):
        hard_schedule(_data(graph), ci)
    # a general batch on the composed path
    case = sparse_loss.CASES[2]
    model, graph, _ = sparse_loss.problem(case)
    monkeypatch.setenv("PFSGNN_SLICED", "0")
    gnn_mod._LAYOUT_CACHE.clear()
    out = _gnn(model, case[4], case[8])(_data(graph))
    with pytest.raises(NotImplementedError, match="composed path"):
        hard_schedule(out, graph.x_t.float().cuda())


# ================================================================ op level
def class_major_edges(G, NF, NC):
    """edge_index in the kernels' canonical order e = (g*NC + c)*NF + f."""
    e = torch.arange(G * NF * NC)
    gc, f = e // NF, e % NF
    return torch.stack([(gc // NC) * NF + f, gc])


def op_inputs(G, NF, NC, F, ei, seed):
    """Random lazy edge state [F, E] (caller's order), a decoder, class_info, and
    the scale (on a 1/8 grid) that puts the median of the float64 quotient
    time / T at about 1.5, so that the counts spread."""
    gen = torch.Generator().manual_seed(seed)
    E = ei.shape[1]
    i = {}
    i["y"] = soc.r(F, E, gen=gen).float()
    i["sc"] = (soc.r(F, gen=gen) * 0.3 + 1).float()
    i["sh"] = soc.nonzero(soc.q(soc.r(F, gen=gen), 1 / 8), 1 / 8).float()
    i["Wd1"], i["bd1"] = soc.r(F, F, scale=0.4, gen=gen).float(), soc.r(F, gen=gen).float()
    i["Wd2"], i["bd2"] = soc.r(1, F, scale=0.6, gen=gen).float(), soc.r(1, gen=gen).float() + 1.0
    T = torch.randint(2, 13, (G * NC,), generator=gen).float() * 0.25
    N = torch.randint(100, 2000, (G * NC,), generator=gen).float()
    i["ci"] = torch.stack([T, N], 1)
    i["scale"] = 1.0
    v = op_refs(i, ei, G, NF, NC, F, "floor")[0]["v"]
    i["scale"] = max(0.125, round(8 * 1.5 / v.median().item()) / 8)
    return i


def op_model(i, F, dtype):
    m = OracleGNN(B=1, Fdim=F, T=12, F_s=1, F_t=2).to(dtype)
    with torch.no_grad():
        m.decoder_e[0].weight.copy_(i["Wd1"])
        m.decoder_e[0].bias.copy_(i["bd1"])
        m.decoder_e[2].weight.copy_(i["Wd2"])
        m.decoder_e[2].bias.copy_(i["bd2"])
    return m


def op_refs(i, ei, G, NF, NC, F, rounding):
    """The references on the same y, sc, sh: x = y * sc + sh formed in each
    dtype; ``total_time`` = scale * NC reproduces the op's scale."""
    out = []
    for dt in (torch.float64, torch.float32):
        x = (i["y"].to(dt) * i["sc"].to(dt)[:, None] + i["sh"].to(dt)[:, None]).t().contiguous()
        out.append(hard_schedule_ref(op_model(i, F, dt), x, ei, i["ci"].to(dt), G, NF, NC, rounding,
                                     total_time=i["scale"] * NC))
    # the flags of ``over`` are the op's own total_time, checked from fiber_time
    return out


def op_run(hb, d, i, y_dev, rounding, mode=2, perm=None, out=None):
    from pfsgnn.train import HardSchedule
    # (the device copies once, before any capture)
    dev = i.setdefault("_dev", {})
    for k in ("sc", "sh", "Wd1", "bd1", "Wd2", "bd2"):
        if k not in dev:
            dev[k] = i[k].cuda().contiguous()
    if "ci" not in dev:
        dev["ci"] = i["ci"].t().cuda().contiguous()
    return HardSchedule(*hb.schedule(d, y_dev, dev["sc"], dev["sh"], dev["Wd1"], dev["bd1"],
                                     dev["Wd2"], dev["bd2"], dev["ci"], i["scale"], TOTAL_TIME,
                                     NFIELDS, rounding={"floor": 0, "round": 1}[rounding], mode=mode,
                                     perm=perm, out=out))


def op_bufs(d, fill=-1):
    i32 = dict(dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    return (torch.full((d.E,), fill, **i32), torch.full((d.NT,), fill, **i32),
            torch.full((d.NS,), float("nan"), **f32), torch.full((d.NT,), float("nan"), **f32),
            torch.full((d.G,), float("nan"), **f32), torch.full((d.G,), fill, **i32),
            torch.full((d.G,), float("nan"), **f32))


BIG = (16, 2050, 24, 10)


@pytest.fixture(scope="module")
def big():
    """G = 16, NF = 2050, NC = 24: 33 fiber groups per graph = 528 groups, so
    make_geo (pfsgnn_common.h) gives ks = ceil(2048 / 528) = 4 <= ceil(24 / 4),
    CPS = 6, KS = 4 -- a wave walks 1-2 classes -- and the last group holds 2
    fibers."""
    G, NF, NC, F = BIG
    ei = class_major_edges(G, NF, NC)
    i = op_inputs(G, NF, NC, F, ei, 501)
    return ei, i, {r: op_refs(i, ei, G, NF, NC, F, r) for r in ("floor", "round")}


@pytest.mark.parametrize("rounding", ["floor", "round"])
def test_dense_op_big(hb, big, rounding):
    from pfsgnn.engine import Dims
    G, NF, NC, F = BIG
    ei, i, refs = big
    d = Dims(G, NF, NC, F)
    y = i["y"].cuda().contiguous()
    hs = op_run(hb, d, i, y, rounding, out=op_bufs(d))
    assert int((hs.visits < 0).sum()) == 0
    r64, r32 = refs[rounding]
    compare(f"dense-op {G}x{NF}x{NC}", hs, r64, r32, rounding)
    check_consistency("big", hs, ei, i["ci"], G, NF, NC)
    again = op_run(hb, d, i, y, rounding)
    for a, b in zip(hs, again):
        assert torch.equal(a, b)


def test_round_half_to_even_op(hb):
    """Wd2 = 0, bd2 = 30 (> softplus' threshold 20) and scale = 1 make time = 30
    exactly; T = 60, 20, 12 makes v = 0.5, 1.5, 2.5 exactly: rint gives 0, 2, 2
    (floor 0, 1, 2), on the dense and on the sliced kernel."""
    from pfsgnn.engine import Dims
    G, NF, NC, F = 2, 40, 12, 10
    ei = canonical_edges(G, NF, NC)                       # fiber-major
    i = op_inputs(G, NF, NC, F, ei, 7)
    i["Wd2"].zero_()
    i["bd2"].fill_(30.0)
    i["scale"] = 1.0
    i["ci"][:, 0] = torch.tensor([60.0, 20.0, 12.0]).repeat(G * NC // 3)
    cls = ei[1] % 3
    yc = i["y"].reshape(F, G, NF, NC).permute(0, 1, 3, 2).reshape(F, -1).contiguous().cuda()
    d = Dims(G, NF, NC, F)
    R = soc.hip_sliced_run(hb, ei, G, NF, NC, F)
    for rounding, want in (("round", [0, 2, 2]), ("floor", [0, 1, 2])):
        want = torch.tensor(want)[cls]
        assert torch.equal(op_run(hb, d, i, yc, rounding, mode=1).visits.cpu().long(), want)
        assert torch.equal(op_run(hb, R.d, i, R.edge_in(i["y"]), rounding).visits.cpu().long(), want)


SLICED = [("hub", 10), ("hub", 16), ("complete", 10), ("one_class", 10), ("one_fiber_block", 8),
          ("ragged", 10)]


@pytest.mark.parametrize("case,F", SLICED)
def test_sliced_op(hb, case, F):
    """tests/sliced_ops_case.py's graphs: the hub (slices of length 0-3 beside
    one of every class, EP / E ~ 7, NC = sliced_max_nc(F), absent fibers), NC =
    1, the block whose only fiber is edgeless."""
    ncmax = min(128, hb.sliced_max_nc(F))
    G, NF, NC, ei = soc.case_edges(case, ncmax)
    assert case != "hub" or NC == ncmax
    E = ei.shape[1]
    i = op_inputs(G, NF, NC, F, ei, 900 + soc.CASES.index(case) + F)
    R = soc.hip_sliced_run(hb, ei, G, NF, NC, F)
    sl = R.d.sp.sl
    if case == "hub":
        assert sl.EP >= 5 * E                              # mostly padding
    y = R.edge_in(i["y"])
    for rounding in ("floor", "round"):
        hs = op_run(hb, R.d, i, y, rounding, out=op_bufs(R.d))
        assert int((hs.visits < 0).sum()) == 0             # every caller edge written
        r64, r32 = op_refs(i, ei, G, NF, NC, F, rounding)
        compare(f"sliced-op {case} F{F}", hs, r64, r32, rounding)
        check_consistency(case, hs, ei, i["ci"], G, NF, NC)
        noc = torch.bincount(ei[1], minlength=G * NC) == 0
        nof = torch.bincount(ei[0], minlength=G * NF) == 0
        assert bool((hs.n.cpu()[noc] == 0).all()) and bool((hs.completeness.cpu()[noc] == 0).all())
        assert bool((hs.fiber_time.cpu()[nof] == 0).all())
        if case in ("hub", "ragged"):
            assert bool(noc.any()) and bool(nof.any())
        again = op_run(hb, R.d, i, y, rounding)
        for a, b in zip(hs, again):
            assert torch.equal(a, b)


def test_sliced_matches_dense_on_the_complete_graph(hb):
    from pfsgnn.engine import Dims
    F = 10
    G, NF, NC, ei = soc.case_edges("complete")
    i = op_inputs(G, NF, NC, F, ei, 77)
    R = soc.hip_sliced_run(hb, ei, G, NF, NC, F)
    a = op_run(hb, R.d, i, R.edge_in(i["y"]), "floor")
    yc = i["y"].reshape(F, G, NF, NC).permute(0, 1, 3, 2).reshape(F, -1).contiguous().cuda()
    b = op_run(hb, Dims(G, NF, NC, F), i, yc, "floor", mode=1)
    assert int(a.visits.max()) >= 2
    assert torch.equal(a.visits, b.visits) and torch.equal(a.n, b.n)
    # both sum the same NC fp32 terms per fiber, in different orders: each within
    # (NC - 1) x 2^-24 of the exact sum (check_consistency), so of each other twice that
    check_consistency("complete/sliced", a, ei, i["ci"], G, NF, NC)
    check_consistency("complete/dense", b, ei, i["ci"], G, NF, NC)
    diff = (a.fiber_time.double() - b.fiber_time.double()).abs()
    assert bool((diff <= 2 * (NC - 1) * 2.0 ** -24 * b.fiber_time.double()).all())


def test_sliced_product(sliced_layouts):
    import test_gpu_sparse_loss as sparse_loss
    from pfsgnn.train import hard_schedule
    case = sparse_loss.CASES[1]
    G, NF, NC, density, B, dup, _, ec, F, _ = case
    model, graph, _ = sparse_loss.problem(case)
    ci = graph.x_t.float().clone()
    ci[:, 0] *= 0.25
    out = _gnn(model, B, F)(_data(graph))
    assert out._pf[2].sp is not None and out._pf[2].sp.sl is not None
    res = {r: hard_schedule(out, ci.cuda(), r) for r in ("floor", "round")}
    assert out.__dict__.get("_x_e_val") is None            # the lazy state was read
    for rounding, hs in res.items():
        r64, r32 = _refs(model, out.x_e, graph.edge_index, ci, G, NF, NC, rounding)
        compare("sliced-product", hs, r64, r32, rounding)
        check_consistency("sliced-product", hs, graph.edge_index, ci, G, NF, NC)


# ================================================================ capture
def _captured_equals_eager(run, bufs):
    eager = [t.clone() for t in run(None)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(bufs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in bufs:
        t.fill_(-1) if t.dtype == torch.int32 else t.fill_(float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(bufs)
    for t in bufs:
        t.fill_(-1) if t.dtype == torch.int32 else t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, bufs):
        assert torch.equal(a, b)


def test_capture_dense(hb):
    from pfsgnn.engine import Dims
    G, NF, NC, F = 2, 70, 9, 10
    i = op_inputs(G, NF, NC, F, class_major_edges(G, NF, NC), 31)
    d = Dims(G, NF, NC, F)
    y = i["y"].cuda().contiguous()
    hb.workspace(d)
    _captured_equals_eager(lambda out: op_run(hb, d, i, y, "floor", out=out), op_bufs(d))


def test_capture_sliced(hb):
    F = 10
    G, NF, NC, ei = soc.case_edges("ragged")
    i = op_inputs(G, NF, NC, F, ei, 32)
    R = soc.hip_sliced_run(hb, ei, G, NF, NC, F)
    y = R.edge_in(i["y"])
    hb.workspace(R.d)
    _captured_equals_eager(lambda out: op_run(hb, R.d, i, y, "floor", out=out), op_bufs(R.d))


# ================================================================ TrainLoop
NEPOCHS, RUN = 8, 7


def _make_loop(prob, B, F, capture, track_hard, tscale=0.0625, lr=1e-3):
    import pfsgnn
    from pfsgnn.train import TrainLoop
    model, graph = prob
    gnn = _gnn(model, B, F)
    opt = pfsgnn.FusedAdam(gnn.parameters(), lr=lr, capturable=True)
    ci = graph.x_t.float().clone()
    ci[:, 0] *= tscale
    loop = TrainLoop(gnn, opt, _data(graph), ci.cuda(), NEPOCHS, [0, 20], 5.0, 0.1, 0.1, seed=77,
                     capture=capture, track_hard=track_hard)
    return loop, gnn, opt


def _host_epoch(loop):
    """TrainLoop._step's launches issued from here, eagerly, with the public
    ``hard_schedule`` on the epoch's forward."""
    from pfsgnn import train
    sharp = loop._advance()
    loop.gnn.zero_grad()
    out = loop.gnn(loop.graph)
    d, ci, outs = train._loss_apply(out, loop.class_info, loop.pclass, loop.pfiber, sharp, True,
                                    None, loop._seed, 0.3)
    loss, utils_g, n_prime, fiber_time, variance_g, time, loss_g = outs
    loop._record(d, ci, loss_g, utils_g, variance_g, n_prime)
    hs = train.hard_schedule(out, loop.class_info)
    loss.backward()
    loop.optimizer.step()
    loop._copy_if(time, fiber_time)
    loop.epoch += 1
    return [t.cpu() for t in hs]


def _soft_state(loop, gnn):
    torch.cuda.synchronize()
    out = {"param." + n: p.detach().cpu() for n, p in gnn.named_parameters()}
    out.update({"buffer." + n: b.detach().cpu() for n, b in gnn.named_buffers()})
    h = loop.history()
    out.update({"hist." + k: torch.as_tensor(h[k]) for k in ("losses", "objective", "variances",
                                                             "completions")})
    out.update({"best." + k: torch.as_tensor(v) for k, v in loop.best().items()})
    return out


def _train_loop_case(prob, B, F):
    hard, gnn_h, _ = _make_loop(prob, B, F, True, True)
    hard.run(RUN)
    assert hard._graph is not None                         # the epoch still captures
    host, gnn_e, _ = _make_loop(prob, B, F, False, False)
    rows = [_host_epoch(host) for _ in range(RUN)]
    h = hard.history()
    obj, over = [], []
    for r in rows:
        u, o = r[4].numpy(), r[5].numpy()
        su, so = u[0], o[0]
        for g in range(1, u.size):
            su, so = np.float32(su + u[g]), so + o[g]
        obj.append(su)
        over.append(so)
    assert h["hard_objective"].tolist() == [float(x) for x in obj]
    assert h["hard_overtime"].tolist() == [int(x) for x in over]
    best, best_e = np.float32(0.0), -1
    for e, u in enumerate(obj):
        if u > best:
            best, best_e = u, e
    hb_ = hard.hard_best()
    assert best_e >= 0 and len(set(float(x) for x in obj)) > 1
    assert hb_["epoch"] == best_e and hb_["utility"] == float(best)
    assert np.array_equal(hb_["visits"], rows[best_e][0].numpy())
    assert np.array_equal(hb_["fiber_time"], rows[best_e][2].numpy())
    assert np.array_equal(hb_["completion"], rows[best_e][3].numpy())
    # the soft run is untouched: the same captured loop without tracking, bitwise
    soft, gnn_s, _ = _make_loop(prob, B, F, True, False)
    soft.run(RUN)
    a, b = _soft_state(hard, gnn_h), _soft_state(soft, gnn_s)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert "hard_objective" not in soft.history()
    c = _soft_state(host, gnn_e)
    for k in a:
        assert torch.equal(a[k], c[k]), "eager " + k


def test_train_loop_tracks_hard_dense():
    _train_loop_case(make_problem(1, 200, 12, B=2, seed=3), 2, 10)


def test_train_loop_tracks_hard_sliced(sliced_layouts):
    import test_gpu_sparse_loss as sparse_loss
    case = sparse_loss.CASES[1]
    model, graph, _ = sparse_loss.problem(case)
    _train_loop_case((model, graph), case[4], case[8])
