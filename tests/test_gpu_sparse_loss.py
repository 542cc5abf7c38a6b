"""The training objective on general (non-complete) bipartite batches
(pfsgnn.train.loss_function on a sliced batch; csrc/pfsgnn_sl_loss.hip) against
the edge_index-indexed restatement of tests/general_loss_ref.py on the CPU
oracle.

The bar is tests/test_gpu_sparse.py's for the sliced kernels: every compared
tensor within max(16 x the fp32 oracle's own error (two edge orders),
6e-5 x its scale, 1e-6) of the float64 oracle.

The objective has a kink at softfloor = 0 (the clamp's gradient mask flips) and
where two classes tie for the minimum completeness; a case must not sit on
either, so every case first ASSERTS on the float64 reference that the smallest
|raw softfloor value| is >= 1e-4 (3e-5 for the 130-fiber case) and that each
graph's two smallest completeness values differ by >= 1 % of the second.
"""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from general_loss_ref import general_loss  # noqa: E402
from harness import make_problem  # noqa: E402
from noise_ref import uniform_numpy  # noqa: E402
from oracle.ref_gnn import Graph as OGraph  # noqa: E402
from test_sparse_emu import sparse_edges  # noqa: E402

TOL_K = 16.0
TOL_REL = 6e-5      # the sliced kernels run the default edge path's numerics (test_gpu_sparse.py)
PCLASS, PFIBER = 0.1, 0.1

# (G, NF, NC, density, B, dup, sharpness, empty_class, F, seed)
CASES = [(1, 40, 12, 0.5, 2, 3, 12.0, True, 10, 1),
         (2, 24, 16, 0.3, 2, 0, 5.0, False, 10, 1),
         (3, 10, 7, 0.7, 3, 4, 0.0, True, 10, 1),
         # three 64-fiber groups per graph, the last holding two fibers: empty
         # slice lanes and a multi-block class merge
         (2, 130, 24, 0.25, 2, 5, 8.0, True, 10, 16),
         (2, 40, 12, 0.4, 2, 3, 10.0, False, 8, 3),
         (2, 40, 12, 0.4, 2, 3, 10.0, False, 16, 7)]
BIG = CASES[3]
CAPTURED = CASES[1]


@pytest.fixture(autouse=True)
def _sliced_layouts(monkeypatch):
    from pfsgnn import gnn
    monkeypatch.setenv("PFSGNN_SLICED", "1")
    gnn._LAYOUT_CACHE.clear()
    yield
    gnn._LAYOUT_CACHE.clear()


def check(name, ours, r64, r32s, tol_rel=TOL_REL):
    ours = torch.as_tensor(ours).detach().double().cpu().reshape(-1)
    r64 = r64.detach().double().cpu().reshape(-1)
    scale = r64.abs().max().item()
    ref_err = max((t.detach().double().cpu().reshape(-1) - r64).abs().max().item() for t in r32s)
    err = (ours - r64).abs().max().item()
    bound = max(TOL_K * ref_err, tol_rel * scale, 1e-6)
    print(f"{name}: err {err:.3e} bound {bound:.3e} (oracle32 {ref_err:.3e}, scale {scale:.3e})")
    assert err <= bound, f"{name}: err {err:.3e} > bound {bound:.3e} (oracle32 {ref_err:.3e}, scale {scale:.3e})"


@functools.lru_cache(maxsize=None)
def problem(case):
    G, NF, NC, density, B, dup, sharp, ec, F, seed = case
    model, graph = make_problem(G, NF, NC, F=F, B=B, seed=G + NF)
    gen = torch.Generator().manual_seed(G + NF + 100)
    ei = sparse_edges(G, NF, NC, density, gen, dup=dup, empty_class=ec)
    E = ei.shape[1]
    xe = 2.0 + 8.0 * torch.rand(E, F, generator=gen, dtype=torch.float64)
    graph = OGraph(ei, graph.x_s, graph.x_t, xe, graph.x_u, graph.s_batch, graph.t_batch)
    uni = torch.as_tensor(uniform_numpy(seed, E), dtype=torch.float64)
    return model, graph, uni


def _oracle_step(model, graph, uni, dims, sharp, dtype, reverse=False, train=True):
    """GNN + general objective on the CPU oracle; results in the caller's edge order."""
    G, NF, NC = dims
    m = copy.deepcopy(model).to(dtype)
    m.train(train)
    ei, xe, u = graph.edge_index, graph.x_e, uni
    if reverse:
        ei, xe, u = ei.flip(1), xe.flip(0), u.flip(0)
    with torch.set_grad_enabled(train):
        out = m(OGraph(ei, graph.x_s.to(dtype), graph.x_t.to(dtype), xe.to(dtype),
                       graph.x_u.to(dtype), graph.s_batch, graph.t_batch))
        loss, diag = general_loss(m, out.x_e, ei, graph.x_t.to(dtype), G, NF, NC, pclass=PCLASS,
                                  pfiber=PFIBER, sharpness=sharp, uniform=u.to(dtype))
    if train:
        loss.backward()
    if reverse:
        diag["time"], diag["raw"] = diag["time"].flip(0), diag["raw"].flip(0)
    return dict(m=m, out=out, loss=loss.detach(), diag=diag)


def _assert_off_the_kinks(r64, dims, raw_min):
    G, NF, NC = dims
    got = r64["diag"]["raw"].abs().min().item()
    assert got >= raw_min, f"min |raw softfloor| {got:.3e} < {raw_min:.0e}: the case sits on the clamp's kink"
    comp = r64["diag"]["completeness"].reshape(G, NC)
    for g in range(G):
        lo = torch.sort(comp[g]).values[:2]
        assert (lo[1] - lo[0]).item() >= 0.01 * lo[1].item(), \
            f"graph {g}: the two smallest completeness values {lo.tolist()} nearly tie"


def _references(model, graph, uni, dims, sharp, train=True, raw_min=1e-4):
    r64 = _oracle_step(model, graph, uni, dims, sharp, torch.float64, train=train)
    _assert_off_the_kinks(r64, dims, raw_min)
    r32 = [_oracle_step(model, graph, uni, dims, sharp, torch.float32, reverse=rv, train=train)
           for rv in (False, True)]
    return r64, r32


@functools.lru_cache(maxsize=None)
def references(case, train=True):
    G, NF, NC, density, B, dup, sharp, ec, F, seed = case
    model, graph, uni = problem(case)
    return _references(model, graph, uni, (G, NF, NC), sharp, train=train,
                       raw_min=3e-5 if NF == 130 else 1e-4)


def _ours_model(model, B, F, train=True):
    import pfsgnn
    gnn = pfsgnn.GNN(B=B, Fdim=F, T=12, F_s=1, F_t=2).cuda()
    gnn.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    gnn.train(train)
    return gnn


def _ours_data(graph):
    import pfsgnn
    return pfsgnn.BipartiteData(graph.edge_index, graph.x_s.float(), graph.x_t.float(),
                                graph.x_e.float(), graph.x_u.float())


def _ours_step(model, graph, B, F, sharp, seed, train=True):
    from pfsgnn.train import loss_function
    gnn = _ours_model(model, B, F, train=train)
    data = _ours_data(graph)
    ci = graph.x_t.float().cuda()
    gnn.zero_grad()
    with torch.set_grad_enabled(train):
        out = gnn(data)
        loss, utils, comp, n_prime, fibers, time, var = loss_function(
            out, ci, pclass=PCLASS, pfiber=PFIBER, sharpness=sharp, finaloutput=True, seed=seed)
    if train:
        loss.backward()
    torch.cuda.synchronize()
    res = dict(loss=loss.detach(), utils=utils.detach(), comp=torch.as_tensor(comp),
               n_prime=n_prime.detach(), fiber_time=torch.as_tensor(fibers), time=time.detach(),
               variance=var.detach())
    return gnn, out, res


def _check_objective(res, r64, r32):
    d64, d32 = r64["diag"], [r["diag"] for r in r32]
    check("loss", res["loss"], r64["loss"], [r["loss"] for r in r32])
    check("utils", res["utils"], d64["utils"].sum(), [d["utils"].sum() for d in d32])
    check("variance", res["variance"], d64["variance"].sum(), [d["variance"].sum() for d in d32])
    for k in ("n_prime", "fiber_time", "time"):
        assert res[k].numel() == d64[k].numel(), k
        check(k, res[k], d64[k], [d[k] for d in d32])
    check("completeness", res["comp"], d64["completeness"], [d["completeness"] for d in d32])


def _check_step(gnn, out, res, r64, r32):
    _check_objective(res, r64, r32)
    for nm in ("x_s", "x_t", "x_u"):
        check(nm, getattr(out, nm), getattr(r64["out"], nm), [getattr(r["out"], nm) for r in r32])
    p64 = dict(r64["m"].named_parameters())
    p32 = [dict(r["m"].named_parameters()) for r in r32]
    for name, p in gnn.named_parameters():
        z = torch.zeros_like(p64[name])
        ours = p.grad if p.grad is not None else torch.zeros_like(p)
        assert torch.isfinite(ours).all(), name
        check("grad " + name, ours, p64[name].grad if p64[name].grad is not None else z,
              [q[name].grad if q[name].grad is not None else z.float() for q in p32])
    b64 = r64["m"].state_dict()
    for k, v in gnn.state_dict().items():
        if "running" in k or "num_batches" in k:
            check(k, v.double(), b64[k].double(), [r["m"].state_dict()[k].double() for r in r32])


def _all_sliced():
    from pfsgnn import gnn as gmod
    lays = [e[3] for e in gmod._LAYOUT_CACHE.d.values()]
    return bool(lays) and all(lay.sp is not None and lay.sp.sl is not None for lay in lays)


# ---------------------------------------------------------------- 1. full-step parity
@pytest.mark.parametrize("case", CASES, ids=[f"G{c[0]}-NF{c[1]}-NC{c[2]}-F{c[8]}" for c in CASES])
def test_full_step_matches_oracle(case):
    G, NF, NC, density, B, dup, sharp, ec, F, seed = case
    model, graph, uni = problem(case)
    r64, r32 = references(case)
    gnn, out, res = _ours_step(model, graph, B, F, sharp, seed)
    assert _all_sliced()
    _check_step(gnn, out, res, r64, r32)


# ---------------------------------------------------------------- 2. degenerate degrees
DEGEN_SEED = 1


@functools.lru_cache(maxsize=None)
def degenerate_problem():
    """G=1, NF=5, NC=3: class 2 has exactly one edge, fiber 4 none, pair (0, 0) twice."""
    model, graph = make_problem(1, 5, 3, B=2, seed=8)
    ei = torch.tensor([[0, 0, 1, 2, 3, 3, 0], [0, 1, 0, 1, 0, 2, 0]])
    gen = torch.Generator().manual_seed(108)
    xe = 2.0 + 8.0 * torch.rand(ei.shape[1], 10, generator=gen, dtype=torch.float64)
    graph = OGraph(ei, graph.x_s, graph.x_t, xe, graph.x_u, None, None)
    uni = torch.as_tensor(uniform_numpy(DEGEN_SEED, ei.shape[1]), dtype=torch.float64)
    return model, graph, uni


def test_degenerate_degrees():
    model, graph, uni = degenerate_problem()
    sharp = 6.0
    r64, r32 = _references(model, graph, uni, (1, 5, 3), sharp)
    assert r64["diag"]["deg"].tolist() == [4.0, 2.0, 1.0]
    assert r64["diag"]["var_c"][2].item() == 0.0
    gnn, out, res = _ours_step(model, graph, 2, 10, sharp, DEGEN_SEED)
    assert _all_sliced()
    assert torch.isfinite(res["loss"]).all()
    for name, p in gnn.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), name
    assert res["fiber_time"][4].item() == 0.0
    # class 2 (one edge) adds 0: the variance is that of classes 0 and 1 alone
    check("variance (classes 0, 1)", res["variance"], r64["diag"]["var_c"][:2].sum(),
          [r["diag"]["var_c"][:2].sum() for r in r32])
    _check_step(gnn, out, res, r64, r32)


# ---------------------------------------------------------------- 3. reproducibility
def test_step_is_bitwise_reproducible():
    G, NF, NC, density, B, dup, sharp, ec, F, seed = BIG
    model, graph, uni = problem(BIG)
    runs = [_ours_step(model, graph, B, F, sharp, seed) for _ in range(2)]
    (g1, _, a), (g2, _, b) = runs
    for k in a:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    for (n, p), (_, q) in zip(g1.named_parameters(), g2.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), n
    _, _, c = _ours_step(model, graph, B, F, sharp, seed + 1)
    assert c["loss"].item() != a["loss"].item()


# ---------------------------------------------------------------- 4. captured step
def test_captured_step_replays_bitwise():
    """forward + loss + backward of a general batch under HIP-graph capture, the
    seed a device int64 tensor: one replay equals the eager step bit for bit."""
    from pfsgnn.train import loss_function
    G, NF, NC, density, B, dup, sharp, ec, F, seed = CAPTURED
    model, graph, uni = problem(CAPTURED)

    def setup():
        gnn = _ours_model(model, B, F)
        return gnn, _ours_data(graph), graph.x_t.float().cuda(), \
            torch.full((), 41, dtype=torch.int64, device="cuda")

    def step(gnn, data, ci, sd):
        gnn.zero_grad()
        out = gnn(data)
        loss, _ = loss_function(out, ci, pclass=PCLASS, pfiber=PFIBER, sharpness=sharp, seed=sd)
        loss.backward()
        return loss

    def grads(gnn):
        return torch.cat([p.grad.reshape(-1) for p in gnn.parameters() if p.grad is not None]).cpu()

    gnn, data, ci, sd = setup()
    step(gnn, data, ci, sd)                      # warm-up (layout caches, workspace)
    eager = step(gnn, data, ci, sd).clone()
    torch.cuda.synchronize()
    e_loss, e_grads = eager.cpu(), grads(gnn)

    gnn, data, ci, sd = setup()
    step(gnn, data, ci, sd)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(gnn, data, ci, sd)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step(gnn, data, ci, sd)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static.cpu(), e_loss), (static.item(), e_loss.item())
    assert torch.equal(grads(gnn), e_grads)


# ---------------------------------------------------------------- 5. inference
def test_eval_mode_loss_matches_oracle():
    G, NF, NC, density, B, dup, sharp, ec, F, seed = CASES[0]
    model, graph, uni = problem(CASES[0])
    r64, r32 = references(CASES[0], False)
    gnn, out, res = _ours_step(model, graph, B, F, sharp, seed, train=False)
    assert _all_sliced()
    _check_objective(res, r64, r32)


# ---------------------------------------------------------------- 6. refusals
def test_refusals(monkeypatch):
    import pfsgnn
    from pfsgnn import gnn as gmod
    from pfsgnn.train import loss_function
    G, NF, NC, density, B, dup, sharp, ec, F, seed = CASES[1]
    model, graph, uni = problem(CASES[1])
    ci = graph.x_t.float().cuda()
    # a general batch on the composed path
    monkeypatch.setenv("PFSGNN_SLICED", "0")
    gmod._LAYOUT_CACHE.clear()
    gnn = _ours_model(model, B, F)
    out = gnn(_ours_data(graph))
    with pytest.raises(NotImplementedError, match="sliced"):
        loss_function(out, ci, seed=1)
    gmod._LAYOUT_CACHE.clear()
    monkeypatch.setenv("PFSGNN_SLICED", "1")
    # a complete batch whose edge order is not fiber-major
    cmodel, cgraph = make_problem(G, NF, NC, F=F, B=B, seed=3)
    perm = torch.randperm(cgraph.edge_index.shape[1], generator=torch.Generator().manual_seed(0))
    data = pfsgnn.BipartiteData(cgraph.edge_index[:, perm], cgraph.x_s.float(), cgraph.x_t.float(),
                                cgraph.x_e[perm].float(), cgraph.x_u.float())
    out = gnn(data)
    with pytest.raises(NotImplementedError, match="fiber-major"):
        loss_function(out, cgraph.x_t.float().cuda(), seed=1)


# ---------------------------------------------------------------- 7. class-sorted slices
NEAR_SEED = 1


@functools.lru_cache(maxsize=None)
def near_complete_problem():
    """A fiber-major complete batch with a few edges removed and one repeated:
    the k-th edge of most fibers of a slice has the same class, so the class
    statistics take the row-reduced path (one class per row of 16 lanes), and
    the slices of the shortened fibers the per-edge rounds."""
    G, NF, NC = 2, 70, 9
    model, graph = make_problem(G, NF, NC, B=2, seed=5)
    E0 = G * NF * NC
    keep = torch.ones(E0, dtype=torch.bool)
    keep[[3, 100, 101, 640, 1200]] = False
    idx = torch.cat([torch.nonzero(keep).flatten(), torch.tensor([17])])
    ei, xe = graph.edge_index[:, idx], graph.x_e[idx]
    graph = OGraph(ei, graph.x_s, graph.x_t, xe, graph.x_u, graph.s_batch, graph.t_batch)
    uni = torch.as_tensor(uniform_numpy(NEAR_SEED, ei.shape[1]), dtype=torch.float64)
    return model, graph, uni


def test_class_sorted_near_complete_batch():
    model, graph, uni = near_complete_problem()
    sharp = 9.0
    r64, r32 = _references(model, graph, uni, (2, 70, 9), sharp)
    gnn, out, res = _ours_step(model, graph, 2, 10, sharp, NEAR_SEED)
    assert _all_sliced()
    _check_step(gnn, out, res, r64, r32)
