"""The captured training loop (pfsgnn.train.TrainLoop) and the device-resident
sharpness of the loss kernels on the HIP library.

Geometry: tests/test_gpu_graph.py's (G = 2, 130 fibers = a partial third
64-fiber block, 24 classes, B = 2, Fdim 10) unless a test says otherwise.
Tolerances: the loss parity bar of tests/test_gpu_parity.py (TOL_K, TOL_REL) and
of tests/test_gpu_sparse_loss.py for the sliced batch; everything else here is
bitwise.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from harness import make_problem  # noqa: E402
import test_gpu_parity as parity  # noqa: E402
import test_gpu_sparse_loss as sparse_loss  # noqa: E402

G, NF, NC, B = 2, 130, 24, 2
SHARPS_TENSOR = [0.0, 5e-4, 0.5, 8.0, 20.0]
SLICED_CASE = sparse_loss.CASES[1]


def _model(model, B=B):
    import pfsgnn
    gnn = pfsgnn.GNN(B=B, Fdim=10, T=12, F_s=1, F_t=2).cuda()
    gnn.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    gnn.train()
    return gnn


def _data(graph):
    import pfsgnn
    return pfsgnn.BipartiteData(graph.edge_index, graph.x_s.float(), graph.x_t.float(),
                                graph.x_e.float(), graph.x_u.float())


_PROBLEM = {}


def problem(shape=(G, NF, NC, B)):
    if shape not in _PROBLEM:
        _PROBLEM[shape] = make_problem(*shape[:3], B=shape[3], seed=3)
    return _PROBLEM[shape]


def make_loop(nepochs, sharps, min_sharp, capture, seed=77, start_epoch=0, lr=1e-3,
              shape=(G, NF, NC, B), state=None, prob=None):
    import pfsgnn
    from pfsgnn.train import TrainLoop
    model, graph = prob or problem(shape)
    gnn = _model(model, shape[3])
    opt = pfsgnn.FusedAdam(gnn.parameters(), lr=lr, capturable=True)
    if state is not None:
        gnn.load_state_dict(state["model_state"])
        opt.load_state_dict(state["optim_state"])
    loop = TrainLoop(gnn, opt, _data(graph), graph.x_t.float().cuda(), nepochs, sharps, min_sharp,
                     0.1, 0.1, seed=seed, start_epoch=start_epoch, capture=capture)
    return loop, gnn, opt


def loop_state(loop, gnn, opt):
    """Everything a run leaves behind, on the host."""
    torch.cuda.synchronize()
    out = {"param." + n: p.detach().cpu() for n, p in gnn.named_parameters()}
    out.update({"buffer." + n: b.detach().cpu() for n, b in gnn.named_buffers()})
    for i, p in enumerate(gnn.parameters()):
        for k, v in opt.state[p].items():
            out[f"adam.{i}.{k}"] = v.detach().cpu()
    out.update({"hist." + k: torch.as_tensor(v) for k, v in loop.history().items()})
    b = loop.best()
    out.update({"best." + k: torch.as_tensor(v) for k, v in b.items()})
    ck = loop.best_checkpoint()
    if ck is not None:
        out.update({"bestck." + k: v.cpu() for k, v in ck["model_state"].items()})
        for i, st in ck["optim_state"]["state"].items():
            out.update({f"bestck.adam.{i}.{k}": v.cpu() for k, v in st.items()})
    out["seed"], out["sharp"] = loop._seed.cpu(), loop._sharp.cpu()
    return out


def assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------- 1. tensor sharpness
@pytest.mark.parametrize("sharp", SHARPS_TENSOR)
def test_tensor_sharpness_matches_oracle(sharp):
    """loss_function(sharpness=<device tensor>): loss and every gradient against
    the fp64 oracle with the same noise (fails before the feature: a tensor
    sharpness was not accepted)."""
    import pfsgnn
    from pfsgnn.train import loss_function
    model, graph = problem()
    seed = 777 + NC
    value = float(np.float32(sharp))                 # what the kernels read
    m64, o64, l64 = parity.oracle_step(model, graph, G, NF, NC, seed, value, torch.float64)
    ref32 = [parity.oracle_step(model, graph, G, NF, NC, seed, value, torch.float32, reverse=rv)
             for rv in (False, True)]
    gnn = _model(model)
    gnn.zero_grad()
    out = gnn(_data(graph))
    st = torch.tensor(sharp, dtype=torch.float32, device="cuda")
    loss, _ = loss_function(out, graph.x_t.float().cuda(), pclass=0.1, pfiber=0.1, sharpness=st,
                            seed=seed)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    print(f"sharpness {sharp}: loss {loss.item():.6f} oracle64 {l64.item():.6f}")
    parity.check("loss", loss, l64, [r[2] for r in ref32])
    p64 = dict(m64.named_parameters())
    p32s = [dict(r[0].named_parameters()) for r in ref32]
    for name, p in gnn.named_parameters():
        assert torch.isfinite(p.grad).all(), name
        r64 = p64[name].grad if p64[name].grad is not None else torch.zeros_like(p64[name])
        r32 = [q[name].grad if q[name].grad is not None else torch.zeros_like(q[name]) for q in p32s]
        parity.check("grad " + name, p.grad, r64, r32)


@pytest.fixture
def sliced_layouts(monkeypatch):
    from pfsgnn import gnn
    monkeypatch.setenv("PFSGNN_SLICED", "1")
    gnn._LAYOUT_CACHE.clear()
    yield
    gnn._LAYOUT_CACHE.clear()


@pytest.mark.parametrize("sharp", SHARPS_TENSOR)
def test_tensor_sharpness_matches_oracle_sliced(sharp, sliced_layouts):
    """The same on one sliced general batch (tests/test_gpu_sparse_loss.py's helpers and bar)."""
    from noise_ref import uniform_numpy
    Gs, NFs, NCs, density, Bs, dup, _, ec, F, _ = SLICED_CASE
    model, graph, _ = sparse_loss.problem(SLICED_CASE)
    # (noise seed 2: with it no edge sits on the clamp's kink at any of the five
    # sharpness values, which _references asserts on the float64 oracle)
    seed = 2
    uni = torch.as_tensor(uniform_numpy(seed, graph.edge_index.shape[1]), dtype=torch.float64)
    value = float(np.float32(sharp))
    r64, r32 = sparse_loss._references(model, graph, uni, (Gs, NFs, NCs), value)
    st = torch.tensor(sharp, dtype=torch.float32, device="cuda")
    gnn, out, res = sparse_loss._ours_step(model, graph, Bs, F, st, seed)
    assert sparse_loss._all_sliced()
    sparse_loss._check_step(gnn, out, res, r64, r32)


def test_softfloor_record_values():
    """The device record: r = exp(-1/s) and atan(r / (1 - r)) in double rounded
    once; s = 0 and a tiny s give r = corr = 0 exactly, never NaN."""
    import math
    import pfsgnn
    be = pfsgnn.gnn.backend()
    for s in SHARPS_TENSOR + [1e-30, 3.3]:
        rec = be.softfloor_record(torch.tensor(s, dtype=torch.float32, device="cuda")).cpu().numpy()
        sv = float(np.float32(s))
        r = 0.0 if sv == 0 else math.exp(-1.0 / sv)
        want = np.array([np.float32(r), np.float32(math.atan(r / (1.0 - r))),
                         np.float32(2.0) * np.float32(math.pi),
                         np.float32(1.0) / np.float32(math.pi)], dtype=np.float32)
        assert np.isfinite(rec).all(), (s, rec)
        if s in (0.0, 5e-4, 1e-30):
            assert rec[0] == 0.0 and rec[1] == 0.0, (s, rec)
        # the device's exp / atan are within an ulp or two of libm's in double:
        # after the single rounding to float at most 1 float ulp apart
        assert np.all(np.abs(rec - want) <= np.spacing(np.abs(want))), (s, rec, want)
        assert rec[2] == want[2] and rec[3] == want[3]


# ---------------------------------------------------------------- 2. the float form
def test_float_form_is_unchanged(monkeypatch):
    """A Python-float sharpness: the BN and the non-BN arm of loss_bwd give the
    same gxe and decoder gradients bit for bit on the same inputs, and
    loss_function is bitwise reproducible with the BN and the non-BN backward."""
    import pfsgnn
    from pfsgnn import native
    from pfsgnn.engine import Dims
    from pfsgnn.train import loss_function
    be = pfsgnn.gnn.backend()
    d = Dims(G, NF, NC, 10)
    gen = torch.Generator().manual_seed(5)
    F, E, NT =10, G * NF * NC, G * NC
    y = torch.randn(F, E, generator=gen).cuda()
    Wd1, bd1 = (0.3 * torch.randn(F, F, generator=gen)).cuda(), (0.1 * torch.randn(F, generator=gen)).cuda()
    Wd2, bd2 = (0.3 * torch.randn(1, F, generator=gen)).cuda(), (0.1 * torch.randn(1, generator=gen)).cuda()
    ci = torch.stack([torch.randint(2, 13, (NT,), generator=gen).float(),
                      torch.randint(100, 2000, (NT,), generator=gen).float()]).cuda()
    mu1, inv1 = torch.randn(F, generator=gen).cuda(), (0.5 + torch.rand(F, generator=gen)).cuda()
    scale, sharp, nl, seed = 42.0 / NC, 8.0, 0.3, 77
    n_prime, fiber_time, tmean, tvar, tt = be.loss_fwd(d, y, None, None, Wd1, bd1, Wd2, bd2, ci,
                                                       scale, sharp, nl, seed, True)
    assert tt.shape == (E,) and all(torch.isfinite(t).all() for t in (n_prime, fiber_time, tmean, tvar, tt))
    _, _, _, Gn, Gf, Gv = be.loss_finalize(d, n_prime, fiber_time, tvar, ci, 0.1, 0.1, 42.0, 10,
                                           2000.0, 1.0)
    arms = []
    for bn in (None, (mu1, inv1)):
        gr = [be.zeros(F, F), be.zeros(F), be.zeros(1, F), be.zeros(1)]
        got = be.loss_bwd(d, y, None, None, Wd1, bd1, Wd2, bd2, ci, scale, sharp, nl, seed, Gn, Gf,
                          Gv, tmean, 1.0, *gr, **({"bn": bn} if bn else {}))
        arms.append(([got] if bn is None else list(got)) + gr)
    plain, fused = arms
    nparts = native.lib().pfsgnn_loss_bn_parts(G, NF, NC)
    assert fused[1].shape == (nparts, 2 * F) and torch.isfinite(fused[1]).all()
    assert plain[0].abs().max() > 0
    for a, b in zip(plain, [fused[0]] + fused[2:]):     # gxe, dWd1, dbd1, dWd2, dbd2
        assert torch.equal(a, b)
    # loss_function, twice per backward form
    model, graph = problem()
    for flag in ("1", "0"):
        monkeypatch.setenv("PFSGNN_LOSS_BN_SUMS", flag)
        vals = []
        for _ in range(2):
            gnn = _model(model)
            gnn.zero_grad()
            loss, _ = loss_function(gnn(_data(graph)), graph.x_t.float().cuda(), pclass=0.1,
                                    pfiber=0.1, sharpness=8.0, seed=5)
            loss.backward()
            vals.append((loss.detach().cpu(), torch.cat([p.grad.reshape(-1) for p in gnn.parameters()]).cpu()))
        assert torch.equal(vals[0][0], vals[1][0]) and torch.equal(vals[0][1], vals[1][1])


# ---------------------------------------------------------------- 3. schedule
@pytest.mark.parametrize("start", [0, 3])
@pytest.mark.parametrize("k", [1, 2, 7])
def test_schedule_after_k_replays(k, start):
    """After k epochs (eager warm-up, side-stream step, then replays) the device
    sharpness is numpy.float32 of train.py:137's expression, bit for bit, and
    the seed has advanced by k."""
    nepochs, sharps, seed = 12, [0.3, 19.7], 1000
    loop, gnn, opt = make_loop(nepochs, sharps, 5.0, True, seed=seed, start_epoch=start)
    loop.run(k)
    torch.cuda.synchronize()
    epoch = start + k - 1
    want = np.float32(sharps[0] + (sharps[1] - sharps[0]) * epoch / nepochs)
    got = loop._sharp.cpu().numpy()
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (got, want)
    assert int(loop._seed.item()) == seed + k
    assert int(loop._epoch.item()) == epoch and loop.epoch == start + k
    assert (k >= 2) == (loop._graph is not None)    # captured after the side-stream step


def test_advance_schedule_is_bitwise_numpys():
    """train_advance alone over the end of the reference's schedule (sharps =
    [0, 20], 40 000 epochs) and a float pair: every value bit for bit."""
    import pfsgnn
    be = pfsgnn.gnn.backend()
    for (s0, s1), nepochs, first in (((0, 20), 40000, 39930), ((0.3, 19.7), 977, 5)):
        epoch = torch.full((1,), first - 1, dtype=torch.int64, device="cuda")
        seed = torch.full((), 9, dtype=torch.int64, device="cuda")
        sharp, sf = be.empty(1), be.empty(4)
        got = []
        for _ in range(64):
            be.train_advance(epoch, seed, s0, s1, nepochs, sharp, sf)
            got.append(sharp.clone())
        got = torch.stack(got).cpu().numpy()
        want = np.array([np.float32(s0 + (s1 - s0) * e / nepochs) for e in range(first, first + 64)],
                        dtype=np.float32)
        assert got.tobytes() == want.tobytes()
        assert int(seed.item()) == 9 + 64 and int(epoch.item()) == first + 63
        assert torch.equal(sf, be.softfloor_record(sharp))


# ---------------------------------------------------------------- 4. replay == eager
def test_replay_equals_eager_bitwise():
    runs = []
    for capture in (True, False):
        loop, gnn, opt = make_loop(4, [0, 20], 7.0, capture)
        loop.run(4)
        runs.append(loop_state(loop, gnn, opt))
        assert (loop._graph is not None) == capture
    assert_same_state(*runs)
    assert runs[0]["best.epoch"].item() >= 2           # (sharp > 7 from epoch 2 on)
    assert any(k.startswith("bestck.") for k in runs[0])


def test_replays_survive_cache_eviction():
    """The capture bakes in the addresses of the batch's cached layout and
    canonical edge tensors; other batches of the process may evict them from
    gnn's caches, and the replays must not then read recycled memory."""
    from pfsgnn import gnn as gmod
    ref, _, _ = make_loop(6, [0, 20], 7.0, False)
    ref.run(6)
    loop, gnn, opt = make_loop(6, [0, 20], 7.0, True)
    loop.run(3)
    torch.cuda.synchronize()
    gmod._EDGE_CACHE.clear()
    gmod._LAYOUT_CACHE.clear()
    # what the allocator would hand a freed canonical x_e [F, E] (or the layout) to
    junk = [torch.full((10, G * NF * NC), float("nan"), device="cuda") for _ in range(8)]
    junk += [torch.full((n,), -1, dtype=torch.int32, device="cuda") for n in (3, G * NF * NC) * 4]
    loop.run(3)
    a, b = loop.history(), ref.history()
    for k in ("losses", "objective", "variances", "completions"):
        assert np.array_equal(a[k], b[k]), k
    del junk


def test_replay_equals_eager_bitwise_sliced(sliced_layouts):
    """TrainLoop on a sliced general batch."""
    Gs, NFs, NCs, density, Bs, dup, _, ec, F, seed = SLICED_CASE
    model, graph, uni = sparse_loss.problem(SLICED_CASE)
    runs = []
    for capture in (True, False):
        loop, gnn, opt = make_loop(4, [0, 20], 7.0, capture, shape=(Gs, NFs, NCs, Bs),
                                   prob=(model, graph))
        loop.run(4)
        assert sparse_loss._all_sliced()
        runs.append(loop_state(loop, gnn, opt))
    assert_same_state(*runs)
    assert np.isfinite(runs[0]["hist.losses"].numpy()).all()
    assert runs[0]["best.time"].numel() == graph.edge_index.shape[1]


# ---------------------------------------------------------------- 5. the replay anneals
def test_replay_really_anneals():
    """lr = 0: the weights stay, so losses[k] of the replayed loop must be the
    eager loss_function at that epoch's sharpness (as a tensor) and seed."""
    from pfsgnn.train import loss_function
    seed, nepochs, sharps = 500, 4, [0, 20]
    loop, gnn, opt = make_loop(nepochs, sharps, 7.0, True, seed=seed, lr=0.0)
    p0 = torch.cat([p.detach().reshape(-1) for p in gnn.parameters()]).clone()
    loop.run(4)
    h = loop.history()
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in gnn.parameters()]), p0)
    model, graph = problem()
    data, ci = _data(graph), graph.x_t.float().cuda()
    for k in range(4):
        st = torch.tensor(np.float32(sharps[0] + (sharps[1] - sharps[0]) * k / nepochs),
                          dtype=torch.float32, device="cuda")
        gnn.zero_grad()
        loss, util = loss_function(gnn(data), ci, pclass=0.1, pfiber=0.1, sharpness=st,
                                   seed=seed + k + 1)
        assert np.float32(loss.item()).tobytes() == np.float32(h["losses"][k]).tobytes(), k
        assert np.float32(util.item()).tobytes() == np.float32(h["objective"][k]).tobytes(), k
    assert h["losses"][0] != h["losses"][3]


# ---------------------------------------------------------------- 6. best tracking
def test_best_tracking_matches_host_loop():
    nepochs, sharps, min_sharp = 6, [0, 20], 7.0        # sharp = 0, 3.3, 6.7, 10, 13.3, 16.7
    eager, gnn_e, opt_e = make_loop(nepochs, sharps, min_sharp, False)
    best = dict(utility=np.float32(0.0), loss=np.float32(0.0), epoch=-1, params=None)
    rows = []
    for epoch in range(nepochs):                        # train.py:133-158 on the host
        eager.run(1)
        h = eager.history()
        sharp = sharps[0] + (sharps[1] - sharps[0]) * epoch / nepochs
        utility, loss = h["objective"][epoch], h["losses"][epoch]
        rows.append(sharp > min_sharp)
        if utility > best["utility"] and sharp > min_sharp:
            best.update(utility=utility, loss=loss, epoch=epoch,
                        completion=h["completions"][:, epoch].copy(),
                        params={n: p.detach().clone() for n, p in gnn_e.named_parameters()},
                        buffers={n: b.detach().clone() for n, b in gnn_e.named_buffers()},
                        adam=[{k: v.detach().clone() for k, v in opt_e.state[p].items()}
                              for p in gnn_e.parameters()],
                        time=eager.best()["time"], fiber_time=eager.best()["fiber_time"])
    assert any(rows) and not all(rows) and best["epoch"] >= 2
    loop, gnn, opt = make_loop(nepochs, sharps, min_sharp, True)
    loop.run(nepochs)
    b, ck = loop.best(), loop.best_checkpoint()
    assert b["epoch"] == best["epoch"] == ck["epoch"]
    assert np.float32(b["utility"]) == best["utility"] and np.float32(b["loss"]) == best["loss"]
    assert np.array_equal(b["completion"], best["completion"])
    assert np.array_equal(b["time"], best["time"]) and np.array_equal(b["fiber_time"], best["fiber_time"])
    assert b["time"].any() and b["fiber_time"].any()
    for n, p in best["params"].items():                 # the weights after that epoch's Adam step
        assert torch.equal(ck["model_state"][n], p), n
    for n, v in best["buffers"].items():
        assert torch.equal(ck["model_state"][n], v), n
    for i, st in enumerate(best["adam"]):
        for k, v in st.items():
            assert torch.equal(ck["optim_state"]["state"][i][k], v), (i, k)
    if best["epoch"] < nepochs - 1:                     # and not the final ones
        assert not all(torch.equal(ck["model_state"][n], p.detach()) for n, p in gnn.named_parameters())


def test_no_qualifying_epoch_leaves_the_best_state_untouched():
    loop, gnn, opt = make_loop(4, [0, 20], 100.0, True)
    loop.run(4)
    b = loop.best()
    assert b["epoch"] == -1 and b["utility"] == 0.0 and b["loss"] == 0.0
    assert not b["time"].any() and not b["fiber_time"].any() and not b["completion"].any()
    assert loop.best_checkpoint() is None
    assert not any(t.any().item() for t in loop._snap.values())
    assert np.isfinite(loop.history()["losses"]).all()


# ---------------------------------------------------------------- 7. reference shape
def test_reference_shape_runs_and_resumes():
    """train.py's workload (one 2000 x 12 graph, B = 3): 5 epochs, the
    checkpoint loads into both optimizers, and the epoch after a reload is the
    uninterrupted one bit for bit."""
    import pfsgnn
    shape, nepochs, seed = (1, 2000, 12, 3), 8, 31
    loop, gnn, opt = make_loop(nepochs, [0, 20], 5.0, True, seed=seed, shape=shape)
    loop.run(5)
    h = loop.history()
    for k in ("losses", "objective", "variances", "completions"):
        assert np.isfinite(h[k]).all() and h[k].shape[-1] == 5, k
    ck = loop.checkpoint()
    assert ck["epoch"] == 4
    ps = [torch.nn.Parameter(p.detach().clone()) for p in gnn.parameters()]
    torch.optim.Adam(ps, lr=1e-3).load_state_dict(ck["optim_state"])
    pfsgnn.FusedAdam(ps, lr=1e-3, capturable=True).load_state_dict(ck["optim_state"])
    loop.run(1)
    resumed, gnn_r, opt_r = make_loop(nepochs, [0, 20], 5.0, True, seed=seed + 5,
                                      start_epoch=ck["epoch"] + 1, shape=shape, state=ck)
    resumed.run(1)
    torch.cuda.synchronize()
    a, b = loop.history(), resumed.history()
    for k in ("losses", "objective", "variances"):
        assert np.float32(a[k][5]).tobytes() == np.float32(b[k][5]).tobytes(), k
    assert np.array_equal(a["completions"][:, 5], b["completions"][:, 5])
    for (n, p), (_, q) in zip(gnn.named_parameters(), gnn_r.named_parameters()):
        assert torch.equal(p, q), n
    for p, q in zip(gnn.parameters(), gnn_r.parameters()):
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(opt.state[p][k], opt_r.state[q][k]), k


def test_refuses_a_non_capturable_optimizer():
    import pfsgnn
    from pfsgnn.train import TrainLoop
    model, graph = problem()
    gnn = _model(model)
    with pytest.raises(ValueError, match="capturable"):
        TrainLoop(gnn, pfsgnn.FusedAdam(gnn.parameters(), lr=1e-3), _data(graph),
                  graph.x_t.float().cuda(), 4, [0, 20], 5.0, 0.1, 0.1)


# ---------------------------------------------------------------- 8. independent references
def test_best_state_and_completions_match_loss_function():
    """lr = 0 keeps the weights, so every epoch's diagnostics can be recomputed
    by loss_function(finaloutput=True) at that epoch's sharpness and seed: the
    completion rows train_record writes, and the time / fiber_time /
    completion copy_if keeps for the best epoch, against values that neither
    kernel produced."""
    from pfsgnn.train import loss_function
    seed, nepochs, sharps, min_sharp = 900, 6, [0, 20], 7.0
    loop, gnn, opt = make_loop(nepochs, sharps, min_sharp, True, seed=seed, lr=0.0)
    loop.run(nepochs)
    h, b = loop.history(), loop.best()
    model, graph = problem()
    data, ci = _data(graph), graph.x_t.float().cuda()
    best = dict(utility=np.float32(0.0), epoch=-1)
    for k in range(nepochs):
        sharp = sharps[0] + (sharps[1] - sharps[0]) * k / nepochs
        st = torch.tensor(np.float32(sharp), dtype=torch.float32, device="cuda")
        gnn.zero_grad()
        loss, util, comp, n_prime, fibers, time, var = loss_function(
            gnn(data), ci, pclass=0.1, pfiber=0.1, sharpness=st, finaloutput=True, seed=seed + k + 1)
        # the row is n_prime / (N_i / NFIELDS) with both divisions IEEE, as
        # k_loss_finalize forms the completeness whose minimum is the utility;
        # loss_function's `comp` divides N_i by the scalar the way torch does (a
        # multiplication by fl(1 / NFIELDS)), which can differ in the last bit
        want = (n_prime.detach().cpu().numpy().astype(np.float32)
                / (ci[:, 1].cpu().numpy().astype(np.float32) / np.float32(10)))
        comp_k = h["completions"][:, k]
        assert np.array_equal(comp_k, want), k
        assert np.all(np.abs(comp_k - comp) <= 2 * np.spacing(np.abs(comp))), k
        umin = comp_k.reshape(G, NC).min(1)
        assert np.float32(umin[0] + umin[1]).tobytes() == np.float32(h["objective"][k]).tobytes(), k
        comp = comp_k
        assert np.float32(var.item()).tobytes() == np.float32(h["variances"][k]).tobytes(), k
        util = np.float32(util.item())
        if util > best["utility"] and sharp > min_sharp:          # train.py:146-152
            best = dict(utility=util, epoch=k, loss=np.float32(loss.item()), completion=comp,
                        time=time.detach().cpu().numpy(), fiber_time=fibers)
    assert best["epoch"] >= 2 and b["epoch"] == best["epoch"]
    assert np.float32(b["utility"]) == best["utility"] and np.float32(b["loss"]) == best["loss"]
    assert np.array_equal(b["time"], best["time"])
    assert np.array_equal(b["fiber_time"], best["fiber_time"])
    assert np.array_equal(b["completion"], best["completion"])


def test_history_sums_graphs_in_serial_order():
    """G = 3: train_record adds the per-graph loss / utils / variance in the
    order g = 0, 1, 2 in fp32.  loss_function returns torch.sum over [G], whose
    order is torch's; two fp32 sums of G terms differ by at most
    (G - 1) * 2^-24 * sum |x_g| * 2, which is the bound asserted against it."""
    from pfsgnn.train import _loss_apply
    shape, seed, nepochs, sharps = (3, 40, 12, 2), 60, 4, [0, 20]
    loop, gnn, opt = make_loop(nepochs, sharps, 7.0, True, seed=seed, lr=0.0, shape=shape)
    loop.run(nepochs)
    h = loop.history()
    model, graph = problem(shape)
    data, ci = _data(graph), graph.x_t.float().cuda()
    for k in range(nepochs):
        st = torch.tensor(np.float32(sharps[0] + (sharps[1] - sharps[0]) * k / nepochs),
                          dtype=torch.float32, device="cuda")
        gnn.zero_grad()
        outs = _loss_apply(gnn(data), ci, 0.1, 0.1, st, False, None, seed + k + 1, 0.3)[2]
        rows = dict(losses=(outs[-1], outs[0]), objective=(outs[1], outs[1].sum()),
                    variances=(outs[4], outs[4].sum()))
        for name, (per_graph, torch_sum) in rows.items():
            x = per_graph.detach().cpu().numpy().astype(np.float32)
            serial = np.float32(x[0])
            for g in range(1, 3):
                serial = np.float32(serial + x[g])
            assert np.float32(h[name][k]).tobytes() == serial.tobytes(), (name, k)
            bound = 2 * 2 * 2.0 ** -24 * np.abs(x).sum()
            assert abs(float(torch_sum.detach()) - float(serial)) <= bound, (name, k)


# ---------------------------------------------------------------- 9. several captured models
class _BareStep:
    """tests/test_gpu_graph.py's captured step (fixed sharpness, no bookkeeping),
    holding everything its graph reads and writes."""

    def __init__(self):
        import test_gpu_graph as tg
        self.tg, self.args = tg, tg._setup()
        tg._step(*self.args)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            tg._step(*self.args)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.static = tg._step(*self.args)

    def run(self):
        self.graph.replay()
        return self.static.detach().clone()


def test_interleaved_captured_models_do_not_interfere():
    """A bare captured step and two TrainLoops alive in one process, replayed in
    turn: each must give, bit for bit, what it gives alone."""
    n = 6

    def alone_loop(seed):
        loop, gnn, opt = make_loop(8, [0, 20], 7.0, True, seed=seed)
        loop.run(n)
        return loop_state(loop, gnn, opt)

    bare = _BareStep()
    bare_alone = torch.stack([bare.run() for _ in range(n)]).cpu()
    del bare
    a_alone, b_alone = alone_loop(77), alone_loop(300)

    bare = _BareStep()
    la, ga, oa = make_loop(8, [0, 20], 7.0, True, seed=77)
    lb, gb, ob = make_loop(8, [0, 20], 7.0, True, seed=300)
    got = []
    for _ in range(n):
        got.append(bare.run())
        la.run(1)
        lb.run(1)
    assert torch.equal(torch.stack(got).cpu(), bare_alone)
    assert_same_state(loop_state(la, ga, oa), a_alone)
    assert_same_state(loop_state(lb, gb, ob), b_alone)
    assert la._graph is not None and lb._graph is not None
