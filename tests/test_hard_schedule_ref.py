"""The hard (integer) schedule on the CPU: the edge_index-indexed reference
(tests/hard_schedule_ref.py) against the positional form of train.py:40, :50;
``pfsgnn.train.hard_schedule``'s torch restatement and ``TrainLoop(track_hard=
True)`` on the torch emulation of the op set; and pfsgnn_schedule's argument
checks (host-only calls).
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from emu_backend import EmuBackend
from hard_schedule_ref import check_visits, hard_schedule_ref
from harness import make_problem
from oracle.ref_scatter import scatter

TOTAL_TIME, NFIELDS = 42.0, 10
G, NF, NC, B = 2, 6, 4, 1
NEPOCHS, RUN, SHARPS, MIN_SHARP, SEED, LR = 8, 7, [0, 20], 5.0, 40, 3e-2
PCLASS, PFIBER = 0.1, 0.1


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("g,nf,nc,tscale", [(1, 7, 5, 1.0), (2, 9, 4, 0.25), (3, 5, 1, 1.0)])
def test_edge_index_form_equals_the_positional_form(g, nf, nc, tscale):
    """train.py:40, :50 on a complete fiber-major batch, graph by graph."""
    model, graph = make_problem(g, nf, nc, B=1, seed=2)
    ci = graph.x_t.clone()
    ci[:, 0] *= tscale
    x_e = 2.0 + 8.0 * torch.rand(g * nf * nc, 10, dtype=torch.float64,
                                 generator=torch.Generator().manual_seed(3))
    ref = hard_schedule_ref(model, x_e, graph.edge_index, ci, g, nf, nc)
    assert ref["visits"].max() >= 1
    with torch.no_grad():
        for k in range(g):
            es = slice(k * nf * nc, (k + 1) * nf * nc)
            T_i = ci[k * nc:(k + 1) * nc, 0]
            time = model.edge_prediction(x_e[es], scale=TOTAL_TIME / nc)
            visited = time.squeeze(-1) / T_i.unsqueeze(0).expand(nf, -1).reshape(-1)  # train.py:40
            tgt = graph.edge_index[1, es] - k * nc
            n = scatter(torch.floor(visited), tgt, nc, reduce="sum")              # train.py:50
            assert torch.equal(n.long(), ref["n"][k * nc:(k + 1) * nc])
            assert torch.equal(torch.floor(visited).long(), ref["visits"][es])
            comp = n / (ci[k * nc:(k + 1) * nc, 1] / NFIELDS)
            assert torch.equal(comp.min(), ref["utility"][k])


def test_reference_rounds_half_to_even():
    v = torch.tensor([0.5, 1.5, 2.5, 3.5], dtype=torch.float64)
    assert torch.round(v).tolist() == np.round(v.numpy()).tolist() == [0.0, 2.0, 2.0, 4.0]


# ---------------------------------------------------------------- the emulation
def _num(x):
    return float(x) if isinstance(x, torch.Tensor) else x


class TrainEmu(EmuBackend):
    """EmuBackend whose loss ops take the sharpness and the seed as tensors; it
    has no ``schedule``, so ``hard_schedule`` takes its torch restatement."""

    def loss_fwd(self, d, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, sharpness, noiselevel, seed,
                 want_time=False):
        return super().loss_fwd(d, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, _num(sharpness),
                                noiselevel, seed, want_time)

    def loss_bwd(self, d, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, sharpness, noiselevel, seed,
                 *args, **kw):
        return super().loss_bwd(d, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, _num(sharpness),
                                noiselevel, seed, *args, **kw)

    def noise_uniform(self, seed, E):
        return super().noise_uniform(int(seed), E)


@pytest.fixture(scope="module")
def emu_pfsgnn():
    import pfsgnn
    from pfsgnn import config, gnn as gnn_mod
    saved = (config.device, gnn_mod._BACKEND, gnn_mod._ParamMixin._check_device)
    config.device = torch.device("cpu")
    gnn_mod._BACKEND = TrainEmu(torch.float32)
    gnn_mod._ParamMixin._check_device = lambda self: None
    gnn_mod._LAYOUT_CACHE.clear()
    assert not hasattr(gnn_mod._BACKEND, "schedule")
    yield pfsgnn
    gnn_mod._LAYOUT_CACHE.clear()
    config.device, gnn_mod._BACKEND, gnn_mod._ParamMixin._check_device = saved


def _product(pfsgnn, g, nf, nc, seed, tscale=1.0, train=True):
    model, graph = make_problem(g, nf, nc, B=B, seed=seed)
    gnn = pfsgnn.GNN(B=B, Fdim=10, T=12, F_s=1, F_t=2)
    gnn.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    gnn.train(train)
    data = pfsgnn.BipartiteData(graph.edge_index, graph.x_s.float(), graph.x_t.float(),
                                graph.x_e.float(), graph.x_u.float())
    ci = graph.x_t.float().clone()
    ci[:, 0] *= tscale
    return model, graph, gnn, data, ci


@pytest.mark.parametrize("rounding", ["floor", "round"])
def test_fallback_equals_the_reference(emu_pfsgnn, rounding):
    pfsgnn = emu_pfsgnn
    from pfsgnn.train import hard_schedule
    g, nf, nc = 2, 12, 5
    model, graph, gnn, data, ci = _product(pfsgnn, g, nf, nc, seed=5, tscale=0.25)
    out = gnn(data)
    hs = hard_schedule(out, ci, rounding)
    assert isinstance(hs, pfsgnn.HardSchedule)
    assert not any(t.requires_grad for t in hs)
    assert hs.visits.dtype == hs.n.dtype == hs.over.dtype == torch.int32
    # the reference on the emulation's own edge state: only the decoder differs
    x_e = out.x_e.detach()
    r64 = hard_schedule_ref(model, x_e.double(), graph.edge_index, ci.double(), g, nf, nc, rounding)
    r32 = hard_schedule_ref(copy.deepcopy(model).float(), x_e, graph.edge_index, ci, g, nf, nc,
                            rounding)
    check_visits("emu " + rounding, hs.visits, r64, r32, rounding)
    # the rest follows from the returned visits exactly
    src, tgt = graph.edge_index
    assert torch.equal(hs.n.long(), scatter(hs.visits.long(), tgt, g * nc, reduce="sum"))
    ft = scatter(hs.visits.double() * ci[tgt, 0].double(), src, g * nf, reduce="sum")
    assert torch.allclose(hs.fiber_time.double(), ft, rtol=nc * 2.0 ** -24, atol=0)
    assert torch.equal(hs.completeness, hs.n.float() / (ci[:, 1] / NFIELDS))
    assert torch.equal(hs.utility, hs.completeness.view(g, nc).min(dim=1).values)
    assert torch.equal(hs.over.long(), (hs.fiber_time.view(g, nf) > TOTAL_TIME).sum(dim=1))
    assert torch.equal(hs.worst, hs.fiber_time.view(g, nf).max(dim=1).values)


def test_fallback_rounds_half_to_even(emu_pfsgnn):
    """decoder_e made constant (last layer: weight 0, bias 30 > softplus'
    threshold) and NC = 3, so time = 30 * 42 / 3 = 420 exactly; T = 840, 280,
    168 gives v = 0.5, 1.5, 2.5 exactly."""
    pfsgnn = emu_pfsgnn
    from pfsgnn.train import hard_schedule
    g, nf, nc = 1, 4, 3
    model, graph, gnn, data, ci = _product(pfsgnn, g, nf, nc, seed=1)
    ci[:, 0] = torch.tensor([840.0, 280.0, 168.0])
    with torch.no_grad():
        gnn.decoder_e[2].weight.zero_()
        gnn.decoder_e[2].bias.fill_(30.0)
    out = gnn(data)
    cls = graph.edge_index[1]
    assert torch.equal(hard_schedule(out, ci, "round").visits.long(), torch.tensor([0, 2, 2])[cls])
    assert torch.equal(hard_schedule(out, ci, "floor").visits.long(), torch.tensor([0, 1, 2])[cls])
    with pytest.raises(ValueError, match="rounding"):
        hard_schedule(out, ci, "ceil")


def test_refusals(emu_pfsgnn):
    pfsgnn = emu_pfsgnn
    from pfsgnn.train import hard_schedule
    model, graph, gnn, data, ci = _product(pfsgnn, 1, 4, 3, seed=1)
    with pytest.raises(NotImplementedError, match="GNN.forward"):
        hard_schedule(data, ci)
    out = gnn(data)
    other = pfsgnn.GNN(B=B, Fdim=10, T=12, F_s=1, F_t=2)
    with pytest.raises(NotImplementedError, match="different GNN"):
        hard_schedule(out, ci, gnn=other)
    hard_schedule(out, ci, gnn=gnn)
    out.x_e = out.x_e * 2
    with pytest.raises(NotImplementedError, match="x_e"):
        hard_schedule(out, ci)
    # a general batch on the composed path
    out = gnn(data)
    lay = out._pf[2]
    saved = lay.sp
    lay.sp = type("Sp", (), {"sl": None})()
    try:
        with pytest.raises(NotImplementedError, match="composed path"):
            hard_schedule(out, ci)
    finally:
        lay.sp = saved


# ---------------------------------------------------------------- the emulated loop
def _loop(pfsgnn, track_hard):
    from pfsgnn.train import TrainLoop
    model, graph, gnn, data, ci = _product(pfsgnn, G, NF, NC, seed=4, tscale=0.25)
    opt = pfsgnn.FusedAdam(gnn.parameters(), lr=LR, capturable=True)
    loop = TrainLoop(gnn, opt, data, ci, NEPOCHS, SHARPS, MIN_SHARP, PCLASS, PFIBER, seed=SEED,
                     capture=False, track_hard=track_hard)
    return loop.run(RUN), gnn


def _host_loop(pfsgnn):
    """The same training, epoch by epoch through the public functions, with
    ``hard_schedule`` called on every epoch's forward."""
    from pfsgnn.train import hard_schedule, loss_function
    model, graph, gnn, data, ci = _product(pfsgnn, G, NF, NC, seed=4, tscale=0.25)
    opt = pfsgnn.FusedAdam(gnn.parameters(), lr=LR, capturable=True)
    rows = []
    for epoch in range(RUN):
        sharp = float(np.float32(SHARPS[0] + (SHARPS[1] - SHARPS[0]) * epoch / NEPOCHS))
        gnn.zero_grad()
        out = gnn(data)
        loss, util = loss_function(out, ci, PCLASS, PFIBER, sharp, seed=SEED + epoch + 1)
        hs = hard_schedule(out, ci)
        hu, ho = hs.utility[0], hs.over[0]
        for k in range(1, G):
            hu, ho = hu + hs.utility[k], ho + hs.over[k]
        rows.append(dict(loss=loss.item(), hard=hu.item(), over=int(ho), hs=hs))
        loss.backward()
        opt.step()
    return rows


@pytest.fixture(scope="module")
def loops(emu_pfsgnn):
    return _loop(emu_pfsgnn, True), _loop(emu_pfsgnn, False), _host_loop(emu_pfsgnn)


def test_emulated_loop_tracks_the_hard_objective(loops):
    (loop, _), _, rows = loops
    h = loop.history()
    assert h["hard_objective"].shape == h["hard_overtime"].shape == (RUN,)
    assert h["hard_overtime"].dtype == np.int32
    assert [r["loss"] for r in rows] == h["losses"].tolist()   # the host loop is the same training
    assert [np.float32(r["hard"]) for r in rows] == h["hard_objective"].tolist()
    assert [r["over"] for r in rows] == h["hard_overtime"].tolist()
    assert max(r["hard"] for r in rows) > 0 and len({r["hard"] for r in rows}) > 1
    best, best_e = np.float32(0.0), -1
    for e, r in enumerate(rows):
        if np.float32(r["hard"]) > best:
            best, best_e = np.float32(r["hard"]), e
    hb = loop.hard_best()
    assert hb["epoch"] == best_e and hb["utility"] == best
    hs = rows[best_e]["hs"]
    assert np.array_equal(hb["visits"], hs.visits.numpy()) and hb["visits"].dtype == np.int32
    assert np.array_equal(hb["fiber_time"], hs.fiber_time.numpy())
    assert np.array_equal(hb["completion"], hs.completeness.numpy())


def test_tracking_leaves_the_soft_run_bitwise(loops):
    (hard, gnn_h), (soft, gnn_s), _ = loops
    hh, hs = hard.history(), soft.history()
    assert "hard_objective" not in hs and "hard_overtime" not in hs
    for k in ("losses", "objective", "variances", "completions"):
        assert np.array_equal(hh[k], hs[k]), k
    for (n, p), (_, q) in zip(gnn_h.named_parameters(), gnn_s.named_parameters()):
        assert torch.equal(p, q), n
    bh, bs = hard.best(), soft.best()
    assert bh["epoch"] == bs["epoch"] >= 0
    for k in bs:
        assert np.array_equal(bh[k], bs[k]), k
    with pytest.raises(ValueError, match="track_hard"):
        soft.hard_best()


# ---------------------------------------------------------------- C ABI (host-only)
@pytest.fixture(scope="module")
def lib():
    from pfsgnn import native
    return native.lib()


def test_abi_struct_sizes_and_version(lib):
    from pfsgnn import native
    assert lib.pfsgnn_version().decode() == native.ABI_VERSION == "pfsgnn 0.3 gfx950"
    assert lib.pfsgnn_schedule_args_bytes() == ctypes.sizeof(native.ScheduleArgs)
    assert native.ScheduleArgs.worst.offset == ctypes.sizeof(native.ScheduleArgs) - 8
    assert [f for f, _ in native.ScheduleArgs._fields_[:5]] == ["G", "NF", "NC", "F", "sl"]
    assert native.ScheduleArgs.sl.offset == 16
    assert lib.pfsgnn_train_record_hard_args_bytes() == ctypes.sizeof(native.TrainRecordHardArgs)


def test_schedule_refuses_bad_arguments_before_any_launch(lib):
    """Fake non-null pointers are never dereferenced: every refusal comes from a
    host-side check and names pfsgnn_schedule."""
    from pfsgnn import native
    FAKE = 0x1000

    def args(**over):
        a = native.ScheduleArgs(G=1, NF=16, NC=2, F=10, mode=1)
        for f, ty in a._fields_[5:]:
            if ty is ctypes.c_void_p and f not in ("pos_user", "perm"):
                setattr(a, f, FAKE)
        for f, v in over.items():
            setattr(a, f, v)
        return a

    def refused(a, *words, ws=(None, 0)):
        rc = lib.pfsgnn_schedule(None if a is None else ctypes.byref(a), ws[0], ws[1], None)
        err = lib.pfsgnn_last_error().decode()
        assert rc != 0, words
        assert err.startswith("pfsgnn_schedule:"), err
        for w in words:
            assert w in err, (err, w)

    sliced = native.Sliced(fib=FAKE, base=FAKE, len=FAKE, cls=FAKE, pco=FAKE, EP=32, E=20, maxdeg=2)
    slp = ctypes.pointer(sliced)
    max_nc = ctypes.c_int(0)
    assert lib.pfsgnn_sliced_max_nc(10, ctypes.byref(max_nc)) == 0 and max_nc.value > 0
    refused(None, "null")
    refused(args(sl=slp), "sl", "pos_user")
    refused(args(pos_user=FAKE), "sl", "pos_user")
    refused(args(sl=slp, pos_user=FAKE, perm=FAKE), "sl", "perm")
    refused(args(mode=0), "mode 0", "perm")
    refused(args(mode=3), "mode")
    for form in (dict(), dict(sl=slp, pos_user=FAKE)):
        refused(args(rounding=2, **form), "rounding")
        refused(args(rounding=-1, **form), "rounding")
        refused(args(F=11, **form), "Fdim")
        for out in ("visits", "n_hard", "fiber_time", "completeness", "utility", "over", "worst"):
            refused(args(**{out: None}, **form), "null output")
        refused(args(y=None, **form), "null input")
        refused(args(**form), "workspace")
        refused(args(**form), "workspace", ws=(FAKE, 64))
    refused(args(sl=slp, pos_user=FAKE, NC=max_nc.value + 1), "pfsgnn_sliced_max_nc")
    rec = native.TrainRecordHardArgs(G=1, nepochs=4)
    assert lib.pfsgnn_train_record_hard(None, None) != 0
    assert lib.pfsgnn_last_error().decode().startswith("pfsgnn_train_record_hard:")
    assert lib.pfsgnn_train_record_hard(ctypes.byref(rec), None) != 0
    assert "null" in lib.pfsgnn_last_error().decode()
