"""pfsgnn.train.TrainLoop on the CPU: the loop's orchestration (schedule,
history, best-tracking, snapshot) with ``capture=False`` on the torch emulation
of the op set, against a literal host transcription of train.py:133-158 driven
by the oracle; and the C ABI of the new entry points (host-only calls).

The emulation backend has none of the three bookkeeping launches, so TrainLoop
takes their torch restatements (as Engine.loss_bnstat falls back for a backend
without loss_bn_part), and it reads a tensor sharpness / seed as host numbers.

Bar for the histories: the parity tests' (tests/test_gpu_parity.py) -- within
max(16 x |oracle32 - oracle64|, 6e-5 x scale, 1e-6) of the float64 oracle; the
emulation runs pfsgnn.GNN's float32 parameters.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from emu_backend import EmuBackend
from harness import make_problem
from noise_ref import uniform_numpy
from oracle.ref_gnn import Graph as OGraph
from oracle.ref_train import loss_function as oracle_loss

TOL_K, TOL_REL = 16.0, 6e-5
G, NF, NC, B = 2, 6, 4, 1
NEPOCHS, RUN, SHARPS, MIN_SHARP, SEED, LR = 6, 5, [0, 20], 5.0, 40, 1e-3
PCLASS, PFIBER, NFIELDS = 0.1, 0.1, 10


def _num(x):
    return float(x) if isinstance(x, torch.Tensor) else x


class TrainEmu(EmuBackend):
    """EmuBackend whose loss ops take the sharpness and the seed as tensors."""

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
    yield pfsgnn
    gnn_mod._LAYOUT_CACHE.clear()
    config.device, gnn_mod._BACKEND, gnn_mod._ParamMixin._check_device = saved


def host_loop(model, graph, dtype):
    """train.py:133-158, literally, on the oracle (softfloor's uniforms from the
    counter hash of the epoch's seed, as the product draws them)."""
    m = copy.deepcopy(model).to(dtype)
    m.train()
    g = OGraph(graph.edge_index, graph.x_s.to(dtype), graph.x_t.to(dtype), graph.x_e.to(dtype),
               graph.x_u.to(dtype), graph.s_batch, graph.t_batch)
    optimizer = torch.optim.Adam(m.parameters(), lr=LR)
    losses, objective, variances = np.zeros(NEPOCHS), np.zeros(NEPOCHS), np.zeros(NEPOCHS)
    completions = np.zeros((G * NC, NEPOCHS))
    best = dict(utility=0.0, loss=0.0, epoch=-1, fiber_time=np.zeros(G * NF),
                completion=np.zeros(G * NC), params=None)
    for epoch in range(0, RUN):
        m.zero_grad()
        out = m(g)
        sharp = SHARPS[0] + (SHARPS[1] - SHARPS[0]) * epoch / NEPOCHS
        uni = torch.as_tensor(uniform_numpy(SEED + epoch + 1, G * NF * NC), dtype=dtype)
        loss, diag = oracle_loss(m, out.x_e, g.x_t, G, NF, NC, pclass=PCLASS, pfiber=PFIBER,
                                 sharpness=sharp, uniform=uni)
        utility = float(torch.stack(diag["utils"]).sum())
        n_prime = torch.cat(diag["n_prime"])
        completions[:, epoch] = (n_prime / (g.x_t[:, 1] / NFIELDS)).numpy()
        loss.backward()
        optimizer.step()
        losses[epoch] = loss.item()
        objective[epoch] = utility
        variances[epoch] = float(torch.stack(diag["variance"]).sum())
        if utility > best["utility"] and sharp > MIN_SHARP:
            best.update(utility=utility, loss=loss.item(), epoch=epoch,
                        fiber_time=torch.cat(diag["fiber_time"]).numpy(),
                        completion=completions[:, epoch].copy(),
                        params={k: v.detach().clone() for k, v in m.named_parameters()})
    return dict(losses=losses, objective=objective, variances=variances, completions=completions,
                best=best)


def check(name, ours, r64, r32):
    ours, r64, r32 = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (ours, r64, r32))
    scale = np.abs(r64).max()
    bound = max(TOL_K * np.abs(r32 - r64).max(), TOL_REL * scale, 1e-6)
    err = np.abs(ours - r64).max()
    print(f"{name}: err {err:.3e} bound {bound:.3e} (scale {scale:.3e})")
    assert err <= bound, f"{name}: err {err:.3e} > bound {bound:.3e}"


@pytest.fixture(scope="module")
def runs(emu_pfsgnn):
    pfsgnn = emu_pfsgnn
    from pfsgnn.train import TrainLoop
    model, graph = make_problem(G, NF, NC, B=B, seed=4)
    gnn = pfsgnn.GNN(B=B, Fdim=10, T=12, F_s=1, F_t=2)
    gnn.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    gnn.train()
    data = pfsgnn.BipartiteData(graph.edge_index, graph.x_s.float(), graph.x_t.float(),
                                graph.x_e.float(), graph.x_u.float())
    opt = pfsgnn.FusedAdam(gnn.parameters(), lr=LR, capturable=True)
    loop = TrainLoop(gnn, opt, data, graph.x_t.float(), NEPOCHS, SHARPS, MIN_SHARP, PCLASS, PFIBER,
                     seed=SEED, capture=False)
    loop.run(RUN)
    return loop, gnn, host_loop(model, graph, torch.float64), host_loop(model, graph, torch.float32)


def test_history_matches_the_reference_loop(runs):
    loop, gnn, r64, r32 = runs
    h = loop.history()
    assert loop.epoch == RUN and h["losses"].shape == (RUN,)
    assert h["completions"].shape == (G * NC, RUN)
    for k in ("losses", "objective", "variances"):
        check(k, h[k], r64[k][:RUN], r32[k][:RUN])
    check("completions", h["completions"], r64["completions"][:, :RUN], r32["completions"][:, :RUN])
    assert loop.sharpness() == np.float32(SHARPS[0] + (SHARPS[1] - SHARPS[0]) * (RUN - 1) / NEPOCHS)
    assert int(loop._seed) == SEED + RUN


def test_best_selection_matches_the_reference_loop(runs):
    loop, gnn, r64, r32 = runs
    b, b64, b32 = loop.best(), r64["best"], r32["best"]
    # the case must select something, and not at the first qualifying epoch only by default
    assert b64["epoch"] >= 2 and b32["epoch"] == b64["epoch"]
    assert b["epoch"] == b64["epoch"]
    check("best utility", b["utility"], b64["utility"], b32["utility"])
    check("best loss", b["loss"], b64["loss"], b32["loss"])
    check("best fiber_time", b["fiber_time"], b64["fiber_time"], b32["fiber_time"])
    check("best completion", b["completion"], b64["completion"], b32["completion"])
    assert b["time"].shape == (G * NF * NC,)
    ck = loop.best_checkpoint()
    assert ck["epoch"] == b64["epoch"]
    for k, v in b64["params"].items():     # the weights after that epoch's optimizer.step()
        check("best " + k, ck["model_state"][k].numpy(), v.numpy(), b32["params"][k].numpy())
    # both optimizers load what the loop saves (train.py:131)
    import pfsgnn
    for ckpt in (ck, loop.checkpoint()):
        ps = [torch.nn.Parameter(p.detach().clone()) for p in gnn.parameters()]
        torch.optim.Adam(ps, lr=LR).load_state_dict(ckpt["optim_state"])
        pfsgnn.FusedAdam(ps, lr=LR, capturable=True).load_state_dict(ckpt["optim_state"])
    assert loop.checkpoint()["epoch"] == RUN - 1


def test_run_refuses_to_pass_nepochs(runs):
    loop = runs[0]
    with pytest.raises(ValueError, match="nepochs"):
        loop.run(NEPOCHS - RUN + 1)
    assert loop.epoch == RUN


def test_needs_a_capturable_fused_adam(emu_pfsgnn):
    from pfsgnn.train import TrainLoop
    pfsgnn = emu_pfsgnn
    model, graph = make_problem(1, 4, 3, B=1, seed=1)
    gnn = pfsgnn.GNN(B=1, Fdim=10, T=12, F_s=1, F_t=2)
    data = pfsgnn.BipartiteData(graph.edge_index, graph.x_s.float(), graph.x_t.float(),
                                graph.x_e.float(), graph.x_u.float())
    for opt in (pfsgnn.FusedAdam(gnn.parameters(), lr=LR), torch.optim.Adam(gnn.parameters(), lr=LR)):
        with pytest.raises(ValueError, match="capturable"):
            TrainLoop(gnn, opt, data, graph.x_t.float(), 4, SHARPS, MIN_SHARP, PCLASS, PFIBER)


# ---------------------------------------------------------------- C ABI (host-only)
@pytest.fixture(scope="module")
def lib():
    from pfsgnn import native
    return native.lib()


def test_abi_struct_sizes_and_version(lib):
    from pfsgnn import native
    assert lib.pfsgnn_version().decode() == native.ABI_VERSION == "pfsgnn 0.3 gfx950"
    assert lib.pfsgnn_loss_args_bytes() == ctypes.sizeof(native.LossArgs)
    assert native.LossArgs.bn_part.offset == ctypes.sizeof(native.LossArgs) - 8
    assert native.LossArgs.sl.offset == 16
    assert lib.pfsgnn_train_record_args_bytes() == ctypes.sizeof(native.TrainRecordArgs)
    assert native.TrainRecordArgs.best_epoch.offset == ctypes.sizeof(native.TrainRecordArgs) - 8
    assert ctypes.sizeof(native.CopyJob) == 24


def test_new_entry_points_refuse_bad_arguments_before_any_launch(lib):
    """Fake non-null pointers are never dereferenced: every refusal comes from a
    host-side check, names its entry point, and leaves no failure state behind."""
    from pfsgnn import native
    FAKE = 0x1000

    def loss_args(**over):
        a = native.LossArgs(G=1, NF=16, NC=2, F=10)
        for f, ty in a._fields_[5:]:
            if ty is ctypes.c_void_p and f not in ("pos_user", "bn_mu1", "bn_inv1", "bn_part"):
                setattr(a, f, FAKE)
        for f, v in over.items():
            setattr(a, f, v)
        return a

    def refused(fn, args, *words):
        rc = getattr(lib, fn)(*args)
        err = lib.pfsgnn_last_error().decode()
        assert rc != 0, (fn, words)
        assert err.startswith(fn + ":"), err
        for w in words:
            assert w in err, (err, w)

    sliced = native.Sliced(fib=FAKE, base=FAKE, len=FAKE, cls=FAKE, pco=FAKE, EP=32, E=20, maxdeg=2)
    slp = ctypes.pointer(sliced)
    max_nc = ctypes.c_int(0)
    assert lib.pfsgnn_sliced_max_nc(10, ctypes.byref(max_nc)) == 0 and max_nc.value > 0
    for fn in ("pfsgnn_loss_fwd", "pfsgnn_loss_bwd"):
        refused(fn, (None, None, 0, None), "null")
        refused(fn, (ctypes.byref(loss_args(pos_user=FAKE)), None, 0, None), "sl", "pos_user")
        refused(fn, (ctypes.byref(loss_args(sl=slp)), None, 0, None), "pos_user")
        refused(fn, (ctypes.byref(loss_args(bn_part=FAKE)), None, 0, None), "bn_mu1", "bn_part")
        refused(fn, (ctypes.byref(loss_args(sl=slp, pos_user=FAKE, bn_mu1=FAKE,
                                            bn_inv1=FAKE, bn_part=FAKE)), None, 0, None), "sl", "bn_part")
        # the dense and the sliced form of the op, each under the op's one name
        for form in (dict(), dict(sl=slp, pos_user=FAKE)):
            refused(fn, (ctypes.byref(loss_args(F=11, **form)), None, 0, None), "Fdim")
            refused(fn, (ctypes.byref(loss_args(y=None, **form)), None, 0, None), "null")
            refused(fn, (ctypes.byref(loss_args(**form)), None, 0, None), "workspace")
        refused(fn, (ctypes.byref(loss_args(sl=slp, pos_user=FAKE, NC=max_nc.value + 1)), None, 0,
                     None), "pfsgnn_sliced_max_nc")
    fin = [1, 16, 2] + [FAKE] * 4 + [0.1, 0.1, 42.0, 10.0, 2000.0, 1.0] + [FAKE] * 6 + [None]
    for sl in (None, slp):
        refused("pfsgnn_loss_finalize", [sl, 1, 1, 2] + fin[3:], "bad dims")
        refused("pfsgnn_loss_finalize", [sl] + fin[:3] + [None] + fin[4:], "null")
        refused("pfsgnn_loss_finalize", [sl] + fin[:-2] + [None, None], "null")
    refused("pfsgnn_softfloor_record", (None, FAKE, None), "null")
    refused("pfsgnn_softfloor_record", (FAKE, FAKE + 4, None), "aligned")
    refused("pfsgnn_train_advance", (FAKE, FAKE, 0.0, 20.0, 0, FAKE, FAKE, None), "nepochs")
    refused("pfsgnn_train_advance", (FAKE, None, 0.0, 20.0, 4, FAKE, FAKE, None), "null")
    refused("pfsgnn_train_record", (None, None), "null")
    refused("pfsgnn_train_record", (ctypes.byref(native.TrainRecordArgs(G=1, NC=2, nepochs=4)), None),
            "null")
    refused("pfsgnn_copy_if", (None, FAKE, 1, None, 0, 4, None), "null")
    refused("pfsgnn_copy_if", (FAKE, None, 0, None, 0, 4, None), "no jobs")
    five = (native.CopyJob * 5)()
    refused("pfsgnn_copy_if", (FAKE, FAKE, 1, five, 5, 4, None), "extra")
    info = (ctypes.c_int * 4)()
    assert lib.pfsgnn_edge_grid(1, 16, 2, info) == 0
