"""Drop-in for the reference ``src/train.py`` objective and training loop.

``loss_function`` (train.py:29-80) runs fused over the edges in
``libpfsgnn.so``: decoder_e (gnn.py:307) + softplus + ``softfloor``
(train.py:21) + the per-class / per-fiber scatters + penalties, with the
backward as one more fused pass that hands the last message-passing block
its edge gradient.  The loss reads the GNN's lazy final edge state directly
(``graph._pf``), so the normalised edge features are never re-read.

softfloor's noise: the reference draws ``torch.rand_like`` (train.py:22);
here the uniforms come from a counter-based hash of (seed, edge id) computed
in-kernel (``pfsgnn_common.h: pf_uniform``), with the per-call seed drawn from
torch's global CPU generator -- so ``torch.manual_seed`` governs it as it
governs the reference, a step is reproducible, and no RNG state lives on the
device.
"""
import collections
import math
import os
import sys

import numpy as np
import torch

from . import config
from . import gnn as _gnn
from .engine import Dims
from .gnn import GNN, BipartiteData, backend

_SEED_SPACE = (1 << 62)


def draw_seed():
    return int(torch.randint(0, _SEED_SPACE, (1,)).item())


def softfloor(x, sharpness=20, noiselevel=0.3):
    """train.py:21-27 on an arbitrary tensor (utility; the training objective
    uses the fused in-kernel version).  Elementwise torch on the device."""
    noise = noiselevel * (torch.rand_like(x) - 0.5)
    x = x + noise
    sharpness = x.new_tensor(sharpness)
    pi = x.new_tensor(np.pi)
    r = torch.where(sharpness == 0, torch.tensor(0.0, device=x.device), torch.exp(-1 / sharpness))
    return x + 1 / pi * (torch.arctan(r * torch.sin(2 * pi * x) / (1 - r * torch.cos(2 * pi * x)))
                         - torch.arctan(r / (torch.ones_like(r) - r)))


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, token, anchor, model, d, ectx, xe3, ci, sharpness, seed, pclass, pfiber,
                want_time, noiselevel):
        ctx.set_materialize_grads(False)   # the diagnostics get no gradient: no zero fills
        eng = model._engine()
        P = model._flat_params()
        loss, diag, lctx = eng.loss_forward(P, d, xe3, ci, sharpness, seed, pclass=pclass,
                                            pfiber=pfiber, total_time=float(config.TOTAL_TIME),
                                            nfields=float(config.NFIELDS), wutils=config.wutils,
                                            wvar=config.wvar, want_time=want_time,
                                            noiselevel=noiselevel)
        ctx.pf = (model, d, ectx, lctx)
        outs = (diag["utils"], diag["n_prime"], diag["fiber_time"], diag["variance"])
        ctx.mark_non_differentiable(*outs)
        if diag["time"] is not None:
            ctx.mark_non_differentiable(diag["time"])
        ctx.mark_non_differentiable(diag["loss"])
        # (the per-graph losses last: TrainLoop's history sums them on the device)
        return ((loss,) + outs + ((diag["time"],) if diag["time"] is not None else ())
                + (diag["loss"],))

    @staticmethod
    def backward(ctx, g_loss, *unused):
        model, d, ectx, lctx = ctx.pf
        if g_loss is None:
            return (None,) * 13
        eng = model._engine()
        P, Gr = model._flat_params(), model._recording_grads()
        prev = ectx.get("g_xe_canonical")
        # the final edge BatchNorm's backward sums come out of the same pass when
        # this loss is the edge state's only consumer so far
        bns = eng.loss_bnstat(ectx) if prev is None else None
        out = eng.loss_backward(P, Gr, lctx, gscale=g_loss, bnstat=bns)
        gc, part = out if bns is not None else (out, None)
        model._mark_live(Gr.used)
        # hand the canonical [F, E] gradient straight to the GNN's backward
        # (gnn._GNNFn.backward); the edge-state token gets none
        if prev is None:
            ectx["g_xe_canonical"] = gc
            if part is not None:
                ectx["g_xe_bn_part"] = part
        else:
            ectx["g_xe_canonical"] = prev + gc
            ectx.pop("g_xe_bn_part", None)
        return (None,) * 13


def _class_info_cm(class_info, d):
    ci = class_info.to(device=config.device, dtype=torch.float32)
    if ci.dim() != 2 or ci.size(0) != d.NT or ci.size(1) < 2:
        raise ValueError(f"class_info must be [G*NC, >=2] = [{d.NT}, >=2]; got {tuple(ci.shape)}")
    return ci[:, :2].t().contiguous()


def loss_function(graph, class_info, pclass=0.1, pfiber=1.0, sharpness=0.5, finaloutput=False,
                  *, gnn=None, seed=None, noiselevel=0.3):
    """train.py:29-80.  ``graph`` is the output of ``GNN.forward``; ``class_info``
    is [NC, 2] (T_i, N_i) per class -- [G*NC, 2] for a batch of G graphs, whose
    loss is the sum of the per-graph losses.  The reference reads the model
    from a global ``gnn`` (train.py:42); here it comes with the graph (or
    ``gnn=``).  On complete graphs the edge order must be the fiber-major layout
    train.py builds (train.py:94), on which train.py:40 and :67 rely.

    General (non-complete) batches -- ragged degrees, missing or repeated
    (fiber, class) pairs, empty fibers or classes -- are accepted when they run
    on the fused sliced kernels (``Layout.SLOTS``: at most
    ``pfsgnn_sliced_max_nc`` classes per graph, an fp32 edge-state path,
    PFSGNN_SLICED not 0).  The objective is then indexed by ``edge_index``
    instead of by position: ``T_e = class_info[tgt_e, 0]``, ``n'_c`` sums
    galaxies over ``tgt_e = c``, ``fiber_time_f`` sums time over ``src_e = f``
    (0 for a fiber without edges, which still pays the under-time penalty), a
    class without edges has completeness 0, and ``variance`` is the sum over
    classes of the unbiased variance of time over the class's own ``deg(c)``
    edges.  One divergence from the reference: a class with ``deg(c) < 2``
    contributes 0 to the variance (and gets no gradient from it) where
    ``torch.var`` would give NaN.  softfloor's uniform of edge ``e`` is the
    counter hash of ``(seed, e)`` with ``e`` the caller's edge position, as on
    complete graphs.  ``class_info`` stays [G*NC, >=2]; with ``finaloutput``
    ``comp`` is per class, ``fibers`` per fiber and ``time`` [E] in the
    caller's edge order.  On a complete fiber-major batch this form equals the
    reference's.  ``seed`` (softfloor's
    noise): None draws one from torch's CPU generator; an int; or a device
    int64 tensor read in-kernel (a captured step then draws fresh noise per
    replay when the tensor is advanced on the device).  ``noiselevel`` is
    softfloor's (train.py:21, fixed at 0.3 by the reference's call).
    ``sharpness``: a Python number, or a 0-d float32 device tensor read
    in-kernel (the reference anneals it every epoch, train.py:137: a captured
    step then follows the tensor); softfloor's coefficients are made from it on
    the device, once per call, in double rounded once to float.  A float32
    device tensor of 4 elements is taken as those coefficients already made
    (``TrainLoop`` fills them in the launch that advances the schedule)."""
    d, ci, outs = _loss_apply(graph, class_info, pclass, pfiber, sharpness, finaloutput, gnn, seed,
                              noiselevel)
    loss, utils_g, n_prime, fiber_time, variance = outs[:5]
    if not finaloutput:
        return loss, utils_g.sum() if d.G > 1 else utils_g[0]
    time = outs[5]
    Ni = ci[1] / config.NFIELDS
    comp = (n_prime / Ni).detach().cpu().numpy()
    fibers = fiber_time.detach().cpu().numpy()
    utils = utils_g.sum() if d.G > 1 else utils_g[0]
    var = variance.sum() if d.G > 1 else variance[0]
    return loss, utils, comp, n_prime, fibers, time, var


def _loss_apply(graph, class_info, pclass, pfiber, sharpness, want_time, gnn, seed, noiselevel):
    """loss_function's checks and the fused op: -> (dims, class_info [2, NT],
    (loss, utils [G], n_prime, fiber_time, variance [G], time [E] if
    ``want_time``, loss [G])), every one a device tensor."""
    pf = graph.__dict__.get("_pf")
    if pf is None or graph.__dict__.get("_pf_replaced"):
        raise NotImplementedError("loss_function needs the BipartiteData returned by "
                                  "pfsgnn.GNN.forward (the fused loss reads its edge state)")
    model, d, lay, token, xe3, ectx = pf
    if token is None:
        # eval-mode forward: the loss is inference-only (no backward through it)
        if torch.is_grad_enabled():
            raise NotImplementedError("loss_function on an eval-mode GNN.forward runs under "
                                      "torch.no_grad() only (train.py:108 trains in train mode)")
        token = xe3[0].new_empty(())
    if gnn is not None and gnn is not model:
        raise ValueError("graph was produced by a different GNN than `gnn`")
    if lay.sp is not None:
        # a general batch: the edge_index-indexed objective of the fused sliced kernels
        if lay.sp.sl is None:
            raise NotImplementedError(
                "loss_function on a general (non-complete) batch runs on the fused sliced "
                "kernels (pfsgnn_loss_fwd / _bwd with sl) only, and this batch is on the composed path: "
                "unset PFSGNN_SLICED=0, keep the classes per graph within "
                "pfsgnn_sliced_max_nc (at most 128) and use an fp32 edge-state path "
                "(not \"bf16\" / \"bf16y\"); or materialise out.x_e and write the loss in torch")
    elif not lay.fiber_major:
        raise NotImplementedError("train.py's objective indexes edges by position "
                                  "(train.py:40, :67): it needs the fiber-major edge order")
    ci = _class_info_cm(class_info, d)
    if seed is None:
        seed = draw_seed()
    elif not isinstance(seed, torch.Tensor):
        seed = int(seed)
    if isinstance(sharpness, torch.Tensor):
        if (sharpness.device.type != config.device.type or not sharpness.is_floating_point()
                or sharpness.numel() not in (1, 4)):
            raise ValueError("a tensor sharpness must be one float on the device (or softfloor's "
                             f"4 coefficients); got {tuple(sharpness.shape)} {sharpness.dtype} on "
                             f"{sharpness.device}")
        sharpness = sharpness.detach()
    else:
        sharpness = float(sharpness)
    outs = _LossFn.apply(token, model.encoder_s[0].weight, model, d, ectx, xe3, ci, sharpness,
                         seed, float(pclass), float(pfiber), bool(want_time), float(noiselevel))
    return d, ci, outs


# ---------------------------------------------------------------- hard schedule
HardSchedule = collections.namedtuple(
    "HardSchedule", "visits n fiber_time completeness utility over worst")

BudgetSchedule = collections.namedtuple(
    "BudgetSchedule", HardSchedule._fields + ("quot", "phase"))

_ROUNDINGS = {"floor": 0, "round": 1}


def hard_schedule(graph, class_info, rounding="floor", *, gnn=None, time=None):
    """The integer evaluation of an allocation: whole visits per edge and what
    follows from them -- train.py:50's commented ``scatter(torch.floor(visited),
    tgt)``, the "hard counts & diagnostics" of train.py:74, and, with
    ``rounding="round"``, the rounding to whole visits of train.py:257
    (``np.round``: half to even).  No noise, no sharpness, no seed.

    ``graph`` is the output of ``GNN.forward`` (train or eval mode, grad on or
    off); ``class_info`` as for ``loss_function``.  Every edge is indexed by
    ``edge_index``: ``visits_e = floor(time_e / T[tgt_e])`` with ``time_e =
    softplus(decoder_e(x_e)) * TOTAL_TIME / NC``, ``n_c`` sums visits over
    ``tgt_e = c`` (int32), ``fiber_time_f`` sums ``visits_e * T[tgt_e]`` over
    ``src_e = f``, ``completeness_c = n_c / (N_c / NFIELDS)``, ``utility`` [G]
    its minimum per graph, ``over`` [G] the fibers above TOTAL_TIME and
    ``worst`` [G] the largest fiber time.  So every complete edge order is
    accepted (there is no positional noise counter), and sliced general
    batches; ``visits`` [E] is in the caller's edge order.  The fused op
    (pfsgnn_schedule) reads the lazy final edge state: ``out.x_e`` is not
    materialised.  Returns a ``HardSchedule`` of device tensors without grad.

    ``rounding="budget"`` is the rounding a user can execute: floor every edge,
    then give each fiber's remaining time to the edges with the largest
    fractional part while they still fit TOTAL_TIME (largest remainder; a fiber
    whose floor alone is over loses visits from the smallest fractional parts
    first) -- the definition is pfsgnn_schedule_budget's in include/pfsgnn.h.
    It returns a ``BudgetSchedule``: ``HardSchedule``'s fields, ``quot`` [E]
    (the fp32 quotient that was rounded) and ``phase`` [NS] (int32; bit 0 the
    fiber took the down phase, bit 1 it got a bump, bit 2 it refused a
    candidate).  ``time`` [E] (budget rounding only; the caller's edge order,
    e.g. ``TrainLoop.best()["time"]``) is rounded in place of the graph's own
    edge times."""
    return _hard_schedule(graph, class_info, rounding, gnn, None, time)


def _budget_round_host(q, inert, src, tgt, T, total_time, NS):
    """pfsgnn_schedule_budget's steps 2-3 on the host, for backends without the
    op: each fiber's edges sorted once by key, one pass per phase.  ``q`` fp32
    [E], ``T`` fp32 [NT] -> (visits int32 [E], phase int32 [NS])."""
    q = q.cpu().numpy().astype(np.float32)
    inert = inert.cpu().numpy()
    src, tgt = src.cpu().numpy(), tgt.cpu().numpy()
    Td = T.cpu().numpy().astype(np.float64)[tgt]
    base = np.floor(q)
    frac = q - base
    vis = base.astype(np.int64)
    pos = np.arange(q.size)
    asc = np.lexsort((pos, tgt, frac))
    desc = np.lexsort((pos, tgt, -frac))
    asc = asc[np.argsort(src[asc], kind="stable")]
    desc = desc[np.argsort(src[desc], kind="stable")]
    lo = np.searchsorted(src[asc], np.arange(NS + 1))
    phase = np.zeros(NS, np.int32)
    total = float(np.float32(total_time))
    for f in range(NS):
        ea, ed = asc[lo[f]:lo[f + 1]], desc[lo[f]:lo[f + 1]]
        ft = 0.0
        for e in ea:
            if vis[e]:                       # (an inert edge: 0 visits, whatever its T)
                ft += float(vis[e]) * Td[e]
        cand = ~inert[ea]
        cand = dict(zip(ea.tolist(), cand.tolist()))
        if ft > total:
            phase[f] |= 1
            for e in ea:
                if ft <= total:
                    break
                if vis[e] == 0:
                    continue
                k = float(np.ceil((ft - total) / Td[e]))
                if k >= 1 and ft - (k - 1) * Td[e] <= total:
                    k -= 1
                elif ft - k * Td[e] > total:
                    k += 1
                r = int(min(float(vis[e]), k))
                ft -= r * Td[e]
                vis[e] -= r
                cand[e] = False
        for e in ed:
            if not cand[e]:
                continue
            if ft + Td[e] <= total:
                ft += Td[e]
                vis[e] += 1
                phase[f] |= 2
            else:
                phase[f] |= 4
    return torch.from_numpy(vis.astype(np.int32)), torch.from_numpy(phase)


def _hard_schedule(graph, class_info, rounding, gnn, out, time=None):
    budget = rounding == "budget"
    if not budget and rounding not in _ROUNDINGS:
        raise ValueError(f"rounding must be 'floor', 'round' or 'budget'; got {rounding!r}")
    if time is not None and not budget:
        raise ValueError("time= is budget rounding only (rounding='budget')")
    pf = graph.__dict__.get("_pf")
    if pf is None or graph.__dict__.get("_pf_replaced"):
        raise NotImplementedError("hard_schedule needs the BipartiteData returned by "
                                  "pfsgnn.GNN.forward with its x_e untouched (the fused op reads "
                                  "its edge state)")
    model, d, lay, token, xe3, ectx = pf
    if gnn is not None and gnn is not model:
        raise NotImplementedError("hard_schedule: graph was produced by a different GNN than "
                                  "`gnn` (the decoder of the GNN that made it is the one read)")
    if lay.sp is not None and lay.sp.sl is None:
        raise NotImplementedError(
            "hard_schedule on a general (non-complete) batch runs on the fused sliced "
            "kernel (pfsgnn_schedule with sl) only, and this batch is on the composed path: "
            "unset PFSGNN_SLICED=0, keep the classes per graph within "
            "pfsgnn_sliced_max_nc (at most 128) and use an fp32 edge-state path "
            "(not \"bf16\" / \"bf16y\"); or materialise out.x_e and count in torch")
    ci = _class_info_cm(class_info, d)
    be = backend()
    scale = float(config.TOTAL_TIME) / d.NC
    if time is not None:
        time = torch.as_tensor(time, dtype=be.dtype, device=ci.device).reshape(-1).contiguous()
        if time.numel() != d.E:
            raise ValueError(f"time has {time.numel()} entries for {d.E} edges")
    op, Result, extra = (("schedule_budget", BudgetSchedule, dict(time_in=time)) if budget else
                         ("schedule", HardSchedule, dict(rounding=_ROUNDINGS[rounding])))
    if hasattr(be, op):
        P = model._flat_params()
        y, sc, sh = (None, None, None) if time is not None else xe3
        res = getattr(be, op)(d, y, sc, sh, P["decoder_e.0.weight"], P["decoder_e.0.bias"],
                              P["decoder_e.2.weight"], P["decoder_e.2.bias"], ci, scale,
                              float(config.TOTAL_TIME), float(config.NFIELDS), mode=lay.mode,
                              perm=lay.perm, out=out, **extra)
        return Result(*res)
    # a backend without the op (a CPU emulation of the op set): torch restatement
    with torch.no_grad():
        src, tgt = graph.edge_index[0], graph.edge_index[1]
        if time is None:
            time = model.edge_prediction(graph.x_e.detach(), scale=scale).reshape(-1)
        T = ci[0][tgt]
        v = time / T
        extra = ()
        if budget:
            inert = torch.isnan(v) | ~(T > 0) | ~torch.isfinite(T)
            quot = torch.where(inert, torch.zeros_like(v), v.clamp(0.0, 2.0 ** 24))
            visits, phase = _budget_round_host(quot, inert, src, tgt, ci[0], config.TOTAL_TIME,
                                               d.NS)
            visits, phase = visits.to(v.device), phase.to(v.device)
            Tz = torch.where(inert, torch.zeros_like(T), T)
            extra = (quot, phase)
        else:
            visits = (torch.floor(v) if rounding == "floor" else torch.round(v)).to(torch.int32)
            Tz = T
        n = torch.zeros(d.NT, dtype=torch.int32, device=v.device).index_add_(0, tgt, visits)
        ft = torch.zeros(d.NS, dtype=v.dtype, device=v.device).index_add_(
            0, src, visits.to(v.dtype) * Tz)
        comp = n.to(v.dtype) / (ci[1] / config.NFIELDS)
        res = (visits, n, ft, comp, comp.view(d.G, d.NC).min(dim=1).values,
               (ft.view(d.G, d.NF) > config.TOTAL_TIME).sum(dim=1).to(torch.int32),
               ft.view(d.G, d.NF).max(dim=1).values) + extra
        if out is not None:
            for o, r in zip(out, res):
                o.copy_(r)
            res = out
    return (BudgetSchedule if budget else HardSchedule)(*res)


# ---------------------------------------------------------------- observing plan
ObservingPlan = collections.namedtuple(
    "ObservingPlan", "visits start used idle n completeness utility over worst cut seg_ptr "
                     "seg_edge seg_start")


def _plan_geometry(graph, F=None):
    """(Dims, Layout) of an input batch or of a ``GNN.forward`` output: only
    ``edge_index`` and the node counts matter, through the cached layout."""
    pf = graph.__dict__.get("_pf")
    if pf is not None:
        return pf[1], pf[2]
    F = int(graph.x_e.size(1)) if F is None else int(F)
    return _gnn.geometry(graph.x_s, graph.x_t, graph.x_u, graph.edge_index, F)


def observing_plan(graph, class_info, visits, *, cap=True, segments=True, _F=None):
    """From an integer schedule to the plan an observer runs (the definition is
    pfsgnn_schedule_plan's in include/pfsgnn.h): visits capped per class by the
    galaxies it has per field (train.py:41's ``N_i``, which train.py:57-58 only
    penalises), each fiber's classes laid end to end (train.py:256-261's
    ``cumsum`` / ``left``) and every single exposure at ``left + m * class_req``
    (train.py:283-284).

    ``graph`` is the input batch or the output of ``GNN.forward`` -- only
    ``edge_index`` and the node counts are used; complete batches in any edge
    order and every general batch (the composed path included).  ``visits`` is
    any int tensor or array of E entries in the caller's edge order, e.g.
    ``hard_schedule(...).visits`` or ``TrainLoop.hard_best()["visits"]``.
    ``cap=True`` trims a class whose visits exceed ``floor(N_c / NFIELDS)`` to
    that number, max-min fair, ties to the lower (fiber, edge position).

    Returns an ``ObservingPlan`` of device tensors: ``visits`` [E] int32 and
    ``start`` [E] (the time at which the fiber turns to the edge's class) in the
    caller's edge order; ``used``, ``idle`` [NS] (``TOTAL_TIME - used``: negative
    for a fiber that is over); ``n`` [NT] int32, ``completeness`` [NT],
    ``utility``, ``over``, ``worst`` [G] as ``hard_schedule``'s; ``cut`` [NT]
    int64, the visits the cap removed; ``seg_ptr`` [NS + 1] int64, and the
    target list ``seg_edge`` (int32, the caller's edge) / ``seg_start`` of
    ``seg_ptr[-1]`` entries: fiber f's exposures are ``seg_ptr[f] :
    seg_ptr[f + 1]``, in the order it takes them.  With ``segments=True`` the
    wrapper runs the op once to count, reads ``seg_ptr[-1]`` -- the ONE host
    synchronisation -- allocates, and runs it again.  With ``segments=False``
    ``seg_edge`` and ``seg_start`` are None and nothing synchronises (the call
    can be captured)."""
    d, lay = _plan_geometry(graph, _F)
    ci = _class_info_cm(class_info, d)
    vis = torch.as_tensor(visits)
    if vis.is_floating_point() or vis.dtype == torch.bool or vis.is_complex():
        raise ValueError(f"visits must be an integer tensor or array; got {vis.dtype}")
    if vis.numel() != d.E:
        raise ValueError(f"visits has {vis.numel()} entries for {d.E} edges")
    if vis.dtype != torch.int32:
        vis = vis.clamp(-(2 ** 31), 2 ** 31 - 1).to(torch.int32)
    vis = vis.to(ci.device).reshape(-1).contiguous()
    be = backend()
    total, nfields = float(config.TOTAL_TIME), float(config.NFIELDS)
    if hasattr(be, "schedule_plan"):
        kw = dict(sp=lay.sp) if lay.sp is not None else dict(mode=lay.mode, perm=lay.perm)
        out = be.schedule_plan(d, ci, vis, total, nfields, cap=cap, **kw)
        seg_edge = seg_start = None
        if segments:
            count = int(out[-1][-1])                # the one host synchronisation
            seg_edge = torch.empty(count, dtype=torch.int32, device=ci.device)
            seg_start = torch.empty(count, dtype=torch.float32, device=ci.device)
            if count:
                be.schedule_plan(d, ci, vis, total, nfields, cap=cap, seg_edge=seg_edge,
                                 seg_start=seg_start, out=out, **kw)
        return ObservingPlan(*out, seg_edge, seg_start)
    # a backend without the op (a CPU emulation of the op set): host restatement
    res = _observing_plan_host(vis.cpu().numpy(), graph.edge_index.cpu().numpy(),
                               ci.cpu().numpy(), total, nfields, d.G, d.NF, d.NC, cap, segments)
    return ObservingPlan(*(None if r is None else torch.from_numpy(r).to(ci.device) for r in res))


def _observing_plan_host(visits, ei, ci, total_time, nfields, G, NF, NC, cap, segments):
    """pfsgnn_schedule_plan on the host, for backends without the op: sorts and
    segment sums in numpy, a Python loop only over the trimmed classes and the
    fibers.  ``ci`` fp32 [2, NT] -> ObservingPlan's fields as numpy arrays."""
    NS, NT = G * NF, G * NC
    src, tgt = ei[0].astype(np.int64), ei[1].astype(np.int64)
    E = src.size
    pos = np.arange(E)
    T, N = ci[0].astype(np.float32), ci[1].astype(np.float32)
    Te = T[tgt]
    live = (Te > 0) & np.isfinite(Te)
    w = np.where(live, np.clip(visits.astype(np.int64), 0, 1 << 24), 0)
    with np.errstate(all="ignore"):
        q = N / np.float32(nfields)
    S = np.zeros(NT, np.int64)
    np.add.at(S, tgt, w)
    cut = np.zeros(NT, np.int64)
    if cap:
        bad = np.isnan(q) | (q < 0)
        nocap = ~bad & (q >= np.float32(2.0 ** 31))
        capc = np.where(bad | nocap, 0, np.floor(np.where(bad | nocap, 0, q))).astype(np.int64)
        byclass = np.lexsort((pos, src, tgt))
        cptr = np.searchsorted(tgt[byclass], np.arange(NT + 1))
        for c in np.nonzero(~nocap & (S > capc))[0]:
            e = byclass[cptr[c]:cptr[c + 1]]          # ascending (src, position)
            wc = w[e]
            ws = np.sort(wc)
            pre = np.concatenate([[0], np.cumsum(ws)])
            # f(L) = sum min(w, L) = pre[k] + L (n - k), k = #{w <= L}
            lo, hi = 0, int(ws[-1])
            while hi - lo > 1:
                mid = (lo + hi) // 2
                k = np.searchsorted(ws, mid, side="right")
                if pre[k] + mid * (ws.size - k) <= capc[c]:
                    lo = mid
                else:
                    hi = mid
            k = np.searchsorted(ws, lo, side="right")
            rem = int(capc[c] - (pre[k] + lo * (ws.size - k)))
            above = np.nonzero(wc > lo)[0]
            wc = np.minimum(wc, lo)
            wc[above[:rem]] += 1
            w[e] = wc
            cut[c] = S[c] - capc[c]
            S[c] = capc[c]
    order = np.lexsort((pos, tgt, src))               # the plan order, fiber by fiber
    fptr = np.searchsorted(src[order], np.arange(NS + 1))
    wo = w[order]
    To = Te[order].astype(np.float64)
    dur = np.where(wo > 0, wo * np.where(wo > 0, To, 0.0), 0.0)
    start_o = np.zeros(E)
    tot = np.zeros(NS)
    for f in range(NS):
        a, b = fptr[f], fptr[f + 1]
        if b > a:
            cs = np.cumsum(dur[a:b])
            start_o[a + 1:b] = cs[:-1]
            tot[f] = cs[-1]
    start = np.empty(E, np.float32)
    start[order] = start_o.astype(np.float32)
    total = float(np.float32(total_time))
    used, idle = tot.astype(np.float32), (total - tot).astype(np.float32)
    cnt = np.zeros(NS, np.int64)
    np.add.at(cnt, src, w)
    seg_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    seg_edge = seg_start = None
    if segments:
        seg_edge = np.repeat(order, wo).astype(np.int32)
        first = np.cumsum(wo) - wo
        m = np.arange(int(wo.sum())) - np.repeat(first, wo)
        seg_start = (np.repeat(start_o, wo) + m * np.repeat(To, wo)).astype(np.float32)
    n = S.astype(np.int32)
    with np.errstate(all="ignore"):
        comp = n.astype(np.float32) / q
    return (w.astype(np.int32), start, used, idle, n, comp, comp.reshape(G, NC).min(axis=1),
            (tot.reshape(G, NF) > total).sum(axis=1).astype(np.int32),
            used.reshape(G, NF).max(axis=1), cut, seg_ptr, seg_edge, seg_start)


# ---------------------------------------------------------------- training
def complete_graph(class_info, nfibers, fdim, lo=2.0, hi=10.0):
    """train.py:88-104: fiber counter x_s, class_info x_t, fiber-major complete
    edges, x_e ~ U[lo, hi), u = 0."""
    class_info = torch.as_tensor(class_info, dtype=torch.float, device=config.device)
    nclasses = class_info.shape[0]
    x_s = torch.arange(nfibers, dtype=torch.float, device=config.device).reshape(-1, 1)
    # torch.cartesian_prod's fiber-major order, built on the device
    edge_index = backend().build_complete(1, nfibers, nclasses, order=0)
    x_e = lo + (hi - lo) * torch.rand(size=(nfibers * nclasses, fdim)).to(config.device)
    x_u = torch.zeros(1, fdim).to(config.device)
    return BipartiteData(edge_index=edge_index, x_s=x_s, x_t=class_info, x_e=x_e, x_u=x_u)


class TrainLoop:
    """train.py:133-165 with nothing of an epoch on the host: the annealed
    sharpness (train.py:137), the history rows (train.py:143-145), the
    best-tracking (train.py:146-152) and the checkpoint of the best state
    (train.py:154-158) are device values and small launches around the forward,
    loss, backward and Adam, so the whole epoch is one HIP-graph replay.

    Launch order of an epoch: ``train_advance`` (epoch += 1, seed += 1, the
    sharpness and softfloor's coefficients) | zero_grad, GNN forward, loss
    forward + finalize | ``train_record`` (history rows, improved?) | backward |
    Adam | ``copy_if`` (improved: parameters, Adam state, BatchNorm buffers,
    time, fiber_time, completion -> the best snapshot).  As in the reference the
    best time / fiber_time / completion are those of the forward before the
    update and the checkpointed weights those after ``optimizer.step()``.

    ``run(n)`` does n epochs: the first eagerly (layout caches, workspace, Adam
    state), the second on a side stream, then it captures the step and replays
    it; ``capture=False`` issues the same launches eagerly.  The host only
    counts epochs.  ``history()``, ``best()``, ``checkpoint()`` and
    ``best_checkpoint()`` read the device state (one sync each, at call time).

    ``track_hard=True`` also evaluates the integer objective every epoch
    (``hard_schedule`` with floor, pfsgnn_schedule into preallocated buffers)
    right after ``train_record``: ``train_record_hard`` sums the graphs' hard
    utilities and over-time fibers into the ``hard_objective`` /
    ``hard_overtime`` history and tracks the best hard utility under strict
    ``>`` from 0 (train.py:117; no ``min_sharp`` condition: the count does not
    depend on the sharpness), and a second ``copy_if`` after Adam keeps that
    epoch's visits, fiber_time and completion (``hard_best()``).  No parameter
    snapshot is kept for it: the checkpoint criterion stays the soft one.  With
    the default False the step issues exactly the launches listed above.
    ``track_hard="budget"`` tracks the best *executable* schedule instead: the
    same rows and best state from ``hard_schedule(..., "budget")``
    (pfsgnn_schedule_budget: every fiber within TOTAL_TIME, so ``hard_overtime``
    stays 0); ``True`` and ``"floor"`` are the floor path, launch for launch.

    One divergence from the reference: it rewrites the checkpoint file on every
    improvement; here the best state stays on the device until asked for.
    ``seed``: softfloor's noise seed before the first epoch (epoch e draws with
    seed + e - start_epoch + 1); None draws one from torch's CPU generator."""

    def __init__(self, gnn, optimizer, graph, class_info, nepochs, sharps, min_sharp, pclass,
                 pfiber, seed=None, start_epoch=0, capture=True, record_completions=True,
                 track_hard=False):
        from .optim import FusedAdam
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError(
                "TrainLoop is single-process: a process group of "
                f"{dist.get_world_size()} ranks is active (collectives inside the capture "
                "and per-rank utilities are not supported)")
        if not isinstance(optimizer, FusedAdam) or not all(
                g.get("capturable", False) for g in optimizer.param_groups):
            raise ValueError("TrainLoop needs pfsgnn.FusedAdam(capturable=True): the step count "
                             "must live on the device")
        nepochs, start_epoch = int(nepochs), int(start_epoch)
        if nepochs <= 0 or not 0 <= start_epoch <= nepochs:
            raise ValueError(f"need nepochs > 0 and 0 <= start_epoch <= nepochs; got {nepochs}, "
                             f"{start_epoch}")
        self.gnn, self.optimizer, self.graph = gnn, optimizer, graph
        self.nepochs, self.start_epoch, self.epoch = nepochs, start_epoch, start_epoch
        self.sharps = (sharps[0], sharps[1])
        self.min_sharp, self.pclass, self.pfiber = float(min_sharp), float(pclass), float(pfiber)
        self.capture = bool(capture)
        be = self._be = backend()
        dev, fdt = config.device, be.dtype
        self.class_info = class_info.to(device=dev)
        NT, NS = self.class_info.shape[0], graph.x_s.shape[0]
        E, G = graph.edge_index.shape[1], graph.x_u.shape[0]
        if NT % G:
            raise ValueError(f"class_info has {NT} rows for {G} graphs")

        def buf(*shape, dtype=fdt, fill=0):
            return torch.full(shape, fill, dtype=dtype, device=dev)

        # the schedule (the epoch counter holds the epoch last run)
        self._epoch = buf(1, dtype=torch.int64, fill=start_epoch - 1)
        self._seed = buf(dtype=torch.int64, fill=draw_seed() if seed is None else int(seed))
        self._sharp, self._sf = buf(), buf(4)
        # the history (train.py:114-122) and the best state (train.py:117-121)
        self._losses, self._objective, self._variances = buf(nepochs), buf(nepochs), buf(nepochs)
        self._completions = buf(NT, nepochs) if record_completions else None
        self._comp, self._improved = buf(NT), buf(1, dtype=torch.int32)
        self._best_utility, self._best_loss = buf(1), buf(1)
        self._best_epoch = buf(1, dtype=torch.int64, fill=-1)
        self._best_time, self._best_fiber_time, self._best_completion = buf(E), buf(NS), buf(NT)
        self._jobs = self._snap = None
        self._graph, self._warm = None, 0
        # the integer objective (hard_schedule's outputs, its history and best state)
        if track_hard not in (False, True, "floor", "budget"):
            raise ValueError(f"track_hard must be False, True, 'floor' or 'budget'; got "
                             f"{track_hard!r}")
        self.track_hard = bool(track_hard)
        self._hard_rounding = "budget" if track_hard == "budget" else "floor"
        if self.track_hard:
            i32 = torch.int32
            self._hard = HardSchedule(buf(E, dtype=i32), buf(NT, dtype=i32), buf(NS), buf(NT),
                                      buf(G), buf(G, dtype=i32), buf(G))
            if self._hard_rounding == "budget":
                self._hard = BudgetSchedule(*self._hard, buf(E), buf(NS, dtype=i32))
            self._hard_objective, self._hard_overtime = buf(nepochs), buf(nepochs, dtype=i32)
            self._improved_hard, self._best_hard_utility = buf(1, dtype=i32), buf(1)
            self._best_hard_epoch = buf(1, dtype=torch.int64, fill=-1)
            self._best_hard = (buf(E, dtype=i32), buf(NS), buf(NT))
            self._hard_jobs = None

    # ------------------------------------------------------------ the three ops
    # (the backend's launches; torch restatements when it has none, for a CPU
    # emulation of the op set)
    def _advance(self):
        be = self._be
        if hasattr(be, "train_advance"):
            be.train_advance(self._epoch, self._seed, self.sharps[0], self.sharps[1], self.nepochs,
                             self._sharp, self._sf)
            return self._sf
        self._epoch += 1
        self._seed += 1
        e = int(self._epoch)
        self._sharp.fill_(self.sharps[0] + (self.sharps[1] - self.sharps[0]) * e / self.nepochs)
        return self._sharp

    def _record(self, d, ci, loss_g, utils_g, variance_g, n_prime):
        be = self._be
        if hasattr(be, "train_record"):
            be.train_record(d, self.nepochs, self._epoch, self._sharp, loss_g, utils_g, variance_g,
                            n_prime, ci, float(config.NFIELDS), self.min_sharp, self._losses,
                            self._objective, self._variances, self._completions, self._comp,
                            self._improved, self._best_utility, self._best_loss, self._best_epoch)
            return
        e = int(self._epoch)
        loss_g, utils_g, variance_g, n_prime = (t.detach() for t in (loss_g, utils_g, variance_g,
                                                                     n_prime))
        loss, util, var = loss_g[0], utils_g[0], variance_g[0]
        for g in range(1, d.G):
            loss, util, var = loss + loss_g[g], util + utils_g[g], var + variance_g[g]
        self._comp.copy_(n_prime / (ci[1] / config.NFIELDS))
        if 0 <= e < self.nepochs:
            self._losses[e], self._objective[e], self._variances[e] = loss, util, var
            if self._completions is not None:
                self._completions[:, e] = self._comp
        improved = bool(util > self._best_utility[0]) and bool(self._sharp > self.min_sharp)
        self._improved.fill_(int(improved))
        if improved:
            self._best_utility[0], self._best_loss[0], self._best_epoch[0] = util, loss, e

    def _copy_if(self, time, fiber_time):
        be = self._be
        extra = [(time, self._best_time), (fiber_time, self._best_fiber_time)]
        if self._jobs is None:
            self._build_snapshot()
        if hasattr(be, "copy_if"):
            be.copy_if(self._improved, self._jobs, extra)
        elif int(self._improved):
            for s, t in self._jobs + extra:
                t.copy_(s.detach())

    def _record_hard(self, out):
        """The epoch's integer objective (floor, or the budgeted rounding) into
        the preallocated buffers, its history rows and best-tracking."""
        be = self._be
        hs = _hard_schedule(out, self.class_info, self._hard_rounding, None, self._hard)
        if hasattr(be, "train_record_hard"):
            d = out.__dict__["_pf"][1]
            be.train_record_hard(d, self.nepochs, self._epoch, hs.utility, hs.over,
                                 self._hard_objective, self._hard_overtime, self._improved_hard,
                                 self._best_hard_utility, self._best_hard_epoch)
            return
        e = int(self._epoch)
        util, over = hs.utility[0], hs.over[0]
        for g in range(1, hs.utility.numel()):
            util, over = util + hs.utility[g], over + hs.over[g]
        if 0 <= e < self.nepochs:
            self._hard_objective[e], self._hard_overtime[e] = util, over
        improved = bool(util > self._best_hard_utility[0])
        self._improved_hard.fill_(int(improved))
        if improved:
            self._best_hard_utility[0], self._best_hard_epoch[0] = util, e

    def _copy_if_hard(self):
        be = self._be
        hs = self._hard
        pairs = list(zip((hs.visits, hs.fiber_time, hs.completeness), self._best_hard))
        if hasattr(be, "copy_if"):
            if self._hard_jobs is None:
                self._hard_jobs = be.copy_jobs(pairs)
            be.copy_if(self._improved_hard, self._hard_jobs)
        elif int(self._improved_hard):
            for s, t in pairs:
                t.copy_(s)

    def _build_snapshot(self):
        """The best state's buffers and the fixed part of the copy list (after
        the first step: Adam's flat moments and the counters' flat buffer exist)."""
        gnn, opt = self.gnn, self.optimizer
        flat = getattr(gnn, "_pf_flat", None)
        if flat is None:
            raise ValueError("TrainLoop needs a pfsgnn.GNN (its parameters in one flat buffer)")
        src = {"flat": flat}
        for gi, group in enumerate(opt.param_groups):
            if gi not in opt._flat:
                raise ValueError("TrainLoop needs FusedAdam's one-launch update: its parameters "
                                 "and gradients as views of the model's flat buffers")
            src[f"m{gi}"], src[f"v{gi}"] = opt._flat[gi]
            src[f"step{gi}"] = opt.state[group["params"][0]]["step"]
        for name, b in gnn.named_buffers():
            src["buf:" + name] = b
        src["comp"] = self._comp
        self._snap = {k: torch.zeros_like(v) for k, v in src.items()}
        self._snap["comp"] = self._best_completion
        pairs = [(src[k].detach(), self._snap[k]) for k in src]
        self._jobs = self._be.copy_jobs(pairs) if hasattr(self._be, "copy_jobs") else pairs

    # ------------------------------------------------------------ an epoch
    def _step(self):
        sharp = self._advance()
        self.gnn.zero_grad()
        out = self.gnn(self.graph)
        # (not finaloutput=True: that form copies its diagnostics to the host)
        d, ci, outs = _loss_apply(out, self.class_info, self.pclass, self.pfiber, sharp, True, None,
                                  self._seed, 0.3)
        loss, utils_g, n_prime, fiber_time, variance_g, time, loss_g = outs
        self._record(d, ci, loss_g, utils_g, variance_g, n_prime)
        if self.track_hard:
            self._record_hard(out)
        loss.backward()
        self.optimizer.step()
        self._copy_if(time, fiber_time)
        if self.track_hard:
            self._copy_if_hard()

    def run(self, n):
        """n more epochs.  Refuses to pass ``nepochs`` (the history has that many
        rows, and the schedule ends there)."""
        n = int(n)
        if n < 0 or self.epoch + n > self.nepochs:
            raise ValueError(f"run({n}) from epoch {self.epoch} would pass nepochs = {self.nepochs}")
        for _ in range(n):
            if not self.capture:
                self._step()
            elif self._graph is not None:
                self._graph.replay()
            elif self._warm == 0:
                self._step()
                self._warm = 1
            else:
                torch.cuda.synchronize()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    self._step()
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):     # a host sync inside the step would raise here
                    self._step()
                self._graph = g
                # the capture baked in the addresses of this batch's cached layout
                # and canonical edge tensor (gnn._LAYOUT_CACHE / _EDGE_CACHE, keyed
                # by the batch's edge_index and x_e): hold those two entries, so
                # that an eviction by other batches of the process cannot free
                # memory the replays read
                self._pinned = [c.d.get(id(t)) for c, t in
                                ((_gnn._LAYOUT_CACHE, self.graph.edge_index),
                                 (_gnn._EDGE_CACHE, self.graph.x_e))]
            self.epoch += 1
        return self

    # ------------------------------------------------------------ reading back
    def sharpness(self):
        """The sharpness of the epoch last run (host float; one sync)."""
        return float(self._sharp)

    def history(self):
        """train.py:114-122's arrays up to the current epoch (rows before
        ``start_epoch`` are 0): losses, objective, variances [epoch] and
        completions [NT, epoch] (None without ``record_completions``); with
        ``track_hard`` also hard_objective and hard_overtime (int32) [epoch]."""
        k = self.epoch
        bufs = dict(losses=self._losses[:k], objective=self._objective[:k],
                    variances=self._variances[:k],
                    completions=None if self._completions is None else self._completions[:, :k])
        if self.track_hard:
            bufs.update(hard_objective=self._hard_objective[:k],
                        hard_overtime=self._hard_overtime[:k])
        return {n: None if t is None else t.cpu().numpy() for n, t in bufs.items()}

    def best(self):
        """train.py:117-121, 148-152: loss, utility, epoch (-1: no epoch has
        qualified) and the time [E], fiber_time [NS], completion [NT] of that epoch."""
        return dict(loss=float(self._best_loss), utility=float(self._best_utility),
                    epoch=int(self._best_epoch), time=self._best_time.cpu().numpy(),
                    fiber_time=self._best_fiber_time.cpu().numpy(),
                    completion=self._best_completion.cpu().numpy())

    def hard_best(self):
        """The best integer objective so far (``track_hard``): utility, epoch
        (-1: no epoch has had a positive hard utility) and the visits [E] (int32,
        caller's edge order), fiber_time [NS], completion [NT] of that epoch."""
        if not self.track_hard:
            raise ValueError("hard_best() needs TrainLoop(..., track_hard=True)")
        visits, fiber_time, completion = self._best_hard
        return dict(utility=float(self._best_hard_utility), epoch=int(self._best_hard_epoch),
                    visits=visits.cpu().numpy(), fiber_time=fiber_time.cpu().numpy(),
                    completion=completion.cpu().numpy())

    def plan(self, cap=True, segments=True):
        """The observing plan (``observing_plan``) of the best integer schedule so
        far (``track_hard``; with ``track_hard="budget"`` the best executable
        one): its visits go from the device buffer straight into the op.  Before
        any epoch has had a positive hard utility the best visits are all 0 and
        the plan is empty."""
        if not self.track_hard:
            raise ValueError("plan() needs TrainLoop(..., track_hard=True)")
        return observing_plan(self.graph, self.class_info, self._best_hard[0], cap=cap,
                              segments=segments, _F=getattr(self.gnn, "Fdim", None))

    def _optim_state(self, tensors):
        """optimizer.state_dict() with its state tensors replaced by
        ``tensors(gi) -> (m flat, v flat, step)``, cloned."""
        from .optim import _flat_base
        sd = self.optimizer.state_dict()
        state, i = {}, 0
        for gi, group in enumerate(self.optimizer.param_groups):
            m, v, step = tensors(gi)
            _, offs = _flat_base([p.detach() for p in group["params"]])
            for p, off in zip(group["params"], offs):
                state[i] = {"step": step.clone(), "exp_avg": m[off:off + p.numel()].view(p.shape).clone(),
                            "exp_avg_sq": v[off:off + p.numel()].view(p.shape).clone()}
                i += 1
        return {"state": state, "param_groups": sd["param_groups"]}

    def checkpoint(self, epoch=None):
        """train.py:161-165's dict for the current state; ``epoch`` defaults to
        the epoch last run, so that a resume (train.py:132) continues with the next."""
        if self._jobs is None:    # before the first step: the optimizer's own (empty) state
            optim_state = self.optimizer.state_dict()
        else:
            opt = self.optimizer
            optim_state = self._optim_state(
                lambda gi: opt._flat[gi] + (opt.state[opt.param_groups[gi]["params"][0]]["step"],))
        model_state = type(self.gnn.state_dict())(
            (k, v.detach().clone()) for k, v in self.gnn.state_dict().items())
        return {"epoch": self.epoch - 1 if epoch is None else int(epoch),
                "model_state": model_state, "optim_state": optim_state}

    def best_checkpoint(self):
        """train.py:154-158's dict of the best epoch (weights and optimizer state
        after that epoch's update); None when no epoch has qualified."""
        e = int(self._best_epoch)
        if e < 0 or self._snap is None:
            return None
        snap, gnn = self._snap, self.gnn
        pslice = {n: snap["flat"][off:off + cnt].view(p.shape)
                  for (n, p), (off, cnt) in zip(gnn.named_parameters(), gnn._pf_off)}
        sd = gnn.state_dict()
        model_state = type(sd)(
            (k, (pslice[k] if k in pslice else snap["buf:" + k]).clone()) for k in sd)
        optim_state = self._optim_state(
            lambda gi: (snap[f"m{gi}"], snap[f"v{gi}"], snap[f"step{gi}"]))
        return {"epoch": e, "model_state": model_state, "optim_state": optim_state}


def main(argv=None):
    """train.py:82-165 (training + checkpointing; the plotting of train.py:168-305
    is not part of the hot path and is skipped)."""
    from .optim import FusedAdam
    argv = sys.argv[1:] if argv is None else argv
    idx = int(os.environ.get("SLURM_ARRAY_TASK_ID", 0))
    ID = str(idx)
    class_info = torch.tensor(np.loadtxt(config.datafile), dtype=torch.float, device=config.device)
    NF, NC = config.NFIBERS, class_info.shape[0]
    graph = complete_graph(class_info, NF, config.Fdim)
    gnn = GNN(Fdim=config.Fdim, B=3, F_s=1, F_t=class_info.shape[1], T=NC).to(config.device)
    gnn.train()
    optimizer = FusedAdam(gnn.parameters(), lr=config.lr, capturable=True)
    nepochs = config.nepochs
    start_epoch = 0
    if argv:
        ck = torch.load(argv[0], map_location=config.device, weights_only=True)
        gnn.load_state_dict(ck["model_state"])
        optimizer.load_state_dict(ck["optim_state"])
        start_epoch = min(ck["epoch"] + 1, nepochs)   # (a final checkpoint: nothing left to run)
    # the whole epoch (schedule, forward, loss, history, backward, Adam, best
    # snapshot) as one graph replay; PFSGNN_TRAIN_CAPTURE=0: the same launches eagerly
    loop = TrainLoop(gnn, optimizer, graph, class_info, nepochs, config.sharps, config.min_sharp,
                     config.pclass, config.pfiber, start_epoch=start_epoch,
                     capture=os.environ.get("PFSGNN_TRAIN_CAPTURE", "1") != "0")
    loop.run(max(0, nepochs - start_epoch))
    # train.py:161-165, and the best state beside it (the reference rewrites the
    # one file on every improvement and then overwrites it with the final state)
    torch.save(loop.checkpoint(epoch=nepochs), config.checkpoint_path + ID + ".pth")
    best = loop.best_checkpoint()
    if best is not None:
        torch.save(best, config.checkpoint_path + ID + "_best.pth")
    return loop


if __name__ == "__main__":
    main()
