"""Helper of tests/test_sliced_ops_ref.py and tests/test_gpu_sliced_ops.py:
adversarial general graphs for the fused sliced edge kernels
(csrc/pfsgnn_sliced.hip), exact-grid inputs in the caller's edge order, and one
runner that takes any backend (the float64 / float32 emulation on the composed
ops of pfsgnn.sparse, the complete-graph emulation, HipBackend on the sliced or
the complete kernels) through the six edge ops and hands every output back in
one form: edge tensors [C, E] in the caller's order, node tensors as they are.

The graphs are the smallest that reach the branches a uniform-density graph
never takes (General graphs, Parity):

* ``hub``: one fiber joined to every class next to many fibers of degree 0-3
  (maxdeg >= 64 -> KS = 8 step splits, most of them empty; slices of length 0
  and 1 -> source_fwd waves without steps; tiles with one valid lane; EP / E
  ~ 7 -> mostly padding; absent fibers; NC at the class-table limit), and a
  graph whose tiles hold 8 lanes on each of two classes (acc_add's owner
  rounds at their longest, 8);
* ``complete``: the full bipartite graph given to the sliced layout (every
  tile 16 valid lanes on one class: acc_add's row-sum form);
* ``one_class``: NC = 1;
* ``one_fiber_block``: a 64-fiber block holding one fiber, edgeless in graph 0;
* ``ragged``: the ordinary case.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "pfs-neural-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from emu_backend import Dims, EmuBackend, _user_index  # noqa: E402
from harness import canonical_edges  # noqa: E402
from test_gpu_ops import cpu, cuda, r  # noqa: E402
from test_sparse_emu import sparse_edges  # noqa: E402

CASES = ("hub", "complete", "one_class", "one_fiber_block", "ragged")


# ------------------------------------------------------------------ graphs
def hub_edges(ncmax):
    """(G, NF, NC, edge_index) of the hub case; NC = ncmax (the class-table limit)."""
    G, NF, NC = 2, 70, int(ncmax)
    assert NC >= 10
    gen = torch.Generator().manual_seed(4100 + NC)
    src, tgt = [], []
    # graph 0: fiber 3 on every class; fibers 0-15 (but 3) on 1-3 classes; fibers
    # 16-63 and 69 on one class; fibers 64-68 edgeless
    src += [3] * NC
    tgt += list(range(NC))
    for f in range(16):
        if f == 3:
            continue
        k = int(torch.randint(1, 4, (1,), generator=gen))
        for c in torch.randperm(NC, generator=gen)[:k].tolist():
            src.append(f)
            tgt.append(c)
    for f in list(range(16, 64)) + [69]:
        src.append(f)
        tgt.append(int(torch.randint(0, NC, (1,), generator=gen)))
    # graph 1: every fiber on classes 5 and 9; fiber 0 on class 5 another 20 times
    first = len(src)
    for f in range(NF):
        src += [NF + f, NF + f]
        tgt += [NC + 5, NC + 9]
    src += [NF] * 20
    tgt += [NC + 5] * 20
    # caller order: a seeded shuffle (sort by random keys).  A fiber's edges keep
    # the caller's relative order in the layout, so within graph 1 the keys of a
    # fiber's (5, 9) pair are ordered by the fiber's parity: class 5 first on even
    # fibers, class 9 first on odd ones -- a full slice's tile then holds 8 lanes
    # on each class whatever the seed
    key = torch.rand(len(src), generator=gen)
    for f in range(NF):
        i = first + 2 * f
        lo, hi = sorted((float(key[i]), float(key[i + 1])))
        key[i], key[i + 1] = (lo, hi) if f % 2 == 0 else (hi, lo)
    p = torch.argsort(key)
    return G, NF, NC, torch.stack([torch.tensor(src)[p], torch.tensor(tgt)[p]])


def case_edges(case, ncmax=128):
    """-> (G, NF, NC, edge_index [2, E] in the caller's order)."""
    if case == "hub":
        return hub_edges(ncmax)
    if case == "complete":
        G, NF, NC = 2, 40, 12
        return G, NF, NC, canonical_edges(G, NF, NC)      # fiber-major, not shuffled
    gen = torch.Generator().manual_seed({"one_class": 31, "one_fiber_block": 32, "ragged": 33}[case])
    if case == "one_class":
        G, NF, NC = 1, 33, 1
        # (its one class cannot be the empty one; fiber 1 is edgeless, 9 repeated pairs)
        return G, NF, NC, sparse_edges(G, NF, NC, 1.0, gen, dup=9, empty_class=False)
    if case == "one_fiber_block":
        G, NF, NC = 3, 65, 7
        return G, NF, NC, sparse_edges(G, NF, NC, 0.5, gen, dup=4)
    if case == "ragged":
        G, NF, NC = 3, 130, 40
        return G, NF, NC, sparse_edges(G, NF, NC, 0.3, gen, dup=17)
    raise KeyError(case)


def plan_of(ei, G, NF, NC):
    """The emulated sparse layout of ``ei`` and its sliced plan (sliced_plan_ref)."""
    from test_gpu_sparse import sliced_plan_ref
    sp = EmuBackend().sparse_layout(ei, G, NF, NC)
    return sp, sliced_plan_ref(sp.fib_ptr, sp.src_p, sp.tgt_p, sp.user_of, G, NF, NC)


def step_classes(plan):
    """For every (slice, step): the classes of its valid lanes (a 1-D tensor)."""
    out = []
    for s in range(plan["len"].numel()):
        for k in range(int(plan["len"][s])):
            q0 = int(plan["base"][s]) + 16 * k
            c = plan["cls"][q0:q0 + 16]
            out.append((s, k, c[c != 255]))
    return out


# ------------------------------------------------------------------ slots
def to_slots(t_user, sl):
    """[C, E] in the caller's order -> [C, EP] over the sliced positions, 0 at padding."""
    pu = sl.pos_user.long()
    out = torch.zeros(t_user.shape[0], pu.numel(), dtype=t_user.dtype, device=t_user.device)
    valid = pu >= 0
    out[:, valid] = t_user[:, pu[valid].to(t_user.device)]
    return out


def from_slots(t_slots, sl):
    """[C, EP] over the sliced positions -> [C, E] in the caller's order."""
    pu = sl.pos_user.long().to(t_slots.device)
    valid = pu >= 0
    out = torch.empty(t_slots.shape[0], sl.E, dtype=t_slots.dtype, device=t_slots.device)
    out[:, pu[valid]] = t_slots[:, valid]
    return out


# ------------------------------------------------------------------ inputs
def q(t, step):
    return torch.round(t / step) * step


def nonzero(t, step):
    return torch.where(t == 0, torch.full_like(t, step), t)


def make_inputs(G, NF, NC, F, E, seed):
    """test_gpu_ops.test_edge_ops's grid recipe (float64, edge tensors in the
    caller's order): weights of every first Linear on 1/64, edge inputs on 1/16,
    node parts on 1/256, lazy-state scales on 1/16 or 1/8 -- every first-layer
    pre-activation is exact on every path, so no LeakyReLU kink can flip.  The
    lazy-state shifts are non-zero in every channel: x = sc * 0 + sh != 0 at a
    padding position unless the kernel masks it.  ``y`` (edge_mlp_fwd's output
    re-quantised to 1/4) is added by the float64 reference run."""
    gen = torch.Generator().manual_seed(seed)
    NS, NT = G * NF, G * NC
    i = {}
    i["xe"] = q(r(F, E, scale=2, off=3, gen=gen), 1 / 16)
    i["xsc"], i["xsh"] = q(r(F, gen=gen) * 0.5 + 1, 1 / 16), nonzero(q(r(F, gen=gen), 1 / 16), 1 / 16)
    i["Ps"], i["Pt"] = q(r(4 * F, NS, gen=gen), 1 / 256), q(r(4 * F, NT, gen=gen), 1 / 256)
    i["W1"], i["W2"], i["b2"] = q(r(4 * F, 4 * F, scale=0.3, gen=gen), 1 / 64), r(F, 4 * F, scale=0.3, gen=gen), r(F, gen=gen)
    i["sc"], i["sh"] = q(r(F, gen=gen) * 0.3 + 1, 1 / 8), nonzero(q(r(F, gen=gen), 1 / 8), 1 / 8)
    i["Qt"] = q(r(2 * F, NT, gen=gen), 1 / 256)
    i["Ws1"], i["Ws2"], i["bs2"] = q(r(2 * F, 2 * F, scale=0.3, gen=gen), 1 / 64), r(2 * F, 2 * F, scale=0.3, gen=gen), r(2 * F, gen=gen)
    i["Rs"], i["Wt1"] = q(r(2 * F, NS, gen=gen), 1 / 256), q(r(2 * F, 2 * F, scale=0.3, gen=gen), 1 / 64)
    i["g_hsum"] = r(2 * F, NT, gen=gen)
    i["mean"] = r(2 * F, NS, gen=gen)
    i["coef"] = r(4, 2 * F, NS, gen=gen) * torch.tensor([1, 0.3, 0.1, 0.03], dtype=torch.float64)[:, None, None]
    i["g_next"] = r(F, E, gen=gen)
    i["mu1"], i["var1"] = r(F, gen=gen), r(F, gen=gen).abs() + 0.5
    i["inv1"] = 1.0 / torch.sqrt(i["var1"] + 1e-5)
    i["alpha"], i["gam0"], i["gam1"] = r(F, gen=gen), r(F, gen=gen) * 0.1, r(F, gen=gen) * 0.1
    # the node epilogues (test_edge_ops_node_epilogues) and the BatchNorm forms
    i["Wt2"], i["bt2"] = r(2 * F, 2 * F, scale=0.3, gen=gen), r(2 * F, gen=gen)
    i["g_xs0"], i["g_xt0"] = r(F, NS, gen=gen), r(F, NT, gen=gen)
    i["gamma"], i["beta"] = r(F, gen=gen).abs() + 0.5, r(F, gen=gen)
    i["rm"], i["rv"] = r(F, gen=gen) * 0.1, r(F, gen=gen).abs() + 0.5
    return i


EDGE_KEYS = ("xe", "g_next", "y")


# ------------------------------------------------------------------ runners
class Run:
    """One backend on one batch: ``conv`` moves a node tensor or a weight to the
    backend, ``edge_in`` a caller-order edge tensor [C, E] into the backend's
    edge layout, ``edge_out`` back.  ``variants``: also run the forms only the
    HIP backend has (the TModel mask buffer).  ``poison(*shapes)`` is called
    with the shapes of the outputs the next op allocates.  ``raw`` collects the
    edge outputs in the backend's own layout (padding checks)."""

    def __init__(self, be, d, conv, edge_in, edge_out, variants=False, poison=None):
        self.be, self.d, self.conv = be, d, conv
        self.edge_in, self.edge_out = edge_in, edge_out
        self.variants = variants
        self.poison = poison or (lambda *shapes: None)
        self.raw = {}

    def zeros(self, *shape):
        return self.conv(torch.zeros(*shape, dtype=torch.float64))

    def full(self, v, *shape):
        return self.conv(torch.full(shape, v, dtype=torch.float64))


def emu_sparse_run(ei, G, NF, NC, F, dtype=torch.float64):
    """The reference: pfsgnn.sparse.SparseEdgeOps on the emulated primitives
    (tests/test_sparse_emu.py holds it to the autograd oracle), edge tensors in
    the emulated layout's position order."""
    be = EmuBackend(dtype=dtype)
    sp = be.sparse_layout(ei, G, NF, NC)
    d = Dims(G, NF, NC, F, sp=sp)
    pos = sp.user_of

    def e_out(t):
        out = torch.empty_like(t)
        out[:, pos] = t
        return out
    return Run(be, d, lambda t: None if t is None else t.to(dtype).clone(),
               lambda t: t[:, pos].to(dtype).contiguous(), e_out)


def emu_complete_run(G, NF, NC, F, dtype=torch.float64):
    """The complete-graph emulation (test_edge_ops's reference), canonical
    class-major edge tensors; the caller's order is train.py's fiber-major one."""
    be = EmuBackend(dtype=dtype)
    d = Dims(G, NF, NC, F)
    eu = _user_index(d, torch.device("cpu"))       # caller position of each canonical edge

    def e_out(t):
        out = torch.empty_like(t)
        out[:, eu] = t
        return out
    return Run(be, d, lambda t: None if t is None else t.to(dtype).clone(),
               lambda t: t[:, eu].to(dtype).contiguous(), e_out)


def nan_poison(*shapes):
    """The wrappers allocate outputs with torch.empty: fill blocks of the outputs'
    sizes with NaN and release them, so that the recycled memory is not zero by luck."""
    ts = [torch.full(s, float("nan"), device="cuda") for s in shapes]
    del ts


def hip_sliced_run(hb, ei, G, NF, NC, F):
    sp = hb.sparse_layout(ei.cuda(), G, NF, NC)
    sp.sl = hb.sliced_layout(sp, G, NF, NC)
    from pfsgnn.engine import Dims as HDims
    d = HDims(G, NF, NC, F, sp=sp)
    return Run(hb, d, cuda, lambda t: to_slots(cuda(t), sp.sl), lambda t: from_slots(t, sp.sl),
               variants=True, poison=nan_poison)


def hip_complete_run(hb, G, NF, NC, F):
    from pfsgnn.engine import Dims as HDims
    d = HDims(G, NF, NC, F)
    eu = _user_index(d, torch.device("cpu")).cuda()

    def e_out(t):
        out = torch.empty_like(t)
        out[:, eu] = t
        return out
    return Run(hb, d, cuda, lambda t: cuda(t)[:, eu].contiguous(), e_out, variants=True,
               poison=nan_poison)


def _node(R, inp):
    return {k: R.conv(v) for k, v in inp.items() if k not in EDGE_KEYS}


def run_ops(R, inp):
    """test_edge_ops's sequence of the six edge ops on backend ``R``.  -> {name:
    tensor}; ``name@variant`` is another form of the call with the same result
    as ``name`` (with the TModel mask buffer, without the optional gxe),
    ``name.bare`` source_bwd without its optional parts.  The first run (the
    float64 reference) adds ``y`` to ``inp``."""
    be, d, F = R.be, R.d, R.d.F
    n = _node(R, inp)
    o = {}
    EP, NS, NT = d.EP, d.NS, d.NT
    xe = R.edge_in(inp["xe"])
    # edge_mlp_fwd
    R.poison((F, EP), (F,), (F,))
    y_, o["mu"], o["var"] = be.edge_mlp_fwd(d, xe, n["xsc"], n["xsh"], n["Ps"], n["Pt"], n["W1"],
                                            n["W2"], n["b2"])
    R.raw["y"] = y_
    o["y"] = R.edge_out(y_)
    if "y" not in inp:
        inp["y"] = q(o["y"].double(), 1 / 4)
    y = R.edge_in(inp["y"])
    sc, sh = n["sc"], n["sh"]
    # source_fwd (hs pre-filled with NaN: every fiber's column must be written)
    hs = R.full(float("nan"), 8 * F, NS)
    R.poison((4, 2 * F, NS))
    mom = be.source_fwd(d, y, sc, sh, n["Qt"], n["Ws1"], n["Ws2"], n["bs2"], hs)
    for i, nm in enumerate(("mean", "c2", "c3", "c4")):
        o[nm] = mom[i]
    o["hs"] = hs
    # target_fwd / target_bwd, without and with the forward's mask buffer
    R.poison((2 * F, NT))
    o["hsum"] = be.target_fwd(d, y, sc, sh, n["Rs"], n["Wt1"])
    tm = be.tmask(d) if R.variants else None
    if R.variants and d.sp is not None:
        assert tm is not None
    if tm is not None:
        tm.fill_(0xA5)
        R.poison((2 * F, NT))
        o["hsum@tm"] = be.target_fwd(d, y, sc, sh, n["Rs"], n["Wt1"], tmask=tm)
    for sfx, kw in (("", {}), ("@tm", {"tmask": tm})):
        if sfx and tm is None:
            continue
        dWt1 = R.zeros(2 * F, 2 * F)
        R.poison((2 * F, NS), (F, EP))
        o["GzT" + sfx], g_ = be.target_bwd(d, y, sc, sh, n["Rs"], n["Wt1"], n["g_hsum"], dWt1,
                                           want_gxe=True, **kw)
        R.raw["gxeT" + sfx] = g_
        o["gxeT" + sfx], o["dWt1" + sfx] = R.edge_out(g_), dWt1
    # source_bwd with T part, g_next and BN sums
    g_next = R.edge_in(inp["g_next"])
    for sfx, kw in (("", {}), ("@tm", {"tmask": tm})):
        if sfx and tm is None:
            continue
        gr = [R.zeros(2 * F, 2 * F), R.zeros(2 * F, 2 * F), R.zeros(2 * F)]
        R.poison((F, EP), (2 * F, NT), (F,), (F,))
        out = be.source_bwd(d, y, sc, sh, n["Qt"], n["Ws1"], n["Ws2"], n["bs2"], n["mean"], n["coef"],
                            (n["Rs"], n["Wt1"], n["g_hsum"]), g_next, (n["mu1"], n["inv1"]), *gr, **kw)
        R.raw["g_tot" + sfx] = out[0]
        o["g_tot" + sfx] = R.edge_out(out[0])
        for v, nm in zip(list(out[1:4]) + gr, ("GzS", "Sg", "Sgx", "dWs1", "dWs2", "dbs2")):
            o[nm + sfx] = v
    # source_bwd bare
    gr = [R.zeros(2 * F, 2 * F), R.zeros(2 * F, 2 * F), R.zeros(2 * F)]
    R.poison((F, EP), (2 * F, NT))
    out = be.source_bwd(d, y, None, None, n["Qt"], n["Ws1"], n["Ws2"], n["bs2"], n["mean"], n["coef"],
                        None, None, None, *gr)
    R.raw["g_tot.bare"] = out[0]
    o["g_tot.bare"], o["GzS.bare"] = R.edge_out(out[0]), out[1]
    for v, nm in zip(gr, ("dWs1", "dWs2", "dbs2")):
        o[nm + ".bare"] = v
    # the edge BatchNorm's gradient sums on their own (on a general batch plain
    # column sums over the slot tensors: they hold because padding holds 0)
    R.poison((F,), (F,))
    o["Sg.sums"], o["Sgx.sums"] = be.edge_bn_grad_sums(d, g_next, y, n["mu1"], n["inv1"])
    # edge_mlp_bwd with and without the edge-input gradient
    for sfx, want in (("", True), ("@ng", False)):
        gr = [R.zeros(4 * F, 4 * F), R.zeros(F, 4 * F), R.zeros(F)]
        R.poison((F, EP), (4 * F, NS), (4 * F, NT))
        out = be.edge_mlp_bwd(d, g_next, n["alpha"], n["gam0"], n["gam1"], y, xe, n["xsc"], n["xsh"],
                              n["Ps"], n["Pt"], n["W1"], n["W2"], *gr, want_gxe=want)
        if want:
            R.raw["gxe"] = out[0]
            o["gxe"] = R.edge_out(out[0])
        else:
            assert out[0] is None
        for v, nm in zip(list(out[1:3]) + gr, ("GzEs", "GzEt", "dW1", "dW2", "db2")):
            o[nm + sfx] = v
    return {k: cpu(v) for k, v in o.items()}


def run_epilogues(R, inp):
    """The forms Engine uses on a general batch (engine.py: target_fwd's second
    Linear with the degree-scaled bias, the node-input gradients in the
    reductions' epilogues, the BatchNorm finish of edge_mlp_fwd and of
    source_bwd).  ``inp`` holds ``y`` (run_ops on the reference first)."""
    be, d, F = R.be, R.d, R.d.F
    n = _node(R, inp)
    o = {}
    EP, NS, NT = d.EP, d.NS, d.NT
    E = d.E
    xe, y, g_next = R.edge_in(inp["xe"]), R.edge_in(inp["y"]), R.edge_in(inp["g_next"])
    sc, sh = n["sc"], n["sh"]
    tm = be.tmask(d) if R.variants else None
    kw = {"tmask": tm} if tm is not None else {}
    # Engine.target_fwd with d.sp set
    R.poison((2 * F, NT))
    hsum = be.target_fwd(d, y, sc, sh, n["Rs"], n["Wt1"], **kw)
    agg = be.lin(n["Wt2"], 0, 2 * F, hsum)
    be.lin(n["bt2"].view(-1, 1), 0, 1, d.sp.deg_t, out=agg, add=True)
    o["hsum"], o["agg"] = hsum, agg
    # target_bwd + g_xs
    dWt1, g_xs = R.zeros(2 * F, 2 * F), R.conv(inp["g_xs0"])
    R.poison((2 * F, NS))
    o["GzT"], _ = be.target_bwd(d, y, sc, sh, n["Rs"], n["Wt1"], n["g_hsum"], dWt1, g_xs=g_xs, **kw)
    o["g_xs(T)"], o["dWt1"] = g_xs, dWt1
    # source_bwd + g_xt + the edge BatchNorm's backward coefficients (n = E)
    gr = [R.zeros(2 * F, 2 * F), R.zeros(2 * F, 2 * F), R.zeros(2 * F)]
    g_xt, dg, db = R.conv(inp["g_xt0"]), R.zeros(F), R.zeros(F)
    R.poison((F, EP), (2 * F, NT), (F,), (F,), (F,))
    out = be.source_bwd(d, y, sc, sh, n["Qt"], n["Ws1"], n["Ws2"], n["bs2"], n["mean"], n["coef"],
                        (n["Rs"], n["Wt1"], n["g_hsum"]), g_next, (n["mu1"], n["inv1"]), *gr,
                        bn2=(n["gamma"], n["var1"], E, 1e-5, dg, db), g_xt=g_xt, **kw)
    assert out[2] is None and out[3] is None
    o["g_tot"], o["GzS"] = R.edge_out(out[0]), out[1]
    o["bn.alpha"], o["bn.gam0"], o["bn.gam1"] = out[4]
    o["bn.dgamma"], o["bn.dbeta"], o["g_xt(S)"] = dg, db, g_xt
    # edge_mlp_bwd + nodes
    gr = [R.zeros(4 * F, 4 * F), R.zeros(F, 4 * F), R.zeros(F)]
    nxs, nxt = R.conv(inp["g_xs0"]), R.conv(inp["g_xt0"])
    R.poison((4 * F, NS), (4 * F, NT), (F, NT))
    out = be.edge_mlp_bwd(d, g_next, n["alpha"], n["gam0"], n["gam1"], y, xe, n["xsc"], n["xsh"],
                          n["Ps"], n["Pt"], n["W1"], n["W2"], *gr, want_gxe=False, nodes=(nxs, nxt))
    o["GzEs"], o["GzEt"], o["Vu"] = out[1:]
    o["g_xs(E)"], o["g_xt(E)"] = nxs, nxt
    # edge_mlp_fwd_bn (bn2_finalize with n = E, the running statistics updated twice)
    rm, rv = R.conv(inp["rm"]), R.conv(inp["rv"])
    R.poison((F, EP), (F,), (F,), (F,), (F,), (F,), (F,))
    out = be.edge_mlp_fwd_bn(d, xe, n["xsc"], n["xsh"], n["Ps"], n["Pt"], n["W1"], n["W2"], n["b2"],
                             (n["gamma"], n["beta"], rm, rv, 0.1, 1e-5))
    o["y"] = R.edge_out(out[0])
    for v, nm in zip(out[1:], ("mu", "var", "bn.sc", "bn.sh", "bn.inv1")):
        o[nm] = v
    o["bn.rm"], o["bn.rv"] = rm, rv
    return {k: cpu(v) for k, v in o.items()}


# ------------------------------------------------------------------ the bound
# test_gpu_ops.test_edge_ops / test_edge_ops_node_epilogues' rtol of each output
RTOL = dict.fromkeys(("y", "mu", "var", "hsum", "agg", "GzT", "gxeT", "dWt1", "Sg.sums", "Sgx.sums",
                      "bn.sc", "bn.sh", "bn.inv1", "bn.rm", "bn.rv"), 2e-4)
RTOL.update(dict.fromkeys(("mean", "c2", "c3", "c4"), 1e-3))
RTOL["hs"] = 2e-3
RTOL.update(dict.fromkeys(("g_tot", "GzS", "Sg", "Sgx", "dWs1", "dWs2", "dbs2", "gxe", "GzEs", "GzEt",
                           "dW1", "dW2", "db2", "Vu", "g_xs(T)", "g_xt(S)", "g_xs(E)", "g_xt(E)",
                           "bn.alpha", "bn.gam0", "bn.gam1", "bn.dgamma", "bn.dbeta"), 5e-4))
ATOL = {"hs": 1e-3}


def ref_name(name):
    """The reference output a (variant) output is compared with."""
    return name.split("@")[0]


def bound_of(name, r64, r32):
    """max(rtol x max|ref64| (+ hs's atol), 16 x max|ref32 - ref64|): the
    op-level tolerance of test_edge_ops for this output, or 16 times the error
    of the same reference run in float32 -- nothing from the code under test."""
    base = ref_name(name).split(".bare")[0]
    scale = r64.abs().max().item() if r64.numel() else 0.0
    e32 = (r32.double() - r64).abs().max().item() if r64.numel() else 0.0
    return max(RTOL[base] * scale + ATOL.get(base, 0.0), 16.0 * e32)


def max_err(a, b):
    return (a - b).abs().max().item() if b.numel() else 0.0


_REFS = {}


def reference(case, F, ncmax=128, epilogues=False):
    """-> (G, NF, NC, ei, inp, ref64, ref32) of a case, computed once per process
    and shared (the float64 run adds ``y`` to ``inp``; nothing is changed after)."""
    key = (case, F, ncmax, epilogues)
    if key not in _REFS:
        if epilogues:
            G, NF, NC, ei, inp, _, _ = reference(case, F, ncmax)
            fn = run_epilogues
        else:
            G, NF, NC, ei = case_edges(case, ncmax)
            inp = make_inputs(G, NF, NC, F, ei.shape[1], 1000 * CASES.index(case) + F)
            fn = run_ops
        r64 = fn(emu_sparse_run(ei, G, NF, NC, F), inp)
        r32 = fn(emu_sparse_run(ei, G, NF, NC, F, dtype=torch.float32), inp)
        _REFS[key] = (G, NF, NC, ei, inp, r64, r32)
    return _REFS[key]
