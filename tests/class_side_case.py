"""Helper of tests/test_class_side_ref.py and tests/test_gpu_class_side_ops.py:
cases, deterministic inputs and float64 references of the fused class-side and
node-MLP ops (csrc/pfsgnn_mlp.hip: k_class_tail_fwd behind
pfsgnn_target_block_fwd, k_class_bwd behind pfsgnn_target_class_bwd,
k_class_global_fwd behind pfsgnn_target_global_fwd, pfsgnn_mlp_fwd_epi and
pfsgnn_mlp_bwd_pre).

The reference of a fused op is the unfused composition on EmuBackend, the calls
Engine makes where the fused op is absent:

* target_block_fwd = target_fwd(agg=(Wt2, bt2, NF)) then target_global_fwd;
* target_class_bwd = graph_reduce_multi(pend) into a copy of gu_up, global_bwd
  (scales 1/NF, 1/NC), mlp_bwd(outs=[(gxt_in, F, add), (g_agg, 2F), (gu_t, F)])
  and lin_t(Wt2, g_agg);
* mlp_fwd_epi and mlp_bwd(bn_part=, mom_coef=) are EmuBackend's own.

Every reference runs in float64 and in float32 (the reference's own rounding).
Inputs are float64 tensors holding float32-representable values, so the device
and the reference read the same numbers.

The unit geometry of the two barrier kernels is restated here from
``tail_ct`` / ``CB_CLS`` (csrc/pfsgnn_mlp.hip) as a function of (G, NF, NC,
ncu), ncu the CU count: the cases are the smallest shapes that reach the
branches whole-model parity never takes (a workgroup's second unit, CT = 32,
a ragged last unit beside full ones, QB = 64, units without fibers, more than
32 column partials).
"""
import collections
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "pfs-neural-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from emu_backend import Dims, EmuBackend  # noqa: E402
from test_gpu_ops import r  # noqa: E402

BN_MOM, BN_EPS = 0.1, 1e-5
RMS_EPS = float(torch.finfo(torch.float32).eps)

# ------------------------------------------------------------------ geometry
CB_CLS = 16          # k_class_bwd: classes per unit
QBMAX = 64           # CT_QBMAX, CB_QBMAX: units per graph
FWD_UNITS_MAX = 512  # tail_ct: G * ceil(NC / CT)
BWD_UNITS_MAX = 4096  # pfsgnn_target_class_bwd
FIBERS_PER_PARTIAL = 64   # one column partial per 64-fiber group (EdgeGeo.NFG)


def tail_ct(G, NC):
    """Classes per unit of k_class_tail_fwd: 16, or 32 where 16 would need more
    than 512 units or more than 64 per graph; 0: refused."""
    for ct in (16, 32):
        qb = -(-NC // ct)
        if G * qb <= FWD_UNITS_MAX and qb <= QBMAX:
            return ct
    return 0


def _side(G, NF, NC, ct, ncu):
    qb = -(-NC // ct)
    nunits = G * qb
    grid = min(nunits, ncu)
    return dict(CT=ct, QB=qb, nunits=nunits, grid=grid, max_trips=-(-nunits // grid),
                last_ncl=NC - (qb - 1) * ct,
                empty_fiber_units=sum(1 for q in range(qb) if NF * q // qb == NF * (q + 1) // qb))


def unit_geometry(G, NF, NC, ncu=256):
    """-> dict(fwd=..., bwd=..., BPG=...): the units of the two barrier kernels
    (None where the op refuses the shape) and the column partials per graph."""
    ct = tail_ct(G, NC)
    bwd_ok = -(-NC // CB_CLS) <= QBMAX and G * -(-NC // CB_CLS) <= BWD_UNITS_MAX
    return dict(fwd=_side(G, NF, NC, ct, ncu) if ct else None,
                bwd=_side(G, NF, NC, CB_CLS, ncu) if bwd_ok else None,
                BPG=-(-NF // FIBERS_PER_PARTIAL))


def unit_columns(G, NC, ct, first_unit):
    """Class columns (of [., G * NC] tables) owned by units >= first_unit."""
    qb = -(-NC // ct)
    cols = []
    for un in range(first_unit, G * qb):
        g, q = divmod(un, qb)
        cols += [g * NC + c for c in range(q * ct, min(NC, (q + 1) * ct))]
    return torch.tensor(cols, dtype=torch.long)


# ------------------------------------------------------------------ cases
CASES = ("one_class", "ragged_tail", "few_fibers", "fwd_limit", "many_units_ct16",
         "many_units_ct32", "many_partials", "bench_like")


def case_shapes(case, ncu=256):
    """-> [(G, NF, NC, F)] of a case on a device of ncu CUs."""
    if case == "one_class":
        return [(2, 5, 1, 10)]
    if case == "ragged_tail":
        return [(2, 7, 17, 10), (3, 4, 33, 8)]
    if case == "few_fibers":
        return [(1, 3, 1024, 10)]
    if case == "fwd_limit":
        return [(1, 2, 2048, 10)]
    if case == "many_units_ct16":
        return [(ncu + 8, 3, 16, 10)]
    if case == "many_units_ct32":
        G = max(40, ncu // 8 + 1)      # 8 G forward units of 32 classes > ncu
        return [(G, 2, 256, 16), (G, 2, 256, 10)]
    if case == "many_partials":
        return [(1, 34 * FIBERS_PER_PARTIAL + 5, 2, 10)]   # 35 partials: 32 + a tail of 3
    if case == "bench_like":
        return [(2, 130, 128, 10)]
    raise KeyError(case)


def assert_reaches_branch(case, shape, ncu):
    """The property a case is named for, from the restated geometry at ``ncu``
    CUs (the CPU test at 256, the GPU test at the device's count)."""
    G, NF, NC, F = shape
    g = unit_geometry(G, NF, NC, ncu)
    fwd, bwd = g["fwd"], g["bwd"]
    both = (fwd, bwd)
    assert fwd is not None and G * NF * NC <= 50000
    if case == "one_class":
        assert NC == 1 and G * NC == 2 and all(s["QB"] == 1 and s["last_ncl"] == 1 for s in both)
    elif case == "ragged_tail":
        assert all(s["CT"] == 16 and s["last_ncl"] == 1 and s["QB"] >= 2 for s in both)
    elif case == "few_fibers":
        assert all(s["QB"] == QBMAX and s["empty_fiber_units"] == QBMAX - NF for s in both)
    elif case == "fwd_limit":
        assert fwd["CT"] == 32 and fwd["QB"] == QBMAX and bwd is None
    elif case == "many_units_ct16":
        assert all(s["CT"] == 16 and ncu < s["nunits"] <= 2 * ncu and s["max_trips"] == 2 for s in both)
    elif case == "many_units_ct32":
        assert fwd["CT"] == 32 and fwd["nunits"] > ncu and fwd["CT"] * F > 256
        assert bwd["nunits"] > 2 * ncu and bwd["max_trips"] >= 3
    elif case == "many_partials":
        assert g["BPG"] > 32 and g["BPG"] % 32 != 0
    elif case == "bench_like":
        assert g["BPG"] == 3 and all(s["max_trips"] == 1 and s["last_ncl"] == 16 for s in both)
    else:
        raise KeyError(case)
    return g


Variant = collections.namedtuple("Variant", "normed nxt rmrv npend tmask scsh")
FULL = Variant(True, True, True, 4, True, True)
BARE = Variant(False, False, False, 0, False, False)
# every value of every option, and each next to both values of its neighbours
VARIANTS = (FULL, BARE, Variant(True, False, False, 1, True, False),
            Variant(False, True, True, 4, False, True), Variant(True, True, False, 1, False, True))
VARIANT_CASES = ("ragged_tail", "many_units_ct16")


def variant_id(v):
    return "-".join(("normed" if v.normed else "unnormed", "nxt" if v.nxt else "last",
                     "rv" if v.rmrv else "norv", f"pend{v.npend}", "tmask" if v.tmask else "nomask",
                     "scsh" if v.scsh else "noscsh"))


def case_list(ncu=256):
    """-> [(case, shape index, variant)] of the GPU tests."""
    out = []
    for case in CASES:
        for i in range(len(case_shapes(case, ncu))):
            for v in (VARIANTS if case in VARIANT_CASES else (FULL,)):
                out.append((case, i, v))
    return out


# ------------------------------------------------------------------ inputs
def f32(t):
    """The float64 tensor of t's float32 roundings."""
    return t.float().double()


def q(t, step):
    return torch.round(t / step) * step


def block_inputs(G, NF, NC, F, v, seed):
    """Inputs of target_block_fwd.  The per-edge layer's on test_edge_ops' grid
    (bf16-exact Wt1, y with few significant bits, Rs on a 1/256 grid: every
    path computes the pre-activation exactly, no LeakyReLU flips); the node
    inputs random, as test_mlp_fused's."""
    gen = torch.Generator().manual_seed(seed)
    d = Dims(G, NF, NC, F)
    i = dict(G=G, NF=NF, NC=NC, F=F)
    i["y"] = q(r(F, d.E, scale=2, gen=gen), 1 / 4)
    sc, sh = q(r(F, gen=gen) * 0.3 + 1, 1 / 8), q(r(F, gen=gen), 1 / 8)
    i["sc"], i["sh"] = (sc, sh) if v.scsh else (None, None)
    i["Rs"] = q(r(2 * F, d.NS, gen=gen), 1 / 256)
    i["Wt1"] = q(r(2 * F, 2 * F, scale=0.3, gen=gen), 1 / 64)
    i["Wt2"], i["bt2"] = r(2 * F, 2 * F, scale=0.3, gen=gen), r(2 * F, gen=gen)
    i["xt"], i["u"], i["xs"] = r(F, d.NT, gen=gen), r(F, G, gen=gen), r(F, d.NS, gen=gen)
    i["W1"], i["b1"] = r(4 * F, 4 * F, scale=0.2, gen=gen), r(4 * F, scale=0.3, gen=gen)
    i["W2"], i["b2"] = r(F, 4 * F, scale=0.2, gen=gen), r(F, gen=gen)
    i["gamma"], i["beta"] = r(F, gen=gen) * 0.2 + 1, r(F, gen=gen) * 0.1
    rm, rv = r(F, gen=gen) * 0.1, r(F, gen=gen).abs() + 0.5
    i["rm"], i["rv"] = (rm, rv) if v.rmrv else (None, None)
    i["gW1"], i["gb1"] = r(3 * F, 3 * F, scale=0.3, gen=gen), r(3 * F, gen=gen)
    i["gW2"], i["gb2"] = r(F, 3 * F, scale=0.3, gen=gen), r(F, gen=gen)
    gw = r(F, gen=gen).abs() + 0.5
    i["gw"] = gw if v.normed else None
    nxt = (r(4 * F, 4 * F, scale=0.3, gen=gen), r(4 * F, gen=gen),
           r(2 * F, 2 * F, scale=0.3, gen=gen), r(2 * F, gen=gen))
    i["nxt"] = nxt if v.nxt else None
    for k, t in i.items():
        if isinstance(t, torch.Tensor):
            i[k] = f32(t)
    if i["nxt"] is not None:
        i["nxt"] = tuple(f32(t) for t in i["nxt"])
    return i


def _cast(t, dtype):
    if t is None:
        return None
    if isinstance(t, (tuple, list)):
        return type(t)(_cast(x, dtype) for x in t)
    return t.to(dtype).clone() if isinstance(t, torch.Tensor) else t


def _tail(be, hT, G, NC, i, rm, rv, keep=None, rv_biased=False):
    """target_global_fwd spelt out (the mutants change it): BatchNorm statistics
    over the ``keep`` columns, the running variance biased or not."""
    F, NF = i["F"], i["NF"]
    N = G * NC
    _, Z, Yp, _, _ = be.mlp_fwd(hT, N, i["W1"], i["b1"], i["W2"], i["b2"], bn=None)
    S = Yp if keep is None else Yp[:, keep]
    n = S.shape[1]
    mu = S.mean(1)
    var = ((S - mu[:, None]) ** 2).mean(1)
    xt = (Yp - mu[:, None]) / torch.sqrt(var[:, None] + BN_EPS) * i["gamma"][:, None] + i["beta"][:, None]
    if rm is not None:
        rm.mul_(1 - BN_MOM).add_(BN_MOM * mu)
        rv.mul_(1 - BN_MOM).add_(BN_MOM * (var if rv_biased else var * n / max(n - 1, 1)))
    un, means, gZ, gV, rms = be.global_fwd(i["xs"], xt, i["u"], i["gW1"], i["gb1"], i["gW2"],
                                           i["gb2"], i["gw"], RMS_EPS, G)
    out = dict(Z=Z, Yp=Yp, xt=xt, mu=mu, var=var, means=means, gZ=gZ, gV=gV, u=un, rms=rms,
               Pt=None, Qt=None)
    if i["nxt"] is not None:
        We, be_, Ws, bs = i["nxt"]
        out["Pt"] = be.lin_cat(We, [(xt, F, False), (un, 3 * F, True)], N, b=be_)
        out["Qt"] = be.lin(Ws, 0, F, xt, b=bs)
    return out


FWD_CLASS_OUTS = ("hsum", "agg", "Z", "Yp", "xt", "Pt", "Qt")
BWD_CLASS_OUTS = ("dYp", "dZ", "g_agg", "gu_t", "g_hsum")
MUTANTS = {   # mutant -> the case named for it
    "bn_drops_last_unit": "ragged_tail",
    "second_unit_skipped": "many_units_ct16",
    "first_32_partials_only": "many_partials",
    "pending_table_left_out": "ragged_tail",
    "mean_scales_swapped": "ragged_tail",
    "agg_bias_not_scaled": "ragged_tail",
    "running_var_biased": "ragged_tail",
}


def ref_block_fwd(inp, dtype=torch.float64, mutant=None, ncu=256, spelt=False):
    """The reference of target_block_fwd (and, from ``agg`` on, of
    target_global_fwd): -> dict of every output.  ``spelt``: through _tail
    instead of EmuBackend.target_global_fwd (the CPU test holds them equal)."""
    be = EmuBackend(dtype)
    i = {k: _cast(t, dtype) for k, t in inp.items()}
    G, NF, NC, F = i["G"], i["NF"], i["NC"], i["F"]
    d = Dims(G, NF, NC, F)
    bscale = 1.0 if mutant == "agg_bias_not_scaled" else float(NF)
    if mutant == "first_32_partials_only":
        assert G == 1
        nf = 32 * FIBERS_PER_PARTIAL
        e = (torch.arange(NC)[:, None] * NF + torch.arange(nf)[None, :]).reshape(-1)
        hsum, agg = be.target_fwd(Dims(1, nf, NC, F), i["y"][:, e], i["sc"], i["sh"],
                                  i["Rs"][:, :nf], i["Wt1"], agg=(i["Wt2"], i["bt2"], bscale))
    else:
        hsum, agg = be.target_fwd(d, i["y"], i["sc"], i["sh"], i["Rs"], i["Wt1"],
                                  agg=(i["Wt2"], i["bt2"], bscale))
    hT = [(i["xt"], 0, False), (agg, F, False), (i["u"], 3 * F, True)]
    rm, rv = i["rm"], i["rv"]
    if mutant in ("bn_drops_last_unit", "running_var_biased") or spelt:
        keep = None
        if mutant == "bn_drops_last_unit":
            ct = tail_ct(G, NC)
            drop = unit_columns(G, NC, ct, G * -(-NC // ct) - 1)
            keep = torch.ones(G * NC, dtype=torch.bool)
            keep[drop] = False
        t = _tail(be, hT, G, NC, i, rm, rv, keep=keep, rv_biased=mutant == "running_var_biased")
    else:
        t = be.target_global_fwd(hT, G, NC, i["W1"], i["b1"], i["W2"], i["b2"],
                                 (i["gamma"], i["beta"], rm, rv, BN_MOM, BN_EPS), i["xs"], NF,
                                 i["u"], i["gW1"], i["gb1"], i["gW2"], i["gb2"], i["gw"], RMS_EPS,
                                 i["nxt"])
    out = dict(hsum=hsum, agg=agg, rm=rm, rv=rv)
    out.update({k: t[k] for k in ("Z", "Yp", "xt", "mu", "var", "means", "gZ", "gV", "u", "Pt", "Qt")})
    if t["rms"] is not None:
        out["y1"], out["r1"], out["r2"] = t["rms"][0], t["rms"][1].reshape(-1), t["rms"][2].reshape(-1)
    else:
        out["y1"] = out["r1"] = out["r2"] = None
    out = {k: v for k, v in out.items() if v is not None}
    if mutant == "second_unit_skipped":
        cols = unit_columns(G, NC, tail_ct(G, NC), ncu)
        for k in FWD_CLASS_OUTS:
            if k in out:
                out[k] = out[k].clone()
                out[k][:, cols] = 0
    return out


def class_bwd_inputs(inp, fwd, v, seed, round32=True):
    """Inputs of target_class_bwd: the forward reference's saved tensors and
    random upstream gradients.  ``round32``: values rounded to float32 (what
    the device is handed); False keeps the float64 forward's own, for autograd."""
    G, NF, NC, F = inp["G"], inp["NF"], inp["NC"], inp["F"]
    gen = torch.Generator().manual_seed(seed)
    NS, NT = G * NF, G * NC
    widths = {0: [], 1: [NS], 4: [NS, NT, NT, NS]}[v.npend]
    b = dict(G=G, NF=NF, NC=NC, F=F)
    b["pend"] = [r(F, n, scale=0.3, gen=gen) for n in widths]
    b["gu_up"], b["gu"] = r(F, G, gen=gen), r(F, G, gen=gen)
    b["g_xs"], b["g_xt"], b["gxt_in"] = r(F, NS, gen=gen), r(F, NT, gen=gen), r(F, NT, gen=gen)
    b["dgamma"], b["dbeta"] = r(F, gen=gen), r(F, gen=gen)
    for k in ("gW1", "gW2", "W1", "W2", "Wt2", "gamma"):
        b[k] = inp[k]
    b["w"] = inp["gw"]
    b["V"], b["gZ"], b["Z"], b["Yp"], b["mu"], b["var"] = (fwd[k] for k in
                                                           ("gV", "gZ", "Z", "Yp", "mu", "var"))
    b["rms"] = (fwd["y1"], fwd["r1"], fwd["r2"]) if inp["gw"] is not None else None
    if round32:
        for k, t in b.items():
            if isinstance(t, torch.Tensor):
                b[k] = f32(t)
        b["pend"] = [f32(t) for t in b["pend"]]
        if b["rms"] is not None:
            b["rms"] = tuple(f32(t) for t in b["rms"])
    return b


def rms2_dwp(dY, X, w, saved):
    """EmuBackend.rms2_bwd's weight gradient before its sum over the graphs
    (the fused op's dwp [F][G])."""
    Y1, r1, r2 = saved
    r1, r2 = r1.reshape(1, -1), r2.reshape(1, -1)
    dxn = dY * w[:, None]
    d1 = r2 * dxn - Y1 * (r2 ** 3) * (dxn * Y1).sum(0, keepdim=True) / X.shape[0]
    return dY * Y1 * r2 + d1 * X * r1


def ref_class_bwd(binp, dtype=torch.float64, mutant=None, ncu=256):
    """The reference of target_class_bwd -> dict of every output (``dw`` =
    dwp summed over the graphs, as global_bwd accumulates it)."""
    be = EmuBackend(dtype)
    b = {k: _cast(t, dtype) for k, t in binp.items()}
    G, NF, NC, F = b["G"], b["NF"], b["NC"], b["F"]
    pend = b["pend"][:-1] if mutant == "pending_table_left_out" else b["pend"]
    dY = b["gu_up"].clone()
    be.graph_reduce_multi(pend, G, dY)
    w, rms = b["w"], b["rms"]
    if rms is not None:
        rms = (rms[0], rms[1].reshape(1, -1), rms[2].reshape(1, -1))
    dw = be.zeros(F) if w is not None else None
    gu, g_xs, g_xt, gxt_in = b["gu"], b["g_xs"], b["g_xt"], b["gxt_in"]
    s1, s2 = (1.0 / NC, 1.0 / NF) if mutant == "mean_scales_swapped" else (1.0 / NF, 1.0 / NC)
    gV, gdZ = be.global_bwd(dY, b["V"], w, rms, RMS_EPS, dw, b["gZ"], b["gW1"], b["gW2"], gu, g_xs,
                            s1, g_xt, s2)
    g_agg, gu_t = be.empty(2 * F, G * NC), be.empty(F, G * NC)
    dg, db = b["dgamma"], b["dbeta"]
    dYp, dZ = be.mlp_bwd(g_xt, b["Z"], b["W1"], b["W2"], 4 * F,
                         bn=(b["Yp"], b["mu"], b["var"], b["gamma"], BN_EPS, dg, db),
                         outs=[(gxt_in, F, True), (g_agg, 2 * F, False), (gu_t, F, False)])
    g_hsum = be.lin_t(b["Wt2"], 0, 2 * F, g_agg)
    out = dict(gV=gV, gdZ=gdZ, gu=gu, g_xs=g_xs, g_xt=g_xt, dgamma=dg, dbeta=db, dYp=dYp, dZ=dZ,
               gxt_in=gxt_in, g_agg=g_agg, gu_t=gu_t, g_hsum=g_hsum)
    if w is not None:
        out["dwp"], out["dw"] = rms2_dwp(dY, b["V"], w, rms), dw
    if mutant == "second_unit_skipped":
        cols = unit_columns(G, NC, CB_CLS, ncu)
        for k in BWD_CLASS_OUTS:
            out[k] = out[k].clone()
            out[k][:, cols] = 0
    return out


# ------------------------------------------------------------------ SModel's node MLP
def moments_of(M):
    """[C, N, n] messages -> source_fwd's mom [4, C, N] = (mean, c2, c3, c4)."""
    mean = M.mean(2)
    dd = M - mean[..., None]
    return torch.stack([mean, (dd ** 2).mean(2), (dd ** 3).mean(2), (dd ** 4).mean(2)])


def moment_rows(mom):
    """The MLP's input rows [mean; std; skew; kurt] (gnn.py:140-151, source_fwd's hs)."""
    mean, c2, c3, c4 = mom
    var = torch.where(c2 > 0, c2, 0.01 * c2)
    std = torch.sqrt(var + 1e-6)
    return torch.cat([mean, std, c3 / std ** 3, c4 / std ** 4])


def bn_part_of(dY, Yp, mu, var, eps=BN_EPS):
    """pfsgnn_target_bwd's bn_part [ceil(N / 64)][32]: per 64-column block sum dY
    in 0..O, sum dY * xhat in 16..16+O."""
    O, N = dY.shape
    xh = (Yp - mu[:, None]) / torch.sqrt(var[:, None] + eps)
    nb = (N + 63) // 64
    pad = nb * 64 - N
    part = torch.zeros(nb, 32, dtype=dY.dtype)
    part[:, :O] = torch.nn.functional.pad(dY, (0, pad)).reshape(O, nb, 64).sum(2).t()
    part[:, 16:16 + O] = torch.nn.functional.pad(dY * xh, (0, pad)).reshape(O, nb, 64).sum(2).t()
    return part


MLP_SHAPES = [(10, 38 * 64 + 26, 2), (10, 37, 1), (8, 38 * 64 + 26, 2), (8, 37, 1)]   # (F, N, G)
NMSG = 5     # messages per fiber behind the moments
# (nepi 1 and 2, nk 20 and 40, col0 0 and F, b None and given): [(col0 in F, nk, with b)]
EPI_FORMS = {"one": [(0, 20, True)], "two": [(1, 40, False), (0, 20, True)]}


def smodel_inputs(F, N, G, seed):
    """SModel node_mlp_2 ([F, 8F, F] -> 10F -> F + BatchNorm) over N fibers of G
    graphs: inputs of mlp_fwd_epi and, with the forward's saved tensors, of
    mlp_bwd(bn_part=, mom_coef=)."""
    gen = torch.Generator().manual_seed(seed)
    K = H = 10 * F
    i = dict(F=F, N=N, G=G)
    # (messages spread over [-1, 1] + noise: c2 stays well above 0, so the
    # coefficients' 1 / std^5 does not let a few fibers set the scale of all)
    M = r(2 * F, N, NMSG, scale=0.3, gen=gen) + torch.linspace(-1, 1, NMSG, dtype=torch.float64)
    i["x"], i["M"], i["u"] = r(F, N, gen=gen), M, r(F, G, gen=gen)
    i["W1"], i["b1"] = r(H, K, scale=0.2, gen=gen), r(H, scale=0.3, gen=gen)
    i["W2"], i["b2"] = r(F, H, scale=0.2, gen=gen), r(F, gen=gen)
    i["gamma"], i["beta"] = r(F, gen=gen) * 0.2 + 1, r(F, gen=gen) * 0.1
    i["rm"], i["rv"] = r(F, gen=gen) * 0.1, r(F, gen=gen).abs() + 0.5
    i["Wa"], i["ba"] = r(40, 4 * F, scale=0.3, gen=gen), r(40, gen=gen)
    i["Wb"], i["bb"] = r(40, 4 * F, scale=0.3, gen=gen), r(40, gen=gen)
    i["dY"], i["g_x"] = r(F, N, gen=gen), r(F, N, gen=gen)
    i["dgamma"], i["dbeta"] = r(F, gen=gen), r(F, gen=gen)
    i = {k: f32(t) if isinstance(t, torch.Tensor) else t for k, t in i.items()}
    i["mom"] = f32(moments_of(i["M"]))
    i["hs"] = f32(moment_rows(i["mom"]))
    return i


def smodel_segs(i, conv=lambda t: t):
    F = i["F"]
    return [(conv(i["x"]), 0, False), (conv(i["hs"]), F, False), (conv(i["u"]), 9 * F, True)]


def epi_maps(i, form, conv=lambda t: t):
    F = i["F"]
    return [(conv(i["Wa" if k == 0 else "Wb"]), c * F, nk, conv(i["ba" if k == 0 else "bb"]) if b else None)
            for k, (c, nk, b) in enumerate(EPI_FORMS[form])]


def ref_mlp_fwd_epi(i, form, dtype=torch.float64, given_rv=True):
    be = EmuBackend(dtype)
    c = {k: _cast(t, dtype) for k, t in i.items()}
    rm, rv = (c["rm"], c["rv"]) if given_rv else (None, None)
    Y, Z, Yp, mu, var, maps = be.mlp_fwd_epi(smodel_segs(c), c["N"], c["W1"], c["b1"], c["W2"], c["b2"],
                                             (c["gamma"], c["beta"], rm, rv, BN_MOM, BN_EPS),
                                             epi_maps(c, form))
    out = dict(Y=Y, Z=Z, Yp=Yp, mu=mu, var=var, **{f"map{k}": m for k, m in enumerate(maps)})
    if given_rv:
        out["rm"], out["rv"] = rm, rv
    return out


def mlp_bwd_pre_inputs(i, round32=True):
    """smodel_inputs + the float64 forward's saved tensors and the synthetic
    BatchNorm partials."""
    f = ref_mlp_fwd_epi(i, "one", given_rv=False)
    b = dict(i)
    for k in ("Z", "Yp", "mu", "var"):
        b[k] = f32(f[k]) if round32 else f[k]
    b["bn_part"] = bn_part_of(b["dY"], b["Yp"], b["mu"], b["var"])
    if round32:
        b["bn_part"] = f32(b["bn_part"])
    return b


def ref_mlp_bwd_pre(binp, dtype=torch.float64, bn_part=True, mom=True):
    """mlp_bwd(bn_part=, mom_coef=(mom, coef, F, NMSG)) with outs = [(g_x, F,
    add), (None, 8F), (gu, F)] -> dict(dYp, dZ, dgamma, dbeta, dX0, dX2, coef)."""
    be = EmuBackend(dtype)
    b = {k: _cast(t, dtype) for k, t in binp.items()}
    F, N = b["F"], b["N"]
    g_x, gu, coef = b["g_x"], be.empty(F, N), be.empty(4, 2 * F, N)
    gst = be.empty(8 * F, N)
    dg, db = b["dgamma"], b["dbeta"]
    kw = {}
    if bn_part:
        kw["bn_part"] = b["bn_part"]
    if mom:
        kw["mom_coef"] = (b["mom"], coef, F, NMSG)
    dYp, dZ = be.mlp_bwd(b["dY"], b["Z"], b["W1"], b["W2"], 10 * F,
                         bn=(b["Yp"], b["mu"], b["var"], b["gamma"], BN_EPS, dg, db),
                         outs=[(g_x, F, True), (None if mom else gst, 8 * F, False), (gu, F, False)],
                         **kw)
    out = dict(dYp=dYp, dZ=dZ, dgamma=dg, dbeta=db, dX0=g_x, dX2=gu)
    if mom:
        out["coef"] = coef
    else:
        out["gst"] = gst
    return out


# ------------------------------------------------------------------ bounds
# rtol of every output: that of the existing test of the unfused op that makes it
#   test_gpu_ops.test_edge_ops_node_epilogues (hsum, agg; g_xs(T): the partials) 2e-4 / 5e-4
#   test_gpu_ops.test_mlp_fused (MLP + BatchNorm, forward and backward)          5e-5
#   test_gpu_ops.test_global_fused (GlobalModel)                       2e-4 forward, 1e-3 backward
#   test_gpu_ops.test_node_ops (lin / lin_t: Pt, Qt, the maps, g_hsum 2e-4; moment_coef 1e-3)
RTOL = {}
RTOL.update({"fwd." + k: 2e-4 for k in ("hsum", "agg", "means", "gZ", "gV", "u", "y1", "r1", "r2",
                                        "Pt", "Qt")})
RTOL.update({"fwd." + k: 5e-5 for k in ("Z", "Yp", "xt", "mu", "var", "rm", "rv")})
RTOL.update({"bwd." + k: 1e-3 for k in ("gV", "gdZ", "dwp", "dw", "gu", "g_xs", "g_xt")})
RTOL.update({"bwd." + k: 5e-5 for k in ("dgamma", "dbeta", "dYp", "dZ", "gxt_in", "g_agg", "gu_t")})
RTOL["bwd.g_hsum"] = 2e-4
RTOL.update({"epi." + k: 5e-5 for k in ("Y", "Z", "Yp", "mu", "var", "rm", "rv")})
RTOL.update({"epi.map0": 2e-4, "epi.map1": 2e-4})
RTOL.update({"pre." + k: 5e-5 for k in ("dYp", "dZ", "dgamma", "dbeta", "dX0", "dX2", "gst")})
RTOL.update({"pre.coef": 1e-3, "pre.part": 5e-4})


def bounds(op, r64, r32):
    """-> {output: max(rtol x max|ref64|, 16 x max|ref32 - ref64|)}; dbeta with
    test_mlp_fused's allowance for a cancelling sum, 1e-6 x max_c sum|dYp[c]|.
    Nothing here comes from the code under test."""
    out = {}
    for k, a in r64.items():
        scale = a.abs().max().item() if a.numel() else 0.0
        e32 = (r32[k].double() - a).abs().max().item() if a.numel() else 0.0
        bnd = RTOL[f"{op}.{k}"] * scale
        if k == "dbeta":
            bnd += 1e-6 * r64["dYp"].abs().sum(1).max().item()
        out[k] = max(bnd, 16.0 * e32)
    return out


def max_err(a, b):
    return (a.double() - b).abs().max().item() if b.numel() else 0.0


# ------------------------------------------------------------------ shared references
_REFS = {}


def case_seed(case, idx):
    return 5000 + 10 * CASES.index(case) + idx


def reference(case, idx, v, ncu=256):
    """-> dict(shape, geo, inp, fwd64, fwd32, binp, bwd64, bwd32) of a case,
    computed once per process and left unchanged (bwd* None where the backward
    refuses the shape)."""
    key = (case, idx, v, ncu)
    if key not in _REFS:
        G, NF, NC, F = shape = case_shapes(case, ncu)[idx]
        inp = block_inputs(G, NF, NC, F, v, case_seed(case, idx))
        R = dict(shape=shape, geo=unit_geometry(G, NF, NC, ncu), inp=inp,
                 fwd64=ref_block_fwd(inp), fwd32=ref_block_fwd(inp, torch.float32),
                 binp=None, bwd64=None, bwd32=None)
        if R["geo"]["bwd"] is not None:
            R["binp"] = class_bwd_inputs(inp, R["fwd64"], v, case_seed(case, idx) + 1)
            R["bwd64"] = ref_class_bwd(R["binp"])
            R["bwd32"] = ref_class_bwd(R["binp"], torch.float32)
        _REFS[key] = R
    return _REFS[key]
