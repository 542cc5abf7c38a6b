"""Op-level parity of the fused class-side and node-MLP ops
(csrc/pfsgnn_mlp.hip: k_class_tail_fwd behind pfsgnn_target_block_fwd,
k_class_bwd behind pfsgnn_target_class_bwd, k_class_global_fwd behind
pfsgnn_target_global_fwd, pfsgnn_mlp_fwd_epi, pfsgnn_mlp_bwd_pre) against the
float64 reference of tests/class_side_case.py -- the unfused composition on
EmuBackend, held to autograd by tests/test_class_side_ref.py -- output by
output, on the edge paths the node level follows, on shapes built to reach
the branches whole-model parity never takes: a workgroup's second and third
unit (more units than CUs, judged by the device's own CU count), CT = 32, a
ragged last unit beside full ones, QB = 64, units without fibers, more than
32 column partials, and the unnormed / last-block / npend forms.

Bound of every output: err <= max(rtol x max|ref64|, 16 x max|ref32 - ref64|),
rtol that of the existing test of the unfused op making the same output
(class_side_case.RTOL), ref32 the same reference in float32.  With
PFSGNN_CLASS_SIDE_ERRORS=<file> the module writes the observed maxima beside
their bounds (profiles/class_side_errors.txt).

Where the wrapper of an op leaves a field of its argument struct NULL (Pt / Qt
without a next block, y1 / r1 / r2 unnormed) or fixed (npend, the workspace
size), ``tamper`` changes the entry point's arguments on their way through
native._call: sentinel buffers for the absent outputs, the refused values."""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import class_side_case as cs  # noqa: E402
from emu_backend import Dims as EDims, EmuBackend  # noqa: E402
from test_gpu_ops import cpu, cuda  # noqa: E402

SENT = -12345.5          # sentinel of buffers no kernel may write
PATHS = {10: ("mfma", "mfma32", "bf16x6"), 8: ("mfma", "mfma32"), 16: ("mfma", "mfma32")}

_TABLE = {}   # (case, path, op.output) -> (err, bound)


def fdim(case, idx):
    return cs.case_shapes(case)[idx][3]


def label(case, idx, v=None):
    return f"{case}{idx}" + ("" if v is None or case not in cs.VARIANT_CASES else ":" + cs.variant_id(v))


CASE_PARAMS = [pytest.param(case, idx, v, path, id=f"{label(case, idx, v)}-{path}")
               for case, idx, v in cs.case_list() for path in PATHS[fdim(case, idx)]]


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def hb():
    """HipBackend whose fresh buffers hold NaN: an output element the kernel
    leaves unwritten fails the finiteness check."""
    from pfsgnn.native import HipBackend

    class NanFilled(HipBackend):
        def empty(self, *shape):
            return torch.full(shape, float("nan"), dtype=torch.float32, device=self.device)

    return NanFilled()


@pytest.fixture(scope="module")
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module", autouse=True)
def error_table():
    from pfsgnn import native
    yield
    path = os.environ.get("PFSGNN_CLASS_SIDE_ERRORS")
    if path and _TABLE:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_class_side_ops.py: max |hip - ref64| of every output beside its bound\n"
                    "# max(rtol * max|ref64|, 16 * max|ref32 - ref64|)\n"
                    "# case path op.output error bound\n")
            for (case, path_, name), (err, bnd) in sorted(_TABLE.items()):
                f.write(f"{case} {path_} {name} {err:.3e} {bnd:.3e}\n")
    assert native.sync_faults() == 0


@pytest.fixture
def edge_path():
    import pfsgnn
    prev = pfsgnn.get_edge_path()
    yield pfsgnn.set_edge_path
    pfsgnn.set_edge_path(prev)


@contextlib.contextmanager
def tamper(fn):
    """Run native calls with fn(name, args) applied to the entry point's
    arguments first (a struct argument is args[i]._obj)."""
    from pfsgnn import native
    orig = native._call

    def call(name, *args):
        args = list(args)
        fn(name, args)
        return orig(name, *args)

    native._call = call
    try:
        yield
    finally:
        native._call = orig


def dev(t):
    if isinstance(t, (tuple, list)):
        return type(t)(dev(x) for x in t)
    return cuda(t) if isinstance(t, torch.Tensor) else t


def sentinel(*shape):
    return torch.full(shape, SENT, dtype=torch.float32, device="cuda")


def untouched(t):
    return bool((t == SENT).all())


def check_all(case, path, op, got, r64, r32, tag=""):
    """Every output of the reference present and within its bound; all figures
    recorded and printed before the assertion."""
    assert set(got) == set(r64), (sorted(got), sorted(r64))
    bnds = cs.bounds(op, r64, r32)
    bad = []
    for name, ref in r64.items():
        v = cpu(got[name])
        assert v.shape == ref.shape, (name, v.shape, ref.shape)
        assert bool(torch.isfinite(v).all()), f"{op}.{name}: not finite (unwritten?)"
        err, bnd = cs.max_err(v, ref), bnds[name]
        key = (case, path, f"{tag}{op}.{name}")
        old = _TABLE.get(key)
        if old is None or err * old[1] > old[0] * bnd:
            _TABLE[key] = (err, bnd)
        print(f"{case} {path} {tag}{op}.{name}: err {err:.3e} bound {bnd:.3e}")
        if not err <= bnd:
            bad.append(f"{tag}{op}.{name}: err {err:.3e} > bound {bnd:.3e}")
    assert not bad, f"{case} {path}: " + "; ".join(bad)


# ------------------------------------------------------------------ runners
def hdims(inp):
    from pfsgnn.engine import Dims
    return Dims(inp["G"], inp["NF"], inp["NC"], inp["F"])


def fwd_outputs(r, rm, rv):
    out = {k: r[k] for k in ("hsum", "agg", "Z", "Yp", "xt", "mu", "var", "means", "gZ", "gV", "u")
           if k in r}
    if rm is not None:
        out["rm"], out["rv"] = rm, rv
    if r["rms"] is not None:
        out["y1"], out["r1"], out["r2"] = r["rms"]
    if r["Pt"] is not None:
        out["Pt"], out["Qt"] = r["Pt"], r["Qt"]
    return out


def hip_block_fwd(hb, inp, tmask=None, extra=None):
    """target_block_fwd -> its outputs.  ``extra``: {struct field: buffer} handed to
    the entry point for outputs the variant does not have."""
    c = {k: dev(t) for k, t in inp.items()}
    rm, rv = c["rm"], c["rv"]

    def hook(name, args):
        if name == "pfsgnn_target_block_fwd" and extra:
            for k, t in extra.items():
                setattr(args[0]._obj, k, t.data_ptr())

    with tamper(hook):
        r = hb.target_block_fwd(hdims(inp), c["y"], c["sc"], c["sh"], c["Rs"], c["Wt1"], c["Wt2"],
                                c["bt2"], tmask, c["xt"], c["u"], c["W1"], c["b1"], c["W2"], c["b2"],
                                (c["gamma"], c["beta"], rm, rv, cs.BN_MOM, cs.BN_EPS), c["xs"],
                                c["gW1"], c["gb1"], c["gW2"], c["gb2"], c["gw"], cs.RMS_EPS, c["nxt"])
    torch.cuda.synchronize()
    return fwd_outputs(r, rm, rv)


def hip_unfused_fwd(hb, inp, agg=None):
    """target_fwd(agg=) + target_global_fwd; with ``agg`` only the latter."""
    c = {k: dev(t) for k, t in inp.items()}
    F, G, NC, NF = inp["F"], inp["G"], inp["NC"], inp["NF"]
    rm, rv = c["rm"], c["rv"]
    head = {}
    if agg is None:
        hsum, agg = hb.target_fwd(hdims(inp), c["y"], c["sc"], c["sh"], c["Rs"], c["Wt1"],
                                  agg=(c["Wt2"], c["bt2"], float(NF)))
        head = dict(hsum=hsum, agg=agg)
    hT = [(c["xt"], 0, False), (agg, F, False), (c["u"], 3 * F, True)]
    r = hb.target_global_fwd(hT, G, NC, c["W1"], c["b1"], c["W2"], c["b2"],
                             (c["gamma"], c["beta"], rm, rv, cs.BN_MOM, cs.BN_EPS), c["xs"], NF,
                             c["u"], c["gW1"], c["gb1"], c["gW2"], c["gb2"], c["gw"], cs.RMS_EPS,
                             c["nxt"])
    torch.cuda.synchronize()
    return fwd_outputs(dict(r, **head), rm, rv)


def hip_class_bwd(hb, binp, hook=None, keep=None):
    """target_class_bwd -> its outputs (dw: dwp summed over the graphs on the
    host).  ``keep``: a dict that receives the device inputs."""
    b = {k: dev(t) for k, t in binp.items()}
    F, G = binp["F"], binp["G"]
    gV, gdZ = hb.empty(F, G), hb.empty(b["gW1"].shape[0], G)
    dwp = hb.empty(F, G) if b["w"] is not None else sentinel(F, G)
    gu_up0 = b["gu_up"].clone()
    if keep is not None:
        keep.update(b, dwp=dwp)
    with tamper(hook or (lambda name, args: None)):
        r = hb.target_class_bwd(hdims(binp), b["pend"], b["gu_up"], b["V"], b["w"], b["rms"], b["gZ"],
                                b["gW1"], b["gW2"], gV, gdZ, dwp, b["gu"], b["g_xs"], b["g_xt"],
                                b["Yp"], b["mu"], b["var"], b["gamma"], cs.BN_EPS, b["dgamma"],
                                b["dbeta"], b["Z"], b["W1"], b["W2"], b["Wt2"], b["gxt_in"])
    torch.cuda.synchronize()
    assert torch.equal(b["gu_up"], gu_up0), "gu_up is read only"
    out = dict(gV=gV, gdZ=gdZ, gu=b["gu"], g_xs=b["g_xs"], g_xt=b["g_xt"], dgamma=b["dgamma"],
               dbeta=b["dbeta"], gxt_in=b["gxt_in"], **r)
    if b["w"] is not None:
        out["dwp"], out["dw"] = dwp, dwp.double().sum(1)
    else:
        assert untouched(dwp), "dwp written without the RMSNorm"
    return out


def hip_unfused_bwd(hb, binp):
    """graph_reduce_multi + global_bwd + mlp_bwd + lin_t (what the fused op replaces)."""
    b = {k: dev(t) for k, t in binp.items()}
    F, G, NF, NC = binp["F"], binp["G"], binp["NF"], binp["NC"]
    dY = b["gu_up"].clone()
    if b["pend"]:
        hb.graph_reduce_multi(b["pend"], G, dY)
    dw = torch.zeros(F, device="cuda") if b["w"] is not None else None
    gV, gdZ = hb.global_bwd(dY, b["V"], b["w"], b["rms"], cs.RMS_EPS, dw, b["gZ"], b["gW1"], b["gW2"],
                            b["gu"], b["g_xs"], 1.0 / NF, b["g_xt"], 1.0 / NC)
    g_agg, gu_t = hb.empty(2 * F, G * NC), hb.empty(F, G * NC)
    dYp, dZ = hb.mlp_bwd(b["g_xt"], b["Z"], b["W1"], b["W2"], 4 * F,
                         bn=(b["Yp"], b["mu"], b["var"], b["gamma"], cs.BN_EPS, b["dgamma"], b["dbeta"]),
                         outs=[(b["gxt_in"], F, True), (g_agg, 2 * F, False), (gu_t, F, False)])
    g_hsum = hb.lin_t(b["Wt2"], 0, 2 * F, g_agg)
    torch.cuda.synchronize()
    out = dict(gV=gV, gdZ=gdZ, gu=b["gu"], g_xs=b["g_xs"], g_xt=b["g_xt"], dgamma=b["dgamma"],
               dbeta=b["dbeta"], gxt_in=b["gxt_in"], dYp=dYp, dZ=dZ, g_agg=g_agg, gu_t=gu_t,
               g_hsum=g_hsum)
    if dw is not None:
        out["dw"] = dw
    return out


def within(case, path, op, a, b, r64, r32, tag):
    """Two device results within the reference's bounds of each other."""
    bnds = cs.bounds(op, r64, r32)
    bad = []
    for k in sorted(set(a) & set(b)):
        err = cs.max_err(cpu(a[k]), cpu(b[k]))
        print(f"{case} {path} {tag}{op}.{k}: diff {err:.3e} bound {bnds[k]:.3e}")
        if not err <= bnds[k]:
            bad.append(f"{k}: {err:.3e} > {bnds[k]:.3e}")
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------ the class side
@pytest.mark.parametrize("case,idx,v,path", CASE_PARAMS)
def test_class_side_ops(hb, ncu, edge_path, case, idx, v, path):
    from pfsgnn import native
    edge_path(path)
    R = cs.reference(case, idx, v, ncu)
    G, NF, NC, F = R["shape"]
    geo = cs.assert_reaches_branch(case, R["shape"], ncu)       # at the device's CU count
    assert geo == R["geo"] and native.edge_grid(G, NF, NC)["NFG"] == geo["BPG"]
    inp, lab = R["inp"], label(case, idx, v)
    d = hdims(inp)
    # --- target_block_fwd
    tm = hb.tmask(d) if v.tmask else None
    assert (tm is not None) == v.tmask, "the MFMA paths keep TModel's mask"
    if tm is not None:
        tm.zero_()
    extra = {}
    if not v.nxt:
        extra.update(Pt=sentinel(4 * F, G * NC), Qt=sentinel(2 * F, G * NC))
    if not v.normed:
        extra.update(y1=sentinel(F, G), r1=sentinel(G), r2=sentinel(G))
    got = hip_block_fwd(hb, inp, tmask=tm, extra=extra)
    for k, t in extra.items():
        assert untouched(t), f"{k} written in a form that has no such output"
    check_all(lab, path, "fwd", got, R["fwd64"], R["fwd32"])
    if tm is not None:   # the mask of the unfused op on the same inputs, bit for bit
        tm2 = torch.zeros_like(tm)
        c = {k: dev(inp[k]) for k in ("y", "sc", "sh", "Rs", "Wt1")}
        hs2 = hb.target_fwd(d, c["y"], c["sc"], c["sh"], c["Rs"], c["Wt1"], tmask=tm2)
        torch.cuda.synchronize()
        assert torch.equal(tm, tm2), "tmask differs from target_fwd's"
        assert cs.max_err(cpu(hs2), R["fwd64"]["hsum"]) <= cs.bounds("fwd", R["fwd64"], R["fwd32"])["hsum"]
    # --- target_global_fwd on the same inputs (agg: the reference's, rounded)
    r64 = {k: t for k, t in R["fwd64"].items() if k not in ("hsum", "agg")}
    got = hip_unfused_fwd(hb, inp, agg=cuda(R["fwd64"]["agg"]))
    check_all(lab, path, "fwd", got, r64, R["fwd32"], tag="global_fwd:")
    # --- target_class_bwd
    if geo["bwd"] is None:
        binp = cs.class_bwd_inputs(inp, R["fwd64"], v, 1)
        with pytest.raises(RuntimeError, match="more than 1024 classes"):
            hip_class_bwd(hb, binp)
        return
    got = hip_class_bwd(hb, R["binp"])
    check_all(lab, path, "bwd", got, R["bwd64"], R["bwd32"])


@pytest.mark.parametrize("path", PATHS[10])
def test_fused_against_unfused_on_the_device(hb, ncu, edge_path, path):
    edge_path(path)
    R = cs.reference("bench_like", 0, cs.FULL, ncu)
    a, b = hip_block_fwd(hb, R["inp"]), hip_unfused_fwd(hb, R["inp"])
    assert set(a) == set(b) == set(R["fwd64"])
    within("bench_like0", path, "fwd", a, b, R["fwd64"], R["fwd32"], "fused-vs-unfused:")
    a, b = hip_class_bwd(hb, R["binp"]), hip_unfused_bwd(hb, R["binp"])
    assert set(b) == set(a) - {"dwp"} and set(a) == set(R["bwd64"])
    check_all("bench_like0", path, "bwd", b, {k: R["bwd64"][k] for k in b}, R["bwd32"], tag="unfused:")
    within("bench_like0", path, "bwd", a, b, R["bwd64"], R["bwd32"], "fused-vs-unfused:")


def test_fused_ops_are_bitwise_reproducible(hb, ncu):
    R = cs.reference("many_units_ct16", 0, cs.FULL, ncu)
    for run in (lambda: hip_block_fwd(hb, R["inp"]), lambda: hip_class_bwd(hb, R["binp"])):
        a, b = run(), run()
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_barrier_forms_bitwise_equal(hb, ncu):
    from pfsgnn import native
    R = cs.reference("many_units_ct32", 0, cs.FULL, ncu)
    res = []
    try:
        for fenced in (False, True):
            native.set_grid_sync_fenced(fenced)
            res.append((hip_block_fwd(hb, R["inp"]), hip_class_bwd(hb, R["binp"])))
    finally:
        native.set_grid_sync_fenced(False)
    for a, b in zip(res[0], res[1]):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert native.sync_faults() == 0


# ------------------------------------------------------------------ refusals
def test_refusals(hb, ncu):
    """Each refused by its error text, before any launch: the in/out tensors of
    the call keep their bits."""
    R = cs.reference("ragged_tail", 0, cs.FULL, ncu)
    binp, F, G, NF, NC = R["binp"], 10, 2, 7, 17
    inout = ("gu", "g_xs", "g_xt", "dgamma", "dbeta", "gxt_in")

    def refused(match, b=binp, hook=None):
        keep = {}
        with pytest.raises(RuntimeError, match=match):
            hip_class_bwd(hb, b, hook=hook, keep=keep)
        torch.cuda.synchronize()
        for k in inout:
            assert torch.equal(keep[k], cuda(b[k])), f"{k} changed by a refused call"

    def set_npend(name, args):
        if name == "pfsgnn_target_class_bwd":
            args[0]._obj.npend = 5

    refused("at most 4 pending tables", hook=set_npend)
    bad = dict(binp, pend=[torch.zeros(F, G * (NF + 1), dtype=torch.float64)])
    assert NF + 1 not in (NF, NC)
    refused("pending tables are per fiber or per class", b=bad)
    refused("RMSNorm needs y1", b=dict(binp, rms=None))
    need = R["geo"]["bwd"]["nunits"] * (F + 32) * 4      # nunits * (F + 32) floats

    def short_ws(name, args):
        if name == "pfsgnn_target_class_bwd":
            assert args[2] >= need
            args[2] = need - 1

    refused("workspace too small", hook=short_ws)

    def exact_ws(name, args):
        if name == "pfsgnn_target_class_bwd":
            args[2] = need

    got = hip_class_bwd(hb, binp, hook=exact_ws)          # ... and exactly enough is taken
    check_all("ragged_tail0", "exact-ws", "bwd", got, R["bwd64"], R["bwd32"])
    # NC = 1025: one class past the backward's 64 units of 16
    inp = cs.block_inputs(1, 1, 1025, F, cs.FULL, 7)
    big = cs.class_bwd_inputs(inp, cs.ref_block_fwd(inp), cs.FULL, 8)
    refused("more than 1024 classes", b=big)
    # target_block_fwd: G * ceil(NC / 32) > 512
    inp = cs.block_inputs(513, 1, 1, F, cs.FULL, 9)
    assert cs.tail_ct(513, 1) == 0
    with pytest.raises(RuntimeError, match="more than 512 class units"):
        hip_block_fwd(hb, inp)
    # mlp_bwd_pre: the moment epilogue on a narrow shape (K, H <= 64)
    N, K = 37, 64
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    with pytest.raises(RuntimeError, match="the moment epilogue needs the RS form"):
        hb.mlp_bwd(z(F, N), z(K, N), z(K, K), z(F, K), K, bn=None, outs=[(z(K, N), K, False)],
                   mom_coef=(z(4, 16, N), z(4, 16, N), 0, 5))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ SModel's node MLP
MLP_PARAMS = [pytest.param(F, N, G, path, id=f"F{F}-N{N}-{path}")
              for F, N, G in cs.MLP_SHAPES for path in PATHS[F]]
_MLP = {}


def smodel(F, N, G):
    if (F, N, G) not in _MLP:
        _MLP[(F, N, G)] = cs.smodel_inputs(F, N, G, 700 + F + N)
    return _MLP[(F, N, G)]


@pytest.mark.parametrize("form", sorted(cs.EPI_FORMS))
@pytest.mark.parametrize("F,N,G,path", MLP_PARAMS)
def test_mlp_fwd_epi(hb, edge_path, F, N, G, path, form):
    edge_path(path)
    i = smodel(F, N, G)
    key = ("epi", F, N, G, form)
    if key not in _MLP:
        _MLP[key] = (cs.ref_mlp_fwd_epi(i, form), cs.ref_mlp_fwd_epi(i, form, torch.float32))
    r64, r32 = _MLP[key]
    rm, rv = cuda(i["rm"]), cuda(i["rv"])
    Y, Z, Yp, mu, var, maps = hb.mlp_fwd_epi(
        cs.smodel_segs(i, cuda), N, cuda(i["W1"]), cuda(i["b1"]), cuda(i["W2"]), cuda(i["b2"]),
        (cuda(i["gamma"]), cuda(i["beta"]), rm, rv, cs.BN_MOM, cs.BN_EPS), cs.epi_maps(i, form, cuda))
    torch.cuda.synchronize()
    got = dict(Y=Y, Z=Z, Yp=Yp, mu=mu, var=var, rm=rm, rv=rv,
               **{f"map{k}": m for k, m in enumerate(maps)})
    assert len(maps) == len(cs.EPI_FORMS[form])
    check_all(f"smodel-F{F}-N{N}:{form}", path, "epi", got, r64, r32)


def hip_mlp_bwd_pre(hb, b, bn_part, dY=None):
    """mlp_bwd(bn_part=, mom_coef=) with the None block's rows guarded: g_x, a
    sentinel of the None block's size and gu are consecutive in one buffer."""
    F, N = b["F"], b["N"]
    flat = sentinel(10 * F * N)
    g_x, guard, gu = flat[:F * N].view(F, N), flat[F * N:9 * F * N], flat[9 * F * N:].view(F, N)
    g_x.copy_(cuda(b["g_x"]))
    coef = hb.empty(4, 2 * F, N)
    dg, db = cuda(b["dgamma"]), cuda(b["dbeta"])
    dYp, dZ = hb.mlp_bwd(cuda(b["dY"]) if dY is None else dY, cuda(b["Z"]), cuda(b["W1"]),
                         cuda(b["W2"]), 10 * F,
                         bn=(cuda(b["Yp"]), cuda(b["mu"]), cuda(b["var"]), cuda(b["gamma"]), cs.BN_EPS,
                             dg, db),
                         outs=[(g_x, F, True), (None, 8 * F, False), (gu, F, False)],
                         bn_part=bn_part, mom_coef=(cuda(b["mom"]), coef, F, cs.NMSG))
    torch.cuda.synchronize()
    assert untouched(guard), "rows of the None block written"
    return dict(dYp=dYp, dZ=dZ, dgamma=dg, dbeta=db, dX0=g_x, dX2=gu, coef=coef)


@pytest.mark.parametrize("F,N,G,path", MLP_PARAMS)
def test_mlp_bwd_pre_synthetic_partials(hb, edge_path, F, N, G, path):
    edge_path(path)
    key = ("pre", F, N, G)
    if key not in _MLP:
        b = cs.mlp_bwd_pre_inputs(smodel(F, N, G))
        _MLP[key] = (b, cs.ref_mlp_bwd_pre(b), cs.ref_mlp_bwd_pre(b, torch.float32))
    b, r64, r32 = _MLP[key]
    assert b["mom"].shape == (4, 2 * F, N) and 2 * F in (16, 20)
    got = hip_mlp_bwd_pre(hb, b, cuda(b["bn_part"]))
    check_all(f"smodel-F{F}-N{N}", path, "pre", got, r64, r32)


def used_slots(part, O):
    """The slots of a [n][32] BatchNorm partial that hold sums: 0..O and 16..16+O."""
    return torch.cat([part[:, :O], part[:, 16:16 + O]], 1)


@pytest.mark.parametrize("path", PATHS[10])
def test_mlp_bwd_pre_partials_from_target_bwd(hb, ncu, edge_path, path):
    """bn_part as hb.target_bwd(bn_sums=) makes it on bench_like: the partials
    themselves, then SModel's backward on them."""
    edge_path(path)
    R = cs.reference("bench_like", 0, cs.FULL, ncu)
    G, NF, NC, F = R["shape"]
    inp, N = R["inp"], G * NF
    key = ("chain",)
    if key not in _MLP:
        b = cs.mlp_bwd_pre_inputs(cs.smodel_inputs(F, N, G, 911))
        g_hsum = cs.f32(R["bwd64"]["g_hsum"])
        refs = []
        for dt in (torch.float64, torch.float32):
            emu = EmuBackend(dt)
            t = lambda x: None if x is None else x.to(dt).clone()  # noqa: E731
            g_xs = t(b["dY"])
            _, _, part = emu.target_bwd(EDims(G, NF, NC, F), t(inp["y"]), t(inp["sc"]), t(inp["sh"]),
                                        t(inp["Rs"]), t(inp["Wt1"]), t(g_hsum), emu.zeros(2 * F, 2 * F),
                                        g_xs=g_xs, bn_sums=(t(b["Yp"]), t(b["mu"]), t(b["var"]), cs.BN_EPS))
            o = cs.ref_mlp_bwd_pre(dict(b, dY=g_xs, bn_part=part), dt)
            refs.append(dict(o, part=used_slots(part, F)))
        _MLP[key] = (b, g_hsum, refs[0], refs[1])
    b, g_hsum, r64, r32 = _MLP[key]
    g_xs = cuda(b["dY"])
    c = {k: dev(inp[k]) for k in ("y", "sc", "sh", "Rs", "Wt1")}
    _, _, part = hb.target_bwd(hdims(inp), c["y"], c["sc"], c["sh"], c["Rs"], c["Wt1"], cuda(g_hsum),
                               torch.zeros(2 * F, 2 * F, device="cuda"), g_xs=g_xs,
                               bn_sums=(cuda(b["Yp"]), cuda(b["mu"]), cuda(b["var"]), cs.BN_EPS))
    assert part.shape == ((N + 63) // 64, 32) and cs.unit_geometry(G, NF, NC, ncu)["BPG"] == 3
    got = hip_mlp_bwd_pre(hb, b, part, dY=g_xs)
    check_all("bench_like0", path, "pre", dict(got, part=used_slots(part, F)), r64, r32,
              tag="from-target_bwd:")


def test_zz_no_barrier_timed_out():
    from pfsgnn import native
    assert native.sync_faults() == 0
