"""Op-level parity of the dense node linear algebra of csrc/pfsgnn_node.hip --
k_gemm / k_gemm_multi (pfsgnn_lin, _lin_t, _lin_cat, _lin_gather,
_gemm_multi), k_wgrad / k_wgrad_multi (pfsgnn_wgrad, _wgrad_cat,
_wgrad_cat_part, _wgrad_multi, the deferred pass), k_reduce_rows /
k_reduce_seg (pfsgnn_reduce_batch) and the small per-graph / per-channel ops --
against the references of tests/node_linalg_case.py (EmuBackend in float64,
held to autograd by tests/test_node_linalg_ref.py), on the smallest shapes
that reach each instantiation and each branch of the launch geometry.

Exact inputs (multiples of 1/8, every sum exact in every order): the device
equals the reference bit for bit on `mfma`, `mfma32` and `bf16x6`.  Where the
op ends in IEEE operations on an exact value (lin_t's * lrelu'(Z), then the
accumulation; lin's and lin_cat's accumulation onto a Y0 that is off the grid)
the float32 reference restates them and equality is still demanded.  The
accumulation after a product may be contracted into one fused multiply-add by
the compiler, so one form (lin_t with Z and add, on a grid Y0) is accepted in
either rounding.

Random inputs: per block -- each input block's columns of dW, db, each job,
each output tensor -- err <= max(rtol * max|ref64|, 16 * max|ref32 - ref64|),
rtol 1e-5 for the fp32 forms and 5e-5 for the bf16x3 weight gradients
(test_gpu_ops.test_node_x3_policy's figures), 2e-4 / 1e-3 for the small ops.
No bar is raised for any case.  With PFSGNN_NODE_LINALG_ERRORS=<file> the
module writes every observed maximum beside its bound
(profiles/node_linalg_errors.txt).

Every output and every partial buffer is a view into a larger buffer filled
with a sentinel; outputs that are not accumulated start as NaN.

What these tests found when first run: the plan's (2, 16), (4, 16) and (8, 16)
weight-gradient shapes had no kernel (refused, in a batch after other groups
had launched); pfsgnn_gemm_multi and pfsgnn_reduce_batch checked a later
launch's jobs after the earlier launches had run.  The refusal tests hold the
fixed order: a refused call writes nothing.  The partial arena of
pfsgnn_wgrad_multi is checked against the jobs' own sizes, which
pfsgnn_wgrad_multi_bytes exceeds by its padding, so the refusal is tested one
byte below the jobs' sizes, not one byte below that figure.
"""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import node_linalg_case as nl  # noqa: E402
from test_gpu_class_side_ops import tamper  # noqa: E402
from test_gpu_ops import cpu, cuda  # noqa: E402

_SET = [k for k in nl.PLAN_KNOBS if os.environ.get(k)]
if _SET:
    pytest.skip(f"{', '.join(_SET)} set: the weight-gradient plan differs from the one restated in "
                "tests/node_linalg_case.py", allow_module_level=True)

SENT = nl.SENT
PAD = 64                 # guard floats before and after a buffer (keeps 256-byte alignment)
EXACT_PATHS = ("mfma", "mfma32", "bf16x6")
RANDOM_PATHS = ("mfma32", "mfma")
_TABLE = {}              # (case, path, output) -> (err, bound)
_GUARDS = []


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def hb():
    from pfsgnn.native import HipBackend

    class NanFilled(HipBackend):
        def empty(self, *shape):
            return torch.full(shape, float("nan"), dtype=torch.float32, device=self.device)

    return NanFilled()


@pytest.fixture(scope="module", autouse=True)
def error_table():
    from pfsgnn import native
    yield
    path = os.environ.get("PFSGNN_NODE_LINALG_ERRORS")
    if path and _TABLE:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_node_linalg.py: max |hip - ref64| of every block beside its bound\n"
                    "# max(rtol * max|ref64|, 16 * max|ref32 - ref64|); exact inputs: bound 0\n"
                    "# case path output error bound\n")
            for (case, path_, name), (err, bnd) in sorted(_TABLE.items()):
                f.write(f"{case} {path_} {name} {err:.3e} {bnd:.3e}\n")
    assert native.sync_faults() == 0


@pytest.fixture
def edge_path():
    import pfsgnn
    prev = pfsgnn.get_edge_path()
    yield pfsgnn.set_edge_path
    pfsgnn.set_edge_path(prev)


def lib():
    from pfsgnn import native
    return native.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ buffers
def guarded(shape, init=None, off=0):
    """A contiguous view ``off`` floats into a sentinel-filled buffer, holding
    ``init`` (a CPU tensor) or NaN; the bands around it are checked by guards_ok."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((PAD + off + n + PAD,), SENT, dtype=torch.float32, device="cuda")
    view = flat[PAD + off:PAD + off + n].view(*shape)
    if init is None:
        view.fill_(float("nan"))
    else:
        view.copy_(init.to(torch.float32))
    _GUARDS.append((flat, PAD + off, n))
    return view


def guards_ok():
    """Every guard band made since the last call still holds the sentinel."""
    torch.cuda.synchronize()
    ok = all(bool((f[:a] == SENT).all()) and bool((f[a + n:] == SENT).all()) for f, a, n in _GUARDS)
    _GUARDS.clear()
    return ok


def record(case, path, name, err, bnd):
    key = (case, path, name)
    old = _TABLE.get(key)
    if old is None or err * max(old[1], 1e-300) > old[0] * max(bnd, 1e-300):
        _TABLE[key] = (err, bnd)
    print(f"{case} {path} {name}: err {err:.3e} bound {bnd:.3e}")


def judge(case, path, got, r64, r32, rtol, bad):
    """One block against its bound (exact: r32 None, bound 0)."""
    for k, ref in r64.items():
        v = cpu(got[k])
        assert v.shape == ref.shape, (case, k, v.shape, ref.shape)
        assert bool(torch.isfinite(v).all()), f"{case} {k}: not finite (unwritten?)"
        err = nl.max_err(v, ref)
        bnd = 0.0 if r32 is None else nl.bound(ref, r32[k], rtol[k] if isinstance(rtol, dict) else rtol)
        record(case, path, k, err, bnd)
        if not err <= bnd:
            bad.append(f"{path} {k}: err {err:.3e} > bound {bnd:.3e}")


# ------------------------------------------------------------------ GEMM
def hip_gemm(hb, c, i, act_in):
    Mo, _ = nl.gemm_dims(c)
    out = guarded((Mo, c.N), i["Y0"] if c.add else None)
    Y = nl.run_gemm(hb, c, i, act_in, cuda, out=out)
    assert Y is out and guards_ok(), f"{c.name}: written outside the output"
    return Y


@pytest.mark.parametrize("c", nl.GEMM_CASES, ids=lambda c: c.name)
def test_gemm(hb, edge_path, c):
    nl.assert_reaches_branch(c)
    bad = []
    i = nl.gemm_inputs(c, "exact")
    r32 = nl.ref_gemm(c, i, False, torch.float32).double()
    for path in EXACT_PATHS:
        edge_path(path)
        Y = hip_gemm(hb, c, i, False)
        assert torch.equal(Y, hip_gemm(hb, c, i, False)), "not reproducible"
        got = cpu(Y)
        if c.z and c.add:      # Y0 + pre * lrelu'(Z): two roundings, or one (a contracted fma)
            pre = nl.ref_gemm(c._replace(z=False, add=False), i, False)
            from emu_backend import dlrelu
            fma = (i["Y0"] + pre * dlrelu(i["Z"]).float().double()).float().double()
            err = torch.minimum((got - r32).abs(), (got - fma).abs()).max().item()
        else:
            err = nl.max_err(got, r32)
        assert bool(torch.isfinite(got).all())
        record(c.name, path, "exact.Y", err, 0.0)
        if err != 0.0:
            bad.append(f"{path} exact: {err:.3e}")
    edge_path("mfma")
    i = nl.gemm_inputs(c, "random")
    for act in (False, True):
        if c.op == "lin_t" and act:
            continue
        r64, r32 = nl.ref_gemm(c, i, act), nl.ref_gemm(c, i, act, torch.float32)
        Y = hip_gemm(hb, c, i, act)
        assert torch.equal(Y, hip_gemm(hb, c, i, act)), "not reproducible"
        judge(c.name, "mfma", {f"Y.act{int(act)}": Y}, {f"Y.act{int(act)}": r64}, {f"Y.act{int(act)}": r32},
              nl.RTOL_FP32, bad)
    assert not bad, f"{c.name}: " + "; ".join(bad)


def test_gemm_refusals(hb):
    """Refused by error text before any launch: the output keeps its sentinel."""
    N = 12
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    out = guarded((177, N), torch.full((177, N), SENT))

    def refused(match, fn):
        with pytest.raises(RuntimeError, match=match):
            fn()
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), f"{match}: output written by a refused call"

    refused("input width > 160", lambda: hb.lin(z(10, 161), 0, 161, z(161, N), out=out[:10]))
    refused("output width > 176", lambda: hb.lin(z(177, 8), 0, 8, z(8, N), out=out))
    refused("input width > 160", lambda: hb.lin_t(z(161, 10), 0, 10, z(161, N), out=out[:10]))
    refused("output width > 176", lambda: hb.lin_t(z(8, 177), 0, 177, z(8, N), out=out))
    refused("bad segment list",
            lambda: hb.lin_cat(z(10, 10), [(z(2, N), 2 * k, False) for k in range(5)], N, out=out[:10]))
    refused("bad segment list",
            lambda: hb.lin_cat(z(10, 10), [(z(2, 3), 0, True), (z(2, 4), 2, True)], N, out=out[:10]))

    def bad_npg(name, args):
        if name == "pfsgnn_lin_cat":
            args[3][0].per_graph = 5          # 12 % 5 != 0

    with tamper(bad_npg):
        refused("bad segment list", lambda: hb.lin_cat(z(10, 10), [(z(2, 3), 0, True)], N, out=out[:10]))
    assert guards_ok()


# ------------------------------------------------------------------ lin_gather
@pytest.mark.parametrize("c", nl.GATHER_CASES, ids=lambda c: c.name)
def test_lin_gather(hb, c):
    dev = lambda t: t.cuda() if t.dtype == torch.int32 else cuda(t)  # noqa: E731
    if c.refused:
        with pytest.raises(RuntimeError, match="gathers need M, K <= 64"):
            nl.run_gather(hb, c, nl.gather_inputs(c, "exact"), dev)
        return
    assert nl.gemm_mt(c.M) <= 4 and nl.gemm_ksm(c.K) <= 16 or not c.ngather   # (k_gemm's GATH forms)
    bad = []
    i = nl.gather_inputs(c, "exact")
    Y = nl.run_gather(hb, c, i, dev)
    assert torch.equal(Y, nl.run_gather(hb, c, i, dev)), "not reproducible"
    judge(c.name, "mfma", {"exact.Y": Y}, {"exact.Y": nl.ref_gather(c, i)}, None, 0, bad)
    i = nl.gather_inputs(c, "random")
    Y = nl.run_gather(hb, c, i, dev)
    assert torch.equal(Y, nl.run_gather(hb, c, i, dev))
    judge(c.name, "mfma", {"Y": Y}, {"Y": nl.ref_gather(c, i)}, {"Y": nl.ref_gather(c, i, torch.float32)},
          nl.RTOL_FP32, bad)
    # the entry point's other arguments, which the wrapper fixes: bscale, act_in, add into Y
    gen = torch.Generator().manual_seed(77)
    Y0 = nl.rnd(gen, c.M, c.N)
    out = guarded((c.M, c.N), Y0)

    def hook(name, args):
        if name == "pfsgnn_lin_gather":
            args[7], args[8], args[9], args[10] = 2.0, 1, out.data_ptr(), 1

    with tamper(hook):
        nl.run_gather(hb, c, i, dev)
    assert guards_ok()
    refs = []
    for dt in (torch.float64, torch.float32):
        from emu_backend import EmuBackend
        be = EmuBackend(dt)
        R = be.lin(i["W"].to(dt), 1, c.K, i["X"].to(dt), b=i["b"].to(dt), act_in=True, bscale=2.0)
        for g, idx in zip(i["G"], i["idx"]):
            R = R + g.to(dt)[:, idx.long()]
        refs.append(Y0.to(dt) + R)
    judge(c.name, "mfma", {"Y.tampered": out}, {"Y.tampered": refs[0]}, {"Y.tampered": refs[1]},
          nl.RTOL_FP32, bad)
    assert not bad, f"{c.name}: " + "; ".join(bad)


# ------------------------------------------------------------------ gemm_multi
def single_launches(hb, ops):
    outs = []
    for op in ops:
        if op[0] == "cat":
            _, W, segs, N, b = op
            outs.append(hb.lin_cat(W, segs, N, b=b))
        else:
            _, W, col0, ncol, dY, Y, add = op
            outs.append(hb.lin_t(W, col0, ncol, dY, out=Y, add=add))
    return outs


@pytest.mark.parametrize("c", nl.BATCH_CASES, ids=lambda c: c.name)
def test_gemm_multi(hb, c):
    nl.assert_reaches_branch(c)
    bad = []
    for kind in ("exact", "random"):
        i = nl.batch_inputs(c, kind)
        got = hb.linear_batch(nl.batch_ops(c, i, cuda))
        one = single_launches(hb, nl.batch_ops(c, i, cuda))
        again = hb.linear_batch(nl.batch_ops(c, i, cuda))
        assert all(torch.equal(a, b) for a, b in zip(got, again)), "not reproducible"
        torch.cuda.synchronize()
        r64 = nl.ref_batch(c, i)
        r32 = nl.ref_batch(c, i, torch.float32) if kind == "random" else None
        for j, (a, b) in enumerate(zip(got, one)):
            assert torch.equal(a, b), f"job {j} ({c.jobs[j][0]}) differs from its single launch"
        names = [f"{kind}.job{j}" for j in range(len(got))]
        judge(c.name, "mfma", dict(zip(names, got)), dict(zip(names, r64)),
              None if r32 is None else dict(zip(names, r32)), nl.RTOL_FP32, bad)
    assert not bad, f"{c.name}: " + "; ".join(bad)


def test_gemm_multi_refusals(hb):
    """A job wider than the batched kernels refuses the whole batch before any
    launch, also when it sits in a later launch of the batch."""
    N = 10
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    outs = [guarded((8, N), torch.full((8, N), SENT)) for _ in range(4)]
    ok = [("t", z(12, 8), 0, 8, z(12, N), o, False) for o in outs]
    for wide in (("t", z(41, 8), 0, 8, z(41, N), None, False),        # Ki = 41
                 ("t", z(12, 65), 0, 65, z(12, N), None, False),      # M = 65
                 ("cat", z(8, 41), [(z(41, N), 0, False)], N, None),
                 ("cat", z(65, 8), [(z(8, N), 0, False)], N, None)):
        with pytest.raises(RuntimeError, match="job wider than the batched kernels"):
            hb.linear_batch(ok + [wide])
        torch.cuda.synchronize()
        assert all(bool((o == SENT).all()) for o in outs), "a refused batch launched its first jobs"
    hb.linear_batch(ok)
    torch.cuda.synchronize()
    assert all(bool((o == 0).all()) for o in outs) and guards_ok()


# ------------------------------------------------------------------ weight gradients
def wg_device_inputs(c, i):
    """dY and the input blocks on the device, laid out as the case asks: one
    float into an aligned buffer for the misaligned ones."""
    dY = guarded((c.M, c.N), i["dY"], off=1 if c.misalign == "dY" else 0)
    X, first_bc = [], True
    for n, (x, (_, k)) in enumerate(zip(i["X"], c.blocks)):
        off = 0
        if c.misalign == "seg" and n == 0:
            off = 1
        if c.misalign == "bc" and k == "g" and first_bc:
            off, first_bc = 1, False
        X.append(guarded(tuple(x.shape), x, off=off))
    assert (dY.data_ptr() % 16 != 0) == (c.misalign == "dY")
    return dY, X


def hip_wg(hb, c, i, act_in, run=None):
    lddw, _ = nl.wg_layout(c)
    dY, X = wg_device_inputs(c, i)
    dW = guarded((c.M, lddw), i["dW0"])
    db = guarded((c.M,), i["db0"]) if c.db else None
    out = (run or nl.run_wg)(hb, c, i, act_in, cuda, dW=dW, db=db, X=X, dY=dY)
    assert guards_ok(), f"{c.name}: written outside dW / db"
    return out


def wg_rtol(c, path):
    p = nl.wg_plan(c)
    return nl.RTOL_X3 if nl.wg_x3_for(p["tm"], p["per"], path) else nl.RTOL_FP32


def check_wg(hb, edge_path, c, tag="", run=None, exact_paths=EXACT_PATHS):
    bad = []
    i = nl.wg_inputs(c, "exact")
    r64 = nl.ref_wg(c, i, False)
    for path in exact_paths:
        edge_path(path)
        got = hip_wg(hb, c, i, False, run)
        judge(c.name, path, {f"{tag}exact.{k}": v for k, v in got.items()},
              {f"{tag}exact.{k}": v for k, v in r64.items()}, None, 0, bad)
    i = nl.wg_inputs(c, "random")
    res = {}
    for act in (False, True):
        b64 = nl.wg_blocks_of(c, nl.ref_wg(c, i, act))
        b32 = nl.wg_blocks_of(c, nl.ref_wg(c, i, act, torch.float32))
        for path in RANDOM_PATHS:
            edge_path(path)
            got = hip_wg(hb, c, i, act, run)
            again = hip_wg(hb, c, i, act, run)
            assert all(torch.equal(got[k], again[k]) for k in got), "not reproducible"
            res[path, act] = got
            blk = nl.wg_blocks_of(c, {k: cpu(v) for k, v in got.items()})
            assert torch.equal(blk.pop("dW.rest"), b64["dW.rest"].float().double()), "gap columns of dW written"
            names = {k: f"{tag}{k}.act{int(act)}" for k in blk}
            judge(c.name, path, {names[k]: v for k, v in blk.items()}, {names[k]: b64[k] for k in blk},
                  {names[k]: b32[k] for k in blk},
                  {names[k]: nl.RTOL_FP32 if k == "db" else wg_rtol(c, path) for k in blk}, bad)   # (db: an exact
            # fp32 sum also in the bf16x3 form)
    assert not bad, f"{c.name}: " + "; ".join(bad)
    return res


@pytest.mark.parametrize("c", nl.WG_CASES, ids=lambda c: c.name)
def test_wgrad(hb, edge_path, c):
    p = nl.assert_reaches_branch(c)
    assert lib().pfsgnn_wgrad_part_bytes(c.M, nl.wg_K(c), c.N, int(c.db)) \
        == nl.wgrad_blocks(c.N) * c.M * p["K1"] * 4
    res = check_wg(hb, edge_path, c)
    # the policy, from behaviour: the two paths agree bit for bit exactly where wg_x3_for says fp32
    x3 = nl.wg_x3_for(p["tm"], p["per"], "mfma")
    for act in (False, True):
        a, b = res["mfma", act], res["mfma32", act]
        assert torch.equal(a["dW"], b["dW"]) == (not x3), (c.name, "bf16x3" if x3 else "fp32", act)
        if c.db:
            assert torch.equal(a["db"], b["db"]) or x3


def test_wgrad_refusals(hb):
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    for text, M, K, N, db in nl.WG_REFUSALS:
        dW = guarded((M, K), torch.full((M, K), SENT))
        with pytest.raises(RuntimeError, match=text):
            hb.wgrad(z(M, N), z(K, N), dW, db=z(M) if db else None)
        torch.cuda.synchronize()
        assert bool((dW == SENT).all()) and guards_ok()


# ------------------------------------------------------------------ the deferred path
def run_part_then_reduce(hb, c, i, act_in, conv, dW=None, db=None, X=None, dY=None):
    """pfsgnn_wgrad_cat_part into a private partial buffer, its descriptors checked
    against the plan, then pfsgnn_reduce_batch."""
    from pfsgnn import native
    p = nl.wg_plan(c)
    K = nl.wg_K(c)
    segs = hb._segs(nl.wg_segs(c, X), c.N)
    need = lib().pfsgnn_wgrad_part_bytes(c.M, K, c.N, int(c.db))
    part = guarded((need // 4,), None)
    red, nred = (native.Red * 5)(), ctypes.c_int(0)
    args = [dY.data_ptr(), c.M, segs, len(c.blocks), c.N, int(act_in), dW.data_ptr(), dW.shape[1],
            None if db is None else db.data_ptr(), float(c.dbscale), part.data_ptr()]
    with pytest.raises(RuntimeError, match="workspace too small"):
        native._call("pfsgnn_wgrad_cat_part", *args, p["part_bytes"] - 1, red, ctypes.byref(nred), stream())
    native._call("pfsgnn_wgrad_cat_part", *args, p["part_bytes"], red, ctypes.byref(nred), stream())
    assert nred.value == len(c.blocks) + int(c.db), "one descriptor per block and one for db"
    _, cols = nl.wg_layout(c)
    for n in range(nred.value):
        d = red[n]
        assert d.nb == p["nblk"] and d.plen == c.M * p["K1"] and d.ldp == p["K1"] and d.rows == c.M
        assert d.add == 1
        if n < len(c.blocks):
            assert d.cols == c.blocks[n][0] and d.out == dW.data_ptr() + 4 * cols[n] and d.ldo == dW.shape[1]
        else:
            assert d.cols == 1 and d.out == db.data_ptr() and abs(d.scale - c.dbscale) == 0
    native._call("pfsgnn_reduce_batch", red, nred.value, stream())
    return dict(dW=dW, db=db) if c.db else dict(dW=dW)


PART_CASES = [c for c in nl.WG_CASES if c.name in ("wg-cat4", "wg-deep-N2100", "wg-tm1-per1-N129",
                                                   "wg-bc-npg50-x3", "wg-flat-N401", "wg-misaligned-seg")]


@pytest.mark.parametrize("c", PART_CASES, ids=lambda c: c.name)
def test_wgrad_cat_part_then_reduce_batch(hb, edge_path, c):
    res = check_wg(hb, edge_path, c, tag="part:", run=run_part_then_reduce, exact_paths=("mfma",))
    i = nl.wg_inputs(c, "random")
    for (path, act), got in res.items():      # bitwise pfsgnn_wgrad_cat's
        edge_path(path)
        ref = hip_wg(hb, c, i, act)
        assert all(torch.equal(got[k], ref[k]) for k in got), (c.name, path, act)


def deferred_run(hb, jobs, inputs, act_of, deferred):
    """The jobs through HipBackend.defer_begin / defer_flush, or one wgrad_cat each
    in job order -> {target: (dW, db list)}."""
    targets, keep = {}, []
    for (c, tgt), i in zip(jobs, inputs):
        lddw, _ = nl.wg_layout(c)
        if tgt.startswith("adj"):
            if "adj" not in targets:
                targets["adj"] = guarded((c.M, 2 * lddw), torch.cat([i["dW0"], i["dW0"]], 1))
            dW = targets["adj"]
        elif tgt not in targets:
            dW = targets[tgt] = guarded((c.M, lddw), i["dW0"])
        else:
            dW = targets[tgt]
        db = guarded((c.M,), i["db0"]) if c.db else None
        keep.append((c, tgt, dW, db, cuda(i["dY"]), [cuda(x) for x in i["X"]]))
    if deferred:
        hb.defer_begin()
    for n, (c, tgt, dW, db, dY, X) in enumerate(keep):
        segs = nl.wg_segs(c, X)
        if tgt == "adj1":      # the adjacent column block of the shared dW
            segs = [(x, col + dW.shape[1] // 2, bc) for x, col, bc in segs]
        hb.wgrad_cat(dY, segs, dW, db=db, act_in=act_of(n), dbscale=c.dbscale)
    if deferred:
        hb.defer_flush()
    assert guards_ok()
    return keep


@pytest.mark.parametrize("njob", [1, 24, 25, 50])
def test_deferred_weight_gradients(hb, edge_path, njob):
    """pfsgnn_defer_begin(NULL, 0) + pfsgnn_defer_end_multi (pfsgnn_wgrad_multi's
    launches): every job bitwise its pfsgnn_wgrad_cat and inside its bound."""
    jobs = nl.defer_jobs(njob)
    bad = []
    for kind, path in (("exact", "mfma"), ("random", "mfma"), ("random", "mfma32")):
        edge_path(path)
        inputs = [nl.wg_inputs(c, kind) for c, _ in jobs]
        act_of = (lambda n: False) if kind == "exact" else (lambda n: n % 2 == 1)
        a = deferred_run(hb, jobs, inputs, act_of, True)
        b = deferred_run(hb, jobs, inputs, act_of, False)
        seen = {}
        for n, ((c, tgt, dW, db, _, _), (_, _, dW1, db1, _, _)) in enumerate(zip(a, b)):
            assert torch.equal(dW, dW1), f"job {n} ({tgt}): dW differs from wgrad_cat's"
            assert db is None or torch.equal(db, db1), f"job {n}: db differs from wgrad_cat's"
            # the reference of a shared dW: every job into it, in job order
            key = "adj" if tgt.startswith("adj") else tgt
            if key not in seen:
                refs = []
                for dt in (torch.float64, torch.float32):
                    i0 = inputs[n]
                    R = i0["dW0"].to(dt).clone() if key != "adj" else torch.cat([i0["dW0"], i0["dW0"]], 1).to(dt)
                    for m, ((c2, t2), i2) in enumerate(zip(jobs, inputs)):
                        if t2 == tgt or (key == "adj" and t2.startswith("adj")):
                            lddw, _ = nl.wg_layout(c2)
                            view = R[:, lddw:] if t2 == "adj1" else R[:, :lddw]
                            o = nl.ref_wg(c2, dict(i2, dW0=view), act_of(m), dt)
                            view.copy_(o["dW"])
                    refs.append(R)
                seen[key] = True
                rtol = max(wg_rtol(c2, path) for c2, t2 in jobs if t2 == tgt or (key == "adj" and t2.startswith("adj")))
                nm = f"{kind}.job{n}.dW"
                judge(f"defer-{njob}jobs", path, {nm: dW}, {nm: refs[0]},
                      None if kind == "exact" else {nm: refs[1]}, rtol, bad)
            if db is not None:
                i0 = inputs[n]
                r64 = nl.ref_wg(c, i0, act_of(n))["db"]
                r32 = nl.ref_wg(c, i0, act_of(n), torch.float32)["db"]
                nm = f"{kind}.job{n}.db"
                judge(f"defer-{njob}jobs", path, {nm: db}, {nm: r64}, None if kind == "exact" else {nm: r32},
                      nl.RTOL_FP32, bad)
    assert not bad, "; ".join(bad)


def test_wgrad_multi_entry_point(hb, edge_path):
    """pfsgnn_wgrad_multi itself (HipBackend only reaches its launches through
    pfsgnn_defer_end_multi): the 5-job list -- two jobs into the same dW cells, two
    into adjacent column blocks -- bitwise pfsgnn_wgrad_cat's, on both forms."""
    from pfsgnn import native
    jobs = nl.defer_jobs(5)
    for path in RANDOM_PATHS:
        edge_path(path)
        inputs = [nl.wg_inputs(c, "random") for c, _ in jobs]
        act_of = lambda n: n % 2 == 1  # noqa: E731
        hb._jobs = []                  # wgrad_cat then records its job instead of launching it
        try:
            a = deferred_run(hb, jobs, inputs, act_of, False)
            recorded = hb._jobs
        finally:
            hb._jobs = None
        arr = (native.WgJob * len(recorded))()
        for n, (job, _keep) in enumerate(recorded):
            arr[n] = job
        need = lib().pfsgnn_wgrad_multi_bytes(arr, len(recorded))
        assert need > 0
        arena = guarded((need // 4,), None)
        native._call("pfsgnn_wgrad_multi", arr, len(recorded), arena.data_ptr(), need, stream())
        assert guards_ok(), "written outside the partial arena"
        b = deferred_run(hb, jobs, inputs, act_of, False)
        for n, ((_, tgt, dW, db, _, _), (_, _, dW1, db1, _, _)) in enumerate(zip(a, b)):
            assert torch.equal(dW, dW1), f"{path} job {n} ({tgt}): dW differs from wgrad_cat's"
            assert db is None or torch.equal(db, db1), f"{path} job {n}: db differs from wgrad_cat's"
    native._call("pfsgnn_wgrad_multi", None, 0, None, 0, stream())      # no jobs: nothing to do


def test_deferred_pass_refusals(hb):
    from pfsgnn import native
    with pytest.raises(RuntimeError, match="no deferred pass is open"):
        native._call("pfsgnn_defer_end", stream())
    with pytest.raises(RuntimeError, match="no deferred pass is open"):
        native._call("pfsgnn_defer_end_multi", None, 0, None, 0, stream())
    native._call("pfsgnn_defer_begin", None, 0)
    try:
        with pytest.raises(RuntimeError, match="a deferred pass is already open"):
            native._call("pfsgnn_defer_begin", None, 0)
    finally:
        native._call("pfsgnn_defer_end", stream())
    # the partial arena: exactly the jobs' partials are taken, one byte less is refused
    jobs = nl.defer_jobs(5)
    inputs = [nl.wg_inputs(c, "exact") for c, _ in jobs]
    plans = [nl.wg_plan(c) for c, _ in jobs]
    tight = sum((p["part_bytes"] + 255) // 256 * 256 for p in plans[:-1]) + plans[-1]["part_bytes"]
    size = [0]

    def short(name, args):
        if name == "pfsgnn_defer_end_multi":
            assert lib().pfsgnn_wgrad_multi_bytes(args[0], args[1]) >= tight
            args[3] = size[0]

    size[0] = tight - 1
    with tamper(short):
        with pytest.raises(RuntimeError, match="partial arena too small"):
            deferred_run(hb, jobs, inputs, lambda n: False, True)
    _GUARDS.clear()
    size[0] = tight
    with tamper(short):
        a = deferred_run(hb, jobs, inputs, lambda n: False, True)
    b = deferred_run(hb, jobs, inputs, lambda n: False, False)
    for (_, _, dW, db, _, _), (_, _, dW1, db1, _, _) in zip(a, b):
        assert torch.equal(dW, dW1) and (db is None or torch.equal(db, db1))


# ------------------------------------------------------------------ reduce_batch
def red_array(descs):
    from pfsgnn import native
    arr = (native.Red * len(descs))()
    for n, (part, nb, plen, ldp, rows, cols, out, ldo, add, scale) in enumerate(descs):
        arr[n] = native.Red(part.data_ptr(), nb, plen, ldp, rows, cols, out.data_ptr(), ldo, add, scale)
    return arr


def hip_reduce(ds, parts, outs0):
    """One pfsgnn_reduce_batch over the descriptors; every partial buffer private
    to the call (the segment stage sums each segment into its first row in place),
    every output [rows][ldo] a sentinel buffer whose first ``cols`` columns hold
    out0 (add) or NaN."""
    from pfsgnn import native
    descs, outs = [], []
    for d, part, out0 in zip(ds, parts, outs0):
        init = torch.full((d.rows, d.ldo), SENT, dtype=torch.float64)
        init[:, :d.cols] = out0[:, :d.cols] if d.add else float("nan")
        out = guarded((d.rows, d.ldo), init)
        descs.append((guarded(tuple(part.shape), part), d.nb, d.rows * d.ldp, d.ldp, d.rows, d.cols, out,
                      d.ldo, d.add, d.scale))
        outs.append(out)
    native._call("pfsgnn_reduce_batch", red_array(descs), len(descs), stream())
    assert guards_ok(), "written outside a partial buffer or an output"
    for d, out in zip(ds, outs):
        assert bool((out[:, d.cols:] == SENT).all()), "columns between the rows of an output written"
    return outs


@pytest.mark.parametrize("name", sorted(nl.red_cases()))
def test_reduce_batch(name):
    ds = nl.red_cases()[name]
    bad = []
    for kind in ("exact", "random"):
        gen = torch.Generator().manual_seed(nl.seed_of(name) + (kind == "exact"))
        parts = [nl.red_part(gen, d, kind) for d in ds]
        outs0 = [nl.draw(kind, gen, d.rows, d.ldo) for d in ds]
        got = hip_reduce(ds, parts, outs0)
        again = hip_reduce(ds, parts, outs0)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), "not reproducible"
        worst = {}
        for n, (d, part, out0, o) in enumerate(zip(ds, parts, outs0, got)):
            r64 = nl.ref_red(d, part, out0)[:, :d.cols]
            r32 = nl.ref_red(d, part, out0, torch.float32)[:, :d.cols]
            v = cpu(o[:, :d.cols])
            assert bool(torch.isfinite(v).all()), f"descriptor {n}: unwritten output"
            err = nl.max_err(v, r64)
            bnd = 0.0 if kind == "exact" else nl.bound(r64, r32, nl.RTOL_FP32)
            if not err <= bnd:
                bad.append(f"{kind} descriptor {n} (nb {d.nb}, {d.rows}x{d.cols}): {err:.3e} > {bnd:.3e}")
            if not worst or err * max(worst["b"], 1e-300) >= worst["e"] * max(bnd, 1e-300):
                worst = dict(e=err, b=bnd)
        record(name, "-", f"{kind}.out", worst["e"], worst["b"])
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", sorted(nl.OVERLAPS))
def test_reduce_batch_overlapping_outputs(name):
    """Two reductions into the same cells never share a launch: the list's order holds."""
    from pfsgnn import native
    rects = nl.OVERLAPS[name]
    R, C = nl.OVERLAP_SHAPE
    for kind in ("exact", "random"):
        gen = torch.Generator().manual_seed(nl.seed_of(name) + (kind == "exact"))
        parts = [nl.draw(kind, gen, 3, r[2], r[3]) for r in rects]
        out0 = nl.draw(kind, gen, R, C)
        out = guarded((R, C), out0)
        flat = out.view(-1)
        descs = [(guarded(tuple(p.shape), p), 3, r[2] * r[3], r[3], r[2], r[3], flat[r[0] * C + r[1]:],
                  C * r[5], r[4], 1.0) for r, p in zip(rects, parts)]
        native._call("pfsgnn_reduce_batch", red_array(descs), len(descs), stream())
        assert guards_ok()
        r64 = nl.ref_overlap(rects, parts, out0)
        if kind == "exact":
            assert torch.equal(cpu(out), r64), name
        else:
            r32 = nl.ref_overlap(rects, [p.float() for p in parts], out0.float())
            err, bnd = nl.max_err(cpu(out), r64), nl.bound(r64, r32, nl.RTOL_FP32)
            record(f"red-overlap-{name}", "-", "out", err, bnd)
            assert err <= bnd, (name, err, bnd)


def test_reduce_batch_refusals():
    from pfsgnn import native
    ok_out = guarded((2, 3), torch.full((2, 3), SENT))
    ok = (torch.ones(2, 2, 3, device="cuda"), 2, 6, 3, 2, 3, ok_out, 3, 0, 1.0)
    for rows, cols in ((65536, 1), (1, 32768)):
        out = guarded((rows, cols), torch.full((rows, cols), SENT))
        wide = (torch.ones(1, rows, cols, device="cuda"), 1, rows * cols, cols, rows, cols, out, cols, 0, 1.0)
        # (ok twice: the second overlaps the first, so the list splits into two launches)
        for descs in ([ok, wide], [ok, ok, wide]):
            with pytest.raises(RuntimeError, match="wider than the packed descriptor"):
                native._call("pfsgnn_reduce_batch", red_array(descs), len(descs), stream())
            torch.cuda.synchronize()
            assert bool((out == SENT).all()) and bool((ok_out == SENT).all()), "a refused batch wrote"
    bad = (ok[0], 0) + ok[2:]
    with pytest.raises(RuntimeError, match="bad reduction"):
        native._call("pfsgnn_reduce_batch", red_array([ok, ok, bad]), 3, stream())
    torch.cuda.synchronize()
    assert bool((ok_out == SENT).all()), "a refused batch wrote"
    assert guards_ok()


# ------------------------------------------------------------------ small ops
@pytest.mark.parametrize("G,n", nl.SMALL_GN)
def test_small_ops(hb, G, n):
    i = nl.small_inputs(G, n)
    r64, r32 = nl.ref_small(i), nl.ref_small(i, torch.float32)
    out = lambda t: guarded(tuple(t.shape), t)  # noqa: E731  (what an op accumulates into)
    got = nl.run_small(hb, i, cuda, out)
    assert guards_ok(), "written outside an accumulated output"
    again = nl.run_small(hb, i, cuda, out)
    assert guards_ok() and set(got) == set(again) == set(r64)
    assert all(torch.equal(got[k], again[k]) for k in got), "not reproducible"
    bad = []
    judge(f"small-G{G}-n{n}", "-", got, r64, r32, {k: nl.SMALL_RTOL[k.split(".")[0]] for k in r64}, bad)
    assert not bad, "; ".join(bad)


def test_graph_reduce_multi_refuses_five_inputs(hb):
    out = guarded((4, 2), torch.full((4, 2), SENT))
    with pytest.raises(RuntimeError, match="1..4 inputs"):
        hb.graph_reduce_multi([torch.ones(4, 6, device="cuda") for _ in range(5)], 2, out)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and guards_ok()


def test_zz_no_barrier_timed_out():
    from pfsgnn import native
    assert native.sync_faults() == 0
