"""The observing plan on the CPU: the numpy reference (tests/observing_plan_ref.py)
against train.py's own timeline and against the trim's defining properties;
``pfsgnn.train.observing_plan`` through the torch emulation of the op set (its
host restatement) against that reference; and pfsgnn_schedule_plan's ABI and
argument checks (host-only calls, no GPU).
"""
import ctypes

import numpy as np
import pytest
import torch

from harness import canonical_edges
from observing_plan_case import (NFIELDS, TOTAL_TIME, assert_branches, craft, level)
from observing_plan_ref import observing_plan_ref
from test_hard_schedule_ref import _product, emu_pfsgnn  # noqa: F401  (fixture)
from test_sparse_emu import sparse_edges

OUT = ("visits", "start", "used", "idle", "n", "completeness", "utility", "over", "worst", "cut",
       "seg_ptr", "seg_edge", "seg_start")


def _ref(vis, ei, ci, G, NF, cap=True, segments=True):
    return observing_plan_ref(vis, ei, ci, TOTAL_TIME, NFIELDS, G * NF, cap=cap, G=G,
                              segments=segments)


# ---------------------------------------------------------------- train.py's timeline
def test_timeline_is_train_py_cumsum_and_left():
    """train.py:256-261, 283-284 on a complete fiber-major graph: rounded =
    visits * class_req as [NF, NC], cumulative = cumsum(axis=1), left =
    hstack(0, cumulative[:, :-1]); target m of (fiber, class) at left + m *
    class_req."""
    G, NF, NC = 1, 17, 6
    ei = canonical_edges(G, NF, NC).numpy()
    vis, ci, _, _ = craft(ei, NF, NC, 3, first=11)         # (every class plain)
    ci[:, 1] = 1e6
    vis = np.abs(vis) % 5
    r = _ref(vis, ei, ci, G, NF, cap=False)
    assert np.array_equal(r["visits"], vis)
    class_req = ci[:, 0].astype(np.float64)
    rounded = vis.reshape(NF, NC) * class_req[None, :]
    cumulative = np.cumsum(rounded, axis=1)
    left = np.hstack([np.zeros((NF, 1)), cumulative[:, :-1]])
    assert np.array_equal(r["start"].reshape(NF, NC), left.astype(np.float32))
    assert np.array_equal(r["used"], cumulative[:, -1].astype(np.float32))
    assert np.array_equal(r["idle"], (TOTAL_TIME - cumulative[:, -1]).astype(np.float32))
    want_e, want_t = [], []
    for f in range(NF):
        for c in range(NC):
            for m in range(vis[f * NC + c]):
                want_e.append(f * NC + c)
                want_t.append(left[f, c] + m * class_req[c])
    assert r["seg_edge"].tolist() == want_e
    assert np.array_equal(r["seg_start"], np.asarray(want_t, np.float32))
    assert r["seg_ptr"][-1] == vis.sum() and (r["total"] > TOTAL_TIME).any()
    assert int(r["over"][0]) == int((cumulative[:, -1] > TOTAL_TIME).sum()) > 0
    assert (r["idle"][r["total"] > TOTAL_TIME] < 0).all()


# ---------------------------------------------------------------- the trim
def general_case(seed, G=2, NF=23, NC=13, density=0.6, dup=9):
    gen = torch.Generator().manual_seed(seed)
    return G, NF, NC, sparse_edges(G, NF, NC, density, gen, dup=dup).numpy()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_trim_properties(seed):
    G, NF, NC, ei = general_case(seed)
    vis, ci, branch, f0 = craft(ei, G * NF, G * NC, seed, first=seed)
    r = _ref(vis, ei, ci, G, NF)
    free = _ref(vis, ei, ci, G, NF, cap=False, segments=False)
    assert_branches(r, ei, vis, branch, f0, need=("rem_pos", "rem_zero", "at_cap", "level_zero",
                                                  "cap_zero", "cap_nan", "no_cap", "single_edge",
                                                  "all_equal", "inert", "negative"))
    src, tgt = ei
    w, v = r["w"], r["visits"].astype(np.int64)
    assert np.array_equal(free["visits"], w) and not free["cut"].any()
    assert (v <= w).all() and (v >= 0).all()               # no edge gains a visit
    n = np.zeros(G * NC, np.int64)
    np.add.at(n, tgt, v)
    capc = np.where(r["capc"] < 0, np.iinfo(np.int64).max, r["capc"])
    assert np.array_equal(n, np.minimum(r["S"], capc)) and np.array_equal(n, r["n"])
    assert np.array_equal(r["cut"], r["S"] - n)
    for c in np.nonzero(r["L"] >= 0)[0]:
        e = np.nonzero(tgt == c)[0]
        L, rem = level(w[e], r["capc"][c])
        assert (L, rem) == (r["L"][c], r["rem"][c])
        red = e[v[e] < w[e]]
        assert np.isin(v[red], (L, L + 1)).all()
        above = e[w[e] > L]
        above = above[np.lexsort((above, src[above]))]     # ascending (src, position)
        assert (v[above[:rem]] == L + 1).all() and (v[above[rem:]] == L).all()
        assert np.array_equal(v[e[w[e] <= L]], w[e[w[e] <= L]])
    assert (r["total"] <= free["total"]).all()             # no fiber's time grows
    assert (r["total"] < free["total"]).any() and (r["total"] > TOTAL_TIME).any()
    assert np.array_equal(r["over"], (r["total"].reshape(G, NF) > TOTAL_TIME).sum(1))
    assert r["seg_ptr"][-1] == v.sum() == r["seg_edge"].size
    # the list repeats each edge visits_e times, fiber by fiber, in (class, position) order
    assert np.array_equal(np.bincount(r["seg_edge"], minlength=v.size), v)
    assert (np.diff(src[r["seg_edge"]]) >= 0).all()
    same = np.diff(src[r["seg_edge"]]) == 0
    assert (np.diff(tgt[r["seg_edge"]])[same] >= 0).all()
    assert (np.diff(r["seg_start"].astype(np.float64))[same] > 0).all()


# ---------------------------------------------------------------- orders and forms
def _orders(G, NF, NC):
    E = G * NF * NC
    e = torch.arange(E)
    g, f, c = e // (NF * NC), (e // NC) % NF, e % NC
    return {"fiber-major": e, "canonical": torch.argsort((g * NC + c) * NF + f),
            "permutation": torch.randperm(E, generator=torch.Generator().manual_seed(11))}


def test_caller_orders_and_the_csr_form_give_the_same_plan():
    """A complete graph fiber-major, canonical and permuted: the same plan
    re-indexed (no repeated pairs, so no position decides anything).  The CSR
    form: the emulated pfsgnn_sparse_layout's arrays, walked the way the general
    kernels walk them -- a class's edges through cls_ord, a fiber's through the
    stable sort of cls_ord by fiber -- visit the edges in the definition's
    orders."""
    from emu_backend import EmuBackend
    G, NF, NC = 2, 14, 9
    ei = canonical_edges(G, NF, NC).numpy()
    vis, ci, branch, f0 = craft(ei, G * NF, G * NC, 5)
    base = _ref(vis, ei, ci, G, NF)
    assert_branches(base, ei, vis, branch, f0)
    for name, p in _orders(G, NF, NC).items():
        p = p.numpy()
        r = _ref(vis[p], ei[:, p], ci, G, NF)
        for k in ("visits", "start"):
            assert np.array_equal(r[k], base[k][p]), (name, k)
        for k in ("used", "idle", "n", "completeness", "utility", "over", "worst", "cut", "seg_ptr",
                  "seg_start"):
            assert np.array_equal(r[k], base[k], equal_nan=True), (name, k)
        assert np.array_equal(p[r["seg_edge"]], base["seg_edge"]), name
        sp = EmuBackend().sparse_layout(torch.as_tensor(ei[:, p]), G, NF, NC)
        src, tgt = ei[0][p], ei[1][p]
        user_of, cls_ord = sp.user_of.numpy(), sp.cls_ord.numpy()
        by_class = user_of[cls_ord]
        assert np.array_equal(by_class, np.lexsort((np.arange(p.size), src, tgt)))
        pord = cls_ord[np.argsort(sp.src_p.numpy()[cls_ord], kind="stable")]
        assert np.array_equal(user_of[pord], np.lexsort((np.arange(p.size), tgt, src)))
        assert np.array_equal(sp.fib_ptr.numpy(), np.searchsorted(src[user_of[pord]],
                                                                  np.arange(G * NF + 1)))


# ---------------------------------------------------------------- the host restatement
def _emu_plan(pfsgnn, ei, G, NF, NC, vis, ci, **kw):
    from pfsgnn.train import observing_plan
    data = pfsgnn.BipartiteData(torch.as_tensor(ei), torch.zeros(G * NF, 1), torch.zeros(G * NC, 2),
                                torch.zeros(ei.shape[1], 10), torch.zeros(G, 10))
    return observing_plan(data, torch.as_tensor(ci), torch.as_tensor(vis), **kw)


def _same(plan, r, fields=OUT):
    for k in fields:
        got = getattr(plan, k).numpy()
        assert got.dtype == r[k].dtype, (k, got.dtype, r[k].dtype)
        assert np.array_equal(got, r[k], equal_nan=True), k


@pytest.mark.parametrize("cap", [True, False])
def test_host_restatement_equals_the_reference(emu_pfsgnn, cap):
    from pfsgnn import config
    assert (config.TOTAL_TIME, config.NFIELDS) == (TOTAL_TIME, NFIELDS)
    G, NF, NC, ei = general_case(4)
    vis, ci, branch, f0 = craft(ei, G * NF, G * NC, 4, first=2)
    if not cap:
        vis = np.minimum(vis, 50)                          # (no 2^24 exposures to list)
    _same(_emu_plan(emu_pfsgnn, ei, G, NF, NC, vis, ci, cap=cap), _ref(vis, ei, ci, G, NF, cap=cap))
    # complete graphs, every caller order; int64 visits; segments=False
    G, NF, NC = 2, 14, 9
    ce = canonical_edges(G, NF, NC).numpy()
    vis, ci, _, _ = craft(ce, G * NF, G * NC, 6, first=5)
    if not cap:
        vis = np.minimum(vis, 50)
    for name, p in _orders(G, NF, NC).items():
        p = p.numpy()
        r = _ref(vis[p], ce[:, p], ci, G, NF, cap=cap)
        _same(_emu_plan(emu_pfsgnn, ce[:, p], G, NF, NC, vis[p].astype(np.int64), ci, cap=cap), r)
        plan = _emu_plan(emu_pfsgnn, ce[:, p], G, NF, NC, vis[p], ci, cap=cap, segments=False)
        assert plan.seg_edge is None and plan.seg_start is None
        _same(plan, r, OUT[:11])
    # off the 2^-20 grid the restatement sums in the definition's order too
    ci[:, 0] += np.float32(0.3)
    _same(_emu_plan(emu_pfsgnn, ce, G, NF, NC, vis, ci, cap=cap), _ref(vis, ce, ci, G, NF, cap=cap))
    with pytest.raises(ValueError, match="integer"):
        _emu_plan(emu_pfsgnn, ce, G, NF, NC, vis.astype(np.float32), ci)
    with pytest.raises(ValueError, match="entries"):
        _emu_plan(emu_pfsgnn, ce, G, NF, NC, vis[:-1], ci)


def test_emulated_loop_plans_its_best_schedule(emu_pfsgnn):
    pfsgnn = emu_pfsgnn
    from pfsgnn.train import ObservingPlan, TrainLoop, observing_plan
    model, graph, gnn, data, ci = _product(pfsgnn, 2, 6, 4, seed=4, tscale=0.25)
    opt = pfsgnn.FusedAdam(gnn.parameters(), lr=3e-2, capturable=True)
    loop = TrainLoop(gnn, opt, data, ci, 8, [0, 20], 5.0, 0.1, 0.1, seed=40, capture=False,
                     track_hard="budget").run(7)
    best = loop.hard_best()
    assert best["epoch"] >= 0 and best["visits"].sum() > 0
    plan = loop.plan()
    assert isinstance(plan, ObservingPlan) and plan._fields == OUT
    _same(plan, _ref(best["visits"], graph.edge_index.numpy(), ci.numpy(), 2, 6))
    again = observing_plan(data, ci, best["visits"])
    for a, b in zip(plan, again):
        assert torch.equal(a, b)
    assert loop.plan(segments=False).seg_edge is None
    # the budget schedule fits every fiber, and the trim only removes visits
    assert int(plan.over.sum()) == 0 and bool((plan.idle >= 0).all())
    plain = TrainLoop(gnn, opt, data, ci, 8, [0, 20], 5.0, 0.1, 0.1, seed=40, capture=False)
    with pytest.raises(ValueError, match="track_hard=True") as a:
        plain.plan()
    with pytest.raises(ValueError, match="track_hard=True") as b:
        plain.hard_best()
    assert type(a.value) is type(b.value)


# ---------------------------------------------------------------- C ABI (host-only)
@pytest.fixture(scope="module")
def lib():
    from pfsgnn import native
    return native.lib()


def test_abi_struct_size_and_version(lib):
    from pfsgnn import native
    assert lib.pfsgnn_version().decode() == native.ABI_VERSION == "pfsgnn 0.3 gfx950"
    assert lib.pfsgnn_schedule_plan_args_bytes() == ctypes.sizeof(native.PlanArgs)
    assert native.PlanArgs.seg_start.offset == ctypes.sizeof(native.PlanArgs) - 8
    assert native.PlanArgs.mode.offset == 12 and native.PlanArgs.perm.offset == 16
    # the existing structs are unchanged
    assert lib.pfsgnn_schedule_args_bytes() == ctypes.sizeof(native.ScheduleArgs)
    assert lib.pfsgnn_schedule_budget_args_bytes() == ctypes.sizeof(native.ScheduleBudgetArgs)
    # one word per edge (three in the CSR form) and the fiber tables
    NS = 2 * 70
    assert lib.pfsgnn_schedule_plan_ws_bytes(2, 70, 9, 0) >= 4 * NS * 9 + 8 * (NS + 1) + 4 * NS
    assert lib.pfsgnn_schedule_plan_ws_bytes(2, 70, 9, 5000) >= 3 * 4 * 5000 + 8 * (NS + 1) + 4 * NS
    assert lib.pfsgnn_schedule_plan_ws_bytes(0, 70, 9, 0) == 0
    assert lib.pfsgnn_schedule_plan_ws_bytes(2, 70, 9, 1 << 31) == 0


def test_schedule_plan_refuses_bad_arguments_before_any_launch(lib):
    """Fake non-null pointers are never dereferenced: every refusal comes from a
    host-side check and names pfsgnn_schedule_plan."""
    from pfsgnn import native
    FAKE = 0x1000
    CSR = ("src_p", "tgt_p", "user_of", "fib_ptr", "cls_ord", "cls_ptr")
    OUTS = ("visits", "start", "used", "idle", "n_hard", "completeness", "utility", "over", "worst",
            "cut", "seg_ptr")

    def args(csr=False, **over):
        a = native.PlanArgs(G=1, NF=16, NC=2, mode=-1 if csr else 1, E=20 if csr else 0, cap=1)
        for f in OUTS + ("ci", "visits_in") + (CSR if csr else ()):
            setattr(a, f, FAKE)
        for f, v in over.items():
            setattr(a, f, v)
        return a

    def refused(a, *words, ws=(None, 0)):
        rc = lib.pfsgnn_schedule_plan(None if a is None else ctypes.byref(a), ws[0], ws[1], None)
        err = lib.pfsgnn_last_error().decode()
        assert rc != 0, words
        assert err.startswith("pfsgnn_schedule_plan:"), err
        for w in words:
            assert w in err, (err, w)

    refused(None, "null argument struct")
    refused(args(src_p=FAKE), "both batch forms")
    refused(args(csr=True, mode=1), "both batch forms")
    refused(args(csr=True, perm=FAKE), "both batch forms")
    refused(args(mode=-1), "neither batch form")
    refused(args(mode=3), "mode must be")
    refused(args(mode=-2), "mode must be")
    refused(args(mode=0), "mode 0 needs perm")
    for k in CSR:
        refused(args(csr=True, **{k: None}), "CSR form needs")
    for csr in (False, True):
        for k in OUTS:
            refused(args(csr, **{k: None}), "null output")
        refused(args(csr, ci=None), "null input")
        refused(args(csr, visits_in=None), "null input")
        refused(args(csr, seg_cap=5), "seg_cap > 0 needs")
        refused(args(csr, seg_cap=5, seg_edge=FAKE), "seg_cap > 0 needs")
        refused(args(csr, seg_cap=-1), "seg_cap must be >= 0")
        refused(args(csr, cap=2), "cap must be 0 or 1")
        refused(args(csr, cap=-1), "cap must be 0 or 1")
        refused(args(csr, NF=0), "need G > 0")
        refused(args(csr, G=-1), "need G > 0")
        refused(args(csr, NC=0), "need G > 0")
        # accepted up to the workspace check: null segment arrays with seg_cap = 0,
        # both segment arrays with a positive seg_cap, cap = 0
        refused(args(csr), "workspace too small")
        refused(args(csr), "workspace too small", ws=(FAKE, 64))
        refused(args(csr, seg_cap=9, seg_edge=FAKE, seg_start=FAKE, cap=0), "workspace too small")
    refused(args(csr=True, E=0), "E > 0")
    refused(args(csr=True, E=1 << 31), "E too large")
    refused(args(G=1 << 10, NF=1 << 11, NC=1 << 10), "E too large")
    refused(args(mode=0, perm=FAKE), "workspace too small")


def test_library_without_the_symbol_says_rebuild(tmp_path):
    """A "pfsgnn 0.3" library from before this op lacks pfsgnn_schedule_plan:
    native.lib() refuses it with the rebuild message, not an AttributeError."""
    from test_abi_and_host import _stand_in_library_is_refused
    from pfsgnn import native
    special = {"pfsgnn_version":
               'const char* pfsgnn_version(void) { return "%s"; }' % native.ABI_VERSION}
    source = "\n".join(special.get(n, "int %s(void) { return 0; }" % n) for n in native._SIGS
                       if not n.startswith("pfsgnn_schedule_plan"))
    out = _stand_in_library_is_refused(tmp_path, source + "\n")
    assert "pfsgnn_schedule_plan" in out and "rebuild" in out and "AttributeError" not in out
