"""The cases, references, geometry and bounds of tests/test_gpu_node_linalg.py,
checked on the CPU (tests/node_linalg_case.py):

* the restated launch geometry: which (tm, per) weight-gradient shapes the
  plan reaches over every M, K <= 256 (14; the ten instantiated ones it never
  selects are listed too), and that the case list covers all 11 MT and all 8
  KSM of k_gemm in both orientations, the 12 batched shapes, the 14 reachable
  weight-gradient shapes with both X3 depths, and the reduce thresholds;
* every case reaches the branch it is named for;
* the exact inputs are exact: sum |terms| * 64 < 2^24 and ref32 == ref64;
* the references equal autograd to 1e-10 in float64 (wgrad_cat and lin_t are
  the gradients of lin_cat with respect to W, b and X), and refx3 stays within
  2^-14 relative of ref64;
* every bound can see a wrong kernel: each mutant of the reference falls 10x or
  more outside a bound on random inputs and gives a non-zero difference on
  exact inputs, in at least one case.
"""
import pytest
import torch

import node_linalg_case as nl
from emu_backend import EmuBackend, dlrelu

GEMM = {c.name: c for c in nl.GEMM_CASES}
WG = {c.name: c for c in nl.WG_CASES}
PATH_X3 = "mfma"


# ------------------------------------------------------------------ geometry
def test_wgrad_pairs():
    reach = nl.reachable_wg_pairs()
    assert tuple(sorted(reach)) == tuple(sorted(nl.REACHABLE_WG)) and len(reach) == 14
    assert set(reach) <= set(nl.WG_ALL), "a reachable shape has no kernel"
    assert tuple(sorted(set(nl.WG_ALL) - set(reach))) == nl.UNREACHABLE_WG
    for (tm, per), (M, K, db) in nl.WG_TABLE.items():
        p = nl.wgrad_plan(M, K, 64, db)
        assert (p["tm"], p["per"]) == (tm, per)
    x3 = [p for p in nl.REACHABLE_WG if nl.wg_x3_for(*p, PATH_X3)]
    assert sorted(x3) == [(4, 4), (4, 8), (4, 16), (8, 8), (8, 16), (16, 8)]
    assert sorted(p for p in x3 if nl.wg_deep(*p)) == [(4, 4), (4, 8), (8, 8)]
    assert not any(nl.wg_x3_for(*p, "mfma32") for p in nl.REACHABLE_WG)
    for text, M, K, N, db in nl.WG_REFUSALS:
        assert nl.wgrad_plan(M, K, N, db) == text.replace("\\", "")


def test_gemm_geometry():
    assert [nl.gemm_ksm(k) for k in (1, 4, 5, 12, 13, 20, 21, 32, 33, 40, 41, 64, 65, 100, 101, 160, 161)] \
        == [1, 1, 3, 3, 5, 5, 8, 8, 10, 10, 16, 16, 25, 25, 40, 40, -1]
    assert nl.gemm_mt(176) == 11 and nl.gemm_mt(177) == 12
    assert nl.gemm_lds(176, 160) == 176 * 161 * 4 == 113344       # the 113 KB corner
    assert nl.gemm_multi_shape([(64, 40), (1, 1)]) == (4, 10)


def test_case_list_covers_every_branch():
    for op in ("lin", "lin_t"):
        cs = [c for c in nl.GEMM_CASES if c.op == op]
        assert {c.want["mt"] for c in cs} == set(range(1, 12)), op
        assert {c.want["ksm"] for c in cs} == set(nl.KSMS), op
        assert any(nl.gemm_dims(c) == (176, 160) for c in cs), op
        assert {c.N for c in cs} >= {1, 63, 64, 65, 130}
    assert {nl.gemm_dims(c)[1] for c in nl.GEMM_CASES} >= {12, 13, 20, 21, 32, 33, 40, 41, 64, 65, 100, 101, 160}
    assert {nl.gemm_dims(c)[0] for c in nl.GEMM_CASES} >= {16, 17, 176}
    cat = [c for c in nl.GEMM_CASES if c.op == "lin_cat"]
    assert {len(c.blocks) for c in cat} == {1, 2, 3, 4}
    assert {[k for _, k in c.blocks].index("g") for c in cat if ("g" in [k for _, k in c.blocks])} >= {0, 1, 2}
    assert {("1" if c.N // c.G == 1 else "N" if c.G == 1 else "mid") for c in cat
            if any(k == "g" for _, k in c.blocks)} == {"1", "N", "mid"}
    for flag in (lambda c: c.add, lambda c: c.b, lambda c: c.bscale != 1.0):
        assert {bool(flag(c)) for c in nl.GEMM_CASES if c.op != "lin_t"} == {True, False}
    assert {c.z for c in nl.GEMM_CASES if c.op == "lin_t"} == {True, False}
    # the batched products
    assert {s for c in nl.BATCH_CASES for s in nl.batch_launches(c)} >= set(nl.GMM_SHAPES)
    assert {c.want["njob"] for c in nl.BATCH_CASES} == {1, 4, 5, 9}
    assert {len(nl.batch_launches(c)) for c in nl.BATCH_CASES} == {1, 2, 3}
    assert {j[0] for c in nl.BATCH_CASES for j in c.jobs} == {"cat", "t"}
    assert any(j[0] == "t" and j[4] for c in nl.BATCH_CASES for j in c.jobs)
    # the weight gradients
    plans = {c.name: nl.wg_plan(c) for c in nl.WG_CASES}
    assert {(p["tm"], p["per"]) for p in plans.values()} == set(nl.REACHABLE_WG)
    assert {p["ntile"] for p in plans.values()} >= {8, 9, 16, 17, 18, 32, 33, 64, 65}
    assert {c.N for c in nl.WG_CASES} >= {1, 3, 37, 63, 64, 65, 129, 400, 401, 801, 2001, 2100}
    for deep in (True, False):      # both X3 depths at one, two and three chunks per block
        assert {p["last_chunks"] for p in plans.values()
                if nl.wg_x3_for(p["tm"], p["per"], PATH_X3) and nl.wg_deep(p["tm"], p["per"]) == deep
                and p["nblk"] == 1} >= {1, 2, 3}
    assert {p["nblk"] for p in plans.values()} >= {1, 2, 3, 6}
    assert {p["last"] for p in plans.values() if p["nblk"] > 1} >= {81, 145, 161, 180}
    assert {(c.misalign, plans[c.name]["vec"]) for c in nl.WG_CASES if c.misalign} \
        == {("dY", 0), ("seg", 0), ("bc", 1)}
    assert any(p["vec"] == 0 and c.N % 4 for c, p in zip(nl.WG_CASES, plans.values()))
    assert {c.N // c.G for c in nl.WG_CASES if any(k == "g" for _, k in c.blocks)} >= {1, 3, 50, 401}
    assert {c.db for c in nl.WG_CASES} == {True, False}
    # the deferred pass: at, past and two launches past the WG_MULTI table
    for njob in (1, 24, 25, 50):
        jobs = nl.defer_jobs(njob)
        assert all(c.N % c.G == 0 for c, _ in jobs)
        shapes = [(p["tm"], p["per"]) for p in (nl.wg_plan(c) for c, _ in jobs)]
        main = [n for n, s in enumerate(shapes) if s == nl.DEFER_MAIN]
        assert len(main) == njob and -(-njob // nl.WG_MULTI) == {1: 1, 24: 1, 25: 2, 50: 3}[njob]
        if njob >= 24:
            x3 = {s for s in shapes if nl.wg_x3_for(*s, PATH_X3)}
            assert len(set(shapes)) >= 3 and len(x3) >= 2
            assert main != list(range(main[0], main[0] + njob)), "the groups are non-contiguous"
            assert {t for _, t in jobs} >= {"same", "adj0", "adj1"}
            sizes = {(c.M, nl.wg_K(c), c.N, nl.wg_plan(c)["lds"]) for n, (c, _) in enumerate(jobs) if n in main}
            assert len({s[3] for s in sizes}) >= 2 and len({s[2] for s in sizes}) >= 3
    # the reductions
    assert nl.red_stages(512) == (False, 512) and nl.red_stages(513) == (True, 3)
    assert nl.red_stages(1031) == (True, 5)
    lists = nl.red_cases()
    assert {d.nb for ds in lists.values() for d in ds} >= set(nl.RED_NB)
    assert {d.rows * d.cols for ds in lists.values() for d in ds} >= {1, 15, 16, 17, 63, 64, 65, 91}
    mixed = lists["red-mixed-seg"]
    assert {nl.red_stages(d.nb)[0] for d in mixed} == {True, False}
    assert len(lists["red-97-descriptors"]) == nl.PF_MAX_RED + 1
    assert len(lists["red-200-descriptors"]) > 2 * nl.PF_MAX_RED


@pytest.mark.parametrize("c", nl.GEMM_CASES + nl.BATCH_CASES + nl.WG_CASES, ids=lambda c: c.name)
def test_case_reaches_its_branch(c):
    nl.assert_reaches_branch(c)


# ------------------------------------------------------------------ exactness
def on_grid(t, step=1 / 64):
    return bool((torch.round(t / step) * step == t).all())


@pytest.mark.parametrize("c", nl.GEMM_CASES, ids=lambda c: c.name)
def test_exact_gemm_inputs_are_exact(c):
    i = nl.gemm_inputs(c, "exact")
    assert nl.gemm_abs_terms(c, i) * 64 < 2 ** 24
    r64, r32 = nl.ref_gemm(c, i, False), nl.ref_gemm(c, i, False, torch.float32)
    if c.z:      # one more IEEE operation on an exact value: * lrelu'(Z), restated in float32
        pre = nl.ref_gemm(c._replace(z=False, add=False), i, False)
        assert on_grid(pre)
        want = pre.float() * dlrelu(i["Z"].float())
        if c.add:
            want = i["Y0"].float() + want
        assert torch.equal(r32, want)
    elif c.add and c.op != "lin_t":  # one more IEEE operation on an exact value: the add onto a non-grid Y0
        pre = nl.ref_gemm(c._replace(add=False), i, False)
        assert on_grid(pre) and not on_grid(i["Y0"])
        assert torch.equal(r32, i["Y0"].float() + pre.float()) and torch.equal(r64, i["Y0"] + pre)
    else:
        assert on_grid(r64) and torch.equal(r32.double(), r64)


@pytest.mark.parametrize("c", nl.WG_CASES, ids=lambda c: c.name)
def test_exact_wgrad_inputs_are_exact(c):
    i = nl.wg_inputs(c, "exact")
    assert nl.wg_abs_terms(c, i) * 64 < 2 ** 24
    r64, r32, rx3 = nl.ref_wg(c, i, False), nl.ref_wg(c, i, False, torch.float32), nl.refx3_wg(c, i, False)
    for k in r64:
        assert on_grid(r64[k]) and torch.equal(r32[k].double(), r64[k]), k
        assert torch.equal(rx3[k], r64[k]), k      # five significant bits: lo = 0


def test_exact_other_inputs_are_exact():
    for c in nl.GATHER_CASES:
        if not c.refused:
            i = nl.gather_inputs(c, "exact")
            a = dict(i, W=i["W"].abs(), X=i["X"].abs(), b=i["b"].abs(), G=[g.abs() for g in i["G"]])
            assert nl.ref_gather(c, a).max().item() * 64 < 2 ** 24
            assert torch.equal(nl.ref_gather(c, i, torch.float32).double(), nl.ref_gather(c, i))
    for c in nl.BATCH_CASES:
        i = nl.batch_inputs(c, "exact")
        for a, b in zip(nl.ref_batch(c, i), nl.ref_batch(c, i, torch.float32)):
            assert on_grid(a) and torch.equal(b.double(), a) and a.abs().max() * 64 < 2 ** 24 / 40
    gen = torch.Generator().manual_seed(3)
    for ds in nl.red_cases().values():
        for d in ds:
            part, out0 = nl.red_part(gen, d, "exact"), nl.grid(gen, d.rows, d.ldo)
            assert (part.abs().sum(0).max().item() * 2 + 2) * 64 < 2 ** 24
            assert torch.equal(nl.ref_red(d, part, out0, torch.float32).double(), nl.ref_red(d, part, out0))


# ------------------------------------------------------------------ autograd
@pytest.mark.parametrize("name", ["lin_cat-bc-last", "lin_cat-bc-middle", "lin_cat-two-bc", "lin_cat-one"])
@pytest.mark.parametrize("act_in", [False, True])
def test_references_equal_autograd(name, act_in):
    """wgrad_cat and lin_t against torch.autograd.grad through lin_cat."""
    c = GEMM[name]
    i = nl.gemm_inputs(c, "random")
    be = EmuBackend()
    _, cols = nl.gemm_layout(c)
    W = i["W"].clone().requires_grad_()
    b = i["b"].clone().requires_grad_() if c.b else None
    X = [x.clone().requires_grad_() for x in i["X"]]
    segs = [(x, col, k == "g") for x, col, (_, k) in zip(X, cols, c.blocks)]
    Y = be.lin_cat(W, segs, c.N, b=b, act_in=act_in, bscale=c.bscale)
    gen = torch.Generator().manual_seed(1)
    dY = nl.rnd(gen, *Y.shape)
    grads = torch.autograd.grad((Y * dY).sum(), [W] + ([b] if c.b else []) + X)
    dW, db = torch.zeros_like(i["W"]), torch.zeros(c.M, dtype=torch.float64)
    be.wgrad_cat(dY, [(x.detach(), col, bc) for x, col, bc in segs], dW, db=db, act_in=act_in,
                 dbscale=c.bscale)
    assert (dW - grads[0]).abs().max() <= 1e-10 * grads[0].abs().max()
    if c.b:
        assert (db - grads[1]).abs().max() <= 1e-10 * grads[1].abs().max()
    for (x, col, bc), g in zip(segs, grads[-len(X):]):
        if bc:
            continue        # (the broadcast block's gradient is lin_t followed by graph_reduce)
        got = be.lin_t(i["W"], col, x.shape[0], dY, z=x.detach() if act_in else None)
        assert (got - g).abs().max() <= 1e-10 * g.abs().max()


@pytest.mark.parametrize("c", [c for c in nl.WG_CASES if c.N >= 37][::3], ids=lambda c: c.name)
def test_refx3_close_to_ref64(c):
    i = nl.wg_inputs(c, "random")
    for act in (False, True):
        a, b = nl.refx3_wg(c, i, act), nl.ref_wg(c, i, act)
        for k, blk in nl.wg_blocks_of(c, b).items():
            got = nl.wg_blocks_of(c, a)[k]
            assert not blk.numel() or nl.max_err(got, blk) < 2.0 ** -14 * blk.abs().max().item(), k


# ------------------------------------------------------------------ mutants
def far_outside(blocks64, blocks32, blocksm, rtol):
    """Some block of the mutant 10x or more beyond that block's bound."""
    return any(nl.max_err(blocksm[k], blocks64[k]) >= 10 * nl.bound(blocks64[k], blocks32[k], rtol) > 0
               for k in blocks64)


def differs(a, b):
    return any(not torch.equal(a[k].double(), b[k].double()) for k in a)


WG_MUTANTS = {"last_node_dropped": ("wg-deep-N2100", "wg-fp32-N2100", "wg-flat-N401"),
              "last_chunk_dropped": ("wg-deep-N2100", "wg-deep-N129"),
              "segment_column_off_by_one": ("wg-cat4", "wg-bc-npg3"),
              "broadcast_next_graph": ("wg-bc-npg3", "wg-bc-npg50-x3", "wg-bc-npg1"),
              "dbscale_ignored": ("wg-cat4", "wg-bc-npg50"),
              "act_in_ignored": ("wg-cat4", "wg-tm1-per1-N129")}


@pytest.mark.parametrize("mutant", sorted(WG_MUTANTS))
def test_wgrad_mutants_are_caught(mutant):
    for name in WG_MUTANTS[mutant]:
        c = WG[name]
        p = nl.wg_plan(c)
        rtol = nl.RTOL_X3 if nl.wg_x3_for(p["tm"], p["per"], PATH_X3) else nl.RTOL_FP32
        i = nl.wg_inputs(c, "random")
        blk = [nl.wg_blocks_of(c, o) for o in (nl.ref_wg(c, i, True), nl.ref_wg(c, i, True, torch.float32),
                                               nl.ref_wg(c, i, True, mutant=mutant))]
        assert far_outside(*blk, rtol), (mutant, name)
        if mutant != "act_in_ignored":
            i = nl.wg_inputs(c, "exact")
            assert differs(nl.ref_wg(c, i, False), nl.ref_wg(c, i, False, mutant=mutant)), (mutant, name)


GEMM_MUTANTS = {"segment_column_off_by_one": ("lin_cat-bc-last", "lin_cat-bc-middle"),
                "broadcast_next_graph": ("lin_cat-bc-last", "lin_cat-two-bc", "lin_cat-bc-first"),
                "bscale_ignored": ("lin_cat-bc-middle", "lin-17x13-N63"),
                "act_in_ignored": ("lin-16x12-N1", "lin_cat-wide"),
                "add_overwrites": ("lin-17x13-N63", "lin_t-16x12-N64", "lin_cat-bc-middle")}


@pytest.mark.parametrize("mutant", sorted(GEMM_MUTANTS))
def test_gemm_mutants_are_caught(mutant):
    for name in GEMM_MUTANTS[mutant]:
        c = GEMM[name]
        i = nl.gemm_inputs(c, "random")
        r64, r32, rm = (nl.ref_gemm(c, i, True), nl.ref_gemm(c, i, True, torch.float32),
                        nl.ref_gemm(c, i, True, mutant=mutant))
        assert far_outside(dict(Y=r64), dict(Y=r32), dict(Y=rm), nl.RTOL_FP32), (mutant, name)
        if mutant != "act_in_ignored":
            i = nl.gemm_inputs(c, "exact")
            assert not torch.equal(nl.ref_gemm(c, i, False), nl.ref_gemm(c, i, False, mutant=mutant))


def test_other_mutants_are_caught():
    # a gather using idx1 for both tables
    c = next(c for c in nl.GATHER_CASES if c.name == "gather2")
    for kind in ("random", "exact"):
        i = nl.gather_inputs(c, kind)
        r64, rm = nl.ref_gather(c, i), nl.ref_gather(c, i, mutant="gather_idx1_for_both")
        if kind == "random":
            assert far_outside(dict(Y=r64), dict(Y=nl.ref_gather(c, i, torch.float32)), dict(Y=rm), nl.RTOL_FP32)
        else:
            assert not torch.equal(r64, rm)
    # a batched job reading its neighbour's bias
    caught = {"random": 0, "exact": 0}
    for c in nl.BATCH_CASES:
        for kind in caught:
            i = nl.batch_inputs(c, kind)
            r64, r32, rm = nl.ref_batch(c, i), nl.ref_batch(c, i, torch.float32), nl.ref_batch(c, i, mutant="neighbour_bias")
            for a, b, m in zip(r64, r32, rm):
                if kind == "random":
                    caught[kind] += far_outside(dict(Y=a), dict(Y=b), dict(Y=m), nl.RTOL_FP32)
                else:
                    caught[kind] += not torch.equal(a, m)
    assert caught["random"] and caught["exact"]
    # the 513th partial dropped
    d = nl.red_cases()["red-nb513"][0]
    for kind in ("random", "exact"):
        gen = torch.Generator().manual_seed(5)
        part, out0 = nl.red_part(gen, d, kind), nl.draw(kind, gen, d.rows, d.ldo)
        r64, rm = nl.ref_red(d, part, out0), nl.ref_red(d, part, out0, drop=512)
        if kind == "random":
            assert far_outside(dict(o=r64), dict(o=nl.ref_red(d, part, out0, torch.float32)), dict(o=rm),
                               nl.RTOL_FP32)
        else:
            assert not torch.equal(r64, rm)
    # two overlapping reductions applied in the wrong order
    for kind in ("random", "exact"):
        gen = torch.Generator().manual_seed(6)
        rects = nl.OVERLAPS["same-cells"]
        parts = [nl.draw(kind, gen, 3, r[2], r[3]) for r in rects]
        out0 = nl.draw(kind, gen, 8, 12)
        r64, rm = nl.ref_overlap(rects, parts, out0), nl.ref_overlap(rects, parts, out0, order=(1, 0))
        if kind == "random":
            r32 = nl.ref_overlap(rects, [p.float() for p in parts], out0.float())
            assert far_outside(dict(o=r64), dict(o=r32), dict(o=rm), nl.RTOL_FP32)
        else:
            assert not torch.equal(r64, rm)
