"""The cases, references and bounds of tests/test_gpu_class_side_ops.py,
checked on the CPU (tests/class_side_case.py):

* the hand-written backward emulation the GPU tests compare with -- the
  composition behind target_class_bwd, and mlp_bwd(bn_part=, mom_coef=) --
  equals torch.autograd.grad through the float64 forward reference to 1e-10;
* every case reaches, by the restated unit geometry, the kernel branch it is
  named for;
* every bound can see a wrong kernel: each mutant of the reference (a plausible
  indexing or scaling slip of the fused kernels) puts at least one output 10x
  or more beyond that output's bound on the case named for it.
"""
import pytest
import torch

import class_side_case as cs
from emu_backend import EmuBackend

NCU = 256


def rel_err(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


# ------------------------------------------------------------------ autograd
AUTOGRAD_CASES = [("ragged_tail", 0, cs.FULL), ("ragged_tail", 1, cs.FULL), ("ragged_tail", 0, cs.BARE),
                  ("ragged_tail", 1, cs.VARIANTS[2]), ("one_class", 0, cs.FULL),
                  ("one_class", 0, cs.BARE)]


@pytest.mark.parametrize("case,idx,v", AUTOGRAD_CASES,
                         ids=[f"{c}{i}-{cs.variant_id(v)}" for c, i, v in AUTOGRAD_CASES])
def test_class_bwd_reference_equals_autograd(case, idx, v):
    G, NF, NC, F = cs.case_shapes(case)[idx]
    inp = cs.block_inputs(G, NF, NC, F, v, cs.case_seed(case, idx))
    be = EmuBackend()
    hsum0 = cs.ref_block_fwd(inp)["hsum"]
    lv = {k: inp[k].clone().requires_grad_() for k in ("xt", "u", "xs", "gamma", "beta")}
    lv["hsum"] = hsum0.clone().requires_grad_()
    if v.normed:
        lv["gw"] = inp["gw"].clone().requires_grad_()
    agg = inp["Wt2"] @ lv["hsum"] + NF * inp["bt2"][:, None]
    hT = [(lv["xt"], 0, False), (agg, F, False), (lv["u"], 3 * F, True)]
    t = be.target_global_fwd(hT, G, NC, inp["W1"], inp["b1"], inp["W2"], inp["b2"],
                             (lv["gamma"], lv["beta"], None, None, cs.BN_MOM, cs.BN_EPS), lv["xs"],
                             NF, lv["u"], inp["gW1"], inp["gb1"], inp["gW2"], inp["gb2"],
                             lv.get("gw"), cs.RMS_EPS, None)
    fwd = {k: t[k].detach() for k in ("Z", "Yp", "mu", "var", "gZ", "gV")}
    if v.normed:
        fwd["y1"], fwd["r1"], fwd["r2"] = (x.detach() for x in t["rms"])
    b = cs.class_bwd_inputs(inp, fwd, v, 99, round32=False)
    dYu = b["gu_up"].clone()
    for X in b["pend"]:
        dYu += X.reshape(F, G, -1).sum(2)
    L = (t["xt"] * b["g_xt"]).sum() + (t["u"] * dYu).sum()
    wrt = dict(lv, agg=agg, xt_new=t["xt"], Yp=t["Yp"], Z=t["Z"], V=t["gV"], gZ=t["gZ"])
    g = dict(zip(wrt, torch.autograd.grad(L, list(wrt.values()))))
    o = cs.ref_class_bwd(b)
    expect = {
        "g_xs": b["g_xs"] + g["xs"], "g_xt": g["xt_new"], "gxt_in": b["gxt_in"] + g["xt"],
        "g_agg": g["agg"], "g_hsum": g["hsum"], "dgamma": b["dgamma"] + g["gamma"],
        "dbeta": b["dbeta"] + g["beta"], "dYp": g["Yp"], "dZ": g["Z"], "gV": g["V"], "gdZ": g["gZ"],
    }
    for k, e in expect.items():
        assert rel_err(o[k], e) <= 1e-10, (k, rel_err(o[k], e))
    # u enters node_mlp_2 (per class: gu_t) and the GlobalModel (gu)
    du = (o["gu"] - b["gu"]) + o["gu_t"].reshape(F, G, NC).sum(2)
    assert rel_err(du, g["u"]) <= 1e-10
    if v.normed:
        assert rel_err(o["dw"], g["gw"]) <= 1e-10
        assert rel_err(o["dwp"].sum(1), o["dw"]) <= 1e-12 and o["dwp"].shape == (F, G)
    else:
        assert "dwp" not in o
    assert set(o) >= set(cs.BWD_CLASS_OUTS)


@pytest.mark.parametrize("F,N,G", [(10, 37, 1), (8, 38, 2), (10, 130, 2)])
def test_mlp_bwd_pre_reference_equals_autograd(F, N, G):
    i = cs.smodel_inputs(F, N, G, 300 + F + N)
    be = EmuBackend()
    lv = {k: i[k].clone().requires_grad_() for k in ("x", "M", "u", "gamma", "beta")}
    mom = cs.moments_of(lv["M"])
    hs = cs.moment_rows(mom)
    segs = [(lv["x"], 0, False), (hs, F, False), (lv["u"], 9 * F, True)]
    Y, Z, Yp, mu, var = be.mlp_fwd(segs, N, i["W1"], i["b1"], i["W2"], i["b2"],
                                   bn=(lv["gamma"], lv["beta"], None, None, cs.BN_MOM, cs.BN_EPS))
    L = (Y * i["dY"]).sum()
    wrt = dict(lv, Yp=Yp, Z=Z, hs=hs)
    g = dict(zip(wrt, torch.autograd.grad(L, list(wrt.values()))))
    b = dict(i, mom=mom.detach(), hs=hs.detach(), Z=Z.detach(), Yp=Yp.detach(), mu=mu.detach(),
             var=var.detach())
    b["bn_part"] = cs.bn_part_of(b["dY"], b["Yp"], b["mu"], b["var"])
    assert b["bn_part"].shape == ((N + 63) // 64, 32)
    o = cs.ref_mlp_bwd_pre(b)
    d = i["M"] - b["mom"][0][..., None]
    C = o["coef"]
    gM = C[0][..., None] + d * (C[1][..., None] + d * (C[2][..., None] + d * C[3][..., None]))
    du = o["dX2"].reshape(F, G, N // G).sum(2)
    expect = {"dYp": (o["dYp"], g["Yp"]), "dZ": (o["dZ"], g["Z"]), "dX0": (o["dX0"], i["g_x"] + g["x"]),
              "du": (du, g["u"]), "coef": (gM, g["M"]),
              "dgamma": (o["dgamma"], i["dgamma"] + g["gamma"]),
              "dbeta": (o["dbeta"], i["dbeta"] + g["beta"])}
    for k, (a, e) in expect.items():
        assert rel_err(a, e) <= 1e-10, (k, rel_err(a, e))
    # the partials carry the same sums mlp_bwd makes itself, and the moment rows
    # written out (no epilogue) are d loss / d [mean; std; skew; kurt]
    o2 = cs.ref_mlp_bwd_pre(b, bn_part=False, mom=False)
    assert rel_err(o2["gst"], g["hs"]) <= 1e-10
    for k in ("dYp", "dZ", "dgamma", "dbeta", "dX0", "dX2"):
        assert rel_err(o[k], o2[k]) <= 1e-12, k


def test_spelt_tail_equals_emulation():
    """class_side_case._tail (which the mutants change) == EmuBackend.target_global_fwd."""
    for case, idx, v in (("ragged_tail", 0, cs.FULL), ("ragged_tail", 1, cs.BARE)):
        G, NF, NC, F = cs.case_shapes(case)[idx]
        inp = cs.block_inputs(G, NF, NC, F, v, cs.case_seed(case, idx))
        a, b = cs.ref_block_fwd(inp), cs.ref_block_fwd(inp, spelt=True)
        assert set(a) == set(b)
        for k in a:
            assert rel_err(b[k], a[k]) <= 1e-13, k


# ------------------------------------------------------------------ reachability
def geo_of(case, idx=0, ncu=NCU):
    G, NF, NC, F = cs.case_shapes(case, ncu)[idx]
    return (G, NF, NC, F), cs.unit_geometry(G, NF, NC, ncu)


def test_tail_ct_restated():
    assert cs.tail_ct(2, 128) == 16 and cs.tail_ct(32, 256) == 16 and cs.tail_ct(33, 256) == 32
    assert cs.tail_ct(1, 1024) == 16 and cs.tail_ct(1, 1025) == 32 and cs.tail_ct(1, 2048) == 32
    assert cs.tail_ct(1, 2049) == 0 and cs.tail_ct(513, 1) == 0 and cs.tail_ct(512, 32) == 32
    assert cs.tail_ct(512, 33) == 0


@pytest.mark.parametrize("ncu", [256, 304])
def test_every_case_reaches_its_branch(ncu):
    (G, NF, NC, F), g = geo_of("one_class", 0, ncu)
    assert (G, NF, NC, F) == (2, 5, 1, 10) and G * NC == 2
    for s in (g["fwd"], g["bwd"]):
        assert s["QB"] == 1 and s["last_ncl"] == 1 and s["nunits"] == G
    for idx, shape in enumerate([(2, 7, 17, 10), (3, 4, 33, 8)]):
        got, g = geo_of("ragged_tail", idx, ncu)
        assert got == shape
        for s in (g["fwd"], g["bwd"]):
            assert s["CT"] == 16 and s["last_ncl"] == 1 and s["QB"] >= 2     # beside full units
    (G, NF, NC, F), g = geo_of("few_fibers", 0, ncu)
    for s in (g["fwd"], g["bwd"]):
        assert s["CT"] == 16 and s["QB"] == cs.QBMAX and s["empty_fiber_units"] == 61
    (G, NF, NC, F), g = geo_of("fwd_limit", 0, ncu)
    assert g["fwd"]["CT"] == 32 and g["fwd"]["QB"] == cs.QBMAX and g["bwd"] is None and NC > 1024
    (G, NF, NC, F), g = geo_of("many_units_ct16", 0, ncu)
    for s in (g["fwd"], g["bwd"]):
        assert s["CT"] == 16 and s["nunits"] == ncu + 8 > ncu and s["max_trips"] == 2
    for idx, F_ in enumerate((16, 10)):
        (G, NF, NC, F), g = geo_of("many_units_ct32", idx, ncu)
        assert F == F_ and G <= 64
        assert g["fwd"]["CT"] == 32 and g["fwd"]["nunits"] == 8 * G > ncu
        assert g["bwd"]["nunits"] == 16 * G > 2 * ncu and g["bwd"]["max_trips"] == 3
        # more rows than threads: the normalising loop takes two rounds (the
        # most, 512 rows, at F = 16)
        assert g["fwd"]["CT"] * F > 256 and (g["fwd"]["CT"] * F == 512) == (F == 16)
    (G, NF, NC, F), g = geo_of("many_partials", 0, ncu)
    assert g["BPG"] > 32 and g["BPG"] % 32 != 0
    (G, NF, NC, F), g = geo_of("bench_like", 0, ncu)
    assert g["BPG"] == 3 and g["fwd"]["CT"] == 16 and g["fwd"]["max_trips"] == 1
    for case in cs.CASES:
        for G, NF, NC, F in cs.case_shapes(case, ncu):
            assert G * NF * NC <= 50000, case
            assert cs.unit_geometry(G, NF, NC, ncu)["fwd"] is not None, case
            cs.assert_reaches_branch(case, (G, NF, NC, F), ncu)   # what the GPU test asserts


def test_variants_cover_every_option():
    for field, values in (("normed", (True, False)), ("nxt", (True, False)), ("rmrv", (True, False)),
                          ("npend", (0, 1, 4)), ("tmask", (True, False)), ("scsh", (True, False))):
        assert {getattr(v, field) for v in cs.VARIANTS} == set(values), field
    ids = [cs.variant_id(v) for v in cs.VARIANTS]
    assert len(set(ids)) == len(ids)
    assert sum(1 for c, i, v in cs.case_list() if c == "ragged_tail") == 2 * len(cs.VARIANTS)
    assert sum(1 for c, i, v in cs.case_list() if c == "many_units_ct16") == len(cs.VARIANTS)
    assert {c for c, i, v in cs.case_list()} == set(cs.CASES)


def test_builders_are_deterministic_and_float32_exact():
    a = cs.block_inputs(2, 7, 17, 10, cs.FULL, 1)
    b = cs.block_inputs(2, 7, 17, 10, cs.FULL, 1)
    for k, t in a.items():
        if isinstance(t, torch.Tensor):
            assert torch.equal(t, b[k]) and torch.equal(t, t.float().double()), k
    i = cs.smodel_inputs(8, 37, 1, 3)
    for k, t in i.items():
        if isinstance(t, torch.Tensor):
            assert torch.equal(t, t.float().double()), k


# ------------------------------------------------------------------ the bounds see a wrong kernel
@pytest.mark.parametrize("mutant", sorted(cs.MUTANTS))
def test_bounds_see_the_mutant(mutant):
    case = cs.MUTANTS[mutant]
    R = cs.reference(case, 0, cs.FULL, NCU)
    G, NF, NC, F = R["shape"]
    assert NF != NC
    fb, bb = cs.bounds("fwd", R["fwd64"], R["fwd32"]), cs.bounds("bwd", R["bwd64"], R["bwd32"])
    mf = cs.ref_block_fwd(R["inp"], mutant=mutant, ncu=NCU)
    mb = cs.ref_class_bwd(R["binp"], mutant=mutant, ncu=NCU)
    ratios = {"fwd." + k: cs.max_err(mf[k], R["fwd64"][k]) / fb[k] for k in fb}
    ratios.update({"bwd." + k: cs.max_err(mb[k], R["bwd64"][k]) / bb[k] for k in bb})
    worst = max(ratios, key=ratios.get)
    print(f"{mutant} on {case}: worst {worst} at {ratios[worst]:.3g} x its bound")
    assert ratios[worst] >= 10.0, (mutant, worst, ratios[worst])
    # and the unmutated reference sits inside every bound of its float32 self by construction
    assert all(cs.max_err(R["fwd32"][k].double(), R["fwd64"][k]) <= fb[k] for k in fb)
