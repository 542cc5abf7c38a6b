"""The folded TModel / SModel edge backward pair (pfsgnn_target_bwd with
`fold` + pfsgnn_source_bwd with `dWt1`: the mask-only target_bwd, and
source_bwd taking dWt1[:, F:2F]) against today's pair
(the same two entry points without `fold` / `dWt1`) on the same inputs and against a
float64 torch evaluation of TModel's part, with zeroed gradient buffers.

What source_bwd computed before is bitwise unchanged (g_tot, GzS, dWs1, dWs2,
dbs2, the edge BatchNorm coefficients); what moved between the kernels (GzT,
g_xs, SModel's BatchNorm partial sums, dWt1[:, F:2F]) and what is made from it
by the unchanged wgrad (dWt1[:, :F], the bias gradient) stays within
test_gpu_ops.close's default tolerances of today's pair and of float64 -- and,
since the fold issues the same operations in the same order from the other
kernel, is bitwise today's too (a training step amplifies any other rounding
within a few optimizer steps); two runs of the folded pair are bitwise
identical.  At Fdim 16 the library keeps today's kernels behind the
folded arguments (pfsgnn_tbwd_fold is 0 there), so those cases compare the
same kernels through both forms of the calls.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_ops import close, cuda, r  # noqa: E402

# (1, 9, 128) and (2, 7, 200): NC above a block's class range (MF_MAX_CPS) and
# more than one class split; (1, 70, 1) / (1, 16, 2): the shortest
# class streams, two fiber groups / one full wave
GEOMS = [(1, 37, 12), (2, 50, 16), (1, 9, 128), (3, 21, 5), (2, 7, 200), (1, 70, 1), (1, 16, 2)]
CASES = [(10, p) for p in ("mfma", "mfma32", "bf16x6", "bf16x3")] + \
        [(F, p) for F in (8, 16) for p in ("mfma", "mfma32")]
LEAKY = 0.1
EPS = 1e-5


@pytest.fixture(scope="module")
def hb():
    from pfsgnn.native import HipBackend
    return HipBackend()


def q(t, step):
    return torch.round(t / step) * step


def make_inputs(G, NF, NC, F):
    """Inputs on test_gpu_ops.test_edge_ops' grid: TModel's pre-activation is
    exact on every path, so the forward's mask and the float64 slopes agree."""
    gen = torch.Generator().manual_seed(31 + G * 1000 + NF * 10 + NC + F)
    E, NS, NT = G * NF * NC, G * NF, G * NC
    i = dict(
        y=q(r(F, E, scale=2, gen=gen), 1 / 4),
        sc=q(r(F, gen=gen) * 0.3 + 1, 1 / 8), sh=q(r(F, gen=gen), 1 / 8),
        Rs=q(r(2 * F, NS, gen=gen), 1 / 256), Wt1=q(r(2 * F, 2 * F, scale=0.3, gen=gen), 1 / 64),
        g_hsum=r(2 * F, NT, gen=gen), g_xs=r(F, NS, gen=gen), xs=r(F, NS, gen=gen),
        Yp=r(F, NS, gen=gen), mu=r(F, gen=gen) * 0.1, var=r(F, gen=gen).abs() + 0.5,
        Qt=q(r(2 * F, NT, gen=gen), 1 / 256), Ws1=q(r(2 * F, 2 * F, scale=0.3, gen=gen), 1 / 64),
        Ws2=r(2 * F, 2 * F, scale=0.3, gen=gen), bs2=r(2 * F, gen=gen), mean=r(2 * F, NS, gen=gen),
        coef=r(4, 2 * F, NS, gen=gen)
        * torch.tensor([1, 0.3, 0.1, 0.03], dtype=torch.float64)[:, None, None],
        g_next=r(F, E, gen=gen), g_xt=r(F, NT, gen=gen),
        mu1=r(F, gen=gen), var1=r(F, gen=gen).abs() + 0.5, gamma=r(F, gen=gen))
    i["inv1"] = 1.0 / torch.sqrt(i["var1"] + EPS)
    return i


def reference(i, G, NF, NC, F):
    """TModel's edge backward in float64 (gnn.py:188-190): GzT, the finished
    g_xs, its BatchNorm sums, dWt1[:, F:2F]."""
    x = (i["sc"][:, None] * i["y"] + i["sh"][:, None]).view(F, G, NC, NF)
    Rs = i["Rs"].view(2 * F, G, 1, NF)
    z = Rs + torch.einsum("hk,kgcf->hgcf", i["Wt1"][:, F:], x)
    slope = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, LEAKY))
    gz = i["g_hsum"].view(2 * F, G, NC, 1) * slope
    GzT = gz.sum(2).reshape(2 * F, G * NF)
    dW = torch.einsum("hgcf,kgcf->hk", gz, x)
    g_xs = i["g_xs"] + i["Wt1"][:, :F].t() @ GzT
    xh = (i["Yp"] - i["mu"][:, None]) / torch.sqrt(i["var"] + EPS)[:, None]
    return dict(GzT=GzT, dWt1=dW, g_xs=g_xs, sg=g_xs.sum(1), sx=(g_xs * xh).sum(1))


def run_pair(hb, d, c, tm, fold):
    """One pair on the cuda inputs c -> every output, gradients from zero."""
    F = d.F
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    dWt1, dWs1, dWs2, dbs2 = z(2 * F, 2 * F), z(2 * F, 2 * F), z(2 * F, 2 * F), z(2 * F)
    dbt1, dg, db = z(2 * F), z(F), z(F)
    g_xs, g_xt = c["g_xs"].clone(), c["g_xt"].clone()
    GzT, _, part = hb.target_bwd(d, c["y"], c["sc"], c["sh"], c["Rs"], c["Wt1"], c["g_hsum"], dWt1,
                                 g_xs=g_xs, tmask=tm, bn_sums=(c["Yp"], c["mu"], c["var"], EPS),
                                 **({"fold": True} if fold else {}))
    out = hb.source_bwd(d, c["y"], c["sc"], c["sh"], c["Qt"], c["Ws1"], c["Ws2"], c["bs2"],
                        c["mean"], c["coef"], (c["Rs"], c["Wt1"], c["g_hsum"]), c["g_next"],
                        (c["mu1"], c["inv1"]), dWs1, dWs2, dbs2,
                        bn2=(c["gamma"], c["var1"], d.E, EPS, dg, db), g_xt=g_xt, tmask=tm,
                        **({"dWt1": dWt1} if fold else {}))
    hb.wgrad(GzT, c["xs"], dWt1, col0=0, db=dbt1)
    torch.cuda.synchronize()
    a, g0, g1 = out[4]
    psum = part.double().sum(0)
    return dict(g_tot=out[0], GzS=out[1], dWs1=dWs1, dWs2=dWs2, dbs2=dbs2, alpha=a, gam0=g0,
                gam1=g1, dgamma=dg, dbeta=db, g_xt=g_xt, GzT=GzT, g_xs=g_xs, part=part,
                sg=psum[:F], sx=psum[16:16 + F], dWt1=dWt1, dbt1=dbt1)


BITWISE = ["g_tot", "GzS", "dWs1", "dWs2", "dbs2", "alpha", "gam0", "gam1", "dgamma", "dbeta", "g_xt",
           "GzT", "g_xs", "part", "dWt1", "dbt1"]


@pytest.mark.parametrize("F,path", CASES)
@pytest.mark.parametrize("G,NF,NC", GEOMS)
def test_fold_matches_pair(hb, G, NF, NC, F, path):
    import pfsgnn
    from pfsgnn.engine import Dims
    prev = pfsgnn.get_edge_path()
    pfsgnn.set_edge_path(path)
    try:
        d = Dims(G, NF, NC, F)
        i = make_inputs(G, NF, NC, F)
        c = {k: cuda(v) for k, v in i.items()}
        tm = hb.tmask(d)
        assert tm is not None
        hb.target_fwd(d, c["y"], c["sc"], c["sh"], c["Rs"], c["Wt1"], tmask=tm)
        assert hb.tbwd_fold(d) == (F != 16)
        old = run_pair(hb, d, c, tm, False)
        new = run_pair(hb, d, c, tm, True)
        again = run_pair(hb, d, c, tm, True)
    finally:
        pfsgnn.set_edge_path(prev)
    ref = reference(i, G, NF, NC, F)
    for k in BITWISE:
        assert torch.equal(new[k], old[k]), k
    for k in new:   # run to run
        assert torch.equal(new[k], again[k]), k + " (run to run)"
    for k in ("GzT", "g_xs", "sg", "sx"):
        close(new[k], old[k], name=k + " vs pair")
        close(new[k], ref[k], name=k + " vs fp64")
    close(new["dWt1"][:, F:], old["dWt1"][:, F:], name="dWt1[:, F:2F] vs pair")
    close(new["dWt1"][:, F:], ref["dWt1"], name="dWt1[:, F:2F] vs fp64")
    close(new["dWt1"][:, :F], old["dWt1"][:, :F], name="dWt1[:, :F] vs pair")
    close(new["dWt1"][:, :F], ref["GzT"] @ i["xs"].t(), name="dWt1[:, :F] vs fp64")
    close(new["dbt1"], old["dbt1"], name="dbt1 vs pair")
    close(new["dbt1"], ref["GzT"].sum(1), name="dbt1 vs fp64")
