"""The general-graph objective restated in tests/general_loss_ref.py equals the
reference objective (oracle/ref_train.py, train.py:29-80) on complete
fiber-major batches: float64, loss, diagnostics and gradients.  This pins the
yardstick of tests/test_gpu_sparse_loss.py.

Bound: both sides evaluate the same per-edge values; they differ only in the
order of float64 sums (index_add over edges vs torch.var / reshape reductions)
of at most NF*NC ~ 500 terms, i.e. a few hundred ulp (1.1e-16) of the largest
term: 1e-12 relative to the compared tensor's largest magnitude.
"""
import copy

import pytest
import torch

from general_loss_ref import general_loss
from harness import make_problem
from noise_ref import uniform_numpy
from oracle.ref_train import loss_function as ref_loss

REL = 1e-12


def _close(name, a, b):
    a, b = a.detach().double(), b.detach().double()
    scale = max(b.abs().max().item(), 1e-300)
    err = (a - b).abs().max().item()
    assert err <= REL * scale, f"{name}: err {err:.3e} > {REL:.0e} * {scale:.3e}"


@pytest.mark.parametrize("G,NF,NC,sharp", [(1, 40, 12, 12.0), (2, 24, 16, 5.0), (3, 10, 7, 0.0)])
def test_general_form_equals_reference_on_complete_fiber_major(G, NF, NC, sharp):
    model, graph = make_problem(G, NF, NC, B=1, seed=G + NF)
    E = G * NF * NC
    uni = torch.as_tensor(uniform_numpy(5, E), dtype=torch.float64)
    ci = graph.x_t
    runs = []
    for fn in ("ref", "general"):
        m = copy.deepcopy(model)
        xe = graph.x_e.clone().requires_grad_()
        if fn == "ref":
            loss, diag = ref_loss(m, xe, ci, G, NF, NC, pclass=0.1, pfiber=0.1, sharpness=sharp,
                                  uniform=uni)
            diag = {k: (torch.stack(v) if v[0].dim() == 0 else torch.cat(v))
                    for k, v in diag.items()}
        else:
            loss, diag = general_loss(m, xe, graph.edge_index, ci, G, NF, NC, pclass=0.1,
                                      pfiber=0.1, sharpness=sharp, uniform=uni)
        loss.backward()
        runs.append((loss, diag, xe.grad, {n: p.grad for n, p in m.named_parameters()}))
    (l0, d0, gx0, gp0), (l1, d1, gx1, gp1) = runs
    _close("loss", l1, l0)
    for k in ("utils", "n_prime", "fiber_time", "variance"):
        _close(k, d1[k], d0[k])
    _close("grad x_e", gx1, gx0)
    for n, g in gp0.items():
        assert (g is None) == (gp1[n] is None), n
        if g is not None:
            _close("grad " + n, gp1[n], g)


def test_general_form_degenerate_degrees():
    """deg(c) < 2 contributes 0 to the variance (no NaN), an edgeless fiber has
    fiber_time 0 and an edgeless class completeness 0."""
    model, graph = make_problem(1, 5, 3, B=1, seed=2)
    ei = torch.tensor([[0, 0, 1, 2, 3, 3, 0], [0, 1, 0, 1, 0, 2, 0]])   # class 2: one edge
    gen = torch.Generator().manual_seed(0)
    xe = 2.0 + 8.0 * torch.rand(ei.shape[1], 10, generator=gen, dtype=torch.float64)
    loss, d = general_loss(model, xe, ei, graph.x_t, 1, 5, 3, pclass=0.1, pfiber=0.1,
                           sharpness=4.0, uniform=torch.full((ei.shape[1],), 0.5,
                                                             dtype=torch.float64))
    assert torch.isfinite(loss)
    assert d["deg"].tolist() == [4.0, 2.0, 1.0]
    assert d["var_c"][2].item() == 0.0 and d["fiber_time"][4].item() == 0.0
    assert abs(d["variance"][0].item() - d["var_c"][:2].sum().item()) <= 1e-12 * d["variance"][0].abs().item()
