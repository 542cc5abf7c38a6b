"""The training objective on a GENERAL bipartite batch, in plain torch (tests only).

The reference objective (train.py:29-80) indexes edges by position, which only
means something on the complete fiber-major graph.  The general form indexes
by ``edge_index`` (include/pfsgnn.h, pfsgnn_loss_args' sl); it is restated here
from ``oracle.ref_scatter.scatter`` and ``oracle.ref_train.softfloor``:

* ``time_e = softplus(decoder_e(x_e)) * total_time / NC`` (train.py:42);
  ``T_e = class_info[tgt_e, 0]``; ``galaxies_e = max(0, softfloor(time_e / T_e))``;
  ``tt_e = galaxies_e * T_e``;
* ``n'_c`` sums galaxies over ``tgt_e = c``, ``fiber_time_f`` sums ``tt`` over
  ``src_e = f`` (``dim_size`` = every fiber / class: 0 without edges);
* ``utils_g`` = min over the graph's classes of ``n'_c / (N_c / nfields)``;
* ``variance_g`` = sum over the graph's classes of the unbiased variance of
  ``tt_e`` over the ``deg(c)`` edges of class c; 0 for ``deg(c) < 2`` (the one
  divergence from the reference, whose ``torch.var`` gives NaN there);
* class and fiber penalties and the sum over graphs as the reference.

On a complete fiber-major batch this equals ``oracle.ref_train.loss_function``
(tests/test_general_loss_ref.py).
"""
import torch
import torch.nn as nn

from oracle.ref_scatter import scatter
from oracle.ref_train import softfloor


def general_loss(gnn, x_e, edge_index, class_info, G, NF, NC, pclass=0.1, pfiber=1.0,
                 sharpness=0.5, total_time=42.0, nfields=10, wutils=2000.0, wvar=1.0,
                 uniform=None):
    """``x_e`` [E, F] and ``uniform`` [E] in the caller's edge order
    (``edge_index`` [2, E], global node ids); ``class_info`` [G*NC, >=2].
    -> (loss, diag): utils / variance [G], n_prime / completeness [G*NC],
    fiber_time [G*NF], time (tt) and raw (softfloor before the clamp) [E]."""
    src, tgt = edge_index[0].long(), edge_index[1].long()
    time = gnn.edge_prediction(x_e, scale=total_time / NC).squeeze(-1)
    T_e = class_info[tgt, 0]
    raw = softfloor(time / T_e, sharpness, uniform=uniform)
    galaxies = torch.maximum(torch.full_like(raw, 0.0), raw)
    tt = galaxies * T_e
    n_prime = scatter(galaxies, tgt, G * NC, reduce="sum")
    fiber_time = scatter(tt, src, G * NF, reduce="sum")
    N_i = class_info[:, 1] / nfields
    completeness = n_prime / N_i
    deg = scatter(torch.ones_like(tt), tgt, G * NC, reduce="sum")
    mean = scatter(tt, tgt, G * NC, reduce="sum") / deg.clamp(min=1)
    ssq = scatter((tt - mean[tgt]) ** 2, tgt, G * NC, reduce="sum")
    var_c = torch.where(deg >= 2, ssq / (deg - 1).clamp(min=1), torch.zeros_like(ssq))
    leaky = nn.LeakyReLU(negative_slope=0.1)
    losses, utils, variance = [], [], []
    for g in range(G):
        cs, fs = slice(g * NC, (g + 1) * NC), slice(g * NF, (g + 1) * NF)
        totutils = torch.min(completeness[cs])
        class_penalty = pclass * torch.sum(torch.relu(n_prime[cs] - N_i[cs]) ** 2)
        fiber_penalty = pfiber * torch.sum(leaky(fiber_time[fs] - total_time) ** 2)
        var_g = torch.sum(var_c[cs])
        losses.append(-wutils * totutils + fiber_penalty + class_penalty - wvar * var_g)
        utils.append(totutils.detach())
        variance.append(var_g.detach())
    diag = {"utils": torch.stack(utils), "variance": torch.stack(variance),
            "n_prime": n_prime.detach(), "fiber_time": fiber_time.detach(),
            "completeness": completeness.detach(), "time": tt.detach(), "raw": raw.detach(),
            "deg": deg.detach(), "var_c": var_c.detach()}
    return torch.stack(losses).sum(), diag
