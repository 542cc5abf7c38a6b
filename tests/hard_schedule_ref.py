"""The hard (integer) schedule of an allocation, in plain torch (tests only).

train.py:50 keeps the hard count as a comment (``n = scatter(torch.floor(visited),
tgt, ...)``), train.py:74 announces "hard counts & diagnostics", and
train.py:256-257 rounds the best time to whole visits with ``np.round``.  The
form here indexes every edge by ``edge_index`` (include/pfsgnn.h,
pfsgnn_schedule), restated from ``oracle.ref_gnn.GNN.edge_prediction`` and
``oracle.ref_scatter.scatter``:

* ``time_e = softplus(decoder_e(x_e)) * total_time / NC``; ``v_e = time_e /
  T[tgt_e]``; ``visits_e = floor(v_e)`` or ``round(v_e)`` (half to even);
* ``n_c`` sums visits over ``tgt_e = c``; ``fiber_time_f`` sums ``visits_e *
  T[tgt_e]`` over ``src_e = f`` (``dim_size`` = every class / fiber: 0 without edges);
* ``completeness_c = n_c / (N_c / nfields)``; per graph ``utility`` = its
  minimum, ``over`` = fibers with ``fiber_time > total_time``, ``worst`` = the
  largest fiber time.

On a complete fiber-major batch it equals the positional form of train.py:40,
:50 (tests/test_hard_schedule_ref.py).
"""
import torch

from oracle.ref_scatter import scatter


def hard_schedule_ref(gnn, x_e, edge_index, class_info, G, NF, NC, rounding="floor",
                      total_time=42.0, nfields=10):
    """``x_e`` [E, F] in the caller's edge order (``edge_index`` [2, E], global
    node ids), in the dtype of ``gnn``; ``class_info`` [G*NC, >=2].  -> dict of
    visits [E] (int64), v (the quotient before rounding, in x_e's dtype), n
    [G*NC] (int64), fiber_time [G*NF], completeness [G*NC], utility / worst [G],
    over [G] (int64)."""
    src, tgt = edge_index[0].long(), edge_index[1].long()
    with torch.no_grad():
        time = gnn.edge_prediction(x_e, scale=total_time / NC).squeeze(-1)
        T_e = class_info[tgt, 0].to(time.dtype)
        v = time / T_e
        vis = torch.floor(v) if rounding == "floor" else torch.round(v)
        n = scatter(vis, tgt, G * NC, reduce="sum")
        fiber_time = scatter(vis * T_e, src, G * NF, reduce="sum")
        completeness = n / (class_info[:, 1].to(time.dtype) / nfields)
        ft = fiber_time.view(G, NF)
        return dict(visits=vis.long(), v=v, n=n.long(), fiber_time=fiber_time,
                    completeness=completeness,
                    utility=completeness.view(G, NC).min(dim=1).values,
                    over=(ft > total_time).sum(dim=1), worst=ft.max(dim=1).values)


def check_visits(name, visits, r64, r32, rounding, k=16.0):
    """The comparison rule for device visit counts against the float64
    reference ``r64`` (``r32``: the same reference run in float32 on the same
    inputs).  err32 = max |v32 - v64|, delta = k * err32 (k = 16, the factor of
    tests/test_gpu_sliced_ops.py).  An edge is decided when v64 is farther than
    delta from the nearest integer (floor) or half-integer (round); decided
    edges must match exactly, undecided ones may differ by at most 1.  Asserted
    on the reference first: undecided <= 1 % of the edges, >= 25 % of the edges
    with visits >= 1, >= 3 distinct values.  -> (err32, undecided count)."""
    v64, v32 = r64["v"].double(), r32["v"].double()
    err32 = (v32 - v64).abs().max().item()
    delta = k * err32
    w = v64 if rounding == "floor" else v64 - 0.5
    decided = (w - torch.round(w)).abs() > delta
    ref = r64["visits"]
    E, undec = ref.numel(), int((~decided).sum())
    print(f"{name}: E {E} err32 {err32:.3e} undecided {undec} "
          f"visits {int(ref.min())}..{int(ref.max())} "
          f">=1: {100.0 * (ref >= 1).double().mean().item():.1f} %")
    assert undec <= 0.01 * E, (name, undec, E)
    assert (ref >= 1).double().mean().item() >= 0.25, name
    assert ref.unique().numel() >= 3, name
    diff = (visits.detach().cpu().long().reshape(-1) - ref).abs()
    assert int(diff[decided].max()) == 0, (name, int((diff[decided] > 0).sum()))
    assert int(diff.max()) <= 1, name
    return err32, undec
