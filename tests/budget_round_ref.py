"""Budgeted rounding (largest-remainder apportionment per fiber) in numpy, int64
and float64 (tests only): steps 2-3 of pfsgnn_schedule_budget's definition in
include/pfsgnn.h, restated edge by edge.

Given the fp32 quotients ``q`` (step 1's output: ``min(max(time / T, 0), 2^24)``,
0 for an inert edge), ``edge_index``, ``ci`` and ``total_time``:

* ``base_e = floor(q_e)``, ``frac_e = q_e - floor(q_e)`` (exact in fp32);
* per fiber, with ``ft = sum visits_e * T_e`` in float64 and the key ``(frac_e,
  class, edge position)``: a **down phase** only if ``ft > total_time`` -- walk
  the edges in ascending key order, remove from each ``min(visits_e, k)`` visits
  with ``k`` the smallest integer such that ``ft - k T_e <= total_time``, stop
  once ``ft <= total_time`` (an edge that lost visits is *reduced*) -- then an
  **up phase** for every fiber: the edges that are neither inert nor reduced, in
  descending ``frac`` (ties: lower class, lower position), get ``+1`` iff ``ft +
  T_e <= total_time``.

An edge is inert when its class has a ``T`` that is not finite or ``<= 0``, or
when the caller marks it (a NaN time).  The walk is written as the definition
reads -- sort the fiber's edges by key, visit them one by one -- and also
records, per fiber, the phase bits (1: down phase, 2: bumped, 4: refused a
candidate) and the number of exact-budget ties (``ft + T == total_time``
accepted).
"""
import numpy as np


def quotient(time, T_e):
    """Step 1 on fp32 arrays: (q, inert)."""
    time, T_e = np.asarray(time, np.float32), np.asarray(T_e, np.float32)
    with np.errstate(all="ignore"):
        v = time / T_e
    inert = np.isnan(v) | ~(T_e > 0) | ~np.isfinite(T_e)
    q = np.minimum(np.maximum(v, np.float32(0)), np.float32(2.0 ** 24))
    q[inert] = 0
    return q.astype(np.float32), inert


def budget_round_ref(q, edge_index, ci, total_time, NS, inert=None):
    """``q`` fp32 [E]; ``edge_index`` [2, E] (global fiber / class ids); ``ci``
    [NT, >= 1] with T in column 0 (fp32 values); ``NS`` fibers.  -> dict of
    visits [E] int64, phase [NS] int32, ties [NS] int64, ft [NS] float64 (the
    double fiber time), reduced [E] bool, base [E] int64."""
    q = np.asarray(q)
    assert q.dtype == np.float32
    src, tgt = np.asarray(edge_index[0]).astype(np.int64), np.asarray(edge_index[1]).astype(np.int64)
    T = np.asarray(ci, np.float32)[:, 0].astype(np.float64)
    T_e = T[tgt]
    dead = ~(T_e > 0) | ~np.isfinite(T_e)
    if inert is not None:
        dead = dead | np.asarray(inert, bool)
    total = float(np.float32(total_time))
    base = np.floor(q)
    frac = (q - base).astype(np.float32)
    vis = base.astype(np.int64)
    vis[dead] = 0
    reduced = np.zeros(q.size, bool)
    phase, ties, fts = np.zeros(NS, np.int32), np.zeros(NS, np.int64), np.zeros(NS, np.float64)
    by_fiber = [[] for _ in range(NS)]
    for e in range(q.size):
        by_fiber[src[e]].append(e)
    for f, edges in enumerate(by_fiber):
        ft = 0.0
        for e in edges:
            if not dead[e]:
                ft += float(vis[e]) * T_e[e]
        if ft > total:
            phase[f] |= 1
            for e in sorted(edges, key=lambda e: (frac[e], tgt[e], e)):
                if ft <= total:
                    break
                if dead[e]:
                    continue
                k = int(np.ceil((ft - total) / T_e[e]))
                if k >= 1 and ft - (k - 1) * T_e[e] <= total:
                    k -= 1
                elif ft - k * T_e[e] > total:
                    k += 1
                r = min(int(vis[e]), k)
                if r > 0:
                    ft -= r * T_e[e]
                    vis[e] -= r
                    reduced[e] = True
        for e in sorted(edges, key=lambda e: (-frac[e], tgt[e], e)):
            if dead[e] or reduced[e]:
                continue
            if ft + T_e[e] <= total:
                ties[f] += ft + T_e[e] == total
                ft += T_e[e]
                vis[e] += 1
                phase[f] |= 2
            else:
                phase[f] |= 4
        fts[f] = ft
    return dict(visits=vis, phase=phase, ties=ties, ft=fts, reduced=reduced,
                base=base.astype(np.int64), frac=frac, dead=dead)
