"""numpy reference of pfsgnn_schedule_plan (include/pfsgnn.h), written from the
definition: one Python loop per class, one per fiber, one per exposure.  No
sorting tricks, no prefix sums beyond the ones the definition names.

    r = observing_plan_ref(visits_in, edge_index, ci, total_time, nfields, NS, cap=True)

(``G``: also utility / over / worst per graph; ``segments=False`` leaves the
target list out -- an uncapped count near 2^24 is not listed exposure by
exposure.)

``ci`` is [NT, 2] (T, N) float32; ``NS`` the number of fibers.  Per-edge results
are in the caller's edge order.  Besides the op's outputs the result carries
what the tests assert branches on: ``w`` (the sanitised visits), ``S`` (class
sums before the cap), ``capc`` (-1: no cap), ``L`` / ``rem`` per class (-1 for
a class that was not trimmed), ``inert`` per edge, ``total`` (each fiber's
double time).
"""
import numpy as np

WMAX = 1 << 24


def class_cap(N, nfields):
    """cap_c per class as int64; -1: no cap (q >= 2^31)."""
    with np.errstate(all="ignore"):
        q = np.asarray(N, np.float32) / np.float32(nfields)     # one fp32 division
    out = np.zeros(q.size, np.int64)
    for c, v in enumerate(q):
        if np.isnan(v) or v < 0:
            out[c] = 0
        elif v >= np.float32(2.0 ** 31):
            out[c] = -1
        else:
            out[c] = int(np.floor(v))
    return out, q


def observing_plan_ref(visits_in, edge_index, ci, total_time, nfields, NS, cap=True, G=None,
                       segments=True):
    src, tgt = np.asarray(edge_index[0], np.int64), np.asarray(edge_index[1], np.int64)
    ci = np.asarray(ci, np.float32)
    NT, E = ci.shape[0], src.size
    T, N = ci[:, 0], ci[:, 1]
    total32 = float(np.float32(total_time))
    # 1. sanitise
    Te = T[tgt]
    inert = ~np.isfinite(Te) | ~(Te > 0)
    w = np.where(inert, 0, np.clip(np.asarray(visits_in, np.int64), 0, WMAX))
    vis = w.copy()
    # 2. class cap
    capc, q = class_cap(N, nfields)
    S = np.zeros(NT, np.int64)
    for e in range(E):
        S[tgt[e]] += w[e]
    cut = np.zeros(NT, np.int64)
    Ls, rems = np.full(NT, -1, np.int64), np.full(NT, -1, np.int64)
    if cap:
        for c in range(NT):
            if capc[c] < 0 or S[c] <= capc[c]:
                continue
            edges = [e for e in range(E) if tgt[e] == c]
            wc = w[edges]
            L = 0
            while np.minimum(wc, L + 1).sum() <= capc[c]:        # the largest L that fits
                # (a jump keeps the loop short for counts near 2^24)
                step = 1
                while np.minimum(wc, L + 2 * step).sum() <= capc[c]:
                    step *= 2
                L += step
            rem = int(capc[c] - np.minimum(wc, L).sum())
            above = sorted((e for e in edges if w[e] > L), key=lambda e: (src[e], e))
            assert rem < len(above)
            for k, e in enumerate(above):
                vis[e] = L + 1 if k < rem else L
            cut[c] = S[c] - capc[c]
            Ls[c], rems[c] = L, rem
    # 3. timeline
    start = np.zeros(E, np.float32)
    startd = np.zeros(E, np.float64)
    used, idle = np.zeros(NS, np.float32), np.zeros(NS, np.float32)
    total = np.zeros(NS, np.float64)
    cnt = np.zeros(NS, np.int64)
    per_fiber = [[] for _ in range(NS)]
    for e in range(E):
        per_fiber[src[e]].append(e)
    plan_order = []
    for f in range(NS):
        edges = sorted(per_fiber[f], key=lambda e: (tgt[e], e))
        plan_order.append(edges)
        run = 0.0
        for e in edges:
            startd[e] = run
            start[e] = np.float32(run)
            if vis[e]:
                run = run + float(vis[e]) * float(Te[e])
            cnt[f] += vis[e]
        total[f] = run
        used[f] = np.float32(run)
        idle[f] = np.float32(total32 - run)
    # 4. target list
    seg_ptr = np.zeros(NS + 1, np.int64)
    for f in range(NS):
        seg_ptr[f + 1] = seg_ptr[f] + cnt[f]
    nseg = seg_ptr[-1] if segments else 0          # (segments=False: the list is left out)
    seg_edge = np.zeros(nseg, np.int32)
    seg_start = np.zeros(nseg, np.float32)
    for f in range(NS if segments else 0):
        i = seg_ptr[f]
        for e in plan_order[f]:
            for m in range(vis[e]):
                seg_edge[i] = e
                seg_start[i] = np.float32(startd[e] + float(m) * float(Te[e]))
                i += 1
        assert i == seg_ptr[f + 1]
    # 5. aggregates
    n = np.zeros(NT, np.int64)
    for e in range(E):
        n[tgt[e]] += vis[e]
    n32 = n.astype(np.int32)
    with np.errstate(all="ignore"):
        comp = n32.astype(np.float32) / q
    out = dict(visits=vis.astype(np.int32), start=start, used=used, idle=idle, n=n32,
               completeness=comp, cut=cut, seg_ptr=seg_ptr, seg_edge=seg_edge, seg_start=seg_start,
               w=w, S=S, capc=capc, L=Ls, rem=rems, inert=inert, total=total)
    if G is not None:
        NF, NC = NS // G, NT // G
        out["utility"] = comp.reshape(G, NC).min(axis=1)
        out["over"] = (total.reshape(G, NF) > total32).sum(axis=1).astype(np.int32)
        out["worst"] = used.reshape(G, NF).max(axis=1)
    return out
