"""Crafted inputs for the observing-plan tests (tests/test_observing_plan_ref.py,
tests/test_gpu_observing_plan.py): seeded random visits on any edge list, and a
class_info built for them so that named branches of the class cap are reached.
Which class got which branch is returned, and ``assert_branches`` checks on the
reference's own result (tests/observing_plan_ref.py) that each was.
"""
import numpy as np

TOTAL_TIME, NFIELDS = 42.0, 10.0

BRANCHES = ("rem_pos", "rem_zero", "at_cap", "level_zero", "cap_zero", "cap_nan", "no_cap",
            "single_edge", "all_equal", "inert", "negative", "plain")


def level(wc, cap):
    """(L, rem) of the max-min fair trim by brute force."""
    L = 0
    while np.minimum(wc, L + 1).sum() <= cap:
        L += 1
    return L, int(cap - np.minimum(wc, L).sum())


def craft(ei, NS, NT, seed, first=0):
    """-> (visits_in int32 [E], ci float32 [NT, 2], {class: branch}, the fiber
    left without visits).  Integer T in 1..6; classes with fewer than 3 edges
    outside that fiber stay plain (a huge N)."""
    rng = np.random.default_rng(seed)
    src, tgt = np.asarray(ei[0]), np.asarray(ei[1])
    E = src.size
    vis = rng.integers(0, 5, E).astype(np.int64)
    T = rng.integers(1, 7, NT).astype(np.float32)
    N = np.full(NT, 1e6, np.float32)
    f0 = int(src[rng.integers(0, E)])
    vis[src == f0] = 0
    branch, b = {}, first
    for c in range(NT):
        edges = np.nonzero((tgt == c) & (src != f0))[0]
        if edges.size < 3:
            continue
        name = BRANCHES[b % len(BRANCHES)]
        b += 1
        branch[c] = name
        if name == "rem_pos":
            vis[edges] = rng.integers(1, 5, edges.size)
            wc = vis[edges]
            caps = [k for k in range(int(wc.sum()) - 1, 0, -1) if level(wc, k)[1] > 0]
            N[c] = caps[0] * NFIELDS + 3            # (floor drops the 0.3)
        elif name == "rem_zero":
            vis[edges[0]] = 4
            N[c] = np.minimum(vis[edges], 3).sum() * NFIELDS
        elif name == "at_cap":
            vis[edges[0]] = 2
            N[c] = vis[edges].sum() * NFIELDS
        elif name == "level_zero":
            vis[edges] = rng.integers(1, 5, edges.size)
            N[c] = (edges.size - 1) * NFIELDS
        elif name == "cap_zero":
            vis[edges[0]] = 3
            N[c] = 0.0
        elif name == "cap_nan":
            vis[edges[0]] = 3
            N[c] = np.nan
        elif name == "no_cap":
            N[c] = np.inf
        elif name == "single_edge":
            vis[edges] = rng.integers(0, 5, edges.size)
            vis[edges[1]] = 1 << 25                  # above 2^24: sanitised, then trimmed
            N[c] = (vis[edges].sum() - vis[edges[1]] + 7) * NFIELDS
        elif name == "all_equal":
            vis[edges] = 3
            N[c] = (2 * edges.size + 1) * NFIELDS
        elif name == "inert":
            vis[edges[0]] = 2
            T[c] = (0.0, np.inf, np.nan, -2.0)[c % 4]
        elif name == "negative":
            vis[edges[0]] = -5
            vis[edges[1]] = -(1 << 31)
    return vis.astype(np.int32), np.stack([T, N], 1), branch, f0


def assert_branches(r, ei, vis_in, branch, f0, need=()):
    """On the reference's result ``r``: every class reached the branch it was
    crafted for; ``need``: branches that must occur in this case."""
    src, tgt = np.asarray(ei[0]), np.asarray(ei[1])
    for c, name in branch.items():
        e = np.nonzero(tgt == c)[0]
        trimmed = r["L"][c] >= 0
        if name == "rem_pos":
            assert trimmed and r["rem"][c] > 0, (c, name)
        elif name == "rem_zero":
            assert trimmed and r["rem"][c] == 0 and r["L"][c] == 3, (c, name)
        elif name == "at_cap":
            assert not trimmed and r["S"][c] == r["capc"][c] > 0 and r["cut"][c] == 0, (c, name)
            assert np.array_equal(r["visits"][e], r["w"][e])
        elif name == "level_zero":
            assert trimmed and r["L"][c] == 0 and r["rem"][c] > 0, (c, name)
        elif name in ("cap_zero", "cap_nan"):
            assert r["capc"][c] == 0 and r["S"][c] > 0 and (r["visits"][e] == 0).all(), (c, name)
            assert r["cut"][c] == r["S"][c]
        elif name == "no_cap":
            assert r["capc"][c] == -1 and not trimmed, (c, name)
        elif name == "single_edge":
            assert trimmed and int((r["visits"][e] < r["w"][e]).sum()) == 1, (c, name)
            assert vis_in[e].max() > (1 << 24) and r["w"][e].max() == 1 << 24
        elif name == "all_equal":
            assert trimmed and r["L"][c] == 2 and r["rem"][c] == 1, (c, name)
            live = e[src[e] != f0]
            first = live[np.lexsort((live, src[live]))][0]
            assert r["visits"][first] == 3 and (r["visits"][live] == 2).sum() == live.size - 1
        elif name == "inert":
            assert r["inert"][e].all() and (r["visits"][e] == 0).all() and vis_in[e].max() > 0
        elif name == "negative":
            assert vis_in[e].min() < 0 and r["visits"][e].min() == 0, (c, name)
    for name in need:
        assert name in branch.values(), (name, sorted(set(branch.values())))
    assert r["seg_ptr"][f0 + 1] == r["seg_ptr"][f0] and r["used"][f0] == 0   # the empty range
