"""Helper of tests/test_node_linalg_ref.py and tests/test_gpu_node_linalg.py:
cases, deterministic inputs, references and launch geometry of the dense node
linear algebra of csrc/pfsgnn_node.hip -- k_gemm / k_gemm_multi behind
pfsgnn_lin, _lin_t, _lin_cat, _lin_gather and _gemm_multi, k_wgrad /
k_wgrad_multi behind pfsgnn_wgrad, _wgrad_cat, _wgrad_cat_part, _wgrad_multi
and the deferred pass, k_reduce_rows / k_reduce_seg behind pfsgnn_reduce_batch,
and the small per-graph / per-channel ops.

References.  Every op runs on EmuBackend in float64 (ref64) and in float32
(ref32, the reference's own rounding).  The bf16x3 weight gradients have a
third one, refx3: the split product restated in torch and accumulated in
float64.  pfsgnn_reduce_batch's is a float64 sum over the partial axis.

Geometry.  gemm_ksm / gemm_mt, gemm_multi_shape, wgrad_blocks / wgrad_plan,
wg_x3_for and the reduce constants are restated here from the host code of
pfsgnn_node.hip; every case carries the branch it is named for (``want``) and
assert_reaches_branch holds the restated plan to it.

Two kinds of input per case.  ``exact``: every operand, bias and initial
output value a multiple of 1/8 with |v| <= 2, bscale / dbscale / scale powers of
two, act_in off: every product is a multiple of 1/64 and every partial sum
stays below 2^24 grid units, so every summation order -- fp32 MFMA, the bf16x3
split (five significant bits fit a bf16, lo = 0), the block partials and their
reduction -- is exact and the device must equal the reference bit for bit.
``random``: unit normal, act_in in both states, judged by bound().
"""
import collections
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "pfs-neural-net_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from emu_backend import EmuBackend, lrelu  # noqa: E402

SENT = -12345.5          # sentinel of guard bands no kernel may write
PLAN_KNOBS = ("PFSGNN_WG_BLOCKS", "PFSGNN_WG_X3_MIN_TM", "PFSGNN_NODE_WG_X3")

# ------------------------------------------------------------------ geometry
KSMS = (1, 3, 5, 8, 10, 16, 25, 40)      # PF_GEMM_KSM: K-steps of 4 instantiated
MT_MAX, KI_MAX, MO_MAX = 11, 160, 176
GM_MULTI, GM_KI_MAX, GM_M_MAX = 4, 40, 64   # k_gemm_multi: jobs per launch, widest job
GMM_SHAPES = tuple((mt, ks) for mt in (1, 2, 3, 4) for ks in (3, 5, 10))   # PF_GMM_ALL
WG_WAVES, WG_LD, WG_MULTI = 8, 68, 24
WG_ALL = ((1, 1), (1, 2), (1, 4), (1, 8), (2, 1), (2, 2), (2, 4), (2, 8), (2, 16), (4, 1), (4, 2),
          (4, 4), (4, 8), (4, 16), (8, 1), (8, 2), (8, 4), (8, 8), (8, 16), (16, 1), (16, 2), (16, 4),
          (16, 8), (16, 16))   # PF_WG_ALL
RED_SEG, PF_MAX_RED = 256, 96
RED_ROWS_MAX, RED_COLS_MAX = 65535, 32767    # the packed 40-byte descriptor


def gemm_ksm(Ki):
    ks = (Ki + 3) // 4
    for v in KSMS:
        if ks <= v:
            return v
    return -1


def gemm_mt(Mo):
    return (Mo + 15) // 16


def gemm_lds(Mo, Ki):
    return gemm_mt(Mo) * 16 * (4 * gemm_ksm(Ki) + 1) * 4


def gemm_multi_shape(jobs):
    """(mt, ks) of one k_gemm_multi launch over [(Mo, Ki)] (at most GM_MULTI)."""
    mt, ks = 1, 3
    for Mo, Ki in jobs:
        mt = max(mt, gemm_mt(Mo))
        k4 = (Ki + 3) // 4
        ks = max(ks, 3 if k4 <= 3 else 5 if k4 <= 5 else 10)
    return mt, ks


def wgrad_blocks(N):
    return max(1, min((N + 399) // 400, 256))


def wgrad_plan(M, K, N, has_db, aligned=True):
    """wgrad_plan of pfsgnn_node.hip -> dict, or the text of its refusal.
    ``aligned``: dY and every per-node block start 16-byte aligned."""
    if M > 256 or K > 256:
        return "M, K too large"
    nbk = wgrad_blocks(N)
    K1 = K + (1 if has_db else 0)
    chunk = ((N + nbk - 1) // nbk + 63) // 64 * 64
    nblk = (N + chunk - 1) // chunk
    MR, KR = (M + 15) & ~15, (K1 + 15) & ~15
    ntile = (MR // 16) * (KR // 16)
    items = (M + K1) * 16
    per = 1 if items <= 512 else 2 if items <= 1024 else 4 if items <= 2048 else 8 if items <= 4096 else 16
    if items > 16 * 64 * WG_WAVES:
        return "M + K too large"
    tm = next((t for t in (1, 2, 4, 8, 16) if ntile <= t * WG_WAVES), -1)
    if tm < 0:
        return "too many output tiles"
    last = N - (nblk - 1) * chunk
    return dict(K1=K1, chunk=chunk, nblk=nblk, tm=tm, per=per, ntile=ntile,
                vec=1 if (N % 4 == 0 and aligned) else 0, lds=(MR + KR) * WG_LD * 4,
                part_bytes=nblk * M * K1 * 4, last=last, last_chunks=(last + 63) // 64)


def wg_x3_for(tm, per, path):
    """bf16x3 weight gradient?  (pf::node_x3: every edge path but the exact-fp32 ones)"""
    return tm >= 4 and not (tm == 16 and per == 16) and path not in ("mfma32", "valu", "bf16y")


def wg_deep(tm, per):
    """wgrad_block's DEEP: the X3 form with two chunks of loads in flight."""
    return per <= 8 and tm <= 8


def reachable_wg_pairs(limit=256):
    """{(tm, per)} the plan yields over every M, K <= limit, with and without db."""
    out = {}
    for M in range(1, limit + 1):
        for K in range(1, limit + 1):
            for db in (0, 1):
                p = wgrad_plan(M, K, 64, db)
                if isinstance(p, dict):
                    out.setdefault((p["tm"], p["per"]), (M, K, db))
    return out


REACHABLE_WG = ((1, 1), (1, 2), (1, 4), (1, 8), (2, 4), (2, 8), (2, 16), (4, 4), (4, 8), (4, 16),
                (8, 8), (8, 16), (16, 8), (16, 16))
# instantiated, never selected by the plan
UNREACHABLE_WG = ((2, 1), (2, 2), (4, 1), (4, 2), (8, 1), (8, 2), (8, 4), (16, 1), (16, 2), (16, 4))


# ------------------------------------------------------------------ inputs
def f32(t):
    return t.float().double()


def grid(gen, *shape):
    """Multiples of 1/8 in [-2, 2]."""
    return torch.randint(-16, 17, shape, generator=gen).double() / 8


def rnd(gen, *shape):
    return f32(torch.randn(*shape, generator=gen, dtype=torch.float64))


def draw(kind, gen, *shape):
    return grid(gen, *shape) if kind == "exact" else rnd(gen, *shape)


def seed_of(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100003


# ------------------------------------------------------------------ GEMM cases
# op lin:     Y[M][N] = W[:, col0:col0+K] . act(X[K][N]) + bscale b       (Mo, Ki) = (M, K)
# op lin_t:   out[K][N] = W[:, col0:col0+K]^T . dY[M][N] (* lrelu'(Z))    (Mo, Ki) = (K, M)
# op lin_cat: Y[M][N] = sum_s W[:, col_s..] . act(X_s) + bscale b, blocks (rows, kind) with
#             kind "n" [rows][N] or "g" [rows][G] broadcast over the N / G nodes of a graph
Gemm = collections.namedtuple("Gemm", "name op M K N blocks G col0 pad b bscale add z want")


def _gemm(name, op, M, K, N, blocks=None, G=1, col0=0, pad=0, b=True, bscale=1.0, add=False,
          z=False, **want):
    return Gemm(name, op, M, K, N, blocks, G, col0, pad, b, bscale, add, z, want)


def _gemm_cases():
    out = []
    # (Mo, Ki): every MT 1..11 and every KSM, Ki on both sides of each KSM step, Mo at 16 | 17
    # and at 176; N cycles through the nc = N - 1 clamp (1), a last block with one valid
    # wave (65, 130), a full block (64) and a ragged one (63)
    shapes = [(16, 12, 3), (17, 13, 5), (33, 20, 5), (49, 21, 8), (65, 32, 8), (81, 33, 10),
              (97, 40, 10), (113, 41, 16), (129, 64, 16), (145, 65, 25), (161, 100, 25),
              (176, 101, 40), (10, 160, 40), (3, 4, 1), (100, 157, 40), (176, 160, 40)]
    Ns = (1, 63, 64, 65, 130)
    for i, (Mo, Ki, ksm) in enumerate(shapes):
        N = Ns[i % 5]
        mt = gemm_mt(Mo)
        out.append(_gemm(f"lin-{Mo}x{Ki}-N{N}", "lin", Mo, Ki, N, col0=i % 3, pad=(i + 1) % 3,
                         b=i % 4 != 3, bscale=(1.0, 2.0, 0.5)[i % 3], add=i % 2 == 1, mt=mt, ksm=ksm))
        N = Ns[(i + 2) % 5]
        out.append(_gemm(f"lin_t-{Mo}x{Ki}-N{N}", "lin_t", Ki, Mo, N, col0=(i + 1) % 3, pad=i % 3,
                         add=i % 2 == 0, z=i % 3 != 2, mt=mt, ksm=ksm))
    # lin_cat: 1..4 blocks, the per-graph block first / in the middle / last, per_graph in
    # {1, N / G, N}, gap columns between the blocks (pad) and ldw > K
    cat = [("one", [(7, "n")], 65, 1), ("bc-last", [(10, "n"), (80, "n"), (10, "g")], 130, 2),
           ("bc-first", [(3, "g"), (5, "n")], 63, 63), ("bc-middle", [(3, "n"), (5, "g"), (7, "n"), (2, "n")], 64, 1),
           ("bc-only", [(12, "g")], 130, 5), ("two-bc", [(4, "g"), (9, "n"), (4, "g")], 130, 13),
           ("wide", [(40, "n"), (40, "g"), (40, "n"), (40, "n")], 65, 5)]
    for i, (nm, blocks, N, G) in enumerate(cat):
        K = sum(rows for rows, _ in blocks)
        M = (20, 100, 17, 40, 33, 64, 176)[i]
        out.append(_gemm(f"lin_cat-{nm}", "lin_cat", M, K, N, blocks=blocks, G=G, pad=1 + i % 2,
                         b=i % 3 != 1, bscale=(1.0, 2.0)[i % 2], add=i % 2 == 1,
                         mt=gemm_mt(M), ksm=gemm_ksm(K), per_graph=N // G))
    return out


GEMM_CASES = _gemm_cases()


def gemm_dims(c):
    """(Mo, Ki) of a GEMM case."""
    return (c.K, c.M) if c.op == "lin_t" else (c.M, c.K)


def gemm_layout(c):
    """-> (ldw, [weight column of each block])."""
    if c.blocks is None:
        return c.col0 + c.K + c.pad, [c.col0]
    cols, col = [], c.col0
    for rows, _ in c.blocks:
        cols.append(col)
        col += rows + c.pad         # pad gap columns after every block
    return col, cols


def gemm_inputs(c, kind):
    gen = torch.Generator().manual_seed(seed_of(c.name) + (kind == "exact"))
    ldw, cols = gemm_layout(c)
    Mo, Ki = gemm_dims(c)
    i = dict(W=draw(kind, gen, c.M, ldw))
    if c.op == "lin_t":
        i["X"] = [draw(kind, gen, c.M, c.N)]
        i["Z"] = draw(kind, gen, c.K, c.N) if c.z else None
        i["b"] = None
    else:
        blocks = c.blocks or [(c.K, "n")]
        i["X"] = [draw(kind, gen, rows, c.G if k == "g" else c.N) for rows, k in blocks]
        i["Z"] = None
        i["b"] = draw(kind, gen, c.M) if c.b else None
    # lin / lin_cat accumulate onto a non-grid Y0 also in the exact kind: the exact sum plus Y0
    # is one IEEE addition, restated in float32 (lin_t's Y0 stays on the grid: its * lrelu'(Z)
    # is the one more operation there)
    i["Y0"] = (rnd(gen, Mo, c.N) if c.op != "lin_t" else draw(kind, gen, Mo, c.N)) if c.add else None
    return i


def run_gemm(be, c, i, act_in, conv, out=None, mutant=None):
    """The case on backend ``be`` (EmuBackend or HipBackend) -> Y.  ``out``: the
    output buffer (holding Y0 where the case accumulates), else a new tensor."""
    W, X, b = conv(i["W"]), [conv(x) for x in i["X"]], conv(i["b"])
    Z = conv(i["Z"]) if c.z else None
    _, cols = gemm_layout(c)
    add = c.add and mutant != "add_overwrites"
    bscale = 1.0 if mutant == "bscale_ignored" else c.bscale
    act = act_in and mutant != "act_in_ignored"
    if out is None and c.add:
        out = conv(i["Y0"])
    if c.op == "lin":
        return be.lin(W, c.col0, c.K, X[0], b=b, act_in=act, out=out, add=add, bscale=bscale)
    if c.op == "lin_t":
        return be.lin_t(W, c.col0, c.K, X[0], z=Z, out=out, add=add)
    if mutant == "segment_column_off_by_one":
        cols = cols[:-1] + [cols[-1] + 1]
    segs = [(x, col, k == "g") for x, col, (_, k) in zip(X, cols, c.blocks)]
    if mutant == "broadcast_next_graph":   # node n reads graph (n + 1) / npg
        npg = c.N // c.G
        g = ((torch.arange(c.N) + 1) // npg).clamp(max=c.G - 1)
        segs = [(x[:, g] if bc else x, col, False) for x, col, bc in segs]
    return be.lin_cat(W, segs, c.N, b=b, act_in=act, out=out, add=add, bscale=bscale)


def ref_gemm(c, i, act_in, dtype=torch.float64, mutant=None):
    return run_gemm(EmuBackend(dtype), c, i, act_in, lambda t: None if t is None else t.to(dtype).clone(),
                    mutant=mutant)


def gemm_abs_terms(c, i):
    """sum |terms| of every output element, largest (the exactness proof)."""
    a = {k: (None if t is None else [x.abs() for x in t] if isinstance(t, list) else t.abs())
         for k, t in i.items()}
    a["Z"] = None
    return ref_gemm(c._replace(z=False), a, False).max().item()


# ------------------------------------------------------------------ lin_gather
Gather = collections.namedtuple("Gather", "name M K N ld ngather refused")
GATHER_CASES = [Gather("gather0-65x65", 65, 65, 65, (), 0, False),
                Gather("gather1", 40, 12, 130, (7,), 1, False),
                Gather("gather2", 20, 33, 63, (63, 200), 2, False),
                Gather("gather2-64x64", 64, 64, 65, (9, 130), 2, False),
                Gather("gather1-M65", 65, 12, 64, (5,), 1, True),
                Gather("gather1-K65", 12, 65, 64, (5,), 1, True)]


def gather_inputs(c, kind):
    gen = torch.Generator().manual_seed(seed_of(c.name) + (kind == "exact"))
    i = dict(W=draw(kind, gen, c.M, c.K + 2), X=draw(kind, gen, c.K, c.N), b=draw(kind, gen, c.M),
             G=[draw(kind, gen, c.M, ld) for ld in c.ld], idx=[])
    for ld in c.ld:     # repeats and both extremes 0 and ld - 1
        idx = torch.randint(0, ld, (c.N,), generator=gen, dtype=torch.int32)
        idx[0], idx[-1] = ld - 1, 0
        if c.N > 3:
            idx[1] = idx[2] = ld // 2
        i["idx"].append(idx)
    return i


def run_gather(be, c, i, conv, mutant=None):
    idx = [i["idx"][0]] * len(i["idx"]) if mutant == "gather_idx1_for_both" else i["idx"]
    if mutant == "gather_idx1_for_both":
        idx = [x.clamp(max=ld - 1) for x, ld in zip(idx, c.ld)]
    gathers = [(conv(g), conv(x)) for g, x in zip(i["G"], idx)]
    return be.lin_gather(conv(i["W"]), 1, c.K, conv(i["X"]), gathers, b=conv(i["b"]))


def ref_gather(c, i, dtype=torch.float64, mutant=None):
    def conv(t):
        return t.clone() if t.dtype == torch.int32 else t.to(dtype).clone()
    return run_gather(EmuBackend(dtype), c, i, conv, mutant=mutant)


# ------------------------------------------------------------------ gemm_multi
# a batch: jobs ("cat", M, blocks, N, G, b) or ("t", Mw, ncol, N, add) through linear_batch
Batch = collections.namedtuple("Batch", "name jobs want")


def _batch_cases():
    out = []
    Kof = {3: 12, 5: 20, 10: 40}
    Ns = (64, 65, 1, 130)
    for n, (mt, ks) in enumerate(GMM_SHAPES):
        Mw, Kw = 16 * mt - (n % 2), Kof[ks] - (n % 3)
        assert gemm_multi_shape([(Mw, Kw)]) == (mt, ks)
        njob = (1, 4, 5, 9)[n % 4]
        jobs = []
        for j in range(njob):
            N = Ns[(n + j) % 4]
            if j == (njob - 1) // 2:          # the widest job, not the first of its launch
                M, K = Mw, Kw
            else:                             # narrower: rows and K-steps of zero padding
                M, K = max(1, Mw - 5 * j - 3), max(1, Kw - 3 * j - 2)
            if j % 3 == 2:                    # out[K][N] (+)= W[M][..K]^T dY[M][N]: (Mo, Ki) = (K, M)
                jobs.append(("t", K, M, N, j % 2 == 0))
            else:
                G = (1, N, 5 if N % 5 == 0 else 1)[j % 3]
                blocks = [(K, "n")] if K < 3 or j % 2 else [(K - 2, "n"), (2, "g")]
                jobs.append(("cat", M, blocks, N, G, (n + j) % 3 != 0))
        out.append(Batch(f"batch-mt{mt}-ks{ks}-{njob}jobs", jobs, dict(mt=mt, ks=ks, njob=njob)))
    return out


BATCH_CASES = _batch_cases()


def batch_job_dims(job):
    """(Mo, Ki) of a batch job."""
    if job[0] == "t":
        return job[2], job[1]
    return job[1], sum(rows for rows, _ in job[2])


def batch_launches(c):
    """[(mt, ks)] of the launches of a batch (GM_MULTI jobs each)."""
    d = [batch_job_dims(j) for j in c.jobs]
    return [gemm_multi_shape(d[k:k + GM_MULTI]) for k in range(0, len(d), GM_MULTI)]


def batch_inputs(c, kind):
    gen = torch.Generator().manual_seed(seed_of(c.name) + (kind == "exact"))
    out = []
    for job in c.jobs:
        if job[0] == "t":
            _, Mw, ncol, N, add = job
            out.append(dict(W=draw(kind, gen, Mw, ncol + 2), dY=draw(kind, gen, Mw, N),
                            Y0=draw(kind, gen, ncol, N) if add else None))
        else:
            _, M, blocks, N, G, b = job
            K = sum(rows for rows, _ in blocks)
            out.append(dict(W=draw(kind, gen, M, K + 1), b=draw(kind, gen, M) if b else None,
                            X=[draw(kind, gen, rows, G if k == "g" else N) for rows, k in blocks]))
    return out


def batch_ops(c, inp, conv, mutant=None):
    """linear_batch's op list (fresh output tensors for the accumulating jobs)."""
    ops = []
    for n, (job, i) in enumerate(zip(c.jobs, inp)):
        if job[0] == "t":
            _, Mw, ncol, N, add = job
            ops.append(("t", conv(i["W"]), 1, ncol, conv(i["dY"]), conv(i["Y0"]) if add else None, add))
        else:
            _, M, blocks, N, G, b = job
            segs, col = [], 0
            for x, (rows, k) in zip(i["X"], blocks):
                segs.append((conv(x), col, k == "g"))
                col += rows
            bias = i["b"]
            if mutant == "neighbour_bias":     # the bias of the next "cat" job of the same height
                for m in range(n + 1, len(c.jobs)):
                    if c.jobs[m][0] == "cat" and inp[m]["b"] is not None and bias is not None \
                            and inp[m]["b"].numel() >= bias.numel():
                        bias = inp[m]["b"][:bias.numel()]
                        break
            ops.append(("cat", conv(i["W"]), segs, N, conv(bias)))
    return ops


def ref_batch(c, inp, dtype=torch.float64, mutant=None):
    conv = lambda t: None if t is None else t.to(dtype).clone()  # noqa: E731
    return EmuBackend(dtype).linear_batch(batch_ops(c, inp, conv, mutant))


# ------------------------------------------------------------------ weight gradients
# dW[:, col_s..] += dY . act(X_s)^T, db += dbscale sum_n dY.  blocks as for lin_cat;
# misalign: None, "dY", "seg" (block 0 starts one float into an aligned buffer: vec off)
# or "bc" (the per-graph block does: vec stays on)
Wg = collections.namedtuple("Wg", "name M blocks N G db dbscale col0 pad misalign want")


def _wg(name, M, blocks, N, G=1, db=True, dbscale=1.0, col0=0, pad=0, misalign=None, **want):
    if isinstance(blocks, int):
        blocks = [(blocks, "n")]
    return Wg(name, M, blocks, N, G, db, dbscale, col0, pad, misalign, want)


# one (M, K, db) per reachable (tm, per) pair
WG_TABLE = {(1, 1): (3, 7, 0), (1, 2): (16, 16, 1), (1, 4): (10, 100, 1), (1, 8): (1, 127, 1),
            (2, 4): (40, 40, 1), (2, 8): (250, 5, 1), (2, 16): (10, 250, 0), (4, 4): (33, 80, 1),
            (4, 8): (96, 79, 1), (4, 16): (17, 239, 1), (8, 8): (100, 100, 1), (8, 16): (33, 223, 1),
            (16, 8): (136, 119, 1), (16, 16): (160, 160, 1)}


def _wg_cases():
    out = []
    Ns = (129, 65, 401, 37, 400, 63, 64, 801, 130, 3, 2001, 1, 2100, 65)
    for n, ((tm, per), (M, K, db)) in enumerate(WG_TABLE.items()):
        out.append(_wg(f"wg-tm{tm}-per{per}-N{Ns[n]}", M, K, Ns[n], db=bool(db),
                       dbscale=(1.0, 2.0, 0.5)[n % 3], col0=n % 3, pad=n % 2, tm=tm, per=per))
    # tile-count edges: ntile 8 | 9, 16 | 17, 32 | 33, 64 | 65 (K1 = K + 1 with db)
    # (ntile 17 = 1 x 17 needs K1 = 257: (tm, per) = (4, 16), the first count past the tm 2 -> 4
    # step, a last wave with a partial run of tiles; 18 = 2 x 9 is the same step at per 8)
    for M, K, db, ntile in [(32, 63, 1, 8), (48, 47, 1, 9), (64, 63, 1, 16), (16, 256, 1, 17),
                            (17, 143, 0, 18), (64, 127, 1, 32), (48, 175, 1, 33), (128, 127, 1, 64), (80, 207, 0, 65)]:
        out.append(_wg(f"wg-ntile{ntile}", M, K, 130, db=bool(db), ntile=ntile))
    # M and K1 at 16 | 17
    out.append(_wg("wg-M16-K1-16", 16, 15, 65, ntile=1))
    out.append(_wg("wg-M17-K1-17", 17, 16, 65, ntile=4))
    # the node range: one chunk, a partial chunk, one / two / three chunks per block (the DEEP
    # prefetch of the X3 form: (8, 8) is DEEP, (8, 16) is not), nblk 1 | 2 | 3 | 6, a last block
    # of 145 (N 401 = 256 + 145), 161 (801 = 2 x 320 + 161), 81 (2001 = 5 x 384 + 81) and 180
    # nodes (2100 = 5 x 384 + 180)
    for N, nblk in [(1, 1), (3, 1), (37, 1), (63, 1), (64, 1), (65, 1), (129, 1), (400, 1), (401, 2),
                    (801, 3), (2001, 6), (2100, 6)]:
        out.append(_wg(f"wg-deep-N{N}", 100, 100, N, nblk=nblk, tm=8, per=8))
        if N in (1, 37, 65, 129, 401, 2100):
            out.append(_wg(f"wg-flat-N{N}", 33, 223, N, nblk=nblk, tm=8, per=16))
            out.append(_wg(f"wg-fp32-N{N}", 10, 100, N, nblk=nblk, tm=1, per=4))
    # alignment: vec off by a dY or a block one float into an aligned buffer; a misaligned
    # per-graph block leaves it on
    for mis, vec in (("dY", 0), ("seg", 0), ("bc", 1)):
        out.append(_wg(f"wg-misaligned-{mis}", 33, [(70, "n"), (10, "g")], 400, G=8, misalign=mis,
                       vec=vec, tm=4, per=4))
        out.append(_wg(f"wg-misaligned-{mis}-fp32", 10, [(30, "n"), (10, "g")], 400, G=8,
                       misalign=mis, vec=vec, tm=1))
    # per-graph blocks whose graph boundary falls inside a float4 item and inside a chunk
    for npg, N in ((1, 130), (3, 129), (50, 400), (401, 401)):
        out.append(_wg(f"wg-bc-npg{npg}", 40, [(10, "g"), (20, "n"), (9, "g")], N, G=N // npg,
                       dbscale=0.5, col0=1, pad=1, per_graph=npg))
        out.append(_wg(f"wg-bc-npg{npg}-x3", 96, [(10, "g"), (60, "n"), (9, "g")], N, G=N // npg,
                       db=npg != 3, pad=2, per_graph=npg, tm=4, per=8))
    # four blocks with gap columns, as SModel's / TModel's concatenations
    out.append(_wg("wg-cat4", 100, [(10, "n"), (70, "n"), (10, "n"), (10, "g")], 801, G=3, pad=1,
                   dbscale=2.0, tm=8, per=8, nblk=3))
    return out


WG_CASES = _wg_cases()
WG_REFUSALS = [("M, K too large", 257, 3, 64, True), ("M, K too large", 3, 257, 64, False),
               ("M \\+ K too large", 256, 256, 64, True), ("too many output tiles", 255, 256, 64, False),
               ("too many output tiles", 192, 192, 64, True)]


def wg_K(c):
    return sum(rows for rows, _ in c.blocks)


def wg_layout(c):
    """-> (lddw, [weight column of each block])."""
    cols, col = [], c.col0
    for rows, _ in c.blocks:
        cols.append(col)
        col += rows + c.pad
    return col, cols


def wg_plan(c):
    return wgrad_plan(c.M, wg_K(c), c.N, c.db, aligned=c.misalign in (None, "bc"))


def wg_inputs(c, kind):
    gen = torch.Generator().manual_seed(seed_of(c.name) + (kind == "exact"))
    lddw, _ = wg_layout(c)
    return dict(dY=draw(kind, gen, c.M, c.N),
                X=[draw(kind, gen, rows, c.G if k == "g" else c.N) for rows, k in c.blocks],
                dW0=draw(kind, gen, c.M, lddw), db0=draw(kind, gen, c.M) if c.db else None)


def wg_segs(c, X):
    _, cols = wg_layout(c)
    return [(x, col, k == "g") for x, col, (_, k) in zip(X, cols, c.blocks)]


def run_wg(be, c, i, act_in, conv, dW=None, db=None, X=None, dY=None, mutant=None):
    """wgrad (one plain block) or wgrad_cat on ``be`` -> dict(dW, db).  dW / db / X /
    dY: device buffers the caller laid out itself (guard bands, misalignment)."""
    dY = conv(i["dY"]) if dY is None else dY
    X = [conv(x) for x in i["X"]] if X is None else X
    dW = conv(i["dW0"]) if dW is None else dW
    db = (conv(i["db0"]) if db is None else db) if c.db else None
    act = act_in and mutant != "act_in_ignored"
    dbscale = 1.0 if mutant == "dbscale_ignored" else c.dbscale
    if mutant in ("last_node_dropped", "last_chunk_dropped"):
        p = wg_plan(c)
        first = (c.N - 1) if mutant == "last_node_dropped" else (p["nblk"] - 1) * p["chunk"] + (p["last_chunks"] - 1) * 64
        dY = dY.clone()
        dY[:, first:] = 0
    segs = wg_segs(c, X)
    if mutant == "segment_column_off_by_one":
        segs = segs[:-1] + [(segs[-1][0], segs[-1][1] + 1, segs[-1][2])]
    if mutant == "broadcast_next_graph":
        npg = c.N // c.G
        g = ((torch.arange(c.N) + 1) // npg).clamp(max=c.G - 1)
        segs = [(x[:, g] if bc else x, col, False) for x, col, bc in segs]
    if len(c.blocks) == 1 and mutant is None:
        be.wgrad(dY, X[0], dW, col0=c.col0, db=db, act_in=act, dbscale=dbscale)
    else:
        be.wgrad_cat(dY, segs, dW, db=db, act_in=act, dbscale=dbscale)
    return dict(dW=dW, db=db) if c.db else dict(dW=dW)


def ref_wg(c, i, act_in, dtype=torch.float64, mutant=None):
    return run_wg(EmuBackend(dtype), c, i, act_in, lambda t: None if t is None else t.to(dtype).clone(),
                  mutant=mutant)


def split_bf16(x):
    """The round-to-nearest split of pf_split4 (csrc/pfsgnn_common.h): hi = bf16(x),
    lo = bf16(x - hi), both as float32 values held in float64."""
    hi = x.float().bfloat16().float()
    lo = (x.float() - hi).bfloat16().float()
    return hi.double(), lo.double()


def refx3_wg(c, i, act_in):
    """The bf16x3 weight gradient restated: hi hi' + hi lo' + lo hi' accumulated in
    float64 (the device accumulates in fp32); db an exact sum, not split."""
    out = ref_wg(c, i, act_in)
    dW = i["dW0"].clone()
    dh, dl = split_bf16(i["dY"])
    for x, col, bc in wg_segs(c, i["X"]):
        xa = f32(lrelu(x)) if act_in else x
        if bc:
            xa = xa.repeat_interleave(c.N // c.G, dim=1)
        xh, xl = split_bf16(xa)
        dW[:, col:col + x.shape[0]] += dh @ xh.t() + dh @ xl.t() + dl @ xh.t()
    out["dW"] = dW
    return out


def wg_blocks_of(c, out):
    """The blocks a weight gradient is judged by: each input block's columns of dW,
    db, and ``rest`` (the gap columns: untouched)."""
    _, cols = wg_layout(c)
    dW = out["dW"]
    blocks, keep = {}, torch.ones(dW.shape[1], dtype=torch.bool)
    for s, ((rows, _), col) in enumerate(zip(c.blocks, cols)):
        blocks[f"dW.s{s}"] = dW[:, col:col + rows]
        keep[col:col + rows] = False
    blocks["dW.rest"] = dW[:, keep]
    if c.db:
        blocks["db"] = out["db"]
    return blocks


def wg_abs_terms(c, i):
    a = dict(dY=i["dY"].abs(), X=[x.abs() for x in i["X"]], dW0=i["dW0"].abs(),
             db0=None if i["db0"] is None else i["db0"].abs())
    o = ref_wg(c._replace(dbscale=abs(c.dbscale)), a, False)
    return max(t.max().item() for t in o.values())


# ------------------------------------------------------------------ the deferred pass
DEFER_MAIN = (1, 2)      # the (tm, per) of defer_jobs' counted jobs


def defer_jobs(njob):
    """njob weight gradients of the (1, 2) kernel shape -- njob = 24, 25 and 50 sit at,
    past and two launches past k_wgrad_multi's WG_MULTI table -- differing in M, K,
    N and LDS size, with jobs of the X3 shapes (4, 4) / (2, 4) and (8, 8) interleaved
    in job order, so that the launch groups are non-contiguous -> [(Wg, target)]: jobs
    with the same target share a dW (target "same": the same cells; "adj0" / "adj1":
    adjacent column blocks of one dW)."""
    def job(name, M, K, N, n):
        G = 5 if N % 5 == 0 else 1
        return _wg(name, M, [(K - 4, "n"), (4, "g")] if n % 2 else K, N, G=G, db=n % 4 != 3,
                   dbscale=(1.0, 0.5)[n % 2])

    out = []
    for j in range(njob):
        out.append((job(f"defer{len(out)}", 10 - j % 3, 30 + j % 5, (65, 401, 130)[j % 3], j), f"own{len(out)}"))
        if njob >= 5 and j % 4 == 1:
            out.append((job(f"defer{len(out)}", 33 + j % 4, 80 - j % 7, (400, 129, 801)[j % 3], j + 1),
                        f"own{len(out)}"))
        if njob >= 5 and j % 8 == 2:
            out.append((job(f"defer{len(out)}", 100 - j % 5, 100 - j % 3, (801, 65, 37)[j % 3], j),
                        f"own{len(out)}"))
    if njob >= 5:     # jobs 0 and 3: the same dW cells; jobs 1 and 5: adjacent column blocks
        c0, c1 = out[0][0], out[1][0]
        out[0] = (c0, "same")
        out[3] = (c0._replace(name="defer3", N=130), "same")
        out[1] = (c1, "adj0")
        out[5] = (c1._replace(name="defer5", N=129, G=1), "adj1")
    return out


# ------------------------------------------------------------------ reduce_batch
# out[r][c] (+)= scale * sum_b part[b * plen + r * ldp + c]
Red = collections.namedtuple("Red", "nb rows cols ldp ldo add scale")
RED_NB = (1, 15, 16, 17, 63, 64, 65, 512, 513, 600, 1031)
RED_RC = ((1, 1), (1, 15), (16, 1), (1, 17), (7, 9), (64, 1), (5, 13), (7, 13))


def red_cases():
    """{name: [Red]}: the descriptor lists of single pfsgnn_reduce_batch calls."""
    out = {}
    for n, nb in enumerate(RED_NB):
        rows, cols = RED_RC[n % len(RED_RC)]
        out[f"red-nb{nb}"] = [Red(nb, rows, cols, cols + n % 3, cols + (n + 1) % 3, n % 2, (1.0, 0.5, -2.0)[n % 3])]
    for n, (rows, cols) in enumerate(RED_RC):
        out[f"red-{rows}x{cols}"] = [Red((3, 513)[n % 2], rows, cols, cols + 2, cols + 1, (n + 1) % 2,
                                         (-2.0, 1.0, 0.5)[n % 3])]
    out["red-mixed-seg"] = [Red(513, 3, 5, 5, 6, 0, 1.0), Red(4, 7, 13, 13, 13, 1, 0.5),
                            Red(1031, 1, 65, 66, 65, 1, -2.0), Red(512, 2, 9, 9, 9, 0, 1.0)]
    out["red-97-descriptors"] = [Red(1 + n % 5, 1 + n % 3, 1 + n % 17, 17, 18, n % 2, (1.0, 0.5)[n % 2])
                                 for n in range(97)]
    out["red-200-descriptors"] = [Red(1 + n % 7, 1 + n % 4, 1 + n % 19, 19, 19, n % 2, (1.0, -2.0)[n % 2])
                                  for n in range(200)]
    return out


def red_stages(nb):
    """(segment stage taken?, partial count k_reduce_rows sees)."""
    seg = nb > 2 * RED_SEG
    return seg, (nb + RED_SEG - 1) // RED_SEG if seg else nb


def red_part(gen, d, kind):
    """A descriptor's private partial buffer [nb][rows][ldp] (the segment stage
    rewrites it in place)."""
    return draw(kind, gen, d.nb, d.rows, d.ldp)


def ref_red(d, part, out0, dtype=torch.float64, drop=None):
    """float64 (or ``dtype``) sum over the partial axis, times scale, plus the old
    value when add is set.  ``drop``: a partial left out (a mutant)."""
    p = part[:, :, :d.cols].to(dtype)
    if drop is not None:
        p = torch.cat([p[:drop], p[drop + 1:]])
    s = p.sum(0) * d.scale
    out = out0.to(dtype).clone()
    out[:, :d.cols] = out[:, :d.cols] + s if d.add else s
    return out


# overlap: reductions into one [8][12] matrix, applied in list order ->
# [(r0, c0, rows, cols, add, row step)]: row step 2 is a descriptor of pitch 24
OVERLAP_SHAPE = (8, 12)
OVERLAPS = {"same-cells": [(1, 2, 4, 5, 0, 1), (1, 2, 4, 5, 1, 1)],
            "partial": [(0, 0, 5, 6, 1, 1), (3, 4, 4, 6, 0, 1), (2, 2, 3, 3, 1, 1)],
            "disjoint-columns": [(0, 0, 8, 4, 0, 1), (0, 4, 8, 4, 0, 1), (0, 8, 8, 4, 1, 1)],
            "pitches": [(0, 0, 8, 4, 0, 1), (1, 2, 3, 5, 1, 2), (0, 3, 4, 2, 1, 2)]}


def ref_overlap(rects, parts, out0, order=None):
    out = out0.clone()
    for n in (order or range(len(rects))):
        r0, c0, rows, cols, add, step = rects[n]
        s = parts[n].sum(0)
        view = out[r0:r0 + rows * step:step, c0:c0 + cols]
        view.copy_(view + s if add else s)
    return out


# ------------------------------------------------------------------ small ops
SMALL_GN = [(G, n) for G in (1, 3) for n in (1, 255, 257)]
SMALL_RTOL = dict(graph_reduce=2e-4, graph_reduce_multi=2e-4, graph_mean2=2e-4, graph_bcast_add2=2e-4,
                  bn_eval_coef=2e-4, affine_rows=2e-4, bn_eval_bwd_coef=1e-3)


def small_inputs(G, n):
    gen = torch.Generator().manual_seed(900 + 10 * G + n)
    C = 10
    ns = (n, 3, 300, 256)
    i = dict(C=C, G=G, n=n, X=rnd(gen, C, G * n), out0=rnd(gen, C, G),
             Xs=[rnd(gen, C, G * m) for m in ns], X2=rnd(gen, C, G * 7),
             o1=rnd(gen, C, G * n), o2=rnd(gen, C, G * 7), src=rnd(gen, 2 * C, G),
             gamma=rnd(gen, C).abs() + 0.5, beta=rnd(gen, C), rm=rnd(gen, C) * 0.3,
             rv=rnd(gen, C).abs() + 0.5, Sg=rnd(gen, C), Sgx=rnd(gen, C), dg0=rnd(gen, C),
             db0=rnd(gen, C))
    return i


def run_small(be, i, conv, conv_out=None):
    """Every small op on ``be`` -> {op.output: tensor}.  ``conv_out``: the conversion
    of the tensors an op accumulates into (guarded device buffers), else ``conv``."""
    G, eps = i["G"], 1e-5
    out = {}
    conv_out = conv_out or conv
    out["graph_reduce.add"] = be.graph_reduce(conv(i["X"]), G, out=conv_out(i["out0"]))
    out["graph_reduce.mean_add"] = be.graph_reduce(conv(i["X"]), G, mean=True, out=conv_out(i["out0"]))
    for m in (1, 2, 3, 4):
        out[f"graph_reduce_multi.{m}"] = be.graph_reduce_multi([conv(x) for x in i["Xs"][:m]], G,
                                                               conv_out(i["out0"]))
    out["graph_mean2.out"] = be.graph_mean2(conv(i["X"]), conv(i["X2"]), G)
    o1, o2 = conv_out(i["o1"]), conv_out(i["o2"])
    be.graph_bcast_add2(o1, 0.5, o2, -1.25, conv(i["src"]))
    out["graph_bcast_add2.out1"], out["graph_bcast_add2.out2"] = o1, o2
    p = [conv(i[k]) for k in ("gamma", "beta", "rm", "rv")]
    for times in (1, 2):
        sc, sh = be.bn_eval_coef(*p, eps, times)
        out[f"bn_eval_coef.sc{times}"], out[f"bn_eval_coef.sh{times}"] = sc, sh
        out[f"affine_rows.Y{times}"] = be.affine_rows(conv(i["X"]), sc, sh)
        dg, db = conv_out(i["dg0"]), conv_out(i["db0"])
        inv, scale = be.bn_eval_bwd_coef(*p, eps, times, Sg=conv(i["Sg"]), Sgx=conv(i["Sgx"]),
                                         dgamma=dg, dbeta=db)
        out[f"bn_eval_bwd_coef.inv{times}"], out[f"bn_eval_bwd_coef.scale{times}"] = inv, scale
        out[f"bn_eval_bwd_coef.dgamma{times}"], out[f"bn_eval_bwd_coef.dbeta{times}"] = dg, db
    return out


def ref_small(i, dtype=torch.float64):
    return run_small(EmuBackend(dtype), i, lambda t: t.to(dtype).clone())


# ------------------------------------------------------------------ bounds
RTOL_FP32, RTOL_X3 = 1e-5, 5e-5     # test_gpu_ops.test_node_x3_policy's, at the 100-wide shape


def max_err(a, b):
    return (a.double() - b.double()).abs().max().item() if b.numel() else 0.0


def bound(r64, r32, rtol):
    """max(rtol * max|ref64|, 16 * max|ref32 - ref64|) of one block.  Nothing here
    comes from the code under test."""
    if not r64.numel():
        return 0.0
    return max(rtol * r64.abs().max().item(), 16.0 * max_err(r32, r64))


# ------------------------------------------------------------------ branches
def assert_reaches_branch(c):
    """The restated geometry gives the branch the case is named for."""
    w = c.want
    if isinstance(c, Gemm):
        Mo, Ki = gemm_dims(c)
        assert Mo <= MO_MAX and Ki <= KI_MAX
        assert gemm_mt(Mo) == w["mt"] and gemm_ksm(Ki) == w["ksm"], (c.name, gemm_mt(Mo), gemm_ksm(Ki))
        assert gemm_lds(Mo, Ki) <= 160 * 1024
        if "per_graph" in w:
            assert c.N % c.G == 0 and c.N // c.G == w["per_graph"]
        return dict(mt=gemm_mt(Mo), ksm=gemm_ksm(Ki), lds=gemm_lds(Mo, Ki))
    if isinstance(c, Batch):
        ls = batch_launches(c)
        assert len(c.jobs) == w["njob"] and (w["mt"], w["ks"]) in ls, (c.name, ls)
        assert all(Ki <= GM_KI_MAX and Mo <= GM_M_MAX for Mo, Ki in map(batch_job_dims, c.jobs))
        return ls
    if isinstance(c, Wg):
        p = wg_plan(c)
        assert isinstance(p, dict), (c.name, p)
        assert c.N <= 2100 and c.N % c.G == 0
        for k in ("tm", "per", "ntile", "nblk", "vec"):
            if k in w:
                assert p[k] == w[k], (c.name, k, p[k], w[k])
        if "per_graph" in w:
            assert c.N // c.G == w["per_graph"]
        return p
    raise TypeError(c)
