"""Budgeted rounding on the CPU: the properties of the numpy reference
(tests/budget_round_ref.py) on random and crafted inputs; ``pfsgnn.train.
hard_schedule(..., "budget")`` through the torch emulation of the op set against
that reference; and pfsgnn_schedule_budget's ABI and argument checks (host-only
calls, no GPU).
"""
import ctypes

import numpy as np
import pytest
import torch

from budget_round_ref import budget_round_ref, quotient
from test_hard_schedule_ref import _product, emu_pfsgnn  # noqa: F401  (fixture)

TOTAL = 42.0


def random_case(seed, NS=23, NT=7, E=260, tmax=9, qscale=3.0, dead_class=False):
    """A general batch with repeated pairs, an edgeless fiber and integer T."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, NS - 1, E)                       # fiber NS - 1 has no edges
    tgt = rng.integers(0, NT, E)
    ci = np.stack([rng.integers(1, tmax, NT), rng.integers(100, 2000, NT)], 1).astype(np.float32)
    if dead_class:
        ci[2, 0] = 0.0
    # quotients on a 1/8 grid: ties in frac are common
    q = (rng.integers(0, int(8 * qscale), E) / 8.0).astype(np.float32)
    q[(ci[tgt, 0] <= 0)] = 0
    return q, np.stack([src, tgt]), ci, NS


def check_properties(q, ei, ci, NS, total=TOTAL, inert=None):
    r = budget_round_ref(q, ei, ci, total, NS, inert)
    src, tgt = ei
    T_e = ci[tgt, 0].astype(np.float64)
    vis, base = r["visits"], r["base"]
    live = ~r["dead"]
    ft = np.zeros(NS)
    np.add.at(ft, src[live], vis[live] * T_e[live])
    assert np.array_equal(ft, r["ft"])                    # integer T: every sum exact
    assert (ft <= total).all()
    assert (vis[~live] == 0).all() and (vis >= 0).all()
    down = (r["phase"] & 1) != 0
    up_only = ~down[src]
    assert ((vis[up_only & live] - base[up_only & live]) >= 0).all()
    assert ((vis[up_only & live] - base[up_only & live]) <= 1).all()
    # maximality: no candidate that kept its floor fits the time left
    kept = live & ~r["reduced"] & (vis == base)
    assert (ft[src[kept]] + T_e[kept] > total).all()
    # a down phase only where the floor alone is over, and then to within the budget
    ftb = np.zeros(NS)
    np.add.at(ftb, src[live], base[live] * T_e[live])
    assert np.array_equal(down, ftb > total)
    bumped = np.zeros(NS, bool)
    bumped[src[live & ~r["reduced"] & (vis > base)]] = True
    assert np.array_equal((r["phase"] & 2) != 0, bumped)
    refused = np.zeros(NS, bool)
    refused[src[kept]] = True
    assert np.array_equal((r["phase"] & 4) != 0, refused)
    return r


@pytest.mark.parametrize("seed,qscale,tmax", [(1, 3.0, 9), (2, 12.0, 9), (3, 1.0, 4), (4, 30.0, 13)])
def test_reference_properties_random(seed, qscale, tmax):
    q, ei, ci, NS = random_case(seed, qscale=qscale, tmax=tmax)
    r = check_properties(q, ei, ci, NS)
    assert r["phase"][NS - 1] == 0 and r["ft"][NS - 1] == 0   # the fiber without edges
    if qscale >= 12:
        assert (r["phase"] & 1).any()                      # some fibers took the down phase
    if qscale <= 1:                                        # every floor is 0
        assert not (r["phase"] & 1).any() and (r["phase"] & 2).any()


@pytest.mark.parametrize("seed,qscale", [(5, 10.0), (6, 2.0)])
def test_reference_is_invariant_under_edge_permutation(seed, qscale):
    """Without repeated pairs a fiber's keys (frac, class) are distinct, so the
    result is the same edge by edge however the edge list is ordered.  (With
    repeated pairs the key's last component, the caller's position, orders two
    edges of one fiber and class with equal frac: that is the definition's
    tie-break, test_ties_resolve_by_class_then_position.)"""
    q, ei, ci, NS = random_case(seed, qscale=qscale)
    check_properties(q, ei, ci, NS)
    _, first = np.unique(ei[0] * 1000 + ei[1], return_index=True)
    q, ei = q[first], ei[:, first]
    a = check_properties(q, ei, ci, NS)
    assert (a["phase"] & 1).any() if qscale > 5 else (a["phase"] == 6).any()
    for k in range(3):
        p = np.random.default_rng(seed + k).permutation(q.size)
        b = check_properties(q[p], ei[:, p], ci, NS)
        assert np.array_equal(a["visits"][p], b["visits"])
        for name in ("phase", "ties", "ft"):
            assert np.array_equal(a[name], b[name]), name


def test_equality_fits_the_budget():
    """One fiber, T = 10, 16, 16: floors 1 + 1 + 0 -> 26; the largest frac
    (class 1, T = 16) brings it to 42 exactly and is accepted; nothing else fits."""
    ci = np.array([[10, 100], [16, 100], [16, 100]], np.float32)
    ei = np.array([[0, 0, 0], [0, 1, 2]])
    q = np.array([1.25, 1.75, 0.5], np.float32)
    r = budget_round_ref(q, ei, ci, TOTAL, 1)
    assert r["visits"].tolist() == [1, 2, 0] and r["ft"][0] == TOTAL
    assert r["ties"][0] == 1 and r["phase"][0] == 2 | 4
    # a floor that alone equals the budget: no down phase, nothing fits
    r = budget_round_ref(np.array([1.5, 2.9, 0.9], np.float32), ei, ci, TOTAL, 1)
    assert r["visits"].tolist() == [1, 2, 0] and r["phase"][0] == 4 and r["ties"][0] == 0


def test_ties_resolve_by_class_then_position():
    """All fracs equal, T = 10 everywhere, floors 0: four bumps fit (40 <= 42).
    Edges in caller order: class 2, class 0, class 1, class 0 (a repeated pair),
    class 1 -> the class 0 pair first (positions 1, 3), then class 1 by position
    (2, 4)."""
    ci = np.array([[10, 100]] * 3, np.float32)
    ei = np.array([[0] * 5, [2, 0, 1, 0, 1]])
    q = np.full(5, 0.5, np.float32)
    r = budget_round_ref(q, ei, ci, TOTAL, 1)
    assert r["visits"].tolist() == [0, 1, 1, 1, 1]
    ci[:, 0] = 14                                          # three fit: the later class 1 loses
    r = budget_round_ref(q, ei, ci, TOTAL, 1)
    assert r["visits"].tolist() == [0, 1, 1, 1, 0]
    # down phase: ascending frac, then lower class, then lower position
    ci[:, 0] = 10
    q = np.full(5, 2.5, np.float32)                        # floors 2 x 5 x 10 = 100 > 42
    r = budget_round_ref(q, ei, ci, TOTAL, 1)
    # 58 over: class 0 pos 1 loses 2 (80), class 0 pos 3 loses 2 (60), class 1 pos 2
    # loses 2 (40 <= 42); nobody left fits a bump (40 + 10 > 42)
    assert r["visits"].tolist() == [2, 0, 0, 0, 2]
    assert r["reduced"].tolist() == [False, True, True, True, False]
    assert r["phase"][0] == 1 | 4


def test_down_phase_can_strip_a_fiber_to_zero_and_then_bump():
    ci = np.array([[50, 100], [4, 100]], np.float32)      # T = 50 never fits 42
    ei = np.array([[0, 0], [0, 1]])
    r = budget_round_ref(np.array([3.25, 0.5], np.float32), ei, ci, TOTAL, 1)
    assert r["visits"].tolist() == [0, 1] and r["phase"][0] == 1 | 2
    assert r["ft"][0] == 4


def test_inert_edges():
    q, ei, ci, NS = random_case(7, qscale=10.0, dead_class=True)
    inert = np.zeros(q.size, bool)
    inert[::17] = True                                     # NaN times
    q[inert] = 0
    r = check_properties(q, ei, ci, NS, inert=inert)
    assert (r["visits"][inert] == 0).all() and (r["visits"][ei[1] == 2] == 0).all()
    tq, ti = quotient(np.array([np.nan, 3.0, -1.0, 1e30, 5.0], np.float32),
                      np.array([2.0, 0.0, 2.0, 1.0, np.inf], np.float32))
    assert tq.tolist() == [0.0, 0.0, 0.0, 2.0 ** 24, 0.0]
    assert ti.tolist() == [True, True, False, False, True]


# ---------------------------------------------------------------- the emulation
@pytest.mark.parametrize("shift,tscale", [(0.0, 1.0), (1.5, 1.0), (0.0, 0.25)])
def test_budget_through_the_emulation_equals_the_reference(emu_pfsgnn, shift, tscale):
    pfsgnn = emu_pfsgnn
    from pfsgnn.train import hard_schedule
    g, nf, nc = 2, 12, 5
    model, graph, gnn, data, ci = _product(pfsgnn, g, nf, nc, seed=5, tscale=tscale)
    with torch.no_grad():
        gnn.decoder_e[2].bias += shift
    out = gnn(data)
    hs = hard_schedule(out, ci, "budget")
    assert isinstance(hs, pfsgnn.BudgetSchedule) and hs._fields[:7] == pfsgnn.HardSchedule._fields
    assert hs.visits.dtype == hs.phase.dtype == torch.int32 and hs.quot.dtype == torch.float32
    ei = graph.edge_index.numpy()
    r = budget_round_ref(hs.quot.numpy(), ei, ci.numpy(), TOTAL, g * nf)
    assert np.array_equal(hs.visits.numpy(), r["visits"])
    assert np.array_equal(hs.phase.numpy(), r["phase"])
    assert np.array_equal(hs.fiber_time.double().numpy(), r["ft"])
    assert int(hs.over.sum()) == 0 and float(hs.worst.max()) <= TOTAL
    if shift:
        assert (r["phase"] & 1).any()
    # the quotient is the floor schedule's: floor(quot) are its visits
    fl = hard_schedule(out, ci, "floor")
    assert torch.equal(torch.floor(hs.quot).int(), fl.visits)
    assert float(hs.utility.sum()) >= float(fl.utility.sum()) or (r["phase"] & 1).any()
    # time=: the same rounding of a given time vector
    time = (hs.quot * ci[graph.edge_index[1], 0]).numpy()
    ht = hard_schedule(out, ci, "budget", time=time)
    rt = budget_round_ref(ht.quot.numpy(), ei, ci.numpy(), TOTAL, g * nf)
    assert np.array_equal(ht.visits.numpy(), rt["visits"])
    with pytest.raises(ValueError, match="budget"):
        hard_schedule(out, ci, "floor", time=time)
    with pytest.raises(ValueError, match="rounding"):
        hard_schedule(out, ci, "ceil")


def test_emulated_loop_tracks_the_budget_schedule(emu_pfsgnn):
    pfsgnn = emu_pfsgnn
    from pfsgnn.train import TrainLoop
    res = {}
    for track in (True, "budget"):
        model, graph, gnn, data, ci = _product(pfsgnn, 2, 6, 4, seed=4, tscale=0.25)
        opt = pfsgnn.FusedAdam(gnn.parameters(), lr=3e-2, capturable=True)
        loop = TrainLoop(gnn, opt, data, ci, 8, [0, 20], 5.0, 0.1, 0.1, seed=40, capture=False,
                         track_hard=track)
        res[track] = loop.run(7)
    hf, hb = res[True].history(), res["budget"].history()
    assert np.array_equal(hf["losses"], hb["losses"])      # the soft run is the same
    assert (hb["hard_overtime"] == 0).all()
    assert (hb["hard_objective"] >= hf["hard_objective"]).all()
    assert hb["hard_objective"].max() > hf["hard_objective"].max()
    assert set(res["budget"].hard_best()) == set(res[True].hard_best())
    with pytest.raises(ValueError, match="track_hard"):
        TrainLoop(gnn, opt, data, ci, 8, [0, 20], 5.0, 0.1, 0.1, track_hard="round")


# ---------------------------------------------------------------- C ABI (host-only)
@pytest.fixture(scope="module")
def lib():
    from pfsgnn import native
    return native.lib()


def test_abi_struct_size_and_limits(lib):
    from pfsgnn import native
    assert lib.pfsgnn_version().decode() == native.ABI_VERSION == "pfsgnn 0.3 gfx950"
    assert lib.pfsgnn_schedule_budget_args_bytes() == ctypes.sizeof(native.ScheduleBudgetArgs)
    assert native.ScheduleBudgetArgs.phase.offset == ctypes.sizeof(native.ScheduleBudgetArgs) - 8
    assert native.ScheduleBudgetArgs.sl.offset == 16
    assert lib.pfsgnn_schedule_budget_max_nc() >= 128
    # one word per edge slot and the class partial rows
    assert lib.pfsgnn_schedule_budget_ws_bytes(2, 70, 9, 0) >= 4 * (2 * 70 * 9) + 4 * (2 * 2 * 9)
    assert lib.pfsgnn_schedule_budget_ws_bytes(2, 70, 9, 5000) >= 4 * 5000 + 4 * (2 * 2 * 9)
    # pfsgnn_schedule and its struct are unchanged
    assert lib.pfsgnn_schedule_args_bytes() == ctypes.sizeof(native.ScheduleArgs)
    assert native.ScheduleArgs.worst.offset == ctypes.sizeof(native.ScheduleArgs) - 8


def test_schedule_budget_refuses_bad_arguments_before_any_launch(lib):
    """Fake non-null pointers are never dereferenced: every refusal comes from a
    host-side check and names pfsgnn_schedule_budget."""
    from pfsgnn import native
    FAKE = 0x1000
    OPTIONAL = ("pos_user", "perm", "time_in", "quot")

    def args(cls=native.ScheduleBudgetArgs, **over):
        a = cls(G=1, NF=16, NC=2, F=10, mode=1)
        for f, ty in a._fields_[5:]:
            if ty is ctypes.c_void_p and f not in OPTIONAL:
                setattr(a, f, FAKE)
        for f, v in over.items():
            setattr(a, f, v)
        return a

    def refused(a, *words, ws=(None, 0), fn="pfsgnn_schedule_budget"):
        rc = getattr(lib, fn)(None if a is None else ctypes.byref(a), ws[0], ws[1], None)
        err = lib.pfsgnn_last_error().decode()
        assert rc != 0, words
        assert err.startswith(fn + ":"), err
        for w in words:
            assert w in err, (err, w)

    sliced = native.Sliced(fib=FAKE, base=FAKE, len=FAKE, cls=FAKE, pco=FAKE, EP=32, E=20, maxdeg=2)
    slp = ctypes.pointer(sliced)
    max_nc = ctypes.c_int(0)
    assert lib.pfsgnn_sliced_max_nc(10, ctypes.byref(max_nc)) == 0 and max_nc.value > 0
    refused(None, "null")
    refused(args(sl=slp), "sl", "pos_user")
    refused(args(pos_user=FAKE), "sl", "pos_user")
    refused(args(sl=slp, pos_user=FAKE, perm=FAKE), "sl", "perm")
    refused(args(mode=0), "mode 0", "perm")
    refused(args(mode=3), "mode")
    for form in (dict(), dict(sl=slp, pos_user=FAKE)):
        refused(args(F=11, **form), "Fdim")
        for out in ("visits", "n_hard", "fiber_time", "completeness", "utility", "over", "worst",
                    "phase"):
            refused(args(**{out: None}, **form), "null output")
        refused(args(y=None, **form), "null input")        # y == NULL without time_in
        refused(args(ci=None, time_in=FAKE, **form), "null input")
        refused(args(**form), "workspace")
        refused(args(**form), "workspace", ws=(FAKE, 64))
        # time_in without quot, y and the decoder NULL: accepted up to the workspace check
        refused(args(time_in=FAKE, y=None, sc=None, sh=None, Wd1=None, bd1=None, Wd2=None,
                     bd2=None, **form), "workspace")
        refused(args(quot=FAKE, **form), "workspace")
    refused(args(sl=slp, pos_user=FAKE, NC=max_nc.value + 1), "pfsgnn_sliced_max_nc")
    refused(args(NC=lib.pfsgnn_schedule_budget_max_nc() + 1), "pfsgnn_schedule_budget_max_nc")
    # not a third mode of pfsgnn_schedule
    refused(args(native.ScheduleArgs, rounding=2), "rounding", fn="pfsgnn_schedule")


def test_library_without_the_symbol_says_rebuild(tmp_path):
    """A "pfsgnn 0.3" library from before this op lacks pfsgnn_schedule_budget:
    native.lib() refuses it with a rebuild message, not an AttributeError."""
    from test_abi_and_host import _stand_in_library_is_refused
    from pfsgnn import native
    special = {"pfsgnn_version":
               'const char* pfsgnn_version(void) { return "%s"; }' % native.ABI_VERSION}
    source = "\n".join(special.get(n, "int %s(void) { return 0; }" % n) for n in native._SIGS
                       if not n.startswith("pfsgnn_schedule_budget"))
    out = _stand_in_library_is_refused(tmp_path, source + "\n")
    assert "pfsgnn_schedule_budget" in out and "rebuild" in out and "AttributeError" not in out
