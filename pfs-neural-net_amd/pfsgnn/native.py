"""ctypes binding of libpfsgnn.so (the C ABI in include/pfsgnn.h) as an op backend.

This is the only compute backend of the product.  There is no fallback: if
the shared library is missing, or the process has no MI355X visible, every
entry point raises ``NativeUnavailable`` -- the hot path never silently runs
in PyTorch or on the CPU.

Tensors are passed as raw device pointers on torch's current HIP stream, so
PyTorch is only the allocator / stream / collective plumbing here.
"""
import ctypes
import os

import torch

from .sparse import SparseEdgeOps, SparseGeo

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libpfsgnn.so")
# tuning builds (tools/variants.sh): PFSGNN_LIB_VARIANT=<name> loads
# pfsgnn/libpfsgnn_<name>.so, an in-tree build of the same sources with other
# compile-time knobs
if os.environ.get("PFSGNN_LIB_VARIANT"):
    _LIB_PATH = os.path.join(os.path.dirname(_LIB_PATH),
                             "libpfsgnn_" + os.environ["PFSGNN_LIB_VARIANT"] + ".so")
# (a test-only build elsewhere in the tree, by path: tests/native/libpfsgnn_lossexact.so)
if os.environ.get("PFSGNN_LIB_PATH"):
    _LIB_PATH = os.environ["PFSGNN_LIB_PATH"]


class NativeUnavailable(RuntimeError):
    pass


_lib = None

P = ctypes.c_void_p
I = ctypes.c_int
LL = ctypes.c_longlong
FL = ctypes.c_float
SZ = ctypes.c_size_t
ULL = ctypes.c_ulonglong


class Seg(ctypes.Structure):
    """pfsgnn_seg (include/pfsgnn.h): one row block of a concatenated node input."""
    _fields_ = [("x", ctypes.c_void_p), ("rows", ctypes.c_int), ("col", ctypes.c_int),
                ("per_graph", ctypes.c_int)]


SEGP = ctypes.POINTER(Seg)


class Red(ctypes.Structure):
    """pfsgnn_red (include/pfsgnn.h): one pending cross-block reduction."""
    _fields_ = [("part", ctypes.c_void_p), ("nb", ctypes.c_int), ("plen", ctypes.c_size_t),
                ("ldp", ctypes.c_int), ("rows", ctypes.c_int), ("cols", ctypes.c_int),
                ("out", ctypes.c_void_p), ("ldo", ctypes.c_int), ("add", ctypes.c_int),
                ("scale", ctypes.c_float)]


REDP = ctypes.POINTER(Red)


class Sliced(ctypes.Structure):
    """pfsgnn_sliced_t (include/pfsgnn.h): a general batch cut into slices of 16
    fibers for the fused edge kernels (pfsgnn_sliced.hip)."""
    _fields_ = [("fib", ctypes.c_void_p), ("base", ctypes.c_void_p), ("len", ctypes.c_void_p),
                ("cls", ctypes.c_void_p), ("pco", ctypes.c_void_p), ("EP", ctypes.c_longlong),
                ("E", ctypes.c_longlong), ("maxdeg", ctypes.c_int)]


SLP = ctypes.POINTER(Sliced)


class OSeg(ctypes.Structure):
    """pfsgnn_oseg (include/pfsgnn.h): one row block of an input-gradient output."""
    _fields_ = [("x", ctypes.c_void_p), ("rows", ctypes.c_int), ("add", ctypes.c_int)]


OSEGP = ctypes.POINTER(OSeg)


class WgJob(ctypes.Structure):
    """pfsgnn_wgrad_job (include/pfsgnn.h): one deferred weight gradient."""
    _fields_ = [("dY", ctypes.c_void_p), ("M", ctypes.c_int), ("segs", SEGP), ("nseg", ctypes.c_int),
                ("N", ctypes.c_int), ("act_in", ctypes.c_int), ("dW", ctypes.c_void_p),
                ("lddw", ctypes.c_int), ("db", ctypes.c_void_p), ("dbscale", ctypes.c_float)]


WGJP = ctypes.POINTER(WgJob)


class GemmJob(ctypes.Structure):
    """pfsgnn_gemm_job (include/pfsgnn.h): one product of a batched launch."""
    _fields_ = [("W", ctypes.c_void_p), ("ldw", ctypes.c_int), ("trans", ctypes.c_int),
                ("M", ctypes.c_int), ("K", ctypes.c_int), ("segs", SEGP), ("nseg", ctypes.c_int),
                ("N", ctypes.c_int), ("b", ctypes.c_void_p), ("bscale", ctypes.c_float),
                ("act_in", ctypes.c_int), ("Z", ctypes.c_void_p), ("Y", ctypes.c_void_p),
                ("add", ctypes.c_int)]


GMJP = ctypes.POINTER(GemmJob)


class LinMap(ctypes.Structure):
    """pfsgnn_linmap (include/pfsgnn.h): out = W[:, col0:col0+O] . Y + b."""
    _fields_ = [("W", ctypes.c_void_p), ("ldw", ctypes.c_int), ("col0", ctypes.c_int),
                ("nk", ctypes.c_int), ("b", ctypes.c_void_p), ("out", ctypes.c_void_p)]


LINMP = ctypes.POINTER(LinMap)


def _ptrs(*names):
    return [(n, ctypes.c_void_p) for n in names]


class ClassBwd(ctypes.Structure):
    """pfsgnn_class_bwd (include/pfsgnn.h): a block's class-side backward."""
    _fields_ = ([("G", I), ("NF", I), ("NC", I), ("F", I), ("pend", ctypes.c_void_p * 4),
                 ("pend_n", I * 4), ("npend", I)]
                + _ptrs("V", "w", "y1", "r1", "r2", "gZ", "gW1", "gW2") + [("gH", I)]
                + _ptrs("gu_up", "gV", "gdZ", "dwp", "gu", "g_xs", "g_xt",
                        "Yp", "mu", "var", "gamma", "Z", "W1", "W2", "Wt2")
                + [("eps", FL)]
                + _ptrs("dgamma", "dbeta", "dYp", "dZ", "gxt_in", "g_agg", "gu_t", "g_hsum"))


class BlockTail(ctypes.Structure):
    """pfsgnn_block_tail (include/pfsgnn.h): a block tail on a complete batch."""
    _fields_ = ([("G", I), ("NF", I), ("NC", I), ("F", I)]
                + _ptrs("y", "sc", "sh", "Rs", "Wt1", "Wt2", "bt2", "tmask", "hsum", "agg",
                        "xt", "u", "W1", "b1", "W2", "b2", "gamma", "beta",
                        "Z", "Yp", "rm", "rv", "xt_new", "mu", "var")
                + [("momentum", FL), ("eps", FL)]
                + _ptrs("xs", "gW1", "gb1", "gW2", "gb2", "gw")
                + [("gH", I), ("reps", FL)]
                + _ptrs("means", "gZ", "gV", "unew", "y1", "r1", "r2",
                        "We", "be", "Ws", "bs", "Pt", "Qt"))


# The edge ops' argument structs (include/pfsgnn.h): each begins with the batch
# and its sliced layout (NULL: complete graphs); an optional part left out is
# NULL / 0, which is what ctypes gives a field that is not set.
_EDGE_HEAD = [("G", I), ("NF", I), ("NC", I), ("F", I), ("sl", SLP)]


class EdgeMlpFwdArgs(ctypes.Structure):
    """pfsgnn_edge_mlp_fwd_args"""
    _fields_ = (_EDGE_HEAD
                + _ptrs("xe", "xsc", "xsh", "Ps", "Pt", "W1", "W2", "b2", "y", "mu", "var",
                        "gamma", "beta", "rm", "rv")
                + [("momentum", FL), ("eps", FL)] + _ptrs("sc", "sh", "inv1", "inv2"))


class SourceFwdArgs(ctypes.Structure):
    """pfsgnn_source_fwd_args"""
    _fields_ = _EDGE_HEAD + _ptrs("y", "sc", "sh", "Qt", "Ws1", "Ws2", "bs2", "mom", "hs", "msg")


class TargetFwdArgs(ctypes.Structure):
    """pfsgnn_target_fwd_args"""
    _fields_ = (_EDGE_HEAD + _ptrs("y", "sc", "sh", "Rs", "Wt1", "hsum", "Wt2", "bt2")
                + [("bscale", FL)] + _ptrs("agg", "tmask"))


class TargetBwdArgs(ctypes.Structure):
    """pfsgnn_target_bwd_args"""
    _fields_ = (_EDGE_HEAD
                + _ptrs("y", "sc", "sh", "Rs", "Wt1", "g_hsum", "GzT", "dWt1", "gxe", "g_xs",
                        "tmask", "bn_Yp", "bn_mu", "bn_var")
                + [("bn_eps", FL)] + _ptrs("bn_part") + [("fold", I)])


class SourceBwdArgs(ctypes.Structure):
    """pfsgnn_source_bwd_args"""
    _fields_ = (_EDGE_HEAD
                + _ptrs("y", "sc", "sh", "Qt", "Ws1", "Ws2", "bs2", "mean", "coef", "Rs", "Wt1",
                        "g_hsum", "g_next", "mu1", "inv1", "var1", "gamma")
                + [("n", LL), ("eps", FL)]
                + _ptrs("g_tot", "GzS", "dWs1", "dWs2", "dbs2", "Sg", "Sgx", "alpha", "gam0",
                        "gam1", "dgamma", "dbeta", "g_xt", "tmask", "msg", "dWt1"))


class EdgeMlpBwdArgs(ctypes.Structure):
    """pfsgnn_edge_mlp_bwd_args"""
    _fields_ = (_EDGE_HEAD
                + _ptrs("g_tot", "alpha", "gam0", "gam1", "y", "xe", "xsc", "xsh", "Ps", "Pt",
                        "W1", "W2", "dW1", "dW2", "db2", "gxe", "GzEs", "GzEt", "g_xs", "g_xt",
                        "Vu"))


class LossArgs(ctypes.Structure):
    """pfsgnn_loss_args: the loss forward / backward on a complete or sliced
    batch; optional groups (sl + pos_user, seed_dev, sf_dev, tt, the bn_* group)
    stay NULL."""
    _fields_ = ([("G", I), ("NF", I), ("NC", I), ("F", I), ("sl", SLP)]
                + _ptrs("pos_user", "y", "sc", "sh", "Wd1", "bd1", "Wd2", "bd2", "ci")
                + [("scale", FL), ("sharpness", FL), ("noiselevel", FL), ("seed", ULL)]
                + _ptrs("seed_dev", "sf_dev", "n_prime", "fiber_time", "tmean", "tvar", "tt",
                        "Gn", "Gf", "Gv", "gscale", "dWd1", "dbd1", "dWd2", "dbd2", "gxe",
                        "bn_mu1", "bn_inv1", "bn_part"))


class TrainRecordArgs(ctypes.Structure):
    """pfsgnn_train_record_args: an epoch's history rows and best-tracking."""
    _fields_ = ([("G", I), ("NC", I), ("nepochs", LL)]
                + _ptrs("epoch", "sharpness", "loss", "utils", "variance", "n_prime", "ci")
                + [("nfields", FL), ("min_sharp", FL)]
                + _ptrs("losses", "objective", "variances", "completions", "comp", "improved",
                        "best_utility", "best_loss", "best_epoch"))


class TrainRecordHardArgs(ctypes.Structure):
    """pfsgnn_train_record_hard_args: an epoch's integer-objective rows and
    best-tracking."""
    _fields_ = ([("G", I), ("nepochs", LL)]
                + _ptrs("epoch", "utility", "over", "hard_objective", "hard_overtime",
                        "improved_hard", "best_hard_utility", "best_hard_epoch"))


class ScheduleArgs(ctypes.Structure):
    """pfsgnn_schedule_args: the hard visit counts of a complete (mode, perm) or
    sliced (sl + pos_user) batch."""
    _fields_ = ([("G", I), ("NF", I), ("NC", I), ("F", I), ("sl", SLP)]
                + _ptrs("pos_user") + [("mode", I)]
                + _ptrs("perm", "y", "sc", "sh", "Wd1", "bd1", "Wd2", "bd2", "ci")
                + [("scale", FL), ("total_time", FL), ("nfields", FL), ("rounding", I)]
                + _ptrs("visits", "n_hard", "fiber_time", "completeness", "utility", "over",
                        "worst"))


class ScheduleBudgetArgs(ctypes.Structure):
    """pfsgnn_schedule_budget_args: budgeted rounding (largest remainder per
    fiber) of a complete (mode, perm) or sliced (sl + pos_user) batch."""
    _fields_ = ([("G", I), ("NF", I), ("NC", I), ("F", I), ("sl", SLP)]
                + _ptrs("pos_user") + [("mode", I)]
                + _ptrs("perm", "y", "sc", "sh", "Wd1", "bd1", "Wd2", "bd2", "ci", "time_in")
                + [("scale", FL), ("total_time", FL), ("nfields", FL)]
                + _ptrs("visits", "n_hard", "fiber_time", "completeness", "utility", "over",
                        "worst", "quot", "phase"))


class PlanArgs(ctypes.Structure):
    """pfsgnn_schedule_plan_args: the observing plan of an integer schedule --
    class caps, fiber timelines, the target list -- of a complete batch (mode,
    perm) or a general one (mode -1 and pfsgnn_sparse_layout's CSR arrays)."""
    _fields_ = ([("G", I), ("NF", I), ("NC", I), ("mode", I)] + _ptrs("perm") + [("E", LL)]
                + _ptrs("src_p", "tgt_p", "user_of", "fib_ptr", "cls_ord", "cls_ptr", "ci")
                + [("total_time", FL), ("nfields", FL)] + _ptrs("visits_in")
                + [("cap", I), ("seg_cap", LL)]
                + _ptrs("visits", "start", "used", "idle", "n_hard", "completeness", "utility",
                        "over", "worst", "cut", "seg_ptr", "seg_edge", "seg_start"))


class CopyJob(ctypes.Structure):
    """pfsgnn_copy_job: n 4-byte words from src to dst."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("n", LL)]


# op name -> argument struct, in the order of the PFSGNN_OP_* codes
EDGE_ARGS = {"edge_mlp_fwd": EdgeMlpFwdArgs, "source_fwd": SourceFwdArgs,
             "target_fwd": TargetFwdArgs, "target_bwd": TargetBwdArgs,
             "source_bwd": SourceBwdArgs, "edge_mlp_bwd": EdgeMlpBwdArgs}

_SIGS = {
    "pfsgnn_version": ([], ctypes.c_char_p),
    "pfsgnn_last_error": ([], ctypes.c_char_p),
    "pfsgnn_workspace_bytes": ([I, I, I, I], SZ),
    "pfsgnn_set_edge_path": ([I], I),
    "pfsgnn_sync_bytes": ([], SZ),
    "pfsgnn_set_sync_buffer": ([P, SZ], I),
    "pfsgnn_get_edge_path": ([], I),
    "pfsgnn_edge_grid": ([I, I, I, ctypes.POINTER(ctypes.c_int)], I),
    "pfsgnn_timing_enable": ([I], I),
    "pfsgnn_timing_reset": ([], I),
    "pfsgnn_timing_repeat": ([ctypes.c_char_p, I], I),
    "pfsgnn_timing_query": ([ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                             ctypes.POINTER(ctypes.c_longlong)], I),
    "pfsgnn_lin": ([P, I, I, I, P, I, P, FL, I, P, I, P], I),
    "pfsgnn_lin_t": ([P, I, I, I, P, I, P, P, I, P], I),
    "pfsgnn_lin_gather": ([P, I, I, I, P, I, P, FL, I, P, I, P, P, I, P, P, I, P], I),
    "pfsgnn_wgrad": ([P, I, P, I, I, I, P, I, P, FL, P, SZ, P], I),
    "pfsgnn_lin_cat": ([P, I, I, SEGP, I, I, P, FL, I, P, I, P], I),
    "pfsgnn_wgrad_cat": ([P, I, SEGP, I, I, I, P, I, P, FL, P, SZ, P], I),
    "pfsgnn_wgrad_part_bytes": ([I, I, I, I], SZ),
    "pfsgnn_wgrad_cat_part": ([P, I, SEGP, I, I, I, P, I, P, FL, P, SZ, REDP,
                               ctypes.POINTER(ctypes.c_int), P], I),
    "pfsgnn_reduce_batch": ([REDP, I, P], I),
    "pfsgnn_wgrad_multi_bytes": ([WGJP, I], SZ),
    "pfsgnn_gemm_multi": ([GMJP, I, P], I),
    "pfsgnn_wgrad_multi": ([WGJP, I, P, SZ, P], I),
    "pfsgnn_defer_begin": ([P, SZ], I),
    "pfsgnn_defer_end": ([P], I),
    "pfsgnn_defer_end_multi": ([WGJP, I, P, SZ, P], I),
    "pfsgnn_defer_need": ([], SZ),
    "pfsgnn_bn_fwd": ([P, I, I, P, P, P, P, FL, FL, P, P, P, P, SZ, P], I),
    "pfsgnn_bn_bwd": ([P, P, P, P, P, FL, I, I, P, P, P, P, SZ, P], I),
    "pfsgnn_mlp_ws_bytes": ([I], SZ),
    "pfsgnn_mlp_fwd": ([SEGP, I, I, P, I, I, P, P, I, P, P, P, P, P, P, P, FL, FL, P, P, P, P,
                        SZ, P], I),
    "pfsgnn_mlp_fwd_epi": ([SEGP, I, I, P, I, I, P, P, I, P, P, P, P, P, P, P, FL, FL, P, P, P,
                            LINMP, I, P, SZ, P], I),
    "pfsgnn_target_global_fwd": ([SEGP, I, I, I, P, I, I, P, P, I, P, P, P, P, P, P, P, FL, FL,
                                  P, P, P, P, I, P, P, I, P, P, P, P, FL] + [P] * 7
                                 + [P] * 6 + [P, SZ, P], I),
    "pfsgnn_mlp_bwd": ([P, I, P, P, P, P, FL, P, P, P, P, I, I, I, P, I, P, P, OSEGP, I, P, SZ,
                        P], I),
    "pfsgnn_mlp_bwd_pre": ([P, I, P, P, P, P, FL, P, P, P, P, I, I, I, P, I, P, P, OSEGP, I, P, I,
                            P, P, I, I, I, P, SZ, P], I),
    "pfsgnn_build_complete": ([I, I, I, I, P, P], I),
    "pfsgnn_graph_reduce": ([P, I, I, I, I, P, P], I),
    "pfsgnn_graph_reduce_add": ([P, I, I, I, I, P, P], I),
    "pfsgnn_graph_bcast_add": ([P, I, I, I, P, FL, P], I),
    "pfsgnn_graph_reduce_multi": ([P, P, I, I, I, P, P], I),
    "pfsgnn_graph_mean2": ([P, I, P, I, I, I, P, P], I),
    "pfsgnn_graph_bcast_add2": ([P, I, FL, P, I, FL, I, I, P, P], I),
    "pfsgnn_rms2_fwd": ([P, I, I, P, FL, P, P, P, P, P], I),
    "pfsgnn_rms2_bwd": ([P, P, P, P, P, P, I, I, FL, P, P, P, SZ, P], I),
    "pfsgnn_global_fwd": ([P, I, P, I, P, I, I, P, I, P, P, P, P, FL] + [P] * 7 + [P], I),
    "pfsgnn_global_bwd": ([P, P, P, P, P, P, I, I, P, I, P, P, P, P, P, P, P, P, I, FL, P, I,
                           FL, P], I),
    "pfsgnn_bn2_finalize": ([P, P, P, P, P, P, I, LL, FL, FL, P, P, P, P, P], I),
    "pfsgnn_bn_eval_coef": ([P, P, P, P, I, FL, I, P, P, P], I),
    "pfsgnn_affine_rows": ([P, I, I, P, P, P, P], I),
    "pfsgnn_bn2_bwd_coef": ([P, P, P, P, P, I, LL, FL, P, P, P, P, P, P], I),
    "pfsgnn_bn2_bwd_coef_part": ([P, I, I, P, P, P, LL, FL, P, P, P, P, P, P], I),
    "pfsgnn_moment_coef": ([P, P, I, I, I, P, P], I),
    "pfsgnn_moment_coef_seg": ([P, P, I, I, P, P, P], I),
    "pfsgnn_sparse_layout_ws_bytes": ([LL], SZ),
    "pfsgnn_sparse_layout": ([P, LL, I, I, I, P, P, P, P, P, P, P, P, SZ, P], I),
    "pfsgnn_gather_cols": ([P, I, I, P, LL, P, I, P, P], I),
    "pfsgnn_segment_sum": ([P, I, LL, P, P, I, I, P, I, P], I),
    "pfsgnn_segment_moments": ([P, I, LL, P, I, P, P, P], I),
    "pfsgnn_segment_moment_grad": ([P, I, LL, P, P, P, I, P, P], I),
    "pfsgnn_rows_ws_bytes": ([I, LL], SZ),
    "pfsgnn_rows_stats": ([P, I, LL, P, P, P, SZ, P], I),
    "pfsgnn_rows_bn_sums": ([P, P, I, LL, P, P, P, P, P, SZ, P], I),
    "pfsgnn_rows_axpby": ([P, P, I, LL, P, P, P, P, P], I),
    "pfsgnn_tmask_bytes": ([I, I, I, I], SZ),
    "pfsgnn_tbwd_fold": ([I], I),
    "pfsgnn_msg_bytes": ([I, I, I, I], SZ),
    "pfsgnn_edge_bn_grad_sums": ([I, I, I, I, P, P, P, P, P, P, P, SZ, P], I),
    "pfsgnn_loss_args_bytes": ([], SZ),
    "pfsgnn_loss_fwd": ([ctypes.POINTER(LossArgs), P, SZ, P], I),
    "pfsgnn_loss_finalize": ([SLP, I, I, I, P, P, P, P, FL, FL, FL, FL, FL, FL, P, P, P, P, P, P,
                              P], I),
    "pfsgnn_loss_bwd": ([ctypes.POINTER(LossArgs), P, SZ, P], I),
    "pfsgnn_loss_bn_parts": ([I, I, I], I),
    "pfsgnn_layout_analyze": ([P, LL, I, I, I, P, P, P, SZ, P], I),
    "pfsgnn_edges_to_canonical": ([P, I, I, I, I, I, P, P, P], I),
    "pfsgnn_edges_from_canonical": ([P, P, P, I, I, I, I, I, P, I, P, P], I),
    "pfsgnn_adam": ([P, P, P, P, LL, I, P, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                     ctypes.c_double, ctypes.c_double, P, P], I),
    "pfsgnn_sliced_max_nc": ([I, ctypes.POINTER(ctypes.c_int)], I),
    "pfsgnn_target_block_fwd": ([ctypes.POINTER(BlockTail), P, SZ, P], I),
    "pfsgnn_sync_faults": ([ctypes.POINTER(ctypes.c_uint)], I),
    "pfsgnn_set_grid_sync_fenced": ([I], I),
    "pfsgnn_block_tail_bytes": ([], SZ),
    "pfsgnn_target_class_bwd": ([ctypes.POINTER(ClassBwd), P, SZ, P], I),
    "pfsgnn_class_bwd_bytes": ([], SZ),
    "pfsgnn_bn_eval_bwd_coef": ([P, P, P, P, I, FL, I, P, P, P, P, P, P, P], I),
    "pfsgnn_sliced_plan_ws_bytes": ([I, I], SZ),
    "pfsgnn_sliced_plan": ([P, I, I, P, P, P, P, P, P, SZ, P], I),
    "pfsgnn_sliced_fill": ([P, P, P, P, LL, I, I, P, P, LL, I, P, P, P, P], I),
    "pfsgnn_edges_to_slots": ([P, LL, LL, I, P, P, P], I),
    "pfsgnn_edges_from_slots": ([P, P, P, LL, LL, I, P, I, P, P], I),
    "pfsgnn_sl_tmask_bytes": ([SLP, I], SZ),
    "pfsgnn_edge_args_bytes": ([I], SZ),
    "pfsgnn_softfloor_record": ([P, P, P], I),
    "pfsgnn_train_advance": ([P, P, ctypes.c_double, ctypes.c_double, LL, P, P, P], I),
    "pfsgnn_train_record_args_bytes": ([], SZ),
    "pfsgnn_train_record": ([ctypes.POINTER(TrainRecordArgs), P], I),
    "pfsgnn_copy_if": ([P, P, I, ctypes.POINTER(CopyJob), I, LL, P], I),
    "pfsgnn_schedule_args_bytes": ([], SZ),
    "pfsgnn_schedule": ([ctypes.POINTER(ScheduleArgs), P, SZ, P], I),
    "pfsgnn_train_record_hard_args_bytes": ([], SZ),
    "pfsgnn_train_record_hard": ([ctypes.POINTER(TrainRecordHardArgs), P], I),
    "pfsgnn_schedule_budget_args_bytes": ([], SZ),
    "pfsgnn_schedule_budget_max_nc": ([], I),
    "pfsgnn_schedule_budget_ws_bytes": ([I, I, I, LL], SZ),
    "pfsgnn_schedule_budget": ([ctypes.POINTER(ScheduleBudgetArgs), P, SZ, P], I),
    "pfsgnn_schedule_plan_args_bytes": ([], SZ),
    "pfsgnn_schedule_plan_ws_bytes": ([I, I, I, LL], SZ),
    "pfsgnn_schedule_plan": ([ctypes.POINTER(PlanArgs), P, SZ, P], I),
}
for _op, _cls in EDGE_ARGS.items():
    _SIGS["pfsgnn_" + _op] = ([ctypes.POINTER(_cls), P, SZ, P], I)


ABI_VERSION = "pfsgnn 0.3 gfx950"  # pfsgnn_version() of the library these signatures describe


def lib():
    """Load libpfsgnn.so (once).  Raises NativeUnavailable if it is missing or
    was built from sources with another C ABI."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise NativeUnavailable(
                f"{_LIB_PATH} not found: build it with `make -C pfs-neural-net_amd` "
                "(or __graft_entry__.build()); there is no non-HIP fallback")
        L = ctypes.CDLL(_LIB_PATH)
        # a library built from other sources (a test-side or variant build left
        # over from an earlier tree) may export the same names with other
        # signatures: refuse it by its version rather than call into it
        L.pfsgnn_version.restype = ctypes.c_char_p
        if L.pfsgnn_version().decode() != ABI_VERSION:
            raise NativeUnavailable(
                f"{_LIB_PATH} is {L.pfsgnn_version().decode()!r}, this binding is for "
                f"{ABI_VERSION!r}: rebuild it with `make -C pfs-neural-net_amd`")
        for name, (args, ret) in _SIGS.items():
            # (a library of this version built before an entry point was added)
            fn = getattr(L, name, None)
            if fn is None:
                raise NativeUnavailable(
                    f"{_LIB_PATH} does not export {name}: it was built from older sources; "
                    "rebuild it with `make -C pfs-neural-net_amd`")
            fn.argtypes = args
            fn.restype = ret
        sizes = [("pfsgnn_loss_args_bytes", (), LossArgs),
                 ("pfsgnn_train_record_args_bytes", (), TrainRecordArgs)]
        sizes += [("pfsgnn_edge_args_bytes", (op,), cls) for op, cls in enumerate(EDGE_ARGS.values())]
        sizes += [("pfsgnn_train_record_hard_args_bytes", (), TrainRecordHardArgs),
                  ("pfsgnn_schedule_args_bytes", (), ScheduleArgs),
                  ("pfsgnn_schedule_budget_args_bytes", (), ScheduleBudgetArgs),
                  ("pfsgnn_schedule_plan_args_bytes", (), PlanArgs)]
        for query, qargs, cls in sizes:
            got, call = getattr(L, query)(*qargs), f"{query}({', '.join(map(str, qargs))})"
            if got != ctypes.sizeof(cls):
                raise NativeUnavailable(
                    f"{_LIB_PATH}: {call} = {got} but this binding's "
                    f"{cls.__name__} has {ctypes.sizeof(cls)} bytes: rebuild the library")
        _lib = L
        path = os.environ.get("PFSGNN_EDGE_PATH")
        if path:
            set_edge_path(path)
    return _lib


EDGE_PATHS = {"valu": 0, "mfma": 1, "mfma32": 2, "bf16y": 3, "bf16": 4, "bf16m": 5, "bf16x3": 6,
              "bf16x6": 7}


def set_edge_path(path):
    """Implementation of the per-edge kernels: "mfma" (default; matrix cores,
    exact fp32 forward products, bf16x3 gradient chains), "mfma32" (matrix
    cores, every layer product exact fp32), "valu" (fp32 fmaf chains), "bf16y"
    (mfma32 with the edge state rounded to bf16), "bf16m" (single-bf16 MFMA
    contractions), "bf16" (bf16m + bf16 edge state) or "bf16x3" (every
    per-edge contraction on bf16 MFMAs with split hi + lo operands, forward and
    recompute included; inside the fp32 bar at the bench geometry only) or "bf16x6"
    (the forward contractions and recompute on bf16 MFMAs with three-way split
    operands, fp32-class products; gradient chains as "mfma").  The bf16
    paths are built for Fdim 10; at other Fdims "bf16x6" runs the "mfma"
    arithmetic.
    Read at launch time; env PFSGNN_EDGE_PATH sets it when the library loads."""
    if path not in EDGE_PATHS:
        raise ValueError(f"edge path must be one of {sorted(EDGE_PATHS)}, got {path!r}")
    _check(lib().pfsgnn_set_edge_path(EDGE_PATHS[path]), "pfsgnn_set_edge_path")


def get_edge_path():
    code = lib().pfsgnn_get_edge_path()
    return {v: k for k, v in EDGE_PATHS.items()}[code]


def edge_grid(G, NF, NC):
    """Grid of the current edge path for a batch: dict(KS, CPS, nblocks, NFG)."""
    info = (ctypes.c_int * 4)()
    _check(lib().pfsgnn_edge_grid(int(G), int(NF), int(NC), info), "pfsgnn_edge_grid")
    return dict(KS=info[0], CPS=info[1], nblocks=info[2], NFG=info[3])


def exported_symbols():
    return list(_SIGS.keys())


KERNELS = ["edge_mlp_fwd", "source_fwd", "target_fwd", "target_bwd", "source_bwd",
           "edge_bn_sums", "edge_mlp_bwd", "loss_fwd", "loss_bwd"]


def timing_enable(on=True):
    """on: False / True (events around each launch) / "spin" (the same behind
    a lead-in spin kernel: the kernel's own time in an eager step)."""
    lib().pfsgnn_timing_enable(2 if on == "spin" else (1 if on else 0))


def sync_faults():
    """Device-wide barrier time-outs since the library was loaded (0 when healthy;
    a time-out also traps its launch)."""
    n = ctypes.c_uint(0)
    _check(lib().pfsgnn_sync_faults(ctypes.byref(n)), "pfsgnn_sync_faults")
    return n.value


def set_grid_sync_fenced(fenced):
    """The device-wide barrier's form for later launches: False the sc1 hand-off
    (default), True acq_rel arrival / acquire poll (pfsgnn_set_grid_sync_fenced)."""
    _check(lib().pfsgnn_set_grid_sync_fenced(1 if fenced else 0), "pfsgnn_set_grid_sync_fenced")


def timing_repeat(name, extra):
    """Launch kernel `name` 1 + extra times back to back (pfsgnn_timing_repeat)."""
    _check(lib().pfsgnn_timing_repeat(name.encode(), int(extra)), "pfsgnn_timing_repeat")


def timing_reset():
    lib().pfsgnn_timing_reset()


def timing_query(name):
    """(total milliseconds, launches) of a main kernel since the last reset."""
    ms = ctypes.c_double(0.0)
    n = ctypes.c_longlong(0)
    lib().pfsgnn_timing_query(name.encode(), ctypes.byref(ms), ctypes.byref(n))
    return ms.value, n.value


def _ptr(t):
    if t is None:
        return None
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(rc, name):
    if rc != 0:
        msg = lib().pfsgnn_last_error().decode()
        raise RuntimeError(f"{name} failed ({rc}): {msg}")


def _call(name, *args):
    _check(getattr(lib(), name)(*args), name)


_SYNC = None


def _ensure_sync(device):
    """The library's in-launch reduction counters (pfsgnn_set_sync_buffer): one
    zeroed device buffer per process, set once.  PFSGNN_NO_HANDOFF=1 leaves it
    unset (the kernels then keep their separate reduce launches: an A/B knob).

    The counters are process-wide, so pfsgnn ops run on ONE device per process
    (the one-process-per-GPU model of torch.distributed) and on one stream at a
    time; a backend on a second device is refused rather than pointed at
    another device's counters."""
    global _SYNC
    if os.environ.get("PFSGNN_NO_HANDOFF", "0") == "1":
        return
    if _SYNC is not None:
        dev = torch.device(device)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        if _SYNC.device.index != idx:
            raise RuntimeError(
                f"pfsgnn runs on one device per process: its sync buffer lives on "
                f"{_SYNC.device}, a backend on {dev} was requested (one process per GPU)")
        return
    n = lib().pfsgnn_sync_bytes()
    _SYNC = torch.zeros(n, dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)
    _call("pfsgnn_set_sync_buffer", _SYNC.data_ptr(), n)


SLOTS = 3   # pfsgnn.gnn.Layout.SLOTS: the positions of a sliced general batch


class SlicedLayout:
    """A sliced general batch's device tensors (pfsgnn_sliced_plan / _fill) and
    the pfsgnn_sliced_t pointing at them, kept alive together.  pos_user [EP]:
    the caller's edge at each position (-1: padding)."""

    def __init__(self, fib, base, ln, slot_of, cls, pos_user, pco, EP, E, maxdeg):
        self.fib, self.base, self.len, self.slot_of = fib, base, ln, slot_of
        self.cls, self.pos_user, self.pco = cls, pos_user, pco
        self.EP, self.E, self.maxdeg = int(EP), int(E), int(maxdeg)
        self.c = Sliced(fib.data_ptr(), base.data_ptr(), ln.data_ptr(), cls.data_ptr(),
                        pco.data_ptr(), self.EP, self.E, self.maxdeg)
        self.ref = ctypes.pointer(self.c)


class HipBackend:
    """The op set of pfsgnn.engine on libpfsgnn.so (fp32, channel-major)."""

    name = "hip"
    fiber_bn_sums = True     # target_bwd(bn_sums=...) / mlp_bwd(bn_part=...)
    loss_bn_part = True      # loss_bwd(bn=...) / bn2_bwd_coef_part

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise NativeUnavailable("no HIP device visible: the pfsgnn hot path runs only on "
                                    "an MI355X (gfx950); there is no CPU fallback")
        lib()
        self.device = torch.device(device or "cuda")
        self.dtype = torch.float32
        self._ws = None
        self._ws_key = None
        # buffers replaced by a larger one stay alive: a HIP graph captured
        # while they were current keeps their addresses baked in, and a replay
        # must never write into memory the allocator has handed out again
        self._retired = []
        self._sp = SparseEdgeOps(self)
        _ensure_sync(self.device)

    def edge_path(self):
        """The current edge path's code (pfsgnn_get_edge_path)."""
        return lib().pfsgnn_get_edge_path()

    # ------------------------------------------------------------ memory
    def empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def zeros(self, *shape):
        return torch.zeros(*shape, dtype=torch.float32, device=self.device)

    def ones(self, *shape):
        return torch.ones(*shape, dtype=torch.float32, device=self.device)

    def workspace(self, d=None, extra=0):
        """``extra``: bytes an op needs beyond pfsgnn_workspace_bytes' promise
        (pfsgnn_schedule_budget_ws_bytes)."""
        need = lib().pfsgnn_workspace_bytes(d.G, d.NF, d.NC, d.F) if d is not None else 0
        need = max(need, 16 << 20, int(extra))
        if self._ws is None or self._ws.numel() < need:
            if self._ws is not None:
                self._retired.append(self._ws)
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _wsargs(self, d=None, extra=0):
        ws = self.workspace(d, extra)
        return ws.data_ptr(), ws.numel()

    @staticmethod
    def _chk(*ts):
        for t in ts:
            if t is not None:
                assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), \
                    (t.dtype, t.device, t.shape, t.stride())

    # ------------------------------------------------------------ node ops
    def lin(self, W, col0, ncol, X, b=None, act_in=False, out=None, add=False, bscale=1.0):
        M, ldw = W.shape
        N = X.shape[1]
        assert X.shape[0] == ncol
        if out is None:
            out = self.empty(M, N)
            add = False
        self._chk(W, X, b, out)
        _call("pfsgnn_lin", W.data_ptr() + 4 * col0, ldw, M, ncol, X.data_ptr(), N, _ptr(b),
              float(bscale), int(act_in), out.data_ptr(), int(add), _stream())
        return out

    def lin_gather(self, W, col0, ncol, X, gathers, b=None):
        """W[:, col0:col0+ncol] . X + b + sum_j G_j[:, idx_j] (up to two
        (G [M, ld], idx int32 [N]) pairs), one launch."""
        M, ldw = W.shape
        N = X.shape[1]
        out = self.empty(M, N)
        self._chk(W, X, b, out)
        g = list(gathers) + [(None, None)] * (2 - len(gathers))
        for G, idx in gathers:
            self._chk(G)
            assert idx.dtype == torch.int32 and idx.numel() == N and G.shape[0] == M
        _call("pfsgnn_lin_gather", W.data_ptr() + 4 * col0, ldw, M, ncol, X.data_ptr(), N, _ptr(b),
              1.0, 0, out.data_ptr(), 0, _ptr(g[0][0]), _ptr(g[0][1]),
              0 if g[0][0] is None else g[0][0].shape[1], _ptr(g[1][0]), _ptr(g[1][1]),
              0 if g[1][0] is None else g[1][0].shape[1], _stream())
        return out

    def lin_t(self, W, col0, ncol, dY, z=None, out=None, add=False):
        M, ldw = W.shape
        N = dY.shape[1]
        if out is None:
            out = self.empty(ncol, N)
            add = False
        self._chk(W, dY, z, out)
        _call("pfsgnn_lin_t", W.data_ptr() + 4 * col0, ldw, M, ncol, dY.data_ptr(), N, _ptr(z),
              out.data_ptr(), int(add), _stream())
        return out

    def linear_batch(self, ops):
        """Independent small products in one launch (pfsgnn_gemm_multi).  ops:
        ("cat", W, segs, N, b) -> Y = W . cat(segs) + b (a new [M, N] tensor), or
        ("t", W, col0, ncol, dY, out, add) -> out (+)= W[:, col0:col0+ncol]^T dY.
        Returns the outputs in order."""
        arr = (GemmJob * len(ops))()
        keep, outs = [], []
        for i, op in enumerate(ops):
            if op[0] == "cat":
                _, W, segs, N, b = op
                M, ldw = W.shape
                Y = self.empty(M, N)
                sg = self._segs(segs, N)
                self._chk(W, b)
                arr[i] = GemmJob(W.data_ptr(), ldw, 0, M, 0, sg, len(segs), N, _ptr(b), 1.0, 0,
                                 None, Y.data_ptr(), 0)
                keep.append(sg)
            else:
                _, W, col0, ncol, dY, Y, add = op
                Mw, ldw = W.shape
                N = dY.shape[1]
                if Y is None:
                    Y, add = self.empty(ncol, N), False
                self._chk(W, dY, Y)
                sg = self._segs([(dY, 0, False)], N)
                arr[i] = GemmJob(W.data_ptr() + 4 * col0, ldw, 1, ncol, Mw, sg, 1, N, None, 1.0,
                                 0, None, Y.data_ptr(), int(add))
                keep.append(sg)
            outs.append(Y)
        _call("pfsgnn_gemm_multi", arr, len(ops), _stream())
        return outs

    # ----------------------------------------------- deferred weight gradients
    # Between defer_begin() and defer_flush(), wgrad/wgrad_cat only record a
    # job; the flush computes them all in a few launches (pfsgnn_wgrad_multi:
    # jobs of one kernel shape share a launch, the reductions are batched).
    # The engine defers over a backward pass: its weight gradients are read
    # only by the optimizer, and the jobs' inputs are activations and
    # gradients that no later op of the pass writes (engine.Engine.backward).
    # The fused edge backward kernels' own weight reductions are deferred the
    # same way inside the library (pfsgnn_defer_begin / _end), their partials
    # in a second arena sized by the previous pass (warm-up sizes it before
    # any graph capture; a pass that does not fit reduces at once).
    def defer_begin(self):
        self._jobs = []
        ea = getattr(self, "_earena", None)
        _call("pfsgnn_defer_begin", None if ea is None else ea.data_ptr(),
              0 if ea is None else ea.numel())

    def defer_flush(self):
        jobs, self._jobs = getattr(self, "_jobs", None), None
        if jobs is None:
            return
        arr, arena = None, None
        if jobs:
            arr = (WgJob * len(jobs))()
            for i, (job, _keep) in enumerate(jobs):
                arr[i] = job
            need = lib().pfsgnn_wgrad_multi_bytes(arr, len(jobs))
            if need == 0:
                raise RuntimeError("pfsgnn_wgrad_multi_bytes: " + lib().pfsgnn_last_error().decode())
            arena = getattr(self, "_arena", None)
            if arena is None or arena.numel() < need:
                # grown during warm-up, before any graph capture; a replaced arena
                # stays alive (see __init__)
                if arena is not None:
                    self._retired.append(arena)
                self._arena = arena = torch.empty(max(need, 64 << 20), dtype=torch.uint8,
                                                  device=self.device)
        # the jobs and every queued reduction of the pass in one flush
        _call("pfsgnn_defer_end_multi", arr, len(jobs), None if arena is None else arena.data_ptr(),
              0 if arena is None else arena.numel(), _stream())
        need = lib().pfsgnn_defer_need()
        ea = getattr(self, "_earena", None)
        if need and (ea is None or ea.numel() < need):
            if ea is not None:
                self._retired.append(ea)
            self._earena = torch.empty(need + (1 << 20), dtype=torch.uint8, device=self.device)

    def _wgrad_job(self, dY, arr, nseg, N, act_in, dW, db, dbscale, keep):
        job = WgJob(dY.data_ptr(), dY.shape[0], arr, nseg, N, int(act_in), dW.data_ptr(),
                    dW.shape[1], _ptr(db), float(dbscale))
        self._jobs.append((job, (arr, dY, dW, db) + tuple(keep)))

    def wgrad(self, dY, X, dW, col0=0, db=None, act_in=False, dbscale=1.0):
        M, N = dY.shape
        K = X.shape[0]
        self._chk(dY, X, dW, db)
        if getattr(self, "_jobs", None) is not None:
            self._wgrad_job(dY, self._segs([(X, col0, False)], N), 1, N, act_in, dW, db, dbscale,
                            (X,))
            return
        ws, wsb = self._wsargs(getattr(self, "_dims", None))
        _call("pfsgnn_wgrad", dY.data_ptr(), M, X.data_ptr(), K, N, int(act_in),
              dW.data_ptr() + 4 * col0, dW.shape[1], _ptr(db), float(dbscale), ws, wsb, _stream())

    def _segs(self, segs, N):
        """[(X, col, per_graph)] -> ctypes pfsgnn_seg array; per_graph segments
        are [rows, G] tensors broadcast over the N // G nodes of each graph."""
        arr = (Seg * len(segs))()
        for i, (X, col, bc) in enumerate(segs):
            self._chk(X)
            assert (N % X.shape[1] == 0) if bc else (X.shape[1] == N), (X.shape, N, bc)
            arr[i].x = X.data_ptr()
            arr[i].rows = X.shape[0]
            arr[i].col = int(col)
            arr[i].per_graph = N // X.shape[1] if bc else 0
        return arr

    def lin_cat(self, W, segs, N, b=None, act_in=False, out=None, add=False, bscale=1.0):
        """Y (+)= sum_s W[:, col_s:col_s+rows_s] @ act(X_s[, broadcast per graph]) + bscale*b."""
        M, ldw = W.shape
        if out is None:
            out = self.empty(M, N)
            add = False
        self._chk(W, b, out)
        arr = self._segs(segs, N)
        _call("pfsgnn_lin_cat", W.data_ptr(), ldw, M, arr, len(segs), N, _ptr(b), float(bscale),
              int(act_in), out.data_ptr(), int(add), _stream())
        return out

    def wgrad_cat(self, dY, segs, dW, db=None, act_in=False, dbscale=1.0):
        """dW[:, col_s:col_s+rows_s] += dY @ act(X_s)^T; db += dbscale * dY.sum(1)."""
        M, N = dY.shape
        self._chk(dY, dW, db)
        arr = self._segs(segs, N)
        if getattr(self, "_jobs", None) is not None:
            self._wgrad_job(dY, arr, len(segs), N, act_in, dW, db, dbscale,
                            tuple(X for X, _, _ in segs))
            return
        ws, wsb = self._wsargs(getattr(self, "_dims", None))
        _call("pfsgnn_wgrad_cat", dY.data_ptr(), M, arr, len(segs), N, int(act_in), dW.data_ptr(),
              dW.shape[1], _ptr(db), float(dbscale), ws, wsb, _stream())

    # ------------------------------------------------------- fused node MLPs
    def mlp_fwd(self, segs, N, W1, b1, W2, b2, bn=None, save_z=True):
        """MLP (gnn.py:65) over a concatenated node input (+ training BatchNorm1d
        when ``bn`` = (gamma, beta, running_mean, running_var, momentum, eps)).
        Returns (Y, Z, Yp, mu, var): Y the module output, Z the saved
        pre-activation, Yp the pre-norm output (Y itself without bn)."""
        H, ldw1 = W1.shape
        O = W2.shape[0]
        self._chk(W1, b1, W2, b2)
        arr = self._segs(segs, N)
        Z = self.empty(H, N) if save_z else None
        Yp = self.empty(O, N)
        g = bt = rm = rv = None
        mom, eps = 0.0, 0.0
        Y = mu = var = None
        if bn is not None:
            g, bt, rm, rv, mom, eps = bn
            self._chk(g, bt, rm, rv)
            Y, mu, var = self.empty(O, N), self.empty(O), self.empty(O)
        ws, wsb = self._wsargs(getattr(self, "_dims", None))
        _call("pfsgnn_mlp_fwd", arr, len(segs), N, W1.data_ptr(), ldw1, H, b1.data_ptr(),
              W2.data_ptr(), O, b2.data_ptr(), _ptr(Z), Yp.data_ptr(), _ptr(g), _ptr(bt), _ptr(rm),
              _ptr(rv), float(mom), float(eps), _ptr(Y), _ptr(mu), _ptr(var), ws, wsb, _stream())
        return (Yp if Y is None else Y), Z, Yp, mu, var

    def mlp_fwd_epi(self, segs, N, W1, b1, W2, b2, bn, epi):
        """mlp_fwd with BatchNorm + up to two linear maps of the normalised output
        done in the normalising pass: ``epi`` = [(W, col0, nk, b)] ->
        W[:, col0:col0+O] . Y + b ([nk, N] each, returned as a 6th item)."""
        H, ldw1 = W1.shape
        O = W2.shape[0]
        self._chk(W1, b1, W2, b2)
        arr = self._segs(segs, N)
        Z, Yp = self.empty(H, N), self.empty(O, N)
        g, bt, rm, rv, mom, eps = bn
        self._chk(g, bt, rm, rv)
        Y, mu, var = self.empty(O, N), self.empty(O), self.empty(O)
        em = (LinMap * len(epi))()
        outs = []
        for i, (W, col0, nk, b) in enumerate(epi):
            self._chk(W, b)
            assert col0 + O <= W.shape[1] and nk <= W.shape[0]
            o = self.empty(nk, N)
            em[i] = LinMap(W.data_ptr(), W.shape[1], int(col0), int(nk), _ptr(b), o.data_ptr())
            outs.append(o)
        ws, wsb = self._wsargs(getattr(self, "_dims", None))
        _call("pfsgnn_mlp_fwd_epi", arr, len(segs), N, W1.data_ptr(), ldw1, H, b1.data_ptr(),
              W2.data_ptr(), O, b2.data_ptr(), Z.data_ptr(), Yp.data_ptr(), g.data_ptr(),
              bt.data_ptr(), _ptr(rm), _ptr(rv), float(mom), float(eps), Y.data_ptr(),
              mu.data_ptr(), var.data_ptr(), em, len(epi), ws, wsb, _stream())
        return Y, Z, Yp, mu, var, outs

    def target_block_fwd(self, d, y, sc, sh, Rs, Wt1, Wt2, bt2, tmask, xt, u, W1, b1, W2, b2,
                         bn, xs, gW1, gb1, gW2, gb2, gw, reps, nxt=None):
        """target_fwd (TModel's per-edge layer) + target_global_fwd on a complete
        batch, the class side in one launch (pfsgnn_target_block_fwd).  -> dict
        with target_global_fwd's keys plus hsum and agg."""
        F, G, NC, NT = d.F, d.G, d.NC, d.NT
        H = W1.shape[0]
        assert W1.shape == (4 * F, 4 * F) and W2.shape == (F, 4 * F) and Wt2.shape == (2 * F, 2 * F)
        self._chk(y, sc, sh, Rs, Wt1, Wt2, bt2, xt, u, W1, b1, W2, b2, xs, gW1, gb1, gW2, gb2, gw)
        g, bt, rm, rv, mom, eps = bn
        self._chk(g, bt, rm, rv)
        gH = gW1.shape[0]
        r = dict(hsum=self.empty(2 * F, NT), agg=self.empty(2 * F, NT), Z=self.empty(H, NT),
                 Yp=self.empty(F, NT), xt=self.empty(F, NT), mu=self.empty(F), var=self.empty(F),
                 means=self.empty(2 * F, G), gZ=self.empty(gH, G), gV=self.empty(F, G),
                 u=self.empty(F, G))
        rms = (self.empty(F, G), self.empty(G), self.empty(G)) if gw is not None else None
        y1, r1, r2 = rms if rms is not None else (None, None, None)
        We = be_ = Ws = bs = Pt = Qt = None
        if nxt is not None:
            We, be_, Ws, bs = nxt
            self._chk(We, be_, Ws, bs)
            assert We.shape == (4 * F, 4 * F) and Ws.shape == (2 * F, 2 * F)
            Pt, Qt = self.empty(4 * F, NT), self.empty(2 * F, NT)
        a = BlockTail(G=G, NF=d.NF, NC=NC, F=F, y=y.data_ptr(), sc=_ptr(sc), sh=_ptr(sh),
                      Rs=Rs.data_ptr(), Wt1=Wt1.data_ptr(), Wt2=Wt2.data_ptr(),
                      bt2=bt2.data_ptr(), tmask=_ptr(tmask), hsum=r["hsum"].data_ptr(),
                      agg=r["agg"].data_ptr(), xt=xt.data_ptr(), u=u.data_ptr(),
                      W1=W1.data_ptr(), b1=b1.data_ptr(), W2=W2.data_ptr(), b2=b2.data_ptr(),
                      gamma=g.data_ptr(), beta=bt.data_ptr(), Z=r["Z"].data_ptr(),
                      Yp=r["Yp"].data_ptr(), rm=_ptr(rm), rv=_ptr(rv), xt_new=r["xt"].data_ptr(),
                      mu=r["mu"].data_ptr(), var=r["var"].data_ptr(), momentum=float(mom),
                      eps=float(eps), xs=xs.data_ptr(), gW1=gW1.data_ptr(), gb1=gb1.data_ptr(),
                      gW2=gW2.data_ptr(), gb2=gb2.data_ptr(), gw=_ptr(gw), gH=gH,
                      reps=float(reps), means=r["means"].data_ptr(), gZ=r["gZ"].data_ptr(),
                      gV=r["gV"].data_ptr(), unew=r["u"].data_ptr(), y1=_ptr(y1), r1=_ptr(r1),
                      r2=_ptr(r2), We=_ptr(We), be=_ptr(be_), Ws=_ptr(Ws), bs=_ptr(bs),
                      Pt=_ptr(Pt), Qt=_ptr(Qt))
        ws, wsb = self._wsargs(d)
        _call("pfsgnn_target_block_fwd", ctypes.byref(a), ws, wsb, _stream())
        r["rms"], r["Pt"], r["Qt"] = rms, Pt, Qt
        return r

    def target_class_bwd(self, d, pend, gu_up, V, w, rms, gZ, gW1, gW2, gV, gdZ, dwp, gu, g_xs,
                         g_xt, Yp, mu, var, gamma, eps, dgamma, dbeta, Z, W1, W2, Wt2, gxt_in):
        """The class side of a block's backward in one launch
        (pfsgnn_target_class_bwd): pending u-gradient sums into gu_up, the
        GlobalModel backward, the means broadcast, TModel node_mlp_2 + BatchNorm
        backward and g_hsum = Wt2^T g_agg.  -> dict(dYp, dZ, g_agg, gu_t, g_hsum)."""
        F, NT = d.F, d.NT
        H = W1.shape[0]
        assert len(pend) <= 4 and W1.shape == (4 * F, 4 * F) and W2.shape == (F, 4 * F)
        self._chk(gu_up, V, w, gZ, gW1, gW2, gV, gdZ, dwp, gu, g_xs, g_xt, Yp, mu, var, gamma,
                  dgamma, dbeta, Z, W1, W2, Wt2, gxt_in, *pend)
        r = dict(dYp=self.empty(F, NT), dZ=self.empty(H, NT), g_agg=self.empty(2 * F, NT),
                 gu_t=self.empty(F, NT), g_hsum=self.empty(2 * F, NT))
        y1, r1, r2 = rms if rms is not None else (None, None, None)
        a = ClassBwd(G=d.G, NF=d.NF, NC=d.NC, F=F, npend=len(pend), gH=gW1.shape[0],
                     eps=float(eps))
        for i, X in enumerate(pend):
            a.pend[i] = X.data_ptr()
            a.pend_n[i] = X.shape[1] // d.G
        for k, v in dict(V=V, w=w, y1=y1, r1=r1, r2=r2, gZ=gZ, gW1=gW1, gW2=gW2, gu_up=gu_up,
                         gV=gV, gdZ=gdZ, dwp=dwp, gu=gu, g_xs=g_xs, g_xt=g_xt, Yp=Yp, mu=mu,
                         var=var, gamma=gamma, Z=Z, W1=W1, W2=W2, Wt2=Wt2, dgamma=dgamma,
                         dbeta=dbeta, dYp=r["dYp"], dZ=r["dZ"], gxt_in=gxt_in,
                         g_agg=r["g_agg"], gu_t=r["gu_t"], g_hsum=r["g_hsum"]).items():
            setattr(a, k, _ptr(v))
        ws, wsb = self._wsargs(d)
        _call("pfsgnn_target_class_bwd", ctypes.byref(a), ws, wsb, _stream())
        return r

    def sync_faults(self):
        """Device-wide barrier time-outs since load (pfsgnn_sync_faults; 0 when healthy)."""
        n = ctypes.c_uint(0)
        _call("pfsgnn_sync_faults", ctypes.byref(n))
        return n.value

    def target_global_fwd(self, segs, G, NC, W1, b1, W2, b2, bn, xs, NF, u, gW1, gb1, gW2, gb2,
                          gw, reps, nxt=None):
        """TModel's node_mlp_2 + BatchNorm1d (gnn.py:191-192) and the GlobalModel
        (gnn.py:218-223), + with ``nxt`` = (We, be, Ws, bs) the next block's
        per-class parts Pt, Qt (pfsgnn_target_global_fwd).  -> dict."""
        H, ldw1 = W1.shape
        F = W2.shape[0]
        N = G * NC
        gH = gW1.shape[0]
        self._chk(W1, b1, W2, b2, xs, u, gW1, gb1, gW2, gb2, gw)
        arr = self._segs(segs, N)
        g, bt, rm, rv, mom, eps = bn
        self._chk(g, bt, rm, rv)
        r = dict(Z=self.empty(H, N), Yp=self.empty(F, N), xt=self.empty(F, N), mu=self.empty(F),
                 var=self.empty(F), means=self.empty(2 * F, G), gZ=self.empty(gH, G),
                 gV=self.empty(F, G), u=self.empty(F, G))
        rms = (self.empty(F, G), self.empty(G), self.empty(G)) if gw is not None else None
        y1, r1, r2 = rms if rms is not None else (None, None, None)
        We = be = Ws = bs = Pt = Qt = None
        if nxt is not None:
            We, be, Ws, bs = nxt
            self._chk(We, be, Ws, bs)
            assert We.shape == (4 * F, 4 * F) and Ws.shape == (2 * F, 2 * F)
            Pt, Qt = self.empty(4 * F, N), self.empty(2 * F, N)
        ws, wsb = self._wsargs(getattr(self, "_dims", None))
        _call("pfsgnn_target_global_fwd", arr, len(segs), G, NC, W1.data_ptr(), ldw1, H,
              b1.data_ptr(), W2.data_ptr(), F, b2.data_ptr(), r["Z"].data_ptr(),
              r["Yp"].data_ptr(), g.data_ptr(), bt.data_ptr(), _ptr(rm), _ptr(rv), float(mom),
              float(eps), r["xt"].data_ptr(), r["mu"].data_ptr(), r["var"].data_ptr(),
              xs.data_ptr(), NF, u.data_ptr(), gW1.data_ptr(), gH, gb1.data_ptr(), gW2.data_ptr(),
              gb2.data_ptr(), _ptr(gw), float(reps), r["means"].data_ptr(), r["gZ"].data_ptr(),
              r["gV"].data_ptr(), r["u"].data_ptr(), _ptr(y1), _ptr(r1), _ptr(r2), _ptr(We),
              _ptr(be), _ptr(Ws), _ptr(bs), _ptr(Pt), _ptr(Qt), ws, wsb, _stream())
        r["rms"], r["Pt"], r["Qt"] = rms, Pt, Qt
        return r

    def mlp_bwd(self, dY, Z, W1, W2, K, bn=None, outs=(), bn_part=None, mom_coef=None):
        """Input side of the MLP(+BN) backward.  ``bn`` = (Yp, mu, var, gamma, eps,
        dgamma, dbeta) or None; ``outs`` = [(tensor or None, rows, add)] covering
        the K input rows (empty: no input gradient); ``bn_part``: the BatchNorm
        sums' partials the producer of dY already made (target_bwd's
        ``bn_sums``), else they are summed here; ``mom_coef`` = (mom, coef, k0,
        n): input rows [k0, k0 + 4C) are SModel's moment gradients, turned into
        moment_coef(mom, ., n)'s coefficients in coef instead of written.
        Returns (dYp, dZ)."""
        H, ldw1 = W1.shape
        O, N = dY.shape
        dY = dY.contiguous()
        self._chk(dY, Z, W1, W2)
        dZ = self.empty(H, N)
        Yp = mu = var = g = dg = db = None
        eps = 0.0
        dYp = dY
        if bn is not None:
            Yp, mu, var, g, eps, dg, db = bn
            self._chk(Yp, mu, var, g, dg, db)
            dYp = self.empty(O, N)
        arr = (OSeg * max(1, len(outs)))()
        for i, (t, rows, add) in enumerate(outs):
            if t is not None:
                self._chk(t)
                assert t.shape == (rows, N), (t.shape, rows, N)
            arr[i].x = None if t is None else t.data_ptr()
            arr[i].rows = int(rows)
            arr[i].add = int(bool(add))
        ws, wsb = self._wsargs(getattr(self, "_dims", None))
        if bn_part is not None or mom_coef is not None:
            nparts = 0
            if bn_part is not None:
                assert bn is not None and bn_part.shape == ((N + 63) // 64, 32), bn_part.shape
                self._chk(bn_part)
                nparts = bn_part.shape[0]
            mom = coef = None
            k0 = C = n = 0
            if mom_coef is not None:
                mom, coef, k0, n = mom_coef
                self._chk(mom, coef)
                C = mom.shape[1]
                assert mom.shape == (4, C, N) and coef.shape == (4, C, N), (mom.shape, coef.shape)
            _call("pfsgnn_mlp_bwd_pre", dY.data_ptr(), N, _ptr(Yp), _ptr(mu), _ptr(var), _ptr(g),
                  float(eps), _ptr(dg), _ptr(db), Z.data_ptr(), W1.data_ptr(), ldw1, H, int(K),
                  W2.data_ptr(), O, None if bn is None else dYp.data_ptr(), dZ.data_ptr(), arr,
                  len(outs), _ptr(bn_part), nparts, _ptr(mom), _ptr(coef), int(k0), int(C),
                  int(n), ws, wsb, _stream())
            return dYp, dZ
        _call("pfsgnn_mlp_bwd", dY.data_ptr(), N, _ptr(Yp), _ptr(mu), _ptr(var), _ptr(g),
              float(eps), _ptr(dg), _ptr(db), Z.data_ptr(), W1.data_ptr(), ldw1, H, int(K),
              W2.data_ptr(), O, None if bn is None else dYp.data_ptr(), dZ.data_ptr(), arr,
              len(outs), ws, wsb, _stream())
        return dYp, dZ

    def bn_fwd(self, X, gamma, beta, rm, rv, momentum, eps):
        C, N = X.shape
        Y, mu, var = self.empty(C, N), self.empty(C), self.empty(C)
        self._chk(X, gamma, beta, rm, rv)
        ws, wsb = self._wsargs(getattr(self, "_dims", None))
        _call("pfsgnn_bn_fwd", X.data_ptr(), C, N, gamma.data_ptr(), beta.data_ptr(), _ptr(rm),
              _ptr(rv), float(momentum), float(eps), Y.data_ptr(), mu.data_ptr(), var.data_ptr(),
              ws, wsb, _stream())
        return Y, mu, var

    def bn_bwd(self, dY, X, mu, var, gamma, eps, dgamma, dbeta):
        C, N = X.shape
        dX = self.empty(C, N)
        dY = dY.contiguous()
        self._chk(dY, X, mu, var, gamma, dgamma, dbeta)
        ws, wsb = self._wsargs(getattr(self, "_dims", None))
        _call("pfsgnn_bn_bwd", dY.data_ptr(), X.data_ptr(), mu.data_ptr(), var.data_ptr(),
              gamma.data_ptr(), float(eps), C, N, dX.data_ptr(), dgamma.data_ptr(),
              dbeta.data_ptr(), ws, wsb, _stream())
        return dX

    def graph_reduce(self, X, G, mean=False, out=None):
        """Per-graph sum (mean) of a node table; with ``out`` it is accumulated."""
        C, N = X.shape
        self._chk(X)
        if out is not None:
            self._chk(out)
            _call("pfsgnn_graph_reduce_add", X.data_ptr(), C, G, N // G, int(mean),
                  out.data_ptr(), _stream())
            return out
        out = self.empty(C, G)
        _call("pfsgnn_graph_reduce", X.data_ptr(), C, G, N // G, int(mean), out.data_ptr(),
              _stream())
        return out

    def graph_reduce_multi(self, Xs, G, out):
        """out[c][g] += per-graph sums of every X in Xs (one launch)."""
        self._chk(out, *Xs)
        m = len(Xs)
        arr = (ctypes.c_void_p * m)(*[X.data_ptr() for X in Xs])
        ns = (ctypes.c_int * m)(*[X.shape[1] // G for X in Xs])
        for X in Xs:
            assert X.shape[0] == out.shape[0] and X.shape[1] % G == 0
        _call("pfsgnn_graph_reduce_multi", arr, ns, m, out.shape[0], G, out.data_ptr(), _stream())
        return out

    def graph_bcast_add(self, out, src, scale=1.0):
        C, N = out.shape
        G = src.shape[1]
        src = src.contiguous()
        self._chk(out, src)
        _call("pfsgnn_graph_bcast_add", out.data_ptr(), C, G, N // G, src.data_ptr(),
              float(scale), _stream())
        return out

    def graph_mean2(self, X1, X2, G):
        """[2C, G]: per-graph means of X1 (rows 0..C) and X2 (rows C..2C)."""
        C = X1.shape[0]
        self._chk(X1, X2)
        out = self.empty(2 * C, G)
        _call("pfsgnn_graph_mean2", X1.data_ptr(), X1.shape[1] // G, X2.data_ptr(),
              X2.shape[1] // G, C, G, out.data_ptr(), _stream())
        return out

    def graph_bcast_add2(self, out1, s1, out2, s2, src):
        C, G = src.shape[0] // 2, src.shape[1]
        src = src.contiguous()
        self._chk(out1, out2, src)
        _call("pfsgnn_graph_bcast_add2", out1.data_ptr(), out1.shape[1] // G, float(s1),
              out2.data_ptr(), out2.shape[1] // G, float(s2), C, G, src.data_ptr(), _stream())

    def rms2_fwd(self, X, w, eps):
        C, G = X.shape
        Y, y1, r1, r2 = self.empty(C, G), self.empty(C, G), self.empty(G), self.empty(G)
        self._chk(X, w)
        _call("pfsgnn_rms2_fwd", X.data_ptr(), C, G, w.data_ptr(), float(eps), Y.data_ptr(),
              y1.data_ptr(), r1.data_ptr(), r2.data_ptr(), _stream())
        return Y, (y1, r1, r2)

    def rms2_bwd(self, dY, X, w, saved, eps, dw):
        y1, r1, r2 = saved
        C, G = X.shape
        dX = self.empty(C, G)
        dY = dY.contiguous()
        self._chk(dY, X, w, dw)
        ws, wsb = self._wsargs(getattr(self, "_dims", None))
        _call("pfsgnn_rms2_bwd", dY.data_ptr(), X.data_ptr(), w.data_ptr(), y1.data_ptr(),
              r1.data_ptr(), r2.data_ptr(), C, G, float(eps), dX.data_ptr(), dw.data_ptr(), ws,
              wsb, _stream())
        return dX

    def global_fwd(self, xs, xt, u, W1, b1, W2, b2, w, eps, G):
        """The whole GlobalModel forward (gnn.py:208-223), one call (two launches).  w: the
        RMSNorm weight or None (unnormed).  -> (u_new, means [2F, G], Z, V, rms)."""
        F = u.shape[0]
        H = W1.shape[0]
        assert W1.shape[1] == 3 * F and W2.shape == (F, H)
        self._chk(xs, xt, u, W1, b1, W2, b2, w)
        means, Z, V, Y = self.empty(2 * F, G), self.empty(H, G), self.empty(F, G), self.empty(F, G)
        rms = (self.empty(F, G), self.empty(G), self.empty(G)) if w is not None else None
        y1, r1, r2 = rms if rms is not None else (None, None, None)
        _call("pfsgnn_global_fwd", xs.data_ptr(), xs.shape[1] // G, xt.data_ptr(), xt.shape[1] // G,
              u.data_ptr(), F, G, W1.data_ptr(), H, b1.data_ptr(), W2.data_ptr(), b2.data_ptr(),
              _ptr(w), float(eps), means.data_ptr(), Z.data_ptr(), V.data_ptr(), Y.data_ptr(),
              _ptr(y1), _ptr(r1), _ptr(r2), _stream())
        return Y, means, Z, V, rms

    def _ones_row(self, n):
        c = getattr(self, "_ones_cache", None)
        if c is None:
            c = self._ones_cache = {}
        if n not in c:
            c[n] = self.ones(1, n)
        return c[n]

    def global_bwd(self, dY, V, w, rms, eps, dw, Z, W1, W2, g_u, g_xs, s1, g_xt, s2):
        """Backward of global_fwd, one call (two launches; + the RMSNorm weight gradient as a
        deferred weight-gradient job).  Accumulates into g_u, g_xs, g_xt and dw;
        -> (gV, dZ) for the MLP's weight gradients."""
        F, G = V.shape
        H = W1.shape[0]
        dY = dY.contiguous()
        self._chk(dY, V, w, Z, W1, W2, g_u, g_xs, g_xt)
        gV, dZ, gm = self.empty(F, G), self.empty(H, G), self.empty(2 * F, G)
        dwp = self.empty(F, G) if w is not None else None
        y1, r1, r2 = rms if rms is not None else (None, None, None)
        _call("pfsgnn_global_bwd", dY.data_ptr(), V.data_ptr(), _ptr(w), _ptr(y1), _ptr(r1),
              _ptr(r2), F, G, Z.data_ptr(), H, W1.data_ptr(), W2.data_ptr(), gV.data_ptr(),
              dZ.data_ptr(), _ptr(dwp), g_u.data_ptr(), gm.data_ptr(), g_xs.data_ptr(),
              g_xs.shape[1] // G,
              float(s1), g_xt.data_ptr(), g_xt.shape[1] // G, float(s2), _stream())
        if w is not None:
            # dw[c] += sum_g dwp[c][g]: a [F, G] x [1, G]^T weight-gradient job
            self.wgrad(dwp, self._ones_row(G), dw.view(F, 1))
        return gV, dZ

    def bn2_finalize(self, mu1, var1, gamma, beta, rm, rv, n, momentum, eps):
        C = mu1.shape[0]
        sc, sh, inv1, inv2 = self.empty(C), self.empty(C), self.empty(C), self.empty(C)
        _call("pfsgnn_bn2_finalize", mu1.data_ptr(), var1.data_ptr(), gamma.data_ptr(),
              beta.data_ptr(), _ptr(rm), _ptr(rv), C, int(n), float(momentum), float(eps),
              sc.data_ptr(), sh.data_ptr(), inv1.data_ptr(), inv2.data_ptr(), _stream())
        return sc, sh, inv1, inv2

    def bn_eval_coef(self, gamma, beta, rm, rv, eps, times):
        """Eval-mode BatchNorm1d applied ``times`` times as (sc, sh)."""
        C = gamma.shape[0]
        self._chk(gamma, beta, rm, rv)
        sc, sh = self.empty(C), self.empty(C)
        _call("pfsgnn_bn_eval_coef", gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
              rv.data_ptr(), C, float(eps), int(times), sc.data_ptr(), sh.data_ptr(), _stream())
        return sc, sh

    def bn_eval_bwd_coef(self, gamma, beta, rm, rv, eps, times, Sg=None, Sgx=None, dgamma=None,
                         dbeta=None):
        """Eval-mode BatchNorm1d backward coefficients (pfsgnn_bn_eval_bwd_coef):
        -> (inv, scale); with the gradient sums (Sg, Sgx) dgamma / dbeta += the
        parameter gradients of the ``times``-fold application."""
        C = gamma.shape[0]
        self._chk(gamma, beta, rm, rv, Sg, Sgx, dgamma, dbeta)
        inv, scale = self.empty(C), self.empty(C)
        _call("pfsgnn_bn_eval_bwd_coef", gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
              rv.data_ptr(), C, float(eps), int(times), _ptr(Sg), _ptr(Sgx), inv.data_ptr(),
              scale.data_ptr(), _ptr(dgamma), _ptr(dbeta), _stream())
        return inv, scale

    def affine_rows(self, X, sc, sh):
        C, N = X.shape
        self._chk(X, sc, sh)
        Y = self.empty(C, N)
        _call("pfsgnn_affine_rows", X.data_ptr(), C, N, sc.data_ptr(), sh.data_ptr(),
              Y.data_ptr(), _stream())
        return Y

    def bn2_bwd_coef_part(self, part, mu1, var1, gamma, n, eps, dgamma, dbeta):
        """bn2_bwd_coef from per-block partials [nparts, 2C] (loss_bwd's ``bn``)."""
        C = mu1.shape[0]
        assert part.dim() == 2 and part.shape[1] == 2 * C, part.shape
        self._chk(part)
        a, g0, g1 = self.empty(C), self.empty(C), self.empty(C)
        _call("pfsgnn_bn2_bwd_coef_part", part.data_ptr(), part.shape[0], C, gamma.data_ptr(),
              mu1.data_ptr(), var1.data_ptr(), int(n), float(eps), a.data_ptr(), g0.data_ptr(),
              g1.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), _stream())
        return a, g0, g1

    def bn2_bwd_coef(self, Sg, Sgx, mu1, var1, gamma, n, eps, dgamma, dbeta):
        C = mu1.shape[0]
        a, g0, g1 = self.empty(C), self.empty(C), self.empty(C)
        _call("pfsgnn_bn2_bwd_coef", Sg.data_ptr(), Sgx.data_ptr(), mu1.data_ptr(),
              var1.data_ptr(), gamma.data_ptr(), C, int(n), float(eps), a.data_ptr(),
              g0.data_ptr(), g1.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), _stream())
        return a, g0, g1

    def moment_coef(self, mom, gst, n):
        """``n``: the messages per fiber -- an int (complete graphs: NC), or a
        general graph's fiber CSR pointer (int32 [NS+1] device tensor)."""
        _, C, NS = mom.shape
        coef = self.empty(4, C, NS)
        gst = gst.contiguous()
        self._chk(mom, gst)
        if isinstance(n, torch.Tensor):
            assert n.dtype == torch.int32 and n.is_cuda and n.numel() == NS + 1
            _call("pfsgnn_moment_coef_seg", mom.data_ptr(), gst.data_ptr(), C, NS, n.data_ptr(),
                  coef.data_ptr(), _stream())
            return coef
        _call("pfsgnn_moment_coef", mom.data_ptr(), gst.data_ptr(), C, NS, int(n), coef.data_ptr(),
              _stream())
        return coef

    # ------------------------------------------------------------ edge ops
    def _set_dims(self, d):
        self._dims = d

    @staticmethod
    def _composed(d):
        """A general batch without a sliced layout: the composed ops (pfsgnn.sparse)."""
        return d.sp is not None and d.sp.sl is None

    def _ecall(self, op, d, **fields):
        """Edge op `op` of the C ABI: pfsgnn_<op>(its argument struct, workspace,
        stream).  ``fields``: the struct's tensors (None: NULL) and scalars after
        the head, which is the batch ``d`` and its sliced layout."""
        a = EDGE_ARGS[op](G=d.G, NF=d.NF, NC=d.NC, F=d.F,
                          sl=d.sp.sl.ref if d.sp is not None else None)
        for k, v in fields.items():
            setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        ws, wsb = self._wsargs(d)
        _call("pfsgnn_" + op, ctypes.byref(a), ws, wsb, _stream())

    def edge_mlp_fwd(self, d, xe, xsc, xsh, Ps, Pt, W1, W2, b2):
        if self._composed(d):
            return self._sp.edge_mlp_fwd(d, xe, xsc, xsh, Ps, Pt, W1, W2, b2)
        self._set_dims(d)
        y, mu, var = self.empty(d.F, d.EP), self.empty(d.F), self.empty(d.F)
        self._chk(xe, Ps, Pt, W1, W2, b2)
        self._ecall("edge_mlp_fwd", d, xe=xe, xsc=xsc, xsh=xsh, Ps=Ps, Pt=Pt, W1=W1, W2=W2, b2=b2,
                    y=y, mu=mu, var=var)
        return y, mu, var

    def edge_mlp_fwd_bn(self, d, xe, xsc, xsh, Ps, Pt, W1, W2, b2, bn):
        """edge_mlp_fwd + bn2_finalize in one call; ``bn`` = (gamma, beta,
        running_mean, running_var, momentum, eps).  -> y, mu1, var1, sc, sh, inv1."""
        gamma, beta, rm, rv, momentum, eps = bn
        if self._composed(d):
            y, mu, var = self._sp.edge_mlp_fwd(d, xe, xsc, xsh, Ps, Pt, W1, W2, b2)
            sc, sh, inv1, _ = self.bn2_finalize(mu, var, gamma, beta, rm, rv, d.E, momentum, eps)
            return y, mu, var, sc, sh, inv1
        self._set_dims(d)
        F = d.F
        y, mu, var = self.empty(F, d.EP), self.empty(F), self.empty(F)
        sc, sh, inv1, inv2 = self.empty(F), self.empty(F), self.empty(F), self.empty(F)
        self._chk(xe, Ps, Pt, W1, W2, b2, gamma, beta, rm, rv)
        self._ecall("edge_mlp_fwd", d, xe=xe, xsc=xsc, xsh=xsh, Ps=Ps, Pt=Pt, W1=W1, W2=W2, b2=b2,
                    y=y, mu=mu, var=var, gamma=gamma, beta=beta, rm=rm, rv=rv,
                    momentum=float(momentum), eps=float(eps), sc=sc, sh=sh, inv1=inv1, inv2=inv2)
        return y, mu, var, sc, sh, inv1

    def source_fwd(self, d, y, sc, sh, Qt, Ws1, Ws2, bs2, hs_out, msg=None):
        """-> mom; ``msg`` (from ``msg_cache(d)``) receives the per-edge messages
        for source_bwd."""
        if self._composed(d):
            return self._sp.source_fwd(d, y, sc, sh, Qt, Ws1, Ws2, bs2, hs_out)
        mom = self.empty(4, 2 * d.F, d.NS)
        self._chk(y, Qt, Ws1, Ws2, bs2, hs_out)
        self._ecall("source_fwd", d, y=y, sc=sc, sh=sh, Qt=Qt, Ws1=Ws1, Ws2=Ws2, bs2=bs2, mom=mom,
                    hs=hs_out, msg=msg)
        return mom

    def msg_cache(self, d):
        """A buffer for SModel's per-edge messages [2F][E] (pfsgnn_msg_bytes),
        or None when the current path recomputes them in the backward."""
        if self._composed(d) or d.sp is not None:
            return None
        n = lib().pfsgnn_msg_bytes(d.G, d.NF, d.NC, d.F)
        return torch.empty(n // 4, dtype=torch.float32, device=self.device) if n else None

    def tmask(self, d):
        """A buffer for TModel's LeakyReLU mask (pfsgnn_tmask_bytes), or None
        when the current edge path recomputes that layer in the backward."""
        if self._composed(d):
            return None
        if d.sp is not None:
            n = lib().pfsgnn_sl_tmask_bytes(d.sp.sl.ref, d.F)
            return torch.empty(n, dtype=torch.uint8, device=self.device) if n else None
        n = lib().pfsgnn_tmask_bytes(d.G, d.NF, d.NC, d.F)
        return torch.empty(n, dtype=torch.uint8, device=self.device) if n else None

    def target_fwd(self, d, y, sc, sh, Rs, Wt1, agg=None, tmask=None):
        """-> hsum; with ``agg`` = (Wt2, bt2, bscale) -> (hsum, Wt2 hsum + bscale bt2),
        the second Linear done in the class reduction's epilogue.  ``tmask``
        (from ``tmask(d)``) receives TModel's LeakyReLU mask for the backward."""
        if self._composed(d):
            hsum = self._sp.target_fwd(d, y, sc, sh, Rs, Wt1)
            if agg is None:
                return hsum
            Wt2, bt2, bscale = agg
            return hsum, self.lin(Wt2, 0, Wt2.shape[1], hsum, b=bt2, bscale=bscale)
        hsum = self.empty(2 * d.F, d.NT)
        Wt2 = bt2 = A = None
        bscale = 1.0
        if agg is not None:
            Wt2, bt2, bscale = agg
            self._chk(Wt2, bt2)
            assert Wt2.shape == (2 * d.F, 2 * d.F)
            A = self.empty(2 * d.F, d.NT)
        self._ecall("target_fwd", d, y=y, sc=sc, sh=sh, Rs=Rs, Wt1=Wt1, hsum=hsum, Wt2=Wt2, bt2=bt2,
                    bscale=float(bscale), agg=A, tmask=tmask)
        return hsum if agg is None else (hsum, A)

    def tbwd_fold(self, d):
        """Whether the folded pair exists for this batch on the current edge
        path (pfsgnn_tbwd_fold): target_bwd(fold=True) + source_bwd(dWt1=...)."""
        return d.sp is None and not self._composed(d) and bool(lib().pfsgnn_tbwd_fold(d.F))

    def target_bwd(self, d, y, sc, sh, Rs, Wt1, g_hsum, dWt1, want_gxe=False, g_xs=None,
                   tmask=None, bn_sums=None, fold=False):
        """-> (GzT, gxe); with ``g_xs``: g_xs += Wt1[:, :F]^T GzT as well;
        ``tmask``: the forward's mask (target_fwd), read instead of recomputed.
        ``bn_sums`` = (Yp, mu, var, eps) of the BatchNorm whose backward reads the
        finished g_xs next (SModel's, gnn.py:154; complete graphs): its sums come
        out of the same call -> (GzT, gxe, partials for mlp_bwd's bn_part).
        ``fold`` (tbwd_fold(d), with ``tmask`` and no gxe): the mask-only form
        (the struct's ``fold``); dWt1[:, F:2F] is then left to the source_bwd
        call that follows, which must be given ``dWt1``."""
        if fold:
            # (where tbwd_fold(d) is false the entry point runs the unfolded form)
            assert tmask is not None and not want_gxe and d.sp is None
        if bn_sums is not None:
            assert g_xs is not None and not self._composed(d) and d.sp is None
        elif self._composed(d):
            out = self._sp.target_bwd(d, y, sc, sh, Rs, Wt1, g_hsum, dWt1, want_gxe=want_gxe)
            if g_xs is not None:
                self.lin_t(Wt1, 0, d.F, out[0], out=g_xs, add=True)
            return out
        self._chk(g_xs)
        GzT = self.empty(2 * d.F, d.NS)
        gxe = self.empty(d.F, d.EP) if want_gxe else None
        Yp = mu = var = part = None
        eps = 0.0
        if bn_sums is not None:
            Yp, mu, var, eps = bn_sums
            self._chk(Yp, mu, var)
            part = self.empty((d.NS + 63) // 64, 32)
        self._ecall("target_bwd", d, y=y, sc=sc, sh=sh, Rs=Rs, Wt1=Wt1, g_hsum=g_hsum.contiguous(),
                    GzT=GzT, dWt1=dWt1, gxe=gxe, g_xs=g_xs, tmask=tmask, bn_Yp=Yp, bn_mu=mu,
                    bn_var=var, bn_eps=float(eps), bn_part=part, fold=int(fold))
        return (GzT, gxe) if bn_sums is None else (GzT, gxe, part)

    def source_bwd(self, d, y, sc, sh, Qt, Ws1, Ws2, bs2, mean, coef, tpart, g_next, bnstat,
                   dWs1, dWs2, dbs2, bn2=None, g_xt=None, tmask=None, msg=None, dWt1=None):
        """-> (g_tot, GzS, Sg, Sgx).  With ``bn2`` = (gamma, var1, n, eps, dgamma,
        dbeta) (and ``bnstat``) the edge BatchNorm's backward is finished in the
        same call: -> (g_tot, GzS, None, None, (alpha, gam0, gam1)).  With
        ``g_xt``: g_xt += Ws1[:, :F]^T GzS as well.  ``dWt1``: the second half of
        the folded pair (target_bwd(fold=True)): dWt1[:, F:2F] += g_zt x^T too."""
        assert dWt1 is None or (tpart is not None and tmask is not None and d.sp is None)
        if self._composed(d):
            out = self._sp.source_bwd(d, y, sc, sh, Qt, Ws1, Ws2, bs2, mean, coef, tpart, g_next,
                                      bnstat, dWs1, dWs2, dbs2)
            if g_xt is not None:
                self.lin_t(Ws1, 0, d.F, out[1], out=g_xt, add=True)
            if bn2 is None:
                return out
            gamma, var1, n, eps, dg, db = bn2
            cf = self.bn2_bwd_coef(out[2], out[3], bnstat[0], var1, gamma, n, eps, dg, db)
            return out[0], out[1], None, None, cf
        g_tot = self.empty(d.F, d.EP)
        GzS = self.empty(2 * d.F, d.NT)
        Rs = Wt1 = g_hsum = None
        if tpart is not None:
            Rs, Wt1, g_hsum = tpart
            g_hsum = g_hsum.contiguous()
        mu1 = inv1 = Sg = Sgx = var1 = gamma = dg = db = a = g0 = g1 = None
        n, eps = 0, 0.0
        if bnstat is not None:
            mu1, inv1 = bnstat
            if bn2 is None:
                Sg, Sgx = self.empty(d.F), self.empty(d.F)
        if bn2 is not None:
            assert bnstat is not None
            gamma, var1, n, eps, dg, db = bn2
            a, g0, g1 = self.empty(d.F), self.empty(d.F), self.empty(d.F)
        self._ecall("source_bwd", d, y=y, sc=sc, sh=sh, Qt=Qt, Ws1=Ws1, Ws2=Ws2, bs2=bs2,
                    mean=mean.contiguous(), coef=coef, Rs=Rs, Wt1=Wt1, g_hsum=g_hsum,
                    g_next=g_next.contiguous() if g_next is not None else None, mu1=mu1,
                    inv1=inv1, var1=var1, gamma=gamma, n=int(n), eps=float(eps), g_tot=g_tot,
                    GzS=GzS, dWs1=dWs1, dWs2=dWs2, dbs2=dbs2, Sg=Sg, Sgx=Sgx, alpha=a, gam0=g0,
                    gam1=g1, dgamma=dg, dbeta=db, g_xt=g_xt, tmask=tmask, msg=msg, dWt1=dWt1)
        return (g_tot, GzS, Sg, Sgx) if bn2 is None else (g_tot, GzS, None, None, (a, g0, g1))

    def edge_bn_grad_sums(self, d, g, y, mu1, inv1):
        if d.sp is not None:   # (slot tensors hold 0 at padding: the column sums hold)
            return self._sp.edge_bn_grad_sums(d, g, y, mu1, inv1)
        Sg, Sgx = self.empty(d.F), self.empty(d.F)
        ws, wsb = self._wsargs(d)
        _call("pfsgnn_edge_bn_grad_sums", d.G, d.NF, d.NC, d.F, g.data_ptr(), y.data_ptr(),
              mu1.data_ptr(), inv1.data_ptr(), Sg.data_ptr(), Sgx.data_ptr(), ws, wsb, _stream())
        return Sg, Sgx

    def edge_mlp_bwd(self, d, g_tot, alpha, gam0, gam1, y, xe, xsc, xsh, Ps, Pt, W1, W2,
                     dW1, dW2, db2, want_gxe=True, nodes=None):
        """-> (gxe, GzEs, GzEt); with ``nodes`` = (g_xs, g_xt) the first Linear's
        node-input gradients are added in the reductions' epilogues and the
        result is (gxe, GzEs, GzEt, Vu), Vu = W1[:, 3F:4F]^T GzEt per class."""
        if self._composed(d):
            out = self._sp.edge_mlp_bwd(d, g_tot, alpha, gam0, gam1, y, xe, xsc, xsh, Ps, Pt, W1,
                                        W2, dW1, dW2, db2, want_gxe=want_gxe)
            if nodes is None:
                return out
            F = d.F
            self.lin_t(W1, 0, F, out[1], out=nodes[0], add=True)
            self.lin_t(W1, F, F, out[2], out=nodes[1], add=True)
            return out + (self.lin_t(W1, 3 * F, F, out[2]),)
        gxe = self.empty(d.F, d.EP) if want_gxe else None
        GzEs, GzEt = self.empty(4 * d.F, d.NS), self.empty(4 * d.F, d.NT)
        g_xs = g_xt = Vu = None
        if nodes is not None:
            g_xs, g_xt = nodes
            self._chk(g_xs, g_xt)
            Vu = self.empty(d.F, d.NT)
        self._ecall("edge_mlp_bwd", d, g_tot=g_tot, alpha=alpha, gam0=gam0, gam1=gam1, y=y, xe=xe,
                    xsc=xsc, xsh=xsh, Ps=Ps, Pt=Pt, W1=W1, W2=W2, dW1=dW1, dW2=dW2, db2=db2,
                    gxe=gxe, GzEs=GzEs, GzEt=GzEt, g_xs=g_xs, g_xt=g_xt, Vu=Vu)
        return (gxe, GzEs, GzEt) if nodes is None else (gxe, GzEs, GzEt, Vu)

    def edge_apply(self, d, y, sc, sh):
        if d.sp is not None:
            return self._sp.edge_apply(d, y, sc, sh)
        out = self.empty(d.F, d.E)
        _call("pfsgnn_edges_from_canonical", y.data_ptr(), _ptr(sc), _ptr(sh), d.G, d.NF, d.NC,
              d.F, 2, None, 0, out.data_ptr(), _stream())
        return out

    # ------------------------------------------------------------ loss
    def _seed_args(self, seed):
        """(value, device pointer): a device int64 tensor is read by the kernels
        (graph-capturable: each replay sees its current value)."""
        if isinstance(seed, torch.Tensor):
            if not seed.is_cuda or seed.dtype != torch.int64 or seed.numel() != 1:
                raise ValueError("a tensor seed must be one int64 on the device")
            return 0, seed.data_ptr()
        return int(seed) & ((1 << 64) - 1), None

    def softfloor_record(self, sharpness):
        """softfloor's coefficients [4] (r, atan(r / (1 - r)), 2 pi, 1 / pi) from a
        device float32 sharpness, on the device (pfsgnn_softfloor_record): what
        the loss kernels read when the sharpness is a tensor."""
        if (not isinstance(sharpness, torch.Tensor) or not sharpness.is_cuda
                or sharpness.dtype != torch.float32 or sharpness.numel() != 1):
            raise ValueError("a tensor sharpness must be one float32 on the device")
        rec = self.empty(4)
        _call("pfsgnn_softfloor_record", sharpness.data_ptr(), rec.data_ptr(), _stream())
        return rec

    def _sharp_args(self, sharpness):
        """(value, device record, keep-alive): a Python number goes by value; a
        device tensor is read by the kernels -- a filled record [4]
        (softfloor_record, train_advance), or one float32 sharpness, whose
        record is made here."""
        if isinstance(sharpness, torch.Tensor):
            rec = sharpness if sharpness.numel() == 4 else self.softfloor_record(sharpness)
            if (not rec.is_cuda or rec.dtype != torch.float32 or not rec.is_contiguous()
                    or rec.data_ptr() % 16):
                raise ValueError("a softfloor record must be 4 contiguous float32 on the device, "
                                 "16-byte aligned")
            return 0.0, rec.data_ptr(), rec
        return float(sharpness), None, None

    def _loss_args(self, d, sl, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, sharpness, noiselevel,
                   seed):
        """pfsgnn_loss_args with the inputs both directions share."""
        a = LossArgs(G=d.G, NF=d.NF, NC=d.NC, F=d.F)
        if sl is not None:
            a.sl, a.pos_user = sl.ref, sl.pos_user.data_ptr()
        a.y, a.sc, a.sh = y.data_ptr(), _ptr(sc), _ptr(sh)
        a.Wd1, a.bd1, a.Wd2, a.bd2 = Wd1.data_ptr(), bd1.data_ptr(), Wd2.data_ptr(), bd2.data_ptr()
        a.ci = ci.data_ptr()
        a.scale, a.noiselevel = float(scale), float(noiselevel)
        a.sharpness, a.sf_dev, a._keep = self._sharp_args(sharpness)
        a.seed, a.seed_dev = self._seed_args(seed)
        return a

    # ------------------------------------------------------------ training loop
    def train_advance(self, epoch, seed, s0, s1, nepochs, sharpness, sf):
        """epoch += 1, seed += 1, sharpness = s0 + (s1 - s0) * epoch / nepochs
        (train.py:137, in double, rounded once) and its softfloor record ``sf``
        [4], in one launch (pfsgnn_train_advance)."""
        assert epoch.dtype == torch.int64 and seed.dtype == torch.int64
        assert sharpness.dtype == torch.float32 and sf.dtype == torch.float32 and sf.numel() == 4
        _call("pfsgnn_train_advance", epoch.data_ptr(), seed.data_ptr(), float(s0), float(s1),
              int(nepochs), sharpness.data_ptr(), sf.data_ptr(), _stream())

    def train_record(self, d, nepochs, epoch, sharpness, loss, utils, variance, n_prime, ci,
                     nfields, min_sharp, losses, objective, variances, completions, comp, improved,
                     best_utility, best_loss, best_epoch):
        """An epoch's history rows and best-tracking (pfsgnn_train_record);
        ``completions`` [NT, nepochs] or None."""
        self._chk(loss, utils, variance, n_prime, ci, losses, objective, variances, completions, comp,
                  best_utility, best_loss, sharpness)
        assert min(losses.numel(), objective.numel(), variances.numel()) >= nepochs
        assert completions is None or completions.numel() >= d.NT * nepochs
        assert comp.numel() >= d.NT and ci.numel() >= 2 * d.NT and n_prime.numel() >= d.NT
        assert improved.dtype == torch.int32 and best_epoch.dtype == epoch.dtype == torch.int64
        a = TrainRecordArgs(G=d.G, NC=d.NC, nepochs=int(nepochs), nfields=float(nfields),
                            min_sharp=float(min_sharp))
        for k, v in dict(epoch=epoch, sharpness=sharpness, loss=loss, utils=utils,
                         variance=variance, n_prime=n_prime, ci=ci, losses=losses,
                         objective=objective, variances=variances, completions=completions,
                         comp=comp, improved=improved, best_utility=best_utility,
                         best_loss=best_loss, best_epoch=best_epoch).items():
            setattr(a, k, _ptr(v))
        _call("pfsgnn_train_record", ctypes.byref(a), _stream())

    def train_record_hard(self, d, nepochs, epoch, utility, over, hard_objective, hard_overtime,
                          improved_hard, best_hard_utility, best_hard_epoch):
        """An epoch's integer-objective rows and best-tracking from ``schedule``'s
        utility / over [G] (pfsgnn_train_record_hard)."""
        self._chk(utility, hard_objective, best_hard_utility)
        assert over.dtype == hard_overtime.dtype == improved_hard.dtype == torch.int32
        assert best_hard_epoch.dtype == epoch.dtype == torch.int64
        assert min(hard_objective.numel(), hard_overtime.numel()) >= nepochs
        assert min(utility.numel(), over.numel()) >= d.G
        a = TrainRecordHardArgs(G=d.G, nepochs=int(nepochs))
        for k, v in dict(epoch=epoch, utility=utility, over=over, hard_objective=hard_objective,
                         hard_overtime=hard_overtime, improved_hard=improved_hard,
                         best_hard_utility=best_hard_utility,
                         best_hard_epoch=best_hard_epoch).items():
            setattr(a, k, _ptr(v))
        _call("pfsgnn_train_record_hard", ctypes.byref(a), _stream())

    @staticmethod
    def _copy_job_array(pairs):
        """(pfsgnn_copy_job array, largest word count) of (src, dst) tensor pairs
        of equal byte size (a multiple of 4)."""
        jobs = (CopyJob * max(len(pairs), 1))()
        nmax = 0
        for j, (s, t) in zip(jobs, pairs):
            nb = s.numel() * s.element_size()
            assert s.is_contiguous() and t.is_contiguous() and s.is_cuda and t.is_cuda
            assert nb == t.numel() * t.element_size() and nb % 4 == 0, (s.shape, t.shape)
            j.src, j.dst, j.n = s.data_ptr(), t.data_ptr(), nb // 4
            nmax = max(nmax, nb // 4)
        return jobs, nmax

    def copy_jobs(self, pairs):
        """The device job list of ``copy_if`` for buffers at fixed addresses."""
        jobs, nmax = self._copy_job_array(pairs)
        host = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8)
        return dict(dev=host.to(self.device), n=len(pairs), nmax=nmax, keep=list(pairs))

    def copy_if(self, flag, jobs, extra=()):
        """Every job of ``jobs`` (copy_jobs) and of the (src, dst) pairs ``extra``
        (at most 4: buffers whose address may differ from step to step) when the
        device int32 ``flag`` is set, in one launch (pfsgnn_copy_if)."""
        assert flag.dtype == torch.int32 and flag.is_cuda
        xs, xmax = self._copy_job_array(list(extra))
        _call("pfsgnn_copy_if", flag.data_ptr(), jobs["dev"].data_ptr(), jobs["n"], xs, len(extra),
              max(jobs["nmax"], xmax), _stream())

    @staticmethod
    def _loss_layout(d):
        """The sliced layout of a general batch (None: a complete batch).  The
        objective has no composed form: it runs on the fused sliced kernels only."""
        if d.sp is None:
            return None
        if d.sp.sl is None:
            raise NotImplementedError(
                "the training objective on a general (non-complete) batch runs on the fused "
                "sliced kernels only; this batch is on the composed path (PFSGNN_SLICED=0, more "
                "classes per graph than pfsgnn_sliced_max_nc, or a bf16 edge-state path)")
        return d.sp.sl

    def loss_fwd(self, d, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, sharpness, noiselevel, seed,
                 want_time=False):
        """On a sliced general batch (``d.sp.sl``): y is [F, EP] in slot order,
        tt [E] in the caller's edge order, and tvar is [2, NT] -- the class
        variances and, for loss_finalize, the class edge counts
        (pfsgnn_loss_fwd with sl set)."""
        sl = self._loss_layout(d)
        n_prime, fiber_time = self.empty(d.NT), self.empty(d.NS)
        tmean = self.empty(d.NT)
        tvar = self.empty(d.NT) if sl is None else self.empty(2, d.NT)
        tt = self.empty(d.E) if want_time else None
        ci = ci.contiguous()
        assert sl is None or tuple(y.shape) == (d.F, sl.EP), (tuple(y.shape), d.F, sl.EP)
        a = self._loss_args(d, sl, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, sharpness, noiselevel,
                            seed)
        a.n_prime, a.fiber_time = n_prime.data_ptr(), fiber_time.data_ptr()
        a.tmean, a.tvar, a.tt = tmean.data_ptr(), tvar.data_ptr(), _ptr(tt)
        ws, wsb = self._wsargs(d)
        _call("pfsgnn_loss_fwd", ctypes.byref(a), ws, wsb, _stream())
        return n_prime, fiber_time, tmean, tvar, tt

    # ---- the schedule ops (pfsgnn_schedule, _budget, _plan): what their wrappers share
    def _sched_out(self, a, d, fields, out, E=None):
        """Allocate (``out`` None), check and bind an op's outputs.  ``fields``
        names them in the order of the returned tuple; an output's length and
        dtype follow from its name."""
        E = d.E if E is None else E
        f32, i32, i64 = torch.float32, torch.int32, torch.int64
        spec = dict(visits=(E, i32), quot=(E, f32), start=(E, f32), n_hard=(d.NT, i32),
                    completeness=(d.NT, f32), cut=(d.NT, i64), fiber_time=(d.NS, f32),
                    used=(d.NS, f32), idle=(d.NS, f32), phase=(d.NS, i32), seg_ptr=(d.NS + 1, i64),
                    utility=(d.G, f32), over=(d.G, i32), worst=(d.G, f32))
        if out is None:
            out = tuple(torch.empty(spec[k][0], dtype=spec[k][1], device=self.device)
                        for k in fields)
        assert len(out) == len(fields)
        for k, t in zip(fields, out):
            n, dt = spec[k]
            assert t.dtype == dt and t.is_cuda and t.is_contiguous(), (k, t.dtype, t.device)
            assert t.numel() == n, (k, t.numel(), n)
            setattr(a, k, t.data_ptr())
        return out

    @staticmethod
    def _sched_batch(a, sl, mode, perm, E):
        """The batch form: sliced (``sl`` + its pos_user), or complete (``mode``, ``perm``)."""
        if sl is not None:
            a.sl, a.pos_user = sl.ref, sl.pos_user.data_ptr()
            return
        a.mode = int(mode)
        if perm is not None:
            assert perm.dtype == torch.int32 and perm.is_cuda and perm.numel() == E
            a.perm = perm.data_ptr()

    def _sched_in(self, a, d, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, total_time, nfields):
        """The lazy edge state, the decoder, the class table and the scalars
        (the edge state and the decoder may be None: ``time_in``)."""
        self._chk(y, sc, sh, Wd1, bd1, Wd2, bd2)
        assert y is None or tuple(y.shape) == (d.F, d.EP), (tuple(y.shape), d.F, d.EP)
        ci = ci.contiguous()
        assert ci.numel() >= 2 * d.NT
        for k, v in dict(y=y, sc=sc, sh=sh, Wd1=Wd1, bd1=bd1, Wd2=Wd2, bd2=bd2, ci=ci).items():
            setattr(a, k, _ptr(v))
        a.scale, a.total_time, a.nfields = float(scale), float(total_time), float(nfields)
        return ci   # (kept alive by the caller until the launch is queued)

    SCHEDULE_FIELDS = ("visits", "n_hard", "fiber_time", "completeness", "utility", "over", "worst")

    def schedule(self, d, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, total_time, nfields,
                 rounding=0, mode=1, perm=None, out=None):
        """The hard visit counts of the lazy edge state (pfsgnn_schedule) ->
        (visits [E] int32 in the caller's edge order, n [NT] int32, fiber_time
        [NS], completeness [NT], utility [G], over [G] int32, worst [G]).
        A complete batch: y canonical [F, E], ``mode`` / ``perm`` its caller
        order (0: perm, 1: fiber-major, 2: canonical); a sliced general batch
        (``d.sp.sl``): y [F, EP] in slot order.  ``out``: the seven tensors to
        write into (a loop's preallocated buffers)."""
        assert y is not None
        a = ScheduleArgs(G=d.G, NF=d.NF, NC=d.NC, F=d.F, rounding=int(rounding))
        out = self._sched_out(a, d, self.SCHEDULE_FIELDS, out)
        self._sched_batch(a, self._loss_layout(d), mode, perm, d.E)
        ci = self._sched_in(a, d, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, total_time, nfields)
        ws, wsb = self._wsargs(d)
        _call("pfsgnn_schedule", ctypes.byref(a), ws, wsb, _stream())
        return out

    def schedule_budget_max_nc(self):
        """The most classes per graph of a complete batch (pfsgnn_schedule_budget_max_nc)."""
        return int(lib().pfsgnn_schedule_budget_max_nc())

    def schedule_budget(self, d, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, total_time, nfields,
                        mode=1, perm=None, time_in=None, out=None):
        """Budgeted rounding of the lazy edge state, or of ``time_in`` [E] (the
        caller's edge order; then y, sc, sh and the decoder may be None)
        (pfsgnn_schedule_budget) -> ``schedule``'s seven tensors, then quot [E]
        (the fp32 quotient that was rounded, caller's order) and phase [NS] int32
        (bit 0: down phase, 1: bumped, 2: refused a candidate).  ``out``: the nine
        tensors to write into."""
        sl = self._loss_layout(d)
        assert time_in is not None or y is not None
        a = ScheduleBudgetArgs(G=d.G, NF=d.NF, NC=d.NC, F=d.F)
        out = self._sched_out(a, d, self.SCHEDULE_FIELDS + ("quot", "phase"), out)
        self._sched_batch(a, sl, mode, perm, d.E)
        ci = self._sched_in(a, d, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, total_time, nfields)
        if time_in is not None:
            self._chk(time_in)
            assert time_in.numel() == d.E
            a.time_in = time_in.data_ptr()
        need = lib().pfsgnn_schedule_budget_ws_bytes(d.G, d.NF, d.NC, 0 if sl is None else sl.EP)
        ws, wsb = self._wsargs(d, need)
        _call("pfsgnn_schedule_budget", ctypes.byref(a), ws, wsb, _stream())
        return out

    PLAN_FIELDS = ("visits", "start", "used", "idle", "n_hard", "completeness", "utility", "over",
                   "worst", "cut", "seg_ptr")

    def schedule_plan(self, d, ci, visits_in, total_time, nfields, *, mode=1, perm=None, sp=None,
                      cap=True, seg_edge=None, seg_start=None, out=None):
        """The observing plan of an integer schedule (pfsgnn_schedule_plan) ->
        (visits [E] int32, start [E], used [NS], idle [NS], n [NT] int32,
        completeness [NT], utility [G], over [G] int32, worst [G], cut [NT] int64,
        seg_ptr [NS + 1] int64); per-edge tensors in the caller's edge order.
        ``visits_in`` [E] int32 in the caller's order.  A complete batch gives
        ``mode`` / ``perm``; a general one its ``sparse.SparseGeo`` as ``sp``
        (``d.sp`` by default; a complete graph laid out by ``sparse_layout`` runs
        through the CSR form when its geo is passed).  ``seg_edge`` (int32) and
        ``seg_start`` (fp32), of equal length, receive the target list's
        entries below their length; without them the call only counts.
        ``out``: the eleven tensors to write into."""
        sp = d.sp if sp is None else sp
        E = d.E if sp is None else sp.E
        a = PlanArgs(G=d.G, NF=d.NF, NC=d.NC, cap=int(bool(cap)))
        out = self._sched_out(a, d, self.PLAN_FIELDS, out, E)
        assert (visits_in.dtype == torch.int32 and visits_in.is_cuda and visits_in.is_contiguous()
                and visits_in.numel() == E)
        ci = ci.contiguous()
        assert ci.numel() >= 2 * d.NT
        if sp is not None:
            a.mode, a.E = -1, E
            for k in ("src_p", "tgt_p", "user_of", "fib_ptr", "cls_ord", "cls_ptr"):
                setattr(a, k, getattr(sp, k).data_ptr())
        else:
            self._sched_batch(a, None, mode, perm, E)
        a.ci, a.visits_in = ci.data_ptr(), visits_in.data_ptr()
        a.total_time, a.nfields = float(total_time), float(nfields)
        if seg_edge is not None or seg_start is not None:
            self._chk(seg_start)
            assert seg_edge.dtype == torch.int32 and seg_edge.is_cuda and seg_edge.is_contiguous()
            assert seg_edge.numel() == seg_start.numel()
            a.seg_cap = seg_edge.numel()
            if a.seg_cap:
                a.seg_edge, a.seg_start = seg_edge.data_ptr(), seg_start.data_ptr()
        need = lib().pfsgnn_schedule_plan_ws_bytes(d.G, d.NF, d.NC, 0 if sp is None else E)
        ws, wsb = self._wsargs(None, need)
        _call("pfsgnn_schedule_plan", ctypes.byref(a), ws, wsb, _stream())
        return out

    def loss_finalize(self, d, n_prime, fiber_time, tvar, ci, pclass, pfiber, total_time, nfields,
                      wutils, wvar, gscale=1.0):
        loss, utils, variance = self.empty(d.G), self.empty(d.G), self.empty(d.G)
        Gn, Gf, Gv = self.empty(d.NT), self.empty(d.NS), self.empty(d.NT)
        ci = ci.contiguous()
        sl = self._loss_layout(d)
        assert tvar.is_contiguous() and tvar.numel() == (d.NT if sl is None else 2 * d.NT)
        _call("pfsgnn_loss_finalize", None if sl is None else sl.ref, d.G, d.NF, d.NC,
              n_prime.data_ptr(), fiber_time.data_ptr(), tvar.data_ptr(), ci.data_ptr(),
              float(pclass), float(pfiber), float(total_time), float(nfields), float(wutils),
              float(wvar), loss.data_ptr(), utils.data_ptr(), variance.data_ptr(), Gn.data_ptr(),
              Gf.data_ptr(), Gv.data_ptr(), _stream())
        return loss, utils, variance, Gn, Gf, Gv

    def loss_bwd(self, d, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, sharpness, noiselevel, seed,
                 Gn, Gf, Gv, tmean, gscale, dWd1, dbd1, dWd2, dbd2, bn=None):
        """-> gxe; with ``bn`` = (mu1, inv1) of the final edge BatchNorm ->
        (gxe, its backward sums' per-block partials) (pfsgnn_loss_bwd's bn_* fields).
        On a sliced general batch gxe is [F, EP] in slot order (0 at padding)
        and ``bn`` is not available (Engine.loss_bnstat gives None)."""
        sl = self._loss_layout(d)
        if sl is not None and bn is not None:
            raise NotImplementedError("loss_bwd(bn=...) is not fused on a sliced general batch")
        gxe = self.empty(d.F, d.EP)
        gs = None
        if isinstance(gscale, torch.Tensor):
            gs = gscale.reshape(1).to(torch.float32).contiguous()
        elif gscale != 1.0:
            gs = torch.full((1,), float(gscale), dtype=torch.float32, device=self.device)
        ci = ci.contiguous()
        a = self._loss_args(d, sl, y, sc, sh, Wd1, bd1, Wd2, bd2, ci, scale, sharpness, noiselevel,
                            seed)
        a.Gn, a.Gf, a.Gv = Gn.data_ptr(), Gf.data_ptr(), Gv.data_ptr()
        a.tmean, a.gscale = tmean.data_ptr(), _ptr(gs)
        a.dWd1, a.dbd1, a.dWd2, a.dbd2 = (dWd1.data_ptr(), dbd1.data_ptr(), dWd2.data_ptr(),
                                          dbd2.data_ptr())
        a.gxe = gxe.data_ptr()
        part = None
        if bn is not None:
            mu1, inv1 = bn
            self._chk(mu1, inv1)
            part = self.empty(lib().pfsgnn_loss_bn_parts(d.G, d.NF, d.NC), 2 * d.F)
            a.bn_mu1, a.bn_inv1, a.bn_part = mu1.data_ptr(), inv1.data_ptr(), part.data_ptr()
        ws, wsb = self._wsargs(d)
        _call("pfsgnn_loss_bwd", ctypes.byref(a), ws, wsb, _stream())
        return gxe if bn is None else (gxe, part)

    # ------------------------------------------------------------ graph building
    def build_complete(self, G, NF, NC, order=0):
        """edge_index [2, G*NF*NC] int64 of G complete bipartite graphs on the
        device; order 0 fiber-major (train.py:94), 1 class-major (graph.py:41)."""
        ei = torch.empty(2, G * NF * NC, dtype=torch.int64, device=self.device)
        _call("pfsgnn_build_complete", int(G), int(NF), int(NC), int(order), ei.data_ptr(),
              _stream())
        return ei

    # ------------------------------------------------------------ general graphs
    def sparse_layout(self, edge_index, G, NF, NC):
        """CSR layout of a batch that is not complete bipartite (pfsgnn.sparse).
        Raises ValueError if an edge is out of range or crosses graphs."""
        E = int(edge_index.shape[1])
        ei = edge_index.to(device=self.device, dtype=torch.int64).contiguous()
        i32 = dict(dtype=torch.int32, device=self.device)
        src_p, tgt_p, user_of, cls_ord = (torch.empty(E, **i32) for _ in range(4))
        fib_ptr = torch.empty(G * NF + 1, **i32)
        cls_ptr = torch.empty(G * NC + 1, **i32)
        status = torch.empty(1, **i32)
        ws = torch.empty(lib().pfsgnn_sparse_layout_ws_bytes(E), dtype=torch.uint8,
                         device=self.device)
        _call("pfsgnn_sparse_layout", ei.data_ptr(), E, int(G), int(NF), int(NC), src_p.data_ptr(),
              tgt_p.data_ptr(), user_of.data_ptr(), fib_ptr.data_ptr(), cls_ord.data_ptr(),
              cls_ptr.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        if int(status.item()) != 0:
            raise ValueError("edge_index has an edge out of range or joining nodes of different "
                             f"graphs (G={G}, NF={NF}, NC={NC}; gnn.py:32-47 batching)")
        deg_t = (cls_ptr[1:] - cls_ptr[:-1]).to(torch.float32).reshape(1, -1).contiguous()
        return SparseGeo(E, src_p, tgt_p, user_of, fib_ptr, cls_ord, cls_ptr, deg_t)

    def sliced_max_nc(self, F):
        """Classes per graph the fused sliced kernels of the current edge path
        take at Fdim F (pfsgnn_sliced_max_nc: static + per-class LDS <= 160 KB);
        0 when that path has no sliced kernels (the bf16 edge-state paths)."""
        nc = ctypes.c_int(0)
        _call("pfsgnn_sliced_max_nc", int(F), ctypes.byref(nc))
        return nc.value

    def sliced_layout(self, sp, G, NF, NC):
        """Slices of 16 fibers over a sparse layout (pfsgnn_sliced_plan / _fill):
        the fused general-graph edge kernels' layout (pfsgnn_sliced.hip).  One
        host read (the position count EP) per edge_index."""
        i32 = dict(dtype=torch.int32, device=self.device)
        nsl = G * ((NF + 63) // 64) * 4
        fib, base, ln = torch.empty(nsl * 16, **i32), torch.empty(nsl, **i32), torch.empty(nsl, **i32)
        slot_of = torch.empty(G * NF, **i32)
        info = torch.empty(2, dtype=torch.int64, device=self.device)
        ws = torch.empty(lib().pfsgnn_sliced_plan_ws_bytes(int(G), int(NF)), dtype=torch.uint8,
                         device=self.device)
        _call("pfsgnn_sliced_plan", sp.fib_ptr.data_ptr(), int(G), int(NF), fib.data_ptr(),
              base.data_ptr(), ln.data_ptr(), slot_of.data_ptr(), info.data_ptr(), ws.data_ptr(),
              ws.numel(), _stream())
        EP, maxdeg = (int(v) for v in info.tolist())
        cls = torch.empty(EP, dtype=torch.uint8, device=self.device)
        pos_user = torch.empty(EP, **i32)
        pco = torch.empty(8 * max(maxdeg, 1), dtype=torch.float32, device=self.device)
        _call("pfsgnn_sliced_fill", sp.src_p.data_ptr(), sp.tgt_p.data_ptr(),
              sp.user_of.data_ptr(), sp.fib_ptr.data_ptr(), sp.E, int(NF), int(NC),
              slot_of.data_ptr(), base.data_ptr(), EP, maxdeg, cls.data_ptr(), pos_user.data_ptr(),
              pco.data_ptr(), _stream())
        return SlicedLayout(fib, base, ln, slot_of, cls, pos_user, pco, EP, sp.E, maxdeg)

    def gather_cols(self, X, idx, mode=0, out=None, Z=None):
        """out[c][e] (=, +=) X[c][idx[e]]; mode 2: X[c][idx[e]] * lrelu'(Z[c][e])."""
        C, N = X.shape
        E = idx.numel()
        if out is None:
            assert mode != 1
            out = self.empty(C, E)
        self._chk(X, Z, out)
        assert idx.dtype == torch.int32 and out.shape == (C, E)
        _call("pfsgnn_gather_cols", X.data_ptr(), C, N, idx.data_ptr(), E, _ptr(Z), int(mode),
              out.data_ptr(), _stream())
        return out

    def segment_sum(self, X, ord, ptr, nseg, act=False, out=None, add=False):
        C, E = X.shape
        if out is None:
            out, add = self.empty(C, nseg), False
        self._chk(X, out)
        assert ptr.numel() == nseg + 1
        _call("pfsgnn_segment_sum", X.data_ptr(), C, E, _ptr(ord), ptr.data_ptr(), int(nseg),
              int(act), out.data_ptr(), int(add), _stream())
        return out

    def segment_moments(self, M, ptr, nseg, hs_out):
        C, E = M.shape
        mom = self.empty(4, C, nseg)
        self._chk(M, hs_out)
        assert hs_out.shape == (4 * C, nseg)
        _call("pfsgnn_segment_moments", M.data_ptr(), C, E, ptr.data_ptr(), int(nseg),
              mom.data_ptr(), hs_out.data_ptr(), _stream())
        return mom

    def segment_moment_grad(self, M, seg, mean, coef):
        C, E = M.shape
        nseg = mean.shape[1]
        mean, coef = mean.contiguous(), coef.contiguous()
        self._chk(M, mean, coef)
        gm = self.empty(C, E)
        _call("pfsgnn_segment_moment_grad", M.data_ptr(), C, E, seg.data_ptr(), mean.data_ptr(),
              coef.data_ptr(), int(nseg), gm.data_ptr(), _stream())
        return gm

    def _rows_ws(self, C, N):
        nb = lib().pfsgnn_rows_ws_bytes(int(C), int(N))
        ws = self.workspace(getattr(self, "_dims", None))
        if ws.numel() < nb:
            return torch.empty(nb, dtype=torch.uint8, device=self.device)
        return ws

    def rows_stats(self, X):
        C, N = X.shape
        self._chk(X)
        mu, var = self.empty(C), self.empty(C)
        ws = self._rows_ws(C, N)
        _call("pfsgnn_rows_stats", X.data_ptr(), C, N, mu.data_ptr(), var.data_ptr(),
              ws.data_ptr(), ws.numel(), _stream())
        return mu, var

    def rows_bn_sums(self, g, y, mu, inv):
        C, N = y.shape
        self._chk(g, y, mu, inv)
        Sg, Sgx = self.empty(C), self.empty(C)
        ws = self._rows_ws(C, N)
        _call("pfsgnn_rows_bn_sums", g.data_ptr(), y.data_ptr(), C, N, mu.data_ptr(),
              inv.data_ptr(), Sg.data_ptr(), Sgx.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        return Sg, Sgx

    def rows_axpby(self, g, y, alpha, gam1, gam0, out=None):
        """out = alpha*g + gam1*y + gam0 per channel (out may be g or y)."""
        C, N = y.shape
        out = self.empty(C, N) if out is None else out
        self._chk(g, y, alpha, gam1, gam0, out)
        _call("pfsgnn_rows_axpby", g.data_ptr(), y.data_ptr(), C, N, alpha.data_ptr(),
              gam1.data_ptr(), gam0.data_ptr(), out.data_ptr(), _stream())
        return out

    # ------------------------------------------------------------ layout / optim
    def layout_analyze(self, edge_index, G, NF, NC):
        """-> (perm [E] int32, complete, caller order is fiber-major, caller order is canonical)."""
        E = edge_index.shape[1]
        ei = edge_index.to(device=self.device, dtype=torch.int64).contiguous()
        perm = torch.empty(E, dtype=torch.int32, device=self.device)
        status = torch.empty(3, dtype=torch.int32, device=self.device)
        ws = torch.empty(max(4 * E, 256), dtype=torch.uint8, device=self.device)
        _call("pfsgnn_layout_analyze", ei.data_ptr(), E, G, NF, NC, perm.data_ptr(),
              status.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        st = status.cpu().tolist()
        return perm, bool(st[0]), bool(st[1]), bool(st[2])

    def edges_to_canonical(self, x, lay):
        """Caller-order [E, F] -> canonical channel-major [F, E]; ``lay`` carries
        (G, NF, NC, mode, perm) (pfsgnn.gnn.Layout)."""
        E, F = x.shape
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if lay.mode == SLOTS:
            sl = lay.sp.sl
            out = self.empty(F, sl.EP)
            _call("pfsgnn_edges_to_slots", x.data_ptr(), E, sl.EP, F, sl.pos_user.data_ptr(),
                  out.data_ptr(), _stream())
            return out
        out = self.empty(F, E)
        _call("pfsgnn_edges_to_canonical", x.data_ptr(), lay.G, lay.NF, lay.NC, F, lay.mode,
              _ptr(lay.perm), out.data_ptr(), _stream())
        return out

    def edges_from_canonical(self, y, sc, sh, lay, rowmajor=True):
        F, E = y.shape
        if lay.mode == SLOTS:
            sl = lay.sp.sl
            E = sl.E
            out = self.empty(E, F) if rowmajor else self.empty(F, E)
            _call("pfsgnn_edges_from_slots", y.data_ptr(), _ptr(sc), _ptr(sh), E, sl.EP, F,
                  sl.pos_user.data_ptr(), int(rowmajor), out.data_ptr(), _stream())
            return out
        out = self.empty(E, F) if rowmajor else self.empty(F, E)
        _call("pfsgnn_edges_from_canonical", y.data_ptr(), _ptr(sc), _ptr(sh), lay.G, lay.NF,
              lay.NC, F, lay.mode, _ptr(lay.perm), int(rowmajor), out.data_ptr(), _stream())
        return out

    def adam(self, p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, live=None):
        """``step``: int, or a device float tensor holding the (already
        incremented) step count (capturable form).  ``live``: optional device
        uint8 mask; elements with 0 are skipped (parameters without a grad)."""
        self._chk(p, g, m, v)
        if live is not None:
            assert live.dtype == torch.uint8 and live.is_cuda and live.numel() == p.numel()
        if isinstance(step, torch.Tensor):
            if not step.is_cuda or step.dtype != torch.float32 or step.numel() != 1:
                raise ValueError("a tensor step must be one float32 on the device")
            sval, sptr = 0, step.data_ptr()
        else:
            sval, sptr = int(step), None
        _call("pfsgnn_adam", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
              sval, sptr, float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
              _ptr(live), _stream())
