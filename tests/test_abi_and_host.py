"""CPU tests: the C ABI library loads and exports every symbol include/pfsgnn.h
declares (no compute calls -- there is no GPU here), the host-side layout /
batching / parameter logic, and the fail-loudly behaviour without a GPU."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pfs-neural-net_amd")


def header_functions():
    txt = open(os.path.join(ROOT, "include", "pfsgnn.h")).read()
    return sorted(set(re.findall(r"\b(pfsgnn_\w+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(PKG, "pfsgnn", "libpfsgnn.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-C", PKG, "-j8"], check=True, capture_output=True)
    from pfsgnn import native
    return native.lib()


def test_library_exports_every_header_symbol(lib):
    from pfsgnn import native
    funcs = header_functions()
    assert len(funcs) >= 30
    for f in funcs:
        assert hasattr(lib, f), f"libpfsgnn.so does not export {f}"
        assert f in native._SIGS, f"native.py binds no signature for {f}"
    assert lib.pfsgnn_version().decode().startswith("pfsgnn")


def test_library_is_gfx950_code_object(lib):
    so = os.path.join(PKG, "pfsgnn", "libpfsgnn.so")
    blob = open(so, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob or b"gfx950" in blob


def test_block_tail_struct_layout_matches(lib):
    """native.BlockTail mirrors pfsgnn_block_tail field for field: same size, and
    the last field where C puts it (every pointer is 8-byte aligned)."""
    import ctypes
    from pfsgnn import native
    assert lib.pfsgnn_block_tail_bytes() == ctypes.sizeof(native.BlockTail)
    assert native.BlockTail.Qt.offset == ctypes.sizeof(native.BlockTail) - 8
    assert lib.pfsgnn_class_bwd_bytes() == ctypes.sizeof(native.ClassBwd)
    assert native.ClassBwd.g_hsum.offset == ctypes.sizeof(native.ClassBwd) - 8


def test_edge_args_struct_layouts_match(lib):
    """The six edge-op argument structs of native.py mirror include/pfsgnn.h:
    same size as C reports, the last field where C puts it (it is a pointer, or
    an int before the struct's tail padding: 8 bytes from the end either way),
    and the head (G, NF, NC, F, sl) in front."""
    import ctypes
    from pfsgnn import native
    last = {"edge_mlp_fwd": "inv2", "source_fwd": "msg", "target_fwd": "tmask",
            "target_bwd": "fold", "source_bwd": "dWt1", "edge_mlp_bwd": "Vu"}
    assert list(native.EDGE_ARGS) == list(last)
    for op, (name, cls) in enumerate(native.EDGE_ARGS.items()):
        assert lib.pfsgnn_edge_args_bytes(op) == ctypes.sizeof(cls), name
        assert cls._fields_[-1][0] == last[name]
        assert getattr(cls, last[name]).offset == ctypes.sizeof(cls) - 8, name
        assert [f for f, _ in cls._fields_[:5]] == ["G", "NF", "NC", "F", "sl"]
        assert cls.sl.offset == 16
    assert lib.pfsgnn_edge_args_bytes(6) == 0
    assert lib.pfsgnn_edge_args_bytes(-1) == 0


# the edge ops' entry points before each op had one (argument structs)
REMOVED_EDGE_ENTRY_POINTS = [
    "pfsgnn_edge_mlp_fwd_bn", "pfsgnn_sl_edge_mlp_fwd", "pfsgnn_sl_edge_mlp_fwd_bn",
    "pfsgnn_source_fwd_msg", "pfsgnn_sl_source_fwd", "pfsgnn_sl_target_fwd",
    "pfsgnn_target_bwd_bn", "pfsgnn_target_bwd_fold", "pfsgnn_sl_target_bwd",
    "pfsgnn_source_bwd_bn", "pfsgnn_source_bwd_msg", "pfsgnn_source_bwd_bn_msg",
    "pfsgnn_source_bwd_fold", "pfsgnn_sl_source_bwd", "pfsgnn_sl_source_bwd_bn",
    "pfsgnn_sl_edge_mlp_bwd"]


def test_removed_edge_entry_points_are_gone(lib):
    """Of the 22 former entry points of the six edge ops, the six base names
    remain (with the struct signature) and the 16 variants are neither exported,
    bound, nor named in the header."""
    from pfsgnn import native
    header = open(os.path.join(ROOT, "include", "pfsgnn.h")).read()
    assert lib.pfsgnn_version().decode() == native.ABI_VERSION == "pfsgnn 0.3 gfx950"
    for name in REMOVED_EDGE_ENTRY_POINTS:
        assert not hasattr(lib, name), f"libpfsgnn.so still exports {name}"
        assert name not in native._SIGS
        assert not re.search(r"\b%s\b" % name, header), f"pfsgnn.h still names {name}"
    for op in native.EDGE_ARGS:
        assert hasattr(lib, "pfsgnn_" + op) and len(native._SIGS["pfsgnn_" + op][0]) == 4


# the loss ops' entry points before each op had one (pfsgnn_loss_args)
REMOVED_LOSS_ENTRY_POINTS = [
    "pfsgnn_loss_bwd_bn", "pfsgnn_sl_loss_fwd", "pfsgnn_sl_loss_finalize", "pfsgnn_sl_loss_bwd",
    "pfsgnn_loss_fwd_ex", "pfsgnn_loss_bwd_ex"]


def test_removed_loss_entry_points_are_gone(lib):
    """The loss forward and backward have one entry point each, with the struct
    signature; finalize has one, led by the sliced layout; the six other names
    are neither exported, bound (native.exported_symbols, _SIGS), nor named in
    the header."""
    import ctypes
    from pfsgnn import native
    header = open(os.path.join(ROOT, "include", "pfsgnn.h")).read()
    for name in REMOVED_LOSS_ENTRY_POINTS:
        assert not hasattr(lib, name), f"libpfsgnn.so still exports {name}"
        assert name not in native._SIGS and name not in native.exported_symbols()
        assert not re.search(r"\b%s\b" % name, header), f"pfsgnn.h still names {name}"
    assert not [n for n in native._SIGS if n.startswith("pfsgnn_sl_loss")]
    for op in ("pfsgnn_loss_fwd", "pfsgnn_loss_bwd"):
        assert hasattr(lib, op)
        assert native._SIGS[op][0] == [ctypes.POINTER(native.LossArgs), native.P, native.SZ, native.P]
    assert native._SIGS["pfsgnn_loss_finalize"][0][0] is native.SLP
    assert len(native._SIGS["pfsgnn_loss_finalize"][0]) == 21


def _stand_in_library_is_refused(tmp_path, source):
    """native.lib() on a stand-in library built from ``source`` -> its refusal text."""
    import shutil
    import sys
    cc = shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "standin.c"
    src.write_text(source)
    so = tmp_path / "libpfsgnn_standin.so"
    subprocess.run([cc, "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from pfsgnn import native\n"
            "try:\n    native.lib()\n"
            "except native.NativeUnavailable as e:\n    print('REFUSED', e)\n" % PKG)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PFSGNN_LIB_PATH=str(so)),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "REFUSED" in r.stdout, r.stdout
    return r.stdout


def test_library_of_another_abi_version_is_refused(tmp_path):
    """A library left over from another tree (PFSGNN_LIB_PATH, a variant build)
    can export the edge ops' names with the old signatures; the binding refuses
    it by its version string instead of calling into it.  "pfsgnn 0.2" is the
    library whose pfsgnn_loss_fwd / pfsgnn_loss_bwd took positional arguments:
    the same names as today's with other signatures."""
    for old in ("pfsgnn 0.1 gfx950", "pfsgnn 0.2 gfx950"):
        out = _stand_in_library_is_refused(
            tmp_path, 'const char* pfsgnn_version(void) { return "%s"; }\n' % old)
        assert old in out and "pfsgnn 0.3 gfx950" in out and "rebuild" in out


def test_library_with_another_edge_struct_layout_is_refused(tmp_path):
    """A library of the right version whose pfsgnn_edge_args_bytes disagrees with
    one of this binding's six edge argument structs is refused when it loads,
    as for LossArgs and TrainRecordArgs."""
    import ctypes
    from pfsgnn import native
    sizes = [ctypes.sizeof(c) for c in native.EDGE_ARGS.values()]
    sizes[3] += 8                                             # target_bwd: one field more
    special = {
        "pfsgnn_version": 'const char* pfsgnn_version(void) { return "%s"; }' % native.ABI_VERSION,
        "pfsgnn_loss_args_bytes": "unsigned long pfsgnn_loss_args_bytes(void) { return %d; }"
                                  % ctypes.sizeof(native.LossArgs),
        "pfsgnn_train_record_args_bytes":
            "unsigned long pfsgnn_train_record_args_bytes(void) { return %d; }"
            % ctypes.sizeof(native.TrainRecordArgs),
        "pfsgnn_edge_args_bytes":
            "unsigned long pfsgnn_edge_args_bytes(int op) { static const unsigned long s[6] = {%s}; "
            "return op >= 0 && op < 6 ? s[op] : 0; }" % ", ".join(map(str, sizes)),
    }
    source = "\n".join(special.get(n, "int %s(void) { return 0; }" % n) for n in native._SIGS)
    out = _stand_in_library_is_refused(tmp_path, source + "\n")
    assert "pfsgnn_edge_args_bytes(3) = %d" % sizes[3] in out
    assert "TargetBwdArgs has %d bytes" % (sizes[3] - 8) in out and "rebuild" in out


def test_edge_ops_refuse_bad_arguments_before_any_launch(lib):
    """Every argument check of an edge op runs before its first launch, so it
    can be seen without a GPU: pointers are fake non-null addresses that are
    never dereferenced.  Each refusal returns non-zero with an error text that
    names the entry point (and the combination refused), and leaves no failure
    state behind for the next call."""
    import ctypes
    from pfsgnn import native
    FAKE = 0x1000
    sliced = native.Sliced(fib=FAKE, base=FAKE, len=FAKE, cls=FAKE, pco=FAKE, EP=32, E=20,
                           maxdeg=2)

    def args(op, sl=False, **over):
        """Valid dimensions, every pointer field set, scalars of a valid call."""
        a = native.EDGE_ARGS[op](G=1, NF=16, NC=2, F=10,
                                 sl=ctypes.pointer(sliced) if sl else None)
        for f, ty in a._fields_[5:]:
            if ty is ctypes.c_void_p:
                setattr(a, f, FAKE)
        if op == "source_bwd":
            a.n = 32
        # the optional parts that have no sliced form are off unless asked for
        for f in {"source_fwd": ["msg"], "target_bwd": ["bn_part"],
                  "source_bwd": ["msg", "dWt1"]}.get(op, []):
            setattr(a, f, None)
        for f, v in over.items():
            setattr(a, f, v)
        return a

    def refused(op, a, *words):
        fn = getattr(lib, "pfsgnn_" + op)
        rc = fn(ctypes.byref(a) if a is not None else None, None, 0, None)
        err = lib.pfsgnn_last_error().decode()
        assert rc != 0, (op, words)
        assert err.startswith("pfsgnn_" + op + ":"), err
        for w in words:
            assert w in err, (err, w)

    for op in native.EDGE_ARGS:
        refused(op, None, "null")                              # a NULL `a`
    refused("edge_mlp_fwd", args("edge_mlp_fwd", y=None), "null")   # a required pointer NULL
    refused("source_fwd", args("source_fwd", Qt=None), "null")
    refused("target_fwd", args("target_fwd", hsum=None), "null")
    refused("target_bwd", args("target_bwd", GzT=None), "null")
    refused("source_bwd", args("source_bwd", coef=None), "null")
    refused("edge_mlp_bwd", args("edge_mlp_bwd", GzEt=None), "null")
    refused("source_fwd", args("source_fwd", sl=True, msg=FAKE), "sl", "msg")
    refused("source_bwd", args("source_bwd", sl=True, msg=FAKE), "sl", "msg")
    refused("target_bwd", args("target_bwd", sl=True, bn_part=FAKE), "sl", "bn_part")
    refused("target_bwd", args("target_bwd", sl=True, fold=1), "sl", "fold")
    refused("source_bwd", args("source_bwd", sl=True, dWt1=FAKE), "sl", "dWt1")
    refused("source_bwd", args("source_bwd", dWt1=FAKE, tmask=None), "dWt1", "tmask")
    refused("source_bwd", args("source_bwd", alpha=None), "gamma", "alpha")
    refused("edge_mlp_fwd", args("edge_mlp_fwd", sc=None), "gamma", "sc")
    refused("target_fwd", args("target_fwd", agg=None), "Wt2", "agg")
    # no failure state is left behind: a valid host-only call succeeds
    info = (ctypes.c_int * 4)()
    assert lib.pfsgnn_edge_grid(1, 16, 2, info) == 0


def test_workspace_query_is_host_only(lib):
    b = lib.pfsgnn_workspace_bytes(16, 2394, 128, 10)
    assert 1 << 20 < b < 1 << 31


def test_no_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import pfsgnn
    with pytest.raises(pfsgnn.NativeUnavailable):
        pfsgnn.HipBackend()


def test_batch_collation_follows_inc(monkeypatch):
    import pfsgnn
    from pfsgnn import config
    monkeypatch.setattr(config, "device", torch.device("cpu"))
    gs = []
    for NF, NC in [(3, 2), (3, 2)]:
        e = torch.arange(NF * NC)
        ei = torch.stack([e // NC, e % NC])
        gs.append(pfsgnn.BipartiteData(ei, torch.zeros(NF, 1), torch.zeros(NC, 2), torch.zeros(NF * NC, 4),
                                       torch.zeros(1, 4)))
    b = pfsgnn.Batch.from_data_list(gs)
    assert b.edge_index[:, 6].tolist() == [3, 2]      # shifted by (x_s rows, x_t rows)
    assert b.num_graphs == 2 and b.x_s.shape == (6, 1) and b.x_t.shape == (4, 2)
    from harness import canonical_edges
    assert torch.equal(b.edge_index, canonical_edges(2, 3, 2))


def test_engine_param_order_is_reference_order():
    from pfsgnn.engine import param_names
    from oracle.ref_gnn import GNN
    for B in (1, 3):
        for normed in (True, False):
            m = GNN(B=B, Fdim=10, T=12, F_s=1, F_t=2, normed=normed)
            assert [n for n, _ in m.named_parameters()] == param_names(B, normed)


def test_noise_reference_is_uniform():
    from noise_ref import uniform_numpy
    u = uniform_numpy(7, 200000)
    assert u.min() >= 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) < 0.005 and abs(u.var() - 1 / 12) < 0.002
    assert (uniform_numpy(7, 10) == u[:10]).all() and (uniform_numpy(8, 10) != u[:10]).any()


def test_edge_grid_query_is_host_only(lib):
    from pfsgnn import native
    g = native.edge_grid(16, 2394, 128)
    # tail-aware split count: KS=5 fills the last dispatch round at the bench shape
    assert g == dict(KS=5, CPS=26, nblocks=3040, NFG=38)
    assert native.edge_grid(256, 2394, 16)["KS"] == 1


def test_tensor_cache_keys_on_object_not_address():
    """A freed tensor's cache entry must never serve a new tensor, even one the
    allocator places at the same address; in-place writes invalidate."""
    import gc
    from pfsgnn.gnn import _TensorCache
    c = _TensorCache(4)
    a = torch.zeros(1000)
    c.put(a, ("k",), "A")
    assert c.get(a, ("k",)) == "A"
    assert c.get(a, ("other",)) is None
    a.add_(1)                                    # bumps _version
    assert c.get(a, ("k",)) is None
    c.put(a, ("k",), "A2")
    ptr = a.data_ptr()
    del a
    gc.collect()
    for _ in range(50):                          # try to land on the same block
        b = torch.zeros(1000)
        if b.data_ptr() == ptr:
            break
    assert c.get(b, ("k",)) is None
    for i in range(10):                          # capacity: dead entries purged first
        t = torch.zeros(3)
        c.put(t, (), i)
    assert len(c.d) <= 4


def test_oversize_reduction_fails_loudly(lib):
    """a reduction wider than the packed 40-byte descriptor (rows >
    65535, cols > 32767) is refused with a non-zero return and an error text,
    before anything is launched (host-only: the pointers are never touched),
    instead of being skipped with success reported."""
    import ctypes
    from pfsgnn import native
    for rows, cols in ((70000, 4), (4, 40000)):
        r = native.Red(part=0x1000, nb=3, plen=rows * cols, ldp=cols, rows=rows, cols=cols,
                       out=0x2000, ldo=cols, add=0, scale=1.0)
        rc = lib.pfsgnn_reduce_batch(ctypes.byref(r), 1, None)
        assert rc != 0
        assert "packed descriptor" in lib.pfsgnn_last_error().decode()
