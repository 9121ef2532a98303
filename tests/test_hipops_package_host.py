"""The hipops package keeps what the single hipops.py module gave its callers: every name on ``hipops``, shared state that is
one object, switches that are defined once (``hipops.REBINDABLE``) and read live through the package, and public functions
that call each other through the package (so that replacing one on ``hipops`` intercepts the calls made from inside it).
No GPU needed: nothing is launched; where a predicate would ask the library, a stub answers."""
import ast
import glob
import inspect
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "egocentric-gaze-prediction_amd", "hipops")
# top-level functions, classes and assigned names (annotated assignments included: _PERSIST_SYNC) of the single-module hipops.py
# this package replaced, from an ast walk over that file
SURFACE = open(os.path.join(ROOT, "tests", "golden", "hipops_surface.txt")).read().split()

# name -> the family module that creates it
SHARED = {"_WS": "_core", "PROF": "_core", "LIB": "_core",
          "_PACKED": "packing", "_USED": "packing", "_BATCH_TABLES": "packing", "_BATCH_PINNED": "packing",
          "_WEIGHT_EPOCH": "packing", "_UID": "packing",
          "PENDING_PRODUCER": "sinks", "ABSMAX_STATS": "absmax",
          "ALGO_CHANNELS": "conv", "PRESPLIT_STATS": "conv", "MASK_FUSE_STATS": "conv", "BNSUMS_STATS": "conv",
          "BN_DEFER_STATS": "bn", "EVAL_FOLD_STATS": "bn", "_PERSIST_SYNC": "lstm",
          "_GAUSS_W": "metrics", "_AREA_T": "dataprep", "_NORM_CONST": "dataprep",
          "_LINEAR_T": "vis", "_JET": "vis", "_JET_WARNED": "vis", "_FLOW_TAPS": "flow", "_FLOW_WS": "flow"}


def H():
    from egaze_amd import hipops
    return hipops


def family(name):
    import importlib
    return importlib.import_module("egaze_amd.hipops." + name)


def family_trees():
    out = {}
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        name = os.path.basename(path)[:-3]
        if name != "__init__":
            out[name] = ast.parse(open(path).read(), path)
    assert len(out) >= 14
    return out


def top_level_names(tree):
    names = []
    for stmt in tree.body:
        if isinstance(stmt, (ast.FunctionDef, ast.ClassDef)):
            names.append(stmt.name)
        elif isinstance(stmt, (ast.Assign, ast.AnnAssign, ast.AugAssign)):
            for t in (stmt.targets if isinstance(stmt, ast.Assign) else [stmt.target]):
                names += [n.id for n in ast.walk(t) if isinstance(n, ast.Name)]
    return names


class StubLib:
    """Stands in for a family module's LIB: every entry point answers ``answer`` and is noted."""

    def __init__(self, answer):
        self.answer, self.calls = answer, []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append(name)
            return self.answer
        return call


# ----------------------------------------------------------------------------- surface
def test_every_name_of_the_single_module_resolves_on_the_package():
    h = H()
    assert len(SURFACE) == len(set(SURFACE)) >= 221
    assert sum(n.startswith("_") for n in SURFACE) >= 52
    missing = [n for n in SURFACE if not hasattr(h, n)]
    assert missing == []
    assert h.check is __import__("egaze_amd")._lib.check
    from egaze_amd.hipops import area_table          # the third import spelling the callers use
    assert area_table is h.area_table
    import egaze_amd.hipops as h2
    assert h2 is h


# ----------------------------------------------------------------------------- identity
@pytest.mark.parametrize("name", sorted(SHARED))
def test_shared_state_is_one_object_created_in_one_module(name):
    h = H()
    assert getattr(h, name) is getattr(family(SHARED[name]), name)
    creators = [m for m, tree in family_trees().items() if name in top_level_names(tree)]
    assert creators == [SHARED[name]]


def test_every_stats_dict_and_every_family_lib_is_covered():
    h = H()
    stats = [n for n in SURFACE if n.endswith("_STATS") and isinstance(getattr(h, n), dict)]
    assert len(stats) >= 6 and all(n in SHARED for n in stats)
    for m in family_trees():
        lib = getattr(family(m), "LIB", None)
        assert lib is None or lib is h.LIB, m          # stream_perturb patches launchers on the one proxy instance


# ----------------------------------------------------------------------------- structure
def test_init_holds_switches_and_reexports_only():
    h = H()
    tree = ast.parse(open(os.path.join(PKG, "__init__.py")).read())
    assert not [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef, ast.Lambda))]
    assigned = top_level_names(tree)
    assert isinstance(h.REBINDABLE, tuple) and len(set(h.REBINDABLE)) == len(h.REBINDABLE)
    for name in h.REBINDABLE:
        assert assigned.count(name) == 1, name
    assert sorted(assigned) == sorted(h.REBINDABLE + ("REBINDABLE",))       # ... and nothing else is defined there


def test_family_modules_read_switches_and_call_public_functions_through_the_package():
    h = H()
    public = {n for n in SURFACE if not n.startswith("_") and inspect.isfunction(getattr(h, n))} - {"check"}
    assert len(public) > 100
    bad = []
    for m, tree in family_trees().items():
        for node in ast.walk(tree):
            if isinstance(node, ast.Name) and node.id in h.REBINDABLE:
                bad.append(f"{m}:{node.lineno}: bare switch {node.id}")
            if isinstance(node, ast.Global):
                bad.append(f"{m}:{node.lineno}: global {node.names}")
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in public:
                bad.append(f"{m}:{node.lineno}: bare call of the public {node.func.id}")
            if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module in family_trees():
                for al in node.names:
                    if al.name in h.REBINDABLE or al.name in public:
                        bad.append(f"{m}:{node.lineno}: imports {al.name} from .{node.module}")
        # the package object is only partly initialised while a family module is imported: no _H.NAME read at import time

        def import_time(node):
            if isinstance(node, (ast.FunctionDef, ast.Lambda)):
                kids = list(getattr(node, "decorator_list", [])) + node.args.defaults + [d for d in node.args.kw_defaults if d]
            else:
                kids = list(ast.iter_child_nodes(node))
            for k in kids:
                if isinstance(k, ast.Attribute) and isinstance(k.value, ast.Name) and k.value.id == "_H":
                    bad.append(f"{m}:{k.lineno}: _H.{k.attr} at import time")
                import_time(k)
        import_time(tree)
    assert bad == []


# ----------------------------------------------------------------------------- liveness
def test_arithmetic_switches_are_read_live(monkeypatch):
    h = H()
    monkeypatch.setattr(h, "PRECISION", "split")
    monkeypatch.setattr(h, "GRAD_SPLIT", "f16")
    monkeypatch.setattr(h, "BWD_PRODUCTS", 3)
    assert h.conv_dtype("fwd", 64, 64) == h.F16X3
    assert h.conv_dtype("dgrad", 64, 64) == h.F16X3
    assert h._p2(h.F16X3) == h.F16X3
    assert h._want_absmax() and h._want_fwd_absmax()
    with monkeypatch.context() as m:
        m.setattr(h, "PRECISION", "f32")
        assert h.conv_dtype("fwd", 64, 64) == h.F32
        assert not h._want_absmax() and not h._want_fwd_absmax()
    with monkeypatch.context() as m:
        m.setattr(h, "GRAD_SPLIT", "bf16")
        assert h.conv_dtype("dgrad", 64, 64) == h.BF16X3
        assert h.conv_dtype("fwd", 64, 64) == h.F16X3
    operand = torch.zeros(8, 64)                      # 512 floats = 2048 bytes, on the CPU: nothing looks at its data
    assert h.conv_dtype("fwd", 64, 64, operand) == h.F16X3
    with monkeypatch.context() as m:
        m.setattr(h, "_SPLIT_MAX_BYTES", 1024)
        assert h.conv_dtype("fwd", 64, 64, operand) == h.F32
    with monkeypatch.context() as m:
        m.setattr(h, "BWD_PRODUCTS", 2)
        assert h._p2(h.F16X3) == h.F16X3 | h.P2_DTYPE
    with monkeypatch.context() as m:
        m.setattr(h, "FWD_SCALE", False)
        assert h._want_fwd_absmax() is False
    assert h._want_fwd_absmax() is True


@pytest.mark.parametrize("switch, module, predicate, args", [
    ("PRESPLIT", "conv", "presplit_ok", (4, 56, 56, 64, 64)),
    ("PRESPLIT_GRAD", "conv", "presplit_grad_ok", (4, 56, 56, 64, 64)),
    ("PRESPLIT", "conv", "presplit_grad_ok", (4, 56, 56, 64, 64)),
    ("FWD_SCALE", "conv", "presplit_ok", (4, 56, 56, 64, 64)),
    ("BNSUMS_FUSE", "conv", "bnsums_ok", (4, 224, 224, 32, 32, 1)),
    ("BNSUMS_FUSE", "bn", "bn_defer_ok", (4, 224, 224, 32, 32, True)),
    ("BN_DEFER", "bn", "bn_defer_ok", (4, 224, 224, 32, 32, True)),
])
def test_route_predicates_read_their_switch_live(switch, module, predicate, args, monkeypatch):
    """On: the predicate goes on to ask the library (a stub that says yes) and returns True.  Off: False, before any library call."""
    h = H()
    for name, v in (("PRECISION", "split"), ("GRAD_SPLIT", "f16"), ("FWD_SCALE", True), ("PRESPLIT", True), ("PRESPLIT_GRAD", True),
                    ("BNSUMS_FUSE", True), ("BN_DEFER", True)):
        monkeypatch.setattr(h, name, v)
    lib = StubLib(1)
    monkeypatch.setattr(family(module), "LIB", lib)
    assert getattr(h, predicate)(*args) is True
    assert lib.calls
    del lib.calls[:]
    monkeypatch.setattr(h, switch, False)
    assert getattr(h, predicate)(*args) is False
    assert lib.calls == []


def test_wide_bnsums_and_splitk_are_read_live(monkeypatch):
    h = H()
    monkeypatch.setattr(h, "BNSUMS_FUSE", True)
    monkeypatch.setattr(h, "BNSUMS_WIDE", True)
    monkeypatch.setattr(h, "SPLITK", False)
    lib = StubLib(2)                                 # streamed_ok: yes; streamed_splits: 2
    monkeypatch.setattr(family("conv"), "LIB", lib)
    assert h.bnsums_ok(4, 56, 56, 64, 64, 1) is True
    assert "egz_conv3x3_streamed_splits" not in lib.calls
    monkeypatch.setattr(h, "SPLITK", True)           # a split-K launch keeps the reduce pass
    assert h.bnsums_ok(4, 56, 56, 64, 64, 1) is False
    assert "egz_conv3x3_streamed_splits" in lib.calls
    monkeypatch.setattr(h, "SPLITK", False)
    monkeypatch.setattr(h, "BNSUMS_WIDE", False)
    assert h.bnsums_ok(4, 56, 56, 64, 64, 1) is False


def test_lstm_persist_switch_is_read_and_written_live(monkeypatch):
    h = H()
    monkeypatch.setattr(h, "LSTM_PERSIST", True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: types.SimpleNamespace(multi_processor_count=256))
    assert h.lstm_persist_ok(2, 4, 512) is True
    with h.lstm_persistent(False) as ctx:
        assert h.LSTM_PERSIST is False and ctx.prev is True
        assert h.lstm_persist_ok(2, 4, 512) is False
        with h.lstm_persistent(True):
            assert h.LSTM_PERSIST is True
        assert h.LSTM_PERSIST is False
    assert h.LSTM_PERSIST is True
    monkeypatch.setattr(torch.cuda, "get_device_properties", None)       # off: False before any device query
    monkeypatch.setattr(h, "LSTM_PERSIST", False)
    assert h.lstm_persist_ok(2, 4, 512) is False
    # a lost hand-off switches the persistent form off on the package, where every reader looks
    monkeypatch.setattr(h, "LSTM_PERSIST", True)
    monkeypatch.setattr(h, "lstm_persist_errors", lambda: {"fwd": 3, "bwd": 0})
    with pytest.raises(RuntimeError, match="lost an in-launch hand-off"):
        h.lstm_persist_check(reset=False)
    assert h.LSTM_PERSIST is False


def test_direct_grads_switch_is_read_live(monkeypatch):
    h = H()
    owner = types.SimpleNamespace(zero_gen=0)
    p = torch.nn.Parameter(torch.zeros(4))
    p._egz_sink = h.GradSink(torch.zeros(4), owner)
    monkeypatch.setattr(h, "DIRECT_GRADS", False)
    assert h.grad_sink(p) is None
    assert p._egz_sink.gen_written == -1             # ... and the sink was not taken
    monkeypatch.setattr(h, "DIRECT_GRADS", True)
    assert h.grad_sink(p) is p._egz_sink.buf
    assert h.grad_sink(p) is None                    # taken for this zero_grad generation


def test_batch_repack_switch_is_read_live(monkeypatch):
    h = H()
    dead = (-1, "fwd_frag", 1)                       # a used packing whose cache entry is gone
    p = torch.nn.Parameter(torch.zeros(1))
    p._egz_uid = -1
    assert dead not in h._USED and dead not in h._PACKED
    h._USED.add(dead)
    try:
        monkeypatch.setattr(h, "BATCH_REPACK", False)
        before = set(h._USED)
        assert h.refresh_packings([]) == 0 and h.refresh_packings([p]) == 0
        assert h._USED == before                     # off: returns before it looks at _USED
        monkeypatch.setattr(h, "BATCH_REPACK", True)
        assert h.refresh_packings([p]) == 0
        assert dead not in h._USED                   # on: the dead entry was dropped
    finally:
        h._USED.discard(dead)


def test_replacing_a_public_function_on_the_package_intercepts_inner_calls(monkeypatch):
    """record() / Recorder / stream_perturb wrap functions by monkeypatch.setattr(hipops, name, wrapped) and rely on it."""
    h = H()
    seen = []
    monkeypatch.setattr(h, "gemm", lambda *a, **kw: seen.append((a[2:5], kw)) or "out")
    assert h.linear_fwd(torch.zeros(3, 5), torch.zeros(7, 5)) == "out"
    assert h.matmul_nn(torch.zeros(3, 7), torch.zeros(7, 5)) == "out"
    assert [s[0] for s in seen] == [(3, 7, 5), (3, 5, 7)]
    monkeypatch.setattr(h, "area_table", lambda s, d: seen.append("area") or h.linear_table(s, d))
    key = (0, (8, 8), (4, 4))
    try:                                             # (the cache entry of this made-up table is dropped again)
        h._area_tables("cpu", (8, 8), (4, 4))
        assert seen[-2:] == ["area", "area"]
    finally:
        h._AREA_T.pop(key, None)
