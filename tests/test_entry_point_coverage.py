"""Host-only bookkeeping: every compute entry point of the C ABI is called by some device test.

``leopard_amd/ops.py`` is read with ``ast``: per ``Ops`` method, the ``self.lib.lmi_*`` names it calls, directly or through another
``Ops`` method.  An entry point of ``_lib.SIGNATURES`` counts as covered when a ``tests/test_gpu_*.py`` file, or a helper module under
``tests/`` that such a file imports, contains a call ``<anything>.<method>(...)`` of a method that reaches it.  That is a necessary
condition, not a proof of a good test: it keeps an entry point from shipping with no device test at all (the state lmi_add_rmsnorm,
lmi_rmsnorm_rows, lmi_decode_advance, lmi_split_hi_lo, lmi_preprocess_images and lmi_gemm_bias_act were in before
tests/test_gpu_row_kernels.py).  Nothing is imported from the test files and nothing is launched."""
import ast
import glob
import os

from leopard_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(REPO, "tests")

# Entry points that are not compute kernels, each with the reason it needs no kernel-level device test.
ALLOWED = {
    "lmi_abi_version": "a constant; read by build() and by test_abi_exports_every_declared_symbol",
    "lmi_debug_copy": "diagnostics only (tools/overlap_probe.py): a 16-byte grid-stride copy",
    # the communicator: its device tests start one process per rank and call it through leopard_amd/dist.py, not through Ops
    # (tests/test_gpu_dist.py)
    "lmi_comm_unique_id": "communicator (leopard_amd/dist.py, tests/test_gpu_dist.py)",
    "lmi_comm_init": "communicator (leopard_amd/dist.py, tests/test_gpu_dist.py)",
    "lmi_comm_destroy": "communicator (leopard_amd/dist.py, tests/test_gpu_dist.py)",
    "lmi_comm_size": "communicator (leopard_amd/dist.py, tests/test_gpu_dist.py)",
    "lmi_allgather": "communicator (leopard_amd/dist.py, tests/test_gpu_dist.py)",
    "lmi_allreduce": "communicator (leopard_amd/dist.py, tests/test_gpu_dist.py)",
    "lmi_reduce_scatter": "communicator (leopard_amd/dist.py, tests/test_gpu_dist.py)",
    "lmi_broadcast": "communicator (leopard_amd/dist.py, tests/test_gpu_dist.py)",
    # the forms without a row selection: one-line forwards to the _rows entries (row_sel = null), which are what Ops calls and what is tested
    "lmi_norm_lo4": "forwards to lmi_norm_lo4_rows",
    "lmi_attn_varlen_fwd_lo4": "forwards to lmi_attn_varlen_fwd_lo4_rows",
}

# Entry points whose device test drives them through a module of the package instead of calling the Ops method itself:
# entry point -> (the Ops method, the module that calls it, the name the device test imports from that module, the device test).
THROUGH_THE_PACKAGE = {
    "lmi_resample_u8": ("resample_u8", "gpu_tiler", "GpuTiler", "test_gpu_tiler.py"),       # bit for bit against PIL
}


def _parse(path):
    with open(path) as f:
        return ast.parse(f.read(), filename=path)


def ops_reach():
    """{Ops method: set of lmi_* names it reaches}, closed over calls of other Ops methods through ``self``."""
    tree = _parse(os.path.join(REPO, "leopard_amd", "ops.py"))
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Ops")
    methods = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    direct, calls = {}, {}
    for name, fn in methods.items():
        direct[name], calls[name] = set(), set()
        for node in ast.walk(fn):
            if not isinstance(node, ast.Attribute):
                continue
            v = node.value
            if node.attr.startswith("lmi_") and isinstance(v, ast.Attribute) and v.attr == "lib" and isinstance(v.value, ast.Name) and v.value.id == "self":
                direct[name].add(node.attr)                              # self.lib.lmi_x
            elif node.attr in methods and isinstance(v, ast.Name) and v.id == "self":
                calls[name].add(node.attr)                               # self.other_method (called, or picked as ``fn = self.a if .. else self.b``)
    reach = {k: set(v) for k, v in direct.items()}
    changed = True
    while changed:
        changed = False
        for name in methods:
            for callee in calls[name]:
                if not reach[callee] <= reach[name]:
                    reach[name] |= reach[callee]
                    changed = True
    for names in reach.values():
        names.discard("lmi_last_error")                                  # the error text behind every _check: not a launch
    return reach


def gpu_test_sources():
    """tests/test_gpu_*.py and, transitively, the helper modules under tests/ they import.  Another test file is not a helper: a device test
    that borrows a config builder from tests/test_emu_*.py does not run that file's emulator tests on the device."""
    todo = sorted(glob.glob(os.path.join(TESTS, "test_gpu_*.py")))
    seen = {}
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        tree = seen[path] = _parse(path)
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.ImportFrom) and node.module:
                names = [node.module] + [node.module + "." + a.name for a in node.names]
            elif isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            for mod in names:
                if mod.startswith("tests.") and not mod.split(".")[-1].startswith("test_"):
                    cand = os.path.join(REPO, *mod.split(".")) + ".py"
                    if os.path.exists(cand):
                        todo.append(cand)
    return seen


def called_method_names(trees, methods):
    out = set()
    for tree in trees:
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in methods:
                out.add(node.func.attr)
    return out


def test_the_reader_sees_what_ops_calls():
    """The ast walk itself: direct calls, calls through another method, and a method chosen by an expression."""
    reach = ops_reach()
    assert reach["rmsnorm_rows"] == {"lmi_rmsnorm_rows"} and reach["split_hi_lo"] == {"lmi_split_hi_lo"}
    assert reach["add_norm"] == {"lmi_add_rmsnorm", "lmi_add_rmsnorm_lo4"}
    assert reach["norm"] == {"lmi_norm_lo4_rows", "lmi_rmsnorm", "lmi_layernorm"}
    assert reach["attend_prefix"] == reach["attention_prefix"] | reach["attention_prefix_lo4"] and len(reach["attend_prefix"]) == 2
    every = set().union(*reach.values())
    assert every <= set(_lib.SIGNATURES) | {"lmi_last_error", "lmi_attn_decode_workspace_bytes", "lmi_llm_prefill_workspace_bytes",
                                            "lmi_vit_workspace_bytes"}, every - set(_lib.SIGNATURES)


def test_every_compute_entry_point_is_called_by_a_device_test():
    reach = ops_reach()
    sources = gpu_test_sources()
    assert any(p.endswith("test_gpu_row_kernels.py") for p in sources) and any(p.endswith("row_kernels_ref.py") for p in sources)
    called = called_method_names(sources.values(), set(reach))
    covered = set().union(*(reach[m] for m in called)) if called else set()
    for entry, (method, module, name, test_file) in THROUGH_THE_PACKAGE.items():
        assert entry in reach[method]
        assert method in called_method_names([_parse(os.path.join(REPO, "leopard_amd", module + ".py"))], {method}), (module, method)
        test_tree = next(t for p, t in sources.items() if os.path.basename(p) == test_file)
        assert any(isinstance(n, ast.ImportFrom) and n.module == "leopard_amd." + module and name in [a.name for a in n.names]
                   for n in ast.walk(test_tree)), (test_file, module, name)
        assert any(isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == name for n in ast.walk(test_tree)), (test_file, name)
        covered.add(entry)
    assert set(ALLOWED) <= set(_lib.SIGNATURES), set(ALLOWED) - set(_lib.SIGNATURES)
    assert not (set(ALLOWED) & covered), "allow-listed, yet a device test reaches it: drop it from ALLOWED: " + ", ".join(sorted(set(ALLOWED) & covered))
    missing = sorted(k for k in _lib.SIGNATURES if k.startswith("lmi_") and k not in covered and k not in ALLOWED)
    assert not missing, ("no tests/test_gpu_*.py (or helper it imports) calls an Ops method that reaches: " + ", ".join(missing))
