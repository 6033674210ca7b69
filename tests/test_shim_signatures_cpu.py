"""The CPU stand-ins of tests/cpu_ops_shim.py against the functions they stand for: every public function the module or one
of its namespaces offers exists in learnmultigrid_amd.ops and takes a prefix of its parameters -- the same names in the same
order with the same defaults -- and every parameter the stand-in leaves out has a default in ops.  A keyword call the package
makes therefore binds on both or on neither, and a trailing option nobody passes to a stand-in (build_gs_schedule's `reverse`)
raises a TypeError there instead of being ignored."""
import inspect

import pytest

import cpu_ops_shim as shim
from learnmultigrid_amd import ops

NAMESPACES = {
    "module": lambda: shim,
    "namespace": shim.namespace,
    "recording_line": shim.recording_line,
    "fused_jacobi": lambda: shim.fused("jacobi"),
    "fused_jacobi_no_turnaround": lambda: shim.fused("jacobi", turnaround=False),
    "fused_cheby": lambda: shim.fused("cheby", max_rows=300),
    "fused_all": lambda: shim.fused("all", max_rows=289),
    "fused_all_none": lambda: shim.fused("all", max_rows=0),
}


def offered(ns, kind):
    return {k: v for k, v in vars(ns).items() if kind(v) and not k.startswith("_") and k not in shim.FACTORIES}


def prefix_mismatch(stand_in, real):
    """None, or what is wrong with the stand-in's parameter list."""
    have, want = (list(inspect.signature(f).parameters.values()) for f in (stand_in, real))
    for i, p in enumerate(have):
        if i >= len(want):
            return "parameter %d (%s) is not in ops" % (i, p.name)
        q = want[i]
        if (p.name, p.kind, p.default) != (q.name, q.kind, q.default):
            return "parameter %d is %s, ops has %s" % (i, p, q)
    missing = [q.name for q in want[len(have):] if q.default is inspect.Parameter.empty]
    return "ops requires %s as well" % ", ".join(missing) if missing else None


@pytest.mark.parametrize("name", sorted(NAMESPACES))
def test_stand_ins_take_a_prefix_of_the_real_parameters(name):
    ns = NAMESPACES[name]()
    functions = offered(ns, inspect.isfunction)
    # (the walk does see the stand-ins: those of the module are in every namespace)
    assert {"csr_jacobi", "multi_axpy", "line_solve"} <= set(offered(shim, inspect.isfunction)) <= set(functions)
    wrong = {}
    for k, fn in sorted(functions.items()):
        real = getattr(ops, k, None)
        if not inspect.isfunction(real):
            wrong[k] = "no such function in ops"
        elif prefix_mismatch(fn, real):
            wrong[k] = prefix_mismatch(fn, real)
    assert not wrong, wrong
    classes = offered(ns, inspect.isclass)
    assert "SpGEMMPlan" in classes
    assert not [k for k, c in classes.items() if not inspect.isclass(getattr(ops, k, None))]


def test_the_plain_module_offers_no_more_than_it_should():
    """What the package reads as "not offered" stays absent from the module, and the factories stay out of its copies."""
    absent = ("gs_prepare", "FUSED_MAX_SWEEPS", "CapturedGraph", "gemm", "coarse_front", "coarse_back")
    for ns in (shim, shim.namespace()):
        assert not [k for k in vars(ns) if k.startswith("stencil_") or k in absent]
    assert set(shim.FACTORIES) <= set(vars(shim)) and not set(shim.FACTORIES) & set(vars(shim.namespace()))
    a, b = shim.namespace(), shim.namespace(SpGEMMPlan=None)
    assert a.calls == [] and a.calls is not b.calls and b.SpGEMMPlan is None and a.SpGEMMPlan is shim.SpGEMMPlan


def test_every_offered_name_has_a_parity_entry():
    """Every function or class a stand-in namespace offers is registered in tests/stand_in_parity.py -- with cases for
    test_stand_in_parity_gpu.py, the GPU test that already compares it with its kernel, or the reason why there is nothing to
    compare --, and the registry names nothing that no namespace offers.  A covering test is looked up in the file's syntax
    tree: GPU test modules are not imported here."""
    import ast
    import os

    import stand_in_parity as SP
    names = SP.all_offered()
    assert {"csr_jacobi", "stencil_smooth", "block_cg_step", "block_scale", "line_solve_banded", "SpGEMMPlan"} <= set(names)
    assert len(SP.NAMESPACES) == 10 and all(names.values())
    missing = sorted(set(names) - set(SP.REGISTRY))
    assert not missing, "offered by a stand-in namespace without an entry in stand_in_parity.REGISTRY: %s" % missing
    stale = sorted(set(SP.REGISTRY) - set(names))
    assert not stale, "registered, but offered by no namespace: %s" % stale
    here = os.path.dirname(os.path.abspath(__file__))
    for op, entry in SP.REGISTRY.items():
        if isinstance(entry, SP.Cases):
            assert entry.cases and len({c.label for c in entry.cases}) == len(entry.cases), op
            assert SP.implementations(op, entry.only), op
        elif isinstance(entry, SP.CoveredBy):
            path, test = entry.test_id.split("::")
            tree = ast.parse(open(os.path.join(here, path)).read())
            found = [f for f in tree.body if isinstance(f, ast.FunctionDef) and f.name == test]
            assert found and "shim" in ast.unparse(found[0]), (op, entry.test_id)
        else:
            assert isinstance(entry, SP.NoValues) and entry.reason.strip(), op


def test_constants_equal_the_library():
    """What a stand-in hard-codes is what the library says (no device is needed for any of these)."""
    import block_cg_ref
    assert shim._MAX_VECTORS == ops.krylov_max_vectors()
    assert block_cg_ref.WIDTHS == ops.BLOCK_WIDTHS
    for passes in ("jacobi", "cheby", "all"):
        assert shim.fused(passes).FUSED_MAX_SWEEPS == ops.FUSED_MAX_SWEEPS, passes


def test_the_check_tells_a_drifted_stand_in():
    def real(A, x, sweeps=1, reverse=False):
        pass
    assert prefix_mismatch(lambda A, x, sweeps=1: None, real) is None
    assert prefix_mismatch(lambda A, x: None, real) is None
    assert prefix_mismatch(lambda A, y: None, real)               # another name
    assert prefix_mismatch(lambda x, A: None, real)               # another order
    assert prefix_mismatch(lambda A, x, sweeps=2: None, real)     # another default
    assert prefix_mismatch(lambda A, x, sweeps=1, reverse=False, more=0: None, real)
    assert prefix_mismatch(lambda A: None, real)                  # leaves out a parameter without a default
    assert prefix_mismatch(lambda *a, **k: None, real)
