"""CPU-only contract of the argument checks of the fused-pass entry points -- the seven lmg_stencil_smooth*, the three
lmg_stencil_cheby_tiled*, lmg_dia_smooth and lmg_dia_cheby: which arguments are refused, with which status, and which
rule answers first when two are broken.

Every call here is refused or has n == 0, so it returns before any HIP call: the pointers are made-up host addresses
that nothing reads (the hot-pattern tables, which the host does read once the checks have passed, are always NULL).
The one exception is the coefficient table of a Chebyshev step, which the host reads in front of the other checks: a
real array.  A call that the library would accept with n > 0 must never be added: it would launch."""
import ctypes

import pytest

from learnmultigrid_amd import _lib

OK, ARG, CAPACITY = 0, -1, -4
M5, M9, M1D, M7A = 0x0BA, 0x1FF, 0x038, 0x1BB       # M7A: a legal slot set that none of the passes is built for
REG_ROWS = 2**29 - 4096                             # first row count the register pass refuses
TILE_ROWS = 2**31 - 4096                            # ... and the tiled pass
# made-up, distinct, 16-byte aligned addresses
PID, VAL, MASK, X, B, OUT, R, EC, PPID, PVAL, PMASK, BC, RPID, RVAL, RMASK, DIA = (0x100000 * (k + 1) for k in range(16))
COEF = (ctypes.c_double * 6)(0.0, 0.8, 0.25, 0.7, 0.2, 0.6)      # (a_k, c_k), k = 0 .. 2: host memory the library reads

OPERATOR = ["n", "line_stride", "pid", "npat", "st_val", "st_mask", "union_mask", "hot_pattern", "h_hot_val"]
SOLVE = ["x_in", "b", "omega", "x_out"]
COARSE = ["n_coarse", "coarse_stride"]
PROL = ["e_coarse", "p_pid", "p_npat", "p_val", "p_mask", "h_hot_pairs", "h_hot_pval"]
REST = ["b_coarse", "r_pid", "r_npat", "r_val", "r_mask", "hot_r", "h_hot_rval"]
PLAIN_ARGS = OPERATOR + ["sweeps"] + SOLVE + ["r_out", "stream"]
PROL_ARGS = OPERATOR + ["sweeps"] + SOLVE + COARSE + PROL + ["stream"]
REST_ARGS = OPERATOR + ["sweeps"] + SOLVE + COARSE + REST + ["stream"]
CHEB = ["degree", "h_coef", "x_in", "b", "x_out"]               # in place of sweeps and omega
ENTRY = {
    "lmg_stencil_smooth": PLAIN_ARGS,
    "lmg_stencil_smooth_prolong": PROL_ARGS,
    "lmg_stencil_smooth_restrict": REST_ARGS,
    "lmg_stencil_smooth_tiled": PLAIN_ARGS,
    "lmg_stencil_smooth_tiled_prolong": PROL_ARGS,
    "lmg_stencil_smooth_tiled_restrict": REST_ARGS,
    "lmg_stencil_smooth_tiled_turnaround": OPERATOR + ["sweeps_post", "sweeps_pre"] + SOLVE + COARSE + PROL + REST + ["stream"],
    "lmg_stencil_cheby_tiled": OPERATOR + CHEB + ["r_out", "stream"],
    "lmg_stencil_cheby_tiled_prolong": OPERATOR + CHEB + COARSE + PROL + ["stream"],
    "lmg_stencil_cheby_tiled_restrict": OPERATOR + CHEB + COARSE + REST + ["stream"],
}
CHEBY = [e for e in ENTRY if "cheby" in e]
REGISTER = [e for e in ENTRY if "tiled" not in e]
TILED = [e for e in ENTRY if "tiled" in e]
WITH_PROL = [e for e in ENTRY if "p_pid" in ENTRY[e]]
WITH_REST = [e for e in ENTRY if "r_pid" in ENTRY[e]]
ROWS = {e: (TILE_ROWS if "tiled" in e else REG_ROWS) for e in ENTRY}


def shape(W, lines):
    """Fine grid of `lines` whole lines of W rows and the coarse grid the restriction demands under it."""
    Wc = (W + 1) // 2
    return {"n": W * lines, "line_stride": W, "n_coarse": ((lines + 1) // 2) * Wc, "coarse_stride": Wc}


def complete(**changes):
    """Arguments that break no rule except that nothing is built for their slot set: with no change, CAPACITY."""
    a = dict(pid=PID, npat=3, st_val=VAL, st_mask=MASK, union_mask=M7A, hot_pattern=-1, h_hot_val=None, sweeps=2,
             sweeps_post=2, sweeps_pre=2, x_in=X, b=B, omega=0.8, x_out=OUT, r_out=R, stream=None, e_coarse=EC, p_pid=PPID,
             p_npat=4, p_val=PVAL, p_mask=PMASK, h_hot_pairs=None, h_hot_pval=None, b_coarse=BC, r_pid=RPID, r_npat=4,
             r_val=RVAL, r_mask=RMASK, hot_r=-1, h_hot_rval=None, h_coef=COEF, dia=DIA)
    a.update(shape(9, 9))
    a.update(changes)
    a.setdefault("degree", a["sweeps"])      # a Chebyshev step reads the sweep count of a case as its degree
    return a


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def call(L, entry, **changes):
    a = complete(**changes)
    assert a["h_hot_val"] is None and a["h_hot_pairs"] is None and a["h_hot_rval"] is None
    assert a["n"] in (0, 1) or a["union_mask"] not in (M5, M9, M1D), "this could launch"
    return getattr(L, entry)(*[a[k] for k in ENTRY[entry]])


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_only_the_slot_set_is_in_the_way(L, entry):
    """The base of every other case: all rules kept, and CAPACITY for a slot set without a kernel."""
    assert call(L, entry) == CAPACITY
    assert call(L, entry, sweeps=1, sweeps_post=1, sweeps_pre=1) == CAPACITY
    assert call(L, entry, sweeps=3, sweeps_post=3, sweeps_pre=3) == CAPACITY
    assert call(L, entry, npat=1, p_npat=1, r_npat=1) == CAPACITY
    assert call(L, entry, npat=64, p_npat=64, r_npat=64) == CAPACITY
    assert call(L, entry, union_mask=0x1BA) == CAPACITY
    assert call(L, entry, **shape(3, 3)) == CAPACITY


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_operator_rules(L, entry):
    assert call(L, entry, n=-1) == ARG
    assert call(L, entry, npat=0) == ARG
    assert call(L, entry, npat=65) == ARG
    assert call(L, entry, union_mask=0x200) == ARG
    assert call(L, entry, union_mask=0x3FF) == ARG
    for name in ("pid", "st_val", "st_mask", "b", "x_out"):
        assert call(L, entry, **{name: None}) == ARG, name
    assert call(L, entry, x_in=OUT) == ARG
    assert call(L, entry, line_stride=2, coarse_stride=1) == ARG
    assert call(L, entry, line_stride=82, coarse_stride=41) == ARG       # longer than the vector


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_row_limit(L, entry):
    last = ROWS[entry] - 1
    assert last % 3 == 0
    assert call(L, entry, **shape(3, last // 3)) == CAPACITY
    assert call(L, entry, **shape(3, last // 3 + 1)) == ARG
    assert call(L, entry, n=ROWS[entry]) == ARG
    if entry in REGISTER:
        assert call(L, entry, n=TILE_ROWS - 1) == ARG


@pytest.mark.parametrize("entry", ["lmg_stencil_smooth", "lmg_stencil_smooth_tiled", "lmg_stencil_cheby_tiled"])
def test_plain_pass(L, entry):
    assert call(L, entry, r_out=None) == CAPACITY
    assert call(L, entry, x_in=None) == CAPACITY                # the zero iterate
    assert call(L, entry, x_in=None, r_out=None) == CAPACITY
    assert call(L, entry, r_out=OUT) == ARG
    assert call(L, entry, r_out=X) == ARG
    assert call(L, entry, x_in=None, r_out=OUT) == ARG
    assert call(L, entry, sweeps=0) == ARG
    assert call(L, entry, sweeps=4) == ARG
    assert call(L, entry, sweeps=-1) == ARG
    # nothing to do: before the pointers and the line stride are looked at, after the sizes and the sweep count
    nothing = dict(n=0, line_stride=0, pid=None, st_val=None, st_mask=None, x_in=None, b=None, x_out=None, r_out=None)
    assert call(L, entry, **nothing) == OK
    assert call(L, entry, union_mask=M9, **nothing) == OK
    assert call(L, entry, npat=0, **nothing) == ARG
    assert call(L, entry, sweeps=4, **nothing) == ARG
    assert call(L, entry, union_mask=0x200, **nothing) == ARG


def test_one_row(L):
    """A single row: CAPACITY from the register pass, before it looks at anything else but sizes and sweep count."""
    assert call(L, "lmg_stencil_smooth", n=1) == CAPACITY
    assert call(L, "lmg_stencil_smooth", n=1, union_mask=M9, pid=None, x_in=OUT) == CAPACITY
    assert call(L, "lmg_stencil_smooth", n=1, sweeps=4) == ARG
    assert call(L, "lmg_stencil_smooth", n=1, npat=0) == ARG
    assert call(L, "lmg_stencil_smooth_prolong", n=1, line_stride=1, pid=None) == CAPACITY
    assert call(L, "lmg_stencil_smooth_prolong", n=1, line_stride=1, p_pid=None) == ARG
    assert call(L, "lmg_stencil_smooth_restrict", n=1, line_stride=1, coarse_stride=1, n_coarse=1, pid=None) == CAPACITY
    assert call(L, "lmg_stencil_smooth_restrict", n=1, line_stride=1, coarse_stride=1, n_coarse=1, r_pid=None) == ARG
    # the tiled pass has no such answer: one row is shorter than any line stride it takes
    assert call(L, "lmg_stencil_smooth_tiled", n=1) == ARG
    assert call(L, "lmg_stencil_smooth_tiled", n=1, line_stride=1) == ARG
    assert call(L, "lmg_stencil_smooth_tiled_prolong", n=1, line_stride=1) == ARG
    assert call(L, "lmg_stencil_smooth_tiled_restrict", n=1, line_stride=1, coarse_stride=1, n_coarse=1) == ARG
    assert call(L, "lmg_stencil_cheby_tiled", n=1) == ARG
    assert call(L, "lmg_stencil_cheby_tiled", n=1, line_stride=1) == ARG
    assert call(L, "lmg_stencil_cheby_tiled_prolong", n=1, line_stride=1) == ARG
    assert call(L, "lmg_stencil_cheby_tiled_restrict", n=1, line_stride=1, coarse_stride=1, n_coarse=1) == ARG


@pytest.mark.parametrize("entry", sorted(set(WITH_PROL + WITH_REST)))
def test_transfer_passes_take_one_to_three_sweeps_each(L, entry):
    for s in (0, 4, -1, 6):
        if "turnaround" in entry:
            assert call(L, entry, sweeps_post=s) == ARG
            assert call(L, entry, sweeps_pre=s) == ARG
        else:
            assert call(L, entry, sweeps=s) == ARG


@pytest.mark.parametrize("entry", WITH_PROL)
def test_prolongation_rules(L, entry):
    for name in ("x_in", "e_coarse", "p_pid", "p_val", "p_mask"):
        assert call(L, entry, **{name: None}) == ARG, name
    assert call(L, entry, p_npat=0) == ARG
    assert call(L, entry, p_npat=65) == ARG
    assert call(L, entry, e_coarse=OUT) == ARG
    assert call(L, entry, n_coarse=0) == ARG
    assert call(L, entry, n_coarse=2**31) == ARG
    assert call(L, entry, coarse_stride=0) == ARG
    assert call(L, entry, coarse_stride=26) == ARG               # longer than the coarse vector
    # these come before "nothing to do"
    assert call(L, entry, n=0, p_pid=None) == ARG
    assert call(L, entry, n=0, n_coarse=0) == ARG


def test_prolongation_differences(L):
    reg, tiled = "lmg_stencil_smooth_prolong", "lmg_stencil_smooth_tiled_prolong"
    # a coarse vector of one row: the register pass takes it, the tiled one wants two
    one = dict(n=0, line_stride=1, n_coarse=1, coarse_stride=1)
    assert call(L, reg, **one) == OK
    assert call(L, tiled, **one) == ARG
    assert call(L, tiled, n=0, line_stride=1, n_coarse=2, coarse_stride=1) == OK
    assert call(L, tiled, n=0, line_stride=1, n_coarse=2, coarse_stride=2) == OK
    # coarse lines shorter than half a fine line: only the register pass refuses them
    assert call(L, reg, coarse_stride=4) == ARG
    assert call(L, reg, coarse_stride=5) == CAPACITY
    assert call(L, reg, coarse_stride=6) == CAPACITY
    assert call(L, tiled, coarse_stride=4) == CAPACITY
    assert call(L, reg, n=0, coarse_stride=4) == ARG
    assert call(L, tiled, n=0, coarse_stride=4) == OK
    # no coarse-grid shape rule here: any coarse length that holds a line
    assert call(L, reg, n_coarse=5) == CAPACITY
    assert call(L, tiled, n_coarse=1000) == CAPACITY
    assert call(L, reg, n_coarse=2**31 - 1) == CAPACITY
    assert call(L, tiled, n_coarse=2**31 - 1) == CAPACITY
    # the sweep count and the operator are looked at after the prolongation, "nothing to do" in between
    assert call(L, reg, n=0, sweeps=4) == ARG
    assert call(L, tiled, n=0, union_mask=0x200) == ARG
    assert call(L, reg, n=0, pid=None, b=None, x_out=None) == OK
    assert call(L, tiled, n=0, pid=None, b=None, x_out=None) == OK
    assert call(L, reg, n=0, x_in=None) == ARG


def test_cheby_prolongation_is_the_tiled_one(L):
    """What test_prolongation_differences pins for lmg_stencil_smooth_tiled_prolong holds for its Chebyshev twin."""
    tiled = "lmg_stencil_cheby_tiled_prolong"
    assert call(L, tiled, n=0, line_stride=1, n_coarse=1, coarse_stride=1) == ARG       # the two-row coarse minimum
    assert call(L, tiled, n=0, line_stride=1, n_coarse=2, coarse_stride=1) == OK
    assert call(L, tiled, n=0, line_stride=1, n_coarse=2, coarse_stride=2) == OK
    assert call(L, tiled, coarse_stride=4) == CAPACITY
    assert call(L, tiled, n=0, coarse_stride=4) == OK
    assert call(L, tiled, n_coarse=1000) == CAPACITY
    assert call(L, tiled, n_coarse=2**31 - 1) == CAPACITY
    assert call(L, tiled, n=0, sweeps=4) == ARG
    assert call(L, tiled, n=0, union_mask=0x200) == ARG
    assert call(L, tiled, n=0, pid=None, b=None, x_out=None) == OK
    assert call(L, tiled, n=0, x_in=None) == ARG


@pytest.mark.parametrize("entry", WITH_REST)
def test_restriction_rules(L, entry):
    for name in ("b_coarse", "r_pid", "r_val", "r_mask"):
        assert call(L, entry, **{name: None}) == ARG, name
    assert call(L, entry, r_npat=0) == ARG
    assert call(L, entry, r_npat=65) == ARG
    for other in (X, OUT, B):
        assert call(L, entry, b_coarse=other) == ARG
    assert call(L, entry, n_coarse=0) == ARG
    assert call(L, entry, coarse_stride=0) == ARG
    assert call(L, entry, n_coarse=2**28, coarse_stride=2**27) == ARG
    assert call(L, entry, n_coarse=2**31, coarse_stride=2**30) == ARG
    # the coarse grid is exactly the one under the fine grid: 5 lines of 5 under 9 lines of 9
    assert call(L, entry, coarse_stride=4, n_coarse=20) == ARG
    assert call(L, entry, coarse_stride=6, n_coarse=30) == ARG
    assert call(L, entry, n_coarse=20) == ARG
    assert call(L, entry, n_coarse=30) == ARG
    assert call(L, entry, n=80) == ARG                           # a last line that is not whole
    assert call(L, entry, **shape(10, 8)) == CAPACITY            # even sizes: 4 lines of 5
    assert call(L, entry, **dict(shape(10, 8), n_coarse=25)) == ARG
    # an empty fine grid has no coarse grid under it, and an empty coarse grid is refused
    assert call(L, entry, n=0) == ARG
    assert call(L, entry, n=0, n_coarse=0) == ARG
    assert call(L, entry, n=0, n_coarse=5) == ARG
    # the zero iterate: fine for the restricting pass, not for the turnaround, which corrects x_in
    assert call(L, entry, x_in=None) == (ARG if "turnaround" in entry else CAPACITY)


def test_turnaround_rules_of_its_own(L):
    entry = "lmg_stencil_smooth_tiled_turnaround"
    assert call(L, entry, b_coarse=EC) == ARG
    assert call(L, entry, b_coarse=EC, e_coarse=EC) == ARG
    assert call(L, entry, sweeps_post=3, sweeps_pre=1) == CAPACITY
    assert call(L, entry, sweeps_post=1, sweeps_pre=3) == CAPACITY
    assert call(L, entry, **shape(3, 3)) == CAPACITY             # a coarse grid of 2 lines of 2
    assert call(L, entry, **shape(3, 1)) == CAPACITY             # ... of one line of 2, the shortest it takes
    assert call(L, entry, n=1, line_stride=1, n_coarse=1, coarse_stride=1) == ARG
    # two faults: the checks in front of the operator's all answer ARG, also where the operator's would say CAPACITY or OK
    assert call(L, entry, b_coarse=EC, union_mask=M7A, pid=None) == ARG
    assert call(L, entry, n=0, sweeps_pre=4) == ARG
    assert call(L, entry, r_pid=None, p_pid=None) == ARG


def test_order_of_checks(L):
    for entry in sorted(ENTRY):
        # an operator fault and a slot set without a kernel: the fault
        assert call(L, entry, pid=None) == ARG
        assert call(L, entry, x_in=OUT, union_mask=0) == ARG
        assert call(L, entry, union_mask=0) == CAPACITY
    for entry in REGISTER:
        assert call(L, entry, n=REG_ROWS, npat=0, sweeps=9, pid=None) == ARG
    # the restriction's shape rule is in front of the row limit and of the single row
    assert call(L, "lmg_stencil_smooth_restrict", n=1, line_stride=3) == ARG
    assert call(L, "lmg_stencil_smooth_restrict", n=REG_ROWS, n_coarse=2**28) == ARG
    # a transfer fault and "nothing to do": the fault
    assert call(L, "lmg_stencil_smooth_tiled_prolong", n=0, e_coarse=OUT) == ARG
    assert call(L, "lmg_stencil_smooth_prolong", n=0, e_coarse=OUT) == ARG
    assert call(L, "lmg_stencil_smooth_prolong", n=1, line_stride=1, e_coarse=OUT) == ARG
    assert call(L, "lmg_stencil_cheby_tiled_prolong", n=0, e_coarse=OUT) == ARG


@pytest.mark.parametrize("entry", CHEBY)
def test_cheby_degree_and_coefficients(L, entry):
    """The degree (1 .. 3) and the coefficient table are looked at in front of everything else, "nothing to do" included."""
    for degree in (1, 2, 3):
        assert call(L, entry, degree=degree) == CAPACITY
    for degree in (0, 4, -1):
        assert call(L, entry, degree=degree) == ARG
    assert call(L, entry, h_coef=None) == ARG
    nothing = dict(n=0, line_stride=0, pid=None, st_val=None, st_mask=None, b=None, x_out=None, r_out=None)
    if "restrict" in entry:
        assert call(L, entry, **nothing) == ARG                 # an empty fine grid has no coarse grid under it
    else:
        assert call(L, entry, **nothing) == OK
    assert call(L, entry, h_coef=None, **nothing) == ARG
    assert call(L, entry, degree=4, **nothing) == ARG


# ---- the DIA passes: no pattern table, a row limit of their own, and no rule against stray bits of the slot set -------------
DIA_ENTRY = {
    "lmg_dia_smooth": ["n", "line_stride", "union_mask", "dia", "sweeps", "x_in", "b", "omega", "x_out", "r_out", "stream"],
    "lmg_dia_cheby": ["n", "line_stride", "union_mask", "dia", "degree", "h_coef", "x_in", "b", "x_out", "r_out", "stream"],
}
DIA_BUILT = (M5, M7A, 0x0FE, M9)                    # the slot sets lmg_dia_smooth_supported answers for


def dia_call(L, entry, **changes):
    """complete() with the 1-D slot set, which the DIA pass is not built for: with no change, CAPACITY."""
    a = complete(**dict(dict(union_mask=M1D), **changes))
    assert a["n"] == 0 or a["union_mask"] not in DIA_BUILT, "this could launch"
    return getattr(L, entry)(*[a[k] for k in DIA_ENTRY[entry]])


@pytest.mark.parametrize("entry", sorted(DIA_ENTRY))
def test_dia_pass(L, entry):
    assert not L.lmg_dia_smooth_supported(M1D) and all(L.lmg_dia_smooth_supported(m) for m in DIA_BUILT)
    assert dia_call(L, entry) == CAPACITY
    for s in (1, 3):
        assert dia_call(L, entry, sweeps=s) == CAPACITY
    for s in (0, 4):
        assert dia_call(L, entry, sweeps=s) == ARG
    assert dia_call(L, entry, r_out=None) == CAPACITY
    assert dia_call(L, entry, x_in=None) == CAPACITY             # the zero iterate
    assert dia_call(L, entry, union_mask=0x200) == CAPACITY      # stray bits: just a slot set without a kernel
    assert dia_call(L, entry, union_mask=0) == CAPACITY
    for name in ("dia", "b", "x_out"):
        assert dia_call(L, entry, **{name: None}) == ARG, name
    assert dia_call(L, entry, x_in=OUT) == ARG
    assert dia_call(L, entry, r_out=X) == ARG
    assert dia_call(L, entry, r_out=OUT) == ARG
    assert dia_call(L, entry, line_stride=2) == ARG
    assert dia_call(L, entry, line_stride=82) == ARG             # longer than the vector
    assert dia_call(L, entry, n=TILE_ROWS - 1, line_stride=3) == CAPACITY
    assert dia_call(L, entry, n=TILE_ROWS) == ARG
    assert dia_call(L, entry, n=-1) == ARG
    # nothing to do: after the sizes and the sweep count, before the pointers and the line stride
    nothing = dict(n=0, line_stride=0, dia=None, x_in=None, b=None, x_out=None, r_out=None)
    assert dia_call(L, entry, **nothing) == OK
    assert dia_call(L, entry, union_mask=M9, **nothing) == OK
    assert dia_call(L, entry, sweeps=4, **nothing) == ARG
    # a fault and a slot set without a kernel: the fault
    assert dia_call(L, entry, union_mask=0x200, dia=None) == ARG


def test_dia_cheby_coefficients(L):
    """In front of everything else, like the tiled Chebyshev passes."""
    entry = "lmg_dia_cheby"
    assert dia_call(L, entry, degree=-1) == ARG
    assert dia_call(L, entry, h_coef=None) == ARG
    assert dia_call(L, entry, h_coef=None, n=0, line_stride=0, dia=None, x_in=None, b=None, x_out=None, r_out=None) == ARG
