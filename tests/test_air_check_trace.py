"""AirBuilder.check_trace (the model sp_air_check_trace is tested against) on hand-derived cases, and what of sp_air_check_trace
needs no GPU: the struct mirror, the symbol probe and the refusals that are decided before the context is touched."""
import ctypes
import os
import re

import pytest

import check_trace_airs as X
import periodic_airs
from lambdaworks_cairo_prover_amd import _lib, air, api

P = air.P
V = air.Violation
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. satisfying traces ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.EXAMPLES))
@pytest.mark.parametrize("rap", [X.SMALL_RAP, X.BIG_RAP])
@pytest.mark.parametrize("n", [16, 64])
def test_satisfying_traces_give_no_violations(name, rap, n):
    b, rows = X.EXAMPLES[name](n)
    raps = [rap] * b.n_rap
    assert b.check_trace(X.full_rows(b, rows, raps), raps) == []


def test_satisfying_mimc_chain_gives_no_violations():
    keys = periodic_airs.keys(5, 8)
    b = air.mimc_chain(64, 8, 3, keys)
    assert b.check_trace(air.mimc_chain_trace(64, 3, keys)) == []


def test_aux_program_rows_may_come_with_or_without_the_aux_columns():
    b, rows = X.EXAMPLES["fibonacci_rap_program"](16)
    with_aux = [r + [z] for r, z in zip(rows, X.permutation_column(rows, X.BIG_RAP))]
    assert b.check_trace(with_aux, [X.BIG_RAP]) == b.check_trace(rows, [X.BIG_RAP]) == []
    spoiled = X.changed(with_aux, (7, 2, 1))                     # the aux column itself: z_7 is read on rows 6 and 7
    got = b.check_trace(spoiled, [X.BIG_RAP])
    assert [(v.kind, v.index, v.rows, v.first_row, v.last_row) for v in got] == [(0, 1, 2, 6, 7)]
    with pytest.raises(ValueError, match="RAP challenges"):
        b.check_trace(rows, [])


# ---- 2. hand-derived ------------------------------------------------------------------------------------------------------------
def test_fibonacci_2_columns_one_cell_by_hand():
    """c0(i) = a(i+1) - a(i) - b(i), c1(i) = b(i+1) - b(i) - a(i+1), both enforced on rows 0 .. 14.  a(5) += d: c0(4) = d, c0(5) = -d,
    c1(4) = -d, nothing else moves."""
    d = 5
    b = air.fibonacci_2_columns(1, 1)
    rows = X.changed(X.fibonacci_2_columns_rows(16), (5, 0, d))
    assert b.check_trace(rows) == [V(0, 0, 2, 4, 5, d), V(0, 1, 1, 4, 4, P - d)]


def test_boundary_cell_by_hand():
    a1 = 1
    b = air.fibonacci_2_columns(1, a1)
    assert b.bcs[1] == (1, 0, a1)
    rows = X.changed(X.fibonacci_2_columns_rows(16), (0, 1, 41))
    got = b.check_trace(rows)
    assert got[-1] == V(1, 1, 1, 0, 0, a1 + 41)
    assert [v.kind for v in got].count(1) == 1                   # boundary(0, 0, a0) still holds
    # cell (0, 1) = b(0) is read by c0(0) = a(1) - a(0) - b(0) and c1(0) = b(1) - b(0) - a(1)
    assert got[:-1] == [V(0, 0, 1, 0, 0, P - 41), V(0, 1, 1, 0, 0, P - 41)]


# ---- 3. exemptions ----------------------------------------------------------------------------------------------------------------
def test_exempted_rows_are_not_reported():
    """simple_fibonacci, n = 16, exemptions 2: c(i) = x(i+2) - x(i+1) - x(i) is enforced on rows 0 .. 13 and frame rows wrap.  On the
    satisfying trace c(14) = x(0) - x(15) - x(14) and c(15) = x(1) - x(0) - x(15) are non-zero and stay unreported.  x(15) is read by
    c(13), c(14) and c(15) - no cell of this AIR is read by exempted rows only - so a change of row 15 reports row 13 alone, whatever
    rows 14 and 15 evaluate to; a change of row 13 is read by c(11) = +d, c(12) = -d, c(13) = -d."""
    n, d = 16, 9
    b = air.simple_fibonacci(1, 1)
    rows = X.simple_fibonacci_rows(n)
    x = [r[0] for r in rows]
    assert (x[0] - x[15] - x[14]) % P != 0 and (x[1] - x[0] - x[15]) % P != 0
    assert b.check_trace(rows) == []
    assert b.check_trace(X.changed(rows, (15, 0, d))) == [V(0, 0, 1, 13, 13, d)]
    assert b.check_trace(X.changed(rows, (13, 0, d))) == [V(0, 0, 3, 11, 13, d)]
    assert b.enforced_exemptions() == [2]


def test_enforced_exemptions_follow_the_composition():
    assert air.dummy().enforced_exemptions() == [0, 2]
    assert air.fibonacci_rap(16, 12).enforced_exemptions() == [6, 1]            # num_transition_exemptions = 2: each its own
    b = air.AirBuilder(1, [0, 1], 1)                                              # num_transition_exemptions = 1: the first non-zero count
    for e in (0, 3, 1):
        b.constraint(b.load(1, 0) - b.load(0, 0), 1, e)
    assert b.enforced_exemptions() == [0, 3, 3]


def test_periodic_values_and_wrap_around():
    """mimc_chain: x(i+1) = (x(i) + K(i mod 8))^3, the last row exempt.  A change of row 21 is read by c(20) and c(21) only; the value on
    row 20 is the change itself."""
    keys = periodic_airs.keys(5, 8)
    b = air.mimc_chain(64, 8, 3, keys)
    rows = X.changed(air.mimc_chain_trace(64, 3, keys), (21, 0, 77))
    got = b.check_trace(rows)
    assert len(got) == 1 and got[0][:5] == (0, 0, 2, 20, 21) and got[0].value == 77


# ---- 4. the library ---------------------------------------------------------------------------------------------------------------
def test_struct_mirror_symbols_and_header(hip_lib):
    assert ctypes.sizeof(air.AirViolationC) == hip_lib.sp_air_violation_size() == 64
    air._check_violation_layout()
    for name in ("sp_air_check_trace", "sp_air_violation_size"):
        assert name in _lib.NEWEST_SYMBOLS and hasattr(hip_lib, name)
    header = open(os.path.join(ROOT, "include", "stark252_hip.h")).read()
    assert re.search(r"int sp_air_check_trace\(sp_ctx\* ctx, const sp_air_desc\* air, const sp_air_aux_desc\* aux", header)
    assert int(re.search(r"#define SP_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.SP_ABI_VERSION == hip_lib.sp_abi_version()


def _call(lib, ctx, desc, trace, n, opt, rap, periodic=None, out=None, cap=0, n_out=True):
    total = ctypes.c_uint32(0)
    return lib.sp_air_check_trace(ctx, ctypes.byref(desc), None, None if periodic is None else ctypes.byref(periodic),
                                  trace.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.c_uint64(n), None if opt is None else ctypes.byref(opt),
                                  rap, out, ctypes.c_uint32(cap), ctypes.byref(total) if n_out else None)


def test_refusals_that_need_no_device(hip_lib):
    """What sp_air_check_trace refuses before it touches its context (a block of zeroed memory stands in for one here, on a machine
    without a GPU too): neither options nor challenges, no place for the count, a capacity without records, and the malformed
    descriptors sp_air_prove_periodic refuses."""
    keys = periodic_airs.keys(1, 8)
    b = air.mimc_chain(16, 8, 3, keys)
    desc, keep = b.build()
    trace = air.ints_to_bytes(air.mimc_chain_trace(16, 3, keys))
    opt = api.ProofOptions.default_test_options().to_c()
    ctx = ctypes.create_string_buffer(1 << 16)
    E = _lib.SP_E_INVALID_ARG
    assert _call(hip_lib, ctx, desc, trace, 16, None, None, desc.periodic_desc) == E
    assert _call(hip_lib, None, desc, trace, 16, opt, None, desc.periodic_desc) == E
    assert _call(hip_lib, ctx, desc, trace, 16, opt, None, desc.periodic_desc, n_out=False) == E
    assert _call(hip_lib, ctx, desc, trace, 16, opt, None, desc.periodic_desc, out=None, cap=4) == E
    for columns in ([keys[:6]], [periodic_airs.keys(1, 32)], [[1]] * 65):               # no power of two, longer than the trace, 65 columns
        other, k2 = air.periodic_desc(columns)
        assert _call(hip_lib, ctx, desc, trace, 16, opt, None, other) == E, len(columns[0])
    other, k2 = air.periodic_desc([keys])
    other.cols[0].period = 1 << 31
    assert _call(hip_lib, ctx, desc, trace, 16, opt, None, other) == E
    other, k2 = air.periodic_desc([keys])
    other.cols[0].values = None
    assert _call(hip_lib, ctx, desc, trace, 16, opt, None, other) == E
    bad, k3 = b.build()
    bad.n_offsets = 9                                                                    # a malformed sp_air_desc
    assert _call(hip_lib, ctx, bad, trace, 16, opt, None, bad.periodic_desc) == E
    assert b"sp_air_check_trace" in hip_lib.sp_last_error()


def test_binding_needs_options_or_challenges():
    class NoContext(api.Context):
        def __init__(self):                      # the refusal comes before the library is called
            self._h = None
    desc, keep = air.fibonacci_2_columns().build()
    with pytest.raises(ValueError, match="options"):
        NoContext().air_check_trace(desc, air.ints_to_bytes(X.fibonacci_2_columns_rows(8)))
