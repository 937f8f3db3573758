"""sp_air_check_trace on the device: the report equals AirBuilder.check_trace field for field, with the same RAP challenges given to
both - at the sizes where the wave-level reduction can go wrong, over the breadth of what sp_air_prove takes, and in agreement with
what the prover and the verifier make of the same traces."""
import pytest

import aux_program_airs
import check_trace_airs as X
import many_column_air as M
import oracle_lib as O
import periodic_airs
import wide_air
from lambdaworks_cairo_prover_amd import _lib, air, api

pytestmark = pytest.mark.gpu

P = air.P
OPT = api.ProofOptions.default_test_options()


def report(ctx, b, rows, rap=(), options=None, given=True, cap=4160):
    """(device report, model report) of the main rows `rows` under the challenges `rap`."""
    desc, keep = b.build()
    main = [list(r[:b.main_cols]) for r in rows]
    got = ctx.air_check_trace(desc, air.ints_to_bytes(main), options, list(rap) if given else None, cap)
    return got, b.check_trace(X.full_rows(b, main, list(rap)), list(rap))


def same(ctx, b, rows, rap=(), **kw):
    got, want = report(ctx, b, rows, rap, **kw)
    assert got == want
    return got


# ---- 5. shapes at which the reduction can go wrong -------------------------------------------------------------------------------
FIB2 = X.fibonacci_2_columns_rows
SHAPES = [
    ("one partial wave", 8, [(3, 0, 1)]),
    ("one full wave", 64, [(40, 1, 2)]),
    ("wave edge", 128, [(63, 0, 1), (64, 1, 1)]),
    ("block edge, last enforced rows", 512, [(255, 0, 1), (256, 0, 3), (510, 1, 1)]),
    ("far from lane 0", 1024, [(1000, 0, 7)]),
]


@pytest.mark.parametrize("what,n,cells", SHAPES, ids=[s[0] for s in SHAPES])
def test_reduction_shapes(hip_ctx, what, n, cells):
    b = air.fibonacci_2_columns(1, 1)
    got = same(hip_ctx, b, X.changed(FIB2(n), *cells))
    assert got and all(v.kind == 0 for v in got)
    assert same(hip_ctx, b, FIB2(n)) == [] and hip_ctx.last_check_total == 0


def test_every_row_wrong(hip_ctx):
    n = 1024
    rows = [[3 * i + 1, 5 * i + 2] for i in range(n)]             # a' - a - b = 1 - 5 i - 2 and b' - b - a' = 5 - 3 i - 4: never zero
    b = air.fibonacci_2_columns(1, 2)
    got = same(hip_ctx, b, rows)
    assert [(v.kind, v.index, v.rows, v.first_row, v.last_row) for v in got] == [(0, 0, n - 1, 0, n - 2), (0, 1, n - 1, 0, n - 2)]
    # every row of dummy's bit column wrong (no exemption: rows == n), its Fibonacci column right
    rows = [[2 + i, x] for i, x in enumerate(X.fib(n))]
    got = same(hip_ctx, air.dummy(), rows)
    assert got == [air.Violation(0, 0, n, 0, n - 1, 2)]


def test_dummy_exemptions_on_the_device(hip_ctx):
    """dummy: constraint 1 (three frame rows, exemptions 2) around the last enforced row, constraint 0 (no exemption) on the last row."""
    n = 128
    rows = X.dummy_rows(n)
    assert same(hip_ctx, air.dummy(), X.changed(rows, (n - 1, 1, 4))) == [air.Violation(0, 1, 1, n - 3, n - 3, 4)]
    got = same(hip_ctx, air.dummy(), X.changed(rows, (n - 1, 0, 2), (64, 1, 1)))
    assert [(v.index, v.rows, v.first_row, v.last_row) for v in got] == [(0, 1, n - 1, n - 1), (1, 3, 62, 64)]


# ---- 6. breadth -------------------------------------------------------------------------------------------------------------------
def test_wide_air_three_columns(hip_ctx):
    n, rap = 16, [X.BIG_RAP, 12345]
    rows = wide_air.main_trace(n)
    b = wide_air.build(n, rows)
    assert same(hip_ctx, b, rows, rap) == []
    bad = X.changed(rows, (5, 0, 1), (9, 1, 2), (0, 2, 3))
    got = same(hip_ctx, wide_air.build(n, bad), bad, rap)
    assert len(got) > 10


def test_many_columns_three_columns(hip_ctx):
    n, m = 256, 96
    b = M.build(n, m, boundary_row_count=4)
    rows = air.trace_to_ints(M.main_trace(n, m)).tolist()
    assert same(hip_ctx, b, rows) == []
    got = same(hip_ctx, b, X.changed(rows, (7, 3, 1), (130, 50, 1), (255, 95, 1)))
    assert len(got) >= 3


def test_64_constraints_first_middle_last(hip_ctx):
    n = 128
    b = X.counters(64)
    rows = X.counters_rows(n)
    assert same(hip_ctx, b, rows) == []
    got = same(hip_ctx, b, X.changed(rows, (5, 0, 1), (70, 31, 1), (127, 63, 1)))
    assert [(v.index, v.rows, v.first_row, v.last_row) for v in got] == [(0, 2, 4, 5), (31, 2, 69, 70), (63, 1, 126, 126)]


def test_periodic_column(hip_ctx):
    keys = periodic_airs.keys(5, 8)
    b = air.mimc_chain(64, 8, 3, keys)
    rows = air.mimc_chain_trace(64, 3, keys)
    assert same(hip_ctx, b, rows) == []
    got = same(hip_ctx, b, X.changed(rows, (21, 0, 77)))
    assert [(v.rows, v.first_row, v.last_row, v.value) for v in got] == [(2, 20, 21, 77)]
    wrong_key = air.mimc_chain(64, 8, 3, keys[:5] + [keys[5] + 1] + keys[6:])       # the statement changed, not the trace: rows 5, 13, ...
    got = same(hip_ctx, wrong_key, rows)
    assert (got[0].rows, got[0].first_row, got[0].last_row) == (8, 5, 61)


def sampled_rap(ctx, desc, trace, options):
    """The challenge a proof samples after round 1's main commitment: the first root of the proof into the reference's transcript."""
    proof = ctx.air_prove(desc, trace, options)
    assert int.from_bytes(proof[8:16], "big") == 2
    t = O.Transcript()
    t.append(proof[16:48])
    return t.to_field()


def test_aux_program_with_given_and_with_sampled_challenges(hip_ctx, oracle):
    n = 64
    b, rows = X.EXAMPLES["fibonacci_rap_program"](n)
    for rap in (X.SMALL_RAP, X.BIG_RAP):
        assert same(hip_ctx, b, rows, [rap]) == []
    bad = X.changed(rows, (20, 0, 1))                  # (z follows the trace and the wrap-around row is exempt: only constraint 0 can break)
    got = same(hip_ctx, b, bad, [X.BIG_RAP])
    assert [(v.index, v.rows, v.first_row, v.last_row) for v in got] == [(0, 3, 18, 20)]
    desc, keep = b.build()
    gamma = sampled_rap(hip_ctx, desc, air.ints_to_bytes(bad), OPT)
    got, want = report(hip_ctx, b, bad, [gamma], options=OPT, given=False)
    assert got == want and len(got) == 1
    # the permutation argument enforced on the wrap-around row: one main cell, and the constraint on the aux column breaks there
    c = X.closed_permutation(n)
    rows = X.closed_permutation_rows(n)
    assert same(hip_ctx, c, rows, [X.BIG_RAP]) == []
    bad = X.changed(rows, (9, 1, 1))
    got = same(hip_ctx, c, bad, [X.BIG_RAP])
    assert [(v.kind, v.index, v.rows, v.first_row, v.last_row) for v in got] == [(0, 0, 1, n - 1, n - 1)]
    desc, keep = c.build()
    gamma = sampled_rap(hip_ctx, desc, air.ints_to_bytes(bad), OPT)
    got, want = report(hip_ctx, c, bad, [gamma], options=OPT, given=False)
    assert got == want and [(v.index, v.first_row) for v in got] == [(0, n - 1)]


def test_host_built_aux_columns(hip_ctx):
    n, steps = 32, 28
    rows = X.fibonacci_rap_rows(n, steps)
    b = air.fibonacci_rap(n, steps)                              # aux_kind 1: the library's own permutation column
    assert same(hip_ctx, b, rows, [X.BIG_RAP]) == []
    assert len(same(hip_ctx, b, X.changed(rows, (10, 0, 1)), [X.SMALL_RAP])) == 1
    ok = X.fibonacci_rap_callback(n, steps, rows)                # aux_kind 2
    assert same(hip_ctx, ok, rows, [X.BIG_RAP]) == []
    spoiled = X.fibonacci_rap_callback(n, steps, rows, spoil=(12, 1))
    got = same(hip_ctx, spoiled, rows, [X.BIG_RAP])
    assert [(v.index, v.rows, v.first_row, v.last_row) for v in got] == [(1, 2, 11, 12)]
    first = X.fibonacci_rap_callback(n, steps, rows, spoil=(0, 5))
    got = same(hip_ctx, first, rows, [X.BIG_RAP])
    assert got[-1] == air.Violation(1, 2, 1, 0, 0, 6)            # boundary(2, 0, 1) finds 1 + 5


def test_40_boundary_constraints_three_wrong(hip_ctx):
    n, m = 64, 16
    b = M.build(n, m, boundary_row_count=8, boundary_total=40)
    assert len(b.bcs) == 40 and len({s for _, s, _ in b.bcs}) == 8
    rows = air.trace_to_ints(M.main_trace(n, m)).tolist()
    assert same(hip_ctx, b, rows) == []
    for j in (0, 17, 39):
        col, step, value = b.bcs[j]
        b.bcs[j] = (col, step, (value + 1 + j) % P)
    got = same(hip_ctx, b, rows)
    assert [(v.kind, v.index, v.rows, v.first_row, v.last_row, v.value) for v in got] == [(1, j, 1, b.bcs[j][1], b.bcs[j][1], M.cell(b.bcs[j][1], b.bcs[j][0])) for j in (0, 17, 39)]


def test_cap_smaller_than_the_report(hip_ctx):
    n = 128
    b = X.counters(64)
    rows = X.changed(X.counters_rows(n), *[(9, k, 1) for k in range(0, 64, 2)], (0, 0, 1))
    full = same(hip_ctx, b, rows)
    assert len(full) == 33 and hip_ctx.last_check_total == 33
    for cap in (0, 1, 5):
        got, want = report(hip_ctx, b, rows, cap=cap)
        assert got == want[:cap] and hip_ctx.last_check_total == 33


def test_refusals_on_the_device(hip_ctx):
    keys = periodic_airs.keys(1, 8)
    b = air.mimc_chain(16, 8, 3, keys)
    trace = air.ints_to_bytes(air.mimc_chain_trace(16, 3, keys))

    def code(desc, **kw):
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_check_trace(desc, trace, OPT, **kw)
        return e.value.code

    desc, k = b.build()
    desc.ops[1].b = 1                                            # PERIODIC(0, 0) -> a column that is not there
    assert code(desc) == _lib.SP_E_INVALID_ARG
    desc, k = b.build()
    del desc.periodic_desc                                       # op 6 without periodic columns
    assert code(desc) == _lib.SP_E_INVALID_ARG
    # a zero denominator in the aux program stays SP_E_ZERO_INVERSE: gamma = -b(3)
    r, rows = X.EXAMPLES["fibonacci_rap_program"](16)
    desc, k = r.build()
    with pytest.raises(api.SpError) as e:
        hip_ctx.air_check_trace(desc, air.ints_to_bytes(rows), None, [P - rows[3][1]])
    assert e.value.code == _lib.SP_E_ZERO_INVERSE
    with pytest.raises(ValueError):
        hip_ctx.air_check_trace(desc, air.ints_to_bytes(rows))
    good, k = b.build()
    assert hip_ctx.air_check_trace(good, trace, OPT) == []       # and the context still checks


# ---- 7. agreement with the prover ------------------------------------------------------------------------------------------------
def test_agreement_with_prover_and_verifier(hip_ctx, oracle):
    options = (4, 3, 3, 1)
    opt = api.ProofOptions(*options)
    clean2 = O.example_trace("fibonacci_2_columns", 64)
    cleand = O.example_trace("dummy", 16)
    broken2 = clean2.copy()
    broken2[33, 0, 31] ^= 1
    keys = periodic_airs.keys(5, 8)
    mimc_rows = X.changed(air.mimc_chain_trace(64, 3, keys), (21, 0, 1))
    cases = [("fibonacci_2_columns", air.fibonacci_2_columns(1, 1), clean2, True), ("dummy", air.dummy(), cleand, True),
             ("fibonacci_2_columns", air.fibonacci_2_columns(1, 1), broken2, False), (None, air.mimc_chain(64, 8, 3, keys), air.ints_to_bytes(mimc_rows), False)]
    for kind, b, trace, clean in cases:
        desc, keep = b.build()
        before = hip_ctx.air_prove(desc, trace, opt)
        found = hip_ctx.air_check_trace(desc, trace, opt)
        assert found == b.check_trace(air.trace_to_ints(trace).tolist())
        accepted = api.air_verify(before, desc, opt)
        assert (hip_ctx.last_check_total == 0) == accepted == clean
        if kind:
            assert before == O.example_prove(kind, trace, options)
        assert hip_ctx.air_prove(desc, trace, opt) == before     # the check left the context as a proof needs it
        found2 = hip_ctx.air_check_trace(desc, trace, None, [])  # without options: the smallest commitments, the same report
        assert found2 == found
        assert hip_ctx.air_prove(desc, trace, opt) == before


# ---- 8. the flag-only check and the report share one row evaluation: the edges of the launch -------------------------------------
@pytest.mark.parametrize("n,cell_rows", [(8, (6, 0)), (512, (510, 0, 256))], ids=["less than one wave", "two blocks"])
def test_flag_and_report_agree_at_the_edges_of_the_launch(hip_ctx, n, cell_rows):
    """periodic_airs.linear (periods 2 and 8: at n = 8 every period wraps inside the one partial wave): a clean trace takes the 2n-point
    path and reports nothing; one cell of column 0 changed on the last enforced row, on row 0, on the first row of the second block
    makes the prover's flag leave that path and the report name constraint 0 on the rows the model names."""
    b, rows = periodic_airs.linear(n, periodic_airs.keys(51, 2), periodic_airs.keys(52, 8))
    desc, keep = b.build()
    hip_ctx.air_prove(desc, air.ints_to_bytes(rows), OPT)
    assert hip_ctx.last_proof_info()["composition_path"] == 1
    assert same(hip_ctx, b, rows) == []
    for row in cell_rows:
        bad = X.changed(rows, (row, 0, 1))
        hip_ctx.air_prove(desc, air.ints_to_bytes(bad), OPT)
        assert hip_ctx.last_proof_info()["composition_path"] != 1, row
        got = same(hip_ctx, b, bad)                                  # rows, first_row, last_row (and value) equal to the model's
        hit = [v for v in got if v.kind == 0 and v.index == 0]      # a' - a - K0 breaks on the row of the cell and on the one before it
        assert [(v.first_row, v.last_row) for v in hit] == [(max(row - 1, 0), row)], row
