"""Randomized main and auxiliary programs without a GPU: the Python models (air.MainProgram.evaluate, air.AuxProgram.evaluate) equal the
plain reference of program_ref.py cell for cell - the first test of the models against something that was not written with them -, every
generated program passes the builder's and the library's decoder, the fixed seed lists of test_gpu_air_program_fuzz.py hold every
combination they are there for, and the generator is deterministic.

One seed alone: `pytest tests/test_air_program_fuzz.py -k "main and n64"` runs all main seeds at 64 rows and names the seed that differs;
`python -c "import program_fuzz as F; print(F.describe_main(17, 64))"` (from tests/) prints that program."""
import ctypes
import random

import pytest

import lookup_airs as L
import program_fuzz as F
import program_ref as R
import program_shapes as S
from lambdaworks_cairo_prover_amd import _lib, air

P = air.P
CPU_SIZES = [8, 64, 256]


def ints(table):
    return [[int(v) for v in row] for row in table]


def first_difference(got, want):
    return next(((i, c, got[i][c], want[i][c]) for i in range(len(want)) for c in range(len(want[i])) if got[i][c] != want[i][c]), None)


# ---- the models against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CPU_SIZES)
def test_main_model_equals_the_reference(n):
    for seed in F.MAIN_SEEDS:
        b, rows, _ = F.random_main(seed, n)
        want = F.main_table(seed, n)                  # (R.main_table, from the generator's own run of it)
        assert n > 8 or want == R.main_table(b.main, rows)
        assert first_difference(ints(b.main.evaluate(rows)), want) is None, ("main seed", seed)


@pytest.mark.parametrize("n", CPU_SIZES)
def test_aux_model_equals_the_reference(n):
    for seed in F.AUX_SEEDS:
        b, rows, _ = F.random_aux(seed, n)
        rap = F.GEN_RAP[:b.n_rap]
        want = F.aux_columns(seed, n)                 # (R.aux_table under GEN_RAP, from the generator's own run of it)
        assert first_difference(ints(b.aux.evaluate(rows, rap)), want) is None, ("aux seed", seed)
        if n == 8:                                    # and under other challenges
            rap = (P - 1, 5, 1 << 200)[:b.n_rap]
            assert want == R.aux_table(b.aux, rows, F.GEN_RAP[:b.n_rap], b.periodic_cols)
            assert first_difference(ints(b.aux.evaluate(rows, rap)), R.aux_table(b.aux, rows, rap, b.periodic_cols)) is None, ("aux seed", seed)


@pytest.mark.parametrize("n", [8, 64])
def test_pinned_rows_satisfy_the_pinning_air(n):
    """The AIR of the device test: the expected auxiliary columns as main columns, one constraint aux_k - E_k a column."""
    for seed in F.AUX_SEEDS[:6]:
        b, rows, rap = F.pinned_aux(seed, n)
        plain, _, _ = F.random_aux(seed, n)
        assert b.aux.cols == plain.aux.cols and len(b.degrees) == len(b.aux.cols) and len(rows[0]) == b.main_cols
        assert b.check_trace(rows, rap) == []
        k, r = len(b.aux.cols) - 1, n - 1
        rows = [list(row) for row in rows]
        rows[r][plain.main_cols + k] = (rows[r][plain.main_cols + k] + 1) % P
        assert b.check_trace(rows, rap) == [air.Violation(air.TRANSITION, k, 1, r, r, P - 1)]


def test_the_reference_on_a_hand_written_table():
    rng = random.Random(3)
    periodic = [rng.randrange(P) for _ in range(L.MIXED_PERIOD)]
    b, cols = L.mixed(periodic)
    rows = L.mixed_inputs(64, periodic, rng)
    assert R.main_table(b.main, rows) == L.hand_table(rows, periodic)


def test_the_reference_raises_where_the_library_refuses():
    b = air.AirBuilder(3, [0], 1, main_inputs=2)
    b.main.value(1, b.main.load(0, 0) - 5)
    with pytest.raises(ZeroDivisionError):
        R.main_table(b.main, [[6, 0], [5, 0]])
    with pytest.raises(ValueError, match="out of range"):
        R.main_table(L.plain_count(8).main, [[255, 1], [3, 256]])
    x = air.AirBuilder(1, [0], 1, aux_cols=2, n_rap=1, aux_kind=air.AUX_PROGRAM).aux
    x.sorted(x.load(0, 0), (), 8)
    x.running_sum(1, x.load(0, 0) - x.rap(0))
    with pytest.raises(ValueError, match="out of range"):
        R.aux_table(x, [[256], [1]], [9], [])
    with pytest.raises(ZeroDivisionError):
        R.aux_table(x, [[7], [9]], [9], [])
    assert R.aux_table(x, [[7], [3]], [9], []) == [[3, 0], [7, pow(7 - 9, P - 2, P)]]


# ---- every program is one the library takes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 64])
def test_generated_main_programs_pass_both_decoders(hip_lib, n):
    for seed in F.MAIN_SEEDS:
        b, rows, _ = F.random_main(seed, n)
        m = b.main
        m.check(n)
        assert 1 <= m.input_cols <= 3 and 4 <= len(m.cols) <= 40 and len(b.periodic_cols) <= 3 and F.max_live(m.ops) <= F.MAX_LIVE
        desc, keep = b.build()
        x = air.ext_of(desc)
        rc = hip_lib.sp_air_main_check_lk(ctypes.byref(desc), ctypes.byref(x), ctypes.byref(desc.main_desc), ctypes.c_uint64(n))
        assert rc == _lib.SP_OK, (seed, hip_lib.sp_last_error().decode())


@pytest.mark.parametrize("n", [8, 64])
def test_generated_aux_programs_are_within_the_limits(hip_lib, n):
    for seed in F.AUX_SEEDS:
        b, rows, _ = F.random_aux(seed, n)
        x = b.aux
        scans = sum(1 for c in x.cols if c[0] != air.AUX_SORTED)
        assert 2 <= b.main_cols <= 6 and 1 <= b.n_rap <= 3 and 3 <= scans <= 40 and 1 <= len(x.sort_groups()) <= 4
        assert F.max_live(x.ops) <= F.MAX_LIVE
        b.build()                                  # check_limits
        assert air.needs_pub(b.build()[0]) == x.reads_table()


# ---- the seed lists hold what they are there for -----------------------------------------------------------------------------------
def test_the_main_seeds_cover_every_combination():
    found = set()
    for n in (8, 64):
        for seed in F.MAIN_SEEDS:
            found |= F.random_main(seed, n)[2]
    missing = [f for f in F.MAIN_FEATURES + F.MAIN_SHAPES if f not in found]
    assert not missing, missing
    kinds = {c[0] for n in (8, 64) for seed in F.MAIN_SEEDS for c in F.random_main(seed, n)[0].main.cols}
    assert kinds == set(range(7))
    key_bits = {c[3] for n in (8, 64) for seed in F.MAIN_SEEDS for c in F.random_main(seed, n)[0].main.cols if c[0] == air.MAIN_COUNT}
    assert key_bits == set(F.KEY_BITS)


def test_the_aux_seeds_cover_every_combination():
    found, key_bits, tables, carried = set(), set(), 0, 0
    for n in (64, 256):
        for seed in F.AUX_SEEDS:
            b, rows, features = F.random_aux(seed, n)
            found |= features
            key_bits |= set(b.aux.key_bits.values())
            tables += b.aux.reads_table()
            carried += any(len(members) > 1 for members in b.aux.sort_groups().values())
    missing = [f for f in F.AUX_FEATURES if f not in found]
    assert not missing, missing
    assert 64 in key_bits and min(key_bits) < 16 and tables and carried


def test_the_features_of_hand_written_programs():
    """main_chunks and main_features on programs whose cuts are known."""
    b = air.AirBuilder(9, [0], 1, periodic=[[1, 2]], main_inputs=1)
    m = b.main
    x = m.load(0, 0) + 3
    m.bit(x, 0)                                           # 1
    m.inv_or_zero(m.load(0, 0))                           # 2
    m.value(m.load(1, 1) + m.periodic(0, 0))              # 3 reads 1: the second chunk
    m.bit(x, 5)                                           # 4: the same N as column 1, in the other chunk
    m.running_sum(m.load(0, 0) + 3)                       # 5: a scan directly behind a BIT
    g = m.chain(8, [m.load(0, 0)])                        # 6
    g.step([g.state(0)])
    m.multiplicity(m.load(7, 6), m.load(0, 0), 8)         # 7
    m.value(m.load(0, 3) + m.load(0, 7))                  # 8
    assert F.main_chunks(m, 8) == [("rows", 0, 2), ("rows", 2, 3), ("chain", 5, 1), ("count", 6, 1), ("rows", 7, 1)]
    assert F.main_features(m, 8) == set(F.MAIN_FEATURES) | {"three_dependency_levels", "chain_block_length_n"}
    assert F.main_chunks(m, 1 << 21) == [("rows", 0, 2), ("rows", 2, 2), ("rows", 4, 1), ("chain", 5, 1), ("count", 6, 1), ("rows", 7, 1)]


def test_the_shape_cases_cut_where_they_are_meant_to():
    # (e) the slot file: 64 values alive with the dead one dropped, one more where it is kept or another value is added
    for make in (S.slot_file_main, S.slot_file_aux):
        for live in (64, 65):
            b = make(live)
            p = b.main if b.main is not None else b.aux
            assert F.max_live(p.ops, [p.cols[0][1]]) == live and F.max_live(p.ops) == live + 1
    rows = [[5 + 3 * i] for i in range(8)]
    b = S.slot_file_main(64)
    assert [r[1] for r in R.main_table(b.main, rows)] == S.slot_file_expected(rows, 64) == [int(r[1]) for r in b.main.evaluate(rows)]
    # (a) 66 columns at 2^16 rows: a chunk of 64 and a chunk of 2, a product and a sum with a D on either side
    x = S.aux_chunk_seam().aux
    assert F.aux_chunks(x, S.AUX_SEAM_N) == [(0, 64), (64, 2)]
    assert [(c[0], c[2] != air.AUX_NO_DEN) for c in x.cols[62:]] == [(air.AUX_PRODUCT, True), (air.AUX_SUM, True)] * 2
    read = [{x.ops[t][2] for t in F.closure(x.ops, [c[1], c[2]]) if x.ops[t][0] == air.OP_LOAD} for c in x.cols]
    assert set().union(*read[:64]) == {0, 1} and set().union(*read[64:]) == {2, 3}
    # (b) 65 carried values where a pass holds 64
    x = S.second_sort_pass().aux
    groups = list(x.sort_groups().values())
    assert [len(g) - 1 for g in groups] == [65, 1] and [x.key_bits[g[0]] for g in groups] == [16, 64]
    assert max(1, min(len(x.cols), F.CHUNK_ELEMS // S.SORT_PASS_N)) == 64 < S.SORT_PASS_CARRIED
    # (c) 512 scan blocks; (d) one chunk, 16 and 15 inverted columns
    assert S.SCAN_TOTALS_N // 2048 == 512 and F.main_chunks(S.scan_totals().main, S.SCAN_TOTALS_N) == [("rows", 0, 3)]
    a = S.scan_totals_input(1 << 13)
    b = S.scan_totals()
    assert S.scan_totals_expected(a).tolist() == air.ints_to_bytes(R.main_table(b.main, [[int(v)] for v in a])).tolist()
    for count in (16, 15):
        m = S.batch_inverse_columns(count).main
        assert F.main_chunks(m, S.BATCH_INVERSE_N) == [("rows", 0, count)]
        assert sum(1 for c in m.cols if c[2] != air.AUX_NO_DEN or c[0] == air.MAIN_INV_OR_ZERO) == count
    assert 16 * S.BATCH_INVERSE_N == 1 << 16 > 15 * S.BATCH_INVERSE_N
    rows = S.batch_inverse_inputs(random.Random(1))[:64]
    whole = R.main_table(S.batch_inverse_columns(16).main, rows)
    assert R.main_table(S.batch_inverse_columns(15).main, rows) == [row[:3] + row[4:] for row in whole]   # the 15 are the last 15 of the 16
    assert [row[5] == 0 for row in whole[:2]] == [True, False]                                          # the first INV_OR_ZERO, z = 0 on row 0


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_the_generator_is_deterministic():
    for seed in (F.MAIN_SEEDS[0], F.MAIN_SEEDS[-1]):
        (b1, rows1, f1, t1), (b2, rows2, f2, t2) = F._main.__wrapped__(seed, 64), F._main.__wrapped__(seed, 64)
        assert b1 is not b2 and (b1.main.ops, b1.main.consts, b1.main.cols, b1.periodic_cols, rows1, f1, t1) == \
            (b2.main.ops, b2.main.consts, b2.main.cols, b2.periodic_cols, rows2, f2, t2)
    for seed in (F.AUX_SEEDS[0], F.AUX_SEEDS[-1]):
        (b1, rows1, f1, t1), (b2, rows2, f2, t2) = F._aux.__wrapped__(seed, 64, False), F._aux.__wrapped__(seed, 64, False)
        assert b1 is not b2 and (b1.aux.ops, b1.aux.consts, b1.aux.cols, b1.aux.key_bits, b1.periodic_cols, rows1, f1, t1) == \
            (b2.aux.ops, b2.aux.consts, b2.aux.cols, b2.aux.key_bits, b2.periodic_cols, rows2, f2, t2)
    assert F.random_main(F.MAIN_SEEDS[0], 64)[0].main.ops != F.random_main(F.MAIN_SEEDS[1], 64)[0].main.ops
