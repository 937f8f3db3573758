"""One multiplicity column for several looked-up columns (joint COUNT columns, op 12, the _multi entry points) without a GPU: the new
symbols in the header, the binding and the Rust block, the unchanged ABI and struct sizes, MainLevel.MULTI, the routing, the decoder's
verdicts through sp_air_main_check_multi - and the older entry points' on the same descriptors -, the builder's mirror of them, and the
Python-integer model (MainProgram.evaluate, AirBuilder.check_trace) against the plain reference of multi_ref and the worked example's
own table."""
import ctypes
import os
import random
import re

import pytest

import multi_programs as G
import multi_ref as R
from air_main_checks import _col, _first, _op, check_with, decoder_refuses_and_the_builder_raises
from lambdaworks_cairo_prover_amd import _lib, air, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = air.P
N = 64
NEW_SYMBOLS = ("sp_air_prove_multi", "sp_air_check_trace_multi", "sp_air_main_trace_multi", "sp_air_main_check_multi", "sp_air_main_multi_limits")
INVALID = _lib.SP_E_INVALID_ARG
OUT_OF_RANGE = "a lookup key is out of range on some row"


def ints(table):
    return [[int(x) for x in r] for r in table]


def test_symbols_are_declared_everywhere_the_abi_is_7_and_the_structs_keep_their_sizes(hip_lib):
    header = open(os.path.join(ROOT, "include", "stark252_hip.h")).read()
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = integ.index("```rust")
    rust = set(re.findall(r"pub fn (sp_[a-z0-9_]+)\s*\(", integ[start:integ.index("```\n", start + 10)]))
    for name in NEW_SYMBOLS:
        assert name in declared and name in rust and name in _lib.NEWEST_SYMBOLS and hasattr(hip_lib, name), name
    assert int(re.search(r"#define SP_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.SP_ABI_VERSION == hip_lib.sp_abi_version() == 7
    assert int(re.search(r"#define SP_AIR_OP_ALSO\s+(\d+)", header).group(1)) == air.OP_ALSO == 12
    assert int(re.search(r"#define SP_AIR_MAIN_COUNT_LIST\s+(\d+)", header).group(1)) == air.MAIN_COUNT_LIST == 256
    assert int(re.search(r"#define SP_AIR_LIST_END\s+(\w+)", header).group(1), 16) == air.LIST_END == 0xFFFF
    hip_lib.sp_air_main_desc_size.restype = ctypes.c_uint64
    assert ctypes.sizeof(air.AirMainDescC) == hip_lib.sp_air_main_desc_size() == 64
    assert ctypes.sizeof(air.AirMainColumnC) == 16 and ctypes.sizeof(air.AirOpC) == 8


def test_the_limits_call(hip_lib):
    assert api.air_main_multi_limits() == {"list": 16, "key_bits": 64, "columns": 16}
    assert api.air_main_multi_limits() == {"list": air.MAIN_COUNT_MAX_LIST, "key_bits": air.MAIN_COUNT_MAX_KEY_BITS, "columns": air.MAIN_COUNT_MAX_COLS}
    out = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    assert hip_lib.sp_air_main_multi_limits(out) == _lib.SP_OK and list(out) == [16, 64, 16, 0]
    assert hip_lib.sp_air_main_multi_limits(None) == INVALID


def test_the_multi_level_stands_above_int_and_the_worked_example_is_routed_to_it(hip_lib):
    level = air.MainLevel.MULTI
    assert (int(level), level.suffix) == (8, "multi") and level is air.MainLevelMulti.MULTI and level not in list(air.MainLevel)
    assert len(list(air.MainLevel)) == 6 and (int(air.MainLevel.INT), air.MainLevel.INT.suffix) == (7, "int")
    assert level > air.MainLevel.INT and all(level > x for x in air.MainLevel)
    b = air.limb_range_check_joint(256, 4, 4)
    desc, keep = b.build()
    assert air.main_level(desc) == level and air.needs_multi(desc) and air.needs_word(desc) and air.needs_lk(desc) and not air.needs_int(desc)
    assert [air.route(desc, c)[0] for c in ("prove", "check_trace")] == ["sp_air_prove_multi", "sp_air_check_trace_multi"]
    assert not air.route(desc, "verify")[0].endswith("_multi")
    assert check_with(hip_lib, "multi", desc, 256) == _lib.SP_OK, hip_lib.sp_last_error()
    api.air_main_check(desc, 256)
    assert (b.main_cols, b.aux_cols) == (6, 3)                           # against the 9 + 4 of limb_range_check(n, 4, 4)
    old = air.limb_range_check(256, 4, 4)
    assert (old.main_cols, old.aux_cols) == (9, 4)
    # a descriptor put together by hand is looked through
    del desc.main_features
    assert air.needs_multi(desc) and air.route(desc, "prove")[0] == "sp_air_prove_multi"


def test_route_picks_multi_only_when_it_must_and_the_new_decoder_takes_the_older_programs(hip_lib):
    older = ((air.zero_count(N, 3), "main"), (air.mimc_blocks(N, 8, [7] * 8, 0), "rec"), (air.xor_lookup(256, 4), "lk"), (air.table_lookup_main(256, list(range(16)), 8), "lk"),
             (air.mimc_sponge(N, 4, 2, [7] * 4, 0), "link"), (air.xor_fetch(256, 4), "fetch"), (air.word_ops(256, 8), "word"), (air.limb_range_check(256, 8, 2), "word"),
             (air.arx_chain(N, 8, [1] * 8, 0), "int"), (G.old_only(), "lk"), (G.single(False), "lk"))
    for b, suffix in older:
        desc, keep = b.build()
        assert not air.needs_multi(desc) and air.main_suffix(desc) == suffix and air.route(desc, "prove")[0] == f"sp_air_prove_{suffix}"
        assert check_with(hip_lib, "multi", desc, 256) == _lib.SP_OK, hip_lib.sp_last_error()
    for b in (G.single(True), G.plain_joint(), G.case(N, 3, 16, "limb", 0)[0]):
        desc, keep = b.build()
        assert air.needs_multi(desc) and air.route(desc, "prove")[0] == "sp_air_prove_multi" and air.route(desc, "check_trace")[0] == "sp_air_check_trace_multi"


# ---- the model against the plain reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_bits", [1, 16, 64])
@pytest.mark.parametrize("n", [8, 64, 512, 4096])
def test_model_equals_the_plain_reference(n, key_bits):
    top = False
    for L in (1, 2, 3, 16):
        for shape in G.SHAPES:
            b, rows = G.case(n, L, key_bits, shape, 1)
            want = R.main_table(b.main, rows)
            got = ints(b.main.evaluate(rows))
            for i in range(n):
                assert got[i] == want[i], (L, shape, i)
            assert b.main.level == air.MainLevel.MULTI and sum(1 for o in b.main.ops if o[0] == air.OP_ALSO) == L
            m_col = b.main_cols - 1
            assert sum(r[m_col] for r in want) <= L * n
            top |= any(v >> 63 for r in rows for v in r[:1]) and shape != "limb"
            if shape in ("hot", "distinct", "period", "periodic"):
                assert sum(r[m_col] for r in want) == L * n, (L, shape)       # every lookup hits
            if shape == "hot":
                assert sorted(r[m_col] for r in want)[-2:] == [0, L * n]       # all of it on one row
            if shape == "unlooked" and key_bits > 1:
                assert 0 < sum(r[m_col] for r in want) < L * n and sum(1 for r in want if r[m_col] == 0) > n // 4
    assert top == (key_bits == 64)


def test_a_list_of_one_is_the_plain_column_and_the_list_order_does_not_matter():
    rng = random.Random(5)
    rows = G.lookup_rows(N, 2, 16, rng)
    assert ints(G.single(True).main.evaluate(rows)) == ints(G.single(False).main.evaluate(rows)) == R.main_table(G.single(True).main, rows) == R.main_table(G.single(False).main, rows)
    b, rows = G.case(N, 3, 16, "unlooked", 2)
    m = b.main
    xs = m.list_of(m.cols[-1][1])
    assert len(xs) == 3 and [m.ops[x][:1] for x in xs] == [(air.OP_LOAD,)] * 3 and [m.ops[x][2] for x in xs] == [0, 1, 2]
    want = R.main_table(m, rows)
    swapped = [[r[2], r[0], r[1], r[3]] for r in rows]
    assert [r[-1] for r in R.main_table(m, swapped)] == [r[-1] for r in want]


def test_evaluate_and_the_reference_refuse_the_same_rows():
    b, rows = G.case(N, 3, 16, "period", 3)
    assert ints(b.main.evaluate(rows)) == R.main_table(b.main, rows)
    for col, value in ((2, 1 << 16), (2, P - 1), (0, 1 << 64), (3, 1 << 16)):       # the last X, the first, the table
        bad = [list(r) for r in rows]
        bad[17][col] = value
        with pytest.raises(ValueError, match=OUT_OF_RANGE):
            b.main.evaluate(bad)
        with pytest.raises(R.KeyOutOfRange):
            R.main_table(b.main, bad)
    quiet = [list(r) for r in rows]
    quiet[17][2] = (1 << 16) - 1                 # in range, and in no table row: counted nowhere, no error
    assert ints(b.main.evaluate(quiet)) == R.main_table(b.main, quiet)


# ---- the worked example ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,limb_bits,count", [(64, 4, 4), (64, 3, 3), (32, 4, 1), (256, 7, 2)])
def test_the_worked_example_satisfies_its_own_constraints_and_names_what_breaks(n, limb_bits, count):
    b = air.limb_range_check_joint(n, limb_bits, count)
    rng = random.Random(n + count)
    rows = air.limb_range_check_joint_inputs(n, limb_bits, count, rng)
    table = air.limb_range_check_joint_trace(rows, limb_bits, count)
    assert table == ints(b.main.evaluate(rows)) == R.main_table(b.main, rows)
    assert (b.main_cols, b.aux_cols) == (count + 2, (count + 1) // 2 + 1) and sum(1 for c in b.main.cols if c[0] == air.MAIN_COUNT) == 1
    assert max(b.degrees) <= 3 and rows[-1] == [0] and table[-1][-1] == 0
    assert sum(r[-1] for r in table) == n * count                       # every limb of every row, the padding row's zeros included
    rap = [rng.randrange(P)]
    assert b.check_trace(rows, rap) == b.check_trace(table, rap) == []
    # an x at or above 2^(limb_bits count): its limbs are limbs all the same, and the recomposition (constraint 0) breaks on its row
    bad = [list(r) for r in rows]
    bad[5] = [(1 << (limb_bits * count)) + 3]
    report = [(v.kind, v.index, v.rows, v.first_row) for v in b.check_trace(bad, rap)]
    assert report == [(air.TRANSITION, 0, 1, 5)], report
    # a wrong m: the sum does not close
    wrong = [list(r) for r in table]
    wrong[2][count + 1] += 1
    report = b.check_trace(wrong, rap)
    assert report and all(v.kind == air.BOUNDARY and v.first_row == n - 1 for v in report), report
    # the padding row is public: another x there breaks its boundary constraint
    moved = [list(r) for r in rows]
    moved[-1] = [1]
    assert any(v.kind == air.BOUNDARY for v in b.check_trace(moved, rap))
    for args in ((64, 6, 2), (64, 4, 17), (64, 0, 2)):
        with pytest.raises(ValueError, match="limb_range_check_joint"):
            air.limb_range_check_joint(*args)


# ---- the decoder and its mirror --------------------------------------------------------------------------------------------------
def refusal_builder():
    """Inputs x, y and a table value t.  Derived column 0: the joint multiplicity of (x, y, x + y) in t; 1: a VALUE; 2: a plain COUNT
    column; 3: a FETCH; 4: a LIMB; 5: a second joint column, over a shifted read of the LIMB."""
    b = air.AirBuilder(9, [0], 1, main_inputs=3)
    m = b.main
    x, y, t = m.load(0, 0), m.load(0, 1), m.load(0, 2)
    m.multiplicity_many([x, y, x + y], t, 16)
    m.value(x + y)
    m.multiplicity(x, t, 16)
    m.fetch(t, t, y, 16)
    c = m.limb(x, 4, 8)
    m.multiplicity_many([m.load(3, c)], t, 16)
    v = b.load(0, 0)
    b.constraint(v - v, degree=1, exemptions=0)
    return b


def _is_cell(o):
    return o[0] == air.OP_ALSO


def _head(m, k=0):
    return m.cols[k][1]


def _new_list(k, *extra_ops):
    """Column k counts a new list of one: the value of the last of `extra_ops`, which are appended first."""
    def mutate(m):
        m.ops.extend(extra_ops)
        m.ops.append((air.OP_ALSO, len(m.ops) - 1, air.LIST_END))
        _col(k, num_op=len(m.ops) - 1)(m)
    return mutate


def _long_list(m):
    cell = _head(m)
    for _ in range(14):                          # 3 + 14 = 17 cells
        m.ops.append((air.OP_ALSO, 0, cell))
        cell = len(m.ops) - 1
    _col(0, num_op=cell)(m)


def _fetch_value_is_a_cell(m):
    kind, num_op, den_op, pad = m.cols[3]
    m.cols[3] = (kind, num_op, den_op, (pad & 255) + 256 * _head(m))


CELL = "names a list cell (op 12), which only the num_op of a COUNT column with bit 8 of its pad may"
REFUSALS = [
    ("pad-bit-9", _col(0, pad=16 + 256 + 512), "derived column 0 is a COUNT column whose pad has a bit above 8"),
    ("pad-bit-31", _col(5, pad=16 + 256 + (1 << 31)), "derived column 5 is a COUNT column whose pad has a bit above 8"),
    ("bit-8-without-a-list", _col(0, num_op=0), "derived column 0 is a COUNT column with bit 8 of its pad whose num_op = 0 is no list cell"),
    ("bit-8-on-the-plain-column", _col(2, pad=16 + 256), "derived column 2 is a COUNT column with bit 8 of its pad whose num_op = 0 is no list cell"),
    ("list-without-bit-8", lambda m: _col(2, num_op=_head(m))(m), "derived column 2 " + CELL),
    ("bit-8-dropped", _col(0, pad=16), "derived column 0 " + CELL),
    ("cell-a-beyond", _op(_is_cell, a=60000), " is a list cell (op 12) whose a = 60000 is no earlier value op"),
    ("cell-a-is-itself", lambda m: _op(_is_cell, a=_first(m, _is_cell))(m), " is a list cell (op 12) whose a = "),
    ("cell-a-is-a-cell", lambda m: m.ops.__setitem__(_head(m), (air.OP_ALSO, _first(m, _is_cell), m.ops[_head(m)][2])), " is no earlier value op (a cell names one looked-up value, and no cell)"),
    ("cell-b-is-a-value", _op(_is_cell, b=2), " is a list cell (op 12) whose b = 2 is neither 0xFFFF nor an earlier cell"),
    ("cell-b-is-later", lambda m: _op(_is_cell, b=_head(m))(m), " is neither 0xFFFF nor an earlier cell"),
    ("seventeen-cells", _long_list, "derived column 0 is a COUNT column with a list of more than 16 looked-up values"),
    ("cell-as-an-operand", lambda m: m.ops.append((air.OP_ADD, _head(m), 0)), " takes a list cell (op 12) for an operand, and a cell has no value"),
    ("cell-as-the-second-operand", lambda m: m.ops.append((air.OP_MUL, 0, _head(m))), " takes a list cell (op 12) for an operand, and a cell has no value"),
    ("cell-as-an-out", lambda m: m.ops.append((air.OP_OUT, 0, _head(m))), " takes a list cell (op 12) for an operand, and a cell has no value"),
    ("cell-as-the-table", lambda m: _col(0, den_op=_head(m, 5))(m), "derived column 0 " + CELL),
    ("cell-as-a-denominator", lambda m: _col(1, den_op=_head(m))(m), "derived column 1 " + CELL),
    ("cell-behind-a-value", lambda m: _col(1, num_op=_head(m))(m), "derived column 1 " + CELL),
    ("cell-behind-a-fetch-key", lambda m: _col(3, num_op=_head(m))(m), "derived column 3 " + CELL),
    ("cell-as-a-fetch-value", _fetch_value_is_a_cell, "derived column 3 " + CELL),
    ("cell-behind-a-limb", lambda m: _col(4, num_op=_head(m))(m), "derived column 4 " + CELL),
    ("x-behind-a-quotient", _new_list(0, (air.OP_DIV, 0, 1)),
     "derived column 0 depends on a quotient (op 7), which only the seed or the step of a CHAIN column may: a row-local quotient is a VALUE column's N / D"),
    ("x-behind-an-integer-op", _new_list(5, (air.OP_INT_XOR, 0, 1), (air.OP_ADD, 0, -1)),
     "derived column 5 depends on an integer op (ops 8 .. 11), which only the seed or the step of a CHAIN column may: a row-local limb or word is a LIMB or WORD column"),
    ("x-reads-a-later-column", _new_list(0, (air.OP_LOAD, 1, 3 + 4)), "derived column 0 reads derived column 4, which is not an earlier one"),
    ("x-reads-its-own-column", _new_list(5, (air.OP_LOAD, 0, 3 + 5)), "derived column 5 reads derived column 5, which is not an earlier one"),
    ("key-bits-0", _col(0, pad=256), "derived column 0 is a COUNT column with key_bits = 0 (1 .. 64)"),
    ("key-bits-65", _col(0, pad=256 + 65), "derived column 0 is a COUNT column with key_bits = 65 (1 .. 64)"),
    ("no-table", _col(5, den_op=air.AUX_NO_DEN), "derived column 5 is a COUNT column without a table"),
]


def _fix_relative(mutate):
    """(air.OP_ADD, 0, -1) in a mutator's ops: -1 stands for the op before it."""
    def fixed(m):
        before = len(m.ops)
        mutate(m)
        for t in range(before, len(m.ops)):
            op, a, b = m.ops[t]
            if b == -1:
                m.ops[t] = (op, a, t - 1)
        # (the new cell names the last value op, which is the one before it)
    return fixed


@pytest.mark.parametrize("mutate,says", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_decoder_refuses_and_the_builder_raises(hip_lib, mutate, says):
    raised, message = decoder_refuses_and_the_builder_raises(hip_lib, "multi", refusal_builder, _fix_relative(mutate), says, N)
    assert ("derived column" in message) == ("derived column" in says)


def test_the_limits_of_the_list_and_of_the_columns(hip_lib):
    """Sixteen looked-up values are a list, seventeen are not; sixteen COUNT columns of both forms together are a program, seventeen are not."""
    b = air.AirBuilder(3, [0], 1, main_inputs=2)
    m = b.main
    m.multiplicity_many([m.load(k % 8, 0) for k in range(16)], m.load(0, 1), 64)
    v = b.load(0, 0)
    b.constraint(v - v, degree=1, exemptions=0)
    desc, keep = b.build()
    assert check_with(hip_lib, "multi", desc, N) == _lib.SP_OK, hip_lib.sp_last_error()
    with pytest.raises(ValueError, match="17 looked-up values"):
        m.multiplicity_many([m.load(0, 0)] * 17, m.load(0, 1))
    with pytest.raises(ValueError, match="0 looked-up values"):
        m.multiplicity_many([], m.load(0, 1))

    def many():      # sixteen COUNT columns, joint and plain in turn, and a VALUE column behind them
        b = air.AirBuilder(2 + 17, [0], 1, main_inputs=2)
        m = b.main
        x, t = m.load(0, 0), m.load(0, 1)
        for k in range(16):
            if k % 2 == 0:
                m.multiplicity_many([x, x + k], t, 16)
            else:
                m.multiplicity(x, t, 16)
        m.value(x)
        v = b.load(0, 0)
        b.constraint(v - v, degree=1, exemptions=0)
        return b
    m = many().main
    with pytest.raises(ValueError, match="more than 16 multiplicity columns"):
        m.multiplicity_many([m.load(0, 0)], m.load(0, 1))
    with pytest.raises(ValueError, match="more than 16 multiplicity columns"):
        m.multiplicity(m.load(0, 0), m.load(0, 1))
    decoder_refuses_and_the_builder_raises(hip_lib, "multi", many, _col(16, kind=air.MAIN_COUNT, den_op=1, pad=16),
                                           "derived column 16 is the program's COUNT column number 17 (at most 16)", N)
    decoder_refuses_and_the_builder_raises(hip_lib, "multi", many, lambda m: _col(16, kind=air.MAIN_COUNT, num_op=_head(m), den_op=1, pad=16 + 256)(m),
                                           "derived column 16 is the program's COUNT column number 17 (at most 16)", N)


def test_below_multi_a_cell_is_a_malformed_op_and_bit_8_a_key_bits_out_of_range(hip_lib):
    b = refusal_builder()
    desc, keep = b.build()
    first = _first(b.main, _is_cell)
    for suffix in ("int", "word", "fetch", "lk"):
        assert check_with(hip_lib, suffix, desc, N) == INVALID, suffix
        message = hip_lib.sp_last_error().decode()
        assert message.startswith(f"sp_air_main_check_{suffix}: main program: malformed op {first} "), message
    for level in (air.MainLevel.INT, air.MainLevel.WORD, air.MainLevel.LK):
        with pytest.raises(ValueError, match=f"malformed op {first} "):
            b.main.check(N, level=level)
    b.main.check(N)
    # bit 8 alone, on a program without a cell: today's refusal of a key_bits above 64
    b = G.single(False)
    desc, keep = b.build()
    _col(0, pad=16 + 256)(b.main)
    desc.main_desc, keep2 = air.main_desc(b.main.input_cols, b.main.ops, b.main.consts, b.main.cols)
    for suffix in ("int", "word", "lk"):
        assert check_with(hip_lib, suffix, desc, N) == INVALID, suffix
        message = hip_lib.sp_last_error().decode()
        assert message == f"sp_air_main_check_{suffix}: main program: derived column 0 is a COUNT column with key_bits = 272 (1 .. 64)", message
    with pytest.raises(ValueError, match=re.escape("derived column 0 is a COUNT column with key_bits = 272 (1 .. 64)")):
        b.main.check(N, level=air.MainLevel.INT)
    # and the old form through the new decoder is the old form
    b = G.single(False)
    desc, keep = b.build()
    assert check_with(hip_lib, "multi", desc, N) == check_with(hip_lib, "lk", desc, N) == _lib.SP_OK


def test_null_arguments(hip_lib):
    desc, keep = G.plain_joint().build()
    n = ctypes.c_uint64(N)
    assert hip_lib.sp_air_main_check_multi(None, None, ctypes.byref(desc.main_desc), n) == INVALID
    assert hip_lib.sp_air_main_check_multi(ctypes.byref(desc), None, None, n) == INVALID
    assert hip_lib.sp_air_prove_multi(None, None, None, None, None, None, n, None, None, None) == INVALID
    assert hip_lib.sp_air_check_trace_multi(None, None, None, None, None, None, n, None, None, None, 0, None) == INVALID
    assert hip_lib.sp_air_main_trace_multi(None, None, None, None, None, n, None) == INVALID
    assert hip_lib.sp_air_main_check_multi(ctypes.byref(desc), None, ctypes.byref(desc.main_desc), n) == _lib.SP_OK     # no op 6: no ext needed


def test_builder_arguments():
    m = air.AirBuilder(8, [0], 1, main_inputs=2).main
    x, t = m.load(0, 0), m.load(0, 1)
    assert not m.multis and m.level == air.MainLevel.REC
    for key_bits in (0, 65):
        with pytest.raises(ValueError, match="key_bits"):
            m.multiplicity_many([x], t, key_bits)
    with pytest.raises(ValueError, match="needs a table value"):
        m.multiplicity_many([x], None)
    other = air.AirBuilder(8, [0], 1, main_inputs=2).main
    with pytest.raises(ValueError, match="values of this program"):
        m.multiplicity_many([x, other.load(0, 0)], t)
    assert not m.multis and not any(o[0] == air.OP_ALSO for o in m.ops)
    before = len(m.ops)
    c = m.multiplicity_many([x, 5, x * x], t, 12)
    assert c == 2 and m.multis and m.level == air.MainLevel.MULTI
    kind, num_op, den_op, pad = m.cols[0]
    assert (kind, den_op, pad) == (air.MAIN_COUNT, t.i, 12 + 256) and m.ops[num_op][0] == air.OP_ALSO and num_op == len(m.ops) - 1
    xs = m.list_of(num_op)
    assert xs[0] == x.i and m.ops[xs[1]][0] == air.OP_CONST and m.ops[xs[2]] == (air.OP_MUL, x.i, x.i)
    cells = [t for t in range(before, len(m.ops)) if m.ops[t][0] == air.OP_ALSO]
    assert len(cells) == 3 and m.ops[cells[0]][2] == air.LIST_END and [m.ops[t][2] for t in cells[1:]] == cells[:2]
    assert air._reachable(m.ops, [num_op]) == [num_op]                  # a leaf: no walk follows it
