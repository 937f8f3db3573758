"""Limbs and bitwise words in a main program (SP_AIR_MAIN_LIMB, SP_AIR_MAIN_WORD, the _word entry points) without a GPU: the new
symbols in the header, the binding and the Rust block, the decoder's verdicts through sp_air_main_check_word - and the older entry
points' on the same descriptors -, the builder's mirror of them, and the Python-integer model (MainProgram.evaluate,
AirBuilder.check_trace) against the plain reference of program_ref and the worked examples' own tables."""
import ctypes
import os
import random
import re

import pytest

import word_airs as W
import program_ref as R
from air_main_checks import _col, _op, check_with, decoder_refuses_and_the_builder_raises
from lambdaworks_cairo_prover_amd import _lib, air, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = air.P
N = 64
NEW_SYMBOLS = ("sp_air_prove_word", "sp_air_check_trace_word", "sp_air_main_trace_word", "sp_air_main_check_word", "sp_air_main_word_limits")
INVALID = _lib.SP_E_INVALID_ARG
OUT_OF_RANGE = "a word operand is out of range on some row"


def ints(table):
    return [[int(x) for x in r] for r in table]


def test_symbols_are_declared_everywhere_and_the_abi_is_7(hip_lib):
    header = open(os.path.join(ROOT, "include", "stark252_hip.h")).read()
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = integ.index("```rust")
    rust = set(re.findall(r"pub fn (sp_[a-z0-9_]+)\s*\(", integ[start:integ.index("```\n", start + 10)]))
    for name in NEW_SYMBOLS:
        assert name in declared and name in rust and name in _lib.NEWEST_SYMBOLS and hasattr(hip_lib, name), name
    assert int(re.search(r"#define SP_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.SP_ABI_VERSION == hip_lib.sp_abi_version() == 7
    assert int(re.search(r"#define SP_AIR_MAIN_LIMB\s+(\d+)", header).group(1)) == 8 == air.MAIN_LIMB == air.SP_AIR_MAIN_LIMB
    assert int(re.search(r"#define SP_AIR_MAIN_WORD\s+(\d+)", header).group(1)) == 9 == air.MAIN_WORD == air.SP_AIR_MAIN_WORD
    hip_lib.sp_air_main_desc_size.restype = ctypes.c_uint64
    assert hip_lib.sp_air_main_desc_size() == ctypes.sizeof(air.AirMainDescC) == 64 and ctypes.sizeof(air.AirMainColumnC) == 16


def test_the_limits_call(hip_lib):
    want = {"limb_end": air.MAIN_LIMB_MAX_END, "bits": air.MAIN_WORD_MAX_BITS, "functions": air.MAIN_WORD_FUNCTIONS}
    assert api.air_main_word_limits() == {"limb_end": 252, "bits": 251, "functions": 3} == want
    out = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    assert hip_lib.sp_air_main_word_limits(out) == _lib.SP_OK and list(out) == [252, 251, 3, 0]
    assert hip_lib.sp_air_main_word_limits(None) == INVALID
    assert (1 << air.MAIN_WORD_MAX_BITS) < P < (1 << air.MAIN_LIMB_MAX_END)


def test_the_word_level_stands_above_fetch_and_its_smallest_example_is_routed_to_it(hip_lib):
    """What tests/test_air_main_level.py holds for each of the six levels below it, for MainLevel.WORD: its place in the order of
    sp::AirMainLevel, its suffix, its four entry points, and the smallest worked example that needs it, at that file's 8 rows."""
    word = air.MainLevel.WORD
    assert (int(word), word.suffix) == (6, "word") and word is air.MainLevelWord.WORD and word not in list(air.MainLevel)
    assert all(word > level for level in air.MainLevel) and max(air.MainLevel.FETCH, word) is word and max(list(air.MainLevel) + [word]) is word
    for name in ("sp_air_prove_word", "sp_air_check_trace_word", "sp_air_main_trace_word", "sp_air_main_check_word"):
        assert hasattr(hip_lib, name), name
    b, rows = air.word_ops(8, 4), air.word_ops_inputs(8, 4, random.Random(6))
    assert len(rows) == 8
    desc, keep = b.build()
    assert air.main_level(desc) == word and air.main_features(desc) == frozenset([word])
    assert air.route(desc, "prove")[0] == "sp_air_prove_word"
    api.air_main_check(desc, 8)


# ---- the model against the plain reference --------------------------------------------------------------------------------------
# (what it covers, n -> (builder, input rows)); every one at 8 and at 64 rows
def _cases(n):
    rng = random.Random(500 + n)
    small = (3, 2) if n == 8 else (4, 2)
    return [
        ("limb_range_check", air.limb_range_check(n, *small), air.limb_range_check_inputs(n, *small, rng)),
        ("word_ops", air.word_ops(n, 8), air.word_ops_inputs(n, 8, rng)),
        ("mixed", W.mixed(4), W.mixed_rows(n, rng)),
        ("limb_group", W.limb_group(), W.limb_rows(n, rng)),
        ("word_groups", W.word_groups(251, 33), W.word_rows(n, 251, 33, rng)),
        ("split_group", W.split_group(True)[0], W.limb_rows(n, rng)),
    ]


@pytest.mark.parametrize("n", [8, 64])
def test_model_equals_the_plain_reference(n):
    for name, b, rows in _cases(n):
        want = R.main_table(b.main, rows)
        got = ints(b.main.evaluate(rows))
        for i in range(n):
            assert got[i] == want[i], (name, i)
        assert any(c[0] in (air.MAIN_LIMB, air.MAIN_WORD) for c in b.main.cols), name


def test_the_worked_examples_tables_are_the_reference_and_the_cells_are_what_they_claim():
    n = 64
    rng = random.Random(3)
    rows = air.limb_range_check_inputs(n, 4, 2, rng)
    b = air.limb_range_check(n, 4, 2)
    table = air.limb_range_check_trace(rows, 4, 2)
    assert table == R.main_table(b.main, rows) == ints(b.main.evaluate(rows))
    assert all(r[0] == r[1] + 16 * r[2] for r in table) and sum(r[3] for r in table) == sum(r[4] for r in table) == n
    rows = air.word_ops_inputs(n, 8, rng)
    b = air.word_ops(n, 8)
    table = air.word_ops_trace(rows, 8)
    assert table == R.main_table(b.main, rows) == ints(b.main.evaluate(rows))
    assert rows[:3] == [[255, 0], [255, 255], [0, 0]] and [r[-3:] for r in table[:3]] == [[0, 255, 255], [255, 255, 0], [0, 0, 0]]
    # a LIMB of width 1 holds the cells of the BIT column, a LIMB of 252 bits from bit 0 the value
    b = W.limb_group()
    rows = W.limb_rows(n, rng)
    table = R.main_table(b.main, rows)
    at = {spec: 1 + j for j, spec in enumerate(W.LIMB_SPECS)}
    bit_at = {j: 1 + len(W.LIMB_SPECS) + k for k, j in enumerate(W.BIT_POSITIONS)}
    for r in table:
        assert all(r[at[(j, 1)]] == r[bit_at[j]] for j in W.BIT_POSITIONS) and r[at[(0, 252)]] == r[0] and r[at[(1, 251)]] == r[0] >> 1
    assert [r[0] for r in table[:6]] + [table[-1][0]] == W.LIMB_OPERANDS
    assert table[2][at[(200, 52)]] == (P - 1) >> 200 == 1 << 51 and table[3][at[(251, 1)]] == 1 and table[4][at[(251, 1)]] == 0


def test_evaluate_and_the_reference_refuse_the_same_rows():
    n = 16
    b = air.word_ops(n, 8)
    rows = air.word_ops_inputs(n, 8, random.Random(4))
    for col, value in ((0, 256), (1, 256), (0, P - 1), (1, P - 1)):
        bad = [list(r) for r in rows]
        bad[n - 1][col] = value
        with pytest.raises(ValueError, match=OUT_OF_RANGE) as e:
            b.main.evaluate(bad)
        assert "both operands of a WORD column must be below 2^bits as canonical integers" in str(e.value)
        with pytest.raises(R.WordOutOfRange):
            R.main_table(b.main, bad)
    b.main.evaluate(rows)


# ---- check_trace: the integer model ------------------------------------------------------------------------------------------------
def test_check_trace_is_clean_on_valid_inputs_and_names_the_recomposition():
    n = 64
    rng = random.Random(6)
    b = air.limb_range_check(n, 4, 2)
    rows = air.limb_range_check_inputs(n, 4, 2, rng)
    table = air.limb_range_check_trace(rows, 4, 2)
    assert b.check_trace(rows, rap=[0x5eed]) == b.check_trace(table, rap=[0x5eed]) == []
    table[9][0] = (table[9][0] + 1) % P                                               # x of one row of the whole table
    report = b.check_trace(table, rap=[0x5eed])
    assert [(v.kind, v.index, v.first_row, v.last_row) for v in report] == [(air.TRANSITION, 0, 9, 9)], report
    bits = 8
    b = air.word_ops(n, bits)
    rows = air.word_ops_inputs(n, bits, rng)
    table = air.word_ops_trace(rows, bits)
    assert b.check_trace(rows) == b.check_trace(table) == []
    table[40][1] ^= 1                                                                 # y of one row: its recomposition is constraint 2 bits + 1
    report = b.check_trace(table)
    assert (air.TRANSITION, 2 * bits + 1, 40, 40) in [(v.kind, v.index, v.first_row, v.last_row) for v in report], report
    assert all(v.first_row == v.last_row == 40 for v in report)


# ---- the decoder and its mirror --------------------------------------------------------------------------------------------------
def builders():
    return (W.limb_group(), W.word_groups(64, 17), W.many_limbs(65), W.split_group(True)[0], W.split_group(False)[0], W.mixed(8), W.verdicts(),
            air.limb_range_check(256, 8, 2), air.word_ops(256, 16))


def test_the_helpers_and_the_examples_pass_the_decoder(hip_lib):
    for b in builders():
        desc, keep = b.build()
        assert air.needs_word(desc) and air.main_suffix(desc) == "word" and air.main_level(desc) == air.MainLevel.WORD
        assert check_with(hip_lib, "word", desc, 256) == _lib.SP_OK, hip_lib.sp_last_error()
        api.air_main_check(desc, 256)
        assert [air.route(desc, c)[0] for c in ("prove", "check_trace")] == ["sp_air_prove_word", "sp_air_check_trace_word"]
        assert not air.route(desc, "verify")[0].endswith("_word")
    # programs without a LIMB or WORD column go where they went, and the new decoder takes them too
    older = ((air.zero_count(N, 3), "main"), (air.bit_range_check(N, 20), "main"), (air.mimc_blocks(N, 8, [7] * 8, 0), "rec"), (air.xor_lookup(256, 4), "lk"),
             (air.mimc_sponge(N, 4, 2, [7] * 4, 0), "link"), (air.xor_fetch(256, 4), "fetch"), (air.rom_reads(256, 16), "fetch"))
    for b, suffix in older:
        desc, keep = b.build()
        assert not air.needs_word(desc) and air.main_suffix(desc) == suffix and air.route(desc, "prove")[0] == f"sp_air_prove_{suffix}"
        assert check_with(hip_lib, "word", desc, 256) == _lib.SP_OK, hip_lib.sp_last_error()
    # a descriptor put together by hand is looked through
    for b in (W.limb_group(), W.word_groups(8, 9)):
        desc, keep = b.build()
        del desc.main_features
        assert air.needs_word(desc) and air.route(desc, "prove")[0] == "sp_air_prove_word"


def _pad(k, low=None, high=None, extra=0):
    def mutate(m):
        kind, num_op, den_op, pad = m.cols[k]
        m.cols[k] = (kind, num_op, den_op, (pad & 255 if low is None else low) + 256 * ((pad >> 8) & 255 if high is None else high) + extra)
    return mutate


def two_builder():
    """Inputs x and y; derived column 0 is the LIMB (x >> 8) mod 2^16, derived column 1 the WORD x XOR y over 32 bits, derived column 2 a
    VALUE that reads both."""
    b = air.AirBuilder(5, [0], 1, main_inputs=2)
    m = b.main
    limb = m.limb(m.load(0, 0), 8, 16)
    word = m.word_xor(m.load(0, 0), m.load(0, 1), 32)
    m.value(m.load(0, limb) + m.load(0, word))
    return W.trivial(b)


def _behind_a_quotient(k, field):
    def mutate(m):
        m.ops.append((air.OP_DIV, 0, 0))
        _col(k, **{field: len(m.ops) - 1})(m)
    return mutate


QUOTIENT = "depends on a quotient (op 7), which only the seed or the step of a CHAIN column may"
REFUSALS = [
    ("limb-pad-bit-16", _pad(0, extra=1 << 16), "derived column 0 is a LIMB column whose pad has a bit at or above 16 (pad = lo + 256 width)"),
    ("limb-pad-bit-31", _pad(0, extra=1 << 31), "derived column 0 is a LIMB column whose pad has a bit at or above 16"),
    ("word-pad-bit-16", _pad(1, extra=1 << 16), "derived column 1 is a WORD column whose pad has a bit at or above 16 (pad = fn + 256 bits)"),
    ("limb-width-0", _pad(0, high=0), "derived column 0 is a LIMB column with width = 0"),
    ("limb-end-253", _pad(0, low=200, high=53), "derived column 0 is a LIMB column with lo + width = 253"),
    ("limb-lo-252", _pad(0, low=252, high=1), "derived column 0 is a LIMB column with lo + width = 253"),
    ("limb-with-a-denominator", _col(0, den_op=0), "derived column 0 is a LIMB column and takes no denominator"),
    ("word-without-a-second-operand", _col(1, den_op=air.AUX_NO_DEN), "derived column 1 is a WORD column without a second operand"),
    ("word-fn-3", _pad(1, low=3), "derived column 1 is a WORD column with fn = 3"),
    ("word-bits-0", _pad(1, high=0), "derived column 1 is a WORD column with bits = 0"),
    ("word-bits-252", _pad(1, high=252), "derived column 1 is a WORD column with bits = 252"),
    ("limb-op-beyond-the-program", _col(0, num_op=60000), "derived column 0 names an op beyond the program"),
    ("word-x-beyond-the-program", _col(1, num_op=60000), "derived column 1 names an op beyond the program"),
    ("word-y-beyond-the-program", _col(1, den_op=60000), "derived column 1 names an op beyond the program"),
    ("limb-reads-itself", _op(lambda o: o == (air.OP_LOAD, 0, 0), b=2), "derived column 0 reads derived column 0, which is not an earlier one"),
    ("word-reads-a-later-column", _op(lambda o: o == (air.OP_LOAD, 0, 1), b=4), "derived column 1 reads derived column 2, which is not an earlier one"),
    ("limb-behind-a-quotient", _behind_a_quotient(0, "num_op"), "derived column 0 " + QUOTIENT),
    ("word-y-behind-a-quotient", _behind_a_quotient(1, "den_op"), "derived column 1 " + QUOTIENT),
    ("kind-10", _col(2, kind=10), "derived column 2 has an unknown kind"),
]


@pytest.mark.parametrize("mutate,says", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_decoder_refuses_and_the_builder_raises(hip_lib, mutate, says):
    decoder_refuses_and_the_builder_raises(hip_lib, "word", two_builder, mutate, says, N)


def test_the_edges_of_the_ranges_are_accepted(hip_lib):
    for mutate in (_pad(0, low=251, high=1), _pad(0, low=0, high=252), _pad(0, low=0, high=1), _pad(1, low=0, high=1), _pad(1, low=2, high=251)):
        b = two_builder()
        mutate(b.main)
        b.main.check(N)
        desc, keep = b.build()
        assert check_with(hip_lib, "word", desc, N) == _lib.SP_OK, hip_lib.sp_last_error()


def test_the_older_entry_points_call_kinds_8_and_9_unknown(hip_lib):
    for b, k in ((W.limb_group(), 0), (W.word_groups(8, 9), 0), (air.word_ops(N, 2), 4), (air.limb_range_check(N, 4, 2), 0)):
        desc, keep = b.build()
        says = f"derived column {k} has an unknown kind"
        for suffix in ("fetch", "div", "link", "lk", "rec", ""):
            if suffix == "" and any(op == air.OP_PERIODIC for op, _, _ in b.main.ops):
                continue                                               # (sp_air_main_check calls the op 6 in front of it malformed)
            assert check_with(hip_lib, suffix, desc, N) == INVALID, suffix
            message = hip_lib.sp_last_error().decode()
            entry = f"sp_air_main_check_{suffix}" if suffix else "sp_air_main_check"
            assert says in message and message.startswith(f"{entry}: main program: "), message
        # the mirror follows the decoder the program would be routed to: without the builder's declaration, or at the level below, kinds
        # 8 and 9 are unknown
        with pytest.raises(ValueError, match=says):
            b.main.check(N, level=air.MainLevel.FETCH)
        b.main.check(N)
        b.main.level = air.MainLevel.FETCH
        with pytest.raises(ValueError, match=says):
            b.main.check(N)
        b.main.check(N, level=air.MainLevel.WORD)


def test_null_arguments(hip_lib):
    desc, keep = W.limb_group().build()
    n = ctypes.c_uint64(N)
    assert hip_lib.sp_air_main_check_word(None, None, ctypes.byref(desc.main_desc), n) == INVALID
    assert hip_lib.sp_air_main_check_word(ctypes.byref(desc), None, None, n) == INVALID
    assert hip_lib.sp_air_prove_word(None, None, None, None, None, None, n, None, None, None) == INVALID
    assert hip_lib.sp_air_check_trace_word(None, None, None, None, None, None, n, None, None, None, 0, None) == INVALID
    assert hip_lib.sp_air_main_trace_word(None, None, None, None, None, n, None) == INVALID
    assert hip_lib.sp_air_main_check_word(ctypes.byref(desc), None, ctypes.byref(desc.main_desc), n) == _lib.SP_OK     # no op 6: no ext needed


def test_builder_arguments():
    m = air.AirBuilder(8, [0], 1, main_inputs=2).main
    x, y = m.load(0, 0), m.load(0, 1)
    for lo, width in ((0, 0), (-1, 4), (252, 1), (200, 53)):
        with pytest.raises(ValueError, match="a limb of"):
            m.limb(x, lo, width)
    with pytest.raises(ValueError, match="limbs of 64 bits"):
        m.limbs(x, 64, 4)
    for bits in (0, 252):
        with pytest.raises(ValueError, match=f"words of {bits} bits"):
            m.word_and(x, y, bits)
    with pytest.raises(ValueError, match="needs two operands"):
        m.word_or(x, None, 8)
    assert not m.words and not m.cols and m.level == air.MainLevel.REC
    cols = m.limbs(x, 16, 3)
    assert cols == [2, 3, 4] and [m.cols[j] for j in range(3)] == [(air.MAIN_LIMB, x.i, air.AUX_NO_DEN, 16 * j + 256 * 16) for j in range(3)] and m.words
    got = [m.word_and(x, y, 251), m.word_or(x, y, 1), m.word_xor(x, y, 64)]
    assert got == [5, 6, 7] and [m.cols[3 + j][3] for j in range(3)] == [air.WORD_AND + 256 * 251, air.WORD_OR + 256, air.WORD_XOR + 256 * 64]
    assert all(c[:3] == (air.MAIN_WORD, x.i, y.i) for c in m.cols[3:])
    with pytest.raises(ValueError, match="limb_range_check"):
        air.limb_range_check(64, 8, 2)                                                # 256 table entries on 64 rows
    with pytest.raises(ValueError, match="word_ops"):
        air.word_ops(64, 17)
