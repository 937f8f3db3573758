"""Integer ops in chain steps (ops 8 .. 11, the _int entry points) without a GPU: the new symbols in the header, the binding and the Rust
block, MainLevel.INT, the routing, the decoder's verdicts through sp_air_main_check_int - and the _word entry point's on the same
descriptors -, the builder's mirror of them, and the Python-integer model (MainProgram.evaluate, AirBuilder.check_trace) against the plain
reference of int_chain_ref and the worked example's own table."""
import ctypes
import os
import random
import re

import pytest

import int_chain_programs as G
import int_chain_ref as R
import program_ref
from air_main_checks import _col, _op, check_with, decoder_refuses_and_the_builder_raises
from lambdaworks_cairo_prover_amd import _lib, air, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = air.P
N = 64
NEW_SYMBOLS = ("sp_air_prove_int", "sp_air_check_trace_int", "sp_air_main_trace_int", "sp_air_main_check_int", "sp_air_main_int_limits")
INVALID = _lib.SP_E_INVALID_ARG
OUT_OF_RANGE = "an integer op's operand is out of range on some row"


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
    codes = {"LIMB": air.OP_INT_LIMB, "AND": air.OP_INT_AND, "OR": air.OP_INT_OR, "XOR": air.OP_INT_XOR}
    for k, (name, code) in enumerate(codes.items()):
        assert int(re.search(rf"#define SP_AIR_OP_{name}\s+(\d+)", header).group(1)) == 8 + k == code, name
    assert ctypes.sizeof(air.AirOpC) == 8           # sp_air_op stays (op, a, b): the LIMB's immediate rides in b


def test_the_limits_call(hip_lib):
    assert api.air_main_int_limits() == {"limb_end": 252, "bits": 251, "ops": 4} == {"limb_end": air.MAIN_LIMB_MAX_END, "bits": air.INT_OP_BITS, "ops": len(air._INT_OPS)}
    out = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    assert hip_lib.sp_air_main_int_limits(out) == _lib.SP_OK and list(out) == [252, 251, 4, 0]
    assert hip_lib.sp_air_main_int_limits(None) == INVALID
    assert (1 << air.INT_OP_BITS) < P and 251 + 256 * 252 < 1 << 16          # every result is canonical; every immediate fits b


def test_the_int_level_stands_above_word_and_the_worked_example_is_routed_to_it(hip_lib):
    level = air.MainLevel.INT
    assert (int(level), level.suffix) == (7, "int") and level is air.MainLevelInt.INT and level not in list(air.MainLevel)
    assert len(list(air.MainLevel)) == 6 and (int(air.MainLevel.WORD), air.MainLevel.WORD.suffix) == (6, "word")
    assert level > air.MainLevel.WORD and all(level > x for x in air.MainLevel) and max(list(air.MainLevel) + [air.MainLevel.WORD, level]) is level
    b, rows, keys, digest = G.arx_case(N, 8, random.Random(6))
    desc, keep = b.build()
    assert air.main_level(desc) == level and air.needs_int(desc) and air.needs_word(desc) and air.needs_rec(desc)
    assert [air.route(desc, c)[0] for c in ("prove", "check_trace")] == ["sp_air_prove_int", "sp_air_check_trace_int"]
    assert not air.route(desc, "verify")[0].endswith("_int")
    assert check_with(hip_lib, "int", desc, N) == _lib.SP_OK, hip_lib.sp_last_error()
    api.air_main_check(desc, N)
    assert (b.main_cols, desc.n_transitions) == (38, 55)
    # a descriptor put together by hand is looked through
    del desc.main_features
    assert air.needs_int(desc) and air.route(desc, "prove")[0] == "sp_air_prove_int"


def test_programs_without_the_ops_go_where_they_went_and_the_new_decoder_takes_them(hip_lib):
    older = ((air.zero_count(N, 3), "main"), (air.bit_range_check(N, 20), "main"), (air.mimc_blocks(N, 8, [7] * 8, 0), "rec"), (air.xor_lookup(256, 4), "lk"),
             (air.mimc_sponge(N, 4, 2, [7] * 4, 0), "link"), (air.xor_fetch(256, 4), "fetch"), (air.rom_reads(256, 16), "fetch"), (air.word_ops(256, 8), "word"),
             (air.limb_range_check(256, 8, 2), "word"))
    for b, suffix in older:
        desc, keep = b.build()
        assert not air.needs_int(desc) and air.main_suffix(desc) == suffix and air.route(desc, "prove")[0] == f"sp_air_prove_{suffix}"
        assert check_with(hip_lib, "int", desc, 256) == _lib.SP_OK, hip_lib.sp_last_error()
    import div_airs
    desc, keep = div_airs.plain_div(8).build()
    assert air.main_suffix(desc) == "div" and check_with(hip_lib, "int", desc, N) == _lib.SP_OK


# ---- the model against the plain reference --------------------------------------------------------------------------------------
def _case(seed, n):
    rng = random.Random(seed * 7 + n)
    periodic = G.periodic_columns(rng) if seed % 2 and n >= G.K2_PERIOD else None
    b = G.group(seed, 4 if n == 8 else 8, 2 if seed % 3 == 0 else 1, periodic, div=seed % 4 >= 2)
    return b, rng


@pytest.mark.parametrize("n", [8, 64, 256])
def test_model_equals_the_plain_reference(n):
    widths, ops, edges = set(), set(), set()
    for seed in G.SEEDS:
        b, rng = _case(seed, n)
        rows, want = G.inputs(b, n, rng)
        got = ints(b.main.evaluate(rows))
        for i in range(n):
            assert got[i] == want[i], (seed, i)
        widths.add(len(b.main.cols) - 1)
        ops |= {o[0] for o in b.main.ops}
        edges |= {(o[2] & 255, o[2] >> 8) for o in b.main.ops if o[0] == air.OP_INT_LIMB}
        assert b.main.level == air.MainLevel.INT
    assert widths == set(range(1, 17)) and ops >= {air.OP_DIV, air.OP_INT_LIMB, air.OP_INT_AND, air.OP_INT_OR, air.OP_INT_XOR} and edges >= set(G.EDGES)
    assert (air.OP_PERIODIC in ops) == (n >= G.K2_PERIOD)


def test_the_seeded_programs_pass_the_decoder_and_the_word_decoder_calls_their_ops_malformed(hip_lib):
    for seed in G.SEEDS:
        b, rng = _case(seed, N)
        desc, keep = b.build()
        assert air.main_suffix(desc) == "int" and check_with(hip_lib, "int", desc, N) == _lib.SP_OK, hip_lib.sp_last_error()
        first = next(t for t, o in enumerate(b.main.ops) if o[0] in air._INT_OPS)
        for suffix in ("word", "fetch", "div"):
            assert check_with(hip_lib, suffix, desc, N) == INVALID, (seed, suffix)
            message = hip_lib.sp_last_error().decode()
            assert message.startswith(f"sp_air_main_check_{suffix}: main program: malformed op {first} "), message
        with pytest.raises(ValueError, match=f"malformed op {first} "):
            b.main.check(N, level=air.MainLevel.WORD)
        b.main.check(N)


def test_each_op_alone_is_malformed_for_the_word_decoder(hip_lib):
    for op in air._INT_OPS:
        b = G.plain_int(8)
        desc, keep = b.build()
        m = b.main
        m.ops = [(op, 0, 1 + 256 if op == air.OP_INT_LIMB else 1) if o[0] in air._INT_OPS else o for o in m.ops]
        kept = next(t for t, o in enumerate(m.ops) if o[0] == op)
        desc.main_desc, keep2 = air.main_desc(m.input_cols, m.ops, m.consts, m.cols)
        assert check_with(hip_lib, "word", desc, N) == INVALID and f"malformed op {kept} " in hip_lib.sp_last_error().decode(), op


def test_the_worked_example_is_the_reference_and_its_cells_are_what_they_claim():
    n, s, bits = 64, 8, 16
    b, rows, keys, digest = G.arx_case(n, s, random.Random(3))
    table = air.arx_chain_trace(rows, s, keys)
    assert table == R.main_table(b.main, rows) == ints(b.main.evaluate(rows))
    assert rows[0] == [65535, 65535] and rows[s] == [0, 0] and table[s - 1][2] == digest
    mask = (1 << bits) - 1
    for i, r in enumerate(table):
        x, y = r[2], r[3]
        assert x == sum(bit << j for j, bit in enumerate(r[4:4 + bits])) and y == sum(bit << j for j, bit in enumerate(r[4 + bits:4 + 2 * bits]))
        if i % s == 0:
            assert (x, y) == (r[0], r[1])
        if i % s != s - 1:
            total = (((x >> 7) | (x << 9)) & mask) + y + keys[i % s]
            assert table[i + 1][2] == total & mask and r[-2] + 2 * r[-1] == total >> bits
            assert table[i + 1][3] == (((y << 2) | (y >> 14)) & mask) ^ table[i + 1][2]
    # other widths and rotations
    for bits, alpha, beta in ((8, 3, 5), (5, 1, 4)):
        rng = random.Random(bits)
        keys = [rng.randrange(1 << bits) for _ in range(s)]
        rows = air.arx_chain_inputs(n, s, rng, bits)
        b = air.arx_chain(n, s, keys, air.arx_chain_digest(rows[0], s, keys, bits, alpha, beta), bits, alpha, beta)
        table = air.arx_chain_trace(rows, s, keys, bits, alpha, beta)
        assert table == R.main_table(b.main, rows) == ints(b.main.evaluate(rows)) and b.check_trace(rows) == []


def test_check_trace_is_clean_on_the_example_and_names_a_flipped_carry():
    n, s, bits = 64, 8, 16
    b, rows, keys, digest = G.arx_case(n, s, random.Random(5))
    table = air.arx_chain_trace(rows, s, keys)
    assert b.check_trace(rows) == b.check_trace(table) == []
    c0 = 4 + 2 * bits
    row = next(i for i in range(n) if i % s != s - 1)
    table[row][c0] ^= 1                                                               # carry bit 0 of one row inside a block
    report = [(v.kind, v.index, v.first_row, v.last_row) for v in b.check_trace(table)]
    assert report == [(air.TRANSITION, 2 * bits + 2 + 2, row, row)], report          # the addition: behind 2 bits + 2 bit-ness and 2 recompositions
    wrong = G.arx_case(n, s, random.Random(5), wrong=1)[0]
    assert wrong.check_trace(rows) == [air.Violation(air.BOUNDARY, 0, 1, s - 1, s - 1, digest)]


def test_evaluate_and_the_reference_refuse_the_same_rows():
    n, s = 32, 8
    b = G.range_case(s)
    rng = random.Random(4)
    rows = [[rng.randrange(1 << 250)] for _ in range(n)]
    assert ints(b.main.evaluate(rows)) == R.main_table(b.main, rows)
    for value in (1 << 251, P - 1):
        bad = [list(r) for r in rows]
        bad[s + 3] = [value]                         # read by the step of row s + 2 alone
        with pytest.raises(ValueError, match=OUT_OF_RANGE) as e:
            b.main.evaluate(bad)
        assert "both operands of an AND, OR or XOR op must be below 2^251 as canonical integers" in str(e.value)
        with pytest.raises(program_ref.WordOutOfRange):
            R.main_table(b.main, bad)
        bad[2 * s] = [7]                             # and a zero denominator in the same program: the reference reports the range
        with pytest.raises(program_ref.WordOutOfRange):
            R.main_table(b.main, bad)
    bad = [list(r) for r in rows]
    bad[2 * s] = [7]
    with pytest.raises(program_ref.ZeroDenominator):
        R.main_table(b.main, bad)
    with pytest.raises(ValueError, match="quotient"):
        b.main.evaluate(bad)
    quiet = [list(r) for r in rows]
    quiet[s] = [(1 << 251) - 1]                      # a block's first row: the seed's limb reads it, no AND does
    assert ints(b.main.evaluate(quiet)) == R.main_table(b.main, quiet)


# ---- the decoder and its mirror --------------------------------------------------------------------------------------------------
def refusal_builder():
    """Inputs x and y and a table key; a one-column chain group whose step holds one op of each kind - LIMB(x, 8, 16), AND, OR, XOR -;
    then derived columns 1 .. 6: a VALUE, a BIT, a COUNT, a FETCH, a LIMB and a WORD over the inputs."""
    b = air.AirBuilder(10, [0], 1, main_inputs=3)
    m = b.main
    x, y, t = m.load(0, 0), m.load(0, 1), m.load(0, 2)
    g = m.chain(8, [x])
    limb = m.int_limb(g.state(0), 8, 16)
    g.step([m.int_xor(m.int_or(m.int_and(limb, y), x), y)])
    m.value(x + y)
    m.bit(x, 3)
    m.multiplicity(t, t, 16)
    m.fetch(t, t, y, 16)
    m.limb(x, 4, 8)
    m.word_xor(t, t, 16)
    v = b.load(0, 0)
    b.constraint(v - v, degree=1, exemptions=0)
    return b


def _limb_op(**fields):
    return _op(lambda o: o[0] == air.OP_INT_LIMB, **fields)


def _behind_an_integer_op(k, field):
    def mutate(m):
        m.ops.append((air.OP_INT_XOR, 0, 1))
        _col(k, **{field: len(m.ops) - 1})(m)
    return mutate


def _fetch_value_behind_an_integer_op(k):
    def mutate(m):
        m.ops.append((air.OP_INT_LIMB, 1, 256))
        kind, num_op, den_op, pad = m.cols[k]
        m.cols[k] = (kind, num_op, den_op, (pad & 255) + 256 * (len(m.ops) - 1))
    return mutate


INTEGER = "depends on an integer op (ops 8 .. 11), which only the seed or the step of a CHAIN column may: a row-local limb or word is a LIMB or WORD column"
REFUSALS = [
    ("limb-op-width-0", _limb_op(b=8), " is a LIMB op with width = 0"),
    ("limb-op-end-253", _limb_op(b=200 + 256 * 53), " is a LIMB op with lo + width = 253"),
    ("limb-op-lo-252", _limb_op(b=252 + 256), " is a LIMB op with lo + width = 253"),
    ("limb-op-a-not-earlier", _limb_op(a=60000), " is an integer op (op 8) whose operands are not earlier values"),
    ("limb-op-a-is-itself", lambda m: _limb_op(a=next(t for t, o in enumerate(m.ops) if o[0] == air.OP_INT_LIMB))(m), " is an integer op (op 8) whose operands are not earlier values"),
    ("and-op-b-not-earlier", _op(lambda o: o[0] == air.OP_INT_AND, b=60000), " is an integer op (op 9) whose operands are not earlier values"),
    ("value-behind-an-integer-op", _behind_an_integer_op(1, "num_op"), "derived column 1 " + INTEGER),
    ("bit-behind-an-integer-op", _behind_an_integer_op(2, "num_op"), "derived column 2 " + INTEGER),
    ("count-table-behind-an-integer-op", _behind_an_integer_op(3, "den_op"), "derived column 3 " + INTEGER),
    ("fetch-key-behind-an-integer-op", _behind_an_integer_op(4, "num_op"), "derived column 4 " + INTEGER),
    ("fetch-value-behind-an-integer-op", _fetch_value_behind_an_integer_op(4), "derived column 4 " + INTEGER),
    ("limb-behind-an-integer-op", _behind_an_integer_op(5, "num_op"), "derived column 5 " + INTEGER),
    ("word-y-behind-an-integer-op", _behind_an_integer_op(6, "den_op"), "derived column 6 " + INTEGER),
]


@pytest.mark.parametrize("mutate,says", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_decoder_refuses_and_the_builder_raises(hip_lib, mutate, says):
    decoder_refuses_and_the_builder_raises(hip_lib, "int", refusal_builder, mutate, says, N)


def test_the_quotient_refusal_keeps_its_words_and_comes_first(hip_lib):
    def mutate(m):
        m.ops.append((air.OP_DIV, 0, 1))
        m.ops.append((air.OP_INT_LIMB, len(m.ops) - 1, 256))
        _col(1, num_op=len(m.ops) - 1)(m)
    says = ("derived column 1 depends on a quotient (op 7), which only the seed or the step of a CHAIN column may: a row-local quotient is a VALUE "
            "column's N / D")
    decoder_refuses_and_the_builder_raises(hip_lib, "int", refusal_builder, mutate, says, N)


def test_the_edges_of_the_ranges_are_accepted(hip_lib):
    for lo, width in G.EDGES + [(251, 1), (0, 252), (0, 1)]:
        b = refusal_builder()
        _limb_op(b=lo + 256 * width)(b.main)
        b.main.check(N)
        desc, keep = b.build()
        assert check_with(hip_lib, "int", desc, N) == _lib.SP_OK, hip_lib.sp_last_error()


def test_null_arguments(hip_lib):
    desc, keep = G.plain_int(8).build()
    n = ctypes.c_uint64(N)
    assert hip_lib.sp_air_main_check_int(None, None, ctypes.byref(desc.main_desc), n) == INVALID
    assert hip_lib.sp_air_main_check_int(ctypes.byref(desc), None, None, n) == INVALID
    assert hip_lib.sp_air_prove_int(None, None, None, None, None, None, n, None, None, None) == INVALID
    assert hip_lib.sp_air_check_trace_int(None, None, None, None, None, None, n, None, None, None, 0, None) == INVALID
    assert hip_lib.sp_air_main_trace_int(None, None, None, None, None, n, None) == INVALID
    assert hip_lib.sp_air_main_check_int(ctypes.byref(desc), None, ctypes.byref(desc.main_desc), n) == _lib.SP_OK     # no op 6: no ext needed


def test_builder_arguments():
    m = air.AirBuilder(8, [0], 1, main_inputs=2).main
    x, y = m.load(0, 0), m.load(0, 1)
    for lo, width in ((0, 0), (-1, 4), (252, 1), (200, 53)):
        with pytest.raises(ValueError, match="a limb of"):
            m.int_limb(x, lo, width)
    other = air.AirBuilder(8, [0], 1, main_inputs=2).main
    with pytest.raises(ValueError, match="values of this program"):
        m.int_and(x, other.load(0, 0))
    assert not m.ints and m.level == air.MainLevel.REC
    v = m.int_limb(x, 251, 1)
    assert m.ops[v.i] == (air.OP_INT_LIMB, x.i, 251 + 256) and m.ints and m.level == air.MainLevel.INT
    got = [m.int_and(x, y), m.int_or(x, y), m.int_xor(x, 5)]
    assert [m.ops[g.i][0] for g in got] == [9, 10, 11] and m.ops[got[0].i] == (9, x.i, y.i) and m.ops[m.ops[got[2].i][2]][0] == air.OP_CONST
    # the compositions: a rotation is two limbs, an addition one
    before = len(m.ops)
    r = m.int_rotl(x, 3, 16)
    assert [o for o in m.ops[before:] if o[0] == air.OP_INT_LIMB] == [(8, x.i, 0 + 256 * 13), (8, x.i, 13 + 256 * 3)] and m.ops[r.i][0] == air.OP_ADD
    before = len(m.ops)
    m.int_rotr(x, 3, 16)
    assert [o for o in m.ops[before:] if o[0] == air.OP_INT_LIMB] == [(8, x.i, 0 + 256 * 3), (8, x.i, 3 + 256 * 13)]
    s = m.int_add(x, y, 32)
    assert m.ops[s.i] == (8, s.i - 1, 256 * 32) and m.ops[s.i - 1] == (air.OP_ADD, x.i, y.i)
    assert m.ops[m.int_rotl(x, 16, 16).i] == (8, x.i, 256 * 16)
    for args in ((64, 3, [1, 2, 3], 0), (64, 8, [1 << 16] * 8, 0)):
        with pytest.raises(ValueError, match="arx_chain"):
            air.arx_chain(*args)
    with pytest.raises(ValueError, match="arx_chain"):
        air.arx_chain(64, 8, [1] * 8, 0, bits=17)
