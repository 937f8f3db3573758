"""Looked-up values in a main program (SP_AIR_MAIN_FETCH, the _fetch entry points) without a GPU: the new symbols in the header, the
binding and the Rust block, the decoder's verdicts through sp_air_main_check_fetch - and the older entry points' on the same descriptors
-, the builder's mirror of them, and the Python-integer model (MainProgram.evaluate, AirBuilder.check_trace) against the plain
reference of program_ref and the worked examples' own tables."""
import ctypes
import os
import random
import re

import pytest

import fetch_airs as F
import program_ref as R
from air_main_checks import _col, _op, check_with, decoder_refuses_and_the_builder_raises
from lambdaworks_cairo_prover_amd import _lib, air, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = air.P
N = 64
NEW_SYMBOLS = ("sp_air_prove_fetch", "sp_air_check_trace_fetch", "sp_air_main_trace_fetch", "sp_air_main_check_fetch", "sp_air_main_fetch_limits")
INVALID = _lib.SP_E_INVALID_ARG


def test_symbols_are_declared_everywhere_and_the_abi_is_7(hip_lib):
    header = open(os.path.join(ROOT, "include", "stark252_hip.h")).read()
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = integ.index("```rust")
    rust = set(re.findall(r"pub fn (sp_[a-z0-9_]+)\s*\(", integ[start:integ.index("```\n", start + 10)]))
    for name in NEW_SYMBOLS:
        assert name in declared and name in rust and name in _lib.NEWEST_SYMBOLS and hasattr(hip_lib, name), name
    assert int(re.search(r"#define SP_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.SP_ABI_VERSION == hip_lib.sp_abi_version() == 7
    assert int(re.search(r"#define SP_AIR_MAIN_FETCH\s+(\d+)", header).group(1)) == 7 == air.MAIN_FETCH == air.SP_AIR_MAIN_FETCH
    hip_lib.sp_air_main_desc_size.restype = ctypes.c_uint64
    assert hip_lib.sp_air_main_desc_size() == ctypes.sizeof(air.AirMainDescC) == 64 and ctypes.sizeof(air.AirMainColumnC) == 16


def test_the_limits_call(hip_lib):
    want = {"key_bits": air.MAIN_FETCH_MAX_KEY_BITS, "group": air.MAIN_FETCH_MAX_GROUP, "columns": air.MAIN_FETCH_MAX_COLS}
    assert api.air_main_fetch_limits() == {"key_bits": 64, "group": 16, "columns": 64} == want
    assert hip_lib.sp_air_main_fetch_limits(None) == INVALID


# ---- the model against the plain reference --------------------------------------------------------------------------------------
def _periodic_case(w, key_bits):
    def make(n, rng):
        keys, values = F.periodic_table(8, w, key_bits, rng)
        held = sorted(set(keys))
        return F.periodic_fetch(keys, values, key_bits), [[rng.choice(keys) if i > 1 else held[-i]] for i in range(n)]
    return make


def _input_case(build, key_bits):
    return lambda n, rng: (build(), F.input_rows(n, key_bits, rng))


# (seed, what it covers, (n, rng) -> (builder, input rows))
SEEDED = [
    (11, "a run of one, a periodic table with a duplicate key", _periodic_case(1, 9)),
    (12, "a run of two, a periodic table, one key bit", _periodic_case(2, 1)),
    (13, "a run of sixteen, a periodic table, 64 key bits", _periodic_case(16, 64)),
    (14, "a run of one, the table in input columns, duplicate keys with different values", _input_case(lambda: F.input_fetch(1), 64)),
    (15, "a run of two, the table in input columns, 8 key bits", _input_case(lambda: F.input_fetch(2, 8), 8)),
    (16, "a run of sixteen, the table in input columns", _input_case(lambda: F.input_fetch(16), 64)),
    (17, "a FETCH that reads a chain column at a wrapping shift", _input_case(lambda: F.chain_fetch(4), 64)),
    (18, "a COUNT and a FETCH on one table", _input_case(lambda: F.count_and_fetch(8), 8)),
    (19, "a FETCH, a chain group that reads it, a COUNT and a second FETCH", _input_case(lambda: F.mixed(4), 64)),
    (20, "sixteen columns in two runs around a VALUE", _input_case(lambda: F.separated(16)[0], 64)),
]


@pytest.mark.parametrize("n", [8, 64, 256])
@pytest.mark.parametrize("seed,make", [(c[0], c[2]) for c in SEEDED], ids=[str(c[0]) for c in SEEDED])
def test_model_equals_the_plain_reference(n, seed, make):
    b, rows = make(n, random.Random(1000 * seed + n))
    want = R.main_table(b.main, rows)                     # (raises on the chosen inputs if they hold a key out of range or a missing one)
    got = [[int(x) for x in r] for r in b.main.evaluate(rows)]
    for i in range(n):
        assert got[i] == want[i], i
    assert any(c[0] == air.MAIN_FETCH for c in b.main.cols)


def test_the_chosen_inputs_hold_what_they_claim():
    rows = F.input_rows(64, 64, random.Random(14064))
    t = [r[1] for r in rows]
    values_of = {}
    for r in rows:
        values_of.setdefault(r[1], set()).add(r[2])
    assert len(set(t)) < 64 and any(len(v) > 1 for v in values_of.values())          # duplicate keys with different values
    assert rows[0][0] == min(t) == 0 and rows[-1][0] == max(t) == (1 << 64) - 1       # the smallest and the largest key are looked up
    first = {}
    for j, key in enumerate(t):
        first.setdefault(key, j)
    table = R.main_table(F.input_fetch(1).main, rows)
    assert all(table[i][3] == rows[first[rows[i][0]]][2] for i in range(64))          # the lowest row wins
    b = F.chain_fetch(4)
    assert any(op == air.OP_LOAD and a == 1 and col == 3 for op, a, col in b.main.ops)


def test_evaluate_and_the_reference_refuse_the_same_rows():
    b = F.input_fetch(2, 8)
    rows = F.input_rows(16, 8, random.Random(4))
    absent = next(v for v in range(256) if v not in {r[1] for r in rows})
    for col, value, words, error in ((0, absent, "a fetched key is in no table row", R.MissingKey), (0, 256, "a lookup key is out of range on some row", R.KeyOutOfRange),
                                     (1, 256, "a lookup key is out of range on some row", R.KeyOutOfRange)):
        bad = [list(r) for r in rows]
        bad[5][col] = value
        with pytest.raises(ValueError, match=words):
            b.main.evaluate(bad)
        with pytest.raises(error):
            R.main_table(b.main, bad)
    both = [list(r) for r in rows]
    both[5][0], both[6][0] = absent, 300                                              # out of range and missing: the range is reported
    with pytest.raises(ValueError, match="a lookup key is out of range on some row"):
        b.main.evaluate(both)
    with pytest.raises(R.KeyOutOfRange):
        R.main_table(b.main, both)


# ---- the worked examples -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 1024])
def test_xor_fetch_builds_the_trace_of_xor_lookup(n):
    bits = 4
    b, whole = air.xor_fetch(n, bits), air.xor_lookup(n, bits)
    rows, rows3 = air.xor_fetch_inputs(n, bits, random.Random(n)), air.xor_lookup_inputs(n, bits, random.Random(n))
    assert [r[:2] for r in rows3] == rows and b.main.input_cols == 2 and whole.main.input_cols == 3
    got = [[int(x) for x in r] for r in b.main.evaluate(rows)]
    assert got == [[int(x) for x in r] for r in whole.main.evaluate(rows3)] == R.main_table(b.main, rows)
    assert all(r[2] == r[0] ^ r[1] for r in got)
    # the statement is xor_lookup's: the same constraint program, boundary and auxiliary program over the same columns
    assert (b.ops, b.consts, b.bcs, b.degrees, b.aux.ops, b.aux.cols) == (whole.ops, whole.consts, whole.bcs, whole.degrees, whole.aux.ops, whole.aux.cols)
    assert b.periodic_cols[0] == whole.periodic_cols[0]
    assert b.check_trace(rows, rap=[0x5eed]) == whole.check_trace(rows3, rap=[0x5eed]) == []


def test_rom_reads_is_clean_and_a_tampered_value_is_reported():
    n, rap = 64, [0x5eed, 0xfeed]
    b = air.rom_reads(n, 16)
    rows = air.rom_reads_inputs(n, 16, random.Random(8))
    assert len({r[0] for r in rows}) == n                                             # the written addresses are distinct
    table = air.rom_reads_trace(rows)
    assert [[int(x) for x in r] for r in b.main.evaluate(rows)] == table == R.main_table(b.main, rows)
    assert sum(r[4] for r in table) == n and any(r[4] > 1 for r in table) and any(r[4] == 0 for r in table)
    assert b.check_trace(rows, rap=rap) == b.check_trace(table, rap=rap) == []
    table[9][3] = (table[9][3] + 1) % P                                               # val_r of one read
    report = b.check_trace(table, rap=rap)
    assert [(v.kind, v.index, v.first_row, v.last_row) for v in report] == [(air.TRANSITION, 0, n - 1, n - 1)], report


# ---- the decoder and its mirror --------------------------------------------------------------------------------------------------
def builders():
    rng = random.Random(2)
    keys, values = F.periodic_table(8, 2, 9, rng)
    return (F.periodic_fetch(keys, values, 9), F.input_fetch(1), F.input_fetch(16, 8), F.chain_fetch(4), F.count_and_fetch(), F.mixed(8), F.separated(16)[0],
            F.zero_den_beside_a_fetch(), air.xor_fetch(256, 4), air.rom_reads(256, 16))


def test_the_helpers_and_the_examples_pass_the_decoder(hip_lib):
    for b in builders():
        desc, keep = b.build()
        assert air.needs_fetch(desc) and air.main_suffix(desc) == "fetch"
        assert check_with(hip_lib, "fetch", desc, 256) == _lib.SP_OK, hip_lib.sp_last_error()
        api.air_main_check(desc, 256)
        assert [air.route(desc, c)[0] for c in ("prove", "check_trace")] == ["sp_air_prove_fetch", "sp_air_check_trace_fetch"]
        assert not air.route(desc, "verify")[0].endswith("_fetch")
    # programs without a FETCH column go where they went, and the new decoder takes them too
    for b, suffix in ((air.zero_count(N, 3), "main"), (air.mimc_blocks(N, 8, [7] * 8, 0), "rec"), (air.xor_lookup(256, 4), "lk")):
        desc, keep = b.build()
        assert not air.needs_fetch(desc) and air.main_suffix(desc) == suffix and check_with(hip_lib, "fetch", desc, 256) == _lib.SP_OK
    # a descriptor put together by hand is looked through
    desc, keep = F.input_fetch(1).build()
    del desc.main_features
    assert air.needs_fetch(desc)


def _pad(k, key_bits=None, v_op=None, high=0):
    def mutate(m):
        kind, num_op, den_op, pad = m.cols[k]
        bits = pad & 255 if key_bits is None else key_bits
        v = (pad >> 8) & 65535 if v_op is None else v_op
        m.cols[k] = (kind, num_op, den_op, bits + 256 * v + high)
    return mutate


def two_builder():
    """count_and_fetch: inputs 0 - 2, the COUNT is derived column 0, the FETCH derived column 1, the VALUE derived column 2."""
    return F.count_and_fetch()


def sixty_four_builder():
    """Sixty-four FETCH columns in four runs and a VALUE behind them."""
    b = air.AirBuilder(3 + 65, [0], 1, main_inputs=3)
    m = b.main
    for _ in range(4):
        m.fetch_many(m.load(0, 0), m.load(0, 1), [m.load(0, 2) + j for j in range(16)], 32)
    m.value(m.load(0, 5))
    return F.trivial(b)


def _sixty_fifth(m):
    m.cols[64] = m.cols[63]


def _value_behind_a_quotient(m):
    """V of the FETCH becomes v / t, an op 7 appended to the program."""
    m.ops.append((air.OP_DIV, next(t for t, o in enumerate(m.ops) if o == (air.OP_LOAD, 0, 2)), next(t for t, o in enumerate(m.ops) if o == (air.OP_LOAD, 0, 1))))
    _pad(1, v_op=len(m.ops) - 1)(m)


def _key_behind_a_quotient(m):
    m.ops.append((air.OP_DIV, 0, 0))
    _col(1, num_op=len(m.ops) - 1)(m)


REFUSALS = [
    ("no-table-key", two_builder, _col(1, den_op=air.AUX_NO_DEN), "derived column 1 is a FETCH column without a table key"),
    ("key-bits-0", two_builder, _pad(1, key_bits=0), "derived column 1 is a FETCH column with key_bits = 0"),
    ("key-bits-65", two_builder, _pad(1, key_bits=65), "derived column 1 is a FETCH column with key_bits = 65"),
    ("v-op-beyond-the-program", two_builder, _pad(1, v_op=60000), "derived column 1 is a FETCH column with v_op = 60000, which is beyond the program or an OUT"),
    ("pad-bit-24", two_builder, _pad(1, high=1 << 24), "derived column 1 is a FETCH column whose pad has a bit at or above 24"),
    ("pad-bit-31", two_builder, _pad(1, high=1 << 31), "derived column 1 is a FETCH column whose pad has a bit at or above 24"),
    ("x-beyond-the-program", two_builder, _col(1, num_op=60000), "derived column 1 names an op beyond the program"),
    ("t-beyond-the-program", two_builder, _col(1, den_op=60000), "derived column 1 names an op beyond the program"),
    ("v-reads-itself", two_builder, _op(lambda o: o == (air.OP_LOAD, 0, 2), b=4), "derived column 1 reads derived column 1, which is not an earlier one"),
    ("v-reads-a-later-column", two_builder, _op(lambda o: o == (air.OP_LOAD, 0, 2), b=5), "derived column 1 reads derived column 2, which is not an earlier one"),
    ("v-behind-a-quotient", two_builder, _value_behind_a_quotient, "derived column 1 depends on a quotient (op 7), which only the seed or the step of a CHAIN column may"),
    ("x-behind-a-quotient", two_builder, _key_behind_a_quotient, "derived column 1 depends on a quotient (op 7), which only the seed or the step of a CHAIN column may"),
    ("sixty-five-columns", sixty_four_builder, _sixty_fifth, "derived column 64 is the program's FETCH column number 65"),
    ("kind-8", two_builder, _col(2, kind=8), "derived column 2 has an unknown kind"),
]


@pytest.mark.parametrize("build,mutate,says", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_decoder_refuses_and_the_builder_raises(hip_lib, build, mutate, says):
    decoder_refuses_and_the_builder_raises(hip_lib, "fetch", build, mutate, says, N)


def test_the_older_entry_points_call_kind_7_unknown(hip_lib):
    for b, k in ((F.count_and_fetch(), 1), (F.input_fetch(2), 0), (air.rom_reads(N, 16), 0)):
        desc, keep = b.build()
        says = f"derived column {k} has an unknown kind"
        for suffix in ("div", "link", "lk", "rec"):
            if suffix == "rec" and any(c[0] == air.MAIN_COUNT for c in b.main.cols[:k]):
                continue                                               # (the COUNT column before it is the unknown kind there)
            assert check_with(hip_lib, suffix, desc, N) == INVALID, suffix
            message = hip_lib.sp_last_error().decode()
            assert says in message and message.startswith(f"sp_air_main_check_{suffix}: main program: "), message
        # the mirror follows the decoder the program would be routed to: without the builder's declaration, or at the level below, kind 7
        # is unknown
        with pytest.raises(ValueError, match=says):
            b.main.check(N, level=air.MainLevel.DIV)
        b.main.check(N)
        b.main.level = air.MainLevel.DIV
        with pytest.raises(ValueError, match=says):
            b.main.check(N)
        b.main.check(N, level=air.MainLevel.FETCH)


def test_null_arguments(hip_lib):
    desc, keep = F.input_fetch(1).build()
    n = ctypes.c_uint64(N)
    assert hip_lib.sp_air_main_check_fetch(None, None, ctypes.byref(desc.main_desc), n) == INVALID
    assert hip_lib.sp_air_main_check_fetch(ctypes.byref(desc), None, None, n) == INVALID
    assert hip_lib.sp_air_prove_fetch(None, None, None, None, None, None, n, None, None, None) == INVALID
    assert hip_lib.sp_air_check_trace_fetch(None, None, None, None, None, None, n, None, None, None, 0, None) == INVALID
    assert hip_lib.sp_air_main_trace_fetch(None, None, None, None, None, n, None) == INVALID
    assert hip_lib.sp_air_main_check_fetch(ctypes.byref(desc), None, ctypes.byref(desc.main_desc), n) == _lib.SP_OK     # no op 6: no ext needed


def test_builder_arguments():
    m = air.AirBuilder(4, [0], 1, main_inputs=3).main
    with pytest.raises(ValueError, match="key_bits 0"):
        m.fetch(m.load(0, 0), m.load(0, 1), m.load(0, 2), 0)
    with pytest.raises(ValueError, match="key_bits 65"):
        m.fetch(m.load(0, 0), m.load(0, 1), m.load(0, 2), 65)
    with pytest.raises(ValueError, match="needs a table key"):
        m.fetch(m.load(0, 0), None, m.load(0, 2))
    with pytest.raises(ValueError, match="at least one table value"):
        m.fetch_many(m.load(0, 0), m.load(0, 1), [])
    assert not m.fetches and not m.cols
    v = m.load(0, 2)
    f = m.fetch(m.load(0, 0), m.load(0, 1), v, 9)
    assert isinstance(f, air.Value) and m.ops[f.i] == (air.OP_LOAD, 0, 3) and m.fetches
    assert m.cols[0][0] == air.MAIN_FETCH and m.cols[0][3] == 9 + 256 * v.i
    wide = air.AirBuilder(3 + 70, [0], 1, main_inputs=3).main
    got = wide.fetch_many(wide.load(0, 0), wide.load(0, 1), [wide.load(0, 2)] * 64)
    assert len(got) == 64 and [wide.ops[x.i][2] for x in got] == list(range(3, 67))
    with pytest.raises(ValueError, match="more than 64 fetched columns"):
        wide.fetch(wide.load(0, 0), wide.load(0, 1), wide.load(0, 2))
