"""Lookup multiplicities in a main program (SP_AIR_MAIN_COUNT, the _lk entry points) without a GPU: the new symbols in the header, the
binding and the Rust block, the decoder's verdicts through sp_air_main_check_lk - and the older entry points' on the same descriptors -,
the builder's mirror of them, and the Python-integer model (MainProgram.evaluate, AirBuilder.check_trace) against
air.table_lookup_trace and a hand-written double loop."""
import ctypes
import os
import random
import re

import pytest

import lookup_airs as L
from air_main_checks import _col, _op, check_with, decoder_refuses_and_the_builder_raises
from lambdaworks_cairo_prover_amd import _lib, air, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = air.P
N = 64
NEW_SYMBOLS = ("sp_air_prove_lk", "sp_air_check_trace_lk", "sp_air_main_trace_lk", "sp_air_main_check_lk", "sp_air_main_count_limits")
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
    assert int(re.search(r"#define SP_AIR_MAIN_COUNT\s+(\d+)", header).group(1)) == 6 == air.MAIN_COUNT
    hip_lib.sp_air_main_desc_size.restype = ctypes.c_uint64
    assert hip_lib.sp_air_main_desc_size() == ctypes.sizeof(air.AirMainDescC) == 64 and ctypes.sizeof(air.AirMainColumnC) == 16


def test_the_limits_call(hip_lib):
    assert api.air_main_count_limits() == {"key_bits": 64, "columns": 16} == {"key_bits": air.MAIN_COUNT_MAX_KEY_BITS, "columns": air.MAIN_COUNT_MAX_COLS}
    assert hip_lib.sp_air_main_count_limits(None) == INVALID


def periodic8():
    rng = random.Random(3)
    return [rng.randrange(P) for _ in range(L.MIXED_PERIOD)]


def mixed_builder():
    return L.mixed(periodic8())[0]


def sixteen_builder():
    """Sixteen COUNT columns and a VALUE behind them."""
    b = air.AirBuilder(19, [0], 1, main_inputs=2)
    m = b.main
    for j in range(16):
        m.multiplicity(m.load(0, 0) + j, m.load(0, 1), 32)
    m.value(m.load(0, 17))
    return L.trivial(b)


def test_the_helpers_and_the_examples_pass_the_decoder(hip_lib):
    builders = (mixed_builder(), sixteen_builder(), L.plain_count(), L.periodic_count([1, 2, 3, 4], 8), L.two_counts(8, [5, 6]), L.input_table_lookup(),
                air.table_lookup_main(N, [3, 5, 5, 9], 8), air.xor_lookup(256, 4))
    for b in builders:
        desc, keep = b.build()
        assert air.needs_lk(desc)
        assert check_with(hip_lib, "lk", desc, 256) == _lib.SP_OK, hip_lib.sp_last_error()
        api.air_main_check(desc, 256)
        assert [air.route(desc, c)[0] for c in ("prove", "check_trace")] == ["sp_air_prove_lk", "sp_air_check_trace_lk"]
        assert not air.route(desc, "verify")[0].endswith("_lk")
    # programs without a COUNT column go where they went, and the new decoder takes them too
    desc, keep = air.zero_count(N, 3).build()
    assert not air.needs_lk(desc) and air.route(desc, "prove")[0] == "sp_air_prove_main" and check_with(hip_lib, "lk", desc, N) == _lib.SP_OK
    keys = [7] * 8
    desc, keep = air.mimc_blocks(N, 8, keys, 0).build()
    assert not air.needs_lk(desc) and air.route(desc, "prove")[0] == "sp_air_prove_rec" and check_with(hip_lib, "lk", desc, N) == _lib.SP_OK
    # a descriptor put together by hand is looked through
    desc, keep = L.plain_count().build()
    del desc.main_features
    assert air.needs_lk(desc)


# ---- the refusal table: the same mutation on the builder's lists (ops [(op, a, b)], cols [(kind, num_op, den_op, pad)]) and, through
# build(), on the C structs.  mixed: derived column 0 is the VALUE (main column 2), 1 the COUNT, 2 the SUM.
def _seventeenth(m):
    m.cols[16] = (air.MAIN_COUNT, m.cols[15][1], m.cols[15][2], 32)


REFUSALS = [
    ("no-table", mixed_builder, _col(1, den_op=air.AUX_NO_DEN), "derived column 1 is a COUNT column without a table"),
    ("key-bits-0", mixed_builder, _col(1, pad=0), "derived column 1 is a COUNT column with key_bits = 0"),
    ("key-bits-65", mixed_builder, _col(1, pad=65), "derived column 1 is a COUNT column with key_bits = 65"),
    ("x-reads-itself", mixed_builder, _op(lambda o: o == (air.OP_LOAD, 0, 2), b=3), "derived column 1 reads derived column 1, which is not an earlier one"),
    ("t-reads-a-later-column", mixed_builder, _op(lambda o: o == (air.OP_LOAD, 0, 1), b=4), "derived column 1 reads derived column 2, which is not an earlier one"),
    ("x-beyond-the-program", mixed_builder, _col(1, num_op=60000), "derived column 1 names an op beyond the program"),
    ("t-beyond-the-program", mixed_builder, _col(1, den_op=60000), "derived column 1 names an op beyond the program"),
    ("seventeen-columns", sixteen_builder, _seventeenth, "derived column 16 is the program's COUNT column number 17"),
    ("kind-7", mixed_builder, _col(2, kind=7), "derived column 2 has an unknown kind"),
]


@pytest.mark.parametrize("build,mutate,says", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_decoder_refuses_and_the_builder_raises(hip_lib, build, mutate, says):
    decoder_refuses_and_the_builder_raises(hip_lib, "lk", build, mutate, says, N, mirror=says.split(" (")[0])


def test_the_older_entry_points_call_kind_6_unknown(hip_lib):
    for b, k in ((mixed_builder(), 1), (L.plain_count(), 0), (air.table_lookup_main(N, [3, 5, 5, 9], 8), 0)):
        desc, keep = b.build()
        says = f"derived column {k} has an unknown kind"
        assert check_with(hip_lib, "rec", desc, N) == INVALID and says in hip_lib.sp_last_error().decode()
        if not any(o[0] == air.OP_PERIODIC for o in b.main.ops):     # (op 6 is a malformed op there, and the ops are judged first)
            assert check_with(hip_lib, "", desc, N) == INVALID and says in hip_lib.sp_last_error().decode()
        # the mirror follows the decoder the program would be routed to: without the builder's declaration, or at the level below, kind 6
        # is unknown
        with pytest.raises(ValueError, match=says):
            b.main.check(N, level=air.MainLevel.REC)
        b.main.check(N)
        b.main.level = air.MainLevel.REC
        with pytest.raises(ValueError, match=says):
            b.main.check(N)
        b.main.check(N, level=air.MainLevel.LK)


def test_null_arguments(hip_lib):
    desc, keep = L.plain_count().build()
    n = ctypes.c_uint64(N)
    assert hip_lib.sp_air_main_check_lk(None, None, ctypes.byref(desc.main_desc), n) == INVALID
    assert hip_lib.sp_air_main_check_lk(ctypes.byref(desc), None, None, n) == INVALID
    assert hip_lib.sp_air_prove_lk(None, None, None, None, None, None, n, None, None, None) == INVALID
    assert hip_lib.sp_air_check_trace_lk(None, None, None, None, None, None, n, None, None, None, 0, None) == INVALID
    assert hip_lib.sp_air_main_trace_lk(None, None, None, None, None, n, None) == INVALID
    bad = air.ext_of(desc)
    bad.size -= 8
    assert hip_lib.sp_air_main_check_lk(ctypes.byref(desc), ctypes.byref(bad), ctypes.byref(desc.main_desc), n) == INVALID
    assert check_with(hip_lib, "lk", desc, N, ext=False) == _lib.SP_OK            # no op 6: no ext needed


def test_builder_arguments():
    m = air.AirBuilder(3, [0], 1, main_inputs=2).main
    with pytest.raises(ValueError, match="key_bits 0"):
        m.multiplicity(m.load(0, 0), m.load(0, 1), 0)
    with pytest.raises(ValueError, match="key_bits 65"):
        m.multiplicity(m.load(0, 0), m.load(0, 1), 65)
    with pytest.raises(ValueError, match="needs a table"):
        m.multiplicity(m.load(0, 0), None)
    assert not m.lookups
    assert m.multiplicity(m.load(0, 0), m.load(0, 1), 1) == 2 and m.lookups and m.cols[0][0] == air.MAIN_COUNT and m.cols[0][3] == 1
    wide = air.AirBuilder(30, [0], 1, main_inputs=2).main
    for j in range(16):
        wide.multiplicity(wide.load(0, 0), wide.load(0, 1))
    with pytest.raises(ValueError, match="more than 16 multiplicity columns"):
        wide.multiplicity(wide.load(0, 0), wide.load(0, 1))


# ---- the model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,table,key_bits", [(64, [3, 5, 5, 9, 11, 200, 7, 1], 8), (64, [0, (1 << 64) - 1], 64), (16, [4] * 16, 3), (32, [6, 2, 6, 6], 64)])
def test_model_equals_table_lookup_trace_cell_for_cell(n, table, key_bits):
    """One table with a value repeated inside its period, one with the ends of the 64-bit range, one of a single value, one of period 4
    with three equal entries."""
    rng = random.Random(n + key_bits)
    b = air.table_lookup_main(n, table, key_bits)
    rows = air.table_lookup_main_inputs(n, table, rng)
    got = [[int(x) for x in r] for r in b.main.evaluate(rows)]
    want = air.table_lookup_trace(n, table, [r[0] for r in rows])
    for i in range(n):
        assert got[i] == want[i], i
    assert sum(r[1] for r in got) == n
    assert b.check_trace(rows, rap=[0x5eed]) == air.table_lookup(n, table).check_trace(want, rap=[0x5eed]) == []


@pytest.mark.parametrize("n", [16, 64])
def test_evaluate_agrees_with_a_hand_written_double_loop(n):
    rng = random.Random(n)
    periodic = periodic8()
    b, cols = L.mixed(periodic)
    assert cols == {"v": 2, "m": 3, "r": 4}
    rows = L.mixed_inputs(n, periodic, rng)
    got = [[int(x) for x in r] for r in b.main.evaluate(rows)]
    want = L.hand_table(rows, periodic)
    for i in range(n):
        assert got[i] == want[i], i
    total = sum(r[3] for r in want)
    assert 0 < total < n and any(r[3] > 1 for r in want)        # some X hit the table, some miss it, some value is looked up twice


def test_evaluate_refuses_a_key_out_of_range():
    b = L.plain_count(8)
    rows = [[i, i] for i in range(16)]
    assert [int(r[2]) for r in b.main.evaluate(rows)] == [1] * 16
    for col in (0, 1):                                                  # on X only, on T only
        bad = [list(r) for r in rows]
        bad[5][col] = 256
        with pytest.raises(ValueError, match="a lookup key is out of range on some row"):
            b.main.evaluate(bad)
    bad = [list(r) for r in rows]
    bad[5][0] = 255                                                     # the largest key is in range, and in no table entry
    assert sum(int(r[2]) for r in b.main.evaluate(bad)) == 15


def test_xor_lookup_is_clean_and_a_wrong_xor_is_counted_nowhere():
    n, bits = 256, 4
    rng = random.Random(5)
    b = air.xor_lookup(n, bits)
    rows = air.xor_lookup_inputs(n, bits, rng)
    assert b.periodic_cols[0] == air.xor_lookup_table(bits) and len(set(b.periodic_cols[0])) == 256
    full = b.main.evaluate(rows)
    assert sum(int(r[3]) for r in full) == n
    for i in range(n):                                                  # the table entry of row i is the triple of a = i mod 16, b = i div 16
        assert int(full[i][3]) == sum(1 for r in rows if r[0] == i % 16 and r[1] == i // 16)
    assert b.check_trace(rows, rap=[0x5eed]) == []
    rows[9][2] ^= 1
    assert sum(int(r[3]) for r in b.main.evaluate(rows)) == n - 1
    assert b.check_trace(rows, rap=[0x5eed]) != []


def test_check_trace_reports_the_broken_logup_constraint():
    """One looked-up value is outside the table: it is counted nowhere, the running sum is short of 1 / (gamma - a) from that row on and
    does not close where the last row wraps to s_0 = 0 - the one constraint, on the last row."""
    n, table, gamma = 64, [3, 5, 5, 9, 11, 200, 7, 1], 0x5eed
    b = air.table_lookup_main(n, table, 8)
    rows = air.table_lookup_main_inputs(n, table, random.Random(6))
    assert b.check_trace(rows, rap=[gamma]) == []
    rows[20] = [4]
    assert sum(int(r[1]) for r in b.main.evaluate(rows)) == n - 1
    report = b.check_trace(rows, rap=[gamma])
    assert [(v.kind, v.index, v.first_row, v.last_row) for v in report] == [(air.TRANSITION, 0, n - 1, n - 1)], report
