"""Main-trace programs (sp_air_main_desc) without a GPU: the struct mirror, the new symbols in the header, the binding and the Rust
block, the decoder's verdicts through sp_air_main_check, and the Python-integer model (MainProgram.evaluate, AirBuilder.check_trace)
on the two worked examples."""
import ctypes
import os
import random
import re

import pytest

from lambdaworks_cairo_prover_amd import _lib, air, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = air.P
N = 16
NEW_SYMBOLS = ("sp_air_prove_main", "sp_air_check_trace_main", "sp_air_main_trace", "sp_air_main_check", "sp_air_main_desc_size")


def test_struct_mirror_matches_the_library(hip_lib):
    hip_lib.sp_air_main_desc_size.restype = ctypes.c_uint64
    assert hip_lib.sp_air_main_desc_size() == ctypes.sizeof(air.AirMainDescC) == 64
    assert ctypes.sizeof(air.AirMainColumnC) == 16
    air._check_main_layout()


def test_symbols_are_declared_everywhere_and_the_abi_is_7(hip_lib):
    header = open(os.path.join(ROOT, "include", "stark252_hip.h")).read()
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = integ.index("```rust")
    rust = set(re.findall(r"pub fn (sp_[a-z0-9_]+)\s*\(", integ[start:integ.index("```\n", start + 10)]))
    for name in NEW_SYMBOLS:
        assert name in declared and name in rust and name in _lib.NEWEST_SYMBOLS and hasattr(hip_lib, name), name
    assert int(re.search(r"#define SP_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.SP_ABI_VERSION == hip_lib.sp_abi_version() == 7
    for name, value in (("VALUE", 0), ("INV_OR_ZERO", 1), ("BIT", 2), ("SUM", 3), ("PRODUCT", 4)):
        assert int(re.search(rf"#define SP_AIR_MAIN_{name}\s+(\d+)", header).group(1)) == value == getattr(air, "MAIN_" + name)


def zero_count_desc():
    return air.zero_count(N, 3).build()


def bit_desc():
    return air.bit_range_check(N, 8).build()


def test_both_examples_pass_the_decoder(hip_lib):
    for desc, keep in (zero_count_desc(), bit_desc(), air.bit_range_check(N, 65).build()):
        assert hip_lib.sp_air_main_check(ctypes.byref(desc), ctypes.byref(desc.main_desc), ctypes.c_uint64(N)) == _lib.SP_OK
        api.air_main_check(desc, N)


# zero_count's program: op 0 LOAD(0, 0), 1 INV_OR_ZERO's operand is op 0; then CONST 1, LOAD(0, 0), LOAD(0, 1), MUL, SUB; LOAD(0, 2)
def _set(path, value):
    def mutate(d):
        obj = d.main_desc
        *head, last = path
        for step in head:
            obj = getattr(obj, step) if isinstance(step, str) else obj[step]
        setattr(obj, last, value)
    return mutate


def _null(member):
    def mutate(d):
        setattr(d.main_desc, member, None)
    return mutate


def _first_op(d, op):
    m = d.main_desc
    return next(i for i in range(m.n_ops) if m.ops[i].op == op)


def _op(op_kind, **fields):
    """Rewrites the first op of kind `op_kind`."""
    def mutate(d):
        o = d.main_desc.ops[_first_op(d, op_kind)]
        for k, v in fields.items():
            setattr(o, k, v)
    return mutate


def _self_operand(d):
    t = _first_op(d, air.OP_MUL)
    d.main_desc.ops[t].a = t


def _later_operand(d):
    t = _first_op(d, air.OP_MUL)
    d.main_desc.ops[t].b = d.main_desc.n_ops - 1


def _load_own_column(d):
    """The ops behind derived column 0 (inv) load derived column 0 itself."""
    d.main_desc.ops[0].b = d.main_desc.input_cols


def _load_later_column(d):
    """f = 1 - x inv (derived column 1) loads c (derived column 2) instead of inv."""
    m = d.main_desc
    t = next(i for i in range(m.n_ops) if m.ops[i].op == air.OP_LOAD and m.ops[i].b == 1)
    m.ops[t].b = 3


def _aux_kind(kind):
    def mutate(d):
        d.aux_kind = kind
    return mutate


INVALID, UNSUPPORTED = _lib.SP_E_INVALID_ARG, _lib.SP_E_UNSUPPORTED
MALFORMED = [
    ("size", zero_count_desc, _set(("size",), 60), INVALID, "size"),
    ("size-zero", zero_count_desc, _set(("size",), 0), INVALID, "size"),
    ("null-ops", zero_count_desc, _null("ops"), INVALID, "null"),
    ("null-consts", zero_count_desc, _null("consts"), INVALID, "null"),
    ("null-cols", zero_count_desc, _null("cols"), INVALID, "null"),
    ("no-inputs", zero_count_desc, _set(("input_cols",), 0), INVALID, "input_cols"),
    ("columns-short", zero_count_desc, _set(("n_cols",), 2), INVALID, "main_cols"),
    ("columns-long", zero_count_desc, _set(("input_cols",), 2), INVALID, "main_cols"),
    ("no-columns", zero_count_desc, _set(("n_cols",), 0), INVALID, "main_cols"),
    ("location", zero_count_desc, _set(("input_location",), 2), INVALID, "input_location"),
    ("no-ops", zero_count_desc, _set(("n_ops",), 0), INVALID, "ops"),
    ("too-many-ops", zero_count_desc, _set(("n_ops",), 65536), INVALID, "ops"),
    ("too-many-consts", zero_count_desc, _set(("n_consts",), 4097), INVALID, "constants"),
    ("unknown-kind", zero_count_desc, _set(("cols", 1, "kind"), 5), INVALID, "unknown kind"),
    ("bit-252", bit_desc, _set(("cols", 3, "pad"), 252), INVALID, "bit 252"),
    ("den-on-inv-or-zero", zero_count_desc, _set(("cols", 0, "den_op"), 0), INVALID, "no denominator"),
    ("den-on-bit", bit_desc, _set(("cols", 0, "den_op"), 0), INVALID, "no denominator"),
    ("op-out", zero_count_desc, _op(air.OP_SUB, op=air.OP_OUT), INVALID, "malformed op"),
    ("op-periodic", zero_count_desc, _op(air.OP_LOAD, op=air.OP_PERIODIC), INVALID, "malformed op"),
    ("op-7", zero_count_desc, _op(air.OP_SUB, op=7), INVALID, "malformed op"),
    ("operand-itself", zero_count_desc, _self_operand, INVALID, "malformed op"),
    ("operand-later", zero_count_desc, _later_operand, INVALID, "malformed op"),
    ("shift-8", zero_count_desc, _op(air.OP_LOAD, a=8), INVALID, "malformed op"),
    ("load-beyond-main", zero_count_desc, _op(air.OP_LOAD, b=4), INVALID, "malformed op"),
    ("const-beyond", zero_count_desc, _op(air.OP_CONST, a=1), INVALID, "malformed op"),
    ("load-own-column", zero_count_desc, _load_own_column, INVALID, "not an earlier one"),
    ("load-later-column", zero_count_desc, _load_later_column, INVALID, "not an earlier one"),
    ("num-op-beyond", zero_count_desc, _set(("cols", 2, "num_op"), 1000), INVALID, "beyond the program"),
    ("den-op-beyond", zero_count_desc, _set(("cols", 1, "den_op"), 1000), INVALID, "beyond the program"),
    ("aux-kind-1", zero_count_desc, _aux_kind(air.AUX_FIBONACCI_RAP), UNSUPPORTED, "aux_kind"),
    ("aux-kind-2", zero_count_desc, _aux_kind(air.AUX_CALLBACK), UNSUPPORTED, "aux_kind"),
]


@pytest.mark.parametrize("build,mutate,code,says", [c[1:] for c in MALFORMED], ids=[c[0] for c in MALFORMED])
def test_decoder_refuses_malformed_programs(hip_lib, build, mutate, code, says):
    desc, keep = build()
    assert hip_lib.sp_air_main_check(ctypes.byref(desc), ctypes.byref(desc.main_desc), ctypes.c_uint64(N)) == _lib.SP_OK
    mutate(desc)
    assert hip_lib.sp_air_main_check(ctypes.byref(desc), ctypes.byref(desc.main_desc), ctypes.c_uint64(N)) == code
    assert says in hip_lib.sp_last_error().decode()
    with pytest.raises(api.SpError) as e:
        api.air_main_check(desc, N)
    assert e.value.code == code


def test_null_arguments(hip_lib):
    desc, keep = zero_count_desc()
    assert hip_lib.sp_air_main_check(None, ctypes.byref(desc.main_desc), ctypes.c_uint64(N)) == INVALID
    assert hip_lib.sp_air_main_check(ctypes.byref(desc), None, ctypes.c_uint64(N)) == INVALID
    assert hip_lib.sp_air_prove_main(None, None, None, None, None, None, ctypes.c_uint64(N), None, None, None) == INVALID
    assert hip_lib.sp_air_check_trace_main(None, None, None, None, None, None, ctypes.c_uint64(N), None, None, None, 0, None) == INVALID
    assert hip_lib.sp_air_main_trace(None, None, None, None, ctypes.c_uint64(N), None) == INVALID


def test_builder_mirrors_the_decoder():
    b = air.zero_count(N, 3)
    with pytest.raises(ValueError, match="neither an input nor a derived column declared so far"):
        b.main.load(0, 4)
    with pytest.raises(ValueError, match="row shift"):
        b.main.load(8, 0)
    with pytest.raises(ValueError, match="more derived columns"):
        b.main.value(1)
    with pytest.raises(ValueError, match="bit 252"):
        air.AirBuilder(3, [0], 1, main_inputs=1).main.bit(1, 252)
    # lists filled by hand go through check_limits: a column that reads a later one, a denominator on a BIT, a missing column
    b = air.zero_count(N, 3)
    b.main.ops[0] = (air.OP_LOAD, 0, 3)
    with pytest.raises(ValueError, match="reads derived column 2"):
        b.build()
    b = air.bit_range_check(N, 4)
    b.main.cols[2] = (air.MAIN_BIT, 0, 0, 2)
    with pytest.raises(ValueError, match="takes no denominator"):
        b.build()
    b = air.zero_count(N, 3)
    b.main.cols.pop()
    with pytest.raises(ValueError, match="main_cols = 4"):
        b.build()
    b = air.AirBuilder(2, [0], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_FIBONACCI_RAP, main_inputs=1)
    b.main.value(b.main.load(0, 0))
    b.constraint(b.load(0, 0) - b.load(0, 1), 1, 0)
    with pytest.raises(ValueError, match="AUX_NONE or AUX_PROGRAM"):
        b.build()
    with pytest.raises(ValueError, match="at least one input"):
        air.AirBuilder(2, [0], 1, main_inputs=2)


def test_evaluate_agrees_with_hand_written_tables():
    rng = random.Random(11)
    # bit_range_check: row i is v, then bit j of v
    bits = 12
    rows = air.bit_range_check_inputs(N, bits, rng)
    rows[0], rows[1] = [0], [(1 << bits) - 1]
    want = [[v] + [(v >> j) & 1 for j in range(bits)] for (v,) in rows]
    got = air.bit_range_check(N, bits).main.evaluate(rows)
    assert got.shape == (N, 1 + bits) and [[int(x) for x in r] for r in got] == want
    # zero_count: x, 1/x or 0, the is-zero flag, the zeros before the row
    zeros = (0, 5, 6, N - 1)
    rows = air.zero_count_inputs(N, zeros, rng)
    want, before = [], 0
    for i, (x,) in enumerate(rows):
        assert (x == 0) == (i in zeros)
        want.append([x, pow(x, P - 2, P) if x else 0, 1 if x == 0 else 0, before])
        before += x == 0
    got = air.zero_count(N, 3).main.evaluate(rows)
    assert [[int(x) for x in r] for r in got] == want
    assert all(x * inv % P == 1 - f for x, inv, f, _ in want)


def test_check_trace_is_clean_and_names_what_a_bad_input_breaks():
    rng = random.Random(12)
    bits, gamma = 10, 0x1234567
    b = air.bit_range_check(N, bits)
    rows = air.bit_range_check_inputs(N, bits, rng)
    assert b.check_trace(rows, rap=[gamma]) == []
    assert b.check_trace(b.main.evaluate(rows), rap=[gamma]) == []          # the whole table, as ever
    rows[9] = [1 << bits]                                                     # its low bits are all zero: the sum is 0, not v
    assert b.check_trace(rows, rap=[gamma]) == [air.Violation(air.TRANSITION, 1, 1, 9, 9, (-(1 << bits)) % P)]
    rows[3] = [(1 << bits) + 5]
    assert b.check_trace(rows, rap=[gamma]) == [air.Violation(air.TRANSITION, 1, 2, 3, 9, (-(1 << bits)) % P)]
    # zero_count: three zeros below the last row (the one on it is not counted)
    zeros = (2, 3, 11, N - 1)
    rows = air.zero_count_inputs(N, zeros, rng)
    assert air.zero_count(N, 3).check_trace(rows) == []
    c = 3                                                                     # main column of the count
    assert air.zero_count(N, 4).check_trace(rows) == [air.Violation(air.BOUNDARY, 1, 1, N - 1, N - 1, 3)]
    assert air.zero_count(N, 3).check_trace(air.zero_count(N, 3).main.evaluate(rows)) == []
    full = air.zero_count(N, 3).main.evaluate(rows)
    assert [int(full[i][c]) for i in (0, 2, 3, 4, 12, N - 1)] == [0, 0, 1, 2, 3, 3]
