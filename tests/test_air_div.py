"""Quotients in chain steps (op 7, the _div entry points) without a GPU: the new symbols in the header, the binding and the Rust block,
the builder's rules, the decoder's verdicts through sp_air_main_check_div - and those of every older entry point on the same
descriptors -, the builder's mirror of them, and the Python-integer model (MainProgram.evaluate, AirBuilder.check_trace) against a
plain per-cell reference (program_ref), hand-written loops (div_airs.hand_table) and an affine curve adder on air.ec_subset_sum.  Every
comparison is exact."""
import ctypes
import os
import random
import re

import pytest

import chain_airs as C
import div_airs as D
import div_ref as R
import link_airs as L
import program_ref
from air_main_checks import _col, check_with, decoder_refuses_and_the_builder_raises
from lambdaworks_cairo_prover_amd import _lib, air, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = air.P
N, S, LINK = 64, 4, 4
NEW_SYMBOLS = ("sp_air_prove_div", "sp_air_check_trace_div", "sp_air_main_trace_div", "sp_air_main_check_div")
INVALID = _lib.SP_E_INVALID_ARG
MALFORMED_BEFORE = ("main program: malformed op {t} (LOAD needs a shift of 0 .. 7 and a main column, CONST a constant, ADD / SUB / MUL earlier ops; there is no "
                    "OUT and no RAP challenge, and op 6 - a shift of 0 .. 7 and a periodic column - only through the _rec entry points)")
QUOTIENT = "depends on a quotient (op 7), which only the seed or the step of a CHAIN column may: a row-local quotient is a VALUE column's N / D"


def test_symbols_are_declared_everywhere_and_the_abi_is_7(hip_lib):
    header = open(os.path.join(ROOT, "include", "stark252_hip.h")).read()
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = integ.index("```rust")
    rust = set(re.findall(r"pub fn (sp_[a-z0-9_]+)\s*\(", integ[start:integ.index("```\n", start + 10)]))
    for name in NEW_SYMBOLS:
        assert name in declared and name in rust and name in _lib.NEWEST_SYMBOLS and hasattr(hip_lib, name), name
    assert int(re.search(r"#define SP_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.SP_ABI_VERSION == hip_lib.sp_abi_version() == 7
    assert int(re.search(r"#define SP_AIR_OP_DIV\s+(\d+)", header).group(1)) == air.OP_DIV == 7


def mixed_builder(link=LINK):
    return D.mixed(S, link, D.periodic_columns(random.Random(3)))[0]


def ec_builder():
    return D.ec_case(N, 8, random.Random(4))[0]


# ---- the builder ----------------------------------------------------------------------------------------------------------------
def test_quotients_live_in_the_main_program_alone():
    b = air.AirBuilder(3, [0], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM, main_inputs=1)
    for value in (b.load(0, 0), b.aux.load(0, 0), b.public.rap(0)):
        with pytest.raises(ValueError, match="a quotient \\(/\\) lives in a main-trace program only"):
            value / 3
        with pytest.raises(ValueError, match="a quotient \\(/\\) lives in a main-trace program only"):
            3 / value
    m = b.main
    assert not m.divs
    x = m.load(0, 0)
    q = x / 3
    assert m.divs and m.ops[q.i] == (air.OP_DIV, x.i, q.i - 1) and m.ops[q.i - 1][0] == air.OP_CONST
    r = 5 / x
    assert m.ops[r.i] == (air.OP_DIV, r.i - 1, x.i)
    assert m.ops[m.div(q, r).i] == (air.OP_DIV, q.i, r.i)
    other = air.AirBuilder(2, [0], 1, main_inputs=1).main
    with pytest.raises(ValueError, match="operands of a quotient must be values of this program"):
        m.div(x, other.load(0, 0))


def test_the_helpers_and_the_example_pass_the_decoder(hip_lib):
    for b in (mixed_builder(), mixed_builder(link=1), ec_builder(), D.plain_div(S)):
        desc, keep = b.build()
        assert air.needs_div(desc) and air.main_suffix(desc) == "div"
        assert check_with(hip_lib, "div", desc, N) == _lib.SP_OK, hip_lib.sp_last_error()
        api.air_main_check(desc, N)
        assert [air.route(desc, c)[0] for c in ("prove", "check_trace")] == ["sp_air_prove_div", "sp_air_check_trace_div"]
        assert not air.route(desc, "verify")[0].endswith("_div")
        del desc.main_features                       # a descriptor put together by hand is looked through
        assert air.needs_div(desc) and air.main_suffix(desc) == "div"


def test_the_suffix_is_div_only_where_a_descriptor_needs_it(hip_lib):
    for b, want in ((C.mimc_case(N, 8, random.Random(6))[0], "rec"), (air.table_lookup_main(N, [3, 5, 7, 11]), "lk"), (air.bit_range_check(N, 8), "main"),
                    (L.sponge_case(N, S, LINK, random.Random(4))[0], "link"), (L.mixed(S, LINK, L.periodic_columns(random.Random(3)))[0], "link"),
                    (D.poly_only(S), "rec")):
        desc, keep = b.build()
        assert not air.needs_div(desc) and air.main_suffix(desc) == want
        assert check_with(hip_lib, "div", desc, N) == _lib.SP_OK, hip_lib.sp_last_error()      # the _div entry points take what the others take
        del desc.main_features
        assert not air.needs_div(desc) and air.main_suffix(desc) == want


@pytest.mark.parametrize("suffix", ["", "rec", "lk", "link"])
def test_the_entry_points_before_call_op_7_malformed_as_ever(hip_lib, suffix):
    cases = [D.plain_div(S)] + ([mixed_builder(), ec_builder()] if suffix else [])     # (sp_air_main_check takes no periodic columns)
    for b in cases:
        desc, keep = b.build()
        t = next(t for t, o in enumerate(b.main.ops) if o[0] == air.OP_DIV)
        assert check_with(hip_lib, suffix, desc, N) == INVALID
        name = "sp_air_main_check" + ("_" + suffix if suffix else "")
        assert hip_lib.sp_last_error().decode() == f"{name}: " + MALFORMED_BEFORE.format(t=t)
        with pytest.raises(ValueError, match=f"main program: malformed op {t} \\(LOAD, CONST, ADD, SUB, MUL over earlier ops, PERIODIC only\\)"):
            b.main.check(N, level=air.MainLevel[suffix.upper() or "MAIN"])


# ---- the refusal table: the same mutation on the builder's lists and, through main_desc, on the C structs.  mixed: derived columns
# 0 .. 2 are group A, 3 and 4 group B, 5 and 6 group C, 7 .. 22 group D, 23 the VALUE, 24 the SUM.
def _a_quotient(m, nth=1):
    """The nth op 7 of the program (0: the dead one over a zero)."""
    return [t for t, o in enumerate(m.ops) if o[0] == air.OP_DIV][nth]


def _behind(m, t):
    """A fresh op whose value depends on op t without being an op 7 itself."""
    m.ops.append((air.OP_ADD, t, t))
    return len(m.ops) - 1


def _value_behind_a_quotient(m):
    _col(23, num_op=_behind(m, _a_quotient(m)))(m)


def _value_over_a_quotient(m):
    _col(23, den_op=_a_quotient(m))(m)


def _sum_of_the_dead_quotient(m):
    _col(24, num_op=_a_quotient(m, 0))(m)


def _kind_behind_a_quotient(kind, pad=0):
    def mutate(m):
        _col(23, kind=kind, num_op=_a_quotient(m), den_op=air.AUX_NO_DEN, pad=pad)(m)
    return mutate


def _count_behind_a_quotient(which):
    def mutate(m):
        t, plain = _behind(m, _a_quotient(m)), 0          # (op 0 is the LOAD of a)
        _col(23, kind=air.MAIN_COUNT, num_op=t if which == "x" else plain, den_op=plain if which == "x" else t, pad=16)(m)
    return mutate


def _forward_operand(m):
    t = _a_quotient(m)
    m.ops[t] = (air.OP_DIV, m.ops[t][1], t)


def _operand_is_itself_beyond_the_program(m):
    t = _a_quotient(m)
    m.ops[t] = (air.OP_DIV, len(m.ops) + 5, m.ops[t][2])


REFUSALS = [
    ("value-behind-a-quotient", _value_behind_a_quotient, "derived column 23 " + QUOTIENT),
    ("value-over-a-quotient", _value_over_a_quotient, "derived column 23 " + QUOTIENT),
    ("sum-of-the-dead-quotient", _sum_of_the_dead_quotient, "derived column 24 " + QUOTIENT),
    ("inv-or-zero-behind-a-quotient", _kind_behind_a_quotient(air.MAIN_INV_OR_ZERO), "derived column 23 " + QUOTIENT),
    ("bit-behind-a-quotient", _kind_behind_a_quotient(air.MAIN_BIT, 3), "derived column 23 " + QUOTIENT),
    ("product-behind-a-quotient", _kind_behind_a_quotient(air.MAIN_PRODUCT), "derived column 23 " + QUOTIENT),
    ("count-x-behind-a-quotient", _count_behind_a_quotient("x"), "derived column 23 " + QUOTIENT),
    ("count-t-behind-a-quotient", _count_behind_a_quotient("t"), "derived column 23 " + QUOTIENT),
    ("forward-operand", _forward_operand, "malformed op 15"),
    ("operand-beyond-the-program", _operand_is_itself_beyond_the_program, "malformed op 15"),
    # a rule of before, through the new entry point
    ("kind-7", _col(23, kind=7), "derived column 23 has an unknown kind"),
]


@pytest.mark.parametrize("mutate,says", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_decoder_refuses_and_the_builder_raises_word_for_word(hip_lib, mutate, says):
    assert _a_quotient(mixed_builder().main) == 15
    raised, message = decoder_refuses_and_the_builder_raises(hip_lib, "div", mixed_builder, mutate, says, N)
    assert raised.startswith("main program: " + says), raised
    assert message.startswith("sp_air_main_check_div: main program: " + says), message
    if "quotient" in says:
        assert message == "sp_air_main_check_div: " + raised


def test_null_arguments(hip_lib):
    desc, keep = D.plain_div(S).build()
    n = ctypes.c_uint64(N)
    assert hip_lib.sp_air_main_check_div(None, None, ctypes.byref(desc.main_desc), n) == INVALID
    assert hip_lib.sp_air_main_check_div(ctypes.byref(desc), None, None, n) == INVALID
    assert hip_lib.sp_air_main_check_div(ctypes.byref(desc), None, ctypes.byref(desc.main_desc), n) == _lib.SP_OK
    assert hip_lib.sp_air_prove_div(None, None, None, None, None, None, n, None, None, None) == INVALID
    assert hip_lib.sp_air_check_trace_div(None, None, None, None, None, None, n, None, None, None, 0, None) == INVALID
    assert hip_lib.sp_air_main_trace_div(None, None, None, None, None, n, None) == INVALID
    bad = air.ext_of(desc)
    bad.size -= 8
    assert hip_lib.sp_air_main_check_div(ctypes.byref(desc), ctypes.byref(bad), ctypes.byref(desc.main_desc), n) == INVALID


# ---- the model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,s,link", [(8, 4, 2), (8, 8, 1), (64, 2, 1), (64, 64, 1), (64, 8, 4), (256, 8, 4), (256, 64, 2)])
def test_model_reference_and_hand_table_agree(n, s, link):
    rng = random.Random(n + s + link)
    periodic = D.periodic_columns(rng)
    b, cols = D.mixed(s, link, periodic)
    rows, hand = D.mixed_inputs(n, s, link, periodic, rng)       # (asserts that the reference meets no zero)
    model = [[int(x) for x in r] for r in b.main.evaluate(rows)]
    ref = program_ref.main_table(b.main, rows)
    assert cols == {"x0": 2, "x1": 3, "x2": 4, "y0": 5, "y1": 6, "z0": 7, "w0": 9, "v": 25, "r": 26}
    for i in range(n):
        assert model[i] == hand[i] == ref[i], i
    for first in range(0, n, s * link):                 # y1 = carry + 1: the carry in front of every run is zero
        assert model[first][cols["y1"]] == 1


def test_ec_subset_sum_is_clean_and_names_what_breaks():
    s = 8
    b, rows, points, shift, result = D.ec_case(N, s, random.Random(21))
    assert b.check_trace(rows) == []
    full = [[int(x) for x in r] for r in b.main.evaluate(rows)]
    assert full == R.ec_subset_sum_table(rows, s, points, shift) == program_ref.main_table(b.main, rows)
    assert b.check_trace(full) == []                                           # the whole table, as ever
    for first in range(0, N, s):                                                # every block is the sum of its own bits
        acc = shift
        for t in range(s - 1):
            if rows[first + t][0]:
                acc = R.ec_add(acc, points[t])
        assert tuple(full[first + s - 1][1:3]) == acc
        assert (acc[1] ** 2 - acc[0] ** 3 - acc[0] - D.EC_BETA) % P == 0
    assert tuple(full[s - 1][1:3]) == result
    wrong = D.ec_case(N, s, random.Random(21), wrong=1)[0]
    assert wrong.check_trace(rows) == [air.Violation(air.BOUNDARY, 0, 1, s - 1, s - 1, result[0])]
    # a bit that is no bit: b (b - 1) there, and the two additions it scales
    bad = [list(r) for r in rows]
    bad[2] = [2]
    assert {(v.kind, v.index) for v in b.check_trace(bad)} >= {(air.TRANSITION, 0)}
    # one slope changed behind the table's back: the chord constraint, its square and its product on that row, the steps out of it
    tampered = [list(r) for r in full]
    tampered[s + 1][3] = (tampered[s + 1][3] + 1) % P
    found = b.check_trace(tampered)
    assert {v.index for v in found} >= {1, 2} and all(v.first_row == v.last_row == s + 1 for v in found)


def test_a_zero_denominator_raises_in_the_model_where_it_is_reached():
    b = D.plain_div(S)                                          # the seed x1 = a(i + 1) / (a + 2) on the rows = 0 (mod 4)
    rng = random.Random(23)
    rows = [[rng.randrange(P)] for _ in range(N)]
    assert b.check_trace(rows) == []
    rows[5] = [P - 2]                                           # a + 2 = 0 on a row where no seed is evaluated: nothing to refuse
    b.main.evaluate(rows)
    program_ref.main_table(b.main, rows)
    rows[8] = [P - 2]
    with pytest.raises(ValueError, match="a denominator of a quotient \\(op 7\\) is zero on some row"):
        b.main.evaluate(rows)
    with pytest.raises(program_ref.ZeroDenominator):
        program_ref.main_table(b.main, rows)
    # an accumulator that meets the point it is to add has no chord
    s = 8
    points, shift = D.ec_points(s)
    rows = [[1]] * N
    meets = air.ec_subset_sum(N, s, points, points[0], (0, 0))
    with pytest.raises(ValueError, match="a denominator of a quotient"):
        meets.main.evaluate(rows)
