"""Block recurrences in a main program (SP_AIR_MAIN_CHAIN, op 6, the _rec entry points) without a GPU: the new symbols in the header, the
binding and the Rust block, the decoder's verdicts through sp_air_main_check_rec - and the old entry point's on the same descriptors -,
the builder's mirror of them, and the Python-integer model (MainProgram.evaluate, AirBuilder.check_trace) against a hand-written double
loop and on air.mimc_blocks."""
import ctypes
import os
import random
import re

import pytest

import chain_airs as C
from air_main_checks import _col, _first, _op, check_with, decoder_refuses_and_the_builder_raises
from lambdaworks_cairo_prover_amd import _lib, air, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = air.P
N, S = 64, 8
LOG_S = 3
NEW_SYMBOLS = ("sp_air_prove_rec", "sp_air_check_trace_rec", "sp_air_main_trace_rec", "sp_air_main_check_rec", "sp_air_main_chain_limits")
INVALID, UNSUPPORTED = _lib.SP_E_INVALID_ARG, _lib.SP_E_UNSUPPORTED


def test_symbols_are_declared_everywhere_and_the_abi_is_7(hip_lib):
    header = open(os.path.join(ROOT, "include", "stark252_hip.h")).read()
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = integ.index("```rust")
    rust = set(re.findall(r"pub fn (sp_[a-z0-9_]+)\s*\(", integ[start:integ.index("```\n", start + 10)]))
    for name in NEW_SYMBOLS:
        assert name in declared and name in rust and name in _lib.NEWEST_SYMBOLS and hasattr(hip_lib, name), name
    assert int(re.search(r"#define SP_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.SP_ABI_VERSION == hip_lib.sp_abi_version() == 7
    assert int(re.search(r"#define SP_AIR_MAIN_CHAIN\s+(\d+)", header).group(1)) == 5 == air.MAIN_CHAIN
    hip_lib.sp_air_main_desc_size.restype = ctypes.c_uint64
    assert hip_lib.sp_air_main_desc_size() == ctypes.sizeof(air.AirMainDescC) == 64 and ctypes.sizeof(air.AirMainColumnC) == 16
    assert api.air_main_chain_limits() == {"width": 16, "shift": 7} == {"width": air.MAIN_CHAIN_MAX_WIDTH, "shift": air.AUX_MAX_SHIFT}
    assert hip_lib.sp_air_main_chain_limits(None) == INVALID


def mixed_builder():
    return C.mixed(S, C.periodic_columns(random.Random(3)))[0]


def wide_builder():
    """A group of sixteen columns and a VALUE behind it."""
    b = air.AirBuilder(18, [0], 1, main_inputs=1)
    m = b.main
    g = m.chain(S, [m.load(0, 0) + j for j in range(16)])
    g.step([g.state(j) * g.state((j + 1) % 16) for j in range(16)])
    m.value(m.load(0, g.cols[15]))
    x = b.load(0, 0)
    b.constraint(x - x, degree=1, exemptions=0)
    return b


def mimc_builder():
    return C.mimc_case(N, S, random.Random(4))[0]


def test_the_helpers_and_the_example_pass_the_decoder(hip_lib):
    for b in (mixed_builder(), wide_builder(), C.plain_pair(S), C.chain_permutation(S), mimc_builder(), C.mimc_case(N, S, random.Random(5), 3)[0]):
        desc, keep = b.build()
        assert air.needs_rec(desc)
        assert check_with(hip_lib, "rec", desc, N) == _lib.SP_OK, hip_lib.sp_last_error()
        api.air_main_check(desc, N)
    desc, keep = air.zero_count(N, 3).build()          # a program without either goes where it went
    assert not air.needs_rec(desc) and air.route(desc, "prove")[0] == "sp_air_prove_main" and check_with(hip_lib, "rec", desc, N) == _lib.SP_OK
    desc, keep = mimc_builder().build()
    assert [air.route(desc, c)[0] for c in ("prove", "check_trace")] == ["sp_air_prove_rec", "sp_air_check_trace_rec"]
    assert not air.route(desc, "verify")[0].endswith("_rec")


# ---- the refusal table: the same mutation on the builder's lists (ops [(op, a, b)], cols [(kind, num_op, den_op, pad)]) and, through
# build(), on the C structs.  mixed: derived columns 0 .. 2 are group A (main columns 2 .. 4), 3 and 4 group B, 5 the VALUE, 6 the SUM.
def is_state_x0(o):
    return o == (air.OP_LOAD, 0, 2)


def _seed_is_state(m):
    _col(1, den_op=_first(m, is_state_x0))(m)


def _seventeenth(m):
    m.cols[16] = (air.MAIN_CHAIN, m.cols[15][1], m.cols[15][2], LOG_S + 256 * 16)


def is_periodic(o):
    return o[0] == air.OP_PERIODIC


REFUSALS = [
    ("j-without-a-group", mixed_builder, _col(0, pad=LOG_S + 256), INVALID, "derived column 0 is a CHAIN column with j = 1 out of sequence"),
    ("j-skips", mixed_builder, _col(2, pad=LOG_S + 256 * 3), INVALID, "derived column 2 is a CHAIN column with j = 3 out of sequence"),
    ("j-repeats", mixed_builder, _col(2, pad=LOG_S + 256), INVALID, "derived column 2 is a CHAIN column with j = 1 out of sequence"),
    ("seventeen-columns", wide_builder, _seventeenth, INVALID, "derived column 16 makes its chain group longer than 16"),
    ("l-zero", mixed_builder, _col(0, pad=0), INVALID, "derived column 0 is a CHAIN column with l = 0"),
    ("block-longer-than-n", mixed_builder, _col(0, pad=7), INVALID, "derived column 0 is a CHAIN column with l = 7"),
    ("l-differs", mixed_builder, _col(1, pad=2 + 256), INVALID, "derived column 1 differs from its chain group in l"),
    ("step-at-a-shift", mixed_builder, _op(is_state_x0, a=1), INVALID, "has a step that loads derived column 0 of its own chain group at a shift other than 0"),
    ("seed-loads-its-group", mixed_builder, _seed_is_state, INVALID, "derived column 1 has a seed that loads derived column 0 of its own chain group"),
    ("step-loads-a-later-column", mixed_builder, _op(is_state_x0, b=7), INVALID, "reads derived column 5, which is not an earlier one"),
    ("seed-loads-a-later-column", mixed_builder, _op(lambda o: o == (air.OP_LOAD, 3, 0), b=8), INVALID, "reads derived column 6, which is not an earlier one"),
    ("no-seed", mixed_builder, _col(0, den_op=air.AUX_NO_DEN), INVALID, "derived column 0 is a CHAIN column without a seed"),
    ("step-beyond-the-program", mixed_builder, _col(4, num_op=60000), INVALID, "derived column 4 names an op beyond the program"),
    ("periodic-column-2-of-2", mixed_builder, _op(is_periodic, b=2), INVALID, "reads periodic column 2"),
    ("periodic-shift-8", mixed_builder, _op(is_periodic, a=8), INVALID, "malformed op"),
    ("kind-6", mixed_builder, _col(5, kind=6), INVALID, "derived column 5 has an unknown kind"),
]


@pytest.mark.parametrize("build,mutate,code,says", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_decoder_refuses_and_the_builder_raises(hip_lib, build, mutate, code, says):
    decoder_refuses_and_the_builder_raises(hip_lib, "rec", build, mutate, says, N, code, mirror=says.split(" (")[0])


def test_periodic_reads_need_the_periodic_columns(hip_lib):
    desc, keep = mixed_builder().build()
    assert check_with(hip_lib, "rec", desc, N, ext=False) == INVALID
    assert "reads periodic column 0, and the statement has 0" in hip_lib.sp_last_error().decode()
    ext = air.ext_of(desc)
    ext.periodic = None
    assert hip_lib.sp_air_main_check_rec(ctypes.byref(desc), ctypes.byref(ext), ctypes.byref(desc.main_desc), ctypes.c_uint64(N)) == INVALID
    desc, keep = C.plain_pair(S).build()           # no op 6: no ext needed
    assert check_with(hip_lib, "rec", desc, N, ext=False) == _lib.SP_OK
    assert check_with(hip_lib, "rec", desc, 4) == INVALID and "l = 3" in hip_lib.sp_last_error().decode()     # blocks of 8 rows on 4
    assert check_with(hip_lib, "rec", desc, 8) == _lib.SP_OK                                                    # the whole trace is one block
    with pytest.raises(ValueError, match="l = 3"):
        C.plain_pair(S).main.evaluate([[1]] * 4)


@pytest.mark.parametrize("kind", [air.AUX_FIBONACCI_RAP, air.AUX_CALLBACK])
def test_host_built_auxiliary_kinds_stay_unsupported(hip_lib, kind):
    desc, keep = C.plain_pair(S).build()
    desc.aux_kind = kind
    assert check_with(hip_lib, "rec", desc, N) == UNSUPPORTED and "aux_kind" in hip_lib.sp_last_error().decode()


def test_the_old_entry_points_refuse_both(hip_lib):
    """Kind 5 is an unknown kind and op 6 a malformed op everywhere but through the _rec entry points."""
    desc, keep = C.plain_pair(S).build()
    assert check_with(hip_lib, "", desc, N) == INVALID and "derived column 0 has an unknown kind" in hip_lib.sp_last_error().decode()
    for b in (mixed_builder(), mimc_builder()):
        desc, keep = b.build()
        assert check_with(hip_lib, "", desc, N) == INVALID and "malformed op" in hip_lib.sp_last_error().decode()
    # a row-local column that reads a periodic column, and no chain at all
    b = air.AirBuilder(2, [0], 1, periodic=[[1, 2]], main_inputs=1)
    b.main.value(b.main.load(0, 0) + b.main.periodic(1, 0))
    b.constraint(b.load(0, 0) - b.load(0, 0), degree=1, exemptions=0)
    desc, keep = b.build()
    assert air.needs_rec(desc) and check_with(hip_lib, "rec", desc, N) == _lib.SP_OK
    assert check_with(hip_lib, "", desc, N) == INVALID and "malformed op" in hip_lib.sp_last_error().decode()
    assert [int(r[1]) for r in b.main.evaluate([[10], [20], [30], [40]])] == [12, 21, 32, 41]


def test_null_arguments(hip_lib):
    desc, keep = C.plain_pair(S).build()
    n = ctypes.c_uint64(N)
    assert hip_lib.sp_air_main_check_rec(None, None, ctypes.byref(desc.main_desc), n) == INVALID
    assert hip_lib.sp_air_main_check_rec(ctypes.byref(desc), None, None, n) == INVALID
    assert hip_lib.sp_air_prove_rec(None, None, None, None, None, None, n, None, None, None) == INVALID
    assert hip_lib.sp_air_check_trace_rec(None, None, None, None, None, None, n, None, None, None, 0, None) == INVALID
    assert hip_lib.sp_air_main_trace_rec(None, None, None, None, None, n, None) == INVALID
    bad = air.ext_of(desc)
    bad.size -= 8
    assert hip_lib.sp_air_main_check_rec(ctypes.byref(desc), ctypes.byref(bad), ctypes.byref(desc.main_desc), n) == INVALID


def test_builder_keeps_a_group_closed_before_anything_else():
    b = air.AirBuilder(4, [0], 1, main_inputs=1)
    m = b.main
    g = m.chain(S, [m.load(0, 0), 7])
    assert g.cols == [1, 2] and g.period == S
    with pytest.raises(ValueError, match="a chain group is open"):
        m.value(m.load(0, 0))
    with pytest.raises(ValueError, match="a chain group is open"):
        m.chain(S, [1])
    with pytest.raises(ValueError, match="a chain group is open"):
        b.build()
    with pytest.raises(ValueError, match="at shift 0 only"):
        m.load(1, g.cols[0])
    with pytest.raises(ValueError, match="1 next values for a chain group of 2"):
        g.step([g.state(0)])
    g.step([g.state(0) * g.state(1), g.state(1) + 1])
    with pytest.raises(ValueError, match="closed already"):
        g.step([1, 2])
    m.value(m.load(3, g.cols[1]))                       # behind the group its columns are read as any other, at any shift
    b.constraint(b.load(0, 0) - b.load(0, 0), degree=1, exemptions=0)
    b.build()
    with pytest.raises(ValueError, match="not a power of two"):
        air.AirBuilder(3, [0], 1, main_inputs=1).main.chain(6, [1])
    with pytest.raises(ValueError, match="not a power of two"):
        air.AirBuilder(3, [0], 1, main_inputs=1).main.chain(1, [1])
    with pytest.raises(ValueError, match="17 columns"):
        air.AirBuilder(30, [0], 1, main_inputs=1).main.chain(S, [1] * 17)
    with pytest.raises(ValueError, match="not one of the AIR's 0 periodic columns"):
        air.AirBuilder(3, [0], 1, main_inputs=1).main.periodic(0, 0)
    with pytest.raises(ValueError, match="row shift 8"):
        air.AirBuilder(3, [0], 1, periodic=[[1, 2]], main_inputs=1).main.periodic(8, 0)


@pytest.mark.parametrize("n,s", [(64, 2), (64, 64), (128, 8)])
def test_evaluate_agrees_with_a_hand_written_double_loop(n, s):
    rng = random.Random(n + s)
    periodic = C.periodic_columns(rng)
    b, cols = C.mixed(s, periodic)
    rows = C.mixed_inputs(n, rng)
    got = [[int(x) for x in r] for r in b.main.evaluate(rows)]
    want = C.hand_table(rows, s, periodic)
    assert cols == {"x0": 2, "x1": 3, "x2": 4, "y0": 5, "y1": 6, "v": 7, "r": 8}
    for i in range(n):
        assert got[i] == want[i], i


def test_mimc_blocks_is_clean_and_names_what_breaks():
    rng = random.Random(21)
    b, rows, keys = C.mimc_case(N, S, rng)
    assert b.check_trace(rows) == []
    full = b.main.evaluate(rows)
    assert b.check_trace(full) == []                                          # the whole table, as ever
    for block in range(N // S):                                                # every block is the permutation of its own message
        x = rows[block * S][0]
        for t in range(S):
            assert int(full[block * S + t][1]) == x and int(full[block * S + t][2]) == pow(x + keys[t], 2, P)
            x = pow(x + keys[t], 3, P)
    digest = int(full[S - 1][1])
    assert digest == air.mimc_blocks_digest([rows[0][0]], S, keys)
    # a wrong public digest: the boundary constraint finds the true one on row s - 1
    wrong = air.mimc_blocks(N, S, keys, digest + 1)
    assert wrong.check_trace(rows) == [air.Violation(air.BOUNDARY, 0, 1, S - 1, S - 1, digest)]
    # a message tampered with behind the table's back: x - m on the block's first row, nothing else (x, q and the steps still agree)
    tampered = [[int(x) for x in r] for r in full]
    tampered[3 * S][0] = (tampered[3 * S][0] + 1) % P
    assert b.check_trace(tampered) == [air.Violation(air.TRANSITION, 2, 1, 3 * S, 3 * S, P - 1)]
    # the filler between the messages is free
    rows[5] = [12345]
    assert b.check_trace(rows) == []
    # the widened group of the benchmark
    b3, rows3, keys3 = C.mimc_case(N, S, rng, width=3)
    assert b3.main_cols == 7 and b3.check_trace(rows3) == []
    assert int(b3.main.evaluate(rows3)[S - 1][1]) == air.mimc_blocks_digest([rows3[0][0]], S, keys3, 3)
