"""Linked chain groups in a main program (the k of a CHAIN column's pad, the _link entry points) without a GPU: the new symbols in the
header, the binding and the Rust block, the decoder's verdicts through sp_air_main_check_link - and the _rec and _lk entry points' on the
same descriptors -, the builder's mirror of them, and the Python-integer model (MainProgram.evaluate, AirBuilder.check_trace) against
hand-written plain loops and on air.mimc_sponge and air.merkle_paths.  Every comparison is exact."""
import ctypes
import os
import random
import re

import pytest

import chain_airs as C
import link_airs as L
from air_main_checks import _col, _first, _op, check_with, decoder_refuses_and_the_builder_raises
from lambdaworks_cairo_prover_amd import _lib, air, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = air.P
N, S, LINK = 64, 4, 4
LOG_S, LOG_LINK = 2, 2
PAD = LOG_S + 65536 * LOG_LINK
NEW_SYMBOLS = ("sp_air_prove_link", "sp_air_check_trace_link", "sp_air_main_trace_link", "sp_air_main_check_link", "sp_air_main_link_limits")
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
    assert api.air_main_link_limits() == {"link_log": 62, "width": 16} == {"link_log": air.MAIN_LINK_MAX_LOG, "width": air.MAIN_LINK_MAX_WIDTH}
    assert hip_lib.sp_air_main_link_limits(None) == INVALID


def mixed_builder():
    return L.mixed(S, LINK, L.periodic_columns(random.Random(3)))[0]


def sponge_builder():
    return L.sponge_case(N, S, LINK, random.Random(4))[0]


def merkle_builder():
    return L.merkle_case(N, S, LINK, random.Random(5))[0]


def test_the_helpers_and_the_examples_pass_the_decoder(hip_lib):
    for b in (mixed_builder(), sponge_builder(), merkle_builder(), L.plain_link(S, LINK), L.link_permutation(S, LINK)):
        desc, keep = b.build()
        assert air.needs_link(desc) and air.main_suffix(desc) == "link"
        assert check_with(hip_lib, "link", desc, N) == _lib.SP_OK, hip_lib.sp_last_error()
        api.air_main_check(desc, N)
        assert [air.route(desc, c)[0] for c in ("prove", "check_trace")] == ["sp_air_prove_link", "sp_air_check_trace_link"]
        assert not air.route(desc, "verify")[0].endswith("_link")


def test_the_suffix_is_link_only_where_a_descriptor_needs_it(hip_lib):
    for b, want in ((C.mimc_case(N, 8, random.Random(6))[0], "rec"), (air.table_lookup_main(N, [3, 5, 7, 11]), "lk"), (air.bit_range_check(N, 8), "main"),
                    (C.mixed(8, C.periodic_columns(random.Random(7)))[0], "rec")):
        desc, keep = b.build()
        assert not air.needs_link(desc) and air.main_suffix(desc) == want
        assert check_with(hip_lib, "link", desc, N) == _lib.SP_OK, hip_lib.sp_last_error()     # the _link entry points take what the others take
        del desc.main_features                                                               # a descriptor put together by hand is looked through
        assert not air.needs_link(desc) and air.main_suffix(desc) == want
    desc, keep = sponge_builder().build()
    del desc.main_features
    assert air.needs_link(desc) and air.main_suffix(desc) == "link"
    # a group opened with link=1 is today's group, bit for bit
    b = air.AirBuilder(3, [0], 1, main_inputs=1)
    g = b.main.chain(S, None, width=1, link=1)
    g.seed([b.main.load(0, 0)])
    g.step([g.state(0) * g.state(0)])
    assert b.main.cols[0][3] == LOG_S and not b.main.links


@pytest.mark.parametrize("suffix", ["rec", "lk"])
def test_the_entry_points_before_refuse_a_linked_descriptor_as_ever(hip_lib, suffix):
    """There the bits at and above 16 belong to j: a j out of sequence, with the code and the message of before."""
    for b in (sponge_builder(), mixed_builder()):
        desc, keep = b.build()
        assert check_with(hip_lib, suffix, desc, N) == INVALID
        message = hip_lib.sp_last_error().decode()
        assert message.startswith(f"sp_air_main_check_{suffix}: main program: derived column 0 is a CHAIN column with j = {256 * LOG_LINK} out of sequence "
                                  "(no group is open: j = 0 opens one)"), message
        with pytest.raises(ValueError, match=f"derived column 0 is a CHAIN column with j = {256 * LOG_LINK} out of sequence"):
            b.main.check(N, level=air.MainLevel[suffix.upper()])


# ---- the refusal table: the same mutation on the builder's lists (ops [(op, a, b)], cols [(kind, num_op, den_op, pad)]) and, through
# build(), on the C structs.  mixed: derived columns 0 .. 2 are group A (main columns 2 .. 4, linked), 3 and 4 group B (k = 0), 5 .. 20
# group C (linked), 21 the VALUE, 22 the SUM.
def is_load_x0(o):       # the first of them is the carry that the seed of x1 reads
    return o == (air.OP_LOAD, 0, 2)


def _all_of_group_a(pad):
    def mutate(m):
        for j in range(3):
            _col(j, pad=pad + 256 * j)(m)
    return mutate


def _step_reads_x0_at_a_shift(m):
    t = [t for t, o in enumerate(m.ops) if is_load_x0(o)][1]       # the second LOAD of x0 is the step's state
    m.ops[t] = (air.OP_LOAD, 1, 2)


def _seed_of_y1_is_the_state_of_y0(m):
    _col(4, den_op=_first(m, lambda o: o == (air.OP_LOAD, 0, 5)))(m)


REFUSALS = [
    # the new rules
    ("run-longer-than-n", _all_of_group_a(LOG_S + 65536 * 5), "derived column 0 is a CHAIN column with l + k = 7"),
    ("k-above-the-limit", _all_of_group_a(LOG_S + 65536 * 63), "derived column 0 is a CHAIN column with k = 63"),
    ("k-differs", _col(1, pad=LOG_S + 256 + 65536), "derived column 1 differs from its chain group in k"),
    ("seed-at-a-shift", _op(is_load_x0, a=1), "derived column 1 has a seed that loads derived column 0 of its own chain group at a shift other than 0"),
    ("seed-loads-its-group-k-0", _all_of_group_a(LOG_S), "derived column 0 has a seed that loads derived column 1 of its own chain group"),
    ("seed-of-the-unlinked-group", _seed_of_y1_is_the_state_of_y0, "derived column 4 has a seed that loads derived column 3 of its own chain group"),
    # rules of before, through the new entry point
    ("j-without-a-group", _col(0, pad=PAD + 256), "derived column 0 is a CHAIN column with j = 1 out of sequence"),
    ("j-skips", _col(2, pad=PAD + 256 * 3), "derived column 2 is a CHAIN column with j = 3 out of sequence"),
    ("l-zero", _col(0, pad=65536 * LOG_LINK), "derived column 0 is a CHAIN column with l = 0"),
    ("l-differs", _col(1, pad=1 + 256 + 65536 * LOG_LINK), "derived column 1 differs from its chain group in l"),
    ("step-at-a-shift", _step_reads_x0_at_a_shift, "has a step that loads derived column 0 of its own chain group at a shift other than 0"),
    ("seed-loads-a-later-column", _op(lambda o: o == (air.OP_LOAD, 3, 0), b=24), "reads derived column 22, which is not an earlier one"),
    ("no-seed", _col(0, den_op=air.AUX_NO_DEN), "derived column 0 is a CHAIN column without a seed"),
    ("kind-7", _col(21, kind=7), "derived column 21 has an unknown kind"),
]


@pytest.mark.parametrize("mutate,says", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_decoder_refuses_and_the_builder_raises(hip_lib, mutate, says):
    decoder_refuses_and_the_builder_raises(hip_lib, "link", mixed_builder, mutate, says, N, mirror=says.split(" (")[0])


def test_a_run_is_held_against_n(hip_lib):
    desc, keep = L.plain_link(S, LINK).build()
    assert check_with(hip_lib, "link", desc, 8) == INVALID and "l + k = 4" in hip_lib.sp_last_error().decode()      # runs of 16 rows on 8
    assert check_with(hip_lib, "link", desc, 16) == _lib.SP_OK                                                       # the whole trace is one run
    with pytest.raises(ValueError, match="l \\+ k = 4"):
        L.plain_link(S, LINK).main.evaluate([[1]] * 8)


def test_null_arguments(hip_lib):
    desc, keep = L.plain_link(S, LINK).build()
    n = ctypes.c_uint64(N)
    assert hip_lib.sp_air_main_check_link(None, None, ctypes.byref(desc.main_desc), n) == INVALID
    assert hip_lib.sp_air_main_check_link(ctypes.byref(desc), None, None, n) == INVALID
    assert hip_lib.sp_air_prove_link(None, None, None, None, None, None, n, None, None, None) == INVALID
    assert hip_lib.sp_air_check_trace_link(None, None, None, None, None, None, n, None, None, None, 0, None) == INVALID
    assert hip_lib.sp_air_main_trace_link(None, None, None, None, None, n, None) == INVALID
    bad = air.ext_of(desc)
    bad.size -= 8
    assert hip_lib.sp_air_main_check_link(ctypes.byref(desc), ctypes.byref(bad), ctypes.byref(desc.main_desc), n) == INVALID


def test_builder_takes_the_seeds_after_the_group_is_open():
    b = air.AirBuilder(4, [0], 1, main_inputs=1)
    m = b.main
    g = m.chain(S, None, width=2, link=LINK)
    assert g.cols == [1, 2] and g.period == S and g.link == LINK and m.links
    with pytest.raises(ValueError, match="a chain group is open"):
        m.value(m.load(0, 0))
    with pytest.raises(ValueError, match="no seeds yet"):
        g.state(0)
    with pytest.raises(ValueError, match="no seeds yet"):
        g.step([1, 2])
    with pytest.raises(ValueError, match="a seed reads its own chain group at shift 0 only"):
        m.load(1, g.cols[0])
    with pytest.raises(ValueError, match="1 seeds for a chain group of 2"):
        g.seed([g.carry(0)])
    g.seed([g.carry(1) + m.load(0, 0), g.carry(0) * 3])
    with pytest.raises(ValueError, match="only while the seeds"):
        g.carry(0)
    with pytest.raises(ValueError, match="has its seeds already"):
        g.seed([1, 2])
    g.step([g.state(0) * g.state(1), g.state(1) + 1])
    with pytest.raises(ValueError, match="only while the seeds"):
        g.carry(0)
    m.value(m.load(3, g.cols[1]))
    b.constraint(b.load(0, 0) - b.load(0, 0), degree=1, exemptions=0)
    b.build()
    fresh = lambda: air.AirBuilder(3, [0], 1, main_inputs=1).main
    with pytest.raises(ValueError, match="not a power of two"):
        fresh().chain(S, None, width=1, link=3)
    with pytest.raises(ValueError, match="needs width"):
        fresh().chain(S, None, link=2)
    with pytest.raises(ValueError, match="2 seeds for a chain group of width 1"):
        fresh().chain(S, [1, 2], width=1)
    m = fresh()
    g = m.chain(S, None, width=1)                        # the seeds afterwards, and no run: the carry is not there to be read
    with pytest.raises(ValueError, match="only in a linked group"):
        g.carry(0)
    m = air.AirBuilder(2, [0], 1, main_inputs=1).main
    g = m.chain(S, [m.load(0, 0)], link=2)               # the call form of before with runs: seeds that read no carry
    g.step([g.state(0) + 1])
    assert m.cols[0][3] == LOG_S + 65536 and m.links
    assert [int(r[1]) for r in m.evaluate([[i] for i in range(8)])] == [0, 1, 2, 3, 4, 5, 6, 7]


@pytest.mark.parametrize("n,s,link", [(64, 2, 2), (64, 8, 8), (64, 32, 2), (64, 4, 4)])
def test_evaluate_agrees_with_hand_written_plain_loops(n, s, link):
    rng = random.Random(n + s + link)
    periodic = L.periodic_columns(rng)
    b, cols = L.mixed(s, link, periodic)
    rows = L.mixed_inputs(n, rng)
    got = [[int(x) for x in r] for r in b.main.evaluate(rows)]
    want = L.hand_table(rows, s, link, periodic)
    assert cols == {"x0": 2, "x1": 3, "x2": 4, "y0": 5, "y1": 6, "z0": 7, "v": 23, "r": 24}
    for i in range(n):
        assert got[i] == want[i], i
    for first in range(0, n, s * link):                 # x2 = carry + 1: the carry in front of every run is zero
        assert got[first][cols["x2"]] == 1
    b, rows, keys = L.sponge_case(n, s, link, rng)
    assert [[int(x) for x in r] for r in b.main.evaluate(rows)] == L.sponge_table(rows, s, link, keys)


def test_mimc_sponge_is_clean_and_names_what_breaks():
    rng = random.Random(21)
    b, rows, keys = L.sponge_case(N, S, LINK, rng)
    assert b.check_trace(rows) == []
    full = [[int(x) for x in r] for r in b.main.evaluate(rows)]
    assert b.check_trace(full) == []                                           # the whole table, as ever
    run = S * LINK
    for first in range(0, N, run):                                              # every run is the sponge of its own messages
        assert full[first + run - 1][1] == air.mimc_sponge_digest([rows[first + t * S][0] for t in range(LINK)], S, keys)
    digest = full[run - 1][1]
    wrong = air.mimc_sponge(N, S, LINK, keys, digest + 1)
    assert wrong.check_trace(rows) == [air.Violation(air.BOUNDARY, 0, 1, run - 1, run - 1, digest)]
    # one digest cell changed behind the table's back: the last step of its block no longer leads to it
    tampered = [list(r) for r in full]
    tampered[2 * run - 1][1] = (tampered[2 * run - 1][1] + 1) % P
    found = b.check_trace(tampered)
    assert [(v.kind, v.index, v.first_row, v.last_row) for v in found] == [(air.TRANSITION, 0, 2 * run - 1, 2 * run - 1), (air.TRANSITION, 1, 2 * run - 2, 2 * run - 2)]
    # an inner block's last state changed: the step into it, and the absorb constraint out of it
    tampered = [list(r) for r in full]
    tampered[S - 1][1] = (tampered[S - 1][1] + 1) % P
    assert [(v.kind, v.index, v.first_row) for v in b.check_trace(tampered)] == [(air.TRANSITION, 0, S - 1), (air.TRANSITION, 1, S - 2), (air.TRANSITION, 2, S - 1)]
    # a message tampered with at a run start: x - m there, nothing else
    tampered = [list(r) for r in full]
    tampered[run][0] = (tampered[run][0] + 1) % P
    assert b.check_trace(tampered) == [air.Violation(air.TRANSITION, 3, 1, run, run, P - 1)]
    rows[5] = [12345]                                                           # the filler between the messages is free
    assert b.check_trace(rows) == []


def test_merkle_paths_is_clean_and_names_what_breaks():
    rng = random.Random(22)
    depth = LINK
    b, rows, keys, root = L.merkle_case(N, S, depth, rng)
    assert b.check_trace(rows) == []
    full = [[int(x) for x in r] for r in b.main.evaluate(rows)]
    run = S * depth
    for first in range(0, N, run):                                              # every run climbs its path to the one root
        cur = rows[first][0]
        for level in range(depth):
            _, sib, bit = rows[first + level * S]
            cur = air.merkle_paths_digest(sib, cur, S, keys) if bit else air.merkle_paths_digest(cur, sib, S, keys)
            assert full[first + level * S + S - 1][3] == cur
        assert cur == root
    wrong = air.merkle_paths(N, S, depth, keys, root + 1)
    assert wrong.check_trace(rows) == [air.Violation(air.TRANSITION, 8, N // run, run - 1, N - 1, P - 1)]
    # one digest cell changed: run 1's last row no longer holds the root (and the step into it breaks)
    tampered = [list(r) for r in full]
    tampered[2 * run - 1][3] = (tampered[2 * run - 1][3] + 1) % P
    found = b.check_trace(tampered)
    assert (air.TRANSITION, 8, 1, 2 * run - 1, 2 * run - 1, 1) in [tuple(v) for v in found]
    assert {v.index for v in found} == {0, 1, 8}
    # a direction that is no bit, a value on a later block start
    bad = [list(r) for r in rows]
    bad[S][2] = 2
    assert 7 in {v.index for v in b.check_trace(bad)}
    bad = [list(r) for r in rows]
    bad[S][0] = 9
    assert {v.index for v in b.check_trace(bad)} >= {3, 8}
