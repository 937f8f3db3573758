"""Integer ops in chain steps on the device (sp_air_prove_int, sp_air_check_trace_int, sp_air_main_trace_int): the columns equal the
plain reference (int_chain_ref) and the Python-integer model cell for cell, and a proof from the input columns has the bytes of the
proof from the whole table through the entry points that existed before.  Every comparison is exact."""
import ctypes
import random

import pytest

import int_chain_programs as G
import int_chain_ref as R
import oracle_lib as O
from air_device_checks import OPTIONS, device_inputs_give_the_same_bytes, model_ints, prove_full, table_ints, three_calls, to_bytes, two_ranks_give_the_one_rank_bytes
from lambdaworks_cairo_prover_amd import _lib, air, api

pytestmark = pytest.mark.gpu
P = air.P
ARX_OPTIONS = (4, 4, 3, 2)      # (degree_bound_factor 2: the composition has 2n coefficients, which needs a blowup above 2)
OUT_OF_RANGE = "an integer op's operand is out of range on some row"


# ---- cell equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("div", [False, True], ids=["nodiv", "div"])
@pytest.mark.parametrize("periodic", [False, True], ids=["noper", "per"])
@pytest.mark.parametrize("n,s,link,width", [(64, 2, 1, 16), (64, 64, 1, 10), (64, 8, 4, 7), (4096, 4, 4, 3), (8192, 2, 2, 1)])
def test_table_equals_the_reference_and_the_model_cell_for_cell(hip_ctx, n, s, link, width, periodic, div):
    """(64, 2, 1): 32 lanes in a half-empty wave, one step a block, the full width of sixteen.  (64, 64, 1): one lane, the whole trace
    one block, the input read at shift 3 wraps on its last rows, ten columns - every LIMB immediate of EDGES.  (64, 8, 4): linked, seeds
    that read a carry through integer ops.  (4096, 4, 4): 256 lanes, four work-groups.  (8192, 2, 2): 2048 lanes, one column.  With and
    without op 6, with and without op 7 in the same group: the eight instantiations that know the integer ops.  Twice on one context
    with a polynomial-only program between: the kept workspace, and the launch with a null range flag."""
    seed = n + 8 * s + link + 2 * periodic + div
    rng = random.Random(seed)
    b = G.group(seed, s, link, G.periodic_columns(rng) if periodic else None, div, width)
    rows, want = G.inputs(b, n, rng)
    desc, keep = b.build()
    assert air.main_suffix(desc) == "int" and (air.OP_DIV in {o[0] for o in b.main.ops}) == div
    assert want == model_ints(b, rows)
    poly = G.poly_only(s)
    poly_desc, poly_keep = poly.build()
    poly_rows = [[r[0]] for r in rows]
    for attempt in range(2):
        got = hip_ctx.air_main_trace(desc, to_bytes(rows))
        assert got.shape == (n, b.main_cols, 32)
        got = table_ints(got)
        for i in range(n):
            assert got[i] == want[i], (attempt, i)
        assert table_ints(hip_ctx.air_main_trace(poly_desc, to_bytes(poly_rows))) == model_ints(poly, poly_rows)


# ---- the worked example ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,s", [(64, 8), (4096, 64)])
def test_arx_chain_table_proof_and_check(hip_ctx, n, s):
    """The proof from the two input columns has the bytes of the proof from the whole table through sp_air_prove_pub and
    sp_air_prove_ext.  (The CPU oracle's entry point takes no periodic columns and no strides, which arx_chain has: it proves plain_int
    below.)"""
    b, rows, keys, digest = G.arx_case(n, s, random.Random(40 + n))
    assert b.check_trace(rows) == []
    desc, keep = b.build()
    table = air.arx_chain_trace(rows, s, keys)
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == table == model_ints(b, rows)
    if n == 64:
        assert table == R.main_table(b.main, rows)
    options = api.ProofOptions(*ARX_OPTIONS)
    proof = hip_ctx.air_prove(desc, to_bytes(rows), options)
    assert api.air_verify(proof, desc, options)
    full = to_bytes(table)
    assert proof == prove_full(hip_ctx, desc, full, ARX_OPTIONS, "ext") == prove_full(hip_ctx, desc, full, ARX_OPTIONS, "pub")
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == proof      # the kept workspace, a second time
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), options) == []


def test_wrong_digest_is_proved_rejected_and_reported(hip_ctx):
    n, s = 64, 8
    wrong, rows, keys, digest = G.arx_case(n, s, random.Random(41), wrong=1)
    desc, keep = wrong.build()
    options = api.ProofOptions(*ARX_OPTIONS)
    proof = hip_ctx.air_prove(desc, to_bytes(rows), options)           # as the reference: a proof all the same ...
    assert not api.air_verify(proof, desc, options)                    # ... which no verifier accepts
    want = wrong.check_trace(rows)
    assert want == [air.Violation(air.BOUNDARY, 0, 1, s - 1, s - 1, digest)]
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), options) == want


# ---- proof bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("div", [False, True], ids=["nodiv", "div"])
@pytest.mark.parametrize("options", OPTIONS)
def test_plain_int_proof_bytes_equal_the_oracles(hip_ctx, oracle, options, div):
    """plain_int has no periodic column and no stride: the CPU oracle, which takes the descriptor alone, proves the same table."""
    n, s = 64, 4
    b = G.plain_int(s, div)
    rng = random.Random(8)
    rows = [[rng.randrange(P)] for _ in range(n)]
    assert b.check_trace(rows) == []
    desc, keep = b.build()
    want = R.main_table(b.main, rows)
    assert model_ints(b, rows) == want
    full = to_bytes(want)
    got = hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    assert got == prove_full(hip_ctx, desc, full, options, "pub") == prove_full(hip_ctx, desc, full, options, "ext")
    assert got == O.program_air_prove(desc, full, options)
    assert api.air_verify(got, desc, api.ProofOptions(*options))


def test_inputs_in_device_memory_give_the_same_bytes(hip_ctx):
    b, rows = G.arx_case(256, 8, random.Random(13))[:2]
    device_inputs_give_the_same_bytes(hip_ctx, b, rows, api.ProofOptions(*ARX_OPTIONS))


def test_a_program_without_integer_ops_gives_the_same_bytes_through_int(hip_ctx):
    """mimc_blocks (through _rec) and plain_div (through _div): the _int entry points take them, launch what their own level launches,
    and give its bytes."""
    import div_airs
    lib = _lib.load()
    rng = random.Random(17)
    keys = [rng.randrange(P) for _ in range(8)]
    mimc_rows = air.mimc_blocks_inputs(64, 8, rng)
    cases = [(air.mimc_blocks(64, 8, keys, air.mimc_blocks_digest([mimc_rows[0][0]], 8, keys)), mimc_rows, "rec", ARX_OPTIONS),
             (div_airs.plain_div(4), [[rng.randrange(P)] for _ in range(64)], "div", (4, 3, 3, 1))]
    for b, rows, suffix, options in cases:
        desc, keep = b.build()
        assert air.main_suffix(desc) == suffix
        want = hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
        ext, opt, a = air.ext_of(desc), api.ProofOptions(*options).to_c(), to_bytes(rows)
        out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
        _lib.check(lib.sp_air_prove_int(hip_ctx._h, ctypes.byref(desc), ctypes.byref(ext), None, ctypes.byref(desc.main_desc), a.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.c_uint64(len(rows)), ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln)))
        assert hip_ctx._take_proof(out, ln) == want, suffix
        table = (ctypes.c_uint8 * (len(rows) * b.main_cols * 32))()
        _lib.check(lib.sp_air_main_trace_int(hip_ctx._h, ctypes.byref(desc), ctypes.byref(ext), ctypes.byref(desc.main_desc), a.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.c_uint64(len(rows)), table))
        assert bytes(table) == hip_ctx.air_main_trace(desc, a).tobytes(), suffix


# ---- what is refused ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [1 << 251, P - 1], ids=["2^251", "p-1"])
def test_an_operand_out_of_range_is_invalid_arg_and_the_context_goes_on(hip_ctx, value):
    """The AND of range_case reads a(i + 1): one input cell on a row inside a block puts one operand of one lane's one step out of range.
    The same value on a block's first row, which the seed's LIMB alone reads, is no error.  With a zero denominator in the same program
    - a 7 on another block's first row - the range error is the one reported; the zero alone is SP_E_ZERO_INVERSE."""
    n, s, options = 64, 8, api.ProofOptions(4, 3, 3, 1)
    b = G.range_case(s)
    rng = random.Random(29)
    rows = [[rng.randrange(1 << 250)] for _ in range(n)]
    desc, keep = b.build()
    want = hip_ctx.air_prove(desc, to_bytes(rows), options)
    quiet = [list(r) for r in rows]
    quiet[s] = [value]
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(quiet))) == R.main_table(b.main, quiet)
    bad = [list(r) for r in rows]
    bad[s + 3] = [value]
    both = [list(r) for r in bad]
    both[2 * s] = [7]
    for data in (bad, both):
        for call in three_calls(hip_ctx, desc, data, options):
            with pytest.raises(api.SpError) as e:
                call()
            assert e.value.code == _lib.SP_E_INVALID_ARG and OUT_OF_RANGE in str(e.value), str(e.value)
        message = _lib.load().sp_last_error().decode()      # behind the callers' names the message begins with these words
        assert message[:message.index(OUT_OF_RANGE)].endswith(": ") and "(" not in message[:message.index(OUT_OF_RANGE)], message
    zero = [list(r) for r in rows]
    zero[2 * s] = [7]
    with pytest.raises(api.SpError) as e:
        hip_ctx.air_main_trace(desc, to_bytes(zero))
    assert e.value.code == _lib.SP_E_ZERO_INVERSE
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want


def test_malformed_program_is_refused_through_every_entry_point_and_the_context_goes_on(hip_ctx):
    n, s, options = 64, 4, api.ProofOptions(4, 3, 3, 1)
    rng = random.Random(30)
    rows = [[rng.randrange(P)] for _ in range(n)]
    b = G.plain_int(s)
    desc, keep = b.build()
    want = hip_ctx.air_prove(desc, to_bytes(rows), options)
    limb = next(t for t, o in enumerate(b.main.ops) if o[0] == air.OP_INT_LIMB)
    num_op = desc.main_desc.cols[2].num_op
    desc.main_desc.cols[2].num_op = limb               # the VALUE column behind the chain group, now N = an integer op
    for call in three_calls(hip_ctx, desc, rows, options):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == _lib.SP_E_INVALID_ARG and "derived column 2 depends on an integer op (ops 8 .. 11)" in str(e.value)
    desc.main_desc.cols[2].num_op = num_op
    saved = desc.main_desc.ops[limb].b
    desc.main_desc.ops[limb].b = 200 + 256 * 53
    for call in three_calls(hip_ctx, desc, rows, options):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == _lib.SP_E_INVALID_ARG and f"op {limb} is a LIMB op with lo + width = 253" in str(e.value)
    desc.main_desc.ops[limb].b = saved
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want
    # and through the entry points that were there before ops 8 .. 11 are the malformed ops they always were
    lib, opt = _lib.load(), options.to_c()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    a = to_bytes(rows)
    for name in ("sp_air_prove_main", "sp_air_prove_rec", "sp_air_prove_div", "sp_air_prove_fetch", "sp_air_prove_word"):
        rc = getattr(lib, name)(hip_ctx._h, ctypes.byref(desc), None, None, ctypes.byref(desc.main_desc), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n),
                                ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
        assert rc == _lib.SP_E_INVALID_ARG and f"malformed op {limb} " in lib.sp_last_error().decode(), name
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want


# ---- two ranks ------------------------------------------------------------------------------------------------------------------
def _rank_case(n, s):
    return G.arx_case(n, s, random.Random(31))


def test_two_ranks_give_the_one_rank_bytes(hip_ctx):
    """Every rank ingests the inputs and builds every column itself: no exchange before the commitment."""
    two_ranks_give_the_one_rank_bytes(hip_ctx, _rank_case, (4096, 8), ARX_OPTIONS)
