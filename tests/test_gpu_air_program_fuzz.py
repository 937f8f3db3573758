"""Randomized main and auxiliary programs on the device against the plain reference of program_ref.py, and the deterministic shape cases
of program_shapes.py, which reach the seams of the host scheduler (csrc/prover_programs.cpp: build_main_program, commit_aux_program) that no
fuzzed size does.  Every comparison is exact; a refusal of a generated program (SP_E_UNSUPPORTED, anything) is a failure.

Main programs: sp_air_main_trace* equals the reference cell for cell.  Auxiliary programs: the reference's columns under fixed
challenges ride as extra main columns E_k of an AIR with one constraint aux_k - E_k a column, and sp_air_check_trace* must find nothing
- and, with one E cell changed, exactly that constraint on that row -; for some seeds the proof of the device-built columns has the
bytes of the proof of the same AIR through a callback that evaluates the Python model.

Every case's id names its seeds: `pytest tests/test_gpu_air_program_fuzz.py -k seed017` runs the cases that hold seed 17 and, on a
difference, names the seed, the row, the column and its kind.  `python -c "import program_fuzz as F; print(F.describe_main(17, 64))"`
(from tests/) prints the program."""
import functools
import random

import numpy as np
import pytest

import program_fuzz as F
import program_ref as R
import program_shapes as S
from lambdaworks_cairo_prover_amd import _lib, air, api

pytestmark = pytest.mark.gpu
P = air.P
OPTIONS = api.ProofOptions(4, 3, 3, 1)
WIDE_OPTIONS = api.ProofOptions(2, 3, 3, 0)          # the 2^16-row shapes: blowup 2
MAIN_KINDS = ["VALUE", "INV_OR_ZERO", "BIT", "SUM", "PRODUCT", "CHAIN", "COUNT"]
AUX_KINDS = ["PRODUCT", "SUM", "SORTED"]
MAIN_LIVE_ERROR = "main program: more than 64 values alive at once"
AUX_LIVE_ERROR = "aux program: more than 64 values alive at once"


def to_bytes(rows):
    return air.ints_to_bytes(np.array(rows, dtype=object))


def as_int(cell):
    return int.from_bytes(bytes(cell), "big")


def batches(seeds, size):
    return [tuple(seeds[i:i + size]) for i in range(0, len(seeds), size)]


def batch_id(value):
    return "-".join(f"seed{s:03d}" for s in value) if isinstance(value, tuple) else f"n{value}"


def large_small(seeds, size_of):
    """The seeds in an order that alternates large and small programs."""
    rest, out = sorted(seeds, key=size_of), []
    while rest:
        out.append(rest.pop())
        if rest:
            out.append(rest.pop(0))
    return out


# ---- main programs ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_case(seed, n):
    b, rows, _ = F.random_main(seed, n)
    desc, keep = b.build()
    return b, desc, keep, to_bytes(rows), to_bytes(F.main_table(seed, n))


def main_table_is_the_reference(ctx, seed, n):
    b, desc, keep, inputs, want = main_case(seed, n)
    got = ctx.air_main_trace(desc, inputs)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        i, c = (int(v) for v in np.argwhere((got != want).any(axis=2))[0])
        kind = "input" if c < b.main.input_cols else MAIN_KINDS[b.main.cols[c - b.main.input_cols][0]]
        pytest.fail(f"main seed {seed}, n = {n}: row {i}, column {c} ({kind}): got {as_int(got[i, c])}, want {as_int(want[i, c])}")


@pytest.mark.parametrize("seeds", batches(F.MAIN_SEEDS, 8), ids=batch_id)
@pytest.mark.parametrize("n", [8, 64], ids=batch_id)
def test_main_programs_equal_the_reference(hip_ctx, n, seeds):
    """n = 8: one partly filled wave in every launch (the entry point takes 8 rows: it has no minimum above 2); 64: one wave.  Twice through
    the batch: the second time every program finds the workspace and the upload block another program left."""
    order = large_small(seeds, lambda s: len(F.random_main(s, n)[0].main.ops))
    for seed in order + order:
        main_table_is_the_reference(hip_ctx, seed, n)


@pytest.mark.parametrize("n,seed", [(n, s) for n in (2048, 4096) for s in F.MAIN_SEEDS_LARGE[n]], ids=lambda v: f"n{v}" if v > 999 else f"seed{v:03d}")
def test_large_main_programs_equal_the_reference(hip_ctx, n, seed):
    """2048 rows: exactly one scan block and one sort tile; 4096: two of each.  A small program of another seed runs in between."""
    main_table_is_the_reference(hip_ctx, seed, n)
    main_table_is_the_reference(hip_ctx, F.MAIN_SEEDS[seed % len(F.MAIN_SEEDS)], 64)
    main_table_is_the_reference(hip_ctx, seed, n)


@pytest.mark.parametrize("seed", F.MAIN_SEEDS_LARGE[16384], ids=lambda s: f"seed{s:03d}")
def test_main_programs_at_16384_rows_equal_the_model(hip_ctx, seed):
    """Two segments of the radix sort's histogram scan.  The expectation is MainProgram.evaluate, which test_air_program_fuzz.py holds
    to the reference at 8, 64 and 256 rows."""
    n = 16384
    main_table_is_the_reference(hip_ctx, seed, n)
    main_table_is_the_reference(hip_ctx, F.MAIN_SEEDS[seed % len(F.MAIN_SEEDS)], 8)
    main_table_is_the_reference(hip_ctx, seed, n)


def test_two_of_the_16384_row_seeds_hold_count_columns():
    with_count = [s for s in F.MAIN_SEEDS_LARGE[16384] if any(c[0] == air.MAIN_COUNT for c in F.random_main(s, 16384)[0].main.cols)]
    assert len(with_count) >= 2, with_count


# ---- auxiliary programs: the reference's columns pinned by constraints -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pinned_case(seed, n):
    b, rows, rap = F.pinned_aux(seed, n)
    desc, keep = b.build()
    return b, desc, keep, rows, to_bytes(rows), rap


def aux_columns_are_the_reference(ctx, seed, n, changed=False):
    b, desc, keep, rows, trace, rap = pinned_case(seed, n)
    K = len(b.aux.cols)
    M = b.main_cols - K
    found = ctx.air_check_trace(desc, trace, rap=rap)
    if found:
        v = found[0]
        pytest.fail(f"aux seed {seed}, n = {n}: auxiliary column {v.index} ({AUX_KINDS[b.aux.cols[v.index][0]]}) differs on {v.rows} rows, first on row "
                    f"{v.first_row}: got - want = {v.value}, want {rows[v.first_row][M + v.index]} ({len(found)} columns differ)")
    if changed:       # one E cell changed: exactly that constraint, on that row
        k, r = (7 * seed + 3) % K, (0, n - 1, n // 2 + 1)[seed % 3]
        bad = trace.copy()
        bad[r, M + k] = np.frombuffer(((rows[r][M + k] + 1) % P).to_bytes(32, "big"), dtype=np.uint8)
        assert ctx.air_check_trace(desc, bad, rap=rap) == [air.Violation(air.TRANSITION, k, 1, r, r, P - 1)], (seed, n, k, r)


@pytest.mark.parametrize("seeds", batches(F.AUX_SEEDS, 8), ids=batch_id)
def test_aux_programs_equal_the_reference(hip_ctx, seeds):
    n = 64
    order = large_small(seeds, lambda s: len(F.random_aux(s, n)[0].aux.ops))
    for seed in order:
        aux_columns_are_the_reference(hip_ctx, seed, n, changed=True)
    for seed in order:
        aux_columns_are_the_reference(hip_ctx, seed, n)


@pytest.mark.parametrize("n,seed", [(n, s) for n in (2048, 4096, 16384) for s in F.AUX_SEEDS_LARGE[n]], ids=lambda v: f"n{v}" if v > 999 else f"seed{v:03d}")
def test_large_aux_programs_equal_the_reference(hip_ctx, n, seed):
    """2048 rows: one scan block, one sort tile; 4096: two; 16384 (against AuxProgram.evaluate, which the CPU tests hold to the
    reference): two segments of the histogram scan.  A small program of another seed runs in between."""
    aux_columns_are_the_reference(hip_ctx, seed, n, changed=True)
    aux_columns_are_the_reference(hip_ctx, F.AUX_SEEDS[(seed + 5) % len(F.AUX_SEEDS)], 64)
    aux_columns_are_the_reference(hip_ctx, seed, n)


def same_proof_as_the_callback(ctx, b, trace, options, again=False):
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=trace)
    want = ctx.air_prove(cb_desc, trace, options)
    desc, keep = b.build()
    got = ctx.air_prove(desc, trace, options)
    assert got == want
    if again:
        assert ctx.air_prove(desc, trace, options) == want      # the kept workspace, a second time
    assert api.air_verify(got, desc, options)
    return desc, want


@pytest.mark.parametrize("n,seeds", [(64, tuple(F.AUX_SEEDS[:6])), (256, tuple(F.AUX_SEEDS[6:10]))], ids=batch_id)
def test_aux_programs_prove_as_the_callback(hip_ctx, n, seeds):
    for seed in seeds:
        b, rows, _ = F.random_aux(seed, n)
        same_proof_as_the_callback(hip_ctx, b, to_bytes(rows), OPTIONS)


# ---- the deterministic shapes -------------------------------------------------------------------------------------------------------
def test_aux_chunk_seam(hip_ctx):
    """(a) 66 auxiliary columns at 2^16 rows: the second chunk of commit_aux_program starts at column 64, with tables of its own, in
    the workspace the first left."""
    same_proof_as_the_callback(hip_ctx, S.aux_chunk_seam(), S.aux_chunk_seam_trace(), WIDE_OPTIONS, again=True)


def test_second_sort_pass(hip_ctx):
    """(b) 65 carried values at 2^16 rows: the second pass of the group takes no key and gathers by the first pass's order."""
    same_proof_as_the_callback(hip_ctx, S.second_sort_pass(), S.second_sort_pass_trace(), WIDE_OPTIONS)


def test_scan_totals_two_a_thread(hip_ctx):
    """(c) 2^20 rows: 512 scan blocks, so every thread of the scan over the block totals takes two (per = 2)."""
    a = S.scan_totals_input()
    want = S.scan_totals_expected(a)
    desc, keep = S.scan_totals().build()
    got = hip_ctx.air_main_trace(desc, np.ascontiguousarray(want[:, :1, :]))
    for c, name in ((0, "input"), (1, "SUM"), (2, "PRODUCT"), (3, "SUM with D")):
        if not np.array_equal(got[:, c], want[:, c]):
            i = int(np.argwhere((got[:, c] != want[:, c]).any(axis=1))[0][0])
            pytest.fail(f"column {c} ({name}): row {i} (scan block {i // 2048}): got {as_int(got[i, c])}, want {as_int(want[i, c])}")


def test_batch_inversion_across_columns(hip_ctx):
    """(d) 16 inverted columns of 4096 rows are one batch of 2^16 elements - the two-level form, a thread's elements 4096 apart, one in
    every column, some of them guarded zeros -, 15 the one-level form; a zero D on the last row of the last column is
    SP_E_ZERO_INVERSE, and the context goes on."""
    rng = random.Random(16)
    good = S.batch_inverse_inputs(rng)
    bad = [list(row) for row in good]
    bad[S.BATCH_INVERSE_N - 1][2] = 0
    good_bytes, bad_bytes = to_bytes(good), to_bytes(bad)
    whole = to_bytes(R.main_table(S.batch_inverse_columns(16).main, good))
    for count in (16, 15):
        b = S.batch_inverse_columns(count)
        desc, keep = b.build()
        # no column reads another, and the 15 are the last 15 of the 16 (test_air_program_fuzz.py holds that to the reference)
        want = whole if count == 16 else np.ascontiguousarray(np.delete(whole, 3, axis=1))
        assert np.array_equal(hip_ctx.air_main_trace(desc, good_bytes), want), count
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_main_trace(desc, bad_bytes)
        assert e.value.code == _lib.SP_E_ZERO_INVERSE and "denominator is zero" in str(e.value), count
        assert np.array_equal(hip_ctx.air_main_trace(desc, good_bytes), want), count


def test_main_program_fills_the_slot_file(hip_ctx):
    """(e) 64 values alive at once and a dead one right there: the reference's table.  65: refused by name, and the context goes on."""
    n = 64
    rows = [[5 + 3 * i * i] for i in range(n)]
    b = S.slot_file_main(64)
    desc, keep = b.build()
    want = R.main_table(b.main, rows)
    assert [r[1] for r in want] == S.slot_file_expected(rows, 64)
    assert np.array_equal(hip_ctx.air_main_trace(desc, to_bytes(rows)), to_bytes(want))
    over, over_keep = S.slot_file_main(65).build()
    for call in (lambda: hip_ctx.air_main_trace(over, to_bytes(rows)), lambda: hip_ctx.air_prove(over, to_bytes(rows), OPTIONS)):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == _lib.SP_E_UNSUPPORTED and MAIN_LIVE_ERROR in str(e.value), str(e.value)
    assert api.air_verify(hip_ctx.air_prove(desc, to_bytes(rows), OPTIONS), desc, OPTIONS)
    assert np.array_equal(hip_ctx.air_main_trace(desc, to_bytes(rows)), to_bytes(want))


def test_aux_program_fills_the_slot_file(hip_ctx):
    n = 64
    rows = [[7 + i * i * i] for i in range(n)]
    trace = to_bytes(rows)
    b = S.slot_file_aux(64)
    terms = S.slot_file_expected(rows, 64)
    assert [r[0] for r in R.aux_table(b.aux, rows, [3], [])] == [sum(terms[:i]) % P for i in range(n)]
    desc, want = same_proof_as_the_callback(hip_ctx, b, trace, OPTIONS)
    over, over_keep = S.slot_file_aux(65).build()
    for call in (lambda: hip_ctx.air_prove(over, trace, OPTIONS), lambda: hip_ctx.air_check_trace(over, trace, rap=[3])):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == _lib.SP_E_UNSUPPORTED and AUX_LIVE_ERROR in str(e.value), str(e.value)
    assert hip_ctx.air_prove(desc, trace, OPTIONS) == want
