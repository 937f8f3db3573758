"""The plain reference of main programs (program_ref.main_table) held to tables of 8 rows written out by hand, one per column kind 0 to
9: everything else - the Python model, the device - is compared against that reference, so the reference itself is anchored here.  The
programs are raw lists in the header's encoding (ops (op, a, b), cols (kind, num_op, den_op, pad)), written without the builder."""
from types import SimpleNamespace

import pytest

import program_ref as R
from program_ref import ADD, CONST, DIV, LOAD, MUL, NO_DEN, PERIODIC, SUB, P

N = 8


def program(input_cols, ops, cols, consts=(), periodic=()):
    return SimpleNamespace(input_cols=input_cols, ops=list(ops), consts=list(consts), cols=list(cols), periodic_cols=[list(v) for v in periodic])


def derived(prog, rows):
    """The derived columns alone, one list per column."""
    table = R.main_table(prog, rows)
    assert [r[:prog.input_cols] for r in table] == [[v % P for v in r] for r in rows]
    return [[r[prog.input_cols + k] for r in table] for k in range(len(prog.cols))]


def inv(x):
    return pow(x, P - 2, P)


def test_value_with_and_without_a_denominator():
    a = [3, 1, 4, 1, 5, 9, 2, 6]
    prog = program(1, [(LOAD, 0, 0), (LOAD, 1, 0), (CONST, 0, 0), (ADD, 0, 2), (MUL, 0, 1)],
                   [(R.VALUE, 4, NO_DEN, 0), (R.VALUE, 1, 3, 0)], consts=[7])
    plain, quotient = derived(prog, [[v] for v in a])
    assert plain == [3, 4, 4, 5, 45, 18, 12, 18]                           # a(i) a(i + 1), the last row wraps to row 0
    assert quotient == [1 * inv(10) % P, 4 * inv(8) % P, 1 * inv(11) % P, 5 * inv(8) % P, 9 * inv(12) % P, 2 * inv(16) % P, 6 * inv(9) % P, 3 * inv(13) % P]
    with pytest.raises(R.ZeroDenominator):
        R.main_table(prog, [[v] for v in a[:5] + [P - 7] + a[6:]])


def test_inv_or_zero():
    a = [0, 1, 2, 0, P - 1, 4, 0, 0]
    (col,) = derived(program(1, [(LOAD, 0, 0)], [(R.INV_OR_ZERO, 0, NO_DEN, 0)]), [[v] for v in a])
    assert col == [0, 1, (P + 1) // 2, 0, P - 1, inv(4), 0, 0]


def test_bit():
    a = [0, 1, 2, 3, 1 << 64, (1 << 64) - 1, 5 << 63, P - 1]
    low, high = derived(program(1, [(LOAD, 0, 0)], [(R.BIT, 0, NO_DEN, 0), (R.BIT, 0, NO_DEN, 64)]), [[v] for v in a])
    assert low == [0, 1, 0, 1, 0, 1, 0, 0]                                  # (P - 1 = 2^251 + 17 2^192 is even)
    assert high == [0, 0, 0, 0, 1, 0, 0, 0]                                 # (5 << 63 has bits 63 and 65)


def test_sum_and_product_are_exclusive_scans():
    a = [1, 2, 3, 4, 5, 6, 7, 8]
    total, product, halves = derived(program(1, [(LOAD, 0, 0), (CONST, 0, 0)], [(R.SUM, 0, NO_DEN, 0), (R.PRODUCT, 0, NO_DEN, 0), (R.SUM, 0, 1, 0)], consts=[2]),
                                     [[v] for v in a])
    assert total == [0, 1, 3, 6, 10, 15, 21, 28]
    assert product == [1, 1, 2, 6, 24, 120, 720, 5040]
    half = inv(2)
    assert halves == [0, half, 3 * half % P, 3, 5, 15 * half % P, 21 * half % P, 14]


def test_count_with_a_repeated_table_key():
    x = [5, 7, 5, 5, 9, 7, 5, 9]
    t = [7, 5, 7, 3, 9, 5, 5, 9]                                            # 7, 5 and 9 repeat; 3 is looked up by nobody
    prog = program(2, [(LOAD, 0, 0), (LOAD, 0, 1)], [(R.COUNT, 0, 1, 4)])
    (z,) = derived(prog, [list(r) for r in zip(x, t)])
    assert z == [2, 4, 0, 0, 2, 0, 0, 0]                                    # the first row of a key holds its whole count, the others zero
    for col in (0, 1):
        bad = [list(r) for r in zip(x, t)]
        bad[6][col] = 16
        with pytest.raises(R.KeyOutOfRange):
            R.main_table(prog, bad)


def test_fetch_whose_key_sits_on_two_rows():
    x = [4, 2, 4, 6, 2, 2, 6, 4]
    t = [2, 4, 6, 4, 0, 1, 3, 5]                                            # the key 4 sits on rows 1 and 3
    v = [10, 11, 12, 13, 14, 15, 16, 17]
    # op 3 = v + v is the fetched value: pad = key_bits + 256 value_op
    prog = program(3, [(LOAD, 0, 0), (LOAD, 0, 1), (LOAD, 0, 2), (ADD, 2, 2)], [(R.FETCH, 0, 1, 3 + 256 * 3)])
    (got,) = derived(prog, [list(r) for r in zip(x, t, v)])
    assert got == [22, 20, 22, 24, 20, 20, 24, 22]                          # 4 fetches row 1 (2 * 11), never row 3
    missing = [list(r) for r in zip(x, t, v)]
    missing[7][0] = 7
    with pytest.raises(R.MissingKey):
        R.main_table(prog, missing)
    both = [list(r) for r in missing]
    both[0][1] = 8                                                          # a table key out of range on a row before the missing one, and
    with pytest.raises(R.KeyOutOfRange):                                    # one behind it: the range comes first wherever it is broken
        R.main_table(prog, both)
    both = [list(r) for r in missing]
    both[7][1] = 8
    with pytest.raises(R.KeyOutOfRange):
        R.main_table(prog, both)


def test_limb_that_crosses_a_32_bit_boundary():
    a = [0x1_2345_6789, 0xFFFF_FFFF, 0x1_0000_0000, 0xABCD_EF01_2345_6789, (1 << 36) - (1 << 28), 1 << 35, P - 1, 0]
    crossing, top = derived(program(1, [(LOAD, 0, 0)], [(R.LIMB, 0, NO_DEN, 28 + 256 * 8), (R.LIMB, 0, NO_DEN, 192 + 256 * 60)]), [[v] for v in a])
    assert crossing == [0x12, 0x0F, 0x10, 0x12, 0xFF, 0x80, 0, 0]           # bits 28 .. 35
    assert top == [0, 0, 0, 0, 0, 0, (1 << 59) + 17, 0]                     # bits 192 .. 251 of P - 1 = 2^251 + 17 2^192


def test_word_of_each_function():
    x = [0b1100, 0xFF, 0, 0xF0, 0xAA, 1, 0x80, 0x7F]
    y = [0b1010, 0x0F, 0, 0x0F, 0x55, 1, 0x80, 0x80]
    prog = program(2, [(LOAD, 0, 0), (LOAD, 0, 1)], [(R.WORD, 0, 1, fn + 256 * 8) for fn in (R.AND, R.OR, R.XOR)])
    w_and, w_or, w_xor = derived(prog, [list(r) for r in zip(x, y)])
    assert w_and == [0b1000, 0x0F, 0, 0, 0, 1, 0x80, 0]
    assert w_or == [0b1110, 0xFF, 0, 0xFF, 0xFF, 1, 0x80, 0xFF]
    assert w_xor == [0b0110, 0xF0, 0, 0xFF, 0xFF, 0, 0, 0xFF]
    for col in (0, 1):
        bad = [list(r) for r in zip(x, y)]
        bad[7][col] = 0x100
        with pytest.raises(R.WordOutOfRange):
            R.main_table(prog, bad)


def test_unlinked_chain_group_with_a_periodic_read():
    a = [1, 2, 3, 4, 5, 6, 7, 8]
    k = [10, 20]
    # blocks of 4 rows (l = 2), two columns: the seeds are a and 1; the step is (x, y) -> (x + y + k(i), x)
    ops = [(LOAD, 0, 0), (CONST, 0, 0), (LOAD, 0, 1), (LOAD, 0, 2), (ADD, 2, 3), (PERIODIC, 0, 0), (ADD, 4, 5)]
    prog = program(1, ops, [(R.CHAIN, 6, 0, 2), (R.CHAIN, 2, 1, 2 + 256)], consts=[1], periodic=[k])
    x, y = derived(prog, [[v] for v in a])
    assert x == [1, 12, 33, 55, 5, 16, 41, 67]                              # 1 + 1 + 10, 12 + 1 + 20, 33 + 12 + 10; then 5 + 1 + 10, ..
    assert y == [1, 1, 12, 33, 1, 5, 16, 41]


def test_linked_chain_group_of_two_blocks_with_a_div_in_its_step():
    a = [2, 3, 4, 5, 6, 7, 8, 9]
    # blocks of 2 rows (l = 1) in runs of 2 blocks (k = 1): seed x = carry + a, step x -> x / a(i)
    ops = [(LOAD, 0, 1), (LOAD, 0, 0), (ADD, 0, 1), (DIV, 0, 1)]
    prog = program(1, ops, [(R.CHAIN, 3, 2, 1 + 65536)])
    (x,) = derived(prog, [[v] for v in a])
    # run 0: seed 0 + 2, step 2 / 2 = 1; seed 1 + 4 = 5, step 5 / 4.  run 1 starts from a zero carry again: 6, 6 / 6 = 1, 1 + 8 = 9, 9 / 8
    assert x == [2, 1, 5, 5 * inv(4) % P, 6, 1, 9, 9 * inv(8) % P]
    zero = [[v] for v in a]
    zero[2] = [0]                                                           # the divisor of the step out of row 2
    with pytest.raises(R.ZeroDenominator):
        R.main_table(prog, zero)
    zero = [[v] for v in a]
    zero[3] = [0]                                                           # no step divides by a(3): row 3 is the last of its block
    assert [r[1] for r in R.main_table(prog, zero)][:4] == [2, 1, 5, 5 * inv(4) % P]


def test_a_cell_read_before_it_is_built_and_an_unknown_kind_raise():
    with pytest.raises(ValueError, match="before it is built"):
        R.main_table(program(1, [(LOAD, 0, 2), (LOAD, 0, 0)], [(R.VALUE, 0, NO_DEN, 0), (R.VALUE, 1, NO_DEN, 0)]), [[1]] * N)
    with pytest.raises(ValueError, match="kind 10"):
        R.main_table(program(1, [(LOAD, 0, 0)], [(10, 0, NO_DEN, 0)]), [[1]] * N)
    assert SUB == 3 and MUL == 4                                            # (the op codes of the header)
