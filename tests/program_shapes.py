"""The deterministic shape cases of test_gpu_air_program_fuzz.py: the smallest programs that reach the seams of the host scheduler
(csrc/prover_programs.cpp: commit_aux_program, build_main_program) which no size of the fuzzed programs reaches.  Builders and inputs only; what
each is held against stands in the test.  test_air_program_fuzz.py checks on the CPU that each shape cuts the way it is meant to."""
import numpy as np

import lookup_airs as L
from lambdaworks_cairo_prover_amd import air

P = air.P
U64 = (1 << 64) - 1


def field_bytes(rng, n):
    """n random field elements below 2^250 as (n, 32) canonical big-endian bytes (rng: numpy Generator)."""
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 0] &= 3
    return a


def word_bytes(values, width):
    """Unsigned integers below 2^(8 width), width <= 8, as (n, 32) canonical big-endian bytes."""
    out = np.zeros((len(values), 32), dtype=np.uint8)
    out[:, 24:] = np.asarray(values, dtype=np.uint64).astype(">u8").view(np.uint8).reshape(-1, 8)
    assert width <= 8 and not out[:, :32 - width].any()
    return out


# ---- (e) the slot file ---------------------------------------------------------------------------------------------------------
def slot_file_sum(p, live):
    """In program p (a MainProgram or an AuxProgram over one column): x = cell (i, 0), y = cell (i + 1, 0), v_k = x + k y for
    k = 1 .. live - 2, all of them read again by the sum that is returned - (x + y) + sum_k v_k -, so that `live` values are alive when
    the last v is made; and right there one value nobody reads (x y), which the host must drop: it has no slot left for it."""
    x, y = p.load(0, 0), p.load(1, 0)
    v = [x + y]
    for _ in range(live - 3):
        v.append(v[-1] + y)
    _dead = x * y
    s = x + y
    for t in v:
        s = s + t
    return s


def slot_file_expected(rows, live):
    n = len(rows)
    return [(rows[i][0] + rows[(i + 1) % n][0] + sum(rows[i][0] + k * rows[(i + 1) % n][0] for k in range(1, live - 1))) % P for i in range(n)]


def slot_file_main(live):
    """One input column, one VALUE column: slot_file_sum."""
    b = air.AirBuilder(2, [0], 1, main_inputs=1)
    b.main.value(slot_file_sum(b.main, live))
    return L.trivial(b)


def slot_file_aux(live):
    """One main column, one running sum of slot_file_sum (the challenge is read by the constraint program only)."""
    b = air.AirBuilder(1, [0], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM)
    b.aux.running_sum(slot_file_sum(b.aux, live))
    return L.trivial(b)


# ---- (a) more auxiliary columns than a chunk holds ---------------------------------------------------------------------------
AUX_SEAM_N, AUX_SEAM_COLS = 1 << 16, 66


def aux_chunk_seam():
    """66 auxiliary columns at 2^16 rows, where a chunk holds 64: columns 0 .. 63 read main columns 0 and 1, columns 64 and 65 main
    columns 2 and 3; 62 and 64 are products with a D, 63 and 65 sums with a D, the others running sums without."""
    b = air.AirBuilder(4, [0], 1, aux_cols=AUX_SEAM_COLS, n_rap=2, aux_kind=air.AUX_PROGRAM)
    x = b.aux
    g, d = x.rap(0), x.rap(1)
    for k in range(AUX_SEAM_COLS):
        c0, c1 = (0, 1) if k < 64 else (2, 3)
        if k in (62, 64):
            x.product(x.load(0, c0) + g, x.load(k % 8, c1) + d)
        elif k in (63, 65):
            x.running_sum(x.load(1, c0) * g, x.load(0, c1) + d + k)
        else:
            x.running_sum(x.load(k % 8, c0) * (k + 1) + g * x.load(0, c1))
    return L.trivial(b)


def aux_chunk_seam_trace(seed=66):
    rng = np.random.default_rng(seed)
    return np.stack([field_bytes(rng, AUX_SEAM_N) for _ in range(4)], axis=1)


# ---- (b) a sort group whose carried values need a second pass ----------------------------------------------------------------
SORT_PASS_N, SORT_PASS_CARRIED = 1 << 16, 65


def second_sort_pass():
    """Auxiliary columns 0 .. 65: main column 0 as a 16-bit key and 65 carried values (j + 1) a + c + j of main columns 1 and 2 - a
    pass carries 64 -; 66, 67: main column 3 as a 64-bit key and one carried value; 68: a product that reads the key, carried columns
    63 and 64 of the first pass and 65 of the second, and the second group's carried column."""
    b = air.AirBuilder(4, [0], 1, aux_cols=SORT_PASS_CARRIED + 4, n_rap=1, aux_kind=air.AUX_PROGRAM)
    x = b.aux
    a, c = x.load(0, 1), x.load(0, 2)
    first = x.sorted(x.load(0, 0) + 0, [a * (j + 1) + c + j for j in range(SORT_PASS_CARRIED)], 16)
    second = x.sorted(x.load(0, 3) + 0, [x.load(1, 1)], 64)
    assert first == list(range(66)) and second == [66, 67]
    g = x.rap(0)
    x.product(x.sorted_load(0, 0) + g * x.sorted_load(1, 63) + x.sorted_load(2, 64) * x.sorted_load(0, 65) + x.sorted_load(3, 67) + g)
    return L.trivial(b)


def second_sort_pass_trace(seed=65):
    """16-bit keys with many ties and both ends of the range; 64-bit keys with 0 and 2^64 - 1 several times."""
    rng = np.random.default_rng(seed)
    n = SORT_PASS_N
    k16 = rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
    k64 = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * 2 + rng.integers(0, 2, size=n, dtype=np.uint64)
    for i, v in ((0, 0xFFFF), (5, 0), (2047, 0), (2048, 0xFFFF), (n - 1, 0)):
        k16[i] = v
    for i, v in ((1, U64), (7, 0), (4095, U64), (4096, 0), (n - 1, U64), (n - 2, 0)):
        k64[i] = v
    return np.stack([word_bytes(k16, 2), field_bytes(rng, n), field_bytes(rng, n), word_bytes(k64, 8)], axis=1)


# ---- (c) the scan of the block totals with two totals a thread ----------------------------------------------------------------
SCAN_TOTALS_N = 1 << 20


def scan_totals():
    """One input column a; a running sum of a, a product of a + 1, a running sum of a / (a + 3): one chunk, one run of three scanned
    columns of 512 blocks of 2048 rows each - the 256 threads that scan the block totals take two each."""
    b = air.AirBuilder(4, [0], 1, main_inputs=1)
    m = b.main
    m.running_sum(m.load(0, 0))
    m.product(m.load(0, 0) + 1)
    m.running_sum(m.load(0, 0), m.load(0, 0) + 3)
    return L.trivial(b)


def scan_totals_input(n=SCAN_TOTALS_N):
    """Every block of 2048 rows has a pattern of its own (step and offset from the block's number), values 1 .. 251."""
    i = np.arange(n, dtype=np.uint64)
    block = i >> np.uint64(11)
    return (np.uint64(1) + (block * np.uint64(37) + (i & np.uint64(2047)) * (block % np.uint64(7) + np.uint64(1))) % np.uint64(251)).astype(np.uint64)


def scan_totals_expected(a):
    """(n, 4, 32) bytes: the input, then the three columns by one loop each in Python integers (the inverses of the at most 251
    denominators from a dictionary)."""
    n = len(a)
    values = [int(v) for v in a]
    inv = {v: pow(v + 3, P - 2, P) for v in set(values)}
    sums = np.concatenate([[0], np.cumsum(a[:-1], dtype=np.uint64)]).astype(np.uint64)       # below 2^28
    prod, quot, z, s = [], [], 1, 0
    for v in values:
        prod.append(z)
        quot.append(s)
        z = z * (v + 1) % P
        s = (s + v * inv[v]) % P
    as_bytes = lambda column: np.frombuffer(b"".join(v.to_bytes(32, "big") for v in column), dtype=np.uint8).reshape(n, 32)
    return np.stack([word_bytes(a, 8), word_bytes(sums, 8), as_bytes(prod), as_bytes(quot)], axis=1)


# ---- (d) the two-level batch inversion over the columns of a chunk -------------------------------------------------------------
BATCH_INVERSE_N = 4096
BATCH_INVERSE_ZERO_ROWS = (0, 255, 256, 4095)


def batch_inverse_columns(count):
    """Inputs a, z (zero on BATCH_INVERSE_ZERO_ROWS) and d; `count` <= 16 inverted columns in one chunk, numbered 16 - count .. 15:
    j = 0 (mod 3) a VALUE (a + j) / (a a + j + 1), j = 1 a SUM of (j + 2) a / (a + 7 j + 1), j = 2 an INV_OR_ZERO of z (a + j); the
    last one, 15, is the VALUE (a + 15) / d.  16 columns of 4096 rows are 2^16 elements: the two-level form; 15 the one-level form."""
    b = air.AirBuilder(3 + count, [0], 1, main_inputs=3)
    m = b.main
    for j in range(16 - count, 16):
        a = m.load(0, 0)
        if j == 15:
            m.value(a + j, m.load(0, 2))
        elif j % 3 == 0:
            m.value(a + j, a * a + (j + 1))
        elif j % 3 == 1:
            m.running_sum(a * (j + 2), a + (7 * j + 1))
        else:
            m.inv_or_zero(m.load(0, 1) * (a + j))
    return L.trivial(b)


def batch_inverse_inputs(rng, zero_d_on_last_row=False):
    """rng: random.Random."""
    n = BATCH_INVERSE_N
    rows = [[rng.randrange(P), rng.randrange(1, P), rng.randrange(1, P)] for _ in range(n)]
    for i in BATCH_INVERSE_ZERO_ROWS:
        rows[i][1] = 0
    if zero_d_on_last_row:
        rows[n - 1][2] = 0
    return rows
