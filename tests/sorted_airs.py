"""AIRs with sorted auxiliary columns (SP_AIR_AUX_SORTED) and their traces for the sorted-column tests: the two worked examples of
air.py with seeded traces that tie keys under different carried values, and a mixed AIR - two sort groups of different key widths, a
table read in a carried value, a product and a LogUp sum that read the sorted columns at shifts 0, 1 and 7, a product that reads none."""
import random

from lambdaworks_cairo_prover_amd import air

P = air.P
OPTION_SETS = [(4, 3, 3, 1), (8, 4, 3, 2)]
U64 = (1 << 64) - 1


def to_bytes(rows):
    return air.ints_to_bytes(rows)


def changed(rows, cell, to=None):
    """A copy of the trace rows with one cell changed (+1, or to the value `to`)."""
    out = [list(r) for r in rows]
    out[cell[0]][cell[1]] = (out[cell[0]][cell[1]] + 1) % P if to is None else to % P
    return out


def range_check(n, seed=11, key_bits=16):
    """(builder, rows): air.sorted_range_check of 40 000 .. 40 000 + n / 4 - 1 (both bytes of the 16-bit key vary), every value about
    four times, in a seeded order."""
    rng = random.Random(seed)
    lo, hi = 40000, 40000 + n // 4 - 1
    order = list(range(n))
    rng.shuffle(order)
    rows = air.sorted_range_check_trace(n, lo, hi, [rng.randrange(lo, hi + 1) for _ in range(n - (hi - lo + 1))], order)
    return air.sorted_range_check(n, lo, hi, key_bits), rows


def memory(n, seed=12, key_bits=64, first=None):
    """(builder, rows): air.memory_consistency over n / 4 random cells that end at the last 64-bit address (or start at `first`), every
    cell read about four times: tied addresses, whose value the sort must carry."""
    rng = random.Random(seed)
    cells = [rng.randrange(P) for _ in range(n // 4)]
    accesses = list(range(len(cells))) + [rng.randrange(len(cells)) for _ in range(n - len(cells))]
    rng.shuffle(accesses)
    first = U64 - len(cells) + 1 if first is None else first
    return air.memory_consistency(n, key_bits), air.memory_consistency_trace(n, first, cells, accesses)


def flipped_memory(rows):
    """(rows with the value of one access changed, the sorted row of that access): the access is one of several of its address."""
    by_addr = {}
    for i, (addr, _) in enumerate(rows):
        by_addr.setdefault(addr, []).append(i)
    addr, at = min((a, rs) for a, rs in by_addr.items() if len(rs) >= 3)
    row = at[1]                                            # neither the first nor the last access of its address
    position = sum(len(rs) for a, rs in by_addr.items() if a < addr) + 1
    return changed(rows, (row, 1)), position


MIXED_TABLE = 8


def mixed(n, seed=13):
    """(builder, rows).  Main columns a (a 16-bit key, 0 and 65535 among few values), k (a 64-bit key, 0 and 2^64 - 1 among few
    values), c, d (any field elements); periodic column 0 a table of 8 values that only the auxiliary program reads.  Auxiliary columns:
      0      z3' (gamma - k) = z3 (gamma - a)                      a product that reads no sorted column, declared first
      1 2    (a; c + T_(i+3)) by a, 16 key bits                    a table read in the carried value
      3 4 5  (k; c, d d) by k, 64 key bits
      6      z1' (gamma - s1[1]) = z1 (gamma - s1[0]) (gamma - s3[7])   a product over sorted columns at shifts 0, 1 and 7
      7      w' = w + (s2[0] + s4[1]) / (gamma - s5[7])                 a LogUp sum over sorted columns at shifts 0, 1 and 7
    with the last row exempt everywhere (s_j[r]: auxiliary column j, r rows ahead), z3_0 = z1_0 = 1, w_0 = 0."""
    rng = random.Random(seed)
    table = [rng.randrange(P) for _ in range(MIXED_TABLE)]
    b = air.AirBuilder(4, [0, 1, 7], 2, aux_cols=8, n_rap=1, aux_kind=air.AUX_PROGRAM, periodic=[table])
    m = b.main_cols
    gamma = b.rap(0)
    b.constraint(b.load(1, m + 0) * (gamma - b.load(0, 1)) - b.load(0, m + 0) * (gamma - b.load(0, 0)), degree=2, exemptions=1)
    b.constraint(b.load(1, m + 6) * (gamma - b.load(1, m + 1)) - b.load(0, m + 6) * (gamma - b.load(0, m + 1)) * (gamma - b.load(2, m + 3)),
                 degree=3, exemptions=1)
    b.constraint((b.load(1, m + 7) - b.load(0, m + 7)) * (gamma - b.load(2, m + 5)) - (b.load(0, m + 2) + b.load(1, m + 4)), degree=2, exemptions=1)
    b.boundary(m + 0, 0, 1); b.boundary(m + 6, 0, 1); b.boundary(m + 7, 0, 0)
    x = b.aux
    g = x.rap(0)
    a, k, c, d = (x.load(0, j) for j in range(4))
    x.product(g - a, g - k)
    s1, s2 = x.sorted(a, carry=[c + x.table(3, 0)], key_bits=16)
    s3, s4, s5 = x.sorted(k, carry=[c, d * d])
    x.product((g - x.sorted_load(0, s1)) * (g - x.sorted_load(7, s3)), g - x.sorted_load(1, s1))
    x.running_sum(x.sorted_load(0, s2) + x.sorted_load(1, s4), g - x.sorted_load(7, s5))
    assert [s1, s2, s3, s4, s5] == [1, 2, 3, 4, 5]
    small = [0, 65535, 255, 256, 257] + [rng.randrange(1 << 16) for _ in range(max(3, n // 8))]
    wide = [0, U64, 1 << 63, (1 << 32) - 1, 1 << 32] + [rng.randrange(1 << 64) for _ in range(max(3, n // 8))]
    rows = [[rng.choice(small), rng.choice(wide), rng.randrange(P), rng.randrange(P)] for _ in range(n)]
    for j, i in enumerate(rng.sample(range(n), 12)):       # both ends of both ranges, several times each
        rows[i][0], rows[i][1] = (0, 65535)[j % 2], (0, U64)[(j // 2) % 2]
    return b, rows
