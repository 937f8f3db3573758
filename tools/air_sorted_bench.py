"""Round 1 of the AIRs with sorted auxiliary columns on one GPU: air.memory_consistency at 2^log-n rows with 64 and with 16 key bits
(eight and two passes of the radix sort), next to air.table_lookup (one LogUp sum, no sort) and air.fibonacci_2_columns (two main
columns, no auxiliary segment at all) at the same size.  All four have two main columns, so round 1 differs by the auxiliary segment
alone: its columns (3, 3, 1, 0), their transform and commitment, and what builds them.  One warm-up proof each, then --reps timed
proofs; prints one JSON line: per shape the median wall time, the median of sp_last_round_ms[1] (round 1, device time) and the proof's sha256.

    python tools/air_sorted_bench.py [--reps 7] [--log-n 18]
"""
import argparse
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lambdaworks_cairo_prover_amd import air, api  # noqa: E402

P = air.P


def memory(n, key_bits):
    """air.memory_consistency over n / 4 cells, every one read about four times in a seeded order; the addresses end at 2^key_bits - 1."""
    rng = random.Random(18)
    cells = [rng.randrange(P) for _ in range(n // 4)]
    accesses = list(range(len(cells))) + [rng.randrange(len(cells)) for _ in range(n - len(cells))]
    rng.shuffle(accesses)
    return air.memory_consistency(n, key_bits), air.memory_consistency_trace(n, (1 << key_bits) - len(cells), cells, accesses)


def lookup(n, period=64):
    table = [7 + 3 * j for j in range(period)]
    return air.table_lookup(n, table), air.table_lookup_trace(n, table, [table[(5 * i + 3) % period] for i in range(n)])


def fibonacci(n):
    rows, a, b = [], 1, 1
    for _ in range(n):
        rows.append([a, b])
        a, b = (a + b) % P, (a + 2 * b) % P
    return air.fibonacci_2_columns(), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log-n", type=int, default=18)
    args = ap.parse_args()
    n, options = 1 << args.log_n, (4, 80, 3, 20)
    if n >> 16 > 4:
        raise SystemExit("memory_consistency with 16 key bits holds at most 2^16 cells: --log-n 18 at the most")
    opt = api.ProofOptions(*options)
    shapes = [("memory_consistency_64", *memory(n, 64)), ("memory_consistency_16", *memory(n, 16)), ("table_lookup_64", *lookup(n)),
              ("fibonacci_2_columns", *fibonacci(n))]
    out = {"tool": "air_sorted_bench", "rows": n, "options": options, "reps": args.reps}
    with api.Context(device=0) as ctx:
        for name, b, rows in shapes:
            desc, keep = b.build()
            trace = air.ints_to_bytes(rows)
            proof = ctx.air_prove(desc, trace, opt)            # warm-up: set-up of the shape, first launches
            assert api.air_verify(proof, desc, opt), name
            wall, round1 = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                assert ctx.air_prove(desc, trace, opt) == proof
                wall.append((time.perf_counter() - t0) * 1e3)
                round1.append(ctx.last_round_ms()[1])
            out[name] = {"aux_cols": b.aux_cols, "wall_median_ms": round(statistics.median(wall), 2), "round1_median_ms": round(statistics.median(round1), 3),
                         "round1_min_ms": round(min(round1), 3), "round1_max_ms": round(max(round1), 3), "proof_sha256": hashlib.sha256(proof).hexdigest()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
