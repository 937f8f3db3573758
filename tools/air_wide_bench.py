"""Wall time of sp_air_prove on one fixed wide shape (tests/many_column_air.py): 256 main columns, 2^18 rows, blowup 4, 80 queries,
grinding 20, 64 transition constraints each tying together 4 column recurrences, 512 boundary constraints on 64 distinct rows
(--boundary-rows 3: the same 512 folded onto 3 rows, which prices the many-row boundary path).  One warm-up proof, then --reps
timed proofs on one GPU; prints one JSON line: the median and sp_last_round_ms of the last proof (rounds 1 - 4, device time).

    python tools/air_wide_bench.py [--boundary-rows 64] [--reps 5] [--log-n 18]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import many_column_air as M  # noqa: E402
from lambdaworks_cairo_prover_amd import api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boundary-rows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log-n", type=int, default=18)
    args = ap.parse_args()
    n, cols, options = 1 << args.log_n, 256, (4, 80, 3, 20)
    b = M.build(n, cols, n_transitions=64, boundary_row_count=args.boundary_rows, boundary_total=512)
    desc, keep = b.build()
    trace = M.main_trace(n, cols)
    opt = api.ProofOptions(*options)
    with api.Context(device=0) as ctx:
        proof = ctx.air_prove(desc, trace, opt)            # warm-up: set-up of the shape, first launches
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            p = ctx.air_prove(desc, trace, opt)
            times.append((time.perf_counter() - t0) * 1e3)
            assert p == proof
        rounds = ctx.last_round_ms()
    print(json.dumps({"tool": "air_wide_bench", "rows": n, "main_cols": cols, "transitions": len(b.degrees), "ops": len(b.ops),
                      "constants": len(b.consts), "boundary_constraints": len(b.bcs), "boundary_rows": args.boundary_rows,
                      "options": options, "proof_bytes": len(proof), "median_ms": round(statistics.median(times), 2),
                      "min_ms": round(min(times), 2), "max_ms": round(max(times), 2), "last_round_ms": [round(x, 2) for x in rounds[1:]]}))


if __name__ == "__main__":
    main()
