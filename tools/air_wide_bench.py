"""Wall time of sp_air_prove on one fixed wide shape (tests/many_column_air.py): 256 main columns, 2^18 rows, blowup 4, 80 queries,
grinding 20, 64 transition constraints each tying together 4 column recurrences, 512 boundary constraints on 64 distinct rows
(--boundary-rows 3: the same 512 folded onto 3 rows, which prices the many-row boundary path).  One warm-up proof, then --reps
timed proofs on one GPU; prints one JSON line: the median and sp_last_round_ms of the last proof (rounds 1 - 4, device time).
--periodic K --period P: the same shape with K periodic columns of period P (sp_air_prove_periodic): column j < K counts up by
k_j + Q_j(i mod P), so its recurrence reads periodic column j, and the boundary values follow the changed trace.
--stride K: every second constraint (1, 3, ...) enforced on the rows = 0 (mod K) only (sp_air_prove_ext; one stride class).  The trace
is the same - it satisfies them on every row -, so the figure prices the class's tables and the strided terms of the composition.
--lookup P: another shape altogether - air.table_lookup (two main columns, one auxiliary column, a public table of P values as periodic
column 0) on 2^log-n rows through sp_air_prove_pub: round 1 (last_round_ms[0]) then holds the auxiliary program that reads the table.
proof_sha256 lets two builds be held against each other byte for byte.

    python tools/air_wide_bench.py [--boundary-rows 64] [--reps 5] [--log-n 18] [--periodic 8 --period 64] [--stride 8] [--lookup 64]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import many_column_air as M  # noqa: E402
from lambdaworks_cairo_prover_amd import air, api  # noqa: E402


def build_periodic(n, cols, n_transitions, boundary_rows, boundary_total, k_periodic, period):
    """The shape of M.build with x_j(i + 1) = x_j(i) + k_j + Q_j(i mod period) for the first k_periodic columns; (builder, trace)."""
    q = [[(5 * j + 3 * t * t + 1) % 1000 for t in range(period)] for j in range(k_periodic)]
    b = air.AirBuilder(cols, [0, 1], 1, periodic=q)
    groups = [[] for _ in range(n_transitions)]
    for j in range(cols):
        groups[j % n_transitions].append(j)
    for g in groups:
        acc = None
        for j in g:
            rec = b.load(1, j) - b.load(0, j) - M.column_step(j)
            if j < k_periodic:
                rec = rec - b.periodic(0, j)
            w = j % 5 + 1
            term = rec if w == 1 else rec * w
            acc = term if acc is None else acc + term
        b.constraint(acc, 1, 1)
    trace = M.main_trace(n, cols)
    values = {}
    for j in range(k_periodic):
        bump = np.concatenate(([0], np.cumsum(np.tile(np.array(q[j], dtype=np.uint64), n // period))[:-1])).astype(np.uint64)
        col = np.uint64(M.column_start(j)) + np.arange(n, dtype=np.uint64) * np.uint64(M.column_step(j)) + bump
        trace[:, j, 24:] = col.astype(">u8").view(np.uint8).reshape(n, 8)
        values[j] = col
    for col, step in M.boundary_list(n, cols, boundary_rows, boundary_total):
        b.boundary(col, step, int(values[col][step]) if col in values else M.cell(step, col))
    return b, trace


def build_lookup(n, period):
    """air.table_lookup over the table 7, 10, 13, ... with row i looking up entry (5 i + 3) mod period; (builder, trace)."""
    table = [7 + 3 * j for j in range(period)]
    pick = (5 * np.arange(n, dtype=np.uint64) + 3) % np.uint64(period)
    cells = np.stack([np.uint64(7) + np.uint64(3) * pick, np.bincount(pick.astype(np.int64), minlength=n).astype(np.uint64)], axis=1)
    trace = np.zeros((n, 2, 32), dtype=np.uint8)
    trace[:, :, 24:] = cells.astype(">u8").view(np.uint8).reshape(n, 2, 8)
    return air.table_lookup(n, table), trace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boundary-rows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log-n", type=int, default=18)
    ap.add_argument("--periodic", type=int, default=0, help="periodic columns read by the first recurrences (0: the plain shape)")
    ap.add_argument("--period", type=int, default=64)
    ap.add_argument("--stride", type=int, default=0, help="put every second constraint on the rows = 0 (mod K) (0: none)")
    ap.add_argument("--lookup", type=int, default=0, help="air.table_lookup against a table of this many values instead of the wide shape (0: the wide shape)")
    args = ap.parse_args()
    n, cols, options = 1 << args.log_n, 256, (4, 80, 3, 20)
    if args.lookup:
        b, trace = build_lookup(n, args.lookup)
        cols = b.main_cols
    elif args.periodic:
        b, trace = build_periodic(n, cols, 64, args.boundary_rows, 512, args.periodic, args.period)
    else:
        b = M.build(n, cols, n_transitions=64, boundary_row_count=args.boundary_rows, boundary_total=512)
        trace = M.main_trace(n, cols)
    if args.stride:
        b.strides = [(args.stride, 0) if k % 2 else (1, 0) for k in range(len(b.degrees))]
    desc, keep = b.build()
    opt = api.ProofOptions(*options)
    with api.Context(device=0) as ctx:
        proof = ctx.air_prove(desc, trace, opt)            # warm-up: set-up of the shape, first launches
        assert ctx.last_proof_info()["composition_path"] == 1, "the trace does not satisfy its constraints"
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            p = ctx.air_prove(desc, trace, opt)
            times.append((time.perf_counter() - t0) * 1e3)
            assert p == proof
        rounds = ctx.last_round_ms()
    print(json.dumps({"tool": "air_wide_bench", "rows": n, "main_cols": cols, "transitions": len(b.degrees), "ops": len(b.ops),
                      "constants": len(b.consts), "boundary_constraints": len(b.bcs), "boundary_rows": args.boundary_rows,
                      "periodic_columns": args.periodic, "period": args.period if args.periodic else 0, "stride": args.stride, "lookup": args.lookup,
                      "options": options, "proof_bytes": len(proof), "proof_sha256": hashlib.sha256(proof).hexdigest(), "median_ms": round(statistics.median(times), 2),
                      "min_ms": round(min(times), 2), "max_ms": round(max(times), 2), "last_round_ms": [round(x, 2) for x in rounds[1:]]}))


if __name__ == "__main__":
    main()
