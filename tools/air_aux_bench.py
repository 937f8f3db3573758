"""Wall time of a RAP AIR whose auxiliary columns are an aux program (tests/aux_program_airs.py): 2^18 rows, 64 main columns,
16 auxiliary columns (8 grand products with a denominator, 8 LogUp running sums with a denominator, row shifts 0 .. 7), blowup 4,
80 queries, grinding 20.  The same AIR two ways on one GPU: sp_air_prove_aux (the columns built on the device) and sp_air_prove
with aux_kind 2 (the columns built by the host callback: AuxProgram.evaluate, numpy object arrays of Python integers - one
vectorised operation per op over all rows, one batch inversion, the product scans row by row - then the row-major upload).
One warm-up proof each, then --reps timed proofs; prints one JSON line: medians and sp_last_round_ms of the last proof of
each side (rounds 1 - 4, device time).

    python tools/air_aux_bench.py [--reps 5] [--callback-reps 3] [--log-n 18]
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

import aux_program_airs as X  # noqa: E402
from lambdaworks_cairo_prover_amd import api  # noqa: E402


def timed(ctx, desc, trace, opt, reps):
    proof = ctx.air_prove(desc, trace, opt)            # warm-up: set-up of the shape, first launches
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        p = ctx.air_prove(desc, trace, opt)
        times.append((time.perf_counter() - t0) * 1e3)
        assert p == proof
    return proof, times, ctx.last_round_ms()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--callback-reps", type=int, default=3)
    ap.add_argument("--log-n", type=int, default=18)
    args = ap.parse_args()
    n, main_cols, options = 1 << args.log_n, 64, (4, 80, 3, 20)
    b = X.rap_air(n, perm_shifts=range(8), logup_shifts=range(8), extra_cols=main_cols - X.BASE_COLS)
    trace = X.main_trace(n, main_cols - X.BASE_COLS)
    desc, keep = b.build()
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=trace)
    opt = api.ProofOptions(*options)
    with api.Context(device=0) as ctx:
        proof, t_dev, r_dev = timed(ctx, desc, trace, opt, args.reps)
        cb_proof, t_cb, r_cb = timed(ctx, cb_desc, trace, opt, args.callback_reps)
    assert cb_proof == proof
    med = lambda t: round(statistics.median(t), 2)
    print(json.dumps({"tool": "air_aux_bench", "rows": n, "main_cols": main_cols, "aux_cols": len(b.aux.cols),
                      "aux_products": 8, "aux_sums": 8, "aux_ops": len(b.aux.ops), "transitions": len(b.degrees), "options": options,
                      "proof_bytes": len(proof), "same_bytes": cb_proof == proof,
                      "aux_program": {"median_ms": med(t_dev), "min_ms": round(min(t_dev), 2), "max_ms": round(max(t_dev), 2),
                                      "last_round_ms": [round(x, 2) for x in r_dev[1:]]},
                      "aux_callback": {"median_ms": med(t_cb), "min_ms": round(min(t_cb), 2), "max_ms": round(max(t_cb), 2),
                                       "last_round_ms": [round(x, 2) for x in r_cb[1:]]},
                      "speedup_median": round(statistics.median(t_cb) / statistics.median(t_dev), 2)}))


if __name__ == "__main__":
    main()
