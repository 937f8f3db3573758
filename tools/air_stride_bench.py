"""What a stride buys: air.strided_mimc_chain (a squaring round on the rows = 0 (mod 4), the rows between free) proved in both of its
statements on one GPU - the stride (4, 0), and the [1, 0, 0, 0] selector column with the declared degree 3 it needs.  The trace is
the same for both.  One warm-up proof each, then --reps timed proofs; prints one JSON line per statement: median wall time,
composition_path and sp_last_round_ms of the last proof (rounds 1 - 4, device time).  Both proofs are verified.

    python tools/air_stride_bench.py [--log-n 18] [--reps 7] [--blowup 4]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=18)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--blowup", type=int, default=4, help="the whole domain is blowup / 2 times the 2n points")
    args = ap.parse_args()
    n, options = 1 << args.log_n, (args.blowup, 80, 3, 20)
    rng = random.Random(7)
    keys = [rng.randrange(air.P) for _ in range(8)]
    trace = air.ints_to_bytes(air.strided_mimc_chain_trace(n, 3, keys, lambda: rng.randrange(air.P)))
    opt = api.ProofOptions(*options)
    with api.Context(device=0) as ctx:
        for statement, selector in (("stride (4, 0)", False), ("selector [1, 0, 0, 0]", True)):
            b = air.strided_mimc_chain(n, 3, keys, selector=selector)
            desc, keep = b.build()
            proof = ctx.air_prove(desc, trace, opt)            # warm-up: set-up of the shape, first launches
            path = ctx.last_proof_info()["composition_path"]
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                p = ctx.air_prove(desc, trace, opt)
                times.append((time.perf_counter() - t0) * 1e3)
                assert p == proof
            rounds = ctx.last_round_ms()
            assert api.air_verify(proof, desc, opt), statement
            print(json.dumps({"tool": "air_stride_bench", "statement": statement, "rows": n, "declared_degree": b.degrees[0],
                              "degree_bound_factor": 2, "options": options, "composition_path": path, "proof_bytes": len(proof),
                              "proof_sha256": hashlib.sha256(proof).hexdigest(), "median_ms": round(statistics.median(times), 2),
                              "min_ms": round(min(times), 2), "max_ms": round(max(times), 2),
                              "last_round_ms": [round(x, 2) for x in rounds[1:]]}), flush=True)


if __name__ == "__main__":
    main()
