"""What one multiplicity column for several looked-up columns costs and saves, at 2^log-n rows, limb_bits 16, count 4, under blowup 4,
80 queries and grinding 20:

  proof   air.limb_range_check(n, 16, 4) from its input column through sp_air_prove_word (9 main + 4 auxiliary columns, four COUNT
          chunks) against air.limb_range_check_joint(n, 16, 4) through sp_air_prove_multi (6 + 3 columns, one joint chunk), in one
          process, --alternations times each after one warm-up of either.  TWO DIFFERENT STATEMENTS of one range check: the proofs
          differ, each side is held to its own warm-up proof, and both are verified once
  table   the main table of one of them alone (--which joint | word), three times through sp_air_main_trace_*: no proof, so that a
          kernel trace holds the column builders' kernels only.  --keys random: x uniform below 2^64; --keys zero: every x = 0, all
          4 n looked-up limbs on one table value
  regress programs without the feature, for the A/B of two builds in alternating processes (--package-root names the tree whose
          package is imported): --which lk: air.table_lookup_main(n, 2^16 values, 16) through sp_air_prove_lk; --which word:
          air.limb_range_check(n, 16, 4) through sp_air_prove_word; the 256-column shape without a main program is
          tools/air_wide_bench.py, which both trees have.  --alternations single proofs, each timed, and the proof's sha256

Prints one JSON line.

    python tools/air_multi_bench.py [--log-n 18] [--alternations 5] --part proof
    rocprofv3 --kernel-trace --stats -d OUT -o p -- python tools/air_multi_bench.py --part table --which joint --keys zero
    python tools/rocprof_summary.py OUT/.../p_results.db
    python tools/air_multi_bench.py --part regress --which lk --package-root /path/to/the/other/tree
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
LIMB_BITS, COUNT = 16, 4


def timed_proofs(ctx, call, alternations):
    proof = call(ctx)            # warm-up: the shape's set-up, first launches, the workspace
    assert ctx.last_proof_info()["composition_path"] == 1, "the trace does not satisfy its constraints"
    ms, rounds = [], []
    for _ in range(alternations):
        t0 = time.perf_counter()
        p = call(ctx)
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        assert p == proof
        rounds.append([round(x, 2) for x in ctx.last_round_ms()[1:]])
    return proof, ms, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=18)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--part", choices=("proof", "table", "regress"), default="proof")
    ap.add_argument("--which", choices=("joint", "word", "lk"), default="joint")
    ap.add_argument("--keys", choices=("random", "zero"), default="random")
    ap.add_argument("--package-root", default=ROOT)
    args = ap.parse_args()
    if args.part == "regress" and args.which not in ("lk", "word"):
        ap.error("--part regress takes --which lk or --which word: programs without the feature")
    if args.part == "table" and args.which not in ("joint", "word"):
        ap.error("--part table takes --which joint or --which word")
    sys.path.insert(0, args.package_root)
    import numpy as np
    from lambdaworks_cairo_prover_amd import air, api

    def to_bytes(rows):
        return air.ints_to_bytes(np.array(rows, dtype=object))

    n, options = 1 << args.log_n, (4, 80, 3, 20)
    opt = api.ProofOptions(*options)
    rng = random.Random(2032)
    top = 1 << (LIMB_BITS * COUNT)
    xs = [[rng.randrange(top) if args.keys == "random" else 0] for _ in range(n - 1)] + [[0]]     # (the joint statement's padding row)
    inputs = to_bytes(xs)
    out = {"tool": "air_multi_bench", "package": os.path.dirname(os.path.abspath(air.__file__)), "rows": n, "limb_bits": LIMB_BITS, "count": COUNT,
           "options": options, "alternations": args.alternations, "part": args.part, "keys": args.keys}

    def statement(which):
        if which == "joint":
            b = air.limb_range_check_joint(n, LIMB_BITS, COUNT)
        elif which == "word":
            b = air.limb_range_check(n, LIMB_BITS, COUNT)
        else:
            b = air.table_lookup_main(n, list(range(1 << LIMB_BITS)), LIMB_BITS)
        desc, keep = b.build()
        return b, desc, keep

    with api.Context(device=0) as ctx:
        if args.part == "proof":
            sides = {}
            for which in ("word", "joint"):
                b, desc, keep = statement(which)
                sides[which] = (b, desc, keep, {"entry": air.route(desc, "prove")[0], "main_cols": b.main_cols, "aux_cols": b.aux_cols, "input_bytes": int(inputs.nbytes),
                                                "ms": [], "round_ms": []})
            proofs = {}
            for which, (b, desc, keep, r) in sides.items():         # warm-up of either, and the one verification
                proofs[which] = ctx.air_prove(desc, inputs, opt)
                assert ctx.last_proof_info()["composition_path"] == 1, which
                assert api.air_verify(proofs[which], desc, opt), which
            for _ in range(args.alternations):
                for which, (b, desc, keep, r) in sides.items():
                    t0 = time.perf_counter()
                    p = ctx.air_prove(desc, inputs, opt)
                    r["ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
                    assert p == proofs[which]
                    r["round_ms"].append([round(x, 2) for x in ctx.last_round_ms()[1:]])
                    r["upload"] = ctx.last_upload_stats()
            for which, (b, desc, keep, r) in sides.items():
                r["median_ms"] = round(statistics.median(r["ms"]), 2)
                r["median_round1_ms"] = round(statistics.median(x[0] for x in r["round_ms"]), 2)
                r["proof_bytes"], r["proof_sha256"] = len(proofs[which]), hashlib.sha256(proofs[which]).hexdigest()
                out[which] = r
        if args.part == "table":
            b, desc, keep = statement(args.which)
            ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                table = ctx.air_main_trace(desc, inputs)
                ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            head = [[int(v) for v in r] for r in air.trace_to_ints(table[:4])]
            out["table"] = {"which": args.which, "entry": air.route(desc, "prove")[0].replace("prove", "main_trace"), "main_cols": b.main_cols, "calls": 3,
                            "main_trace_ms": ms, "first_rows": head}
        if args.part == "regress":
            b, desc, keep = statement(args.which)
            data = inputs if args.which == "word" else to_bytes([[x[0] & ((1 << LIMB_BITS) - 1)] for x in xs])
            proof, ms, rounds = timed_proofs(ctx, lambda c: c.air_prove(desc, data, opt), args.alternations)
            out["regress"] = {"which": args.which, "entry": air.route(desc, "prove")[0], "ms": ms, "median_ms": round(statistics.median(ms), 2), "min_ms": min(ms),
                              "max_ms": max(ms), "round1_ms": [r[0] for r in rounds], "proof_bytes": len(proof), "proof_sha256": hashlib.sha256(proof).hexdigest()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
