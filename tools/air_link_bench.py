"""What a linked chain group saves on one shape: air.mimc_sponge at 2^log-n rows in blocks of --block rows and runs of --link blocks -
one input column (the messages), the sponge state as a one-column linked group and its square, 3 main columns in all - proved in one
process alternately (a) from the whole host table through sp_air_prove_ext and (b) from the input column through sp_air_prove_link,
--alternations times each after one warm-up of either.  Both give the same bytes (asserted).  Prints one JSON line: per side the
median wall time of a proof, sp_last_round_ms of the last one (rounds 1 - 4, device time) and sp_last_upload_stats of the last one
(its bytes uploaded); and the estimate the linked kernel's own time is to be held against, as tools/air_chain_bench.py has it for the
chain kernel: products per step x steps of a run x the time of one product of a wave that has its SIMD to itself
(profiles/r06_mul3_v2_ubench.txt: 211.34 G products/s over 1024 SIMDs of 64 lanes).  The kernel's own time is the
air_main_chain_kernel<PER, true> row of a kernel trace of this script, in a run of its own:

    python tools/air_link_bench.py [--log-n 18] [--block 64] [--link 8] [--alternations 5]
    rocprofv3 --kernel-trace --stats -d OUT -o p -- python tools/air_link_bench.py --alternations 1
    python tools/rocprof_summary.py OUT/.../p_results.db
"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from lambdaworks_cairo_prover_amd import _lib, air, api  # noqa: E402

PRODUCTS_PER_STEP = 2                              # (x + K)^3: two products
WAVE_PRODUCT_US = 1024 * 64 / 211.34e9 * 1e6       # one product of all 64 lanes on one SIMD: 0.31 us


def prove_ext(ctx, desc, full, opt):
    ext = air.ext_of(desc)
    c_opt = opt.to_c()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    _lib.check(_lib.load().sp_air_prove_ext(ctx._h, ctypes.byref(desc), ctypes.byref(ext), full.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            ctypes.c_uint64(full.shape[0]), ctypes.byref(c_opt), ctypes.byref(out), ctypes.byref(ln)))
    return ctx._take_proof(out, ln)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=18)
    ap.add_argument("--block", type=int, default=64)
    ap.add_argument("--link", type=int, default=8)
    ap.add_argument("--alternations", type=int, default=5)
    args = ap.parse_args()
    n, s, link, options = 1 << args.log_n, args.block, args.link, (4, 80, 3, 20)
    rng = random.Random(2026)
    keys = [rng.randrange(air.P) for _ in range(s)]
    rows = air.mimc_sponge_inputs(n, s, link, rng)
    b = air.mimc_sponge(n, s, link, keys, air.mimc_sponge_digest([rows[t * s][0] for t in range(link)], s, keys))
    desc, keep = b.build()
    assert air.route(desc, "prove")[0] == "sp_air_prove_link"
    inputs = air.ints_to_bytes(np.array(rows, dtype=object))
    t0 = time.perf_counter()
    table = b.main.evaluate(rows)                            # the integer model's table: what a caller computed on the host until now
    model_s = time.perf_counter() - t0
    full = air.ints_to_bytes(table)
    opt = api.ProofOptions(*options)
    sides = {"whole_table_ext": lambda ctx: prove_ext(ctx, desc, full, opt), "inputs_link": lambda ctx: ctx.air_prove(desc, inputs, opt)}
    result = {name: {"ms": []} for name in sides}
    with api.Context(device=0) as ctx:
        proof = None
        for name, call in sides.items():          # warm-up: the shape's set-up, first launches, the workspace
            p = call(ctx)
            assert proof is None or p == proof, "the two paths disagree"
            proof = p
        assert ctx.last_proof_info()["composition_path"] == 1, "the trace does not satisfy its constraints"
        for _ in range(args.alternations):
            for name, call in sides.items():
                t0 = time.perf_counter()
                p = call(ctx)
                result[name]["ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
                assert p == proof
                result[name]["last_round_ms"] = [round(x, 2) for x in ctx.last_round_ms()[1:]]
                result[name]["upload"] = ctx.last_upload_stats()
    for r in result.values():
        r["median_ms"] = round(statistics.median(r["ms"]), 2)
    steps = link * (s - 1)
    estimate = {"products_per_step": PRODUCTS_PER_STEP, "steps_of_a_run": steps, "wave_product_us": round(WAVE_PRODUCT_US, 3),
                "linked_kernel_us": round(PRODUCTS_PER_STEP * steps * WAVE_PRODUCT_US, 1), "lanes": n // (s * link), "waves": max(1, n // (s * link) // 64)}
    print(json.dumps({"tool": "air_link_bench", "rows": n, "block": s, "link": link, "main_cols": b.main_cols, "input_cols": 1, "options": options,
                      "alternations": args.alternations, "table_bytes": int(full.nbytes), "input_bytes": int(inputs.nbytes), "proof_bytes": len(proof),
                      "proof_sha256": hashlib.sha256(proof).hexdigest(), "host_model_s": round(model_s, 2), "estimate": estimate, **result}))


if __name__ == "__main__":
    main()
