"""What a quotient in a chain step costs and saves on one shape: air.ec_subset_sum at 2^log-n rows in blocks of --block rows - one input
column (the bits), the accumulator and its slope as a chain group of three with one DIV a seed and one a step, two row-local VALUE
columns, 6 main columns in all - proved in one process alternately (a) from the whole host table through sp_air_prove_ext and (b) from
the input column through sp_air_prove_div, --alternations times each after one warm-up of either.  Both give the same bytes (asserted).
Prints one JSON line: per side the median wall time of a proof, sp_last_round_ms of the last one (rounds 1 - 4, device time) and
sp_last_upload_stats of the last one (its bytes uploaded); and the model the DIV kernel's own time is to be held against: rows of a
block x DIVs a step x the time of one fe_inv of a wave that has its SIMD to itself.  That last figure is measured, not assumed:
--inverse-wave runs nothing but batch inversions of 512 elements - 64 lanes of one work-group, each a chain of 8 elements around one
fe_inv (field_kernels.hip) -, whose batch_inverse_kernel row in a kernel trace is one such wave.  The DIV kernel's own time is the
air_main_chain_kernel<true, false, true> row of a kernel trace of this script.  Each trace in a run of its own:

    python tools/air_div_bench.py [--log-n 18] [--block 256] [--alternations 5]
    rocprofv3 --kernel-trace --stats -d OUT -o p -- python tools/air_div_bench.py --alternations 1
    rocprofv3 --kernel-trace --stats -d OUT2 -o p -- python tools/air_div_bench.py --inverse-wave
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

P = air.P
DIVS_PER_STEP = 1
# the Stark curve's generator (y^2 = x^3 + x + beta), as StarkWare publishes it; the points are 2 G, 4 G, .., the shift G + P_0 + P_1
G = (0x1ef15c18599971b7beced415a40f0c7deacfd9b0d1819e03d723d8bc943cfca, 0x5668060aa49730b7be4801df46ec62de53ecd11abe43a32873000c36e8dc1f)


def ec_double(p):
    lam = (3 * p[0] * p[0] + 1) * pow(2 * p[1], -1, P) % P
    x = (lam * lam - 2 * p[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def ec_add(p, q):
    lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x = (lam * lam - p[0] - q[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def prove_ext(ctx, desc, full, opt):
    ext = air.ext_of(desc)
    c_opt = opt.to_c()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    _lib.check(_lib.load().sp_air_prove_ext(ctx._h, ctypes.byref(desc), ctypes.byref(ext), full.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            ctypes.c_uint64(full.shape[0]), ctypes.byref(c_opt), ctypes.byref(out), ctypes.byref(ln)))
    return ctx._take_proof(out, ln)


def inverse_wave(reps):
    rng = random.Random(7)
    data = api.felts_to_bytes([1 + rng.randrange(P - 1) for _ in range(512)])
    with api.Context(device=0) as ctx:
        for _ in range(reps):
            out = ctx.batch_inverse(data)
    assert int.from_bytes(bytes(ctx_first(out)), "big") * int.from_bytes(bytes(ctx_first(data)), "big") % P == 1
    print(json.dumps({"tool": "air_div_bench", "mode": "inverse-wave", "elements": 512, "lanes": 64, "calls": reps}))


def ctx_first(a):
    return np.asarray(a, dtype=np.uint8).reshape(-1, 32)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=18)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--inverse-wave", action="store_true")
    args = ap.parse_args()
    if args.inverse_wave:
        return inverse_wave(20)
    n, s, options = 1 << args.log_n, args.block, (4, 80, 3, 20)
    rng = random.Random(2026)
    points, q = [], G
    for _ in range(s):
        q = ec_double(q)
        points.append(q)
    shift = ec_add(ec_add(G, points[0]), points[1])
    rows = air.ec_subset_sum_inputs(n, rng)
    b = air.ec_subset_sum(n, s, points, shift, air.ec_subset_sum_result([r[0] for r in rows[:s]], points, shift))
    desc, keep = b.build()
    assert air.route(desc, "prove")[0] == "sp_air_prove_div"
    inputs = air.ints_to_bytes(np.array(rows, dtype=object))
    t0 = time.perf_counter()
    table = b.main.evaluate(rows)                            # the integer model's table: what a caller computed on the host until now
    model_s = time.perf_counter() - t0
    full = air.ints_to_bytes(table)
    opt = api.ProofOptions(*options)
    sides = {"whole_table_ext": lambda ctx: prove_ext(ctx, desc, full, opt), "inputs_div": lambda ctx: ctx.air_prove(desc, inputs, opt)}
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
    model = {"rows_of_a_block": s, "divs_per_step": DIVS_PER_STEP, "inversions_of_a_lane": s * DIVS_PER_STEP, "lanes": n // s, "waves": max(1, n // s // 64),
             "div_kernel_us": "inversions_of_a_lane x the batch_inverse_kernel time of --inverse-wave"}
    print(json.dumps({"tool": "air_div_bench", "rows": n, "block": s, "main_cols": b.main_cols, "input_cols": 1, "options": options,
                      "alternations": args.alternations, "table_bytes": int(full.nbytes), "input_bytes": int(inputs.nbytes), "proof_bytes": len(proof),
                      "proof_sha256": hashlib.sha256(proof).hexdigest(), "host_model_s": round(model_s, 2), "model": model, **result}))


if __name__ == "__main__":
    main()
