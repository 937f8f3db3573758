"""What a device-built lookup multiplicity saves on one shape: air.table_lookup_main at 2^log-n rows with a table of 2^log-table entries
and --key-bits key bits - one input column (the looked-up values), the multiplicity column, the LogUp running sum as the auxiliary
column - proved in one process alternately (a) from the whole host table (air.table_lookup_trace, both main columns) through
sp_air_prove_pub and (b) from the input column through sp_air_prove_lk, --alternations times each after one warm-up of either.  Both
give the same bytes (asserted).  Prints one JSON line: per side the wall time of every proof and their median, sp_last_round_ms of the
last one (rounds 1 - 4, device time) and sp_last_upload_stats of the last one (its bytes uploaded).  The kernels' own times - the two
key passes (air_aux_sort_terms_*), the radix passes (rs_hist_kernel, rs_scatter_kernel and the scan's kernels) and air_main_count_kernel -
are their rows of a kernel trace of this script:

    python tools/air_lookup_bench.py [--log-n 18] [--log-table 16] [--key-bits 16] [--alternations 3]
    rocprofv3 --kernel-trace --stats -d OUT -o p -- python tools/air_lookup_bench.py --alternations 1
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


def prove_pub(ctx, desc, full, opt):
    ext = air.ext_of(desc)
    c_opt = opt.to_c()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    _lib.check(_lib.load().sp_air_prove_pub(ctx._h, ctypes.byref(desc), ctypes.byref(ext), None, full.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            ctypes.c_uint64(full.shape[0]), ctypes.byref(c_opt), ctypes.byref(out), ctypes.byref(ln)))
    return ctx._take_proof(out, ln)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=18)
    ap.add_argument("--log-table", type=int, default=16)
    ap.add_argument("--key-bits", type=int, default=16)
    ap.add_argument("--alternations", type=int, default=3)
    args = ap.parse_args()
    n, entries, options = 1 << args.log_n, 1 << args.log_table, (4, 80, 3, 20)
    if args.log_table > args.key_bits or entries > n:
        raise SystemExit("the table's distinct entries need log-table <= key-bits and at most n of them")
    rng = random.Random(2026)
    table = rng.sample(range(1 << args.key_bits), entries)
    b = air.table_lookup_main(n, table, args.key_bits)
    rows = air.table_lookup_main_inputs(n, table, rng)
    desc, keep = b.build()
    assert air.route(desc, "prove")[0] == "sp_air_prove_lk"
    inputs = air.ints_to_bytes(np.array(rows, dtype=object))
    t0 = time.perf_counter()
    whole = air.table_lookup_trace(n, table, [r[0] for r in rows])     # what a caller computed on the host until now
    host_s = time.perf_counter() - t0
    full = air.ints_to_bytes(np.array(whole, dtype=object))
    opt = api.ProofOptions(*options)
    sides = {"whole_table_pub": lambda ctx: prove_pub(ctx, desc, full, opt), "inputs_lk": lambda ctx: ctx.air_prove(desc, inputs, opt)}
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
    print(json.dumps({"tool": "air_lookup_bench", "rows": n, "table_entries": entries, "key_bits": args.key_bits, "radix_passes": (args.key_bits + 7) // 8,
                      "main_cols": b.main_cols, "input_cols": 1, "options": options, "alternations": args.alternations, "table_bytes": int(full.nbytes),
                      "input_bytes": int(inputs.nbytes), "host_multiplicities_s": round(host_s, 3), "proof_bytes": len(proof),
                      "proof_sha256": hashlib.sha256(proof).hexdigest(), **result}))


if __name__ == "__main__":
    main()
