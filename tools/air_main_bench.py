"""What a main-trace program saves on one shape: air.bit_range_check(2^log-n, 64) - one input column, 64 derived bit columns, 65 main
columns in all - proved in one process alternately (a) from the whole host table through sp_air_prove_ext and (b) from the input
column through sp_air_prove_main, --alternations times each after one warm-up of either.  Both give the same bytes (asserted).  Prints
one JSON line: per side the median wall time of a proof, sp_last_round_ms of the last one (rounds 1 - 4, device time) and
sp_last_upload_stats of the last one.

    python tools/air_main_bench.py [--log-n 18] [--bits 64] [--alternations 3]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from lambdaworks_cairo_prover_amd import _lib, air, api  # noqa: E402


def tables(n, bits):
    """(inputs (n, 1, 32), whole table (n, 1 + bits, 32)) in canonical big-endian bytes, for n values below 2^bits (bits <= 64)."""
    rng = np.random.default_rng(2026)
    v = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    if bits < 64:
        v &= np.uint64((1 << bits) - 1)
    full = np.zeros((n, 1 + bits, 32), dtype=np.uint8)
    full[:, 0, 24:] = v.astype(">u8").view(np.uint8).reshape(n, 8)
    for j in range(bits):
        full[:, 1 + j, 31] = ((v >> np.uint64(j)) & np.uint64(1)).astype(np.uint8)
    return np.ascontiguousarray(full[:, :1, :]), full


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
    ap.add_argument("--bits", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=3)
    args = ap.parse_args()
    n, options = 1 << args.log_n, (4, 80, 3, 20)
    b = air.bit_range_check(n, args.bits)
    desc, keep = b.build()
    inputs, full = tables(n, args.bits)
    opt = api.ProofOptions(*options)
    sides = {"whole_table_ext": lambda ctx: prove_ext(ctx, desc, full, opt), "inputs_main": lambda ctx: ctx.air_prove(desc, inputs, opt)}
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
    print(json.dumps({"tool": "air_main_bench", "rows": n, "main_cols": 1 + args.bits, "input_cols": 1, "options": options, "alternations": args.alternations,
                      "table_bytes": int(full.nbytes), "input_bytes": int(inputs.nbytes), "proof_bytes": len(proof),
                      "proof_sha256": hashlib.sha256(proof).hexdigest(), **result}))


if __name__ == "__main__":
    main()
