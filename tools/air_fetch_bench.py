"""What a device-fetched lookup result saves on two shapes, at 2^log-n rows under blowup 4, 80 queries and grinding 20, in one process,
--alternations times each side after one warm-up of either:

  xor   air.xor_fetch(n, bits) from its two input columns (a, b) through sp_air_prove_fetch against air.xor_lookup(n, bits) from its
        three (a, b, a xor b) through sp_air_prove_lk: the same statement, the same proof bytes (asserted)
  rom   air.rom_reads(n, key_bits) from its three input columns through sp_air_prove_fetch against the whole five-column table
        (air.rom_reads_trace) through sp_air_prove_pub: the same proof bytes (asserted)
  chunk the main table of air.rom_reads alone, three times through sp_air_main_trace_fetch: no proof, so that a kernel trace holds the
        column builders' kernels only (one FETCH chunk and one COUNT chunk a call)

Prints one JSON line: per side the wall time of every proof and their median, sp_last_round_ms of the last one (rounds 1 - 4, device
time) and sp_last_upload_stats of the last one.  The FETCH chunk's own kernels - the two key passes (air_aux_sort_terms_*), V's terms
(air_aux_terms_*), the radix passes (rs_hist_kernel, rs_scatter_kernel and the scan's kernels) and air_main_fetch_kernel - are their
rows of a kernel trace of this script, taken in a run of its own:

    python tools/air_fetch_bench.py [--log-n 18] [--bits 8] [--key-bits 32] [--alternations 5] [--part both]
    rocprofv3 --kernel-trace --stats -d OUT -o p -- python tools/air_fetch_bench.py --part chunk
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


def to_bytes(rows):
    return air.ints_to_bytes(np.array(rows, dtype=object))


def alternate(ctx, sides, alternations):
    result = {name: {"ms": []} for name in sides}
    proof = None
    for name, call in sides.items():          # warm-up: the shape's set-up, first launches, the workspace
        p = call(ctx)
        assert proof is None or p == proof, "the two paths disagree"
        proof = p
    assert ctx.last_proof_info()["composition_path"] == 1, "the trace does not satisfy its constraints"
    for _ in range(alternations):
        for name, call in sides.items():
            t0 = time.perf_counter()
            p = call(ctx)
            result[name]["ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
            assert p == proof
            result[name]["last_round_ms"] = [round(x, 2) for x in ctx.last_round_ms()[1:]]
            result[name]["upload"] = ctx.last_upload_stats()
    for r in result.values():
        r["median_ms"] = round(statistics.median(r["ms"]), 2)
    result["proof_bytes"] = len(proof)
    result["proof_sha256"] = hashlib.sha256(proof).hexdigest()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=18)
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--key-bits", type=int, default=32)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--part", choices=("xor", "rom", "both", "chunk"), default="both")
    args = ap.parse_args()
    n, options = 1 << args.log_n, (4, 80, 3, 20)
    opt = api.ProofOptions(*options)
    out = {"tool": "air_fetch_bench", "rows": n, "options": options, "alternations": args.alternations}
    with api.Context(device=0) as ctx:
        if args.part in ("xor", "both"):
            fetch, lookup = air.xor_fetch(n, args.bits), air.xor_lookup(n, args.bits)
            f_desc, f_keep = fetch.build()
            l_desc, l_keep = lookup.build()
            assert air.route(f_desc, "prove")[0] == "sp_air_prove_fetch" and air.route(l_desc, "prove")[0] == "sp_air_prove_lk"
            rows3 = air.xor_lookup_inputs(n, args.bits, random.Random(2026))
            in2, in3 = to_bytes([r[:2] for r in rows3]), to_bytes(rows3)
            out["xor"] = {"bits": args.bits, "table_entries": 1 << (2 * args.bits), "fetch_key_bits": 2 * args.bits, "count_key_bits": 3 * args.bits,
                          "input_bytes_fetch": int(in2.nbytes), "input_bytes_lk": int(in3.nbytes),
                          **alternate(ctx, {"xor_lookup_lk": lambda c: c.air_prove(l_desc, in3, opt), "xor_fetch_fetch": lambda c: c.air_prove(f_desc, in2, opt)},
                                      args.alternations)}
        if args.part in ("rom", "both"):
            b = air.rom_reads(n, args.key_bits)
            desc, keep = b.build()
            assert air.route(desc, "prove")[0] == "sp_air_prove_fetch"
            rows = air.rom_reads_inputs(n, args.key_bits, random.Random(2027))
            t0 = time.perf_counter()
            whole = air.rom_reads_trace(rows)         # what a caller computed on the host until now
            host_s = time.perf_counter() - t0
            inputs, full = to_bytes(rows), to_bytes(whole)
            out["rom"] = {"key_bits": args.key_bits, "radix_passes": (args.key_bits + 7) // 8, "input_bytes": int(inputs.nbytes), "table_bytes": int(full.nbytes),
                          "host_join_s": round(host_s, 3),
                          **alternate(ctx, {"whole_table_pub": lambda c: prove_pub(c, desc, full, opt), "inputs_fetch": lambda c: c.air_prove(desc, inputs, opt)},
                                      args.alternations)}
        if args.part == "chunk":
            b = air.rom_reads(n, args.key_bits)
            desc, keep = b.build()
            rows = air.rom_reads_inputs(n, args.key_bits, random.Random(2027))
            inputs, ms = to_bytes(rows), []
            for _ in range(3):
                t0 = time.perf_counter()
                table = ctx.air_main_trace(desc, inputs)
                ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            assert [int(x) for x in air.trace_to_ints(table[:64])[63]] == air.rom_reads_trace(rows)[63]
            out["chunk"] = {"key_bits": args.key_bits, "radix_passes": (args.key_bits + 7) // 8, "calls": 3, "main_trace_ms": ms}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
