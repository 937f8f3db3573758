"""What device-built limbs and bitwise words cost, at 2^log-n rows under blowup 4, 80 queries and grinding 20, in one process,
--alternations times each side after one warm-up of either:

  range  air.limb_range_check(n, limb_bits, count) from its one input column through sp_air_prove_word against the whole table of
         1 + 2 count columns (air.limb_range_check_trace) through sp_air_prove_pub: the same proof bytes (asserted)
  chunk  the main table of a program with one LIMB group of 4 (the 16-bit limbs of x) and one WORD group of 3 (AND, OR, XOR of x and y
         over 64 bits) alone, three times through sp_air_main_trace_word: no proof, so that a kernel trace holds the column builders'
         kernels only (air_aux_terms_*, air_main_limbs_kernel, air_main_words_kernel)
  bits   air.bit_range_check(n, 64) from its input column through sp_air_prove_main, --alternations proofs: a program without the new
         kinds, for the A/B of two builds in alternating processes

Prints one JSON line: per side the wall time of every proof and their median, sp_last_round_ms of the last one (rounds 1 - 4, device
time) and sp_last_upload_stats of the last one.

    python tools/air_word_bench.py [--log-n 18] [--limb-bits 16] [--count 4] [--alternations 5] [--part range]
    rocprofv3 --kernel-trace --stats -d OUT -o p -- python tools/air_word_bench.py --part chunk
    python tools/rocprof_summary.py OUT/.../p_results.db
    python tools/air_word_bench.py --part bits
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


def prove_pub(ctx, desc, full, opt, _lib, air):
    ext = air.ext_of(desc)
    c_opt = opt.to_c()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    _lib.check(_lib.load().sp_air_prove_pub(ctx._h, ctypes.byref(desc), ctypes.byref(ext), None, full.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            ctypes.c_uint64(full.shape[0]), ctypes.byref(c_opt), ctypes.byref(out), ctypes.byref(ln)))
    return ctx._take_proof(out, ln)


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


def chunk_program(air):
    """Inputs x and y (below 2^64): the four 16-bit limbs of x (one LIMB group) and AND, OR, XOR of x and y over 64 bits (one WORD group)."""
    b = air.AirBuilder(9, [0], 1, main_inputs=2)
    m = b.main
    m.limbs(m.load(0, 0), 16, 4)
    x, y = m.load(0, 0), m.load(0, 1)
    m.word_and(x, y, 64); m.word_or(x, y, 64); m.word_xor(x, y, 64)
    v = b.load(0, 0)
    b.constraint(v - v, degree=1, exemptions=0)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=18)
    ap.add_argument("--limb-bits", type=int, default=16)
    ap.add_argument("--count", type=int, default=4)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--part", choices=("range", "chunk", "bits"), default="range")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from lambdaworks_cairo_prover_amd import _lib, air, api

    def to_bytes(rows):
        return air.ints_to_bytes(np.array(rows, dtype=object))

    n, options = 1 << args.log_n, (4, 80, 3, 20)
    opt = api.ProofOptions(*options)
    out = {"tool": "air_word_bench", "package": os.path.dirname(os.path.abspath(air.__file__)), "rows": n, "options": options, "alternations": args.alternations}
    with api.Context(device=0) as ctx:
        if args.part == "range":
            b = air.limb_range_check(n, args.limb_bits, args.count)
            desc, keep = b.build()
            assert air.route(desc, "prove")[0] == "sp_air_prove_word"
            rows = air.limb_range_check_inputs(n, args.limb_bits, args.count, random.Random(2028))
            t0 = time.perf_counter()
            whole = air.limb_range_check_trace(rows, args.limb_bits, args.count)      # what a caller computed on the host until now
            host_s = time.perf_counter() - t0
            inputs, full = to_bytes(rows), to_bytes(whole)
            out["range"] = {"limb_bits": args.limb_bits, "count": args.count, "input_bytes": int(inputs.nbytes), "table_bytes": int(full.nbytes),
                            "host_table_s": round(host_s, 3),
                            **alternate(ctx, {"whole_table_pub": lambda c: prove_pub(c, desc, full, opt, _lib, air), "input_word": lambda c: c.air_prove(desc, inputs, opt)},
                                        args.alternations)}
        if args.part == "chunk":
            b = chunk_program(air)
            desc, keep = b.build()
            rng = random.Random(2029)
            rows = [[rng.randrange(1 << 64), rng.randrange(1 << 64)] for _ in range(n)]
            inputs, ms = to_bytes(rows), []
            for _ in range(3):
                t0 = time.perf_counter()
                table = ctx.air_main_trace(desc, inputs)
                ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            x, y = rows[63]
            assert [int(v) for v in air.trace_to_ints(table[:64])[63]] == [x, y] + [(x >> (16 * j)) & 0xffff for j in range(4)] + [x & y, x | y, x ^ y]
            out["chunk"] = {"limb_group": 4, "word_group": 3, "word_bits": 64, "calls": 3, "main_trace_ms": ms}
        if args.part == "bits":
            b = air.bit_range_check(n, 64)
            desc, keep = b.build()
            assert air.route(desc, "prove")[0] == "sp_air_prove_main"
            inputs = to_bytes(air.bit_range_check_inputs(n, 64, random.Random(2030)))
            out["bits"] = {"bits": 64, "input_bytes": int(inputs.nbytes), **alternate(ctx, {"input_main": lambda c: c.air_prove(desc, inputs, opt)}, args.alternations)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
