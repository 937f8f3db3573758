"""What integer ops in chain steps cost and save, at 2^log-n rows under blowup 4, 80 queries and grinding 20, in one process,
--alternations times each side after one warm-up of either:

  arx    air.arx_chain(n, block, keys, digest) from its two input columns through sp_air_prove_int against the whole table of 38 columns
         (air.arx_chain_trace) through sp_air_prove_pub: the same proof bytes (asserted)
  chain  the main table of arx_chain alone, three times through sp_air_main_trace_int: no proof, so that a kernel trace holds the column
         builders' kernels only - the air_main_chain_kernel<true, false, false, true> row is the group's, and its time over
         (n / block) lanes x (block - 1) steps x INT_OPS_PER_STEP is the time per interpreted integer op; the step's field ops ride in
         it (the figure is an upper bound).  --part mul builds a chain group of the same shape whose step holds as many MULs as the
         arx step has ops in all: its row over the same count is the time of a Montgomery product in the interpreter, the unit the
         integer ops are held against
  rec    air.mimc_blocks(n, block) through sp_air_prove_rec; div: air.ec_subset_sum(n, 256) through sp_air_prove_div, by
         tools/air_chain_bench.py and tools/air_div_bench.py - programs without the new ops, for the A/B of two builds in alternating
         processes: those tools exist in both trees, this one only says so

Prints one JSON line: per side the wall time of every proof and their median, sp_last_round_ms of the last one (rounds 1 - 4, device
time) and sp_last_upload_stats of the last one.

    python tools/air_int_bench.py [--log-n 18] [--block 64] [--alternations 5] [--part arx]
    rocprofv3 --kernel-trace --stats -d OUT -o p -- python tools/air_int_bench.py --part chain
    rocprofv3 --kernel-trace --stats -d OUT2 -o p -- python tools/air_int_bench.py --part mul
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
# the arx step: rotr (2 LIMBs), the addition's LIMB, rotl (2 LIMBs), the XOR
INT_OPS_PER_STEP = 6


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


def mul_program(air, s, keys, muls):
    """A two-column chain group in blocks of s rows whose step is `muls` dependent field products (and the two adds that keep the
    columns apart): the polynomial launch, air_main_chain_kernel<true, false, false, false>, on the arx group's shape."""
    b = air.AirBuilder(4, [0], 1, periodic=[list(keys)], main_inputs=2)
    m = b.main
    g = m.chain(s, [m.load(0, 0), m.load(0, 1)])
    x, y, k = g.state(0), g.state(1), m.periodic(0, 0)
    for _ in range(muls // 2):
        x, y = x * y + k, y * x
    g.step([x, y])
    v = b.load(0, 0)
    b.constraint(v - v, degree=1, exemptions=0)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=18)
    ap.add_argument("--block", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--part", choices=("arx", "chain", "mul"), default="arx")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from lambdaworks_cairo_prover_amd import _lib, air, api

    def to_bytes(rows):
        return air.ints_to_bytes(np.array(rows, dtype=object))

    n, s, options = 1 << args.log_n, args.block, (4, 80, 3, 20)
    opt = api.ProofOptions(*options)
    rng = random.Random(2031)
    keys = [rng.randrange(1 << 16) for _ in range(s)]
    rows = air.arx_chain_inputs(n, s, rng)
    out = {"tool": "air_int_bench", "package": os.path.dirname(os.path.abspath(air.__file__)), "rows": n, "block": s, "options": options,
           "alternations": args.alternations}
    with api.Context(device=0) as ctx:
        b = air.arx_chain(n, s, keys, air.arx_chain_digest(rows[0], s, keys))
        desc, keep = b.build()
        assert air.route(desc, "prove")[0] == "sp_air_prove_int"
        inputs = to_bytes(rows)
        if args.part == "arx":
            t0 = time.perf_counter()
            whole = air.arx_chain_trace(rows, s, keys)      # what a caller computed on the host until now
            host_s = time.perf_counter() - t0
            full = to_bytes(whole)
            out["arx"] = {"input_bytes": int(inputs.nbytes), "table_bytes": int(full.nbytes), "host_table_s": round(host_s, 3),
                          **alternate(ctx, {"whole_table_pub": lambda c: prove_pub(c, desc, full, opt, _lib, air), "input_int": lambda c: c.air_prove(desc, inputs, opt)},
                                      args.alternations)}
        if args.part == "chain":
            ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                table = ctx.air_main_trace(desc, inputs)
                ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            want = air.arx_chain_trace(rows[:s], s, keys)
            assert [[int(v) for v in r] for r in air.trace_to_ints(table[:s])] == want
            out["chain"] = {"lanes": n // s, "steps": s - 1, "int_ops_per_step": INT_OPS_PER_STEP, "interpreted_int_ops": (n // s) * (s - 1) * INT_OPS_PER_STEP,
                            "program_ops": len(b.main.ops), "calls": 3, "main_trace_ms": ms}
        if args.part == "mul":
            muls = 12
            mb = mul_program(air, s, keys, muls)
            mdesc, mkeep = mb.build()
            ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                ctx.air_main_trace(mdesc, inputs)
                ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            out["mul"] = {"lanes": n // s, "steps": s - 1, "muls_per_step": muls, "interpreted_muls": (n // s) * (s - 1) * muls, "calls": 3, "main_trace_ms": ms}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
