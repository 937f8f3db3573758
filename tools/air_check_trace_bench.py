"""Device time of sp_air_check_trace's report kernel beside the flag-only check of sp_air_prove, on the shape of tools/air_wide_bench.py
(256 main columns, 2^18 rows, 64 transition constraints, 512 boundary constraints on 64 rows).  --trace clean: the satisfying trace;
--trace wrong: every column counts up by one too much, so every constraint is non-zero on every enforced row and every wave of the
report kernel issues its three atomics for each of the 64 constraints.  One proof (whose round 2 runs the flag-only check
air_check_kernel<false> on the same trace), then --reps reports.  Meant to run under the profiler:

    rocprofv3 --kernel-trace --stats -d OUT -o p -- python tools/air_check_trace_bench.py --trace clean
    rocprofv3 --kernel-trace --stats -d OUT2 -o p -- python tools/air_check_trace_bench.py --trace wrong
    python tools/rocprof_summary.py OUT/*/p_results.db        (the air_report_kernel and air_check_kernel rows)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import many_column_air as M  # noqa: E402
from lambdaworks_cairo_prover_amd import api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", choices=("clean", "wrong"), default="clean")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log-n", type=int, default=18)
    args = ap.parse_args()
    n, cols, options = 1 << args.log_n, 256, (4, 80, 3, 20)
    b = M.build(n, cols, n_transitions=64, boundary_row_count=64, boundary_total=512)
    trace = M.main_trace(n, cols)
    if args.trace == "wrong":
        i = np.arange(n, dtype=np.uint64)[:, None]
        j = np.arange(cols, dtype=np.uint64)[None, :]
        v = (3 * j + 1) + i * (7 * j + 6)
        trace[:, :, 24:] = v.astype(">u8").view(np.uint8).reshape(n, cols, 8)
    desc, keep = b.build()
    opt = api.ProofOptions(*options)
    with api.Context(device=0) as ctx:
        ctx.air_prove(desc, trace, opt)
        path = ctx.last_proof_info()["composition_path"]
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            found = ctx.air_check_trace(desc, trace, opt)
            times.append((time.perf_counter() - t0) * 1e3)
        transitions = [v for v in found if v.kind == 0]
        if args.trace == "clean":
            assert found == [] and path == 1
        else:
            assert path == 3 and len(transitions) == 64 and all((v.rows, v.first_row, v.last_row) == (n - 1, 0, n - 2) for v in transitions)
    print(json.dumps({"tool": "air_check_trace_bench", "trace": args.trace, "rows": n, "main_cols": cols, "transitions": len(b.degrees), "ops": len(b.ops),
                      "boundary_constraints": len(b.bcs), "violations": ctx.last_check_total, "composition_path_of_the_proof": path,
                      "check_wall_ms": [round(t, 2) for t in times]}))


if __name__ == "__main__":
    main()
