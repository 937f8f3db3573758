"""One context through shapes and paths that allocate, grow and drop the prover's on-demand device buffers: a Cairo run, a program
AIR with an auxiliary program, the same shape with more exempted rows (the exemption roots grow) and with more boundary constraints
(the program buffer grows), a constraint-violating Cairo trace (the whole-domain composition buffers) and the first run again -
three times over.  Every proof is the oracle's, and the device memory the prover holds stops growing after the first cycle."""
import pytest

import aux_program_airs as X
from lambdaworks_cairo_prover_amd import air, api

pytestmark = pytest.mark.gpu

OPTIONS = (4, 3, 3, 1)


def _rap_case(oracle, n, extra_boundary):
    b = X.rap_air(n, perm_shifts=(0, 3), logup_shifts=(1, 6))
    for i in range(1, 1 + extra_boundary):
        b.boundary(X.A, i, i + 1)                      # a_i = i + 1 holds on every row
    trace = X.main_trace(n)
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=trace)
    want = oracle.program_air_prove(cb_desc, trace, OPTIONS)
    desc, keep = b.build()
    return (lambda ctx: ctx.air_prove(desc, trace, api.ProofOptions(*OPTIONS))), want, (desc, keep)


def _fib_rap_case(oracle, steps):
    trace = oracle.example_trace("fibonacci_rap", steps, (1, 1))
    assert trace.shape[0] == 256
    want = oracle.example_prove("fibonacci_rap", trace, OPTIONS, (1, 1), steps)
    desc, keep = air.fibonacci_rap_program(trace.shape[0], steps).build()
    return (lambda ctx: ctx.air_prove(desc, trace, api.ProofOptions(*OPTIONS))), want, (desc, keep)


def _cairo_case(oracle, run, trace):
    want = oracle.cairo_prove(trace, run.public_inputs_c, OPTIONS)
    return (lambda ctx: ctx.cairo_prove(trace, run.public_inputs_c, api.ProofOptions(*OPTIONS))), want, run


def test_on_demand_buffers_follow_the_shape_and_do_not_accumulate(hip_lib, oracle):
    run = api.CairoRun.fibonacci(10)
    violated = run.main_trace().copy()
    violated[5, 20, 31] ^= 1                           # a full-width cell: deg H >= 2n, the whole-domain composition
    cases = [
        ("cairo fib(10)", _cairo_case(oracle, run, run.main_trace())),
        ("fibonacci_rap, 8 exempted rows", _fib_rap_case(oracle, 250)),
        ("fibonacci_rap, 108 exempted rows", _fib_rap_case(oracle, 150)),      # same shape: the exemption roots outgrow their 64
        ("rap_air", _rap_case(oracle, 64, 0)),
        ("rap_air, 40 more boundary constraints", _rap_case(oracle, 64, 40)),  # same shape: the program's tables outgrow their buffer
        ("cairo fib(10), violated", _cairo_case(oracle, run, violated)),
        ("cairo fib(10) again", _cairo_case(oracle, run, run.main_trace())),
    ]
    held = []
    with api.Context(device=0) as ctx:
        for cycle in range(3):
            for name, (prove, want, _keep) in cases:
                assert prove(ctx) == want, (cycle, name)
                if name.endswith("violated"):
                    assert ctx.last_proof_info()["composition_path"] == 3
            held.append(ctx.prover_device_bytes())
    print("prover_device_bytes after each cycle:", held)
    assert held[0] > 0
    assert held[2] == held[1]
