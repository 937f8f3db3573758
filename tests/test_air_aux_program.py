"""Auxiliary programs of program AIRs (sp_air_prove_aux, air.AUX_PROGRAM) on the host side: the binding's struct mirror and ABI
number, the Python evaluator of the program's semantics against hand-computed columns, and the builder's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

from lambdaworks_cairo_prover_amd import _lib, air

P = air.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_aux_desc_mirror_and_abi_version(hip_lib):
    assert ctypes.sizeof(air.AirAuxDescC) == hip_lib.sp_air_aux_desc_size()
    assert ctypes.sizeof(air.AirAuxColumnC) == 16
    header = open(os.path.join(ROOT, "include", "stark252_hip.h")).read()
    assert int(re.search(r"#define SP_ABI_VERSION\s+(\d+)", header).group(1)) == 7
    assert _lib.SP_ABI_VERSION == 7 and hip_lib.sp_abi_version() == 7
    assert int(re.search(r"#define SP_AIR_AUX_PROGRAM\s+(\d+)", header).group(1)) == air.AUX_PROGRAM == 3
    assert "sp_air_prove_aux" in _lib.NEWEST_SYMBOLS and "sp_air_aux_desc_size" in _lib.NEWEST_SYMBOLS


ROWS = [[2, 5], [3, 7], [4, 11], [6, 13]]      # 4 rows, columns a, b
G = 10                                         # the RAP challenge


def inv(x):
    return pow(x % P, P - 2, P)


def _program():
    b = air.AirBuilder(2, [0, 1], 1, aux_cols=4, n_rap=1, aux_kind=air.AUX_PROGRAM)
    x = b.aux
    g = x.rap(0)
    x.product(x.load(0, 0) + g, x.load(0, 1) + g)          # z_i = prod_(j<i) (a_j + g) / (b_j + g)
    x.running_sum(x.load(0, 0), x.load(0, 1) - g)          # s_i = sum_(j<i) a_j / (b_j - g)
    x.running_sum(x.load(0, 0) * 3)                        # D = 1
    x.product(x.load(3, 1) - x.load(1, 0))                 # shift 3 wraps: row j reads b of row j + 3 mod 4, a of row j + 1
    return b


def test_reference_evaluator_gives_hand_computed_columns():
    out = _program().aux.evaluate(ROWS, [G])
    a = [r[0] for r in ROWS]
    b = [r[1] for r in ROWS]
    z = [1, (a[0] + G) * inv(b[0] + G) % P]
    z.append(z[1] * (a[1] + G) * inv(b[1] + G) % P)
    z.append(z[2] * (a[2] + G) * inv(b[2] + G) % P)
    s = [0, a[0] * inv(b[0] - G) % P]
    s.append((s[1] + a[1] * inv(b[1] - G)) % P)
    s.append((s[2] + a[2] * inv(b[2] - G)) % P)
    u = [0, 6, 6 + 9, 6 + 9 + 12]
    w = [1, 13 - 3, (13 - 3) * (5 - 4), (13 - 3) * (5 - 4) * (7 - 6)]   # rows 0, 1, 2: b[3] - a[1], b[0] - a[2], b[1] - a[3]
    assert [[int(v) for v in r] for r in out] == [list(r) for r in zip(z, s, u, w)]


def test_reference_evaluator_matches_fibonacci_rap_column():
    """fibonacci_rap_program's column is the permutation column of the reference example (fibonacci_rap.rs:69-93)."""
    b = air.fibonacci_rap_program(8, 8)
    rows = [[1, 1], [1, 2], [2, 1], [3, 3]]
    out = b.aux.evaluate(rows, [5])
    want, z = [], 1
    for a_, b_ in rows:
        want.append(z)
        z = z * (a_ + 5) * inv(b_ + 5) % P
    assert [int(v) for v in out[:, 0]] == want


def test_reference_evaluator_rejects_a_zero_denominator():
    b = air.AirBuilder(1, [0, 1], 1, aux_cols=1, n_rap=0, aux_kind=air.AUX_PROGRAM)
    b.aux.running_sum(1, b.aux.load(0, 0))
    with pytest.raises(ValueError):
        b.aux.evaluate([[1], [0], [2], [3]], [])


def test_bytes_round_trip():
    vals = np.array([[0, 1], [P - 1, 2**200 + 7]], dtype=object)
    raw = air.ints_to_bytes(vals)
    assert raw.shape == (2, 2, 32) and bytes(raw[1, 1]) == (2**200 + 7).to_bytes(32, "big")
    assert (air.trace_to_ints(raw) == vals).all()


def test_builder_refusals(hip_lib):
    b = air.AirBuilder(2, [0, 1], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM)
    with pytest.raises(ValueError):
        b.aux.load(0, 2)                     # not a main column
    with pytest.raises(ValueError):
        b.aux.load(8, 0)                     # shift beyond 7
    with pytest.raises(ValueError):
        b.aux.rap(1)                         # one challenge only
    b.constraint(b.load(1, 0) - b.load(0, 0), 1, 1)
    with pytest.raises(ValueError):
        b.build()                            # aux_cols = 1, no column declared
    b.aux.product(b.aux.load(0, 0))
    b.aux.running_sum(b.aux.load(0, 1))
    with pytest.raises(ValueError):
        b.build()                            # two columns declared, aux_cols = 1
    lim = __import__("lambdaworks_cairo_prover_amd.api", fromlist=["air_limits"]).air_limits()
    c = air.AirBuilder(2, [0, 1], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM)
    c.constraint(c.load(1, 0) - c.load(0, 0), 1, 1)
    v = c.aux.load(0, 0)
    c.aux.product(v)
    while len(c.aux.ops) <= lim["ops"]:
        v = v + v
    with pytest.raises(ValueError):
        c.build()                            # too many ops
    d = air.AirBuilder(2, [0, 1], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM)
    d.constraint(d.load(1, 0) - d.load(0, 0), 1, 1)
    for k in range(lim["constants"] + 1):
        d.aux.const(k + 2)
    d.aux.product(d.aux.load(0, 0))
    with pytest.raises(ValueError):
        d.build()                            # too many constants


def test_build_carries_the_aux_desc(hip_lib):
    b = air.fibonacci_rap_program(16, 16)
    desc, keep = b.build()
    assert desc.aux_kind == air.AUX_PROGRAM and desc.aux_cols == 1
    x = desc.aux_desc
    assert (x.n_ops, x.n_consts, x.n_cols) == (len(b.aux.ops), 0, 1)
    assert (x.cols[0].kind, x.cols[0].den_op) == (air.AUX_PRODUCT, 4)
    assert x.ops[0].op == air.OP_CONST and x.ops[0].a == 0       # the RAP challenge follows the (no) constants
    cb, keep2 = b.build(aux_as_callback=True, main_trace=[[1, 1]] * 16)
    assert cb.aux_kind == air.AUX_CALLBACK and cb.aux_fn and getattr(cb, "aux_desc", None) is None
    with pytest.raises(ValueError):
        b.build(aux_as_callback=True)        # the callback needs the trace
    # the AIRs that had no aux program keep their build() exactly
    d2, k2 = air.fibonacci_rap(16, 16).build()
    assert d2.aux_kind == air.AUX_FIBONACCI_RAP and getattr(d2, "aux_desc", None) is None and len(k2) == 4
