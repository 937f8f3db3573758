"""What the CPU tests of the main-program features (test_air_chain, _lookup, _link, _div, _fetch) share: mutators of a MainProgram's lists
(ops [(op, a, b)], cols [(kind, num_op, den_op, pad)]), the decoder's verdict through sp_air_main_check_<suffix>, and the one test body
that holds a refusal of the decoder against the builder's mirror of it."""
import ctypes

import pytest

from lambdaworks_cairo_prover_amd import _lib, air, api


def _col(k, **fields):
    def mutate(m):
        c = dict(zip(("kind", "num_op", "den_op", "pad"), m.cols[k]))
        c.update(fields)
        m.cols[k] = (c["kind"], c["num_op"], c["den_op"], c["pad"])
    return mutate


def _first(m, want):
    return next(t for t, o in enumerate(m.ops) if want(o))


def _op(want, **fields):
    def mutate(m):
        t = _first(m, want)
        o = dict(zip(("op", "a", "b"), m.ops[t]))
        o.update(fields)
        m.ops[t] = (o["op"], o["a"], o["b"])
    return mutate


def check_with(lib, suffix, desc, n, ext=True):
    """sp_air_main_check_<suffix> on desc and its own main program; "": sp_air_main_check, which takes no sp_air_ext."""
    if suffix == "":
        return lib.sp_air_main_check(ctypes.byref(desc), ctypes.byref(desc.main_desc), ctypes.c_uint64(n))
    x = air.ext_of(desc) if ext else None
    return getattr(lib, f"sp_air_main_check_{suffix}")(ctypes.byref(desc), None if x is None else ctypes.byref(x), ctypes.byref(desc.main_desc), ctypes.c_uint64(n))


def decoder_refuses_and_the_builder_raises(lib, suffix, build, mutate, says, n, code=_lib.SP_E_INVALID_ARG, mirror=None):
    """build() passes the decoder; with `mutate` applied to its main program's lists the builder's check() raises - its message holds
    `mirror` (None: `says` whole) - and the same lists as C structs, past the builder, are refused with `code` and a message that holds
    `says`.  Returns (the builder's message, the library's)."""
    desc, keep = build().build()
    assert check_with(lib, suffix, desc, n) == _lib.SP_OK, lib.sp_last_error()
    b = build()
    mutate(b.main)
    with pytest.raises(ValueError) as e:          # the builder's mirror, rule for rule
        b.main.check(n)
    raised = str(e.value)
    assert (says if mirror is None else mirror) in raised, raised
    # the same lists as C structs, past the builder
    main, main_keep = air.main_desc(b.main.input_cols, b.main.ops, b.main.consts, b.main.cols)
    desc.main_desc = main
    assert check_with(lib, suffix, desc, n) == code
    message = lib.sp_last_error().decode()
    assert says in message and message.startswith(f"sp_air_main_check_{suffix}: main program: "), message
    with pytest.raises(api.SpError) as e:
        api.air_main_check(desc, n)
    assert e.value.code == code
    return raised, message
