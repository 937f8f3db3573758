"""Builder for `sp_air_desc` (include/stark252_hip.h): an AIR other than Cairo, given as a straight-line program over
frame cells.  Mirrors what an implementor of the reference's `AIR` trait provides (src/starks/traits.rs:15-119):
context (columns, transition offsets / degrees / exemptions), `compute_transition`, `boundary_constraints`,
`composition_poly_degree_bound`, the number of RAP challenges and the auxiliary-trace builder (by kind).

    b = AirBuilder(main_cols=1, offsets=[0, 1, 2], degree_bound_factor=1)
    r0, r1, r2 = b.load(0, 0), b.load(1, 0), b.load(2, 0)
    b.constraint(r2 - r1 - r0, degree=1, exemptions=2)
    b.boundary(col=0, step=0, value=1); b.boundary(0, 1, 1)
    desc = b.build()

Periodic columns (an extension beyond the reference's trait): AirBuilder(..., periodic=[values0, values1, ...]) declares public
sequences that repeat down the trace (each a power-of-two number of values, at most the trace length); b.periodic(row, k) reads
column k at frame row `row`.  In a constraint's declared degree such a value counts as a trace cell.  See mimc_chain below.

Strided constraints (another extension): b.constraint(value, degree, exemptions, period=4, offset=1) enforces the constraint on the rows
= 1 (mod 4) only, dividing by that progression's own zerofier instead of multiplying by a selector column: the declared degree stays
the constraint's own.  `exemptions` then counts the last rows of the progression.  See strided_mimc_chain below.

Public data inside a randomized (RAP) argument (sp_air_prove_pub): b.aux.table(shift, k) reads periodic column k from the auxiliary
program - the public table of a LogUp lookup -, and b.boundary_from(col, step, num, den) declares a boundary constraint whose value is
N / D of b.public, a small program over constants and the RAP challenges: the reference's boundary_constraints(rap_challenges).  See
table_lookup and public_permutation below.

Derived main columns (sp_air_prove_main): AirBuilder(..., main_inputs=I) says that the caller supplies main columns 0 .. I - 1 only;
b.main (MainProgram) declares the others as row-local functions of columns that exist already - b.main.value, inv_or_zero, bit / bits,
running_sum, product -, which the device builds before it commits the main segment.  The proof is the one of the whole table.  See
bit_range_check and zero_count below.

Block recurrences (sp_air_prove_rec): g = b.main.chain(period, seeds) declares a group of columns that hold the states of independent
permutations, one per block of `period` rows - seeded on the block's first row, every later cell a polynomial of the row before it
(g.state(j), g.step([...])) -, and b.main.periodic(shift, k) reads a periodic column (round constants) from the main program.  See
mimc_blocks below.

Linked chain groups (sp_air_prove_link): g = b.main.chain(period, None, width=w, link=L) links L consecutive blocks into a run; until
g.seed([...]) gives the seeds, g.carry(j) reads column j on the last row of the block before (zero on a run's first block).  A sponge
over several blocks, a Merkle path.  See mimc_sponge and merkle_paths below.

Lookup multiplicities (sp_air_prove_lk): b.main.multiplicity(x, table, key_bits) declares the column m of a LogUp lookup - how often
the table value of row i occurs among the looked-up values of all rows, on the first row that holds it -, which the device builds by
sorting both sides.  With it a lookup's whole witness comes from the inputs.  See table_lookup_main and xor_lookup below.

Quotients in chain steps (sp_air_prove_div): inside the seeds and steps of a chain group b.main.div(num, den) - or num / den - is a
value like any other: the slope of an elliptic-curve addition, which the next state needs and the AIR constrains as a column.  See
ec_subset_sum below.
"""
import collections
import ctypes
import enum

P = 2**251 + 17 * 2**192 + 1

OP_LOAD, OP_CONST, OP_ADD, OP_SUB, OP_MUL, OP_OUT, OP_PERIODIC = range(7)
OP_DIV = 7      # a main-trace program only, behind the seed or step of a CHAIN column (sp_air_prove_div)
# Integer ops of a main-trace program, behind the seed or step of a CHAIN column too (sp_air_prove_int): functions of the canonical integer
OP_INT_LIMB, OP_INT_AND, OP_INT_OR, OP_INT_XOR = 8, 9, 10, 11   # LIMB: a = a value, b = lo + 256 width (an immediate); the others: two values
_INT_OPS = (OP_INT_LIMB, OP_INT_AND, OP_INT_OR, OP_INT_XOR)
INT_OP_BITS = 251                                # both operands of AND, OR and XOR stay below 2^251 < p
_TWO_VALUES = (OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_INT_AND, OP_INT_OR, OP_INT_XOR)   # the ops whose a and b name earlier values
# A list cell of a joint COUNT column (sp_air_prove_multi): a = one looked-up value, b = the cell of the rest of the list or LIST_END.  It has no value.
OP_ALSO, LIST_END, MAIN_COUNT_LIST, MAIN_COUNT_MAX_LIST = 12, 0xFFFF, 256, 16
_ONE_VALUE = (OP_INT_LIMB,)                      # the ops whose a names an earlier value and whose b is an immediate


def _value_operands(op, a, b):
    """The earlier values an op reads: what every operand walk follows.  A list cell (op 12) is a leaf: it holds a list and no value."""
    return (a, b) if op in _TWO_VALUES else (a,) if op in _ONE_VALUE else ()


def _marked_operands(op, a, b):
    """What the decoder's marks of an op (reads, quotients, integers) are taken over: its value operands, and for a list cell - which
    stands for its whole list there - its looked-up value and the cell of the rest."""
    if op == OP_ALSO:
        return (a,) if b == LIST_END else (a, b)
    return _value_operands(op, a, b)
MAX_OFFSETS, MAX_TRANSITIONS = 8, 64
AUX_TRACE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint8))


class AirOpC(ctypes.Structure):
    _fields_ = [("op", ctypes.c_uint8), ("pad", ctypes.c_uint8), ("a", ctypes.c_uint16), ("b", ctypes.c_uint16), ("pad2", ctypes.c_uint16)]


class AirBoundaryC(ctypes.Structure):
    _fields_ = [("col", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("step", ctypes.c_uint64), ("value", ctypes.c_uint8 * 32)]


class AirDescC(ctypes.Structure):
    _fields_ = [("main_cols", ctypes.c_uint32), ("aux_cols", ctypes.c_uint32),
                ("n_offsets", ctypes.c_uint32), ("offsets", ctypes.c_uint32 * MAX_OFFSETS),
                ("n_transitions", ctypes.c_uint32), ("degrees", ctypes.c_uint32 * MAX_TRANSITIONS),
                ("exemptions", ctypes.c_uint32 * MAX_TRANSITIONS),
                ("num_transition_exemptions", ctypes.c_uint32), ("degree_bound_factor", ctypes.c_uint32),
                ("n_ops", ctypes.c_uint32), ("ops", ctypes.POINTER(AirOpC)),
                ("n_consts", ctypes.c_uint32), ("consts", ctypes.c_void_p),
                ("n_rap", ctypes.c_uint32), ("aux_kind", ctypes.c_uint32),
                ("n_boundary", ctypes.c_uint32), ("boundary", ctypes.POINTER(AirBoundaryC)),
                ("aux_fn", AUX_TRACE_FN), ("aux_user", ctypes.c_void_p)]


def _check_layout():
    """The library reports the size of its sp_air_desc: a mirror with other field sizes must not reach sp_air_prove."""
    from . import _lib
    want = _lib.load().sp_air_desc_size()
    if ctypes.sizeof(AirDescC) != want:
        raise ImportError(f"AirDescC is {ctypes.sizeof(AirDescC)} bytes, the library's sp_air_desc {want}: the binding is out of date")


AUX_NONE, AUX_FIBONACCI_RAP, AUX_CALLBACK, AUX_PROGRAM = 0, 1, 2, 3
AUX_PRODUCT, AUX_SUM, AUX_SORTED = 0, 1, 2   # sp_air_aux_column.kind
AUX_MAX_SORT_GROUPS = 16             # SP_AIR_AUX_MAX_SORT_GROUPS: sorted columns with one key op form a group
AUX_NO_DEN = 0xFFFFFFFF              # sp_air_aux_column.den_op: D = 1
AUX_MAX_SHIFT = 7
_RAP_TAG = 0x8000


class AirAuxColumnC(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("num_op", ctypes.c_uint32), ("den_op", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class AirAuxDescC(ctypes.Structure):
    _fields_ = [("n_ops", ctypes.c_uint32), ("ops", ctypes.POINTER(AirOpC)),
                ("n_consts", ctypes.c_uint32), ("consts", ctypes.c_void_p),
                ("n_cols", ctypes.c_uint32), ("cols", ctypes.POINTER(AirAuxColumnC))]


def _check_aux_layout():
    from . import _lib
    want = _lib.load().sp_air_aux_desc_size()
    if ctypes.sizeof(AirAuxDescC) != want:
        raise ImportError(f"AirAuxDescC is {ctypes.sizeof(AirAuxDescC)} bytes, the library's sp_air_aux_desc {want}: the binding is out of date")


class AirPeriodicColumnC(ctypes.Structure):
    _fields_ = [("period", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("values", ctypes.c_void_p)]


class AirPeriodicDescC(ctypes.Structure):
    _fields_ = [("n_cols", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("cols", ctypes.POINTER(AirPeriodicColumnC))]


def _check_periodic_layout():
    from . import _lib
    want = _lib.load().sp_air_periodic_desc_size()
    if ctypes.sizeof(AirPeriodicDescC) != want:
        raise ImportError(f"AirPeriodicDescC is {ctypes.sizeof(AirPeriodicDescC)} bytes, the library's sp_air_periodic_desc {want}: the binding is out of date")


class AirStrideC(ctypes.Structure):
    _fields_ = [("period", ctypes.c_uint32), ("offset", ctypes.c_uint32)]


class AirStrideDescC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("strides", ctypes.POINTER(AirStrideC))]


class AirExtC(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("aux", ctypes.POINTER(AirAuxDescC)),
                ("periodic", ctypes.POINTER(AirPeriodicDescC)), ("strides", ctypes.POINTER(AirStrideDescC))]


def _check_stride_layout():
    from . import _lib
    lib = _lib.load()
    for name, mirror in (("sp_air_stride_size", AirStrideC), ("sp_air_stride_desc_size", AirStrideDescC), ("sp_air_ext_size", AirExtC)):
        want = getattr(lib, name)()
        if ctypes.sizeof(mirror) != want:
            raise ImportError(f"{mirror.__name__} is {ctypes.sizeof(mirror)} bytes, the library's struct ({name}) {want}: the binding is out of date")


def stride_desc(strides):
    """[(period, offset), ...], one per transition constraint -> (AirStrideDescC, keepalive): sp_air_stride_desc."""
    _check_stride_layout()
    arr = (AirStrideC * max(1, len(strides)))()
    for k, (period, offset) in enumerate(strides):
        arr[k].period, arr[k].offset = period, offset
    d = AirStrideDescC()
    d.n, d.strides = len(strides), ctypes.cast(arr, ctypes.POINTER(AirStrideC))
    return d, arr


def ext_of(desc):
    """The sp_air_ext of a built descriptor: what it carries of desc.aux_desc, desc.periodic_desc and desc.stride_desc."""
    _check_stride_layout()
    x = AirExtC()
    x.size = ctypes.sizeof(AirExtC)
    for field, attr in (("aux", "aux_desc"), ("periodic", "periodic_desc"), ("strides", "stride_desc")):
        part = getattr(desc, attr, None)
        if part is not None:
            setattr(x, field, ctypes.pointer(part))
    return x


class AirBoundaryValueC(ctypes.Structure):
    _fields_ = [("boundary", ctypes.c_uint32), ("num_op", ctypes.c_uint32), ("den_op", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class AirBoundaryDescC(ctypes.Structure):
    _fields_ = [("n_ops", ctypes.c_uint32), ("ops", ctypes.POINTER(AirOpC)),
                ("n_consts", ctypes.c_uint32), ("consts", ctypes.c_void_p),
                ("n_values", ctypes.c_uint32), ("values", ctypes.POINTER(AirBoundaryValueC))]


def _check_boundary_layout():
    from . import _lib
    lib = _lib.load()
    lib.sp_air_boundary_desc_size.restype = ctypes.c_uint64
    want = lib.sp_air_boundary_desc_size()
    if ctypes.sizeof(AirBoundaryDescC) != want:
        raise ImportError(f"AirBoundaryDescC is {ctypes.sizeof(AirBoundaryDescC)} bytes, the library's sp_air_boundary_desc {want}: the binding is out of date")


def boundary_desc(ops, consts, values):
    """ops [(op, a, b), ...] as the library reads them, consts [int, ...], values [(boundary, num_op, den_op), ...] ->
    (AirBoundaryDescC, keepalive): sp_air_boundary_desc."""
    _check_boundary_layout()
    c_ops = (AirOpC * max(1, len(ops)))()
    for i, (op, a, b) in enumerate(ops):
        c_ops[i].op, c_ops[i].a, c_ops[i].b = op, a, b
    c_consts = ctypes.create_string_buffer(b"".join((int(c) % P).to_bytes(32, "big") for c in consts), max(1, 32 * len(consts)))
    c_values = (AirBoundaryValueC * max(1, len(values)))()
    for j, (boundary, num_op, den_op) in enumerate(values):
        c_values[j].boundary, c_values[j].num_op, c_values[j].den_op = boundary, num_op, den_op
    d = AirBoundaryDescC()
    d.n_ops, d.ops = len(ops), ctypes.cast(c_ops, ctypes.POINTER(AirOpC))
    d.n_consts, d.consts = len(consts), ctypes.cast(c_consts, ctypes.c_void_p)
    d.n_values, d.values = len(values), ctypes.cast(c_values, ctypes.POINTER(AirBoundaryValueC))
    return d, (c_ops, c_consts, c_values)


MAIN_VALUE, MAIN_INV_OR_ZERO, MAIN_BIT, MAIN_SUM, MAIN_PRODUCT, MAIN_CHAIN, MAIN_COUNT = range(7)   # sp_air_main_column.kind
MAIN_MAX_BIT = 251
MAIN_CHAIN_MAX_WIDTH = 16            # sp_air_main_chain_limits
MAIN_COUNT_MAX_KEY_BITS, MAIN_COUNT_MAX_COLS = 64, 16   # sp_air_main_count_limits
MAIN_LINK_MAX_LOG, MAIN_LINK_MAX_WIDTH = 62, 16         # sp_air_main_link_limits
MAIN_FETCH = SP_AIR_MAIN_FETCH = 7                      # sp_air_main_column.kind of a looked-up value (the _fetch entry points)
MAIN_FETCH_MAX_KEY_BITS, MAIN_FETCH_MAX_GROUP, MAIN_FETCH_MAX_COLS = 64, 16, 64   # sp_air_main_fetch_limits
MAIN_LIMB = SP_AIR_MAIN_LIMB = 8                        # sp_air_main_column.kind of a limb of a canonical integer (the _word entry points)
MAIN_WORD = SP_AIR_MAIN_WORD = 9                        # ... and of the AND, OR or XOR of two (the _word entry points)
MAIN_LIMB_MAX_END, MAIN_WORD_MAX_BITS, MAIN_WORD_FUNCTIONS = 252, 251, 3   # sp_air_main_word_limits
WORD_AND, WORD_OR, WORD_XOR = range(3)                  # the fn of a WORD column's pad
INPUTS_HOST, INPUTS_DEVICE = 0, 1    # sp_air_main_desc.input_location


class AirMainColumnC(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("num_op", ctypes.c_uint32), ("den_op", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class AirMainDescC(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("input_cols", ctypes.c_uint32), ("input_location", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                ("n_ops", ctypes.c_uint32), ("ops", ctypes.POINTER(AirOpC)),
                ("n_consts", ctypes.c_uint32), ("consts", ctypes.c_void_p),
                ("n_cols", ctypes.c_uint32), ("cols", ctypes.POINTER(AirMainColumnC))]


def _check_main_layout():
    from . import _lib
    lib = _lib.load()
    lib.sp_air_main_desc_size.restype = ctypes.c_uint64
    want = lib.sp_air_main_desc_size()
    if ctypes.sizeof(AirMainDescC) != want:
        raise ImportError(f"AirMainDescC is {ctypes.sizeof(AirMainDescC)} bytes, the library's sp_air_main_desc {want}: the binding is out of date")


def main_desc(input_cols, ops, consts, cols, input_location=INPUTS_HOST):
    """ops [(op, a, b), ...], consts [int, ...], cols [(kind, num_op, den_op, pad), ...] -> (AirMainDescC, keepalive): sp_air_main_desc."""
    _check_main_layout()
    c_ops = (AirOpC * max(1, len(ops)))()
    for i, (op, a, b) in enumerate(ops):
        c_ops[i].op, c_ops[i].a, c_ops[i].b = op, a, b
    c_consts = ctypes.create_string_buffer(b"".join((int(c) % P).to_bytes(32, "big") for c in consts), max(1, 32 * len(consts)))
    c_cols = (AirMainColumnC * max(1, len(cols)))()
    for k, (kind, num_op, den_op, pad) in enumerate(cols):
        c_cols[k].kind, c_cols[k].num_op, c_cols[k].den_op, c_cols[k].pad = kind, num_op, den_op, pad
    d = AirMainDescC()
    d.size, d.input_cols, d.input_location = ctypes.sizeof(AirMainDescC), input_cols, input_location
    d.n_ops, d.ops = len(ops), ctypes.cast(c_ops, ctypes.POINTER(AirOpC))
    d.n_consts, d.consts = len(consts), ctypes.cast(c_consts, ctypes.c_void_p)
    d.n_cols, d.cols = len(cols), ctypes.cast(c_cols, ctypes.POINTER(AirMainColumnC))
    return d, (c_ops, c_consts, c_cols)


def needs_pub(desc):
    """Whether a built descriptor needs the _pub entry points: it carries boundary values computed from the challenges
    (desc.boundary_desc), or its auxiliary program reads a periodic column (op 6)."""
    if getattr(desc, "boundary_desc", None) is not None:
        return True
    aux = getattr(desc, "aux_desc", None)
    if aux is None:
        return False
    known = getattr(desc, "aux_reads_table", None)   # (AirBuilder.build() says so; a descriptor put together by hand is looked through)
    return any(aux.ops[i].op == OP_PERIODIC for i in range(aux.n_ops)) if known is None else known


class MainLevel(enum.IntEnum):
    """The entry points a main-trace program goes through, in the order of sp::AirMainLevel (air_desc.h): each level's decoder knows what
    the levels below it know, and the entry points carry its suffix (sp_air_prove_rec, sp_air_main_check_rec, ...; sp_air_main_trace and
    sp_air_main_check at MAIN).  MainLevel.WORD, the level above FETCH, is the one member of MainLevelWord below: it orders, compares and
    carries its suffix like a member, and iterating MainLevel goes on giving the six levels MAIN .. FETCH.  MainLevel.INT, above WORD, is
    the one member of MainLevelInt in the same way, and MainLevel.MULTI, above INT, the one member of MainLevelMulti."""
    MAIN, REC, LK, LINK, DIV, FETCH = range(6)

    @property
    def suffix(self):
        return self.name.lower()


class MainLevelWord(enum.IntEnum):
    """sp::AirMainLevel::Word, the _word entry points (LIMB and WORD columns), reached as MainLevel.WORD.  An enumeration of its own:
    an IntEnum with members cannot be extended, and what iterates MainLevel - tests/test_air_main_level.py holds each of its six levels
    against the library and a worked example - goes on seeing those six; tests/test_air_word.py holds this one the same way."""
    WORD = 6

    suffix = MainLevel.suffix


MainLevel.WORD = MainLevelWord.WORD


class MainLevelInt(enum.IntEnum):
    """sp::AirMainLevel::Int, the _int entry points (ops 8 .. 11 behind chain seeds and steps), reached as MainLevel.INT: an enumeration
    of its own for the reason MainLevelWord is one; tests/test_air_int.py holds it against the library."""
    INT = 7

    suffix = MainLevel.suffix


MainLevel.INT = MainLevelInt.INT


class MainLevelMulti(enum.IntEnum):
    """sp::AirMainLevel::Multi, the _multi entry points (a COUNT column over a list of looked-up values, op 12), reached as
    MainLevel.MULTI: an enumeration of its own for the reason MainLevelWord is one; tests/test_air_multi.py holds it against the library."""
    MULTI = 8

    suffix = MainLevel.suffix


MainLevel.MULTI = MainLevelMulti.MULTI


# What in a main program demands each level above MAIN: a test of a column's (kind, pad) and a test of an op code (None: no such thing).
_MAIN_DEMANDS = {
    MainLevel.REC: (lambda kind, pad: kind == MAIN_CHAIN, lambda op: op == OP_PERIODIC),      # a chain column, a read of a periodic column
    MainLevel.LK: (lambda kind, pad: kind == MAIN_COUNT, None),                               # a lookup multiplicity
    MainLevel.LINK: (lambda kind, pad: kind == MAIN_CHAIN and pad >> 16 != 0, None),          # a pad that carries k >= 1: runs of 2^k blocks
    MainLevel.DIV: (None, lambda op: op == OP_DIV),                                           # a quotient behind a chain group
    MainLevel.FETCH: (lambda kind, pad: kind == MAIN_FETCH, None),                            # a looked-up value
    MainLevel.WORD: (lambda kind, pad: kind in (MAIN_LIMB, MAIN_WORD), None),                 # a limb or a bitwise word
    MainLevel.INT: (None, lambda op: op in _INT_OPS),                                         # an integer op behind a chain group
    MainLevel.MULTI: (lambda kind, pad: kind == MAIN_COUNT and pad & MAIN_COUNT_LIST != 0, lambda op: op == OP_ALSO),   # a joint multiplicity, a list cell
}


def _demanded(cols, ops):
    """The levels that the columns (kind, pad) and the op codes of a main program demand, one pass over each."""
    found = {level for kind, pad in cols for level, (col, _) in _MAIN_DEMANDS.items() if col is not None and col(kind, pad)}
    found |= {level for code in ops for level, (_, op) in _MAIN_DEMANDS.items() if op is not None and op(code)}
    return frozenset(found)


def main_features(desc):
    """The levels a built descriptor's main program demands (none without one): what AirBuilder.build() recorded as desc.main_features,
    or, for a descriptor put together by hand, what its C arrays show."""
    main = getattr(desc, "main_desc", None)
    if main is None:
        return frozenset()
    known = getattr(desc, "main_features", None)
    if known is not None:
        return known
    return _demanded([(main.cols[k].kind, main.cols[k].pad) for k in range(main.n_cols)] if main.cols else [],
                     [main.ops[i].op for i in range(main.n_ops)] if main.ops else [])


def main_level(desc):
    """The level a descriptor's main program is routed to: the highest it demands, or MAIN."""
    return max(main_features(desc), default=MainLevel.MAIN)


def main_suffix(desc):
    """The suffix of the entry points of main_level(desc): the newer ones only where the program needs them."""
    return main_level(desc).suffix


# Whether a descriptor's main program holds what demands a level - a fact about the program, not about where it is routed.
def needs_rec(desc): return MainLevel.REC in main_features(desc)
def needs_lk(desc): return MainLevel.LK in main_features(desc)
def needs_link(desc): return MainLevel.LINK in main_features(desc)
def needs_div(desc): return MainLevel.DIV in main_features(desc)
def needs_fetch(desc): return MainLevel.FETCH in main_features(desc)
def needs_word(desc): return MainLevel.WORD in main_features(desc)
def needs_int(desc): return MainLevel.INT in main_features(desc)
def needs_multi(desc): return MainLevel.MULTI in main_features(desc)


def route(desc, call):
    """Where a built descriptor goes for call = "prove", "check_trace" or "verify" - new entry points only when the descriptor needs
    them: (the entry point's name, its arguments between `air` and the trace / the options, keepalive).  _pub for boundary values
    computed from the challenges or an auxiliary program that reads a table, _ext for strides, else the parts one by one (the
    verifier takes no auxiliary program).  A descriptor with a main-trace program (desc.main_desc) is proved and checked through the
    entry points of its MainLevel (main_level), which take everything the _pub ones do; it is verified as if it had none."""
    def ref(part):
        return None if part is None else ctypes.byref(part)
    aux, per = getattr(desc, "aux_desc", None), getattr(desc, "periodic_desc", None)
    main = getattr(desc, "main_desc", None)
    if main is not None and call != "verify":
        # a main-trace program: the trace argument holds its input columns (a verifier never learns how the trace was made)
        ext = ext_of(desc)
        return f"sp_air_{call}_{main_suffix(desc)}", (ctypes.byref(ext), ref(getattr(desc, "boundary_desc", None)), ctypes.byref(main)), ext
    if needs_pub(desc):
        ext = ext_of(desc)
        return f"sp_air_{call}_pub", (ctypes.byref(ext), ref(getattr(desc, "boundary_desc", None))), ext
    if getattr(desc, "stride_desc", None) is not None:
        ext = ext_of(desc)
        return f"sp_air_{call}_ext", (ctypes.byref(ext),), ext
    if call == "check_trace":
        return "sp_air_check_trace", (ref(aux), ref(per)), None
    if call == "verify":
        return ("sp_air_verify_periodic", (ref(per),), None) if per is not None else ("sp_air_verify_backend", (), None)
    if per is not None:
        return "sp_air_prove_periodic", (ref(aux), ref(per)), None
    return ("sp_air_prove_aux", (ref(aux),), None) if aux is not None else ("sp_air_prove", (), None)


class AirViolationC(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("index", ctypes.c_uint32), ("rows", ctypes.c_uint64), ("first_row", ctypes.c_uint64),
                ("last_row", ctypes.c_uint64), ("value", ctypes.c_uint8 * 32)]


def _check_violation_layout():
    from . import _lib
    want = _lib.load().sp_air_violation_size()
    if ctypes.sizeof(AirViolationC) != want:
        raise ImportError(f"AirViolationC is {ctypes.sizeof(AirViolationC)} bytes, the library's sp_air_violation {want}: the binding is out of date")


# One violated constraint, as sp_air_check_trace reports it (sp_air_violation): kind 0 a transition constraint (index = its number;
# rows = enforced rows on which it is non-zero, first_row / last_row the lowest / highest of them, value its evaluation on first_row),
# kind 1 a boundary constraint (index into the builder's list; rows 1, first_row = last_row = its step, value the cell found).
Violation = collections.namedtuple("Violation", "kind index rows first_row last_row value")
TRANSITION, BOUNDARY = 0, 1


def periodic_desc(columns):
    """[values0, values1, ...] (ints) -> (AirPeriodicDescC, keepalive): sp_air_periodic_desc, canonical big-endian values."""
    _check_periodic_layout()
    cols = (AirPeriodicColumnC * max(1, len(columns)))()
    bufs = []
    for k, values in enumerate(columns):
        buf = ctypes.create_string_buffer(b"".join((int(v) % P).to_bytes(32, "big") for v in values), max(1, 32 * len(values)))
        bufs.append(buf)
        cols[k].period, cols[k].values = len(values), ctypes.cast(buf, ctypes.c_void_p)
    d = AirPeriodicDescC()
    d.n_cols, d.cols = len(columns), ctypes.cast(cols, ctypes.POINTER(AirPeriodicColumnC))
    return d, (cols, bufs)


class Value:
    """An SSA value of the constraint program; arithmetic operators emit ops into the owning builder."""

    def __init__(self, builder, index):
        self.b, self.i = builder, index

    def _lift(self, other):
        return self.b._lift(other)

    def __add__(self, o): return self.b._emit(OP_ADD, self.i, self._lift(o).i)
    def __sub__(self, o): return self.b._emit(OP_SUB, self.i, self._lift(o).i)
    def __mul__(self, o): return self.b._emit(OP_MUL, self.i, self._lift(o).i)
    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o): return self._lift(o) - self

    def _div(self, num, den):
        if not hasattr(self.b, "div"):
            raise ValueError("a quotient (/) lives in a main-trace program only, behind the seed or step of a chain group (b.main.div); a constraint, "
                             "auxiliary or boundary program has N / D of a column or a boundary value instead")
        return self.b.div(num, den)

    def __truediv__(self, o): return self._div(self, self._lift(o))
    def __rtruediv__(self, o): return self._div(self._lift(o), self)


class _Program:
    """What every builder of a straight-line program shares: ops [(op, a, b)], the constants - interned, so that the first sight of a
    value appends it - and the emitter that Value's operators go through."""

    def __init__(self):
        self.ops, self.consts = [], []
        self._const_at = {}

    def _emit(self, op, a, b):
        self.ops.append((op, a, b))
        return Value(self, len(self.ops) - 1)

    def const(self, v):
        v %= P
        if v not in self._const_at:
            self._const_at[v] = len(self.consts)
            self.consts.append(v)
        return self._emit(OP_CONST, self._const_at[v], 0)

    def _lift(self, x):
        return x if isinstance(x, Value) else self.const(x)


class _ChallengeProgram(_Program):
    """A program that reads the RAP challenges (n_rap of them): a CONST whose index carries _RAP_TAG until resolved_ops() resolves it."""
    _what = None    # the prefix of the refusal: "aux program", "public values"

    def rap(self, i):
        if not 0 <= i < self.n_rap:
            raise ValueError(f"{self._what}: RAP challenge {i} of {self.n_rap}")
        return self._emit(OP_CONST, _RAP_TAG | i, 0)

    def resolved_ops(self):
        """The ops as the library reads them: RAP challenges follow the constants."""
        return [(op, len(self.consts) + (a & ~_RAP_TAG) if op == OP_CONST and a & _RAP_TAG else a, b) for op, a, b in self.ops]


def _reachable(ops, targets, done=lambda u: False):
    """The ops that the values `targets` depend on, ascending, without those that are `done` and what only they need."""
    todo, stack = set(), list(targets)
    while stack:
        u = stack.pop()
        if u in todo or done(u):
            continue
        todo.add(u)
        stack += _value_operands(*ops[u])
    return sorted(todo)


def _interpret(ops, which, vals, unknown, const, load=None, periodic=None, div=None, out=None, integer=None):
    """vals[t] for the ops `which` (ascending) of `ops`: the one place the op codes are dispatched.  The values are whatever supports
    + - * % - Python integers, or numpy object arrays, one vectorised operation per op.  What differs between the callers comes as
    callables, and an op whose callable is None is unknown to the caller, as is any other code: ValueError(unknown(t, op)).
    const(a) fetches a constant (or a challenge), load(a, b) reads a cell, periodic(a, b) reads op 6, div(num, den) is op 7's quotient and
    out(a, value) takes an OUT (whose own value is what it returns); integer(op, x, y) is an op 8 .. 11 - y the immediate of a LIMB, the
    second value of the others."""
    for t in which:
        op, a, b = ops[t]
        if op == OP_ADD:
            v = (vals[a] + vals[b]) % P
        elif op == OP_SUB:
            v = (vals[a] - vals[b]) % P
        elif op == OP_MUL:
            v = (vals[a] * vals[b]) % P
        elif op == OP_LOAD and load is not None:
            v = load(a, b)
        elif op == OP_CONST:
            v = const(a)
        elif op == OP_PERIODIC and periodic is not None:
            v = periodic(a, b)
        elif op == OP_DIV and div is not None:
            v = div(vals[a], vals[b])
        elif op == OP_OUT and out is not None:
            v = out(a, vals[b])
        elif op in _INT_OPS and integer is not None:
            v = integer(op, vals[a], b if op == OP_INT_LIMB else vals[b])
        else:
            raise ValueError(unknown(t, op))
        vals[t] = v


class AuxProgram(_ChallengeProgram):
    """The auxiliary program of an AIR built with aux_kind=AUX_PROGRAM (sp_air_aux_desc): evaluated once per trace row i on the
    device.  load(shift, col) reads main column `col` of row (i + shift) mod n; product(N, D) and running_sum(N, D) each declare the
    next auxiliary column: z_0 = 1, z_i = z_(i-1) N(i-1) / D(i-1), or z_0 = 0, z_i = z_(i-1) + N(i-1) / D(i-1) (D = 1 when None).
    sorted(key, carry) declares 1 + len(carry) columns: the key and the carried values, each evaluated on the main-trace row alone, in
    the stable ascending order of the rows by the key's canonical integer; sorted_load(shift, k) reads such a column from a product
    or a running sum."""

    _what = "aux program"

    def __init__(self, main_cols, n_rap, periodic_cols=()):
        super().__init__()
        self.main_cols, self.n_rap = main_cols, n_rap
        self.periodic_cols = periodic_cols   # the owning AirBuilder's periodic columns: what table() may read
        self.cols = []
        self.key_bits = {}                   # sorted column -> the bits of its group's key (sp_air_aux_column.pad)

    def load(self, shift, col):
        if not 0 <= shift <= AUX_MAX_SHIFT:
            raise ValueError(f"aux program: row shift {shift} outside 0 .. {AUX_MAX_SHIFT}")
        if not 0 <= col < self.main_cols:
            raise ValueError(f"aux program: column {col} is not a main column (main_cols = {self.main_cols})")
        return self._emit(OP_LOAD, shift, col)

    def periodic(self, row, k):
        raise ValueError("aux program: an auxiliary program cannot read periodic columns (sp_air_prove_periodic refuses op 6 there); "
                         "only the constraint program can")

    def table(self, shift, k):
        """Periodic column k of the owning AirBuilder on row (i + shift): values[(i + shift) mod period] - the public table of a lookup.
        Op 6 in an auxiliary program, which only sp_air_prove_pub and its siblings take."""
        if not 0 <= shift <= AUX_MAX_SHIFT:
            raise ValueError(f"aux program: row shift {shift} outside 0 .. {AUX_MAX_SHIFT}")
        if not 0 <= k < len(self.periodic_cols):
            raise ValueError(f"aux program: column {k} is not one of the AIR's {len(self.periodic_cols)} periodic columns")
        return self._emit(OP_PERIODIC, shift, k)

    def reads_table(self):
        return any(op == OP_PERIODIC for op, _, _ in self.ops)

    def _column(self, kind, num, den):
        num, den = self._lift(num), None if den is None else self._lift(den)
        self.cols.append((kind, num.i, AUX_NO_DEN if den is None else den.i))

    def product(self, num, den=None):
        self._column(AUX_PRODUCT, num, den)

    def running_sum(self, num, den=None):
        self._column(AUX_SUM, num, den)

    def sorted(self, key, carry=(), key_bits=64):
        """Declares 1 + len(carry) auxiliary columns and returns their indices: the key first, then the carried values, row i of each
        holding its expression on row pi(i), pi the stable ascending order of the rows by the key's canonical integer (ties stay in row
        order).  The key must be < 2^key_bits on every row (1 <= key_bits <= 64: the device sorts ceil(key_bits / 8) digits); key and
        carried values depend on the main-trace row only - none may read a sorted column.  Columns declared with the same key Value
        form one group: one sort serves them all."""
        if not 1 <= key_bits <= 64:
            raise ValueError(f"aux program: key_bits {key_bits} outside 1 .. 64")
        values = [self._lift(v) for v in (key, *carry)]
        tainted = self._reads_sorted()
        for v in values:
            if v.b is not self or tainted[v.i]:
                raise ValueError("aux program: the key and the carried values of a sorted column are values of this program that read no sorted column")
        first = len(self.cols)
        for v in values:
            self.key_bits[len(self.cols)] = key_bits
            self.cols.append((AUX_SORTED, v.i, values[0].i))
        return list(range(first, len(self.cols)))

    def sorted_load(self, shift, k):
        """Sorted auxiliary column k (an index sorted() returned) on row (i + shift) mod n: OP_LOAD(shift, main_cols + k)."""
        if not 0 <= shift <= AUX_MAX_SHIFT:
            raise ValueError(f"aux program: row shift {shift} outside 0 .. {AUX_MAX_SHIFT}")
        if not 0 <= k < len(self.cols) or self.cols[k][0] != AUX_SORTED:
            raise ValueError(f"aux program: auxiliary column {k} is not a sorted column declared so far")
        return self._emit(OP_LOAD, shift, self.main_cols + k)

    def _reads_sorted(self):
        """Per op: whether its value depends on a sorted column."""
        tainted = []
        for op, a, b in self.ops:
            if op == OP_LOAD:
                tainted.append(b >= self.main_cols)
            else:
                tainted.append(op in (OP_ADD, OP_SUB, OP_MUL) and (tainted[a] or tainted[b]))
        return tainted

    def sort_groups(self):
        """{key op: [sorted column, ...]} in declaration order."""
        groups = {}
        for k, (kind, _, den_op) in enumerate(self.cols):
            if kind == AUX_SORTED:
                groups.setdefault(den_op, []).append(k)
        return groups

    def evaluate(self, rows, rap, periodic=None):
        """The auxiliary columns in Python integers (the semantics of sp_air_prove_aux): rows = n x main_cols field elements (any
        sequence of rows, or a numpy array of Python ints); returns an (n, len(cols)) numpy object array.  Each op is one vectorised
        numpy operation over all rows; the inverses are one batch inversion; the scans run row by row.  periodic: the columns table()
        reads, one list of values each (None: those of the owning AirBuilder).  Two phases: the ops that read no sorted column, from
        which the sorted columns are built (Python's stable sort by the key's integer; ValueError on a key >= 2^key_bits), then the ops
        that read them."""
        import numpy as np
        m = np.empty((len(rows), self.main_cols), dtype=object)
        m[:, :] = rows if not isinstance(rows, np.ndarray) else rows.astype(object)
        n = m.shape[0]
        consts = list(self.consts) + [int(r) % P for r in rap]
        out = np.empty((n, len(self.cols)), dtype=object)
        tainted = self._reads_sorted()
        vals = [None] * len(self.ops)
        for phase in (False, True):
            self._evaluate_ops(vals, [t for t, late in enumerate(tainted) if late == phase], m, out, consts, periodic)
            if phase:
                break
            for key_op, members in self.sort_groups().items():
                for k in members:
                    if tainted[key_op] or tainted[self.cols[k][1]]:
                        raise ValueError(f"aux program: the key or the value of sorted column {k} reads a sorted column")
                keys = [int(x) for x in vals[key_op]]
                worst = max(range(n), key=keys.__getitem__)
                for k in members:
                    if keys[worst] >> self.key_bits.get(k, 64):
                        raise ValueError(f"aux program: a sort key is out of range (row {worst} has {keys[worst]} >= 2^{self.key_bits.get(k, 64)}, column {k})")
                order = sorted(range(n), key=keys.__getitem__)
                for k in members:
                    out[:, k] = vals[self.cols[k][1]][order]
        dens = [k for k, (kind, _, d) in enumerate(self.cols) if d != AUX_NO_DEN and kind != AUX_SORTED]
        flat = [int(x) for k in dens for x in vals[self.cols[k][2]]]
        inv = _batch_inverse(flat)
        for k, (kind, num_op, den_op) in enumerate(self.cols):
            if kind == AUX_SORTED:
                continue
            t = vals[num_op]
            if den_op != AUX_NO_DEN:
                j = dens.index(k)
                t = (t * np.array(inv[j * n:(j + 1) * n], dtype=object)) % P
            if kind == AUX_SUM:
                out[0, k] = 0
                out[1:, k] = np.cumsum(t[:-1]) % P
                continue
            z, col = 1, out[:, k]
            for i in range(n):
                col[i] = z
                z = z * int(t[i]) % P
        return out

    def _evaluate_ops(self, vals, which, m, out, consts, periodic):
        """vals[t] for the ops `which` (ascending), each one vectorised operation over all rows; a LOAD beyond the main columns reads
        the sorted column of `out`."""
        import numpy as np
        n = m.shape[0]

        def table(a, b):
            values = (self.periodic_cols if periodic is None else periodic)[b]
            return np.array([int(x) % P for x in values], dtype=object)[(np.arange(n) + a) % len(values)]

        _interpret(self.resolved_ops(), which, vals, lambda t, op: f"aux program: op {op}", lambda a: np.full(n, consts[a], dtype=object),
                   load=lambda a, b: np.roll(m[:, b] if b < self.main_cols else out[:, b - self.main_cols], -a), periodic=table)


def _batch_inverse(xs):
    """Montgomery's trick over Python integers; ValueError on a zero (sp_air_prove_aux answers SP_E_ZERO_INVERSE there)."""
    pre, acc = [], 1
    for x in xs:
        if x % P == 0:
            raise ValueError("aux program: a denominator is zero")
        pre.append(acc)
        acc = acc * x % P
    inv = pow(acc, P - 2, P)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % P
        inv = inv * xs[i] % P
    return out


class MainProgram(_Program):
    """The main-trace program of an AIR built with main_inputs=I (sp_air_main_desc): the caller supplies main columns 0 .. I - 1, the
    device derives the others, each a row-local function of columns that exist already.  load(shift, col) reads main column `col` - an
    input, or a derived column declared so far - on row (i + shift) mod n; every declaration below adds the next main column and returns
    its index:

        value(N, D)          z_i = N(i) / D(i)   (D = 1 when None): intermediate products, selectors, anything row-local
        inv_or_zero(x)       z_i = 0 where x(i) = 0, else 1 / x(i): the witness of an is-zero gadget
        bit(x, j)            z_i = bit j (0 .. 251) of the canonical integer of x(i); bits(x, count): bits 0 .. count - 1
        running_sum(N, D)    z_0 = 0, z_i = z_(i-1) + N(i-1) / D(i-1): counters and running totals
        product(N, D)        z_0 = 1, z_i = z_(i-1) N(i-1) / D(i-1)

    A column that reads a derived column must come after it.  A column whose next value is a non-linear function of its own - the
    state of a hash chain - is a true recurrence: a chain group (sp_air_prove_rec).

        g = chain(period, seeds)   len(seeds) columns g.cols (at most 16) in blocks of `period` = 2^l rows, 2 <= period <= n: on the
                                   first row of a block column j is seeds[j] - values that read inputs, earlier columns and periodic
                                   columns -, on every other row what g.step gave on the row before
        g.state(j)                 the group's column j on the current row (a LOAD at shift 0: the only way a step reads its group)
        g.step([next_0, ...])      the value of each column on the NEXT row, all computed from the current one; closes the group
        periodic(shift, k)         periodic column k of the AirBuilder on row (i + shift): values[(i + shift) mod period_k] (op 6)

    Between chain() and step() no other column can be declared.  Seeds and steps are polynomial, unless they divide (sp_air_prove_div):

        div(num, den)              num / den, also written num / den: a value like any other - it may feed further arithmetic and
                                   another quotient, and several next values may share it - but only the seed or the step of a chain
                                   group may depend on it.  A zero den on a row the group evaluates fails the call (SP_E_ZERO_INVERSE;
                                   ValueError in evaluate).  A row-local quotient is value(N, D), which is far cheaper.

    Blocks seeded from the block before - a sponge that absorbs several blocks, a Merkle path - are a linked group (sp_air_prove_link):

        g = chain(period, None, width=w, link=L)   L = 2^k consecutive blocks form a run of L * period rows, L * period <= n
        g.carry(j)                 while the seeds are declared: the group's column j on the last row of the block before, and zero on
                                   the first block of a run (a LOAD of the group at shift 0 inside a seed)
        g.seed([seed_0, ...])      the seeds, which may read any column's carry; then g.state / g.step as above

    A lookup multiplicity (sp_air_prove_lk) is no row-local column either: it joins one value against another over all rows.

        multiplicity(X, T, key_bits)   z_i = #{ j : X(j) = T(i) } on the first row i that holds the table value T(i), 0 on its later
                                       rows: the column m of a LogUp lookup of X into the table T.  X and T are values of this
                                       program whose canonical integers stay below 2^key_bits (1 .. 64) on every row; a tuple is
                                       packed on both sides.  At most 16 such columns.

    The looked-up result itself (sp_air_prove_fetch) is the same join read the other way:

        fetch(X, T, V, key_bits)       a column z_i = V(j*), j* the lowest row j with T(j) = X(i): the result of a lookup of the key X
                                       into the table whose row j holds the key T(j) and the value V(j) - c = a xor b, the word at a
                                       program counter, a read from read-only memory.  X and T as for multiplicity; V is any value.
                                       Returns the column as a Value (a load at shift 0).  A key that no table row holds fails the
                                       call (SP_E_INVALID_ARG; ValueError in evaluate): idle rows point at a key the table holds.
        fetch_many(X, T, [V...], key_bits)   one column per V, declared as one run: the device sorts the table and searches once for
                                       up to 16 of them - the fields of an instruction word.  At most 64 FETCH columns.

    Pieces of a value's canonical integer int(x), 0 <= int(x) < p, wider than one bit, and bitwise functions of two
    (sp_air_prove_word), are row-local again:

        limb(x, lo, width)             z_i = (int(x(i)) >> lo) mod 2^width, 1 <= width, lo + width <= 252: a 16-bit limb of a range
                                       check, a field of an instruction word.  Returns the column's index.
        limbs(x, width, count)         `count` consecutive limbs of `width` bits from bit 0, one column each; they share x (the
                                       device takes it out of Montgomery form once per row)
        word_and(x, y, bits), word_or, word_xor   z_i = int(x(i)) AND / OR / XOR int(y(i)), 1 <= bits <= 251.  An x or y at or above
                                       2^bits on some row fails the call (SP_E_INVALID_ARG; ValueError in evaluate).  Columns with one
                                       x, y and bits share their two passes out of Montgomery form.
        A shift, a rotation, NOT, an add with carry or a comparison is a limb and a value: rotl(x, r) over w bits is
        value(limb(x, 0, w - r) 2^r + limb(x, w - r, r)).

    A recurrence whose next state is an integer function of the state - a round of an ARX cipher, of SHA-2 or of Blake - takes the same
    functions as values inside a seed or a step (sp_air_prove_int), where a column cannot stand:

        int_limb(x, lo, width)         (int(x) >> lo) mod 2^width as a value (op 8), 1 <= width, lo + width <= 252
        int_and(x, y), int_or, int_xor int(x) AND / OR / XOR int(y) as a value (ops 9 .. 11).  An x or y at or above 2^251 on a row the
                                       group evaluates fails the call (SP_E_INVALID_ARG; ValueError in evaluate)
        int_rotl(x, r, bits), int_rotr(x, r, bits), int_add(x, y, bits)   a rotation of a `bits`-wide word and (x + y) mod 2^bits, written
                                       with int_limb and field ops
        Like a quotient, such a value may feed anything, but only the seed or the step of a chain group may depend on it.

    The usual shape of a lookup argument - many columns looked up in one table under ONE multiplicity column (sp_air_prove_multi):

        multiplicity_many(xs, table, key_bits)   z_i = the number of (k, j) with xs[k](j) = table(i) on the first row of each table value,
                                       0 on its repeats: a joint COUNT column over 1 .. 16 looked-up values, each as the x of
                                       multiplicity(); the device sorts the table once and searches it from every looked-up key."""

    def __init__(self, input_cols, main_cols, periodic_cols=()):
        if not 1 <= input_cols < main_cols:
            raise ValueError(f"main program: {input_cols} input columns of {main_cols} main columns (at least one input, at least one derived)")
        super().__init__()
        self.input_cols, self.main_cols = input_cols, main_cols
        self.periodic_cols = periodic_cols   # the owning AirBuilder's periodic columns: what periodic() may read
        self.cols = []                       # (kind, num_op, den_op, pad)
        self._open = None                    # the chain group between chain() and step()
        # the entry points whose decoder check() mirrors: multiplicity(), chain(link > 1), div(), fetch_many(), limb() and word_*() raise it
        self.level = MainLevel.REC

    lookups = property(lambda self: self.level >= MainLevel.LK)     # what was declared, as the level says it
    links = property(lambda self: self.level >= MainLevel.LINK)
    divs = property(lambda self: self.level >= MainLevel.DIV)
    fetches = property(lambda self: self.level >= MainLevel.FETCH)
    words = property(lambda self: self.level >= MainLevel.WORD)
    ints = property(lambda self: self.level >= MainLevel.INT)
    multis = property(lambda self: self.level >= MainLevel.MULTI)

    def load(self, shift, col):
        if not 0 <= shift <= AUX_MAX_SHIFT:
            raise ValueError(f"main program: row shift {shift} outside 0 .. {AUX_MAX_SHIFT}")
        if not 0 <= col < self.input_cols + len(self.cols):
            raise ValueError(f"main program: column {col} is neither an input nor a derived column declared so far")
        if self._open is not None and col in self._open.cols:
            if self._open.seeding and self._open.link == 1:
                raise ValueError(f"main program: a seed reads its own chain group only in a linked group (column {col}; chain(..., link=L))")
            if shift != 0:
                raise ValueError(f"main program: a {'seed' if self._open.seeding else 'step'} reads its own chain group at shift 0 only (column {col} at shift {shift})")
        return self._emit(OP_LOAD, shift, col)

    def periodic(self, shift, k):
        """Periodic column k of the owning AirBuilder on row (i + shift): op 6, which only sp_air_prove_rec and its siblings take."""
        if not 0 <= shift <= AUX_MAX_SHIFT:
            raise ValueError(f"main program: row shift {shift} outside 0 .. {AUX_MAX_SHIFT}")
        if not 0 <= k < len(self.periodic_cols):
            raise ValueError(f"main program: column {k} is not one of the AIR's {len(self.periodic_cols)} periodic columns")
        return self._emit(OP_PERIODIC, shift, k)

    def div(self, num, den):
        """num / den (op 7): see the class.  Legal behind the seed or step of a chain group only, which check() holds the columns to."""
        num, den = self._lift(num), self._lift(den)
        if num.b is not self or den.b is not self:
            raise ValueError("main program: the operands of a quotient must be values of this program")
        self.level = max(self.level, MainLevel.DIV)
        return self._emit(OP_DIV, num.i, den.i)

    def _own(self, *values):
        values = [self._lift(v) for v in values]
        if any(v.b is not self for v in values):
            raise ValueError("main program: the operands of an integer op must be values of this program")
        self.level = max(self.level, MainLevel.INT)
        return values

    def int_limb(self, x, lo, width):
        """(int(x) >> lo) mod 2^width as a value (op 8): see the class.  Legal behind the seed or step of a chain group only."""
        if lo < 0 or width < 1 or lo + width > MAIN_LIMB_MAX_END:
            raise ValueError(f"main program: a limb of {width} bits from bit {lo} (1 <= width, 0 <= lo, lo + width <= {MAIN_LIMB_MAX_END})")
        x, = self._own(x)
        return self._emit(OP_INT_LIMB, x.i, lo + 256 * width)

    def int_and(self, x, y):
        """int(x) AND int(y) of two values below 2^251 as a value (op 9): see the class."""
        x, y = self._own(x, y)
        return self._emit(OP_INT_AND, x.i, y.i)

    def int_or(self, x, y):
        x, y = self._own(x, y)
        return self._emit(OP_INT_OR, x.i, y.i)

    def int_xor(self, x, y):
        x, y = self._own(x, y)
        return self._emit(OP_INT_XOR, x.i, y.i)

    def int_rotl(self, x, r, bits):
        """x, below 2^bits, rotated left by r of its `bits` bits: limb(x, 0, bits - r) 2^r + limb(x, bits - r, r)."""
        r %= bits
        if r == 0:
            return self.int_limb(x, 0, bits)
        x, = self._own(x)
        return self.int_limb(x, 0, bits - r) * (1 << r) + self.int_limb(x, bits - r, r)

    def int_rotr(self, x, r, bits):
        return self.int_rotl(x, -r % bits, bits)

    def int_add(self, x, y, bits):
        """(x + y) mod 2^bits, for x + y below 2^252 as a canonical integer: limb(x + y, 0, bits)."""
        x, y = self._own(x, y)
        return self.int_limb(x + y, 0, bits)

    def chain(self, period, seeds, width=None, link=1):
        """Opens a chain group of len(seeds) columns in blocks of `period` rows (see the class); returns its ChainGroup.  link = L > 1
        (a power of two) links L consecutive blocks into a run.  seeds=None with width=w declares the columns first and takes the
        seeds through g.seed([...]), which may then read g.carry(j)."""
        if self._open is not None:
            raise ValueError("main program: a chain group is open (g.step closes it)")
        if period < 2 or period & (period - 1):
            raise ValueError(f"main program: the block length {period} of a chain group is not a power of two >= 2")
        if link < 1 or link & (link - 1) or link.bit_length() - 1 > MAIN_LINK_MAX_LOG:
            raise ValueError(f"main program: a run of {link} blocks is not a power of two (1 .. 2^{MAIN_LINK_MAX_LOG})")
        if seeds is None and width is None:
            raise ValueError("main program: chain(period, None) needs width=w, the number of columns whose seeds g.seed will give")
        w = len(seeds) if seeds is not None else width
        if width is not None and width != w:
            raise ValueError(f"main program: {w} seeds for a chain group of width {width}")
        if not 1 <= w <= MAIN_CHAIN_MAX_WIDTH:
            raise ValueError(f"main program: a chain group of {w} columns (1 .. {MAIN_CHAIN_MAX_WIDTH})")
        log = period.bit_length() - 1
        first = self.input_cols + len(self.cols)
        deferred = seeds is None
        if deferred:
            seeds = [self.const(0)] * w    # (den_op, the seed, is filled in by g.seed)
        else:
            seeds = [self._lift(x) for x in seeds]
        for j, seed in enumerate(seeds):   # (num_op, the step, is filled in by g.step)
            self._column(MAIN_CHAIN, seed, seed, log + 256 * j + 65536 * (link.bit_length() - 1))
        if link > 1:
            self.level = max(self.level, MainLevel.LINK)
        self._open = ChainGroup(self, list(range(first, first + w)), period, link, seeding=deferred)
        return self._open

    def _column(self, kind, num, den=None, pad=0):
        num, den = self._lift(num), None if den is None else self._lift(den)
        if num.b is not self or (den is not None and den.b is not self):
            raise ValueError("main program: N and D must be values of this program")
        if self._open is not None:
            raise ValueError("main program: a chain group is open: g.step([...]) closes it before another column is declared")
        if self.input_cols + len(self.cols) >= self.main_cols:
            raise ValueError(f"main program: more derived columns than main_cols - main_inputs = {self.main_cols - self.input_cols}")
        self.cols.append((kind, num.i, AUX_NO_DEN if den is None else den.i, pad))
        return self.input_cols + len(self.cols) - 1

    def value(self, num, den=None):
        return self._column(MAIN_VALUE, num, den)

    def inv_or_zero(self, x):
        return self._column(MAIN_INV_OR_ZERO, x)

    def bit(self, x, j):
        if not 0 <= j <= MAIN_MAX_BIT:
            raise ValueError(f"main program: bit {j} outside 0 .. {MAIN_MAX_BIT}")
        return self._column(MAIN_BIT, x, None, j)

    def bits(self, x, count):
        """Bits 0 .. count - 1 of x, one column each (they share x: the device takes it out of Montgomery form once per row)."""
        x = self._lift(x)
        return [self.bit(x, j) for j in range(count)]

    def running_sum(self, num, den=None):
        return self._column(MAIN_SUM, num, den)

    def product(self, num, den=None):
        return self._column(MAIN_PRODUCT, num, den)

    def multiplicity(self, x, table, key_bits=64):
        """The lookup multiplicity of x in table (see the class): a COUNT column; returns its index."""
        if table is None:
            raise ValueError("main program: a multiplicity column needs a table value")
        if not 1 <= key_bits <= MAIN_COUNT_MAX_KEY_BITS:
            raise ValueError(f"main program: key_bits {key_bits} outside 1 .. {MAIN_COUNT_MAX_KEY_BITS}")
        if sum(1 for c in self.cols if c[0] == MAIN_COUNT) >= MAIN_COUNT_MAX_COLS:
            raise ValueError(f"main program: more than {MAIN_COUNT_MAX_COLS} multiplicity columns")
        self.level = max(self.level, MainLevel.LK)
        return self._column(MAIN_COUNT, x, table, key_bits)

    def multiplicity_many(self, xs, table, key_bits=64):
        """One multiplicity column for the 1 .. 16 looked-up values xs in one table (see the class): a joint COUNT column - bit 8 of its
        pad, its num_op the first of a list of op 12 cells, one per x - (sp_air_prove_multi); returns its index."""
        xs = list(xs)
        if table is None:
            raise ValueError("main program: a multiplicity column needs a table value")
        if not 1 <= len(xs) <= MAIN_COUNT_MAX_LIST:
            raise ValueError(f"main program: a multiplicity column over {len(xs)} looked-up values (1 .. {MAIN_COUNT_MAX_LIST})")
        if not 1 <= key_bits <= MAIN_COUNT_MAX_KEY_BITS:
            raise ValueError(f"main program: key_bits {key_bits} outside 1 .. {MAIN_COUNT_MAX_KEY_BITS}")
        if sum(1 for c in self.cols if c[0] == MAIN_COUNT) >= MAIN_COUNT_MAX_COLS:
            raise ValueError(f"main program: more than {MAIN_COUNT_MAX_COLS} multiplicity columns")
        xs = [self._lift(x) for x in xs]
        if any(x.b is not self for x in xs):
            raise ValueError("main program: the looked-up values of a multiplicity column must be values of this program")
        table = self._lift(table)
        cell = LIST_END
        for x in reversed(xs):      # X_0 is the a of the cell the column names, X_1 that of its b, ...
            cell = self._emit(OP_ALSO, x.i, cell).i
        self.level = max(self.level, MainLevel.MULTI)
        return self._column(MAIN_COUNT, Value(self, cell), table, key_bits + MAIN_COUNT_LIST)

    def list_of(self, cell):
        """The ops X_0, X_1, .. of the list that starts at the op 12 `cell`."""
        xs = []
        while cell != LIST_END:
            _, a, cell = self.ops[cell]
            xs.append(a)
        return xs

    def fetch(self, x, table_key, table_value, key_bits=64):
        """The value of the table row whose key is x (see the class): a FETCH column; returns it as a Value."""
        return self.fetch_many(x, table_key, [table_value], key_bits)[0]

    def fetch_many(self, x, table_key, table_values, key_bits=64):
        """One FETCH column per table value, as one run that shares x, table_key and key_bits; returns the columns as Values."""
        if table_key is None:
            raise ValueError("main program: a fetch needs a table key")
        if not 1 <= key_bits <= MAIN_FETCH_MAX_KEY_BITS:
            raise ValueError(f"main program: key_bits {key_bits} outside 1 .. {MAIN_FETCH_MAX_KEY_BITS}")
        table_values = list(table_values)
        if not table_values:
            raise ValueError("main program: a fetch needs at least one table value")
        if sum(1 for c in self.cols if c[0] == MAIN_FETCH) + len(table_values) > MAIN_FETCH_MAX_COLS:
            raise ValueError(f"main program: more than {MAIN_FETCH_MAX_COLS} fetched columns")
        x, table_key = self._lift(x), self._lift(table_key)
        values = [self._lift(v) for v in table_values]
        if any(v.b is not self for v in values):
            raise ValueError("main program: the table values of a fetch must be values of this program")
        if max(v.i for v in values) >= 1 << 16:
            raise ValueError("main program: the table value of a fetch must be one of the program's first 65536 ops (v_op rides in 16 bits of the pad)")
        self.level = max(self.level, MainLevel.FETCH)
        cols = [self._column(MAIN_FETCH, x, table_key, key_bits + 256 * v.i) for v in values]
        return [self.load(0, c) for c in cols]

    def limb(self, x, lo, width):
        """Bits lo .. lo + width - 1 of the canonical integer of x (see the class): a LIMB column; returns its index."""
        if lo < 0 or width < 1 or lo + width > MAIN_LIMB_MAX_END:
            raise ValueError(f"main program: a limb of {width} bits from bit {lo} (1 <= width, 0 <= lo, lo + width <= {MAIN_LIMB_MAX_END})")
        self.level = max(self.level, MainLevel.WORD)
        return self._column(MAIN_LIMB, x, None, lo + 256 * width)

    def limbs(self, x, width, count):
        """`count` consecutive limbs of `width` bits of x from bit 0, one column each (they share x: one group on the device)."""
        if count < 1 or width < 1 or width * count > MAIN_LIMB_MAX_END:
            raise ValueError(f"main program: {count} limbs of {width} bits (at least one, and width * count <= {MAIN_LIMB_MAX_END})")
        x = self._lift(x)
        return [self.limb(x, j * width, width) for j in range(count)]

    def _word(self, fn, x, y, bits):
        if y is None:
            raise ValueError("main program: a word column needs two operands")
        if not 1 <= bits <= MAIN_WORD_MAX_BITS:
            raise ValueError(f"main program: words of {bits} bits (1 .. {MAIN_WORD_MAX_BITS})")
        self.level = max(self.level, MainLevel.WORD)
        return self._column(MAIN_WORD, x, y, fn + 256 * bits)

    def word_and(self, x, y, bits):
        """int(x) AND int(y) of two values below 2^bits (see the class): a WORD column; returns its index."""
        return self._word(WORD_AND, x, y, bits)

    def word_or(self, x, y, bits):
        return self._word(WORD_OR, x, y, bits)

    def word_xor(self, x, y, bits):
        return self._word(WORD_XOR, x, y, bits)

    def reads(self):
        """Per op: one more than the highest derived column its value depends on (0: inputs only) - what the decoder follows."""
        return self._reads(False)

    def _reads(self, shifted_only):
        reads = []
        for op, a, b in self.ops:
            if op == OP_LOAD:
                reads.append(max(0, b - self.input_cols + 1) if a or not shifted_only else 0)
            else:
                reads.append(max((reads[u] for u in _marked_operands(op, a, b)), default=0))
        return reads

    def _quotients(self):
        """Per op: whether its value depends on a quotient (op 7) - the decoder's mark of the same name."""
        quot = []
        for op, a, b in self.ops:
            quot.append(op == OP_DIV or any(quot[u] for u in _marked_operands(op, a, b)))
        return quot

    def _integers(self):
        """Per op: whether its value depends on an integer op 8 .. 11 - the decoder's other chain-only mark."""
        ints = []
        for op, a, b in self.ops:
            ints.append(op in _INT_OPS or any(ints[u] for u in _marked_operands(op, a, b)))
        return ints

    def check(self, n=None, level=None):
        """The decoder's rules (air_statement_from_c), for a program whose lists were filled by hand too: ValueError naming the first one
        broken.  n: the trace length a chain group's block length is held against (None: not yet known).  level: the MainLevel whose
        decoder is mirrored (None: self.level, where the program would be routed after what was declared).  Below LK kind 6 is an
        unknown kind; below LINK the bits of a CHAIN column's pad at and above 16 belong to j; below DIV op 7 is a malformed op; below
        FETCH kind 7 is an unknown kind; below WORD kinds 8 and 9 are; below INT ops 8 .. 11 are malformed ops; below MULTI op 12 is one and
        a COUNT column's pad with bit 8 a key_bits out of range.  The _main entry points' refusal of chain columns and op 6 was
        never modelled here, and is not: MAIN is judged as REC."""
        level = self.level if level is None else level
        lookups, links, divs, fetches = (level >= at for at in (MainLevel.LK, MainLevel.LINK, MainLevel.DIV, MainLevel.FETCH))
        words, ints, multis = level >= MainLevel.WORD, level >= MainLevel.INT, level >= MainLevel.MULTI
        pos = (lambda pad: (pad >> 8) & 255) if links else (lambda pad: pad >> 8)
        n_count = n_fetch = 0
        if self._open is not None:
            raise ValueError("main program: a chain group is open: g.step([...]) closes it")
        if self.input_cols < 1 or not self.cols or self.input_cols + len(self.cols) != self.main_cols:
            raise ValueError(f"main program: {self.input_cols} input + {len(self.cols)} derived columns, the AIR has main_cols = {self.main_cols}")
        for t, (op, a, b) in enumerate(self.ops):
            if op == OP_PERIODIC and 0 <= a <= AUX_MAX_SHIFT and not 0 <= b < len(self.periodic_cols):
                raise ValueError(f"main program: op {t} reads periodic column {b}, and the AIR has {len(self.periodic_cols)}")
            ok = ((op == OP_LOAD and 0 <= a <= AUX_MAX_SHIFT and 0 <= b < self.main_cols) or (op == OP_CONST and 0 <= a < len(self.consts)) or
                  (op in (OP_ADD, OP_SUB, OP_MUL) and 0 <= a < t and 0 <= b < t) or (op == OP_PERIODIC and 0 <= a <= AUX_MAX_SHIFT) or
                  (divs and op == OP_DIV and 0 <= a < t and 0 <= b < t))
            if multis:      # (a list cell, and what takes one for a value, by name)
                def cell(u, t=t):
                    return 0 <= u < t and self.ops[u][0] == OP_ALSO
                if op == OP_ALSO:
                    if not 0 <= a < t or self.ops[a][0] in (OP_OUT, OP_ALSO):
                        raise ValueError(f"main program: op {t} is a list cell (op 12) whose a = {a} is no earlier value op (a cell names one looked-up value, and no cell)")
                    if b != LIST_END and not cell(b):
                        raise ValueError(f"main program: op {t} is a list cell (op 12) whose b = {b} is neither 0xFFFF nor an earlier cell (b names the rest of the list)")
                    ok = True
                elif any(cell(u) for u in _value_operands(op, a, b)) or (op == OP_OUT and cell(b)):
                    raise ValueError(f"main program: op {t} takes a list cell (op 12) for an operand, and a cell has no value")
            if ints and op in _INT_OPS:
                earlier = [0 <= u < t and self.ops[u][0] != OP_OUT for u in _value_operands(op, a, b)]
                if not all(earlier):
                    raise ValueError(f"main program: op {t} is an integer op (op {op}) whose operands are not earlier values (LIMB: a; AND / OR / XOR: a and b)")
                if op == OP_INT_LIMB and b >> 8 == 0:
                    raise ValueError(f"main program: op {t} is a LIMB op with width = 0 (b = lo + 256 width, 1 <= width, lo + width <= {MAIN_LIMB_MAX_END})")
                if op == OP_INT_LIMB and (b & 255) + (b >> 8) > MAIN_LIMB_MAX_END:
                    raise ValueError(f"main program: op {t} is a LIMB op with lo + width = {(b & 255) + (b >> 8)} (b = lo + 256 width, 1 <= width, "
                                     f"lo + width <= {MAIN_LIMB_MAX_END})")
                ok = True
            if not ok and ints:
                raise ValueError(f"main program: malformed op {t} (LOAD, CONST, ADD, SUB, MUL, DIV, LIMB, AND, OR, XOR over earlier ops, PERIODIC only)")
            if not ok and divs:
                raise ValueError(f"main program: malformed op {t} (LOAD, CONST, ADD, SUB, MUL, DIV over earlier ops, PERIODIC only)")
            if not ok:
                raise ValueError(f"main program: malformed op {t} (LOAD, CONST, ADD, SUB, MUL over earlier ops, PERIODIC only)")
        reads, shifted, quot, integers = self.reads(), self._reads(True), self._quotients(), self._integers()
        refused = ("depends on a quotient (op 7), which only the seed or the step of a CHAIN column may: a row-local quotient is a VALUE "
                   "column's N / D")
        refused_int = ("depends on an integer op (ops 8 .. 11), which only the seed or the step of a CHAIN column may: a row-local limb or word "
                       "is a LIMB or WORD column")

        def chain_only(k, *operands):   # (the quotient's refusal first, as the decoder)
            if any(quot[u] for u in operands):
                raise ValueError(f"main program: derived column {k} {refused}")
            if any(integers[u] for u in operands):
                raise ValueError(f"main program: derived column {k} {refused_int}")
        def is_cell(t):
            return 0 <= t < len(self.ops) and self.ops[t][0] == OP_ALSO
        list_len = []       # of an op 12: the cells of its list, itself included
        for op, a, b in self.ops:
            list_len.append(1 + (list_len[b] if b != LIST_END else 0) if op == OP_ALSO else 0)
        g0 = g_end = 0      # the chain group that column k belongs to is [g0, g_end), when k < g_end
        for k, (kind, num_op, den_op, pad) in enumerate(self.cols):
            den = den_op != AUX_NO_DEN
            if not MAIN_VALUE <= kind <= (MAIN_WORD if words else MAIN_FETCH if fetches else MAIN_COUNT if lookups else MAIN_CHAIN):
                raise ValueError(f"main program: derived column {k} has an unknown kind")
            joint = multis and kind == MAIN_COUNT and pad & MAIN_COUNT_LIST != 0
            if multis and ((den and is_cell(den_op)) or (not joint and is_cell(num_op)) or (kind == MAIN_FETCH and is_cell((pad >> 8) & 65535))):
                raise ValueError(f"main program: derived column {k} names a list cell (op 12), which only the num_op of a COUNT column with bit 8 of its pad may "
                                 "(a cell has no value)")
            if kind in (MAIN_LIMB, MAIN_WORD):
                limb, low, high = kind == MAIN_LIMB, pad & 255, (pad >> 8) & 255      # LIMB: lo, width; WORD: fn, bits
                who = f"main program: derived column {k} is a {'LIMB' if limb else 'WORD'} column"
                if pad >> 16:
                    raise ValueError(f"{who} whose pad has a bit at or above 16 (pad = {'lo + 256 width' if limb else 'fn + 256 bits'})")
                if limb and den:
                    raise ValueError(f"{who} and takes no denominator")
                if not limb and not den:
                    raise ValueError(f"{who} without a second operand (den_op names it)")
                if limb and high == 0:
                    raise ValueError(f"{who} with width = 0 (1 <= width, lo + width <= {MAIN_LIMB_MAX_END})")
                if limb and low + high > MAIN_LIMB_MAX_END:
                    raise ValueError(f"{who} with lo + width = {low + high} (1 <= width, lo + width <= {MAIN_LIMB_MAX_END})")
                if not limb and low >= MAIN_WORD_FUNCTIONS:
                    raise ValueError(f"{who} with fn = {low} (0 AND, 1 OR, 2 XOR)")
                if not limb and not 1 <= high <= MAIN_WORD_MAX_BITS:
                    raise ValueError(f"{who} with bits = {high} (1 .. {MAIN_WORD_MAX_BITS})")
                if not 0 <= num_op < len(self.ops) or (den and not 0 <= den_op < len(self.ops)):
                    raise ValueError(f"main program: derived column {k} names an op beyond the program")
                chain_only(k, num_op, *([den_op] if den else []))
                r = max(reads[num_op], reads[den_op] if den else 0)
                if r > k:
                    raise ValueError(f"main program: derived column {k} reads derived column {r - 1}, which is not an earlier one")
                continue
            if kind == MAIN_FETCH:
                key_bits, v_op = pad & 255, (pad >> 8) & 65535
                if pad >> 24:
                    raise ValueError(f"main program: derived column {k} is a FETCH column whose pad has a bit at or above 24 (pad = key_bits + 256 v_op)")
                if not den:
                    raise ValueError(f"main program: derived column {k} is a FETCH column without a table key (den_op names the table key)")
                if not 1 <= key_bits <= MAIN_FETCH_MAX_KEY_BITS:
                    raise ValueError(f"main program: derived column {k} is a FETCH column with key_bits = {key_bits} (1 .. {MAIN_FETCH_MAX_KEY_BITS})")
                if not (0 <= num_op < len(self.ops) and 0 <= den_op < len(self.ops)):
                    raise ValueError(f"main program: derived column {k} names an op beyond the program")
                if v_op >= len(self.ops) or self.ops[v_op][0] == OP_OUT:
                    raise ValueError(f"main program: derived column {k} is a FETCH column with v_op = {v_op}, which is beyond the program or an OUT")
                chain_only(k, num_op, den_op, v_op)
                r = max(reads[num_op], reads[den_op], reads[v_op])
                if r > k:
                    raise ValueError(f"main program: derived column {k} reads derived column {r - 1}, which is not an earlier one")
                n_fetch += 1
                if n_fetch > MAIN_FETCH_MAX_COLS:
                    raise ValueError(f"main program: derived column {k} is the program's FETCH column number {n_fetch} (at most {MAIN_FETCH_MAX_COLS})")
                continue
            if kind == MAIN_COUNT:
                if not den:
                    raise ValueError(f"main program: derived column {k} is a COUNT column without a table (den_op names the table value)")
                if multis and pad >> 9:
                    raise ValueError(f"main program: derived column {k} is a COUNT column whose pad has a bit above 8 (pad = key_bits, and + 256 when num_op names "
                                     "a list of looked-up values)")
                key_bits = pad & 255 if joint else pad
                if not 1 <= key_bits <= MAIN_COUNT_MAX_KEY_BITS:
                    raise ValueError(f"main program: derived column {k} is a COUNT column with key_bits = {key_bits} (1 .. {MAIN_COUNT_MAX_KEY_BITS})")
                if not (0 <= num_op < len(self.ops) and 0 <= den_op < len(self.ops)):
                    raise ValueError(f"main program: derived column {k} names an op beyond the program")
                if joint and not is_cell(num_op):
                    raise ValueError(f"main program: derived column {k} is a COUNT column with bit 8 of its pad whose num_op = {num_op} is no list cell (op 12 names "
                                     "the looked-up values)")
                if joint and list_len[num_op] > MAIN_COUNT_MAX_LIST:
                    raise ValueError(f"main program: derived column {k} is a COUNT column with a list of more than {MAIN_COUNT_MAX_LIST} looked-up values")
                chain_only(k, num_op, den_op)
                r = max(reads[num_op], reads[den_op])
                if r > k:
                    raise ValueError(f"main program: derived column {k} reads derived column {r - 1}, which is not an earlier one")
                n_count += 1
                if n_count > MAIN_COUNT_MAX_COLS:
                    raise ValueError(f"main program: derived column {k} is the program's COUNT column number {n_count} (at most {MAIN_COUNT_MAX_COLS})")
                continue
            if kind == MAIN_CHAIN:
                log, j, kr = pad & 255, pos(pad), pad >> 16 if links else 0     # kr: the k of a run of 2^k blocks
                if k >= g_end:
                    if j != 0:
                        raise ValueError(f"main program: derived column {k} is a CHAIN column with j = {j} out of sequence (no group is open)")
                    g0, g_end = k, k + 1
                    while g_end < len(self.cols) and self.cols[g_end][0] == MAIN_CHAIN and pos(self.cols[g_end][3]):
                        jj = pos(self.cols[g_end][3])
                        if jj != g_end - g0:
                            raise ValueError(f"main program: derived column {g_end} is a CHAIN column with j = {jj} out of sequence (the next of its group is {g_end - g0})")
                        if jj >= MAIN_CHAIN_MAX_WIDTH:
                            raise ValueError(f"main program: derived column {g_end} makes its chain group longer than {MAIN_CHAIN_MAX_WIDTH} columns")
                        g_end += 1
                if log == 0 or log >= 64 or (n is not None and (1 << log) > n):
                    raise ValueError(f"main program: derived column {k} is a CHAIN column with l = {log} (block length 2^l: 1 <= l and 2^l <= n)")
                if log != self.cols[g0][3] & 255:
                    raise ValueError(f"main program: derived column {k} differs from its chain group in l")
                if kr > MAIN_LINK_MAX_LOG:
                    raise ValueError(f"main program: derived column {k} is a CHAIN column with k = {kr} (runs of 2^k blocks: k <= {MAIN_LINK_MAX_LOG})")
                if kr and (log + kr >= 64 or (n is not None and (1 << (log + kr)) > n)):
                    raise ValueError(f"main program: derived column {k} is a CHAIN column with l + k = {log + kr} (a run is 2^(l + k) rows: 2^(l + k) <= n)")
                if links and kr != self.cols[g0][3] >> 16:
                    raise ValueError(f"main program: derived column {k} differs from its chain group in k")
                if not den:
                    raise ValueError(f"main program: derived column {k} is a CHAIN column without a seed")
                if not (0 <= num_op < len(self.ops) and 0 <= den_op < len(self.ops)):
                    raise ValueError(f"main program: derived column {k} names an op beyond the program")
                r = max(reads[num_op], reads[den_op])
                if r > g_end:
                    raise ValueError(f"main program: derived column {k} reads derived column {r - 1}, which is not an earlier one")
                if kr == 0 and reads[den_op] > g0:
                    raise ValueError(f"main program: derived column {k} has a seed that loads derived column {reads[den_op] - 1} of its own chain group")
                if shifted[den_op] > g0:    # (k >= 1: a load of the group at shift 0 is the carry)
                    raise ValueError(f"main program: derived column {k} has a seed that loads derived column {shifted[den_op] - 1} of its own chain group "
                                     "at a shift other than 0")
                if shifted[num_op] > g0:
                    raise ValueError(f"main program: derived column {k} has a step that loads derived column {shifted[num_op] - 1} of its own chain group "
                                     "at a shift other than 0")
                continue
            if not 0 <= num_op < len(self.ops) or (den and not 0 <= den_op < len(self.ops)):
                raise ValueError(f"main program: derived column {k} names an op beyond the program")
            chain_only(k, num_op, *([den_op] if den else []))
            if den and kind in (MAIN_INV_OR_ZERO, MAIN_BIT):
                raise ValueError(f"main program: derived column {k} is an INV_OR_ZERO or a BIT and takes no denominator")
            if kind == MAIN_BIT and not 0 <= pad <= MAIN_MAX_BIT:
                raise ValueError(f"main program: derived column {k} names bit {pad} (0 .. {MAIN_MAX_BIT})")
            r = max(reads[num_op], reads[den_op] if den else 0)
            if r > k:
                raise ValueError(f"main program: derived column {k} reads derived column {r - 1}, which is not an earlier one")

    def evaluate(self, input_rows):
        """The whole main segment in Python integers (the semantics of sp_air_prove_main): input_rows = n x input_cols field elements;
        returns an (n, main_cols) numpy object array.  Columns in index order, each op one vectorised numpy operation, evaluated when the
        first column that needs it is built (the columns it loads are complete by then).  ValueError on a zero denominator.  A chain
        group is a loop over the rows t of a block, each step vectorised over the n / period blocks; a linked group a loop over the
        blocks of a run and the rows of each, vectorised over the runs, the carry zero in front of each run.  A quotient (op 7) is one
        batch inversion per op and step, over the blocks or runs; ValueError on a zero under one that a seed or a step reaches.  A COUNT
        column is a dictionary count of X, read on the first row of each table value; ValueError on a key at or above 2^key_bits.  A
        FETCH column is a dictionary from each table key to the first row that holds it; ValueError on a key out of range (the COUNT
        columns' words) or on a looked-up key that no row holds.  LIMB and WORD columns are Python's shifts, masks and bitwise operators
        on the integers; ValueError, in the device's words, on a WORD operand at or above 2^bits.  An integer op 8 .. 11 behind a seed or
        a step is the same on the rows its group evaluates; ValueError, in the device's words, on an AND, OR or XOR operand at or
        above 2^251."""
        import numpy as np
        self.check(len(input_rows))
        rows = input_rows if not isinstance(input_rows, np.ndarray) else input_rows.astype(object)
        n = len(rows)
        m = np.empty((n, self.main_cols), dtype=object)
        m[:, :self.input_cols] = rows
        m[:, :self.input_cols] %= P
        vals = [None] * len(self.ops)

        def unknown(u, op):
            return f"main program: op {u} has the unknown code {op}"

        def quotient(num, dens):    # one batch inversion per op 7 (and step, over the blocks or runs)
            try:
                return (num * np.array(_batch_inverse([int(x) for x in dens]), dtype=object)) % P
            except ValueError:
                raise ValueError("main program: a denominator of a quotient (op 7) is zero on some row") from None

        def integer(op, x, y):    # ops 8 .. 11 on the canonical integers, element by element
            xs = [int(v) for v in x]
            if op == OP_INT_LIMB:
                lo, mask = y & 255, (1 << (y >> 8)) - 1
                return np.array([(v >> lo) & mask for v in xs], dtype=object)
            ys = [int(v) for v in y]
            if any(v >> INT_OP_BITS for v in xs) or any(v >> INT_OP_BITS for v in ys):
                raise ValueError("main program: an integer op's operand is out of range on some row (both operands of an AND, OR or XOR op must be "
                                 "below 2^251 as canonical integers)")
            fn = {OP_INT_AND: int.__and__, OP_INT_OR: int.__or__, OP_INT_XOR: int.__xor__}[op]
            return np.array([fn(u, v) for u, v in zip(xs, ys)], dtype=object)

        def need(t):
            """The value of op t on all rows.  (check() lets no row-local column reach an op 7: kept for a program it was not asked about.)"""
            _interpret(self.ops, _reachable(self.ops, [t], lambda u: vals[u] is not None), vals, unknown, lambda a: np.full(n, self.consts[a], dtype=object),
                       load=lambda a, b: np.roll(m[:, b], -a), periodic=lambda a, b: periodic[b][(np.arange(n) + a) % len(periodic[b])], div=quotient, integer=integer)
            return vals[t]

        def run(targets, rows, first, state):
            """The values of the ops `targets` on the rows `rows` alone, a LOAD of group column first + j being state[j]."""
            got = {}
            _interpret(self.ops, _reachable(self.ops, targets), got, unknown, lambda a: np.full(len(rows), self.consts[a], dtype=object),
                       load=lambda a, b: state[b - first] if first <= b < first + len(state) else m[(rows + a) % n, b],
                       periodic=lambda a, b: periodic[b][(rows + a) % len(periodic[b])], div=quotient, integer=integer)
            return [got[u] for u in targets]

        periodic = [np.array(values, dtype=object) for values in self.periodic_cols]
        for k, (kind, num_op, den_op, pad) in enumerate(self.cols):
            if kind == MAIN_CHAIN:
                linked = self.level >= MainLevel.LINK    # (the _div and _fetch entry points read the k of a pad as the _link ones do)
                pos = (lambda pad: (pad >> 8) & 255) if linked else (lambda pad: pad >> 8)
                if pos(pad):
                    continue            # (built with its group, at the column that opens it)
                period, w = 1 << (pad & 255), 1
                while k + w < len(self.cols) and self.cols[k + w][0] == MAIN_CHAIN and pos(self.cols[k + w][3]):
                    w += 1
                link = 1 << (pad >> 16) if linked else 1
                first = self.input_cols + k
                state = [np.zeros(n // (period * link), dtype=object) for _ in range(w)] if link > 1 else []   # the carry in front of a run
                for block in range(link):
                    rows = np.arange(block * period, n, period * link)
                    state = run([self.cols[k + j][2] for j in range(w)], rows, first, state)   # all w seeds together, from the carry
                    for t in range(period):
                        for j in range(w):
                            m[rows + t, first + j] = state[j]
                        if t + 1 < period:   # all w next values from the state of row t, assigned together
                            state = run([self.cols[k + j][1] for j in range(w)], rows + t, first, state)
                continue
            if kind == MAIN_COUNT:
                if pad & MAIN_COUNT_LIST:   # a joint column: every looked-up value of the list, one after the other
                    pad &= 255
                    xs = [int(v) for x_op in self.list_of(num_op) for v in need(x_op)]
                else:
                    xs = [int(v) for v in need(num_op)]
                ts = [int(v) for v in need(den_op)]
                if any(v >> pad for v in xs) or any(v >> pad for v in ts):
                    raise ValueError("main program: a lookup key is out of range on some row")
                counts, seen = {}, set()
                for v in xs:
                    counts[v] = counts.get(v, 0) + 1
                col = m[:, self.input_cols + k]
                for i, v in enumerate(ts):
                    col[i] = 0 if v in seen else counts.get(v, 0)
                    seen.add(v)
                continue
            if kind == MAIN_FETCH:
                key_bits = pad & 255
                xs, ts, vs = [int(v) for v in need(num_op)], [int(v) for v in need(den_op)], need((pad >> 8) & 65535)
                if any(v >> key_bits for v in xs) or any(v >> key_bits for v in ts):
                    raise ValueError("main program: a lookup key is out of range on some row")
                first = {}
                for j, v in enumerate(ts):
                    first.setdefault(v, j)
                if any(v not in first for v in xs):
                    raise ValueError("main program: a fetched key is in no table row")
                m[:, self.input_cols + k] = [vs[first[v]] for v in xs]
                continue
            if kind == MAIN_LIMB:
                lo, mask = pad & 255, (1 << ((pad >> 8) & 255)) - 1
                m[:, self.input_cols + k] = [(int(x) >> lo) & mask for x in need(num_op)]
                continue
            if kind == MAIN_WORD:
                fn, bits = pad & 255, (pad >> 8) & 255
                xs, ys = [int(v) for v in need(num_op)], [int(v) for v in need(den_op)]
                if any(v >> bits for v in xs) or any(v >> bits for v in ys):
                    raise ValueError("main program: a word operand is out of range on some row (both operands of a WORD column must be below 2^bits "
                                     "as canonical integers)")
                m[:, self.input_cols + k] = [x & y if fn == WORD_AND else x | y if fn == WORD_OR else x ^ y for x, y in zip(xs, ys)]
                continue
            t = need(num_op)
            if den_op != AUX_NO_DEN:
                t = (t * np.array(_batch_inverse([int(x) for x in need(den_op)]), dtype=object)) % P
            col = m[:, self.input_cols + k]
            if kind == MAIN_VALUE:
                col[:] = t
            elif kind == MAIN_INV_OR_ZERO:
                where = [i for i in range(n) if int(t[i]) != 0]
                col[:] = 0
                for i, inv in zip(where, _batch_inverse([int(t[i]) for i in where])):
                    col[i] = inv
            elif kind == MAIN_BIT:
                col[:] = [(int(x) >> pad) & 1 for x in t]
            elif kind == MAIN_SUM:
                col[0] = 0
                col[1:] = np.cumsum(t[:-1]) % P
            else:
                z = 1
                for i in range(n):
                    col[i] = z
                    z = z * int(t[i]) % P
        return m


class ChainGroup:
    """A chain group of a MainProgram between chain() and step(): cols = its main columns, state(j) = column j on the current row."""

    def __init__(self, program, cols, period, link=1, seeding=False):
        self.program, self.cols, self.period = program, cols, period
        self.link = link            # blocks in a run (1: every block stands alone)
        self.seeding = seeding      # opened without seeds: g.seed([...]) gives them, and until then g.carry(j) may be read

    def state(self, j):
        if self.seeding:
            raise ValueError("main program: this chain group has no seeds yet: g.seed([...]) comes before the step reads the state")
        return self.program.load(0, self.cols[j])

    def carry(self, j):
        """Column j on the last row of the block before, zero on a run's first block: legal only while the seeds are being declared."""
        if self.program._open is not self or not self.seeding:
            raise ValueError("main program: g.carry(j) is read only while the seeds of an open group are declared (chain(period, None, width=w, link=L))")
        return self.program.load(0, self.cols[j])

    def seed(self, seeds):
        """seeds[j]: the value of column j on a block's first row, from that row's inputs and - in a linked group - the carry."""
        m = self.program
        if m._open is not self or not self.seeding:
            raise ValueError("main program: this chain group has its seeds already")
        if len(seeds) != len(self.cols):
            raise ValueError(f"main program: {len(seeds)} seeds for a chain group of {len(self.cols)} columns")
        seeds = [m._lift(x) for x in seeds]
        if any(x.b is not m for x in seeds):
            raise ValueError("main program: the seeds must be values of this program")
        for col, x in zip(self.cols, seeds):
            kind, _, _, pad = m.cols[col - m.input_cols]
            m.cols[col - m.input_cols] = (kind, x.i, x.i, pad)
        self.seeding = False

    def step(self, nexts):
        """nexts[j]: the value of column j on the next row, from the current one; the group is complete with it."""
        m = self.program
        if m._open is not self:
            raise ValueError("main program: this chain group is closed already")
        if self.seeding:
            raise ValueError("main program: this chain group has no seeds yet: g.seed([...]) comes before g.step([...])")
        if len(nexts) != len(self.cols):
            raise ValueError(f"main program: {len(nexts)} next values for a chain group of {len(self.cols)} columns")
        nexts = [m._lift(x) for x in nexts]
        if any(x.b is not m for x in nexts):
            raise ValueError("main program: the next values must be values of this program")
        for col, x in zip(self.cols, nexts):
            kind, _, seed, pad = m.cols[col - m.input_cols]
            m.cols[col - m.input_cols] = (kind, x.i, seed, pad)
        m._open = None


class PublicProgram(_ChallengeProgram):
    """Values computed from constants and the RAP challenges alone (sp_air_boundary_desc): const(v), rap(i) and + - * through Value.
    AirBuilder.boundary_from names two of them as the N and D of a boundary value."""
    _what = "public values"

    def __init__(self, n_rap):
        super().__init__()
        self.n_rap = n_rap

    def evaluate(self, rap):
        """Every op's value in Python integers."""
        values = list(self.consts) + [int(r) % P for r in rap]
        vals = [None] * len(self.ops)
        _interpret(self.resolved_ops(), range(len(vals)), vals, lambda t, op: f"public values: op {op}", values.__getitem__)
        return vals


def trace_to_ints(trace):
    """(n, cols, 32) canonical big-endian bytes -> (n, cols) numpy object array of Python ints."""
    import numpy as np
    a = np.ascontiguousarray(trace, dtype=np.uint8)
    limbs = a.reshape(a.shape[0], a.shape[1], 4, 8).view(">u8")[..., 0].astype(object)
    return ((limbs[..., 0] << 192) | (limbs[..., 1] << 128) | (limbs[..., 2] << 64) | limbs[..., 3])


def ints_to_bytes(values):
    """(n, cols) Python ints (reduced mod P) -> (n, cols, 32) canonical big-endian bytes."""
    import numpy as np
    v = np.asarray(values, dtype=object) % P
    mask = (1 << 64) - 1
    limbs = np.stack([((v >> s) & mask).astype(np.uint64) for s in (192, 128, 64, 0)], axis=-1)
    return np.ascontiguousarray(limbs.astype(">u8")).view(np.uint8).reshape(v.shape[0], v.shape[1], 32)


class AirBuilder(_ChallengeProgram):
    def __init__(self, main_cols, offsets, degree_bound_factor, aux_cols=0, n_rap=0, aux_kind=AUX_NONE, num_transition_exemptions=1,
                 aux_builder=None, periodic=None, main_inputs=None):
        """aux_builder(rap: list[int]) -> (n, aux_cols) nested list of ints: the AIR's build_auxiliary_trace (aux_kind AUX_CALLBACK).
        periodic: the periodic columns, one list of values each (a power-of-two number of them; the trace must be at least as long).
        main_inputs: the number of main columns the caller supplies; the others are declared through b.main (MainProgram) and derived
        on the device (sp_air_prove_main).  None: the caller supplies the whole main segment."""
        assert 1 <= len(offsets) <= MAX_OFFSETS
        super().__init__()
        self.periodic_cols = [[int(v) % P for v in values] for values in (periodic or [])]
        for k, values in enumerate(self.periodic_cols):
            if len(values) == 0 or len(values) & (len(values) - 1):
                raise ValueError(f"periodic column {k}: its period {len(values)} is not a power of two")
        self.aux_builder = aux_builder
        self.main_cols, self.aux_cols, self.offsets = main_cols, aux_cols, list(offsets)
        self.degree_bound_factor, self.n_rap, self.aux_kind = degree_bound_factor, n_rap, aux_kind
        self.num_transition_exemptions = num_transition_exemptions
        self.degrees, self.exemptions, self.bcs = [], [], []
        self.strides = []   # per constraint (period, offset): enforced on the rows = offset (mod period)
        # aux_kind AUX_PROGRAM: the auxiliary columns as a program over the main-trace row (sp_air_prove_aux)
        self.aux = AuxProgram(main_cols, n_rap, self.periodic_cols) if aux_kind == AUX_PROGRAM else None
        # boundary values computed from the RAP challenges (sp_air_boundary_desc): the program, and per value (index into bcs, N, D)
        self.public = PublicProgram(n_rap)
        self.bvalues = []
        # main_inputs: the derived main columns as a program over the main columns before them (sp_air_prove_main)
        self.main = MainProgram(main_inputs, main_cols, self.periodic_cols) if main_inputs is not None else None

    def load(self, row, col):
        """Cell (frame row `row` = index into the transition offsets, column `col` of main||aux)."""
        assert row < len(self.offsets) and col < self.main_cols + self.aux_cols
        return self._emit(OP_LOAD, row, col)

    def periodic(self, row, k):
        """Periodic column k at frame row `row` (index into the transition offsets): op 6."""
        if not 0 <= row < len(self.offsets):
            raise ValueError(f"periodic: frame row {row} of {len(self.offsets)}")
        if not 0 <= k < len(self.periodic_cols):
            raise ValueError(f"periodic: column {k} is not one of the AIR's {len(self.periodic_cols)} periodic columns")
        return self._emit(OP_PERIODIC, row, k)

    def rap(self, i):
        assert i < self.n_rap
        return self._emit(OP_CONST, _RAP_TAG | i, 0)

    def constraint(self, value, degree, exemptions, period=1, offset=0):
        """period, offset: enforce the constraint on the rows = offset (mod period) only (a power of two; 1, 0: every row).  With a
        period > 1 `exemptions` counts the last rows of that progression, and must leave one: exemptions < n / period."""
        assert len(self.degrees) < MAX_TRANSITIONS
        if period < 1 or period & (period - 1):
            raise ValueError(f"constraint {len(self.degrees)}: its period {period} is not a power of two")
        if not 0 <= offset < period:
            raise ValueError(f"constraint {len(self.degrees)}: offset {offset} outside 0 .. period - 1 = {period - 1}")
        self._emit(OP_OUT, len(self.degrees), value.i)
        self.degrees.append(degree)
        self.exemptions.append(exemptions)
        self.strides.append((period, offset))

    def boundary(self, col, step, value):
        self.bcs.append((col, step, value % P))

    def boundary_from(self, col, step, num, den=None):
        """A boundary constraint whose value is N / D of b.public (D = 1 when None): known once the RAP challenges are - the reference's
        boundary_constraints(rap_challenges).  The descriptor holds 0 in its place; sp_air_prove_pub and its siblings put the value in."""
        num, den = self.public._lift(num), None if den is None else self.public._lift(den)
        if num.b is not self.public or (den is not None and den.b is not self.public):
            raise ValueError("boundary_from: N and D must be values of b.public")
        self.bvalues.append((len(self.bcs), num.i, AUX_NO_DEN if den is None else den.i))
        self.bcs.append((col, step, 0))

    def resolve_boundary(self, rap):
        """The values of the boundary_from constraints under these challenges, in the order they were declared (Python integers: the
        model of sp_air_boundary_resolve).  ValueError when a D is zero (SP_E_ZERO_INVERSE there)."""
        rap = [int(r) % P for r in rap]
        if len(rap) != self.n_rap:
            raise ValueError(f"resolve_boundary: {len(rap)} RAP challenges for an AIR with n_rap = {self.n_rap}")
        vals = self.public.evaluate(rap)
        out = []
        for _, num_op, den_op in self.bvalues:
            if den_op == AUX_NO_DEN:
                out.append(vals[num_op])
                continue
            if vals[den_op] == 0:
                raise ValueError("resolve_boundary: a denominator is zero")
            out.append(vals[num_op] * pow(vals[den_op], P - 2, P) % P)
        return out

    def resolved_bcs(self, rap):
        """bcs with the boundary_from values put in."""
        bcs = list(self.bcs)
        for (j, _, _), value in zip(self.bvalues, self.resolve_boundary(rap) if self.bvalues else []):
            bcs[j] = (bcs[j][0], bcs[j][1], value)
        return bcs

    def enforced_exemptions(self):
        """Per constraint, the number of last rows it is not enforced on - what the composition uses: its own exemption count, or,
        with num_transition_exemptions == 1, the first non-zero count of the AIR for every constraint that has one."""
        strided = [period > 1 for period, _ in self._strides()]   # (a strided constraint always uses its own count)
        nonzero = [e for e, s in zip(self.exemptions, strided) if e > 0 and not s]
        if self.num_transition_exemptions == 1 and nonzero:
            return [e if s else (nonzero[0] if e > 0 else 0) for e, s in zip(self.exemptions, strided)]
        return list(self.exemptions)

    def _strides(self):
        """One (period, offset) per constraint, also for a builder whose lists were filled by hand."""
        return list(self.strides) + [(1, 0)] * (len(self.degrees) - len(self.strides))

    def enforced_rows(self, k, n):
        """The rows constraint k is enforced on in a trace of n rows: its progression without its last enforced_exemptions()[k] rows."""
        period, offset = self._strides()[k]
        rows = list(range(offset, n, period))
        return rows[:max(0, len(rows) - self.enforced_exemptions()[k])]

    def check_trace(self, rows, rap=()):
        """Which constraints the trace breaks, and where, in Python integers: the model of sp_air_check_trace (the reference's
        validate_trace, src/starks/debug.rs:13-104).  rows: (n, main_cols + aux_cols) ints, main||aux; with an aux program also
        (n, main_cols), to which self.aux.evaluate(rows, rap) is appended; with a main program also (n, main_inputs), the input columns
        alone, which self.main.evaluate completes first.  rap: the RAP challenges.  Constraint k is enforced on rows
        0 .. n - 1 - enforced_exemptions()[k] - with a period > 1 on enforced_rows(k, n), its progression without that many of its last
        rows; frame rows wrap modulo n.  Boundary values declared with boundary_from are resolved under `rap` first.  Returns
        [Violation, ...]: the transition constraints by index, then the boundary constraints by index; [] for a trace that satisfies the AIR."""
        import numpy as np
        m = np.empty((len(rows), len(rows[0])), dtype=object)
        m[:, :] = rows if not isinstance(rows, np.ndarray) else rows.astype(object)
        m %= P
        n = m.shape[0]
        rap = [int(r) % P for r in rap]
        if len(rap) != self.n_rap:
            raise ValueError(f"check_trace: {len(rap)} RAP challenges for an AIR with n_rap = {self.n_rap}")
        if self.main is not None and m.shape[1] == self.main.input_cols:
            m = self.main.evaluate(m)
        if self.aux is not None and m.shape[1] == self.main_cols and self.aux_cols:
            m = np.concatenate([m, self.aux.evaluate(m, rap)], axis=1)
        if m.shape[1] != self.main_cols + self.aux_cols:
            raise ValueError(f"check_trace: {m.shape[1]} columns, the AIR has {self.main_cols} + {self.aux_cols}")
        consts = list(self.consts) + rap
        index = np.arange(n)
        vals, outs = [None] * len(self.ops), {}

        def periodic(a, b):
            values = self.periodic_cols[b]
            return np.array(values, dtype=object)[(index + self.offsets[a]) % len(values)]

        _interpret(self.resolved_ops(), range(len(vals)), vals, lambda t, op: f"check_trace: op {op}", lambda a: np.full(n, consts[a], dtype=object),
                   load=lambda a, b: np.roll(m[:, b], -self.offsets[a]), periodic=periodic, out=outs.__setitem__)
        found = []
        for k, ex in enumerate(self.enforced_exemptions()):
            if k not in outs:
                continue
            bad = [i for i in self.enforced_rows(k, n) if outs[k][i] != 0]
            if bad:
                found.append(Violation(TRANSITION, k, len(bad), bad[0], bad[-1], int(outs[k][bad[0]])))
        for j, (col, step, value) in enumerate(self.resolved_bcs(rap)):
            if int(m[step, col]) != value:
                found.append(Violation(BOUNDARY, j, 1, step, step, int(m[step, col])))
        return found

    def check_limits(self):
        """Raises ValueError naming the first bound of sp_air_limits (api.air_limits) this AIR exceeds."""
        from .api import air_limits
        lim = air_limits()
        have = {"columns": self.main_cols + self.aux_cols, "transitions": len(self.degrees), "frame_rows": len(self.offsets),
                "boundary_constraints": len(self.bcs), "constants": len(self.consts), "ops": len(self.ops)}
        for name, value in have.items():
            if value > lim[name]:
                raise ValueError(f"AIR exceeds the {name} limit of sp_air_prove: {value} > {lim[name]}")
        if self.periodic_cols:
            from .api import air_periodic_limits
            most = air_periodic_limits()["periodic_columns"]
            if len(self.periodic_cols) > most:
                raise ValueError(f"AIR exceeds the periodic_columns limit of sp_air_prove_periodic: {len(self.periodic_cols)} > {most}")
        classes = sorted({s for s in self._strides() if s[0] > 1})
        for k, (period, _) in enumerate(self._strides()):
            if period > 1 and self.degrees[k] > self.degree_bound_factor:
                raise ValueError(f"constraint {k}: degree {self.degrees[k]} on a stride needs degree_bound_factor >= {self.degrees[k]} (the quotient by "
                                 f"the progression's zerofier has degree d n - n / period; only a constraint on every row may have d = f + 1)")
        if classes:
            from .api import air_stride_limits
            slim = air_stride_limits()
            kinds = {(s, e) for s, e in zip(self._strides(), self.exemptions) if s[0] > 1 and e > 0}
            if len(classes) > slim["stride_classes"]:
                raise ValueError(f"AIR exceeds the stride_classes limit of sp_air_prove_ext: {len(classes)} > {slim['stride_classes']}")
            if len(kinds) > slim["stride_exemption_products"]:
                raise ValueError(f"AIR exceeds the stride_exemption_products limit of sp_air_prove_ext: {len(kinds)} > {slim['stride_exemption_products']}")
        if self.aux is not None:
            if len(self.aux.cols) != self.aux_cols:
                raise ValueError(f"aux program declares {len(self.aux.cols)} auxiliary columns, the AIR has aux_cols = {self.aux_cols}")
            for name, value in (("constants", len(self.aux.consts)), ("ops", len(self.aux.ops))):
                if value > lim[name]:
                    raise ValueError(f"aux program exceeds the {name} limit of sp_air_prove_aux: {value} > {lim[name]}")
            if len(self.aux.consts) + self.n_rap > 65535:
                raise ValueError("aux program: constants and RAP challenges exceed the 16-bit operand range")
            groups = self.aux.sort_groups()
            if len(groups) > AUX_MAX_SORT_GROUPS:
                raise ValueError(f"aux program exceeds the limit of {AUX_MAX_SORT_GROUPS} sort groups: {len(groups)}")
            for members in groups.values():
                bits = {self.aux.key_bits.get(k, 64) for k in members}
                if len(bits) > 1 or not 1 <= min(bits) <= 64:
                    raise ValueError(f"aux program: the sorted columns {members} share a key and must agree on key_bits in 1 .. 64, not {sorted(bits)}")
        if self.main is not None:
            for name, value in (("constants", len(self.main.consts)), ("ops", len(self.main.ops))):
                if value > lim[name]:
                    raise ValueError(f"main program exceeds the {name} limit of sp_air_prove_main: {value} > {lim[name]}")
            self.main.check()   # (a chain group's block length is held against n by evaluate and by the decoder)
            if self.aux_kind not in (AUX_NONE, AUX_PROGRAM):
                raise ValueError("main program: aux_kind must be AUX_NONE or AUX_PROGRAM (the other kinds build the auxiliary segment from a host "
                                 "table of the main segment)")
        if self.bvalues:
            for name, value in (("constants", len(self.public.consts)), ("ops", len(self.public.ops))):
                if value > lim[name]:
                    raise ValueError(f"boundary values exceed the {name} limit of sp_air_prove_pub: {value} > {lim[name]}")
            if len(self.public.consts) + self.n_rap > 65535:
                raise ValueError("boundary values: constants and RAP challenges exceed the 16-bit operand range")

    def build(self, aux_as_callback=False, main_trace=None):
        """Returns (AirDescC, keepalive).  Raises ValueError if the AIR exceeds a bound of sp_air_limits.

        With a constraint of period > 1 the returned desc carries the AirStrideDescC of all constraints (desc.stride_desc):
        api.Context.air_prove, air_check_trace and api.air_verify then go through the _ext entry points (sp_air_prove_ext ...) with
        whatever else the desc carries.  A builder that never passes `period` produces the descriptor it always produced.
        With periodic columns the returned desc carries their AirPeriodicDescC (desc.periodic_desc): api.Context.air_prove proves it with
        sp_air_prove_periodic, api.air_verify checks it with sp_air_verify_periodic.
        With an aux program (aux_kind AUX_PROGRAM) the returned desc carries its AirAuxDescC (desc.aux_desc), and
        api.Context.air_prove proves it with sp_air_prove_aux.  aux_as_callback=True returns the same AIR as aux_kind AUX_CALLBACK
        instead, its callback evaluating the aux program in Python over `main_trace` ((n, main_cols, 32) canonical big-endian
        bytes, or n rows of ints): what the CPU oracle and sp_air_prove accept.
        With boundary_from constraints the returned desc carries their AirBoundaryDescC (desc.boundary_desc); with that, or an aux program
        that reads a table, api.Context.air_prove, air_check_trace and api.air_verify go through sp_air_prove_pub and its siblings.
        With a main program (main_inputs) the returned desc carries its AirMainDescC (desc.main_desc): api.Context.air_prove and
        air_check_trace then take the input columns only and go through sp_air_prove_main / sp_air_check_trace_main."""
        _check_layout()
        self.check_limits()
        if self.aux is not None and aux_as_callback:
            if main_trace is None:
                raise ValueError("build(aux_as_callback=True) needs the main trace the callback evaluates the aux program over")
            return self._build_aux_callback(main_trace)
        d = AirDescC()
        d.main_cols, d.aux_cols = self.main_cols, self.aux_cols
        d.n_offsets = len(self.offsets)
        for i, o in enumerate(self.offsets):
            d.offsets[i] = o
        d.n_transitions = len(self.degrees)
        for i, (g, e) in enumerate(zip(self.degrees, self.exemptions)):
            d.degrees[i], d.exemptions[i] = g, e
        d.num_transition_exemptions = self.num_transition_exemptions
        d.degree_bound_factor = self.degree_bound_factor
        ops = (AirOpC * len(self.ops))()
        for i, (op, a, b) in enumerate(self.resolved_ops()):
            ops[i].op, ops[i].a, ops[i].b = op, a, b
        consts = ctypes.create_string_buffer(b"".join(c.to_bytes(32, "big") for c in self.consts), max(1, 32 * len(self.consts)))
        bcs = (AirBoundaryC * max(1, len(self.bcs)))()
        for i, (col, step, value) in enumerate(self.bcs):
            bcs[i].col, bcs[i].step = col, step
            ctypes.memmove(bcs[i].value, value.to_bytes(32, "big"), 32)
        d.n_ops, d.ops = len(self.ops), ctypes.cast(ops, ctypes.POINTER(AirOpC))
        d.n_consts, d.consts = len(self.consts), ctypes.cast(consts, ctypes.c_void_p)
        d.n_rap, d.aux_kind = self.n_rap, self.aux_kind
        d.n_boundary, d.boundary = len(self.bcs), ctypes.cast(bcs, ctypes.POINTER(AirBoundaryC))
        cb = None
        if self.aux_kind == AUX_CALLBACK:
            builder, aux_cols = self.aux_builder, self.aux_cols

            def _aux(user, rap_ptr, n_rap, out_ptr):   # canonical big-endian contexts (the default encoding)
                try:
                    raw = ctypes.string_at(rap_ptr, 32 * n_rap)
                    rows = builder([int.from_bytes(raw[32 * i:32 * i + 32], "big") for i in range(n_rap)])
                    flat = b"".join((int(v) % P).to_bytes(32, "big") for row in rows for v in row)
                    assert len(flat) == 32 * aux_cols * len(rows)
                    ctypes.memmove(out_ptr, flat, len(flat))
                    return 0
                except Exception:  # never let an exception cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return -1
            cb = AUX_TRACE_FN(_aux)
            d.aux_fn = cb
        keep = (ops, consts, bcs, cb)
        if self.periodic_cols:
            per_desc, per_keep = periodic_desc(self.periodic_cols)
            d.periodic_desc = per_desc
            keep = keep + (per_desc, per_keep)
        if any(period > 1 for period, _ in self._strides()):
            s_desc, s_keep = stride_desc(self._strides())
            d.stride_desc = s_desc
            keep = keep + (s_desc, s_keep)
        if self.aux is not None:
            aux_desc, aux_keep = self._aux_desc()
            d.aux_desc = aux_desc
            d.aux_reads_table = self.aux.reads_table()
            keep = keep + (aux_desc, aux_keep)
        if self.bvalues:
            b_desc, b_keep = self.build_boundary_desc()
            d.boundary_desc = b_desc
            keep = keep + (b_desc, b_keep)
        if self.main is not None:
            m_desc, m_keep = main_desc(self.main.input_cols, self.main.ops, self.main.consts, self.main.cols)
            d.main_desc = m_desc
            # (LINK and FETCH only where the program declared them: below its level check() has read those pad bits as a j)
            d.main_features = _demanded([(c[0], c[3]) for c in self.main.cols], [op for op, _, _ in self.main.ops]) - {
                level for level in (MainLevel.LINK, MainLevel.FETCH) if self.main.level < level}
            keep = keep + (m_desc, m_keep)
        return d, keep

    def build_boundary_desc(self):
        """(AirBoundaryDescC, keepalive) of the boundary_from constraints: what build() attaches as desc.boundary_desc."""
        return boundary_desc(self.public.resolved_ops(), self.public.consts, self.bvalues)

    def _aux_desc(self):
        _check_aux_layout()
        p = self.aux
        ops = (AirOpC * max(1, len(p.ops)))()
        for i, (op, a, b) in enumerate(p.resolved_ops()):
            ops[i].op, ops[i].a, ops[i].b = op, a, b
        consts = ctypes.create_string_buffer(b"".join(c.to_bytes(32, "big") for c in p.consts), max(1, 32 * len(p.consts)))
        cols = (AirAuxColumnC * max(1, len(p.cols)))()
        for k, (kind, num_op, den_op) in enumerate(p.cols):
            cols[k].kind, cols[k].num_op, cols[k].den_op = kind, num_op, den_op
            cols[k].pad = p.key_bits.get(k, 64) if kind == AUX_SORTED else 0   # (key_bits; the library reads 0 as 64)
        x = AirAuxDescC()
        x.n_ops, x.ops = len(p.ops), ctypes.cast(ops, ctypes.POINTER(AirOpC))
        x.n_consts, x.consts = len(p.consts), ctypes.cast(consts, ctypes.c_void_p)
        x.n_cols, x.cols = len(p.cols), ctypes.cast(cols, ctypes.POINTER(AirAuxColumnC))
        return x, (ops, consts, cols)

    def _build_aux_callback(self, main_trace):
        import numpy as np
        rows = main_trace
        if isinstance(rows, np.ndarray) and rows.dtype == np.uint8:
            rows = trace_to_ints(rows)
        program, aux_kind, main = self.aux, self.aux_kind, self.main
        self.aux_kind, self.aux, self.main = AUX_CALLBACK, None, None   # (the callback's AIR takes the whole main segment: no main program)
        try:
            d, keep = self.build()
        finally:
            self.aux_kind, self.aux, self.main = aux_kind, program, main
        aux_cols, periodic = self.aux_cols, self.periodic_cols

        def _aux(user, rap_ptr, n_rap, out_ptr):   # canonical big-endian contexts (the default encoding)
            try:
                raw = ctypes.string_at(rap_ptr, 32 * n_rap)
                flat = ints_to_bytes(program.evaluate(rows, [int.from_bytes(raw[32 * i:32 * i + 32], "big") for i in range(n_rap)], periodic=periodic))
                assert flat.shape[1] == aux_cols
                ctypes.memmove(out_ptr, flat.ctypes.data, flat.nbytes)
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return -1
        cb = AUX_TRACE_FN(_aux)
        d.aux_fn = cb
        return d, keep + (cb,)


# ---- the reference's example AIRs in program form (src/starks/example/*.rs) ------------------------------------------
def simple_fibonacci(a0=1, a1=1):
    b = AirBuilder(1, [0, 1, 2], 1)
    b.constraint(b.load(2, 0) - b.load(1, 0) - b.load(0, 0), degree=1, exemptions=2)
    b.boundary(0, 0, a0); b.boundary(0, 1, a1)
    return b


def fibonacci_2_columns(a0=1, a1=1):
    b = AirBuilder(2, [0, 1], 1)
    b.constraint(b.load(1, 0) - b.load(0, 0) - b.load(0, 1), 1, 1)
    b.constraint(b.load(1, 1) - b.load(0, 1) - b.load(1, 0), 1, 1)
    b.boundary(0, 0, a0); b.boundary(1, 0, a1)
    return b


def quadratic(a0=3):
    b = AirBuilder(1, [0, 1], 2)
    x = b.load(0, 0)
    b.constraint(b.load(1, 0) - x * x, 2, 1)
    b.boundary(0, 0, a0)
    return b


def dummy():
    b = AirBuilder(2, [0, 1, 2], 1)
    f = b.load(0, 0)
    b.constraint(f * (f - 1), 2, 0)
    b.constraint(b.load(2, 1) - b.load(1, 1) - b.load(0, 1), 1, 2)
    b.boundary(1, 0, 1); b.boundary(1, 1, 1)
    return b


def fibonacci_rap(trace_length, steps):
    b = AirBuilder(2, [0, 1, 2], 1, aux_cols=1, n_rap=1, aux_kind=AUX_FIBONACCI_RAP, num_transition_exemptions=2)
    b.constraint(b.load(2, 0) - b.load(1, 0) - b.load(0, 0), 1, 3 + trace_length - steps - 1)
    gamma = b.rap(0)
    b.constraint(b.load(1, 2) * (b.load(0, 1) + gamma) - b.load(0, 2) * (b.load(0, 0) + gamma), 2, 1)
    b.boundary(0, 0, 1); b.boundary(0, 1, 1); b.boundary(2, 0, 1)
    return b


def fibonacci_rap_program(trace_length, steps):
    """fibonacci_rap with its permutation column as an aux program (sp_air_prove_aux): z_0 = 1, z_i = z_(i-1) (a + gamma) / (b + gamma)
    of row i - 1 - the column aux_kind AUX_FIBONACCI_RAP builds on the host."""
    b = AirBuilder(2, [0, 1, 2], 1, aux_cols=1, n_rap=1, aux_kind=AUX_PROGRAM, num_transition_exemptions=2)
    b.constraint(b.load(2, 0) - b.load(1, 0) - b.load(0, 0), 1, 3 + trace_length - steps - 1)
    gamma = b.rap(0)
    b.constraint(b.load(1, 2) * (b.load(0, 1) + gamma) - b.load(0, 2) * (b.load(0, 0) + gamma), 2, 1)
    b.boundary(0, 0, 1); b.boundary(0, 1, 1); b.boundary(2, 0, 1)
    g = b.aux.rap(0)
    b.aux.product(b.aux.load(0, 0) + g, b.aux.load(0, 1) + g)
    return b


# ---- periodic columns: a worked example ---------------------------------------------------------------------------------
def mimc_chain(n, period, x0, keys):
    """x_(i+1) = (x_i + K_(i mod period))^3 on one column: a MiMC-style chain whose round constants `keys` (period of them, a power
    of two <= n) are a periodic column.  The constraint x' - (x + K)^3 has degree 3 (K counts as a trace cell), so the composition
    degree bound is 2n; the last row is exempt; x_0 = x0."""
    if len(keys) != period or period > n:
        raise ValueError(f"mimc_chain: {len(keys)} keys for period {period} on {n} rows (the period is the number of keys, at most n)")
    b = AirBuilder(1, [0, 1], 2, periodic=[keys])
    t = b.load(0, 0) + b.periodic(0, 0)
    b.constraint(b.load(1, 0) - t * t * t, degree=3, exemptions=1)
    b.boundary(0, 0, x0)
    return b


def mimc_chain_trace(n, x0, keys):
    """The chain's trace as (n, 1) Python ints (ints_to_bytes gives the bytes sp_air_prove_periodic takes)."""
    rows, x = [], x0 % P
    for i in range(n):
        rows.append([x])
        x = pow((x + keys[i % len(keys)]) % P, 3, P)
    return rows


# ---- strided constraints: a worked example ------------------------------------------------------------------------------
STRIDED_CHAIN_PERIOD = 4


def strided_mimc_chain(n, x0, keys, selector=False):
    """mimc_chain's shape with a SQUARING round on the rows = 0 (mod 4) only: x_(i+1) = (x_i + K_(i mod period))^2 for i = 0, 4, 8,
    ..., n - 8, the three rows between free (a real layout would put other cells there) and the last row of the progression, n - 4,
    exempt as the last row of mimc_chain is.  One statement, two ways to say it, both under degree_bound_factor 2:

    selector=False  the constraint x' - (x + K)^2 with period=4, offset=0, exemptions=1: declared degree 2.  Its quotient by
                    x^(n/4) - 1 has degree 2 (n - 1) + 1 - n/4, the term of the composition 2n - 2 + 1 + 1 = 2n coefficients.
    selector=True   the same constraint times the periodic column [1, 0, 0, 0] on every row but the last four: declared degree 3 =
                    degree_bound_factor + 1, 2n - 3 + 4 + 1 = 2n + 2 coefficients by the declared degrees: above 2n, so the 2n-point
                    path is refused before the trace is looked at and the whole LDE domain is evaluated (blowup / 2 times the
                    composition points), and every lane reads and multiplies the selector.

    The cube of mimc_chain cannot be put on a stride under degree_bound_factor 2: a strided constraint needs degree <= the factor
    (AirBuilder.check_limits), and a factor of 3 is beyond the two halves H1, H2 of the proof format.

    keys: a power-of-two number of round constants, at most n; n >= 8."""
    if n < 2 * STRIDED_CHAIN_PERIOD or len(keys) > n:
        raise ValueError(f"strided_mimc_chain: {n} rows, {len(keys)} keys (at least 8 rows, at most n keys)")
    if selector:
        b = AirBuilder(1, [0, 1], 2, periodic=[keys, [1, 0, 0, 0]])
        t = b.load(0, 0) + b.periodic(0, 0)
        b.constraint(b.periodic(0, 1) * (b.load(1, 0) - t * t), degree=3, exemptions=4)
    else:
        b = AirBuilder(1, [0, 1], 2, periodic=[keys])
        t = b.load(0, 0) + b.periodic(0, 0)
        b.constraint(b.load(1, 0) - t * t, degree=2, exemptions=1, period=STRIDED_CHAIN_PERIOD, offset=0)
    b.boundary(0, 0, x0)
    return b


def strided_mimc_chain_trace(n, x0, keys, free):
    """A trace of strided_mimc_chain as (n, 1) Python ints: row i + 1 = (x_i + K_(i mod period))^2 for i = 0 (mod 4), the other rows
    from `free` (a callable giving the next free value)."""
    rows, x = [], x0 % P
    for i in range(n):
        rows.append([x])
        x = pow((x + keys[i % len(keys)]) % P, 2, P) if i % STRIDED_CHAIN_PERIOD == 0 else free() % P
    return rows


# ---- public data inside a RAP argument: two worked examples -------------------------------------------------------------------
def table_lookup(n, table):
    """Every a_i is an entry of the public `table` (a power-of-two number of values, at most n): a LogUp lookup.  Main columns a and m
    (m_i: how often the table entry of row i, T_i = table[i mod len(table)], is looked up - a prover's choice that sums right), T periodic
    column 0, one challenge gamma.  The auxiliary column is the running sum s_0 = 0, s' = s + m / (gamma - T) - 1 / (gamma - a), built on
    the device by an auxiliary program that reads T with table().  The constraint (s' - s)(gamma - T)(gamma - a) - m (gamma - a) +
    (gamma - T) has degree 3 under degree_bound_factor 2 and NO exempted row: on row n - 1 it wraps to s_0 = 0 and closes the sum."""
    if len(table) > n:
        raise ValueError(f"table_lookup: {len(table)} table entries on {n} rows")
    b = AirBuilder(2, [0, 1], 2, aux_cols=1, n_rap=1, aux_kind=AUX_PROGRAM, periodic=[table])
    gamma = b.rap(0)
    ga, gt = gamma - b.load(0, 0), gamma - b.periodic(0, 0)
    b.constraint((b.load(1, 2) - b.load(0, 2)) * gt * ga - b.load(0, 1) * ga + gt, degree=3, exemptions=0)
    b.boundary(2, 0, 0)
    g = b.aux.rap(0)
    xa, xt = g - b.aux.load(0, 0), g - b.aux.table(0, 0)
    b.aux.running_sum(b.aux.load(0, 1) * xa - xt, xt * xa)
    return b


def table_lookup_trace(n, table, looked_up):
    """(n, 2) Python ints [a_i, m_i] for the n values `looked_up` (each an entry of the table): each distinct table value's multiplicity
    sits on the first row that holds it, every other m is 0."""
    first = {}
    for j, v in enumerate(table):
        first.setdefault(int(v) % P, j)
    a = [int(v) % P for v in looked_up]
    if len(a) != n or any(v not in first for v in a):
        raise ValueError("table_lookup_trace: n looked-up values, each an entry of the table")
    m = [0] * n
    for v in a:
        m[first[v]] += 1
    return [[a[i], m[i]] for i in range(n)]


def public_permutation(n, public):
    """Column a is column b with L of its zeros replaced by the public list (L = len(public) < n), in any order: main columns a and b,
    one challenge gamma, the grand product z_0 = 1, z' (gamma - b) = z (gamma - a) with the last row exempt.  a_(n-1) = b_(n-1) = 0 and
    z_0 = 1 are constants; z_(n-1) = prod_j (gamma - v_j) / gamma^L depends on the challenge and goes through boundary_from - the short
    public list never becomes a column of n values."""
    if len(public) >= n:
        raise ValueError(f"public_permutation: {len(public)} public values on {n} rows")
    b = AirBuilder(2, [0, 1], 1, aux_cols=1, n_rap=1, aux_kind=AUX_PROGRAM)
    gamma = b.rap(0)
    b.constraint(b.load(1, 2) * (gamma - b.load(0, 1)) - b.load(0, 2) * (gamma - b.load(0, 0)), degree=2, exemptions=1)
    b.boundary(0, n - 1, 0); b.boundary(1, n - 1, 0); b.boundary(2, 0, 1)
    g = b.aux.rap(0)
    b.aux.product(g - b.aux.load(0, 0), g - b.aux.load(0, 1))
    pg = b.public.rap(0)
    num, den = b.public.const(1), None
    for v in public:
        num = num * (pg - v)
        den = pg if den is None else den * pg
    b.boundary_from(2, n - 1, num, den)
    return b


def public_permutation_trace(n, public, fill, order):
    """(n, 2) Python ints [a_i, b_i]: b holds the non-zero values `fill` (n - 1 - len(public) of them) and len(public) zeros on its rows
    0 .. n - 2 in the order `order` (a permutation of range(n - 1)), a holds `fill` and the public list there in their given order;
    the last row is [0, 0]."""
    L = len(public)
    if len(fill) != n - 1 - L or sorted(order) != list(range(n - 1)):
        raise ValueError("public_permutation_trace: n - 1 - len(public) fill values and a permutation of range(n - 1)")
    a = [int(v) % P for v in list(public) + list(fill)]
    src = [0] * L + [int(v) % P for v in fill]
    return [[a[i], src[order[i]]] for i in range(n - 1)] + [[0, 0]]


# ---- sorted auxiliary columns: two worked examples ------------------------------------------------------------------------------
def sorted_range_check(n, lo, hi, key_bits=16):
    """Every a_i lies in lo .. hi, and every value of that range occurs: range check by sorting.  Main column a; auxiliary columns a'
    (a sorted, trace column 1) and the grand product z (trace column 2), one challenge gamma.  z_0 = 1 and z' (gamma - a') = z (gamma - a) on every
    row - no exemption: the last row wraps to z_0 = 1 and closes the product, so a' is a permutation of a.  Continuity: (a'_(i+1) - a'_i)
    (a'_(i+1) - a'_i - 1) = 0 with the last row exempt; a'_0 = lo and a'_(n-1) = hi.  degree_bound_factor 1."""
    if not 0 <= lo <= hi < 1 << key_bits or hi - lo >= n:
        raise ValueError(f"sorted_range_check: the range {lo} .. {hi} on {n} rows with keys of {key_bits} bits")
    b = AirBuilder(1, [0, 1], 1, aux_cols=2, n_rap=1, aux_kind=AUX_PROGRAM)
    gamma = b.rap(0)
    b.constraint(b.load(1, 2) * (gamma - b.load(0, 1)) - b.load(0, 2) * (gamma - b.load(0, 0)), degree=2, exemptions=0)
    step = b.load(1, 1) - b.load(0, 1)
    b.constraint(step * (step - 1), degree=2, exemptions=1)
    b.boundary(2, 0, 1); b.boundary(1, 0, lo); b.boundary(1, n - 1, hi)
    g = b.aux.rap(0)
    a = b.aux.load(0, 0)
    s, = b.aux.sorted(a, key_bits=key_bits)
    b.aux.product(g - a, g - b.aux.sorted_load(0, s))
    return b


def sorted_range_check_trace(n, lo, hi, extra, order):
    """(n, 1) Python ints: every value of lo .. hi once and the n - (hi - lo + 1) values `extra` (each in the range), row i holding
    entry order[i] of that list (`order` a permutation of range(n))."""
    values = list(range(lo, hi + 1)) + [int(v) for v in extra]
    if len(values) != n or any(not lo <= v <= hi for v in values) or sorted(order) != list(range(n)):
        raise ValueError("sorted_range_check_trace: n - (hi - lo + 1) extra values inside the range and a permutation of range(n)")
    return [[values[order[i]]] for i in range(n)]


def memory_consistency(n, key_bits=64):
    """A read-only memory: every access (addr, val) of the main trace agrees with every other access of its address, and the addresses
    used are contiguous - Cairo's memory argument (src/cairo/air.rs in the reference) in program form.  Main columns addr and val;
    the sorted group (addr'; val') = the accesses by address (trace columns 2 and 3) and the grand product z (trace column 4); challenges alpha and
    gamma.  z_0 = 1 and z' (gamma - (addr' + alpha val')) = z (gamma - (addr + alpha val)) on every row, the last wrapping to z_0;
    (addr'_(i+1) - addr'_i)(addr'_(i+1) - addr'_i - 1) = 0 and (val'_(i+1) - val'_i)(addr'_(i+1) - addr'_i - 1) = 0 with the last row
    exempt.  degree_bound_factor 1; the addresses must be < 2^key_bits."""
    b = AirBuilder(2, [0, 1], 1, aux_cols=3, n_rap=2, aux_kind=AUX_PROGRAM)
    alpha, gamma = b.rap(0), b.rap(1)
    b.constraint(b.load(1, 4) * (gamma - (b.load(0, 2) + alpha * b.load(0, 3))) - b.load(0, 4) * (gamma - (b.load(0, 0) + alpha * b.load(0, 1))),
                 degree=2, exemptions=0)
    step = b.load(1, 2) - b.load(0, 2)
    b.constraint(step * (step - 1), degree=2, exemptions=1)
    b.constraint((b.load(1, 3) - b.load(0, 3)) * (step - 1), degree=2, exemptions=1)
    b.boundary(4, 0, 1)
    al, g = b.aux.rap(0), b.aux.rap(1)
    addr, val = b.aux.load(0, 0), b.aux.load(0, 1)
    sa, sv = b.aux.sorted(addr, carry=[val], key_bits=key_bits)
    b.aux.product(g - (addr + al * val), g - (b.aux.sorted_load(0, sa) + al * b.aux.sorted_load(0, sv)))
    return b


def memory_consistency_trace(n, first, cells, accesses):
    """(n, 2) Python ints [addr_i, val_i]: the memory holds `cells` at the addresses first, first + 1, ...; row i reads cell accesses[i]
    (an index into `cells`; every cell at least once, or the addresses are not contiguous)."""
    if len(accesses) != n or set(accesses) != set(range(len(cells))):
        raise ValueError("memory_consistency_trace: n accesses that reach every cell")
    return [[first + j, int(cells[j]) % P] for j in accesses]


# ---- derived main columns: two worked examples ----------------------------------------------------------------------------------
def bit_range_check(n, bits):
    """Every v_i is below 2^bits: one input column v and `bits` derived columns b_0 .. b_(bits-1), the bits of v (MainProgram.bits), so
    the caller uploads n values where the table has n x (1 + bits).  Two constraints on every row, no exemption: sum_j gamma^j b_j
    (b_j - 1) = 0 - every b_j (b_j - 1) = 0, folded with the powers of one challenge gamma sampled behind the main commitment, since a
    descriptor takes at most 64 transition constraints and there may be up to 251 bits - and sum_j 2^j b_j = v.  degree_bound_factor 1
    (the products have degree 2 = factor + 1, as in `dummy`); no auxiliary column."""
    if not 1 <= bits <= MAIN_MAX_BIT:
        raise ValueError(f"bit_range_check: {bits} bits (1 .. {MAIN_MAX_BIT}: the canonical integers of the field have 252)")
    b = AirBuilder(1 + bits, [0], 1, n_rap=1, main_inputs=1)
    cols = b.main.bits(b.main.load(0, 0), bits)
    gamma = b.rap(0)
    power, boolean, total = None, None, None
    for j, c in enumerate(cols):
        x = b.load(0, c)
        power = b.const(1) if power is None else power * gamma
        term, weighted = power * (x * (x - 1)), x * (1 << j)
        boolean = term if boolean is None else boolean + term
        total = weighted if total is None else total + weighted
    b.constraint(boolean, degree=2, exemptions=0)
    b.constraint(total - b.load(0, 0), degree=1, exemptions=0)
    return b


def bit_range_check_inputs(n, bits, rng):
    """(n, 1) Python ints below 2^bits from rng.randrange: the input column of bit_range_check."""
    return [[rng.randrange(1 << bits)] for _ in range(n)]


def zero_count(n, count):
    """The public `count` is the number of zeros among x_0 .. x_(n-2): one input column x; derived columns inv = INV_OR_ZERO(x) (column
    1), f = VALUE(1 - x inv), the is-zero flag, which reads inv (column 2), and c = SUM(f), the zeros before each row, which reads f
    (column 3).  Constraints x f = 0 and f = 1 - x inv on every row, c' = c + f with the last row exempt; boundaries c_0 = 0 and
    c_(n-1) = count.  degree_bound_factor 1."""
    b = AirBuilder(4, [0, 1], 1, main_inputs=1)
    m = b.main
    inv = m.inv_or_zero(m.load(0, 0))
    f = m.value(1 - m.load(0, 0) * m.load(0, inv))
    c = m.running_sum(m.load(0, f))
    x = b.load(0, 0)
    b.constraint(x * b.load(0, f), degree=2, exemptions=0)
    b.constraint(b.load(0, f) - (1 - x * b.load(0, inv)), degree=2, exemptions=0)
    b.constraint(b.load(1, c) - b.load(0, c) - b.load(0, f), degree=1, exemptions=1)
    b.boundary(c, 0, 0); b.boundary(c, n - 1, count)
    return b


def zero_count_inputs(n, zeros, rng):
    """(n, 1) Python ints: zero on the rows `zeros`, a non-zero value from rng.randrange elsewhere; the statement's count is the number
    of those rows below n - 1."""
    zeros = set(zeros)
    return [[0 if i in zeros else 1 + rng.randrange(P - 1)] for i in range(n)]


# ---- block recurrences: a worked example ----------------------------------------------------------------------------------------
def mimc_blocks(n, s, keys, digest, width=1):
    """n / s independent MiMC permutations of s rounds each, one per block of s rows: the caller uploads the messages m (column 0, of
    which only the rows = 0 (mod s) matter) and the device builds the rest (sp_air_prove_rec).  Column 1 is the state x, a chain group
    with seed m and step (x + K_t)^3; column 2 the row-local q = (x + K)^2, a VALUE that reads x and the periodic column K.  Periodic
    columns K = keys (period s) and sel = [1] (s - 1) + [0].  Constraints under degree_bound_factor 2, no exemption: q - (x + K)^2
    (degree 2) on every row; sel (x' - q (x + K)) (degree 3) on every row - sel switches it off where a block ends, the trace's last
    row among them; x - m (degree 1) on the rows = 0 (mod s).  The boundary constraint x_(s-1) = digest is block 0's public digest
    (mimc_blocks_digest).

    width > 1 widens the group: states x_0 .. x_(w-1) in columns 1 .. w with seeds m + j and steps (x_j + x_((j+1) mod w) + K)^3, their
    squares q_j in columns w + 1 .. 2 w, every constraint once per j; the digest is that of x_0."""
    if s < 2 or s & (s - 1) or s > n or len(keys) != s:
        raise ValueError(f"mimc_blocks: blocks of {s} rows with {len(keys)} keys on {n} rows (a power of two in 2 .. n, one key per row of a block)")
    w = width
    b = AirBuilder(1 + 2 * w, [0, 1], 2, periodic=[keys, [1] * (s - 1) + [0]], main_inputs=1)
    m = b.main
    g = m.chain(s, [m.load(0, 0) + j for j in range(w)] if w > 1 else [m.load(0, 0)])

    def round_input(load, key, j):
        return load(j) + key if w == 1 else load(j) + load((j + 1) % w) + key

    t = [round_input(g.state, m.periodic(0, 0), j) for j in range(w)]
    g.step([t[j] * t[j] * t[j] for j in range(w)])
    x = g.cols
    q = []
    for j in range(w):
        u = round_input(lambda j: m.load(0, x[j]), m.periodic(0, 0), j)
        q.append(m.value(u * u))
    for j in range(w):
        u = round_input(lambda j: b.load(0, x[j]), b.periodic(0, 0), j)
        b.constraint(b.load(0, q[j]) - u * u, degree=2, exemptions=0)
        b.constraint(b.periodic(0, 1) * (b.load(1, x[j]) - b.load(0, q[j]) * u), degree=3, exemptions=0)
        b.constraint(b.load(0, x[j]) - (b.load(0, 0) + j if j else b.load(0, 0)), degree=1, exemptions=0, period=s, offset=0)
    b.boundary(x[0], s - 1, digest)
    return b


def mimc_blocks_digest(messages, s, keys, width=1):
    """x_0 on the last row of the block seeded from messages[0]: the public digest of mimc_blocks (rounds 0 .. s - 2; the last key is
    read by q alone)."""
    x = [(int(messages[0]) + j) % P for j in range(width)]
    for t in range(s - 1):
        x = [pow((x[j] + (x[(j + 1) % width] if width > 1 else 0) + keys[t]) % P, 3, P) for j in range(width)]
    return x[0]


def mimc_blocks_inputs(n, s, rng):
    """(n, 1) Python ints from rng.randrange: a message on every row = 0 (mod s), the caller's filler on the others."""
    return [[rng.randrange(P)] for _ in range(n)]


# ---- linked chain groups: two worked examples --------------------------------------------------------------------------------------
def _run_selector(s, link):
    """Period s * link: 1 on the last row of every block of a run but the run's last - the rows whose next row absorbs."""
    return [1 if t % s == s - 1 and t != s * link - 1 else 0 for t in range(s * link)]


def mimc_sponge(n, s, link, keys, digest):
    """n / (s link) MiMC sponges, each absorbing `link` message blocks: the caller uploads the messages m (column 0, of which only the
    rows = 0 (mod s) matter) and the device builds the rest (sp_air_prove_link).  Column 1 is the state x, a one-column linked group in
    runs of `link` blocks with seed carry + m - the state the block before ended on, zero in front of a run - and step (x + K_t)^3;
    column 2 the row-local q = (x + K)^2 as in mimc_blocks.  Periodic columns K = keys (period s), sel = [1] (s - 1) + [0] and ab
    (period s link), 1 on the block ends that are no run ends.  Constraints under degree_bound_factor 2, no exemption: q - (x + K)^2
    (degree 2) and sel (x' - q (x + K)) (degree 3) on every row, which tie the steps inside a block; ab (x' - x - m') (degree 2) on
    every row, which ties a block's seed to the block before; x - m (degree 1) on the rows = 0 (mod s link), the run starts.  The
    boundary constraint x_(s link - 1) = digest is run 0's public digest (mimc_sponge_digest)."""
    if s < 2 or s & (s - 1) or link < 2 or link & (link - 1) or s * link > n or len(keys) != s:
        raise ValueError(f"mimc_sponge: runs of {link} blocks of {s} rows with {len(keys)} keys on {n} rows (powers of two, link >= 2, s link <= n, one key "
                         "per row of a block)")
    b = AirBuilder(3, [0, 1], 2, periodic=[keys, [1] * (s - 1) + [0], _run_selector(s, link)], main_inputs=1)
    m = b.main
    g = m.chain(s, None, width=1, link=link)
    g.seed([g.carry(0) + m.load(0, 0)])
    t = g.state(0) + m.periodic(0, 0)
    g.step([t * t * t])
    x = g.cols[0]
    u = m.load(0, x) + m.periodic(0, 0)
    q = m.value(u * u)
    u = b.load(0, x) + b.periodic(0, 0)
    b.constraint(b.load(0, q) - u * u, degree=2, exemptions=0)
    b.constraint(b.periodic(0, 1) * (b.load(1, x) - b.load(0, q) * u), degree=3, exemptions=0)
    b.constraint(b.periodic(0, 2) * (b.load(1, x) - b.load(0, x) - b.load(1, 0)), degree=2, exemptions=0)
    b.constraint(b.load(0, x) - b.load(0, 0), degree=1, exemptions=0, period=s * link, offset=0)
    b.boundary(x, s * link - 1, digest)
    return b


def mimc_sponge_digest(messages, s, keys):
    """The state after absorbing `messages`, one per block (rounds 0 .. s - 2 of each block; the last key is read by q alone): the
    public digest of mimc_sponge for the `link` messages of run 0."""
    x = 0
    for msg in messages:
        x = (x + int(msg)) % P
        for t in range(s - 1):
            x = pow((x + keys[t]) % P, 3, P)
    return x


def mimc_sponge_inputs(n, s, link, rng):
    """(n, 1) Python ints from rng.randrange: a message on every row = 0 (mod s), the caller's filler on the others."""
    return [[rng.randrange(P)] for _ in range(n)]


def merkle_paths(n, s, depth, keys, root):
    """n / (s depth) Merkle paths of `depth` levels against one public root, each level a Feistel-MiMC compression of (left, right) in
    a block of s rows: (L, R) -> (R + (L + K_t)^3, L), the digest the L of the block's last row (merkle_paths_digest).  Inputs: the
    value v (column 0: the leaf on a run's first row, 0 on the other block starts), the sibling (column 1) and the direction bit d
    (column 2: 1 where the path's node is the right child); all three matter on the rows = 0 (mod s) only.  Columns 3 and 4 are (L, R),
    a two-column linked group in runs of `depth` blocks whose seeds read cur = carry_0 + v - the digest of the level below, or the leaf
    where the carry is zero - and place it by the bit: L = cur + d (sib - cur), R = sib + d (cur - sib).  Column 5 is q = (L + K)^2.
    Constraints under degree_bound_factor 2 (sel and ab as in mimc_sponge): q - (L + K)^2; sel (L' - R - q (L + K)) and sel (R' - L);
    ab (L' - L - d' (sib' - L)) and ab (R' - sib' - d' (L - sib')), degree 3 - a value other than 0 on a later block start breaks
    them -; L - v - d (sib - v) and R - sib - d (v - sib) on the run starts; d (d - 1) on the rows = 0 (mod s); L - root on every run's
    last row."""
    if s < 2 or s & (s - 1) or depth < 2 or depth & (depth - 1) or s * depth > n or len(keys) != s:
        raise ValueError(f"merkle_paths: paths of {depth} levels in blocks of {s} rows with {len(keys)} keys on {n} rows (powers of two, depth >= 2, "
                         "s depth <= n, one key per row of a block)")
    b = AirBuilder(6, [0, 1], 2, periodic=[keys, [1] * (s - 1) + [0], _run_selector(s, depth)], main_inputs=3)
    m = b.main
    g = m.chain(s, None, width=2, link=depth)
    cur, sib, d = g.carry(0) + m.load(0, 0), m.load(0, 1), m.load(0, 2)
    g.seed([cur + d * (sib - cur), sib + d * (cur - sib)])
    t = g.state(0) + m.periodic(0, 0)
    g.step([g.state(1) + t * t * t, g.state(0)])
    left, right = g.cols
    u = m.load(0, left) + m.periodic(0, 0)
    q = m.value(u * u)
    run = s * depth
    u = b.load(0, left) + b.periodic(0, 0)
    sel, ab = b.periodic(0, 1), b.periodic(0, 2)
    b.constraint(b.load(0, q) - u * u, degree=2, exemptions=0)
    b.constraint(sel * (b.load(1, left) - b.load(0, right) - b.load(0, q) * u), degree=3, exemptions=0)
    b.constraint(sel * (b.load(1, right) - b.load(0, left)), degree=2, exemptions=0)
    cur, sib, d = b.load(0, left), b.load(1, 1), b.load(1, 2)
    b.constraint(ab * (b.load(1, left) - cur - d * (sib - cur)), degree=3, exemptions=0)
    b.constraint(ab * (b.load(1, right) - sib - d * (cur - sib)), degree=3, exemptions=0)
    cur, sib, d = b.load(0, 0), b.load(0, 1), b.load(0, 2)
    b.constraint(b.load(0, left) - cur - d * (sib - cur), degree=2, exemptions=0, period=run, offset=0)
    b.constraint(b.load(0, right) - sib - d * (cur - sib), degree=2, exemptions=0, period=run, offset=0)
    b.constraint(d * (d - 1), degree=2, exemptions=0, period=s, offset=0)
    b.constraint(b.load(0, left) - root, degree=1, exemptions=0, period=run, offset=run - 1)
    return b


def merkle_paths_digest(left, right, s, keys):
    """The compression of merkle_paths: s - 1 Feistel-MiMC rounds on (left, right), the digest the left half."""
    lo, hi = int(left) % P, int(right) % P
    for t in range(s - 1):
        lo, hi = (hi + pow((lo + keys[t]) % P, 3, P)) % P, lo
    return lo


def merkle_paths_inputs(n, s, depth, keys, rng):
    """(rows, root): a tree of 2^depth leaves from rng.randrange under merkle_paths_digest, and for each of the n / (s depth) runs the
    path of a leaf rng picks - (n, 3) Python ints: leaf, sibling and direction bit on the block starts, filler on the other rows (the
    bit column's filler is free as well: d (d - 1) is enforced on the block starts alone)."""
    levels = [[rng.randrange(P) for _ in range(1 << depth)]]
    while len(levels[-1]) > 1:
        below = levels[-1]
        levels.append([merkle_paths_digest(below[2 * i], below[2 * i + 1], s, keys) for i in range(len(below) // 2)])
    rows = [[rng.randrange(P), rng.randrange(P), rng.randrange(P)] for _ in range(n)]
    for first in range(0, n, s * depth):
        index = rng.randrange(1 << depth)
        for level in range(depth):
            rows[first + level * s] = [levels[0][index] if level == 0 else 0, levels[level][index ^ 1], index & 1]
            index >>= 1
    return rows, levels[-1][0]


# ---- lookup multiplicities: two worked examples -----------------------------------------------------------------------------------
def _logup_sum(b, looked_up, aux_looked_up, m_col, s_col):
    """The LogUp running sum of table_lookup for a looked-up value given as an expression: column s_col, s_0 = 0, s' = s + m / (gamma -
    T) - 1 / (gamma - X) with T periodic column 0, its constraint (degree 3, no exempted row) and its boundary."""
    gamma = b.rap(0)
    ga, gt = gamma - looked_up, gamma - b.periodic(0, 0)
    b.constraint((b.load(1, s_col) - b.load(0, s_col)) * gt * ga - b.load(0, m_col) * ga + gt, degree=3, exemptions=0)
    b.boundary(s_col, 0, 0)
    g = b.aux.rap(0)
    xa, xt = g - aux_looked_up, g - b.aux.table(0, 0)
    b.aux.running_sum(b.aux.load(0, m_col) * xa - xt, xt * xa)


def table_lookup_main(n, table, key_bits=64):
    """table_lookup with main_inputs=1 (sp_air_prove_lk): the caller uploads the looked-up column a alone, and the device builds m =
    multiplicity(a, T, key_bits) - every a_i and every table entry below 2^key_bits - and, as before, the running sum.  The same
    statement, the same trace (table_lookup_trace) and the same proof as table_lookup from the whole table."""
    if len(table) > n:
        raise ValueError(f"table_lookup_main: {len(table)} table entries on {n} rows")
    b = AirBuilder(2, [0, 1], 2, aux_cols=1, n_rap=1, aux_kind=AUX_PROGRAM, periodic=[table], main_inputs=1)
    b.main.multiplicity(b.main.load(0, 0), b.main.periodic(0, 0), key_bits)
    _logup_sum(b, b.load(0, 0), b.aux.load(0, 0), 1, 2)
    return b


def table_lookup_main_inputs(n, table, rng):
    """(n, 1) Python ints: n entries of the table, drawn with rng.randrange."""
    return [[int(table[rng.randrange(len(table))]) % P] for _ in range(n)]


def xor_lookup_table(bits):
    """The 2^(2 bits) packed triples a + 2^bits b + 2^(2 bits) (a xor b), in the order of a + 2^bits b."""
    return [a + (b << bits) + ((a ^ b) << (2 * bits)) for b in range(1 << bits) for a in range(1 << bits)]


def xor_lookup(n, bits=4):
    """c_i = a_i xor b_i on every row, for `bits`-bit a and b, by one lookup of the packed triple a + 2^bits b + 2^(2 bits) c into the
    table of all 2^(2 bits) such triples (periodic column 0; at most n of them).  Inputs a, b, c (columns 0 - 2); column 3 is m =
    multiplicity(a + 2^bits b + 2^(2 bits) c, T, 3 bits), built on the device; the auxiliary column 4 is the LogUp running sum of
    table_lookup over the packed value.  A row whose c is not a xor b - or whose a or b has more than `bits` bits, while the packed
    value stays below 2^(3 bits) - packs to no table entry, is counted nowhere, and the sum does not close."""
    table = xor_lookup_table(bits)
    if len(table) > n:
        raise ValueError(f"xor_lookup: {len(table)} table entries on {n} rows")
    b = AirBuilder(4, [0, 1], 2, aux_cols=1, n_rap=1, aux_kind=AUX_PROGRAM, periodic=[table], main_inputs=3)

    def packed(load):
        return load(0, 0) + load(0, 1) * (1 << bits) + load(0, 2) * (1 << (2 * bits))

    b.main.multiplicity(packed(b.main.load), b.main.periodic(0, 0), 3 * bits)
    _logup_sum(b, packed(b.load), packed(b.aux.load), 3, 4)
    return b


def xor_lookup_inputs(n, bits, rng):
    """(n, 3) Python ints [a, b, a xor b] with a, b from rng.randrange(2^bits)."""
    rows = []
    for _ in range(n):
        a, b = rng.randrange(1 << bits), rng.randrange(1 << bits)
        rows.append([a, b, a ^ b])
    return rows


# ---- looked-up values: two worked examples ----------------------------------------------------------------------------------------
def xor_fetch(n, bits=4):
    """xor_lookup with main_inputs=2 (sp_air_prove_fetch): the caller uploads a and b alone, and the device fetches c = a xor b as the
    value of the table row whose key is a + 2^bits b - periodic column 1 holds the keys, periodic column 2 the values, both in the order
    of xor_lookup_table (periodic column 0, which the statement reads as before).  Behind it the statement of xor_lookup unchanged: m =
    multiplicity over the packed triple and the LogUp sum.  The same trace and the same proof as xor_lookup from [a, b, a xor b].  An a
    or b of more than `bits` bits packs to a key of more than 2 bits bits or to no table row, and the call is refused."""
    table = xor_lookup_table(bits)
    if len(table) > n:
        raise ValueError(f"xor_fetch: {len(table)} table entries on {n} rows")
    keys = [a + (b << bits) for b in range(1 << bits) for a in range(1 << bits)]
    values = [a ^ b for b in range(1 << bits) for a in range(1 << bits)]
    b = AirBuilder(4, [0, 1], 2, aux_cols=1, n_rap=1, aux_kind=AUX_PROGRAM, periodic=[table, keys, values], main_inputs=2)
    m = b.main
    m.fetch(m.load(0, 0) + m.load(0, 1) * (1 << bits), m.periodic(0, 1), m.periodic(0, 2), 2 * bits)

    def packed(load):
        return load(0, 0) + load(0, 1) * (1 << bits) + load(0, 2) * (1 << (2 * bits))

    m.multiplicity(packed(m.load), m.periodic(0, 0), 3 * bits)
    _logup_sum(b, packed(b.load), packed(b.aux.load), 3, 4)
    return b


def xor_fetch_inputs(n, bits, rng):
    """(n, 2) Python ints [a, b]: the first two columns of xor_lookup_inputs under the same rng."""
    return [r[:2] for r in xor_lookup_inputs(n, bits, rng)]


def rom_reads(n, key_bits=64):
    """n reads from a read-only memory of n cells, one write and one read a row (Cairo's access pattern for its program segment and
    its public memory).  Inputs: the written address addr_w (column 0), the written value val_w (column 1) and the read address addr_r
    (column 2), addresses below 2^key_bits.  The device builds val_r = fetch(addr_r, addr_w, val_w) (column 3) and m =
    multiplicity(addr_r, addr_w) (column 4); the auxiliary column 5 is one LogUp sum over (address, value) pairs compressed with a
    second challenge: s_0 = 0, s' = s + m / (gamma - addr_w - alpha val_w) - 1 / (gamma - addr_r - alpha val_r), degree 3 with no
    exempted row, so that row n - 1 wraps to s_0 = 0 and closes the sum.  The written addresses must be DISTINCT for the statement to
    mean a memory: of two rows that write one address the lowest is the one every read fetches and the one that carries the
    multiplicity, and the sum says nothing about the other."""
    b = AirBuilder(5, [0, 1], 2, aux_cols=1, n_rap=2, aux_kind=AUX_PROGRAM, main_inputs=3)
    m = b.main
    m.fetch(m.load(0, 2), m.load(0, 0), m.load(0, 1), key_bits)
    m.multiplicity(m.load(0, 2), m.load(0, 0), key_bits)
    gamma, alpha = b.rap(0), b.rap(1)
    dw, dr = gamma - b.load(0, 0) - alpha * b.load(0, 1), gamma - b.load(0, 2) - alpha * b.load(0, 3)
    b.constraint((b.load(1, 5) - b.load(0, 5)) * dw * dr - b.load(0, 4) * dr + dw, degree=3, exemptions=0)
    b.boundary(5, 0, 0)
    g, a = b.aux.rap(0), b.aux.rap(1)
    xw, xr = g - b.aux.load(0, 0) - a * b.aux.load(0, 1), g - b.aux.load(0, 2) - a * b.aux.load(0, 3)
    b.aux.running_sum(b.aux.load(0, 4) * xr - xw, xw * xr)
    return b


def rom_reads_inputs(n, key_bits, rng):
    """(n, 3) Python ints [addr_w, val_w, addr_r]: n distinct addresses below 2^key_bits in a shuffled order, values from the whole
    field, and reads of addresses that were written - some of them several times, some never."""
    if key_bits < 64 and (1 << key_bits) < n:
        raise ValueError(f"rom_reads_inputs: {n} distinct addresses need more than {key_bits} key bits")
    if (1 << key_bits) <= 4 * n:
        addrs = list(range(1 << key_bits))
        rng.shuffle(addrs)
        addrs = addrs[:n]
    else:
        seen = set()
        while len(seen) < n:
            seen.add(rng.randrange(1 << key_bits))
        addrs = sorted(seen)
        rng.shuffle(addrs)
    return [[addrs[i], rng.randrange(P), addrs[rng.randrange(max(1, n // 2))]] for i in range(n)]


def rom_reads_trace(inputs):
    """The whole main table of rom_reads as (n, 5) Python ints, from rom_reads_inputs' rows: a dictionary read and a count."""
    first, counts = {}, {}
    for j, (addr_w, val_w, addr_r) in enumerate(inputs):
        first.setdefault(addr_w, j)
        counts[addr_r] = counts.get(addr_r, 0) + 1
    return [[addr_w, val_w, addr_r, inputs[first[addr_r]][1], counts.get(addr_w, 0) if first[addr_w] == j else 0]
            for j, (addr_w, val_w, addr_r) in enumerate(inputs)]


# ---- limbs and bitwise words: two worked examples ---------------------------------------------------------------------------------
def limb_range_check(n, limb_bits, count=2):
    """Every x_i is below 2^(limb_bits count), by limbs (the shape of Cairo's range-check builtin): one input x (column 0); the device
    builds its `count` limbs of limb_bits bits (columns 1 .. count, MainProgram.limbs: one group) and m_j = multiplicity(limb_j, T,
    limb_bits) for each (columns count + 1 .. 2 count), T periodic column 0, which holds all 2^limb_bits values (at most n of them).
    One recomposition constraint x = sum_j 2^(j limb_bits) limb_j on every row, and per limb the LogUp running sum of table_lookup
    (auxiliary column j, under one challenge).  The caller uploads n values where the table has n x (1 + 2 count); with bits() the same
    range would take limb_bits count committed columns instead of count."""
    if not (1 <= limb_bits <= MAIN_COUNT_MAX_KEY_BITS and 1 <= count <= MAIN_COUNT_MAX_COLS and limb_bits * count <= MAIN_WORD_MAX_BITS):
        raise ValueError(f"limb_range_check: {count} limbs of {limb_bits} bits (at most {MAIN_COUNT_MAX_COLS} limbs, {MAIN_WORD_MAX_BITS} bits in all)")
    if (1 << limb_bits) > n:
        raise ValueError(f"limb_range_check: {1 << limb_bits} table entries on {n} rows")
    main_cols = 1 + 2 * count
    b = AirBuilder(main_cols, [0, 1], 2, aux_cols=count, n_rap=1, aux_kind=AUX_PROGRAM, periodic=[list(range(1 << limb_bits))], main_inputs=1)
    m = b.main
    limbs = m.limbs(m.load(0, 0), limb_bits, count)
    mults = [m.multiplicity(m.load(0, c), m.periodic(0, 0), limb_bits) for c in limbs]
    total = None
    for j, c in enumerate(limbs):
        term = b.load(0, c) * (1 << (j * limb_bits))
        total = term if total is None else total + term
    b.constraint(total - b.load(0, 0), degree=1, exemptions=0)
    for j, (c, mult) in enumerate(zip(limbs, mults)):
        _logup_sum(b, b.load(0, c), b.aux.load(0, c), mult, main_cols + j)
    return b


def limb_range_check_inputs(n, limb_bits, count, rng):
    """(n, 1) Python ints below 2^(limb_bits count) from rng.randrange: the input column of limb_range_check."""
    return [[rng.randrange(1 << (limb_bits * count))] for _ in range(n)]


def limb_range_check_trace(inputs, limb_bits, count):
    """The whole main table of limb_range_check as (n, 1 + 2 count) Python ints, from its input rows: shifts, masks and counts."""
    n, mask = len(inputs), (1 << limb_bits) - 1
    limbs = [[(int(x) % P >> (j * limb_bits)) & mask for j in range(count)] for (x,) in inputs]
    counts = [{} for _ in range(count)]
    for row in limbs:
        for j, v in enumerate(row):
            counts[j][v] = counts[j].get(v, 0) + 1
    # (T(i) = i mod 2^limb_bits: the first row that holds a table value is the value itself)
    return [[int(inputs[i][0]) % P] + limbs[i] + [counts[j].get(i, 0) if i <= mask else 0 for j in range(count)] for i in range(n)]


def limb_range_check_joint(n, limb_bits, count=2):
    """limb_range_check under ONE multiplicity column (sp_air_prove_multi) - another statement of the same range check: one input x
    (column 0), its `count` limbs (columns 1 .. count, one limbs() group) and m = multiplicity_many(limbs, T, limb_bits) (column count +
    1), T periodic column 0, which holds all 2^limb_bits values; 2^limb_bits <= n / 2, so the table entry on the last row is a repeat and
    m is 0 there.  count + 2 main columns where limb_range_check has 1 + 2 count, and the table is sorted once.

    A transition constraint has degree at most 3, so the LogUp sum over count + 1 fractions takes helper columns: auxiliary column p <
    ceil(count / 2) is u_p, the running sum of 1 / (gamma - a) + 1 / (gamma - b) over limbs a = 2 p and b = 2 p + 1 (of 1 / (gamma - a)
    alone for the last limb of an odd count): u_p(0) = 0 and (u_p' - u_p) (gamma - a) (gamma - b) = (gamma - a) + (gamma - b), degree 3.
    The last auxiliary column is v, the running sum of m / (gamma - T) - sum_k 1 / (gamma - limb_k), which the device builds from the
    one fraction: v(0) = 0 and ((v' - v) + sum_p (u_p' - u_p)) (gamma - T) = m, degree 2.  Both leave the last row out (the u_p do not
    close), so that row is a public padding row: x(n - 1) = 0 and limb_k(n - 1) = 0 are boundary constraints, and v(n - 1) = count /
    gamma (boundary_from) is the term of the row the constraints skip, since the whole sum is zero.  The recomposition constraint
    x = sum_j 2^(j limb_bits) limb_j holds on every row, as in limb_range_check.  ceil(count / 2) + 1 auxiliary columns against count."""
    if not (1 <= limb_bits <= MAIN_COUNT_MAX_KEY_BITS and 1 <= count <= MAIN_COUNT_MAX_LIST and limb_bits * count <= MAIN_WORD_MAX_BITS):
        raise ValueError(f"limb_range_check_joint: {count} limbs of {limb_bits} bits (at most {MAIN_COUNT_MAX_LIST} limbs, {MAIN_WORD_MAX_BITS} bits in all)")
    if (2 << limb_bits) > n:
        raise ValueError(f"limb_range_check_joint: {1 << limb_bits} table entries on {n} rows (at most n / 2: the last row's entry must be a repeat)")
    main_cols, pairs = count + 2, (count + 1) // 2
    b = AirBuilder(main_cols, [0, 1], 2, aux_cols=pairs + 1, n_rap=1, aux_kind=AUX_PROGRAM, periodic=[list(range(1 << limb_bits))], main_inputs=1)
    m = b.main
    limbs = m.limbs(m.load(0, 0), limb_bits, count)
    mult = m.multiplicity_many([m.load(0, c) for c in limbs], m.periodic(0, 0), limb_bits)
    total = None
    for j, c in enumerate(limbs):
        term = b.load(0, c) * (1 << (j * limb_bits))
        total = term if total is None else total + term
    b.constraint(total - b.load(0, 0), degree=1, exemptions=0)
    gamma, g = b.rap(0), b.aux.rap(0)
    steps = None        # sum_p (u_p' - u_p)
    for p in range(pairs):
        u_col, members = main_cols + p, limbs[2 * p:2 * p + 2]
        ds = [gamma - b.load(0, c) for c in members]
        step = b.load(1, u_col) - b.load(0, u_col)
        if len(ds) == 2:
            b.constraint(step * ds[0] * ds[1] - ds[0] - ds[1], degree=3, exemptions=1)
        else:
            b.constraint(step * ds[0] - 1, degree=2, exemptions=1)
        b.boundary(u_col, 0, 0)
        steps = step if steps is None else steps + step
        xs = [g - b.aux.load(0, c) for c in members]
        if len(xs) == 2:
            b.aux.running_sum(xs[0] + xs[1], xs[0] * xs[1])
        else:
            b.aux.running_sum(1, xs[0])
    v_col = main_cols + pairs
    b.constraint((b.load(1, v_col) - b.load(0, v_col) + steps) * (gamma - b.periodic(0, 0)) - b.load(0, mult), degree=2, exemptions=1)
    b.boundary(v_col, 0, 0)
    # v as one fraction: N / D with D = (g - T) prod_k (g - limb_k), N = m prod_k (g - limb_k) - (g - T) sum_k prod_(j != k) (g - limb_j)
    xs, xt = [g - b.aux.load(0, c) for c in limbs], g - b.aux.table(0, 0)
    prod, others = xs[0], b.aux.const(1)     # over the limbs so far: their product, and the sum over k of the products without k
    for x in xs[1:]:
        others, prod = others * x + prod, prod * x
    b.aux.running_sum(b.aux.load(0, mult) * prod - xt * others, xt * prod)
    b.boundary(0, n - 1, 0)
    for c in limbs:
        b.boundary(c, n - 1, 0)
    b.boundary_from(v_col, n - 1, b.public.const(count), b.public.rap(0))
    return b


def limb_range_check_joint_inputs(n, limb_bits, count, rng):
    """(n, 1) Python ints below 2^(limb_bits count) from rng.randrange, the last row the public padding row x = 0: the input column of
    limb_range_check_joint."""
    return [[rng.randrange(1 << (limb_bits * count))] for _ in range(n - 1)] + [[0]]


def limb_range_check_joint_trace(inputs, limb_bits, count):
    """The whole main table of limb_range_check_joint as (n, count + 2) Python ints, from its input rows: shifts, masks and one count
    over all limbs of all rows."""
    n, mask = len(inputs), (1 << limb_bits) - 1
    limbs = [[(int(x) % P >> (j * limb_bits)) & mask for j in range(count)] for (x,) in inputs]
    counts = {}
    for row in limbs:
        for v in row:
            counts[v] = counts.get(v, 0) + 1
    # (T(i) = i mod 2^limb_bits: the first row that holds a table value is the value itself)
    return [[int(inputs[i][0]) % P] + limbs[i] + [counts.get(i, 0) if i <= mask else 0] for i in range(n)]


def word_ops(n, bits):
    """a = x AND y, o = x OR y and e = x XOR y on every row, for `bits`-bit x and y (the shape of Cairo's bitwise builtin, at a width a
    bit decomposition can still pin down).  Inputs x and y (columns 0 and 1); the device builds the bits of x (columns 2 .. 1 + bits)
    and of y (the next `bits` columns) - BIT columns - and the three WORD columns a, o, e behind them.  Constraints, all of degree 2 on
    every row, with no auxiliary segment and no periodic column: every bit is a bit, the two recompositions, a = sum_j 2^j xb_j yb_j,
    e = x + y - 2 a and o = x + y - a.  degree_bound_factor 1."""
    if not 1 <= bits <= 16:
        raise ValueError(f"word_ops: {bits} bits (1 .. 16: 2 bits + 5 transition constraints, and a descriptor takes 64)")
    b = AirBuilder(5 + 2 * bits, [0], 1, main_inputs=2)
    m = b.main
    xb, yb = m.bits(m.load(0, 0), bits), m.bits(m.load(0, 1), bits)
    a, o, e = m.word_and(m.load(0, 0), m.load(0, 1), bits), m.word_or(m.load(0, 0), m.load(0, 1), bits), m.word_xor(m.load(0, 0), m.load(0, 1), bits)
    for c in xb + yb:
        v = b.load(0, c)
        b.constraint(v * (v - 1), degree=2, exemptions=0)
    x, y = b.load(0, 0), b.load(0, 1)
    for value, cols in ((x, xb), (y, yb)):
        total = None
        for j, c in enumerate(cols):
            term = b.load(0, c) * (1 << j)
            total = term if total is None else total + term
        b.constraint(total - value, degree=1, exemptions=0)
    both = None
    for j, (cx, cy) in enumerate(zip(xb, yb)):
        term = b.load(0, cx) * b.load(0, cy) * (1 << j)
        both = term if both is None else both + term
    b.constraint(both - b.load(0, a), degree=2, exemptions=0)
    b.constraint(b.load(0, e) - (x + y - b.load(0, a) * 2), degree=1, exemptions=0)
    b.constraint(b.load(0, o) - (x + y - b.load(0, a)), degree=1, exemptions=0)
    return b


def word_ops_inputs(n, bits, rng):
    """(n, 2) Python ints [x, y] below 2^bits from rng.randrange; the first rows hold the all-ones and the all-zeros words."""
    top = (1 << bits) - 1
    rows = [[rng.randrange(top + 1), rng.randrange(top + 1)] for _ in range(n)]
    rows[:3] = [[top, 0], [top, top], [0, 0]]
    return rows


def word_ops_trace(inputs, bits):
    """The whole main table of word_ops as (n, 5 + 2 bits) Python ints, from its input rows."""
    return [[x, y] + [(x >> j) & 1 for j in range(bits)] + [(y >> j) & 1 for j in range(bits)] + [x & y, x | y, x ^ y] for x, y in inputs]


# ---- quotients in chain steps: a worked example -----------------------------------------------------------------------------------
def ec_subset_sum(n, s, points, shift, result):
    """n / s fixed-base accumulations on a curve y^2 = x^3 + a x + beta, one per block of s rows (the shape of Cairo's Pedersen, EC-op
    and ECDSA builtins): the caller uploads the bits b (column 0) and the device builds the rest (sp_air_prove_div).  Columns 1 - 3 are
    the chain group (x, y, lambda): the accumulator and the slope of the chord to the row's public point P_t = `points`[t] (periodic
    columns 0 and 1, period s).  Seeds: (x, y) = `shift`, a public point, and lambda = (y - y_P) / (x - x_P) - a quotient in a seed.
    Step: the row adds P_t when b = 1 and keeps the accumulator when b = 0,

        x' = b (lambda^2 - x - x_P) + (1 - b) x,    y' = b (lambda (x - x_add) - y) + (1 - b) y    (x_add the added point's x),
        lambda' = (y' - y_P(i + 1)) / (x' - x_P(i + 1))

    - a quotient over the step's own new values, with the periodic columns read at shift 1.  Columns 4 and 5 are the row-local q =
    lambda^2 and u = b lambda (VALUE), which keep every constraint at degree 3 under degree_bound_factor 2.  Periodic column 2 is
    sel = [1] (s - 1) + [0].  Constraints, no exemption: b (b - 1); lambda (x - x_P) - (y - y_P); q - lambda^2; u - b lambda;
    sel (b (q - x - x_P - x') + (1 - b) (x' - x)); sel (u (x - x') - b (y + y') + (1 - b) (y' - y)) on every row - sel switches the
    last two off where a block ends -; x - shift_x and y - shift_y on the rows = 0 (mod s).  The boundary constraints (x, y) = `result`
    on row s - 1 are block 0's public sum (ec_subset_sum_result): shift + the sum of b_t P_t over t < s - 1; the last point of a block
    is met by the slope alone.  An accumulator that meets +-P_t has no chord: the device answers SP_E_ZERO_INVERSE, evaluate ValueError
    - `shift` is there to keep the sums off the points."""
    if s < 2 or s & (s - 1) or s > n or len(points) != s:
        raise ValueError(f"ec_subset_sum: blocks of {s} rows with {len(points)} points on {n} rows (a power of two in 2 .. n, one point per row of a block)")
    b = AirBuilder(6, [0, 1], 2, periodic=[[p[0] for p in points], [p[1] for p in points], [1] * (s - 1) + [0]], main_inputs=1)
    m = b.main
    sx, sy = m.const(shift[0]), m.const(shift[1])
    g = m.chain(s, [sx, sy, (sy - m.periodic(0, 1)) / (sx - m.periodic(0, 0))])
    bit, x, y, lam = m.load(0, 0), g.state(0), g.state(1), g.state(2)
    x_add = lam * lam - x - m.periodic(0, 0)
    x2 = bit * x_add + (1 - bit) * x
    y2 = bit * (lam * (x - x_add) - y) + (1 - bit) * y
    g.step([x2, y2, (y2 - m.periodic(1, 1)) / (x2 - m.periodic(1, 0))])
    cx, cy, cl = g.cols
    q = m.value(m.load(0, cl) * m.load(0, cl))
    u = m.value(m.load(0, 0) * m.load(0, cl))
    B, X, Y, L, Q, U = b.load(0, 0), b.load(0, cx), b.load(0, cy), b.load(0, cl), b.load(0, q), b.load(0, u)
    X1, Y1 = b.load(1, cx), b.load(1, cy)
    XP, YP, SEL = b.periodic(0, 0), b.periodic(0, 1), b.periodic(0, 2)
    b.constraint(B * (B - 1), degree=2, exemptions=0)
    b.constraint(L * (X - XP) - (Y - YP), degree=2, exemptions=0)
    b.constraint(Q - L * L, degree=2, exemptions=0)
    b.constraint(U - B * L, degree=2, exemptions=0)
    b.constraint(SEL * (B * (Q - X - XP - X1) + (1 - B) * (X1 - X)), degree=3, exemptions=0)
    b.constraint(SEL * (U * (X - X1) - B * (Y + Y1) + (1 - B) * (Y1 - Y)), degree=3, exemptions=0)
    b.constraint(X - shift[0], degree=1, exemptions=0, period=s, offset=0)
    b.constraint(Y - shift[1], degree=1, exemptions=0, period=s, offset=0)
    b.boundary(cx, s - 1, result[0])
    b.boundary(cy, s - 1, result[1])
    return b


def _ec_add(p, q):
    """The chord addition of two affine points with different x (the only case ec_subset_sum meets)."""
    lam = (p[1] - q[1]) * pow(p[0] - q[0], P - 2, P) % P
    x = (lam * lam - p[0] - q[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def ec_subset_sum_result(bits, points, shift):
    """(x, y) on the last row of the block whose bits are `bits` (its first s - 1 count): the public sum of ec_subset_sum."""
    acc = (shift[0] % P, shift[1] % P)
    for bit, point in zip(bits[:len(points) - 1], points):
        if int(bit):
            acc = _ec_add(acc, point)
    return acc


def ec_subset_sum_inputs(n, rng):
    """(n, 1) Python ints: a random bit on every row."""
    return [[rng.randrange(2)] for _ in range(n)]


# ---- integer ops in chain steps: a worked example ----------------------------------------------------------------------------------
def _arx_round(x, y, key, bits, alpha, beta):
    """One round of the Speck-like permutation of arx_chain on two `bits`-wide words: (x', y', the sum before it is reduced)."""
    mask = (1 << bits) - 1
    a, r = alpha % bits, beta % bits
    total = (((x >> a) | (x << (bits - a))) & mask) + y + key
    x2 = total & mask
    return x2, (((y << r) | (y >> (bits - r))) & mask) ^ x2, total


def arx_chain(n, s, keys, digest, bits=16, alpha=7, beta=2):
    """n / s independent Speck-like permutations over two `bits`-wide words, one per block of s rows (the shape of an ARX cipher's
    rounds, and of the additions, rotations and XORs of a SHA-2 or Blake compression): the caller uploads the words a and b (columns 0
    and 1, below 2^bits, of which only the rows = 0 (mod s) matter) and the device builds the rest (sp_air_prove_int).  Columns 2 and 3
    are the chain group (x, y) with seeds a and b and the step - integer ops inside a recurrence -

        x' = (rotr(x, alpha) + y + K) mod 2^bits,    y' = rotl(y, beta) xor x'

    K periodic column 0 (period s, values below 2^bits); periodic column 1 is sel = [1] (s - 1) + [0].  Behind the group, all row-local:
    the bits of x (columns 4 .. 3 + bits) and of y (the next `bits`) - BIT columns - and the two carry bits c_j = limb(rotr(x) + y + K,
    bits + j, 1) - LIMB columns, rotr(x) written linearly over x's bits.  Constraints under degree_bound_factor 2, no exemption: every
    bit and carry is a bit; the two recompositions; sel (x' + 2^bits (c_0 + 2 c_1) - rotr(x) - y - K); per bit j sel (yb'_j - r_j - xb'_j +
    2 r_j xb'_j) with r_j = yb_((j - beta) mod bits) - sel switches both off where a block ends -; x - a and y - b on the rows = 0
    (mod s).  The boundary constraint x_(s-1) = digest is block 0's public digest (arx_chain_digest).  At bits = 16: 38 columns and 55
    transition constraints.  No auxiliary segment."""
    if s < 2 or s & (s - 1) or s > n or len(keys) != s:
        raise ValueError(f"arx_chain: blocks of {s} rows with {len(keys)} keys on {n} rows (a power of two in 2 .. n, one key per row of a block)")
    if not 2 <= bits <= 16 or not 0 < alpha % bits or not 0 < beta % bits:
        raise ValueError(f"arx_chain: {bits}-bit words rotated by {alpha} and {beta} (2 .. 16 bits - 3 bits + 7 transition constraints, and a descriptor "
                         "takes 64 -, rotations that are no multiple of the width)")
    if any(not 0 <= int(k) < 1 << bits for k in keys):
        raise ValueError(f"arx_chain: a key outside 0 .. 2^{bits} - 1")
    alpha, beta = alpha % bits, beta % bits
    b = AirBuilder(6 + 2 * bits, [0, 1], 2, periodic=[list(keys), [1] * (s - 1) + [0]], main_inputs=2)
    m = b.main
    g = m.chain(s, [m.load(0, 0), m.load(0, 1)])
    x2 = m.int_add(m.int_rotr(g.state(0), alpha, bits) + g.state(1), m.periodic(0, 0), bits)
    g.step([x2, m.int_xor(m.int_rotl(g.state(1), beta, bits), x2)])
    cx, cy = g.cols
    xb, yb = m.bits(m.load(0, cx), bits), m.bits(m.load(0, cy), bits)

    def rotr_of_bits(load):
        total = None
        for j in range(bits):
            term = load(0, xb[(j + alpha) % bits]) * (1 << j)
            total = term if total is None else total + term
        return total

    total = rotr_of_bits(m.load) + m.load(0, cy) + m.periodic(0, 0)
    carry = [m.limb(total, bits + j, 1) for j in range(2)]
    for c in xb + yb + carry:
        v = b.load(0, c)
        b.constraint(v * (v - 1), degree=2, exemptions=0)
    for col, cols in ((cx, xb), (cy, yb)):
        word = None
        for j, c in enumerate(cols):
            term = b.load(0, c) * (1 << j)
            word = term if word is None else word + term
        b.constraint(word - b.load(0, col), degree=1, exemptions=0)
    sel = b.periodic(0, 1)
    b.constraint(sel * (b.load(1, cx) + (b.load(0, carry[0]) + b.load(0, carry[1]) * 2) * (1 << bits) - rotr_of_bits(b.load) - b.load(0, cy) - b.periodic(0, 0)),
                 degree=2, exemptions=0)
    for j in range(bits):
        r, nx = b.load(0, yb[(j - beta) % bits]), b.load(1, xb[j])
        b.constraint(sel * (b.load(1, yb[j]) - r - nx + r * nx * 2), degree=3, exemptions=0)
    b.constraint(b.load(0, cx) - b.load(0, 0), degree=1, exemptions=0, period=s, offset=0)
    b.constraint(b.load(0, cy) - b.load(0, 1), degree=1, exemptions=0, period=s, offset=0)
    b.boundary(cx, s - 1, digest)
    return b


def arx_chain_digest(words, s, keys, bits=16, alpha=7, beta=2):
    """x on the last row of the block seeded from words = (a, b): the public digest of arx_chain (rounds 0 .. s - 2; the last key is read
    by the carries alone)."""
    x, y = int(words[0]), int(words[1])
    for t in range(s - 1):
        x, y, _ = _arx_round(x, y, int(keys[t]), bits, alpha, beta)
    return x


def arx_chain_inputs(n, s, rng, bits=16):
    """(n, 2) Python ints [a, b] below 2^bits from rng.randrange: two words on every row = 0 (mod s), the caller's filler on the others;
    the first blocks hold the all-ones and the all-zeros words."""
    top = (1 << bits) - 1
    rows = [[rng.randrange(top + 1), rng.randrange(top + 1)] for _ in range(n)]
    for block, words in enumerate(([top, top], [0, 0], [top, 0])):
        if block * s < n:
            rows[block * s] = list(words)
    return rows


def arx_chain_trace(inputs, s, keys, bits=16, alpha=7, beta=2):
    """The whole main table of arx_chain as (n, 6 + 2 bits) Python ints, from its input rows: shifts, masks and Python's operators."""
    table = []
    for i, (a, b) in enumerate(inputs):
        t = i % s
        x, y = (int(a), int(b)) if t == 0 else nxt
        x2, y2, total = _arx_round(x, y, int(keys[t]), bits, alpha, beta)
        nxt = (x2, y2)
        table.append([int(a), int(b), x, y] + [(x >> j) & 1 for j in range(bits)] + [(y >> j) & 1 for j in range(bits)] + [(total >> (bits + j)) & 1 for j in range(2)])
    return table
