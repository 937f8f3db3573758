"""Traces and AIRs for the trace-report tests (AirBuilder.check_trace, sp_air_check_trace): satisfying traces of the example AIRs in
Python integers, the trace a report is compared on (main||aux, however the AIR builds its auxiliary columns), and a few AIRs whose
reports exercise what the examples do not (64 constraints, a permutation argument that closes on the wrap-around row)."""
from lambdaworks_cairo_prover_amd import air

P = air.P
SMALL_RAP = 10
BIG_RAP = (1 << 250) + 0x1234567890ABCDEF1234567890ABCDEF      # ~250 bits


def fib(n, a0=1, a1=1):
    v = [a0 % P, a1 % P]
    while len(v) < n:
        v.append((v[-1] + v[-2]) % P)
    return v[:n]


def simple_fibonacci_rows(n, a0=1, a1=1):
    return [[x] for x in fib(n, a0, a1)]


def fibonacci_2_columns_rows(n, a0=1, a1=1):
    """a' = a + b, b' = b + a': the Fibonacci sequence two terms a row."""
    f = fib(2 * n, a0, a1)
    return [[f[2 * i], f[2 * i + 1]] for i in range(n)]


def quadratic_rows(n, a0=3):
    rows, x = [], a0 % P
    for _ in range(n):
        rows.append([x])
        x = x * x % P
    return rows


def dummy_rows(n):
    return [[i & 1, x] for i, x in enumerate(fib(n))]


def fibonacci_rap_rows(n, steps):
    """Column a: `steps` Fibonacci terms, then zeros; column b: a rotated by one row (a permutation of it)."""
    a = fib(steps) + [0] * (n - steps)
    return [[a[i], a[(i + 1) % n]] for i in range(n)]


def permutation_column(rows, gamma):
    """z_0 = 1, z_(i+1) = z_i (a_i + gamma) / (b_i + gamma): what aux_kind AUX_FIBONACCI_RAP builds."""
    z, out = 1, []
    for a, b in rows:
        out.append(z)
        z = z * (a + gamma) % P * pow((b + gamma) % P, P - 2, P) % P
    return out


def full_rows(b, rows, rap):
    """main||aux as the prover holds it before round 2, in ints: what AirBuilder.check_trace is given."""
    if b.aux_cols == 0 or b.aux is not None:
        return [list(r) for r in rows]              # (an aux program is evaluated by check_trace itself)
    if b.aux_kind == air.AUX_FIBONACCI_RAP:
        return [list(r) + [z] for r, z in zip(rows, permutation_column(rows, rap[0]))]
    return [list(r) + [int(v) % P for v in x] for r, x in zip(rows, b.aux_builder(list(rap)))]


def changed(rows, *cells):
    """A copy of the rows with delta added to each (row, column, delta) cell."""
    out = [list(r) for r in rows]
    for i, j, d in cells:
        out[i][j] = (out[i][j] + d) % P
    return out


def fibonacci_rap_callback(n, steps, rows, spoil=None):
    """fibonacci_rap with its permutation column from a callback (aux_kind AUX_CALLBACK); spoil = (row, delta) corrupts the column the
    callback returns."""
    def build_aux(rap):
        z = permutation_column(rows, rap[0])
        if spoil:
            z[spoil[0]] = (z[spoil[0]] + spoil[1]) % P
        return [[v] for v in z]
    b = air.AirBuilder(2, [0, 1, 2], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_CALLBACK, num_transition_exemptions=2, aux_builder=build_aux)
    b.constraint(b.load(2, 0) - b.load(1, 0) - b.load(0, 0), 1, 3 + n - steps - 1)
    gamma = b.rap(0)
    b.constraint(b.load(1, 2) * (b.load(0, 1) + gamma) - b.load(0, 2) * (b.load(0, 0) + gamma), 2, 1)
    b.boundary(0, 0, 1); b.boundary(0, 1, 1); b.boundary(2, 0, 1)
    return b


def closed_permutation(n):
    """fibonacci_rap_program's permutation column with its constraint enforced on EVERY row: on row n - 1 the frame wraps to z_0 = 1,
    which holds exactly when the product over all rows is 1 - column b a permutation of column a.  One changed main cell breaks it
    there (fibonacci_rap_program exempts that row, so no main cell can break its permutation constraint: z follows the trace)."""
    b = air.AirBuilder(2, [0, 1], 2, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM)
    gamma = b.rap(0)
    b.constraint(b.load(1, 2) * (b.load(0, 1) + gamma) - b.load(0, 2) * (b.load(0, 0) + gamma), 2, 0)
    b.boundary(2, 0, 1)
    g = b.aux.rap(0)
    b.aux.product(b.aux.load(0, 0) + g, b.aux.load(0, 1) + g)
    return b


def closed_permutation_rows(n):
    return [[i + 1, (5 * i + 3) % n + 1] for i in range(n)]


def counters(n_constraints=64):
    """Column k counts up by k + 1; constraint k says so (one constraint per column, the last row exempt)."""
    b = air.AirBuilder(n_constraints, [0, 1], 1)
    for k in range(n_constraints):
        b.constraint(b.load(1, k) - b.load(0, k) - (k + 1), 1, 1)
    b.boundary(0, 0, 0)
    return b


def counters_rows(n, n_constraints=64):
    return [[i * (k + 1) for k in range(n_constraints)] for i in range(n)]


EXAMPLES = {
    "simple_fibonacci": lambda n: (air.simple_fibonacci(1, 1), simple_fibonacci_rows(n)),
    "fibonacci_2_columns": lambda n: (air.fibonacci_2_columns(1, 1), fibonacci_2_columns_rows(n)),
    "quadratic": lambda n: (air.quadratic(3), quadratic_rows(n)),
    "dummy": lambda n: (air.dummy(), dummy_rows(n)),
    "fibonacci_rap": lambda n: (air.fibonacci_rap(n, n - 4), fibonacci_rap_rows(n, n - 4)),
    "fibonacci_rap_program": lambda n: (air.fibonacci_rap_program(n, n - 4), fibonacci_rap_rows(n, n - 4)),
}
