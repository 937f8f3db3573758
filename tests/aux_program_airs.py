"""AIRs whose auxiliary columns are aux programs (sp_air_prove_aux, air.AUX_PROGRAM): a permutation argument and a LogUp lookup,
and the callback-built test AIRs of wide_air / many_column_air with the same columns written as programs.

Main columns (row i of n, n a power of two >= 4):
    a = i + 1, b = 3 i + 2                       the pairs
    a_perm, b_perm = (a, b) of row s(i)          s(i) = (5 i + 3) mod n, a permutation of the rows
    t = i                                        the lookup table
    m = 2 for i < n / 2, else 0                  how often t_i is looked up
    f = s(i) // 2                                the looked-up values: every table value below n / 2 twice
    extra columns x_j = j + i (no constraint reads them; they widen the trace)

Permutation argument (challenges beta, gamma).  Column z with shift r reads the permuted pair r rows further on:
    z_0 = 1,  z_(i+1) = z_i (a_i + beta b_i + gamma) / (a_perm_(i+r) + beta b_perm_(i+r) + gamma)   (row indices mod n)
The rows i + r run over every row once, so the denominators over all n rows are the numerators in another order and the
product over all n rows is 1: z_n = z_0.  The transition z_(i+1) D(i) - z_i N(i) = 0 therefore holds on every row (it is declared
with one exempted row, as the reference's examples do), and a boundary constraint pins z_0 = 1.

LogUp lookup (challenge gamma).  Column s with shift r:
    s_0 = 0,  s_(i+1) = s_i + m_i / (gamma - t_i) - 1 / (gamma - f_(i+r))
written as one fraction N / D with N = m_i (gamma - f_(i+r)) - (gamma - t_i), D = (gamma - t_i)(gamma - f_(i+r)).  Every value
of f is looked up once over the n rows and table value j has multiplicity m_j = #{i : f_i = j}, so the sum over all rows is 0
and s_n = s_0; the transition (s_(i+1) - s_i) D - N = 0 holds, and s_0 = 0 is a boundary constraint.
"""
from lambdaworks_cairo_prover_amd import air

P = air.P
A, B, AP, BP, T, M, F = range(7)
BASE_COLS = 7


def perm_index(i, n):
    return (5 * i + 3) % n


def main_rows(n, extra_cols=0):
    rows = []
    for i in range(n):
        s = perm_index(i, n)
        rows.append([i + 1, 3 * i + 2, s + 1, 3 * s + 2, i, 2 if i < n // 2 else 0, s // 2] + [j + i for j in range(extra_cols)])
    return rows


def main_trace(n, extra_cols=0):
    """(n, 7 + extra_cols, 32) canonical big-endian bytes (the default context encoding)."""
    return air.ints_to_bytes(main_rows(n, extra_cols))


def rap_air(n, perm_shifts=(), logup_shifts=(), extra_cols=0):
    """One product column per entry of perm_shifts, then one running-sum column per entry of logup_shifts (as above)."""
    K = len(perm_shifts) + len(logup_shifts)
    offsets = list(range(max(2, 1 + max([0, *perm_shifts, *logup_shifts]))))   # frame rows 0, 1 and every shift
    b = air.AirBuilder(BASE_COLS + extra_cols, offsets, 2, aux_cols=K, n_rap=2, aux_kind=air.AUX_PROGRAM)
    beta, gamma = b.rap(0), b.rap(1)
    b.constraint(b.load(1, A) - b.load(0, A) - 1, 2, 1)
    b.constraint(b.load(1, B) - b.load(0, B) - 3, 2, 1)
    b.constraint(b.load(1, T) - b.load(0, T) - 1, 2, 1)
    x = b.aux
    xbeta, xgamma = x.rap(0), x.rap(1)
    col = BASE_COLS + extra_cols
    for r in perm_shifts:
        x.product(x.load(0, A) + xbeta * x.load(0, B) + xgamma, x.load(r, AP) + xbeta * x.load(r, BP) + xgamma)
        num = b.load(0, A) + beta * b.load(0, B) + gamma
        den = b.load(r, AP) + beta * b.load(r, BP) + gamma
        b.constraint(b.load(1, col) * den - b.load(0, col) * num, 2, 1)
        b.boundary(col, 0, 1)
        col += 1
    for r in logup_shifts:
        gt, gf = xgamma - x.load(0, T), xgamma - x.load(r, F)
        x.running_sum(x.load(0, M) * gf - gt, gt * gf)
        ct, cf = gamma - b.load(0, T), gamma - b.load(r, F)
        b.constraint((b.load(1, col) - b.load(0, col)) * ct * cf - (b.load(0, M) * cf - ct), 3, 1)
        b.boundary(col, 0, 0)
        col += 1
    b.boundary(A, 0, 1); b.boundary(B, 0, 2); b.boundary(T, 0, 0)
    return b


def permutation_air(n):
    """The grand product, the permuted pair read three rows on (a shift that wraps on the last three rows)."""
    return rap_air(n, perm_shifts=(3,))


def logup_air(n):
    """The LogUp running sum, f read one row on (row n - 1 reads row 0)."""
    return rap_air(n, logup_shifts=(1,))


def _as_program(b, fill):
    b.aux_kind, b.aux_builder = air.AUX_PROGRAM, None
    b.aux = air.AuxProgram(b.main_cols, b.n_rap)
    fill(b.aux)
    return b


def wide_air_program(n):
    """wide_air.build(n) with its callback columns as an aux program: z' = z (a + gamma), s' = s + delta c."""
    import wide_air

    def fill(x):
        gamma, delta = x.rap(0), x.rap(1)
        x.product(x.load(0, 0) + gamma)
        x.running_sum(delta * x.load(0, 2))
    return _as_program(wide_air.build(n), fill)


def many_column_air_program(n, main_cols, aux_cols, **kw):
    """many_column_air.build(...) with its callback columns as an aux program: z_q' = z_q + gamma x_q."""
    import many_column_air

    def fill(x):
        gamma = x.rap(0)
        for q in range(aux_cols):
            x.running_sum(gamma * x.load(0, q))
    return _as_program(many_column_air.build(n, main_cols, aux_cols, **kw), fill)
