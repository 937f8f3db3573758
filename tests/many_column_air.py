"""AIRs wider than the Cairo kernels' constant blocks, for sp_air_prove (include/stark252_hip.h sp_air_desc; the reference's
AIR trait, src/starks/traits.rs:15-119, bounds none of this): up to 1024 columns, boundary constraints on many rows.

Main column j counts up by its own constant k_j (x_j(i) = s_j + i k_j), so the constant pool grows with the width.  Every
transition constraint sums the weighted recurrences x_j(i+1) - x_j(i) - k_j of several columns; with three frame rows one more
constraint ties rows i and i+2.  Auxiliary column q (AUX_CALLBACK, one RAP challenge gamma) is the running sum
z_q(i+1) = z_q(i) + gamma x_q(i), z_q(0) = 0.  Boundary constraints pin rows 0 and n-1 and a spread of rows in between, several
constraints per row, and some columns more than once."""
import numpy as np

from lambdaworks_cairo_prover_amd import air

P = air.P


def column_start(j):
    return 3 * j + 1


def column_step(j):
    return 7 * j + 5


def cell(i, j):
    return column_start(j) + i * column_step(j)


def main_trace(n, main_cols):
    """row-major (n, main_cols, 32) canonical big-endian bytes (the default context encoding)."""
    i = np.arange(n, dtype=np.uint64)[:, None]
    j = np.arange(main_cols, dtype=np.uint64)[None, :]
    v = (3 * j + 1) + i * (7 * j + 5)
    out = np.zeros((n, main_cols, 32), dtype=np.uint8)
    out[:, :, 24:] = v.astype(">u8").view(np.uint8).reshape(n, main_cols, 8)
    return out


def aux_trace(n, aux_cols, rap):
    gamma = rap[0]
    rows = [[0] * aux_cols for _ in range(n)]
    for q in range(aux_cols):
        z = 0
        for i in range(n):
            rows[i][q] = z
            z = (z + gamma * cell(i, q)) % P
    return rows


def boundary_rows(n, rows):
    """0, n - 1 and rows - 2 rows spread in between (distinct)."""
    if rows <= 1:
        return [0]
    inner = sorted({1 + (k * (n - 2)) // (rows - 1) for k in range(1, rows - 1)}) if rows > 2 else []
    out = [0] + [r for r in inner if 0 < r < n - 1] + [n - 1]
    assert len(out) == rows, (n, rows)
    return out


def boundary_list(n, main_cols, rows, total):
    """(col, step) of `total` constraints over `rows` distinct rows: constraint b on row rows[b % rows]."""
    steps = boundary_rows(n, rows)
    return [((b * 37 + 11) % main_cols, steps[b % rows]) for b in range(total)]


def build(n, main_cols, aux_cols=0, frame_rows=2, boundary_row_count=4, boundary_total=None, n_transitions=None,
          per_constraint=None, value_offset=None):
    """AirBuilder of the AIR described above.  boundary_total defaults to 2 per boundary row; value_offset = (index, delta) adds
    delta to the value of one boundary constraint (a trace that violates it)."""
    assert frame_rows in (2, 3)
    extra = (1 if frame_rows == 3 else 0) + aux_cols
    if n_transitions is None:
        n_transitions = min(air.MAX_TRANSITIONS - extra, max(1, main_cols // 4))
    b = air.AirBuilder(main_cols, list(range(frame_rows)), 1, aux_cols=aux_cols, n_rap=1 if aux_cols else 0,
                       aux_kind=air.AUX_CALLBACK if aux_cols else air.AUX_NONE,
                       num_transition_exemptions=2 if frame_rows == 3 else 1,
                       aux_builder=(lambda rap: aux_trace(n, aux_cols, rap)) if aux_cols else None)
    groups = [[] for _ in range(n_transitions)]
    for j in range(main_cols):
        groups[j % n_transitions].append(j)
    if per_constraint:
        groups = [g[:per_constraint] for g in groups]
    for g in groups:
        acc = None
        for j in g:
            rec = b.load(1, j) - b.load(0, j) - column_step(j)
            w = j % 5 + 1
            term = rec if w == 1 else rec * w
            acc = term if acc is None else acc + term
        b.constraint(acc, 1, 1)
    if frame_rows == 3:
        acc = None
        for j in range(min(8, main_cols)):
            t = b.load(2, j) - b.load(0, j) - 2 * column_step(j)
            acc = t if acc is None else acc + t
        b.constraint(acc, 1, 2)
    if aux_cols:
        gamma = b.rap(0)
        for q in range(aux_cols):
            b.constraint(b.load(1, main_cols + q) - b.load(0, main_cols + q) - gamma * b.load(0, q), 1, 1)
    total = 2 * boundary_row_count if boundary_total is None else boundary_total
    for idx, (col, step) in enumerate(boundary_list(n, main_cols, boundary_row_count, total)):
        v = cell(step, col)
        if value_offset and value_offset[0] == idx:
            v += value_offset[1]
        b.boundary(col, step, v)
    for q in range(aux_cols):
        b.boundary(main_cols + q, 0, 0)
    return b
