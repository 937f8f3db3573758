"""An affine elliptic-curve adder over plain integers, and the table of air.ec_subset_sum written with it: what the quotients of a chain
step (op 7) are checked against beside the plain reference of program_ref."""
from program_ref import P, ZeroDenominator


# ---- affine points of y^2 = x^3 + x + beta ----------------------------------------------------------------------------------------
def ec_add(p, q):
    """p + q for affine points with different x."""
    if (p[0] - q[0]) % P == 0:
        raise ZeroDenominator("the chord of two points with one x")
    lam = (q[1] - p[1]) * pow(q[0] - p[0], P - 2, P) % P
    x = (lam * lam - p[0] - q[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def ec_subset_sum_table(rows, s, points, shift):
    """The main segment of air.ec_subset_sum over the bits `rows`: [b, x, y, lambda, lambda^2, b lambda] on every row, the accumulator
    moved by ec_add and the slope computed from the two points it joins."""
    out = []
    for i, (bit,) in enumerate(rows):
        t = i % s
        if t == 0:
            acc = (shift[0] % P, shift[1] % P)
        elif out[i - 1][0]:
            acc = ec_add(acc, points[t - 1])
        px, py = points[t]
        if (acc[0] - px) % P == 0:
            raise ZeroDenominator(i)
        lam = (acc[1] - py) * pow(acc[0] - px, P - 2, P) % P
        out.append([int(bit) % P, acc[0], acc[1], lam, lam * lam % P, int(bit) * lam % P])
    return out
