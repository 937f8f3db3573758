"""The plain reference of program_ref for main programs that hold integer ops in chain steps (ops 8 .. 11, the _int entry points): the
same builder of the table - Python integers, one cell at a time, a chain group by state -, with an evaluator that knows

    op 8  LIMB a, b = lo + 256 width   (int(v[a]) >> lo) mod 2^width      - b is an immediate, never a value
    op 9 / 10 / 11  AND / OR / XOR a b  over the canonical integers, both below 2^251

beside ops 0 .. 7.  It shares nothing with MainProgram.evaluate.  program_ref.py stays as it is: main_table below runs its main_table
with this evaluator in the place of program_ref._Ops.

Errors as the device reports them: WordOutOfRange for an AND, OR or XOR operand at or above 2^251 on a row its group evaluates,
ZeroDenominator for a zero under an op 7 or a column's D - and where a program meets both, the range error, as the device's verdict
puts it first.  The device does not stop at either: a quotient over zero is zero and a word is masked to 251 bits, and the lanes go on;
`lenient` follows it through the table to find out which flags such a run raises."""
import program_ref
from program_ref import P, DIV, WordOutOfRange, ZeroDenominator, limb, word

INT_LIMB, INT_AND, INT_OR, INT_XOR = 8, 9, 10, 11
INT_BITS = 251


class _IntOps(program_ref._Ops):
    lenient = False          # True: go on as the device does, and note what it would flag
    flagged_range = flagged_zero = False

    def _op(self, t, i, load, operand):
        op, a, b = self.ops[t]
        if op == INT_LIMB:
            assert b >> 8 >= 1 and (b & 255) + (b >> 8) <= 252, f"op {t}: a LIMB op with lo + 256 width = {b}"
            return limb(operand(a), b & 255, b >> 8)
        if op in (INT_AND, INT_OR, INT_XOR):
            x, y = operand(a), operand(b)
            if x >> INT_BITS or y >> INT_BITS:
                if not self.lenient:
                    raise WordOutOfRange(f"op {t}, row {i}: {x} or {y} >= 2^{INT_BITS}")
                type(self).flagged_range = True
            return word(op - INT_AND, x, y) & ((1 << INT_BITS) - 1)
        if op == DIV:        # (Euclid's inverse: a tenth of the time of program_ref's exponentiation, for tables of thousands of rows)
            u, v = operand(a), operand(b)
            if v == 0:
                if not self.lenient:
                    raise ZeroDenominator(f"op {t} divides by zero on row {i}")
                type(self).flagged_zero = True
                return 0
            return u * pow(v, -1, P) % P
        return super()._op(t, i, load, operand)

    def quotient(self, num_op, den_op, i):
        if self.lenient and den_op != program_ref.NO_DEN and self.val(den_op, i) == 0:
            type(self).flagged_zero = True
            return 0
        return super().quotient(num_op, den_op, i)


def _run(program, input_rows, lenient):
    saved = program_ref._Ops
    _IntOps.lenient, _IntOps.flagged_range, _IntOps.flagged_zero = lenient, False, False
    program_ref._Ops = _IntOps
    try:
        return program_ref.main_table(program, input_rows)
    finally:
        program_ref._Ops = saved
        _IntOps.lenient = False


def main_table(program, input_rows):
    """program_ref.main_table for a program with ops 0 .. 11.  WordOutOfRange where an integer op's operand is out of range on a row its
    group evaluates (or a WORD column's is), ZeroDenominator for a zero denominator that the device would report alone."""
    try:
        return _run(program, input_rows, False)
    except (WordOutOfRange, ZeroDenominator) as first:
        try:
            _run(program, input_rows, True)
        except WordOutOfRange:       # (a WORD column of the same program: the same verdict word)
            raise WordOutOfRange(str(first)) from None
        if _IntOps.flagged_range:
            raise first if isinstance(first, WordOutOfRange) else WordOutOfRange("an integer op's operand is out of range beside a zero denominator") from None
        raise first
