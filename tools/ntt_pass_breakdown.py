#!/usr/bin/env python3
"""Per-pass figures of the NTT from rocprofv3 rocpd SQLite outputs.  The kernel trace reports the two strided passes of a 2^22
transform under one symbol; here every transform is cut at its first (contiguous) pass and the dispatches are told apart by their
position in the chain.
usage: ntt_pass_breakdown.py <kernel_trace.db> [<pmc.db> ...]"""
import sqlite3
import statistics
import sys


def chains(rows):
    """rows = (kernel name, value) in dispatch order -> {position in the transform: [values]}, whole transforms only."""
    out, pos, names = {}, None, {}
    for name, val in rows:
        if "ntt_pass_kernel" not in name:
            continue
        if ", true, false>" in name:      # CONTIG without global twiddles: the first pass of a whole transform
            pos = 0
        elif pos is None:
            continue
        out.setdefault(pos, []).append(val)
        names[pos] = name.split("(")[0]
        pos += 1
    return out, names


def report(title, unit, per_pos, names, tail):
    print(f"# {title}")
    for pos in sorted(per_pos):
        v = per_pos[pos][-tail:]
        print(f"  pass {pos + 1}  n={len(v):5d}  median {statistics.median(v):10.1f}  mean {statistics.fmean(v):10.1f}  "
              f"min {min(v):10.1f}  max {max(v):10.1f} {unit}  {names[pos]}")


def main():
    kt = sqlite3.connect(sys.argv[1])
    rows = [(n, (e - s) / 1e3) for n, s, e in kt.execute("select name,start,end from kernels order by start")]
    per_pos, names = chains(rows)
    report(f"kernel durations, last 200 transforms of {sys.argv[1]}", "us", per_pos, names, 200)
    for path in sys.argv[2:]:
        db = sqlite3.connect(path)
        cols = [r[1] for r in db.execute("pragma table_info(counters_collection)")]
        order = "dispatch_id" if "dispatch_id" in cols else ("start" if "start" in cols else "rowid")
        for (ctr,) in list(db.execute("select distinct counter_name from counters_collection")):
            q = f"select kernel_name, value from counters_collection where counter_name = ? order by {order}"
            per_pos, names = chains(db.execute(q, (ctr,)))
            report(f"{ctr} per dispatch (raw counter value, KB), {path}, ordered by {order}", "KB", per_pos, names, 10 ** 9)


if __name__ == "__main__":
    main()
