"""Checks a `rocprofv3 --kernel-trace --stats` run of tests/test_attn_wo_matrix_gpu.py (without the LDS-poison test) against the
helpers' mirror of launch_attn_wo_g: every attn_wo_kernel instantiation that launched, with its call count, next to what the
matrix predicts (2 calls per case without PICK -- in place and out of place --, 1 per PICK case).  Given the run's rocpd database
(`<name>_results.db`, rocprofv3's default output) it also walks the dispatches in order, case by case (the test's parameter order),
and checks each one's instantiation and grid (column groups x row pairs) against the case's.

    python tools/awo_trace_check.py <..._kernel_stats.csv | ..._results.db> [summary.txt]"""
import csv
import re
import sys
from collections import Counter
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from attn_wo_helpers import CASES, instance  # noqa: E402

DEMANGLED = re.compile(r"attn_wo_kernel<(\d+), (\d+), (true|false), (true|false), (true|false), (\d+)>")
MANGLED = re.compile(r"attn_wo_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])ELi(\d+)EE")


def parse(name: str):
    m = DEMANGLED.search(name) or MANGLED.search(name)
    if not m:
        return None
    G, T, two, w8, pick, nbf = m.groups()
    b = lambda x: x in ("true", "1")  # noqa: E731
    return (int(G), int(T), b(two), b(w8), b(pick), int(nbf))


def dispatches(db: Path) -> list:
    import sqlite3

    con = sqlite3.connect(str(db))
    rows = con.execute("select name, grid_x, grid_y, workgroup_x from kernels order by start").fetchall()
    return [(parse(n), gx, gy, wx) for n, gx, gy, wx in rows if parse(n) is not None]


def walk(disp: list) -> list:
    """Per case of the test order (non-PICK cases, then PICK cases), the dispatches it must have made, against the trace."""
    order = [c for c in CASES if not c.pick] + [c for c in CASES if c.pick]
    bad, i = [], 0
    for c in order:
        N = c.Hq * 64
        T = 3 if c.M > 16 else 1
        want = (instance(c), ((N + 15) // 16 + T - 1) // T, (c.M + 1) // 2)
        for _ in range(1 if c.pick else 2):
            got = (disp[i][0], disp[i][1] // disp[i][3], disp[i][2]) if i < len(disp) else None
            if got != want:  # rocpd grid sizes are in work-items: grid_x / workgroup_x = column groups
                bad.append(f"{c.id}: dispatch {i}: trace {got}, predicted {want}")
            i += 1
    if i != len(disp):
        bad.append(f"{len(disp)} attn_wo dispatches in the trace, {i} predicted")
    return bad


def main():
    stats, out = Path(sys.argv[1]), (Path(sys.argv[2]) if len(sys.argv) > 2 else None)
    seen, bad = Counter(), None
    if stats.suffix == ".db":
        disp = dispatches(stats)
        for k, *_ in disp:
            seen[k] += 1
        bad = walk(disp)
    else:
        with stats.open() as f:
            for row in csv.DictReader(f):
                k = parse(row.get("Name", ""))
                if k is not None:
                    seen[k] += int(row["Calls"])
    want = Counter()
    for c in CASES:
        want[instance(c)] += 1 if c.pick else 2
    lines = [f"attn_wo_kernel launches in {stats.name}: {len(seen)} instantiations, {sum(seen.values())} calls; "
             f"mirror: {len(want)} instantiations, {sum(want.values())} calls",
             "G T TWO   W8    PICK  NBF  calls  predicted"]
    for k in sorted(set(seen) | set(want)):
        flag = "" if seen[k] == want[k] else "   <-- MISMATCH"
        lines.append(f"{k[0]} {k[1]} {str(k[2]):5} {str(k[3]):5} {str(k[4]):5} {k[5]:3}  {seen[k]:5}  {want[k]:9}{flag}")
    ok = seen == want
    if bad is not None:
        lines.append(f"dispatch by dispatch, in the test's case order: {len(bad)} mismatches (form and grid of every case)")
        lines += bad[:50]
        ok = ok and not bad
    lines.append("every case launched the instantiation the mirror predicted" if ok else "MISMATCH between the trace and the mirror")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        out.write_text(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
