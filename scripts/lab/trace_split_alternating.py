#!/usr/bin/env python3
"""Lab: one kernel, two shapes launched in turn (the residual producer: o_proj, down_proj, o_proj, ... through the layers of a decode step) --
split its launches in a rocprofv3 kernel trace (rocpd sqlite `*_results.db`) by their position in start order and print count, mean, median,
min and max of each half in us.  rocprof_summary.py only splits by a gap in the durations, which a few slow outliers take.
    python scripts/lab/trace_split_alternating.py trace_results.db "gemv_mfma_kernel<TBF16, 5, false, 1, true, 1, true>" [out.txt]"""
import sqlite3
import statistics
import sys


def main(db, fragment, out=None):
    c = sqlite3.connect(db)
    names = [r[0] for r in c.execute("select distinct name from kernels") if fragment in r[0]]
    assert len(names) == 1, f"{fragment!r} matches {names}"
    d = [r[0] / 1e3 for r in c.execute("select end-start from kernels where name = ? order by start", (names[0],))]
    lines = [f"# {names[0][:120]}: {len(d)} launches in start order, split by position (even / odd)"]
    for tag, part in (("even (first, third, ...)", d[0::2]), ("odd (second, fourth, ...)", d[1::2])):
        lines.append(f"{tag:28s} {len(part):7d} launches  mean {statistics.fmean(part):7.2f}  median {statistics.median(part):7.2f}  "
                     f"min {min(part):7.2f}  max {max(part):7.2f} us")
    text = "\n".join(lines) + "\n"
    if out:
        open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
