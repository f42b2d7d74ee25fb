#!/usr/bin/env python3
"""One forward of a rocprofv3 kernel trace, kernel by kernel, as a markdown table
(the form of profiles/r6x_resnet18_b400_split_forward_trace.md).

usage: rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/fwd_loop.py ...
       python tools/trace_table.py DIR/**/run_kernel_trace.csv [--last softmax_top1_kernel] [--title T]

A forward is the run of kernels after one launch of the ``--last`` kernel up to
and including the next; the last one of the trace is printed (the replays before
it are the warm-up).  Gap = start of the next kernel minus end of this one.
"""
import argparse
import csv
import re


def short(name: str) -> str:
    m = re.match(r"void idunno::(\w+)<(.*)>\(", name)
    if m:
        return f"{m.group(1)}<{m.group(2)}>"
    m = re.match(r"(?:void )?idunno::(\w+)\(", name)
    if m:
        return m.group(1)
    return name[:60]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--last", default="softmax_top1_kernel", help="substring of the forward's last kernel")
    ap.add_argument("--title", default="one forward, kernel by kernel")
    a = ap.parse_args()
    rows = []
    for r in csv.DictReader(open(a.path)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    ends = [i for i, r in enumerate(rows) if a.last in r[2]]
    if len(ends) < 2:
        raise SystemExit(f"fewer than two launches of a kernel matching {a.last!r} in {a.path}")
    fwd = rows[ends[-2] + 1:ends[-1] + 1]
    print(f"### {a.title}\n")
    print("Gap = start of the next kernel minus end of this one (graph replay, one stream).\n")
    print("| # | kernel | us | gap us |")
    print("|---:|---|---:|---:|")
    for i, (s, e, name) in enumerate(fwd):
        gap = (fwd[i + 1][0] - e) / 1e3 if i + 1 < len(fwd) else float("nan")
        print(f"| {i} | `{short(name)}` | {(e - s) / 1e3:.1f} | {gap:.1f} |")
    tot = sum(e - s for s, e, _ in fwd) / 1e3
    print(f"\nsum of kernel time {tot:.0f} us; span first start -> last end {(fwd[-1][1] - fwd[0][0]) / 1e3:.0f} us")


if __name__ == "__main__":
    main()
