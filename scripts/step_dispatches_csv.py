"""Per-step dispatch lists from rocprofv3 kernel-trace CSVs (``--kernel-trace --output-format csv``),
for comparing the engine step of two builds.

A step is what runs from one ``k_set_step_params`` to the next; only the project's kernels (``k_*``)
are listed.  Prints, per trace, the number of distinct steady-state dispatch sequences and their
lengths, then whether the first two traces run the same sequence and which kernels any further trace
adds; ``--md`` also writes one step of each trace as a table.

    python scripts/step_dispatches_csv.py parent=a/run_kernel_trace.csv this=b/run_kernel_trace.csv [--md out.md]
"""
from __future__ import annotations

import argparse
import collections
import csv


def steps(path: str) -> list:
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"].split("(")[0] for r in rows]
    starts = [i for i, n in enumerate(names) if n == "k_set_step_params"]
    return [[(names[i], int(rows[i]["Grid_Size_X"]) // max(1, int(rows[i]["Workgroup_Size_X"])),
              (int(rows[i]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"])) / 1000.0)
             for i in range(a, b) if names[i].startswith("k_")] for a, b in zip(starts, starts[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("traces", nargs="+", help="tag=path of a kernel-trace CSV")
    ap.add_argument("--skip", type=int, default=5, help="warm-up steps left out of the comparison")
    ap.add_argument("--step", type=int, default=15, help="the step --md prints")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    res = {}
    for spec in a.traces:
        tag, path = spec.split("=", 1)
        st = steps(path)
        seqs = collections.Counter(tuple(n for n, _, _ in s) for s in st[a.skip:])
        res[tag] = (st, seqs)
        print(f"{tag}: {len(st)} steps, {len(seqs)} distinct steady-state sequence(s), dispatches per step "
              f"{sorted(len(k) for k in seqs)}")
    tags = list(res)
    if len(tags) >= 2:
        print(f"{tags[0]} and {tags[1]} run the same sequence: {set(res[tags[0]][1]) == set(res[tags[1]][1])}")
        base = next(iter(res[tags[0]][1]))
        for t in tags[2:]:
            other = next(iter(res[t][1]))
            print(f"{t} adds: {sorted({n for n in other if other.count(n) != base.count(n)})}")
    if a.md:
        with open(a.md, "w") as f:
            for tag in tags:
                st = res[tag][0][a.step]
                f.write(f"\n### {tag}: step {a.step} of the trace, {len(st)} dispatches\n\n"
                        "| # | kernel | workgroups | us |\n|---:|---|---:|---:|\n")
                for i, (n, g, us) in enumerate(st):
                    f.write(f"| {i + 1} | `{n}` | {g} | {us:.1f} |\n")


if __name__ == "__main__":
    main()
