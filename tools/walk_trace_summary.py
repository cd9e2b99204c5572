#!/usr/bin/env python3
"""Per-call kernel times of vx_grid_walk_field from a rocprofv3 rocpd sqlite output of tools/walk_bench.py
(`rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/walk_bench.py 1024 5`): the dispatches in start order, cut
into calls at every k_walk_stand; per group of calls with the same workgroup count, goal count and sweep count the medians of
the kernels' sums, and of the time from the first kernel's start to the last one's end.
Usage: tools/walk_trace_summary.py DIR/NAME_results.db [out.txt]"""
import sqlite3
import sys

import numpy as np


def main():
    db = sqlite3.connect(sys.argv[1])
    tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if "kernel_dispatch" in t][0]
    ks = [t for t in tabs if "kernel_symbol" in t][0]
    rows = db.execute(f"select s.kernel_name, d.start, d.end, d.grid_size_x from {kd} d join {ks} s on d.kernel_id = s.id "
                      f"where s.kernel_name like '%k_walk_%' order by d.start").fetchall()
    calls = []
    for name, start, end, grid in rows:
        kind = next(k for k in ("stand", "seed", "relax", "finish") if "k_walk_" + k in name)
        if kind == "stand":
            calls.append({"tiles": grid // 256, "seed_grid": 0, "first": start, "stand": 0, "seed": 0, "relax": 0, "finish": 0, "sweeps": 0, "busy": 0})
        c = calls[-1]
        c[kind] += end - start
        c["last"] = end
        if kind == "seed":
            c["seed_grid"] = grid // 256
        if kind == "relax":
            c["sweeps"] += 1
            c["busy"] += 1 if end - start > 6000 else 0
    groups, order = {}, []
    for c in calls:
        key = (c["tiles"], c["seed_grid"], c["sweeps"])
        if key not in groups:
            order.append(key)
        groups.setdefault(key, []).append(c)
    lines = ["%8s %10s %7s %6s | %10s %9s %11s %11s | %12s %11s   (medians, microseconds)" %
             ("tiles", "seed wgs", "sweeps", "calls", "stand", "seed", "relax sum", "finish", "kernels sum", "first..last")]
    for key in order:
        g = groups[key]
        med = lambda f: float(np.median([f(c) for c in g])) / 1e3
        lines.append("%8d %10d %7d %6d | %10.1f %9.1f %11.1f %11.1f | %12.1f %11.1f" %
                     (key[0], key[1], key[2], len(g), med(lambda c: c["stand"]), med(lambda c: c["seed"]), med(lambda c: c["relax"]), med(lambda c: c["finish"]),
                      med(lambda c: c["stand"] + c["seed"] + c["relax"] + c["finish"]), med(lambda c: c["last"] - c["first"])))
        lines.append("%41s relax launches longer than 6 us: %d of %d" % ("", int(np.median([c["busy"] for c in g])), key[2]))
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
