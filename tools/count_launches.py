"""Launches per call from a kernel trace of `tools/time_batch.py launches`:

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/time_batch.py launches > calls.txt
    python tools/count_launches.py <dir> calls.txt [--all]

The traced script separates its calls by fills of a marker tensor; the library's kernels (namespace wl) dispatched between
fill k and fill k + 1 are the launches of call k.  Markdown rows: call, launches, kernels in dispatch order.  --all counts every
kernel between the fills (the callers around the hot path live outside namespace wl, and a host loop adds torch's own kernels),
runs of one kernel folded to `name x count`.  --instances keeps each launch's template arguments, grid size and workgroup size
(`k_fwd2d_tile<float, 8, 2> 4096x1x1/256x1x1`): two builds that dispatch alike give identical tables (tools/dispatch_cases.py).
"""
import csv
import glob
import os
import re
import sys


def _geometry(r):
    return "x".join(r.get("Grid_Size_" + a, "?") for a in "XYZ") + "/" + "x".join(r.get("Workgroup_Size_" + a, "?") for a in "XYZ")


def main(trace_dir, calls_txt, every=False, instances=False):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under " + trace_dir)
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], _geometry(r)))
    rows.sort()
    labels = [m.group(2) for m in (re.match(r"call (\d+): (.*)", l) for l in open(calls_txt)) if m]
    fills = [i for i, (_, name, _g) in enumerate(rows) if "FillFunctor" in name]
    fills = fills[-(len(labels) + 1):]                       # (the marker tensor's own zero fill comes first)
    if len(fills) != len(labels) + 1:
        sys.exit("found %d marker fills for %d calls" % (len(fills), len(labels)))
    print("| call | launches | kernels |")
    print("|---|---|---|")
    for k, label in enumerate(labels):
        mine = [(n, g) for _, n, g in rows[fills[k] + 1:fills[k + 1]] if every or "wl::" in n]
        names = [re.sub(r"^void ", "", re.sub(r"\(.*$", "", n.replace("(anonymous namespace)::", ""))) for n, _ in mine]
        short = [re.sub(r"<.*$", "", n.split("wl::")[-1]) for n in names]
        if instances:        # (the parameter list is cut at the first parenthesis: casts inside template arguments do not occur in this library)
            short = [n.replace("wl::", "") + " " + g for n, (_, g) in zip(names, mine)]
        if every:
            folded = []
            for n in short:
                if folded and folded[-1][0] == n:
                    folded[-1][1] += 1
                else:
                    folded.append([n, 1])
            short = [n if c == 1 else "%s x %d" % (n, c) for n, c in folded]
        print("| %s | %d | %s |" % (label, len(names), ", ".join(short)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], "--all" in sys.argv[3:], "--instances" in sys.argv[3:])
