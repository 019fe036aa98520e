#!/usr/bin/env python3
"""Which template instances of the library's kernels does the instance case table (tests/instance_cases.py) launch?

W.last_kernel() reports a kernel's name; the instance behind it (element type, tap count, waves, request distance, ...) is chosen
inside the launchers.  This tool measures the choice instead of restating it:

    instance_trace.py run                      run every row of the table once: no pytest, no comparison, one process.  Meant to
                                               run under `rocprofv3 --kernel-trace --stats` (and nothing else), through tools/rp.sh:
                                                   tools/rp.sh OUT trace "--kernel-trace --stats" python tools/instance_trace.py run
    instance_trace.py read CSV [CSV ...]       reduce the *_kernel_stats.csv of such runs to (family, template arguments), write
                                               tests/instances_reached.json (family -> sorted argument strings) and print the
                                               shipped instances that were not reached (--json PATH: write elsewhere)
    instance_trace.py shipped                  print the shipped instances, per family

Shipped instances are the kernel symbols of the gfx950 code objects in libwavelets_mi355x.so (tools/isa_check.py's
extract_code_objects and llvm-readelf's symbol listing, raw and demangled).  Both sides go through normalise(), so namespaces, `(anonymous namespace)` and the
spelling of integers cannot make two names of one instance.
"""
import csv
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "wavelets.jl_amd", "libwavelets_mi355x.so")
REACHED = os.path.join(ROOT, "tests", "instances_reached.json")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import isa_check  # noqa: E402


def _split_args(s):
    """top-level commas of a template argument list"""
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    return out


_re_cast = re.compile(r"\((?:unsigned |signed )?(?:int|long|short|char|bool|unsigned)\)")
_re_int = re.compile(r"^(-?\d+)(?:[uU]?[lL]{0,2}|[lL]{1,2}[uU])$")


def _norm_arg(a):
    a = a.strip().replace("(anonymous namespace)::", "")
    a = re.sub(r"\b(?:\w+::)+", "", a)                      # namespaces
    a = _re_cast.sub("", a).strip()
    if a == "true":
        return "1"
    if a == "false":
        return "0"
    g = _re_int.match(a)
    if g:
        return str(int(g.group(1)))
    if "<" in a:                                            # a templated type argument: normalise what it holds
        head, rest = a.split("<", 1)
        return "%s<%s>" % (head.strip(), ", ".join(_norm_arg(x) for x in _split_args(rest[:rest.rindex(">")])))
    return a


def normalise(demangled):
    """'void wl::k_inv2d_lds_long<float, 10, 1, 2, 0, 2>(wl::InvLongArgs<float, 10>)' -> ('k_inv2d_lds_long', 'float, 10, 1, 2, 0, 2');
    None for a name that is no kernel of the library (its family does not start with k_)"""
    s = demangled.strip()
    if s.endswith(" [clone .kd]"):
        s = s[:-len(" [clone .kd]")]
    if s.endswith(".kd"):
        s = s[:-3]
    if s.startswith("void "):
        s = s[5:]
    s = s.replace("(anonymous namespace)::", "")
    i = 0                                                   # the function's own name ends at the first '<' or '('
    while i < len(s) and s[i] not in "<(":
        i += 1
    family = s[:i].split("::")[-1].strip()
    if not family.startswith("k_"):
        return None
    args = ""
    if i < len(s) and s[i] == "<":
        depth, j = 0, i
        while j < len(s):
            if s[j] in "<(":
                depth += 1
            elif s[j] in ">)":
                depth -= 1
                if depth == 0:
                    break
            j += 1
        args = ", ".join(_norm_arg(a) for a in _split_args(s[i + 1:j]))
    return family, args


def _tool(name):
    return os.path.join(isa_check.LLVM, name)


def shipped(lib=LIB):
    """-> {family: set of argument strings} of every kernel in the library's gfx950 code objects"""
    out = {}
    with tempfile.TemporaryDirectory(prefix="wl_inst_") as tmp:
        for co in isa_check.extract_code_objects(lib, tmp):
            raw, dem = (_symbols(co, d) for d in (False, True))
            kernels = {n[:-3] for n in raw.values() if n.endswith(".kd")}      # a kernel descriptor: one per __global__ function
            for num, name in raw.items():
                if name in kernels:
                    n = normalise(dem[num])
                    if n is not None:
                        out.setdefault(n[0], set()).add(n[1])
    return out


def _symbols(co, demangle):
    """-> {symbol number: name} of a code object's symbol table (llvm-readelf; the demangled listing keeps the numbers)"""
    cmd = [_tool("llvm-readelf"), "--symbols", "--wide", co] + (["--demangle"] if demangle else [])
    out = {}
    for line in subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.splitlines():
        f = line.split(None, 7)
        if len(f) == 8 and f[0].endswith(":") and f[0][:-1].isdigit():
            out[int(f[0][:-1])] = f[7].strip()
    return out


def read_stats(paths):
    """-> {family: set of argument strings} of the kernels named in rocprofv3's *_kernel_stats.csv files"""
    out = {}
    for p in paths:
        with open(p, newline="") as f:
            for row in csv.DictReader(f):
                n = normalise(row["Name"])
                if n is not None:
                    out.setdefault(n[0], set()).add(n[1])
    return out


def _table():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import instance_cases
    return instance_cases


def run():
    import torch
    IC = _table()
    import oracle                   # (the inputs of a few rows are built with it; nothing is compared here)
    import wavelets_jl_amd as W
    oracle.build()
    W._lib.load()
    n = 0
    for fam, rows in IC.FAMILIES.items():
        for row in rows:
            IC.run_row(W, oracle, row, compare=False)
            n += 1
    torch.cuda.synchronize()
    print("instance_trace: ran %d rows of %d families" % (n, len(IC.FAMILIES)))


def unreached(ship, reach, exempt=()):
    return sorted((f, a) for f, s in ship.items() for a in s if a not in reach.get(f, ()) and (f, a) not in exempt)


def main(argv):
    if len(argv) >= 2 and argv[1] == "run":
        run()
        return 0
    if len(argv) >= 2 and argv[1] == "shipped":
        ship = shipped()
        for f in sorted(ship):
            print("%-28s %4d  %s" % (f, len(ship[f]), " | ".join(sorted(ship[f]))))
        print("%d instances under %d names" % (sum(len(s) for s in ship.values()), len(ship)))
        return 0
    if len(argv) >= 3 and argv[1] == "read":
        args = argv[2:]
        dest = REACHED
        if "--json" in args:
            k = args.index("--json")
            dest = args[k + 1]
            del args[k:k + 2]
        reach = read_stats(args)
        with open(dest, "w") as f:
            json.dump({fam: sorted(reach[fam]) for fam in sorted(reach)}, f, separators=(",", ":"))
            f.write("\n")
        ship = shipped()
        exempt = set(_table().EXEMPT)
        miss = unreached(ship, reach, exempt)
        stale = sorted((f, a) for f, s in reach.items() for a in s if a not in ship.get(f, ()))
        print("| family | shipped | reached | exempt |\n|---|---|---|---|")
        for fam in sorted(ship):
            print("| `%s` | %d | %d | %d |" % (fam, len(ship[fam]), len(reach.get(fam, set()) & ship[fam]),
                                              sum(1 for e in exempt if e[0] == fam)))
        print("\n%d shipped, %d reached, %d exempt, %d unreached" % (sum(len(s) for s in ship.values()),
              sum(len(reach.get(f, set()) & s) for f, s in ship.items()), len(exempt), len(miss)))
        for fam, a in miss:
            print("unreached: %s<%s>" % (fam, a))
        for fam, a in stale:
            print("traced but not shipped: %s<%s>" % (fam, a))
        return 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv))
