"""Lint of the denoise_batch Julia glue (wavelets.jl_amd/julia/WaveletsMI355X_denoise_batch.jl) -- CPU only, the rules
tests/test_julia_glue.py applies to WaveletsMI355X.jl:
  * every `ccall` matches _lib.SIGNATURES (name, return type, arity, each argument type), and the glue binds the three new
    entry points;
  * every pointer(...) handed to C is kept alive by GC.@preserve;
  * the module includes the file and the file defines denoise_batch (filter and lifting), noisest_batch and mad_batch!.
"""
import os
import re

import test_julia_glue as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "wavelets.jl_amd", "julia")
GLUE = os.path.join(JL, "WaveletsMI355X_denoise_batch.jl")
SYMS = {"wl_mad_batch", "wl_denoise_batch_filter", "wl_denoise_batch_lifting"}


def _ccalls(src):
    src = re.sub(r"#[^\n]*", "", src)
    calls = []
    for m in re.finditer(r"ccall\(", src):
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0)
            j += 1
        parts = G._split_top(src[m.end():j - 1])
        ls = src.rfind("\n", 0, m.start()) + 1
        calls.append({"sym": re.match(r"\(:(\w+),\s*LIB\)", parts[0]).group(1), "ret": parts[1].strip(),
                      "types": [t.strip() for t in G._split_top(parts[2].strip()[1:-1])], "args": parts[3:],
                      "line": src.count("\n", 0, m.start()) + 1, "prefix": src[ls:m.start()]})
    return calls


def _mismatches(calls):
    from wavelets_jl_amd import _lib
    bad = []
    for c in calls:
        if c["sym"] not in _lib.SIGNATURES:
            bad.append((c["sym"], c["line"], "unknown symbol"))
            continue
        restype, argtypes = _lib.SIGNATURES[c["sym"]]
        if G.JL2C.get(c["ret"]) is not restype:
            bad.append((c["sym"], c["line"], "return type " + c["ret"]))
        if not len(c["types"]) == len(argtypes) == len(c["args"]):
            bad.append((c["sym"], c["line"], "arity %d types / %d values / ABI %d" % (len(c["types"]), len(c["args"]), len(argtypes))))
            continue
        for k, (jt, ct) in enumerate(zip(c["types"], argtypes)):
            if G.JL2C.get(jt) is not ct:
                bad.append((c["sym"], c["line"], "argument %d: Julia %s, ABI %s" % (k + 1, jt, ct)))
    return bad


def test_module_includes_the_file():
    assert re.search(r'^include\("WaveletsMI355X_denoise_batch\.jl"\)$', open(os.path.join(JL, "WaveletsMI355X.jl")).read(), re.M)
    src = open(GLUE).read()
    assert len(re.findall(r"^function denoise_batch\(x::ROCArray\{T,N\}, wt::(?:OrthoFilter|GLS)", src, re.M)) == 2
    assert re.search(r"^function noisest_batch\(x::ROCArray\{T,N\}", src, re.M)
    assert re.search(r"^function mad_batch!\(y::ROCMatrix\{T\}\)", src, re.M)


def test_every_ccall_matches_the_abi():
    calls = _ccalls(open(GLUE).read())
    assert {c["sym"] for c in calls} == SYMS
    assert _mismatches(calls) == []


def test_device_pointers_are_gc_preserved():
    for c in _ccalls(open(GLUE).read()):
        names = [m.group(1) for a in c["args"] for m in re.finditer(r"pointer\((\w+)\)", a)]
        assert names, c["sym"]
        m = re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", c["prefix"].rstrip())
        assert m, "%s (line %d): pointer(...) passed to C outside GC.@preserve" % (c["sym"], c["line"])
        assert set(names) <= set(m.group(1).split()), (c["sym"], c["line"], names)
    # y, x and both sigma vectors of the two denoise calls
    by = {c["sym"]: c for c in _ccalls(open(GLUE).read())}
    for s in ("wl_denoise_batch_filter", "wl_denoise_batch_lifting"):
        assert {"y", "x", "sig_in", "sout"} <= set(re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", by[s]["prefix"].rstrip()).group(1).split())


def test_lint_is_not_vacuous():
    """a dropped argument, a wrong argument type and a wrong return type are all reported"""
    src = open(GLUE).read()
    good = "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Cvoid})"
    assert good in src
    for broken in ("(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Cvoid})",
                   "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Float64}, Ptr{Cvoid})"):
        bad = _mismatches(_ccalls(src.replace(good, broken)))
        assert bad and all(b[0] == "wl_mad_batch" for b in bad), bad
    bad = _mismatches(_ccalls(src.replace("(:wl_mad_batch, LIB), Cint,", "(:wl_mad_batch, LIB), Cdouble,")))
    assert [b[0] for b in bad] == ["wl_mad_batch"]
