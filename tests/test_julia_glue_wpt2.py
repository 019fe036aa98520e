"""Lint of the wpt2 Julia glue (wavelets.jl_amd/julia/WaveletsMI355X_wpt2.jl) -- CPU only, the rules
tests/test_julia_glue_matchingpursuit.py applies to its file (and the same ccall parser):
  * every `ccall` matches _lib.SIGNATURES (name, return type, arity, each argument type), and both entry points are bound;
  * every `ccall` sits under `GC.@preserve ... check(`, and every pointer(...) handed to C is in that statement's list;
  * the module includes the file, and the file defines plain (not Transforms.-qualified) wpt2 / iwpt2 / wpt2! / iwpt2! on ROCMatrix
    plus maketree2 and isvalidtree2.
"""
import os
import re

import test_julia_glue_wpt_batch as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "wavelets.jl_amd", "julia")
GLUE = os.path.join(JL, "WaveletsMI355X_wpt2.jl")
SYMS = {"wl_wpt2_filter", "wl_wpt2_filter_full"}
_ccalls, _mismatches = B.D._ccalls, B.D._mismatches


def test_module_includes_the_file_and_the_functions_exist():
    main = open(os.path.join(JL, "WaveletsMI355X.jl")).read()
    assert re.search(r'^include\("WaveletsMI355X_wpt2\.jl"\)$', main, re.M)
    src = open(GLUE).read()
    for f in ("wpt2", "iwpt2"):
        assert re.search(r"^%s\(x::ROCMatrix, filter::OrthoFilter, L_or_tree=" % f, src, re.M), f
        assert re.search(r"^%s!\(y::ROCMatrix, x::ROCMatrix, filter::OrthoFilter, L_or_tree=" % f, src, re.M), f
    assert re.search(r"^function maketree2\(n0::Integer, n1::Integer, L::Integer=", src, re.M)
    assert re.search(r"^function isvalidtree2\(x::AbstractMatrix, tree::AbstractVector\)", src, re.M)
    assert len(re.findall(r"where \{T<:Union\{Float32,Float64\}\}", src)) == 2
    code = re.sub(r"#[^\n]*", "", src)
    # the reference has no such methods: nothing is added to its modules; no lifting form and no complex form
    assert "Transforms." not in code and "GLS" not in code and "Complex" not in code
    assert len(re.findall(r'size\(x\) == size\(y\) \|\| throw\(DimensionMismatch\("in and out array size must match"\)\)', code)) == 2
    assert 'isvalidtree2(x, tree) || throw(ArgumentError("invalid tree"))' in code


def test_every_ccall_matches_the_abi():
    calls = _ccalls(open(GLUE).read())
    assert {c["sym"] for c in calls} == SYMS and len(calls) == 2
    assert _mismatches(calls) == []


def test_every_ccall_is_checked_and_its_device_pointers_are_gc_preserved():
    src = open(GLUE).read()
    calls = _ccalls(src)
    assert len(re.findall(r"check\(ccall\(", src)) == len(calls)
    for c in calls:
        names = [m.group(1) for a in c["args"] for m in re.finditer(r"pointer\((\w+)\)", a)]
        m = re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", c["prefix"].rstrip())
        assert m, "%s (line %d): ccall outside GC.@preserve ... check(" % (c["sym"], c["line"])
        assert set(names) == {"y", "x"} and set(names) <= set(m.group(1).split()), (c["sym"], c["line"], names)


def test_what_the_ccalls_pass():
    calls = {c["sym"]: [" ".join(a.split()) for a in c["args"]] for c in _ccalls(open(GLUE).read())}
    assert calls["wl_wpt2_filter_full"] == ["ctx()", "DT[T]", "pointer(y)", "pointer(x)", "dims", "filter.qmf", "length(filter.qmf)", "L", "fw",
                                            "stream()"]
    assert calls["wl_wpt2_filter"] == ["ctx()", "DT[T]", "pointer(y)", "pointer(x)", "dims", "filter.qmf", "length(filter.qmf)", "t", "length(t)",
                                       "fw", "stream()"]
    assert "dims = Int64[size(x, 1), size(x, 2)]" in open(GLUE).read()


def test_lint_is_not_vacuous():
    """a dropped argument, a wrong argument type and a wrong return type are all reported"""
    src = open(GLUE).read()
    good = "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Cint, Cint, Cint, Ptr{Cvoid})"
    assert src.count(good) == 1
    for broken in ("(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Cint, Cint, Ptr{Cvoid})",
                   "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Cint, Cint, Cint, Ptr{Cvoid})"):
        bad = _mismatches(_ccalls(src.replace(good, broken)))
        assert bad and all(b[0] == "wl_wpt2_filter_full" for b in bad), bad
    bad = _mismatches(_ccalls(src.replace("(:wl_wpt2_filter, LIB), Cint,", "(:wl_wpt2_filter, LIB), Cdouble,")))
    assert bad and {b[0] for b in bad} == {"wl_wpt2_filter"}
