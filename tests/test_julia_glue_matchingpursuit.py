"""Lint of the matchingpursuit Julia glue (wavelets.jl_amd/julia/WaveletsMI355X_matchingpursuit.jl) -- CPU only, the rules
tests/test_julia_glue_modwt_mra.py applies to its file (and the same ccall parser):
  * every `ccall` matches _lib.SIGNATURES (name, return type, arity, each argument type), and the four entry points are bound;
  * every `ccall` sits under `GC.@preserve ... check(`, and every pointer(...) handed to C is in that statement's list;
  * the module includes the file, and the file adds the two forms of Threshold.matchingpursuit and Threshold.findmaxabs on
    ROCVector{T}; both forms assert what the reference asserts.
"""
import os
import re

import test_julia_glue_wpt_batch as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "wavelets.jl_amd", "julia")
GLUE = os.path.join(JL, "WaveletsMI355X_matchingpursuit.jl")
SYMS = {"wl_findmaxabs", "wl_mp_select", "wl_mp_residual", "wl_matchingpursuit_filter"}
_ccalls, _mismatches = B.D._ccalls, B.D._mismatches


def test_module_includes_the_file_and_the_methods_exist():
    main = open(os.path.join(JL, "WaveletsMI355X.jl")).read()
    assert re.search(r'^include\("WaveletsMI355X_matchingpursuit\.jl"\)$', main, re.M)
    assert main.index("using Wavelets.Threshold: Threshold") < main.index('include("WaveletsMI355X_matchingpursuit.jl")')
    src = open(GLUE).read()
    assert re.search(r"^function Threshold\.matchingpursuit\(x::ROCVector\{T\}, wts::AbstractVector\{<:OrthoFilter\}, tol::Real, nmax::Int=-1;$",
                     src, re.M)
    assert re.search(r"^function Threshold\.matchingpursuit\(x::ROCVector\{T\}, f::Function, ft::Function, tol::Real, nmax::Int=-1\) where", src, re.M)
    assert re.search(r"^function Threshold\.findmaxabs\(v::ROCVector\{T\}\) where", src, re.M)
    assert len(re.findall(r"where \{T<:Union\{Float32,Float64\}\}", src)) == 5
    # the reference's assertions, in both forms, and the documented overwrite of x
    assert len(re.findall(r"^    @assert nmax >= -1$", src, re.M)) == 2 and len(re.findall(r"^    @assert tol > 0$", src, re.M)) == 2
    assert "OVERWRITE x with the residual" in src and "`oop` / `N` arguments are not mirrored" in src
    code = re.sub(r"#[^\n]*", "", src)
    assert "GLS" not in code and "Complex" not in code and re.search(r"^    r = x$", code, re.M)
    assert "+ 1" in code.split("function Threshold.findmaxabs")[1].split("end")[0]          # 1-based for the Julia caller


def test_every_ccall_matches_the_abi():
    calls = _ccalls(open(GLUE).read())
    assert {c["sym"] for c in calls} == SYMS and len(calls) == 6
    assert _mismatches(calls) == []


def test_every_ccall_is_checked_and_its_device_pointers_are_gc_preserved():
    src = open(GLUE).read()
    calls = _ccalls(src)
    assert len(re.findall(r"check\(ccall\(", src)) == len(calls)
    for c in calls:
        names = [m.group(1) for a in c["args"] for m in re.finditer(r"pointer\((\w+)\)", a)]
        m = re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", c["prefix"].rstrip())
        assert m, "%s (line %d): ccall outside GC.@preserve ... check(" % (c["sym"], c["line"])
        assert names and set(names) <= set(m.group(1).split()), (c["sym"], c["line"], names)
    main = open(os.path.join(JL, "WaveletsMI355X.jl")).read()
    assert "rc == -4 && throw(DimensionMismatch(msg))" in main and "rc in (-1, -2, -3, -5, -6, -7, -9, -10) && throw(ArgumentError(msg))" in main


def test_what_the_ccalls_pass():
    calls = {}
    for c in _ccalls(open(GLUE).read()):
        calls.setdefault(c["sym"], []).append([" ".join(a.split()) for a in c["args"]])
    assert calls["wl_matchingpursuit_filter"] == [["ctx()", "DT[T]", "pointer(y)", "pointer(x)", "n", "nb", "q", "fl", "Ls", "tol", "nmax", "niter", "nrm",
                                                   "stream()"]]
    assert calls["wl_findmaxabs"] == [["ctx()", "DT[T]", "pointer(v)", "length(v)", "pointer(idx)", "stream()"]]
    # the dense dictionary: spat is as long as y, so the atom's position is its index
    assert calls["wl_mp_select"] == [["ctx()", "DT[T]", "pointer(spat)", "N", "pointer(y)", "pointer(ftr)", "N", "pointer(idx)", "stream()"]]
    res = calls["wl_mp_residual"]
    assert [a[3:8] for a in res] == [["C_NULL", "n", "C_NULL", "0", "C_NULL"], ["pointer(aphi)", "n", "C_NULL", "0", "C_NULL"],
                                     ["pointer(aphi)", "n", "pointer(spat)", "n", "pointer(idx)"]]


def test_lint_is_not_vacuous():
    """a dropped argument, a wrong argument type and a wrong return type are all reported"""
    src = open(GLUE).read()
    good = "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid})"
    assert src.count(good) == 1
    for broken in ("(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid})", "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid})"):
        bad = _mismatches(_ccalls(src.replace(good, broken)))
        assert bad and all(b[0] == "wl_findmaxabs" for b in bad), bad
    bad = _mismatches(_ccalls(src.replace("(:wl_matchingpursuit_filter, LIB), Cint,", "(:wl_matchingpursuit_filter, LIB), Cdouble,")))
    assert bad and {b[0] for b in bad} == {"wl_matchingpursuit_filter"}
