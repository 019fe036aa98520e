"""Lint of the threshold_batch! Julia glue (wavelets.jl_amd/julia/WaveletsMI355X_threshold_batch.jl) -- CPU only, the rules
tests/test_julia_glue_bestbasis_batch.py applies to its glue (and the ccall parser of tests/test_julia_glue_denoise_batch.py):
  * every `ccall` matches _lib.SIGNATURES (name, return type, arity, each argument type), and the glue binds the two new entry points;
  * every pointer(...) handed to C is kept alive by GC.@preserve;
  * the module includes the file, and the file defines threshold_batch! on ROCArray{T,N} with one method per threshold type.
"""
import os
import re

import test_julia_glue_denoise_batch as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "wavelets.jl_amd", "julia")
GLUE = os.path.join(JL, "WaveletsMI355X_threshold_batch.jl")
SYMS = {"wl_threshold_batch", "wl_threshold_biggest_batch"}
_ccalls, _mismatches = D._ccalls, D._mismatches


def test_module_includes_the_file_and_the_methods_exist():
    main = open(os.path.join(JL, "WaveletsMI355X.jl")).read()
    assert re.search(r'^include\("WaveletsMI355X_threshold_batch\.jl"\)$', main, re.M)
    # behind the single threshold!, whose THCODE / t_is_f64 / threshold-type imports it uses
    assert main.index("const THCODE") < main.index('include("WaveletsMI355X_threshold_batch.jl")')
    src = open(GLUE).read()
    assert re.search(r"^for TH in \(:HardTH, :SoftTH, :SemiSoftTH, :SteinTH\)$", src, re.M)
    assert re.search(r"@eval function threshold_batch!\(x::ROCArray\{T,N\}, ::\$TH, t::Real\)", src)
    assert re.search(r"@eval function threshold_batch!\(x::ROCArray\{T,N\}, ::\$TH, t::ROCVector\{Float64\}\)", src)
    assert re.search(r"^for TH in \(:PosTH, :NegTH\)$", src, re.M)
    assert re.search(r"@eval function threshold_batch!\(x::ROCArray\{T,N\}, ::\$TH\) where", src)
    assert re.search(r"^function threshold_batch!\(x::ROCArray\{T,N\}, ::BiggestTH, m::Integer\)", src, re.M)
    assert re.search(r"^function threshold_batch!\(x::ROCArray\{T,N\}, ::BiggestTH, m::ROCVector\{Int64\}\)", src, re.M)
    assert len(re.findall(r"where \{T<:Union\{Float32,Float64\},N\}", src)) == 5


def test_the_reference_assertions_on_host_numbers_only():
    src = open(GLUE).read()
    assert len(re.findall(r't >= 0 \|\| throw\(AssertionError\("t >= 0"\)\)', src)) == 1
    assert len(re.findall(r'm >= 0 \|\| throw\(AssertionError\("m >= 0"\)\)', src)) == 1
    assert len(re.findall(r"length\((?:t|m)\) == nb \|\| throw\(DimensionMismatch", src)) == 2


def test_every_ccall_matches_the_abi():
    calls = _ccalls(open(GLUE).read())
    assert {c["sym"] for c in calls} == SYMS and len(calls) == 5
    assert _mismatches(calls) == []


def test_device_pointers_are_gc_preserved():
    seen = []
    for c in _ccalls(open(GLUE).read()):
        names = [m.group(1) for a in c["args"] for m in re.finditer(r"pointer\((\w+)\)", a)]
        assert "x" in names, c["sym"]
        m = re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", c["prefix"].rstrip())
        assert m, "%s (line %d): pointer(...) passed to C outside GC.@preserve" % (c["sym"], c["line"])
        assert set(names) == set(m.group(1).split()), (c["sym"], c["line"], names)
        seen.append(tuple(sorted(names)))
    assert sorted(seen) == [("m", "x"), ("t", "x"), ("x",), ("x",), ("x",)]


def test_lint_is_not_vacuous():
    """a dropped argument, a wrong argument type and a wrong return type are all reported"""
    src = open(GLUE).read()
    good = "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid})"
    assert src.count(good) == 2
    for broken in ("(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid})",
                   "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid})"):
        bad = _mismatches(_ccalls(src.replace(good, broken)))
        assert bad and all(b[0] == "wl_threshold_biggest_batch" for b in bad), bad
    bad = _mismatches(_ccalls(src.replace("(:wl_threshold_batch, LIB), Cint,", "(:wl_threshold_batch, LIB), Cdouble,")))
    assert bad and {b[0] for b in bad} == {"wl_threshold_batch"}
