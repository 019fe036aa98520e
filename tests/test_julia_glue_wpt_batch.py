"""Lint of the wpt_batch Julia glue (wavelets.jl_amd/julia/WaveletsMI355X_wpt_batch.jl) -- CPU only, the rules
tests/test_julia_glue_denoise_batch.py applies to the denoise_batch glue:
  * every `ccall` matches _lib.SIGNATURES (name, return type, arity, each argument type), and the glue binds the two new entry points;
  * every pointer(...) handed to C is kept alive by GC.@preserve;
  * the module includes the file, and the file defines wpt_batch / iwpt_batch / wpt_batch! / iwpt_batch! on ROCMatrix{T} for
    OrthoFilter and GLS with L::Integer and tree::BitVector, and throws the reference's exceptions.
"""
import os
import re

import test_julia_glue_denoise_batch as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "wavelets.jl_amd", "julia")
GLUE = os.path.join(JL, "WaveletsMI355X_wpt_batch.jl")
SYMS = {"wl_wpt_filter_batch", "wl_wpt_lifting_batch"}


def test_module_includes_the_file_and_the_methods_exist():
    assert re.search(r'^include\("WaveletsMI355X_wpt_batch\.jl"\)$', open(os.path.join(JL, "WaveletsMI355X.jl")).read(), re.M)
    src = open(GLUE).read()
    # the in-place forms are generated for both directions ...
    assert re.search(r"^for \(f, fw\) in \(\(:wpt_batch!, true\), \(:iwpt_batch!, false\)\)$", src, re.M)
    assert re.search(r"@eval function \$f\(y::ROCMatrix\{T\}, x::ROCMatrix\{T\}, filter::OrthoFilter,\s*tree::Union\{Integer,BitVector\}", src)
    assert re.search(r"@eval function \$f\(y::ROCMatrix\{T\}, scheme::GLS,\s*tree::Union\{Integer,BitVector\}", src)
    # ... and so are the allocating ones
    assert re.search(r"^for \(f, fb, fw\) in \(\(:wpt_batch, :wpt_batch!, true\), \(:iwpt_batch, :iwpt_batch!, false\)\)$", src, re.M)
    assert re.search(r"@eval function \$f\(x::ROCMatrix\{T\}, filter::OrthoFilter,\s*tree::Union\{Integer,BitVector\}", src)
    assert re.search(r"@eval function \$f\(x::ROCMatrix\{T\}, scheme::GLS,\s*tree::Union\{Integer,BitVector\}", src)
    assert len(re.findall(r"where \{T<:Union\{Float32,Float64\}\}", src)) == 5
    # both forms of the tree argument
    assert re.search(r"^function wpt_batch_tree\(n::Integer, L::Integer\)$", src, re.M)
    assert re.search(r"^function wpt_batch_tree\(n::Integer, tree::BitVector\)$", src, re.M)


def test_the_reference_exceptions():
    src = open(GLUE).read()
    assert len(re.findall(r'size\(x\) == size\(y\) \|\| throw\(DimensionMismatch\("in and out array size must match"\)\)', src)) == 2
    assert re.search(r'pointer\(y\) == pointer\(x\) && throw\(ArgumentError\("in array is out array"\)\)', src)
    assert re.search(r'Util\.isvalidtree\(zeros\(n\), tree\) \|\| throw\(ArgumentError\("invalid tree"\)\)', src)
    assert re.search(r'0 <= L <= Util\.maxtransformlevels\(n\) \|\| throw\(AssertionError\("0 <= L <= maxtransformlevels\(n\)"\)\)', src)
    # the status codes of the library map onto the same exceptions in check() (DimensionMismatch for WL_EDIMS, ArgumentError else)
    main = open(os.path.join(JL, "WaveletsMI355X.jl")).read()
    assert "rc == -4 && throw(DimensionMismatch(msg))" in main and "rc in (-1, -2, -3, -5, -6, -7, -9, -10) && throw(ArgumentError(msg))" in main


def test_every_ccall_matches_the_abi():
    calls = D._ccalls(open(GLUE).read())
    assert {c["sym"] for c in calls} == SYMS and len(calls) == 2
    assert D._mismatches(calls) == []


def test_device_pointers_are_gc_preserved():
    for c in D._ccalls(open(GLUE).read()):
        names = [m.group(1) for a in c["args"] for m in re.finditer(r"pointer\((\w+)\)", a)]
        assert set(names) == {"y", "x", "t"}, (c["sym"], names)
        m = re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", c["prefix"].rstrip())
        assert m, "%s (line %d): pointer(...) passed to C outside GC.@preserve" % (c["sym"], c["line"])
        assert set(names) <= set(m.group(1).split()), (c["sym"], c["line"], names)


def test_lint_is_not_vacuous():
    """a dropped argument, a wrong argument type and a wrong return type are all reported"""
    src = open(GLUE).read()
    good = "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Cint, Ptr{UInt8}, Int64, Cint, Cint, Ptr{Cvoid})"
    assert good in src
    for broken in ("(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Cint, Ptr{UInt8}, Int64, Cint, Cint, Ptr{Cvoid})",
                   "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Float64}, Cint, Ptr{UInt8}, Int64, Cint, Cint, Ptr{Cvoid})"):
        bad = D._mismatches(D._ccalls(src.replace(good, broken)))
        assert bad and all(b[0] == "wl_wpt_filter_batch" for b in bad), bad
    bad = D._mismatches(D._ccalls(src.replace("(:wl_wpt_lifting_batch, LIB), Cint,", "(:wl_wpt_lifting_batch, LIB), Cdouble,")))
    assert [b[0] for b in bad] == ["wl_wpt_lifting_batch"]
