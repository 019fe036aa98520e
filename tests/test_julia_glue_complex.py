"""Lint of the complex Julia glue (wavelets.jl_amd/julia/WaveletsMI355X_complex.jl) -- CPU only, the rules
tests/test_julia_glue_denoise_batch.py applies to its file:
  * every `ccall` matches _lib.SIGNATURES (name, return type, arity, each argument type), and the glue binds the four complex
    transform entry points;
  * every pointer(...) handed to C is kept alive by GC.@preserve;
  * the module includes the file and the file defines the _dwt! methods (filter and GLS, N = 1..3) and the _wpt! methods
    (filter and GLS; tree and depth forms) for Complex{Float32} / Complex{Float64} device arrays.
"""
import os
import re

import test_julia_glue_denoise_batch as D

JL = D.JL
GLUE = os.path.join(JL, "WaveletsMI355X_complex.jl")
SYMS = {"wl_dwt_filter_complex", "wl_dwt_lifting_complex", "wl_wpt_filter_complex", "wl_wpt_lifting_complex"}
ARRAYS = (r"ROCVector\{Complex\{T\}\}", r"ROCMatrix\{Complex\{T\}\}", r"ROCArray\{Complex\{T\},3\}")


def test_module_includes_the_file():
    assert re.search(r'^include\("WaveletsMI355X_complex\.jl"\)$', open(os.path.join(JL, "WaveletsMI355X.jl")).read(), re.M)


def test_file_defines_the_methods():
    src = open(GLUE).read()
    assert re.search(r"^const CplxT = Union\{Float32,Float64\}$", src, re.M)
    for a in ARRAYS:
        assert re.search(r"^function Transforms\._dwt!\(y::%s, x::%s, filter::OrthoFilter, L::Integer, fw::Bool\) where \{T<:CplxT\}$" % (a, a),
                         src, re.M), a
        assert re.search(r"^function Transforms\._dwt!\(y::%s, scheme::GLS, L::Integer, fw::Bool\) where \{T<:CplxT\}$" % a, src, re.M), a
    v = ARRAYS[0]
    assert re.search(r"^function Transforms\._wpt!\(y::%s, x::%s, filter::OrthoFilter, tree::BitVector, fw::Bool\) where \{T<:CplxT\}$" % (v, v),
                     src, re.M)
    assert re.search(r"^function Transforms\._wpt!\(y::%s, scheme::GLS, tree::BitVector, fw::Bool\) where \{T<:CplxT\}$" % v, src, re.M)
    # the depth forms: wpt! / iwpt! (filter, GLS) and wpt / iwpt
    assert re.search(r"@eval function Transforms\.\$f\(y::%s, x::%s, filter::OrthoFilter,\s*L::Integer=" % (v, v), src)
    assert re.search(r"@eval function Transforms\.\$f\(y::%s, scheme::GLS, L::Integer=" % v, src)
    assert re.search(r"@eval function Transforms\.\$f\(x::%s, filter::OrthoFilter, L::Integer=" % v, src)
    assert re.search(r"@eval function Transforms\.\$f\(x::%s, scheme::GLS, L::Integer=" % v, src)


def test_every_ccall_matches_the_abi():
    calls = D._ccalls(open(GLUE).read())
    assert {c["sym"] for c in calls} == SYMS
    assert len(calls) >= 7
    assert D._mismatches(calls) == []


def test_device_pointers_are_gc_preserved():
    for c in D._ccalls(open(GLUE).read()):
        names = [m.group(1) for a in c["args"] for m in re.finditer(r"pointer\((\w+)\)", a)]
        assert names, c["sym"]
        m = re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", c["prefix"].rstrip())
        assert m, "%s (line %d): pointer(...) passed to C outside GC.@preserve" % (c["sym"], c["line"])
        assert set(names) <= set(m.group(1).split()), (c["sym"], c["line"], names)


def test_lint_is_not_vacuous():
    """a dropped argument and a wrong argument type are reported"""
    src = open(GLUE).read()
    good = "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Int64, Ptr{Float64}, Cint, Cint, Cint, Ptr{Cvoid})"
    assert good in src
    for broken in ("(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Ptr{Float64}, Cint, Cint, Cint, Ptr{Cvoid})",
                   "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Cint, Ptr{Float64}, Cint, Cint, Cint, Ptr{Cvoid})"):
        bad = D._mismatches(D._ccalls(src.replace(good, broken)))
        assert bad and all(b[0] == "wl_dwt_filter_complex" for b in bad), bad
