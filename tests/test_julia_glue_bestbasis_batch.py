"""Lint of the bestbasistree_batch Julia glue (wavelets.jl_amd/julia/WaveletsMI355X_bestbasis_batch.jl) -- CPU only, the rules
tests/test_julia_glue_wpt_batch.py applies to the wpt_batch glue (and its ccall parser):
  * every `ccall` matches _lib.SIGNATURES (name, return type, arity, each argument type), and the glue binds the two new entry points;
  * every pointer(...) handed to C is kept alive by GC.@preserve;
  * the module includes the file, and the file defines bestbasistree_batch on ROCMatrix{T} for OrthoFilter with L::Integer and
    tree::BitVector, and wpt_batch / iwpt_batch / wpt_batch! / iwpt_batch! taking trees::ROCMatrix{UInt8}.
"""
import os
import re

import test_julia_glue_wpt_batch as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "wavelets.jl_amd", "julia")
GLUE = os.path.join(JL, "WaveletsMI355X_bestbasis_batch.jl")
SYMS = {"wl_bestbasistree_filter_batch", "wl_wpt_filter_batch_trees"}
_ccalls, _mismatches = B.D._ccalls, B.D._mismatches


def test_module_includes_the_file_and_the_methods_exist():
    main = open(os.path.join(JL, "WaveletsMI355X.jl")).read()
    assert re.search(r'^include\("WaveletsMI355X_bestbasis_batch\.jl"\)$', main, re.M)
    # after the files whose helpers it uses (entcode, wpt_batch_tree)
    pos = {f: main.index('include("WaveletsMI355X_%s.jl")' % f) for f in ("bestbasis", "wpt_batch", "bestbasis_batch")}
    assert pos["bestbasis"] < pos["bestbasis_batch"] and pos["wpt_batch"] < pos["bestbasis_batch"]
    src = open(GLUE).read()
    assert re.search(r"^function bestbasistree_batch\(x::ROCMatrix\{T\}, wt::OrthoFilter, tree::Union\{Integer,BitVector\}", src, re.M)
    assert re.search(r"et::Entropy=ShannonEntropy\(\)\) where \{T<:Union\{Float32,Float64\}\}", src)
    assert re.search(r"trees = ROCMatrix\{UInt8\}\(undef, ntree, size\(x, 2\)\)", src) and re.search(r"^    return trees$", src, re.M)
    assert re.search(r"^for \(f, fw\) in \(\(:wpt_batch!, true\), \(:iwpt_batch!, false\)\)$", src, re.M)
    assert re.search(r"@eval function \$f\(y::ROCMatrix\{T\}, x::ROCMatrix\{T\}, filter::OrthoFilter, trees::ROCMatrix\{UInt8\}", src)
    assert re.search(r"^for \(f, fb\) in \(\(:wpt_batch, :wpt_batch!\), \(:iwpt_batch, :iwpt_batch!\)\)$", src, re.M)
    assert re.search(r"@eval function \$f\(x::ROCMatrix\{T\}, filter::OrthoFilter, trees::ROCMatrix\{UInt8\}", src)
    assert len(re.findall(r"where \{T<:Union\{Float32,Float64\}\}", src)) == 3
    # no lifting form: per-unit trees and the search are defined for filters only
    assert "GLS" not in re.sub(r"#[^\n]*", "", src)


def test_the_exceptions():
    src = open(GLUE).read()
    assert re.search(r'size\(x\) == size\(y\) \|\| throw\(DimensionMismatch\("in and out array size must match"\)\)', src)
    assert re.search(r'pointer\(y\) == pointer\(x\) && throw\(ArgumentError\("in array is out array"\)\)', src)
    assert re.search(r'0 <= L <= Util\.maxtransformlevels\(n\) \|\| throw\(AssertionError\("0 <= L <= maxtransformlevels\(n\)"\)\)', src)
    assert re.search(r"size\(trees\) == \(2\^Util\.maxtransformlevels\(n\) - 1, size\(x, 2\)\) \|\| throw\(DimensionMismatch", src)
    # the input tree of the search goes through the helper of the wpt_batch glue: the reference's errors for a bad depth / tree
    assert re.search(r"t, nt, L = wpt_batch_tree\(n, tree\)", src)


def test_every_ccall_matches_the_abi():
    calls = _ccalls(open(GLUE).read())
    assert {c["sym"] for c in calls} == SYMS and len(calls) == 2
    assert _mismatches(calls) == []


def test_device_pointers_are_gc_preserved():
    want = {"wl_bestbasistree_filter_batch": {"x", "t", "trees"}, "wl_wpt_filter_batch_trees": {"y", "x", "trees"}}
    for c in _ccalls(open(GLUE).read()):
        names = [m.group(1) for a in c["args"] for m in re.finditer(r"pointer\((\w+)\)", a)]
        assert set(names) == want[c["sym"]], (c["sym"], names)
        m = re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", c["prefix"].rstrip())
        assert m, "%s (line %d): pointer(...) passed to C outside GC.@preserve" % (c["sym"], c["line"])
        assert set(names) <= set(m.group(1).split()), (c["sym"], c["line"], names)


def test_lint_is_not_vacuous():
    """a dropped argument, a wrong argument type and a wrong return type are all reported"""
    src = open(GLUE).read()
    good = "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Cint, Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cvoid})"
    assert good in src
    for broken in ("(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Cint, Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cvoid})",
                   "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Cint, Ptr{UInt8}, Int64, Cint, Cint, Ptr{Cvoid})"):
        bad = _mismatches(_ccalls(src.replace(good, broken)))
        assert bad and all(b[0] == "wl_wpt_filter_batch_trees" for b in bad), bad
    bad = _mismatches(_ccalls(src.replace("(:wl_bestbasistree_filter_batch, LIB), Cint,", "(:wl_bestbasistree_filter_batch, LIB), Cdouble,")))
    assert [b[0] for b in bad] == ["wl_bestbasistree_filter_batch"]
