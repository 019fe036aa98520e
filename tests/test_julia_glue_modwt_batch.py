"""Lint of the modwt_batch Julia glue (wavelets.jl_amd/julia/WaveletsMI355X_modwt_batch.jl) -- CPU only, the rules
tests/test_julia_glue_bestbasis_batch.py applies to the bestbasistree_batch glue (and its ccall parser):
  * every `ccall` matches _lib.SIGNATURES (name, return type, arity, each argument type), and the glue binds the two new entry points;
  * every pointer(...) handed to C is kept alive by GC.@preserve;
  * the module includes the file, and the file defines modwt_batch on ROCMatrix{T} and imodwt_batch on ROCArray{T,3} for
    OrthoFilter, with the reference's errors for a bad L.
"""
import os
import re

import test_julia_glue_wpt_batch as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "wavelets.jl_amd", "julia")
GLUE = os.path.join(JL, "WaveletsMI355X_modwt_batch.jl")
SYMS = {"wl_modwt_batch", "wl_imodwt_batch"}
_ccalls, _mismatches = B.D._ccalls, B.D._mismatches


def test_module_includes_the_file_and_the_methods_exist():
    main = open(os.path.join(JL, "WaveletsMI355X.jl")).read()
    assert re.search(r'^include\("WaveletsMI355X_modwt_batch\.jl"\)$', main, re.M)
    src = open(GLUE).read()
    assert re.search(r"^function modwt_batch\(x::ROCMatrix\{T\}, wt::OrthoFilter, L::Integer=Util\.maxmodwttransformlevels\(size\(x, 1\)\)\)", src, re.M)
    assert re.search(r"^function imodwt_batch\(xw::ROCArray\{T,3\}, wt::OrthoFilter\)", src, re.M)
    assert len(re.findall(r"where \{T<:Union\{Float32,Float64\}\}", src)) == 2
    assert re.search(r"out = similar\(x, n, L \+ 1, nb\)", src) and re.search(r"^    return out$", src, re.M)
    assert re.search(r"x = similar\(xw, n, nb\)", src) and re.search(r"^    return x$", src, re.M)
    # no lifting form and no complex form: modwt is defined for orthogonal filters on real vectors
    code = re.sub(r"#[^\n]*", "", src)
    assert "GLS" not in code and "Complex" not in code


def test_the_reference_exceptions():
    src = open(GLUE).read()
    assert re.search(r'L <= Util\.maxmodwttransformlevels\(n\) \|\| throw\(ArgumentError\("Too many transform levels \(length\(x\) < 2\^L\)"\)\)', src)
    assert re.search(r'L >= 1 \|\| throw\(ArgumentError\("L must be >= 1"\)\)', src)
    main = open(os.path.join(JL, "WaveletsMI355X.jl")).read()
    assert "rc == -4 && throw(DimensionMismatch(msg))" in main and "rc in (-1, -2, -3, -5, -6, -7, -9, -10) && throw(ArgumentError(msg))" in main


def test_every_ccall_matches_the_abi():
    calls = _ccalls(open(GLUE).read())
    assert {c["sym"] for c in calls} == SYMS and len(calls) == 2
    assert _mismatches(calls) == []


def test_the_dense_layout_is_what_the_ccalls_pass():
    """out / xw are dense n x cols x B arrays: ld = n, unit stride = n * cols; the panel's unit stride is n"""
    calls = {c["sym"]: [" ".join(a.split()) for a in c["args"]] for c in _ccalls(open(GLUE).read())}
    assert calls["wl_modwt_batch"][2:9] == ["pointer(out)", "n", "n * (L + 1)", "pointer(x)", "n", "nb", "n"]
    assert calls["wl_imodwt_batch"][2:10] == ["pointer(x)", "n", "pointer(xw)", "n", "n * nc", "n", "nc", "nb"]


def test_device_pointers_are_gc_preserved():
    want = {"wl_modwt_batch": {"out", "x"}, "wl_imodwt_batch": {"x", "xw"}}
    for c in _ccalls(open(GLUE).read()):
        names = [m.group(1) for a in c["args"] for m in re.finditer(r"pointer\((\w+)\)", a)]
        assert set(names) == want[c["sym"]], (c["sym"], names)
        m = re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", c["prefix"].rstrip())
        assert m, "%s (line %d): pointer(...) passed to C outside GC.@preserve" % (c["sym"], c["line"])
        assert set(names) <= set(m.group(1).split()), (c["sym"], c["line"], names)


def test_lint_is_not_vacuous():
    """a dropped argument, a wrong argument type and a wrong return type are all reported"""
    src = open(GLUE).read()
    good = "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Cint, Cint, Ptr{Cvoid})"
    assert good in src
    for broken in ("(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Cint, Cint, Ptr{Cvoid})",
                   "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Cint, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Cint, Cint, Ptr{Cvoid})"):
        bad = _mismatches(_ccalls(src.replace(good, broken)))
        assert bad and all(b[0] == "wl_modwt_batch" for b in bad), bad
    bad = _mismatches(_ccalls(src.replace("(:wl_imodwt_batch, LIB), Cint,", "(:wl_imodwt_batch, LIB), Cdouble,")))
    assert [b[0] for b in bad] == ["wl_imodwt_batch"]
