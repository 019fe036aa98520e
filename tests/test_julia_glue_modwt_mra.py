"""Lint of the modwt_mra Julia glue (wavelets.jl_amd/julia/WaveletsMI355X_modwt_mra.jl) -- CPU only, the rules
tests/test_julia_glue_modwt_batch.py applies to the modwt_batch glue (and its ccall parser):
  * every `ccall` matches _lib.SIGNATURES (name, return type, arity, each argument type), and the glue binds the new entry point;
  * every pointer(...) handed to C is kept alive by GC.@preserve;
  * the module includes the file, at the end of its list, and the file defines modwt_mra_batch on ROCArray{T,3} and modwt_mra on
    ROCMatrix{T} for OrthoFilter; the status -> exception mapping is the module's `check`.
"""
import os
import re

import test_julia_glue_wpt_batch as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "wavelets.jl_amd", "julia")
GLUE = os.path.join(JL, "WaveletsMI355X_modwt_mra.jl")
SYM = "wl_modwt_mra_batch"
_ccalls, _mismatches = B.D._ccalls, B.D._mismatches


def test_module_includes_the_file_and_the_methods_exist():
    main = open(os.path.join(JL, "WaveletsMI355X.jl")).read()
    assert re.search(r'^include\("WaveletsMI355X_modwt_mra\.jl"\)$', main, re.M)
    assert re.findall(r'^include\("(\w+)\.jl"\)$', main, re.M)[-1] == "WaveletsMI355X_modwt_mra"
    src = open(GLUE).read()
    assert re.search(r"^function modwt_mra_batch\(xw::ROCArray\{T,3\}, wt::OrthoFilter\)", src, re.M)
    assert re.search(r"^function modwt_mra\(xw::ROCMatrix\{T\}, wt::OrthoFilter\)", src, re.M)
    assert len(re.findall(r"where \{T<:Union\{Float32,Float64\}\}", src)) == 2
    assert re.search(r"out = similar\(xw, n, nc, nb\)", src) and re.search(r"out = similar\(xw, n, nc\)", src)
    assert len(re.findall(r"^    return out$", src, re.M)) == 2
    # no lifting form and no complex form
    code = re.sub(r"#[^\n]*", "", src)
    assert "GLS" not in code and "Complex" not in code
    # the sibling glue keeps its two methods: nothing was added there
    sib = open(os.path.join(JL, "WaveletsMI355X_modwt_batch.jl")).read()
    assert "mra" not in sib


def test_status_codes_become_the_modules_exceptions():
    src = open(GLUE).read()
    assert len(re.findall(r"check\(ccall\(", src)) == 2
    main = open(os.path.join(JL, "WaveletsMI355X.jl")).read()
    assert "rc == -4 && throw(DimensionMismatch(msg))" in main and "rc in (-1, -2, -3, -5, -6, -7, -9, -10) && throw(ArgumentError(msg))" in main


def test_every_ccall_matches_the_abi():
    calls = _ccalls(open(GLUE).read())
    assert {c["sym"] for c in calls} == {SYM} and len(calls) == 2
    assert _mismatches(calls) == []


def test_the_dense_layout_is_what_the_ccalls_pass():
    """out / xw are dense n x nc x B arrays: ld = n, unit stride = n * nc; the matrix form is a batch of one unit"""
    calls = [[" ".join(a.split()) for a in c["args"]] for c in _ccalls(open(GLUE).read())]
    assert calls[0][2:11] == ["pointer(out)", "n", "n * nc", "pointer(xw)", "n", "n * nc", "n", "nc", "nb"]
    assert calls[1][2:11] == ["pointer(out)", "n", "n * nc", "pointer(xw)", "n", "n * nc", "n", "nc", "1"]


def test_device_pointers_are_gc_preserved():
    for c in _ccalls(open(GLUE).read()):
        names = [m.group(1) for a in c["args"] for m in re.finditer(r"pointer\((\w+)\)", a)]
        assert set(names) == {"out", "xw"}, (c["sym"], names)
        m = re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", c["prefix"].rstrip())
        assert m, "%s (line %d): pointer(...) passed to C outside GC.@preserve" % (c["sym"], c["line"])
        assert set(names) <= set(m.group(1).split()), (c["sym"], c["line"], names)


def test_lint_is_not_vacuous():
    """a dropped argument, a wrong argument type and a wrong return type are all reported"""
    src = open(GLUE).read()
    good = "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Int64, Ptr{Float64}, Cint, Ptr{Cvoid})"
    assert src.count(good) == 2
    for broken in ("(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Cint, Int64, Ptr{Float64}, Cint, Ptr{Cvoid})",
                   "(Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Int64, Int64, Int64, Ptr{Float64}, Cint, Ptr{Cvoid})"):
        bad = _mismatches(_ccalls(src.replace(good, broken)))
        assert bad and all(b[0] == SYM for b in bad), bad
    bad = _mismatches(_ccalls(src.replace("(:wl_modwt_mra_batch, LIB), Cint,", "(:wl_modwt_mra_batch, LIB), Cdouble,")))
    assert bad and {b[0] for b in bad} == {SYM}
