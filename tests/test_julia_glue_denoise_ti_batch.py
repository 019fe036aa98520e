"""Lint of the denoise_ti_batch Julia glue (wavelets.jl_amd/julia/WaveletsMI355X_denoise_ti_batch.jl) -- CPU only, the rules
tests/test_julia_glue_denoise_batch.py applies to the denoise_batch glue (its parser is reused):
  * every `ccall` matches _lib.SIGNATURES (name, return type, arity, each argument type), and the glue binds the two new entry points;
  * every pointer(...) handed to C is kept alive by GC.@preserve, and failures go through `check`;
  * the module includes the file after the denoise_batch glue it builds on, and the file defines denoise_ti_batch for filters and
    lifting schemes with nspin handed over in front of the sigmas.
"""
import os
import re

import test_julia_glue_denoise_batch as GB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "wavelets.jl_amd", "julia")
GLUE = os.path.join(JL, "WaveletsMI355X_denoise_ti_batch.jl")
SYMS = {"wl_denoise_ti_batch_filter", "wl_denoise_ti_batch_lifting"}


def test_module_includes_the_file():
    mod = open(os.path.join(JL, "WaveletsMI355X.jl")).read()
    m = re.search(r'^include\("WaveletsMI355X_denoise_ti_batch\.jl"\)$', mod, re.M)
    assert m and mod.index('include("WaveletsMI355X_denoise_batch.jl")') < m.start()      # batch_units / batch_sigma / BATCH_TH
    src = open(GLUE).read()
    assert len(re.findall(r"^function denoise_ti_batch\(x::ROCArray\{T,N\}, wt::(?:OrthoFilter|GLS)", src, re.M)) == 2
    assert re.search(r"^function batch_nspin\(", src, re.M)


def test_every_ccall_matches_the_abi():
    calls = GB._ccalls(open(GLUE).read())
    assert {c["sym"] for c in calls} == SYMS and len(calls) == 2
    assert GB._mismatches(calls) == []
    for c in calls:
        # ..., t_unit, nspin, sigma_in, sigma_out, stream
        assert c["types"][-5:] == ["Cdouble", "Ptr{Int64}", "Ptr{Float64}", "Ptr{Float64}", "Ptr{Cvoid}"], c["sym"]
        assert c["args"][-4].strip() == "nsp" and c["args"][-1].strip() == "stream()", c["sym"]


def test_device_pointers_are_gc_preserved_and_the_status_is_checked():
    for c in GB._ccalls(open(GLUE).read()):
        names = [m.group(1) for a in c["args"] for m in re.finditer(r"pointer\((\w+)\)", a)]
        m = re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", c["prefix"].rstrip())
        assert m, "%s (line %d): pointer(...) passed to C outside GC.@preserve / check" % (c["sym"], c["line"])
        assert {"y", "x", "sig_in", "sout"} == set(names) <= set(m.group(1).split()), (c["sym"], c["line"], names)


def test_lint_is_not_vacuous():
    """a dropped argument, a wrong argument type and a wrong return type are all reported"""
    src = open(GLUE).read()
    good = "Cdouble,\n                 Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid})"
    assert src.count(good) == 1
    for broken in (good.replace("Ptr{Int64}, ", ""), good.replace("Ptr{Int64}", "Int64")):
        bad = GB._mismatches(GB._ccalls(src.replace(good, broken)))
        assert bad and all(b[0] == "wl_denoise_ti_batch_filter" for b in bad), bad
    bad = GB._mismatches(GB._ccalls(src.replace("(:wl_denoise_ti_batch_lifting, LIB), Cint,", "(:wl_denoise_ti_batch_lifting, LIB), Cdouble,")))
    assert [b[0] for b in bad] == ["wl_denoise_ti_batch_lifting"]
