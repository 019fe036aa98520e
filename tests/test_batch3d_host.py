"""wl_dwt_filter_batch3 (a batch of independent 3-D filter-bank transforms) at the ABI boundary and in the host mirror:
everything that can be checked without a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED_ARGTYPES = ["void*", "int", "void*", "void*", "int64*", "int64", "int64", "double*", "int", "int", "int", "void*"]
EXPECTED_PARAMS = ["wl_ctx *ctx", "int dtype", "void *y", "const void *x", "const int64_t *dims", "int64_t nvolumes",
                   "int64_t volume_stride", "const double *qmf", "int flen", "int L", "int fw", "void *stream"]
# the ccall argument tuple that matches them (Julia's names of the same C types)
EXPECTED_JULIA = ["Ptr{Cvoid}", "Cint", "Ptr{Cvoid}", "Ptr{Cvoid}", "Ptr{Int64}", "Int64", "Int64", "Ptr{Float64}", "Cint", "Cint", "Cint",
                  "Ptr{Cvoid}"]


def _ctype_name(t):
    names = {C.c_void_p: "void*", C.c_int: "int", C.c_int64: "int64", C.c_double: "double"}
    if t in names:
        return names[t]
    if hasattr(t, "_type_"):
        return {C.c_int64: "int64*", C.c_int32: "int32*", C.c_double: "double*"}[t._type_]
    raise AssertionError(t)


def test_symbol_and_signature(W):
    from wavelets_jl_amd import _lib
    assert "wl_dwt_filter_batch3" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["wl_dwt_filter_batch3"]
    assert res is C.c_int
    assert len(args) == 12
    assert [_ctype_name(t) for t in args] == EXPECTED_ARGTYPES
    lib = _lib.load()
    assert hasattr(lib, "wl_dwt_filter_batch3")
    hdr = open(os.path.join(ROOT, "include", "wavelets_mi355x.h")).read()
    m = re.search(r"WL_API int wl_dwt_filter_batch3\((.*?)\);", hdr, re.S)
    assert m, "wl_dwt_filter_batch3 is not declared in include/wavelets_mi355x.h"
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == EXPECTED_PARAMS


def test_null_context_returns_einval_arg(W):
    lib = W._lib.load()
    buf = (C.c_float * 1024)()
    p = C.cast(buf, C.c_void_p)
    q = (C.c_double * 2)(0.5, 0.5)
    rc = lib.wl_dwt_filter_batch3(None, 0, p, p, (C.c_int64 * 3)(8, 8, 8), 2, 512, q, 2, 1, 1, None)
    assert W._lib.STATUS[rc] == "WL_EINVAL_ARG", rc


def test_host_wrapper_type_errors(W):
    import torch
    import lifting_schemes as LS
    gls = LS.scheme(W, "cdf97")
    db2 = W.wavelet(W.WT.db2)
    x4 = torch.zeros(2, 8, 8, 8)                                 # host tensors: these checks come before the device is asked for
    for f in (W.dwt_batch, W.idwt_batch):
        # there is no batched lifting transform of volumes
        with pytest.raises(TypeError):
            f(x4, gls, 1)
        # ... and nothing beyond a batch of volumes
        for wt in (gls, db2):
            with pytest.raises(TypeError):
                f(torch.zeros(2, 2, 8, 8, 8), wt, 1)
            with pytest.raises(TypeError):
                f(torch.zeros(8, 8), wt, 1)
        with pytest.raises(TypeError):
            f(x4, "db2", 1)
    # a batch of volumes with an orthogonal filter gets as far as the device check (no TypeError), here without a device
    if not torch.cuda.is_available():
        xs = torch.zeros(2, 8, 8, 8).permute(3, 2, 1, 0)
        for f in (W.dwt_batch, W.idwt_batch):
            with pytest.raises(Exception) as ei:
                f(xs, db2, 1)
            assert not isinstance(ei.value, TypeError), ei.value


def test_julia_glue_calls_the_symbol(W):
    src = open(os.path.join(ROOT, "wavelets.jl_amd", "julia", "WaveletsMI355X.jl")).read()
    m = re.search(r"GC\.@preserve y x check\(ccall\(\(:wl_dwt_filter_batch3, LIB\), Cint,\s*\((.*?)\),\s*ctx\(\)", src, re.S)
    assert m, "no GC.@preserve'd ccall of wl_dwt_filter_batch3"
    assert [" ".join(t.split()) for t in m.group(1).split(",")] == EXPECTED_JULIA
    # methods of both directions for 4-D device arrays and an orthogonal filter
    assert re.search(r"for \(f, fw\) in \(\(:dwt_batch, true\), \(:idwt_batch, false\)\)\s*\n\s*@eval function \$f\(x::ROCArray\{T,4\}, filter::OrthoFilter", src)
