"""wl_dwt_lifting_batch3 (a batch of independent 3-D lifting transforms of cubes) at the ABI boundary and in the host mirrors:
everything that can be checked without a device.

The argument checks of the entry point need no device and run before the context is touched (include/wavelets_mi355x.h), so their
status codes -- and their order -- are observable here through a NULL or a dummy context: a block of zero bytes that a call which
fails one of those checks never reads."""
import ctypes as C
import os
import re

import pytest

import lifting_schemes as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED_ARGTYPES = ["void*", "int", "void*", "void*", "int64*", "int64", "int64", "int", "int32*", "int32*", "int32*", "double*",
                     "double", "double", "int", "int", "void*"]
EXPECTED_PARAMS = ["wl_ctx *ctx", "int dtype", "void *y", "const void *x", "const int64_t *dims", "int64_t nvolumes",
                   "int64_t volume_stride", "int nsteps", "const int32_t *step_is_update", "const int32_t *step_ncoef",
                   "const int32_t *step_shift", "const double *coefs_flat", "double norm1", "double norm2", "int L", "int fw",
                   "void *stream"]
# the ccall argument tuple that matches them (Julia's names of the same C types)
EXPECTED_JULIA = ["Ptr{Cvoid}", "Cint", "Ptr{Cvoid}", "Ptr{Cvoid}", "Ptr{Int64}", "Int64", "Int64", "Cint", "Ptr{Int32}", "Ptr{Int32}",
                  "Ptr{Int32}", "Ptr{Float64}", "Cdouble", "Cdouble", "Cint", "Cint", "Ptr{Cvoid}"]


def _ctype_name(t):
    names = {C.c_void_p: "void*", C.c_int: "int", C.c_int64: "int64", C.c_double: "double"}
    if t in names:
        return names[t]
    if hasattr(t, "_type_"):
        return {C.c_int64: "int64*", C.c_int32: "int32*", C.c_double: "double*"}[t._type_]
    raise AssertionError(t)


def test_symbol_and_signature(W):
    from wavelets_jl_amd import _lib
    assert "wl_dwt_lifting_batch3" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["wl_dwt_lifting_batch3"]
    assert res is C.c_int
    assert [_ctype_name(t) for t in args] == EXPECTED_ARGTYPES
    lib = _lib.load()
    assert hasattr(lib, "wl_dwt_lifting_batch3")
    hdr = open(os.path.join(ROOT, "include", "wavelets_mi355x.h")).read()
    m = re.search(r"WL_API int wl_dwt_lifting_batch3\((.*?)\);", hdr, re.S)
    assert m, "wl_dwt_lifting_batch3 is not declared in include/wavelets_mi355x.h"
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == EXPECTED_PARAMS
    # the sentences that named the hole are gone
    assert "volumes does not exist" not in " ".join(hdr.split())
    assert "no batched lifting transform of volumes" not in " ".join(hdr.split())


def _call(lib, ctx, y, x, dims, nvol, stride, sch, L, fw=1, dtype=0, nsteps=None):
    iu, nc, sh, cf = sch.flatten()
    d = (C.c_int64 * 3)(*dims) if dims is not None else None
    i32 = C.POINTER(C.c_int32)
    return lib.wl_dwt_lifting_batch3(ctx, dtype, y, x, d, nvol, stride, len(iu) if nsteps is None else nsteps, iu.ctypes.data_as(i32),
                                     nc.ctypes.data_as(i32), sh.ctypes.data_as(i32), cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1,
                                     sch.norm2, L, fw, None)


def test_null_arguments_return_einval_arg(W):
    lib = W._lib.load()
    sch = LS.scheme(W, "cdf97")
    buf = (C.c_float * 1024)()
    p = C.cast(buf, C.c_void_p)
    dummy = C.cast((C.c_char * 4096)(), C.c_void_p)
    ST = W._lib.STATUS
    assert ST[_call(lib, None, p, p, (8, 8, 8), 2, 512, sch, 1)] == "WL_EINVAL_ARG"
    # ... before every later rule
    assert ST[_call(lib, None, p, p, (8, 4, 8), 0, 1, sch, -1, dtype=7, nsteps=-1)] == "WL_EINVAL_ARG"
    assert ST[_call(lib, dummy, None, p, (8, 4, 8), 0, 1, sch, -1, dtype=7, nsteps=-1)] == "WL_EINVAL_ARG"
    assert ST[_call(lib, dummy, p, None, (8, 4, 8), 0, 1, sch, -1, dtype=7, nsteps=-1)] == "WL_EINVAL_ARG"
    assert ST[_call(lib, dummy, p, p, None, 0, 1, sch, -1, dtype=7, nsteps=-1)] == "WL_EINVAL_ARG"


def test_status_codes_in_order_through_a_dummy_context(W):
    """one argument set per rule that breaks that rule and every later one; the context is never read by a call that fails one"""
    lib = W._lib.load()
    sch = LS.scheme(W, "cdf97")
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    dummy = C.cast((C.c_char * 4096)(), C.c_void_p)
    ST = W._lib.STATUS

    def call(dims=(12, 12, 12), nvol=2, stride=4096, L=3, dtype=0, nsteps=-1):
        return ST[_call(lib, dummy, p, p, dims, nvol, stride, sch, L, dtype=dtype, nsteps=nsteps)]

    assert call(dims=(8, 12, 12), nvol=0, L=-1, dtype=7) == "WL_EINVAL_DTYPE"
    assert call(dims=(8, 12, 12), nvol=0, L=-1) == "WL_EINVAL_CUBE"            # the cube rule before the extents
    assert call(dims=(12, 12, 8), nvol=0, L=-1) == "WL_EINVAL_CUBE"
    assert call(dims=(12, 8, 12), nvol=0, L=-1) == "WL_EINVAL_CUBE"
    assert call(nvol=0, L=-1) == "WL_EDIMS"                                    # nvolumes < 1
    assert call(stride=1727, L=-1) == "WL_EDIMS"                               # volume_stride < 12^3
    assert call(dims=(0, 0, 0), L=-1) == "WL_EDIMS"
    assert call(dims=(-2, -2, -2), L=-1) == "WL_EDIMS"
    assert call(L=-1) == "WL_EINVAL_L"
    assert call(L=3) == "WL_EINVAL_SIZE"                                       # 12 has no 2^3 factor
    assert call(L=2) == "WL_EINVAL_SCHEME"                                     # nsteps = -1
    assert call(L=2, nsteps=17) == "WL_EINVAL_SCHEME"                          # more than WL_MAX_STEPS


def test_host_wrapper_type_and_shape_errors(W):
    import torch
    gls = LS.scheme(W, "cdf97")
    for f in (W.dwt_batch, W.idwt_batch):
        # a 4-D tensor that is no batch of cubes: TypeError, as before the batched transform existed (not ArgumentError)
        for shape in ((3, 8, 8, 2), (3, 8, 4, 8), (3, 4, 8, 8)):
            with pytest.raises(TypeError, match="cubes only"):
                f(torch.zeros(*shape).permute(3, 2, 1, 0), gls, 1)
        # nothing beyond a batch of volumes
        with pytest.raises(TypeError):
            f(torch.zeros(2, 2, 8, 8, 8), gls, 1)
        # a batch of cubes with a scheme gets as far as the device check (no TypeError any more), here without a device
        if not torch.cuda.is_available():
            with pytest.raises(Exception) as ei:
                f(torch.zeros(3, 8, 8, 8).permute(3, 2, 1, 0), gls, 1)
            assert not isinstance(ei.value, TypeError), ei.value


def test_julia_glue_calls_the_symbol(W):
    src = open(os.path.join(ROOT, "wavelets.jl_amd", "julia", "WaveletsMI355X.jl")).read()
    m = re.search(r"GC\.@preserve y x check\(ccall\(\(:wl_dwt_lifting_batch3, LIB\), Cint,\s*\((.*?)\),\s*ctx\(\)", src, re.S)
    assert m, "no GC.@preserve'd ccall of wl_dwt_lifting_batch3"
    assert [" ".join(t.split()) for t in m.group(1).split(",")] == EXPECTED_JULIA
    # methods of both directions for 4-D device arrays and a scheme
    assert re.search(r"for \(f, fw\) in \(\(:dwt_batch, true\), \(:idwt_batch, false\)\)\s*\n\s*@eval function \$f\(x::ROCArray\{T,4\}, scheme::GLS", src)
    # the GLS denoise method passes cubes on
    gls = src[src.index("function Threshold.denoise(x::ROCArray{T,N}, wt::GLS;"):]
    assert "(N == 3 && length(nspt) == 3)" in gls[:gls.index("\nend\n")]
