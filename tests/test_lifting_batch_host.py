"""wl_dwt_lifting_batch at the ABI boundary and in the host mirror: everything that can be checked without a device.

The argument checks of the entry point that need no device run before the device is touched (include/wavelets_mi355x.h), so
their status codes -- and their order -- are observable here through a NULL or a dummy context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lifting_schemes as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED_ARGTYPES = ["void*", "int", "void*", "void*", "int64*", "int64", "int64", "int", "int32*", "int32*", "int32*", "double*",
                     "double", "double", "int", "int", "void*"]


def _ctype_name(t):
    names = {C.c_void_p: "void*", C.c_int: "int", C.c_int64: "int64", C.c_double: "double"}
    if t in names:
        return names[t]
    if hasattr(t, "_type_"):
        return {C.c_int64: "int64*", C.c_int32: "int32*", C.c_double: "double*"}[t._type_]
    raise AssertionError(t)


def test_symbol_and_signature(W):
    from wavelets_jl_amd import _lib
    assert "wl_dwt_lifting_batch" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["wl_dwt_lifting_batch"]
    assert res is C.c_int
    assert [_ctype_name(t) for t in args] == EXPECTED_ARGTYPES
    lib = _lib.load()
    assert hasattr(lib, "wl_dwt_lifting_batch")
    # the declaration in the public header: same parameter list
    hdr = open(os.path.join(ROOT, "include", "wavelets_mi355x.h")).read()
    m = re.search(r"WL_API int wl_dwt_lifting_batch\((.*?)\);", hdr, re.S)
    assert m, "wl_dwt_lifting_batch is not declared in include/wavelets_mi355x.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["wl_ctx *ctx", "int dtype", "void *y", "const void *x", "const int64_t *dims", "int64_t nimages",
                      "int64_t image_stride", "int nsteps", "const int32_t *step_is_update", "const int32_t *step_ncoef",
                      "const int32_t *step_shift", "const double *coefs_flat", "double norm1", "double norm2", "int L", "int fw",
                      "void *stream"]


def _call(lib, ctx, y, x, dims, nimages, stride, sch, L, fw=1, dtype=0):
    iu, nc, sh, cf = sch.flatten()
    d = (C.c_int64 * 2)(*dims) if dims is not None else None
    return lib.wl_dwt_lifting_batch(ctx, dtype, y, x, d, nimages, stride, len(iu), iu.ctypes.data_as(C.POINTER(C.c_int32)),
                                    nc.ctypes.data_as(C.POINTER(C.c_int32)), sh.ctypes.data_as(C.POINTER(C.c_int32)),
                                    cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1, sch.norm2, L, fw, None)


def test_null_arguments_return_einval_arg(W):
    lib = W._lib.load()
    sch = LS.scheme(W, "cdf97")
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    rc = _call(lib, None, p, p, (8, 8), 1, 64, sch, 1)
    assert W._lib.STATUS[rc] == "WL_EINVAL_ARG", rc


def test_host_wrapper_type_and_shape_errors(W):
    import torch
    gls = LS.scheme(W, "cdf97")
    x = torch.zeros(4, 8, 8)                                     # a host tensor: the checks below come before the device is asked for
    # what is neither a filter nor a scheme keeps raising TypeError
    for bad in ("cdf97", None, 3, W.WT.cdf97):
        with pytest.raises(TypeError):
            W.dwt_batch(x, bad, 1)
        with pytest.raises(TypeError):
            W.idwt_batch(x, bad, 1)
    # a batch is an n0 x n1 x B array
    for wt in (gls, W.wavelet(W.WT.db2)):
        with pytest.raises(TypeError):
            W.dwt_batch(torch.zeros(8, 8), wt, 1)
    # non-square images with a scheme: what dwt(x[:, :, i], scheme) raises ("array must be square/cube", transforms_lifting.jl:131-132)
    xr = torch.zeros(3, 8, 16).permute(2, 1, 0)                  # 16 x 8 x 3
    with pytest.raises(W.ArgumentError, match="square"):
        W.dwt_batch(xr, gls, 1)
    with pytest.raises(W.ArgumentError, match="square"):
        W.idwt_batch(xr, gls, 1)
    # a square batch with a scheme gets as far as the device check (no TypeError any more), here without a device
    if not torch.cuda.is_available():
        xs = torch.zeros(3, 8, 8).permute(2, 1, 0)
        with pytest.raises(Exception) as ei:
            W.dwt_batch(xs, gls, 1)
        assert not isinstance(ei.value, TypeError), ei.value


def test_julia_glue_calls_the_symbol(W):
    src = open(os.path.join(ROOT, "wavelets.jl_amd", "julia", "WaveletsMI355X.jl")).read()
    assert re.search(r"ccall\(\(:wl_dwt_lifting_batch, LIB\)", src)
    # methods of both directions for a scheme
    assert re.search(r"for \(f, fw\) in \(\(:dwt_batch, true\), \(:idwt_batch, false\)\)\s*\n\s*@eval function \$f\(x::ROCArray\{T,3\}, scheme::GLS", src)
