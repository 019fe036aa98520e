"""wpt_batch / iwpt_batch (wl_wpt_filter_batch, wl_wpt_lifting_batch; W.wpt_batch / W.iwpt_batch): everything that can be checked
without a device.

- the two symbols in the header, in _lib.SIGNATURES with the prototype's arity and pointer / scalar positions, and in `nm -D` of
  both libraries; a C99 translation unit that references them compiles against the header;
- the status codes whose rules need no device, in the documented order;
- the argument errors of the Python mirror, raised before any device call.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lifting_schemes as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "wavelets_mi355x.h")
SYMS = ("wl_wpt_filter_batch", "wl_wpt_lifting_batch")
C2CTYPES = {"wl_ctx *": C.c_void_p, "void *": C.c_void_p, "const void *": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64, "double": C.c_double,
            "const double *": C.POINTER(C.c_double), "const uint8_t *": C.POINTER(C.c_uint8), "const int32_t *": C.POINTER(C.c_int32)}


def _prototype(sym):
    hdr = open(HDR).read()
    params = re.search(r"WL_API int %s\((.*?)\);" % sym, hdr, re.S).group(1)
    out = []
    for p in params.split(","):
        p = " ".join(p.split())
        m = re.match(r"(.*?)(\w+)$", p)
        out.append((m.group(1).strip(), m.group(2)))
    return out


def test_symbols_in_header_signatures_and_both_libraries(W):
    from wavelets_jl_amd import _lib
    lib = _lib.load()
    for s in SYMS:
        proto = _prototype(s)
        assert s in _lib.SIGNATURES and _lib.SIGNATURES[s][0] is C.c_int
        argtypes = _lib.SIGNATURES[s][1]
        assert len(proto) == len(argtypes), s
        for k, ((ctype, name), at) in enumerate(zip(proto, argtypes)):
            assert C2CTYPES[ctype] is at, (s, k, name, ctype, at)
        assert hasattr(lib, s)
    names = [n for _, n in _prototype("wl_wpt_filter_batch")]
    assert names == ["ctx", "dtype", "y", "x", "n", "nunits", "unit_stride", "qmf", "flen", "tree", "ntree", "L", "fw", "stream"]
    names = [n for _, n in _prototype("wl_wpt_lifting_batch")]
    assert names == ["ctx", "dtype", "y", "x", "n", "nunits", "unit_stride", "nsteps", "step_is_update", "step_ncoef", "step_shift", "coefs_flat",
                     "norm1", "norm2", "tree", "ntree", "L", "fw", "stream"]
    for path in _lib.LIB_PATHS.values():
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert set(SYMS) <= set(re.findall(r" T (wl_[a-z0-9_]+)", out)), path
    # the order of the status codes and the workspace rule are part of the header comment
    flat = " ".join(open(HDR).read().split())
    assert "WL_EINVAL_DTYPE, * WL_EINVAL_FILTER, WL_EDIMS (n < 1, nunits < 1, unit_stride < n, nunits * unit_stride >= 2^61), WL_EALIAS (y == x), WL_EINVAL_L * (tree == NULL), WL_EINVAL_TREE." in flat
    assert "nothing is allocated once wl_workspace_bytes_full(dtype, 1, {nunits * unit_stride}, L)" in flat


def test_a_c99_translation_unit_compiles_against_the_header(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "wavelets_mi355x.h"\n'
                   "int use(wl_ctx *c, void *y, const void *x, const double *q, const uint8_t *t, const int32_t *i, void *s)\n"
                   "{ return wl_wpt_filter_batch(c, WL_F32, y, x, 64, 3, 68, q, 8, t, 63, 0, 1, s)\n"
                   "       + wl_wpt_lifting_batch(c, WL_F64, y, x, 64, 3, 64, 4, i, i, i, q, 1.0, 1.0, (const uint8_t *)0, 0, 6, 0, s); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def test_status_codes_in_order_through_a_dummy_context(W):
    """one argument set per rule that breaks that rule and every later one; the argument rules run before the context is touched, so
    a block of zero bytes serves as the context"""
    lib = W._lib.load()
    ST = W._lib.STATUS
    buf, buf2 = (C.c_float * 4096)(), (C.c_float * 4096)()
    p, p2 = C.cast(buf, C.c_void_p), C.cast(buf2, C.c_void_p)
    dummy = C.cast((C.c_char * 4096)(), C.c_void_p)
    q = (C.c_double * 64)(*([0.5] * 64))
    sch = LS.scheme(W, "cdf97")
    iu, nc, sh, cf = sch.flatten()
    i32 = C.POINTER(C.c_int32)
    bad_tree = np.zeros(63, dtype=np.uint8)
    bad_tree[1] = 1
    bt = bad_tree.ctypes.data_as(C.POINTER(C.c_uint8))

    def f(ctx=dummy, y=p, x=p, dtype=0, n=64, nunits=2, stride=64, qmf=True, flen=4, tree=None, ntree=0, L=2):
        return ST[lib.wl_wpt_filter_batch(ctx, dtype, y, x, n, nunits, stride, q if qmf else None, flen, tree, ntree, L, 1, None)]

    bad = dict(dtype=7, flen=1, nunits=0, L=-1)                          # (y == x as well: every later rule is broken)
    assert f(ctx=None, **bad) == f(y=None, **bad) == f(x=None, **bad) == f(qmf=False, **bad) == "WL_EINVAL_ARG"
    assert f(**bad) == "WL_EINVAL_DTYPE"
    assert f(**{**bad, "dtype": 0}) == f(**{**bad, "dtype": 1, "flen": 65}) == "WL_EINVAL_FILTER"
    assert f(nunits=0, L=-1) == f(n=0, L=-1) == f(stride=63, L=-1) == f(nunits=1 << 40, stride=1 << 40, L=-1) == "WL_EDIMS"
    assert f(L=-1) == f(tree=bt, ntree=63) == "WL_EALIAS"
    assert f(y=p2, L=-1) == f(y=p2, L=7) == "WL_EINVAL_L"
    assert f(y=p2, tree=bt, ntree=63, L=-1) == f(y=p2, tree=bt, ntree=62) == "WL_EINVAL_TREE"       # (L is ignored with a tree)

    def g(ctx=dummy, y=p, x=p, dtype=0, n=64, nunits=2, stride=64, nsteps=len(iu), tree=None, ntree=0, L=2):
        return ST[lib.wl_wpt_lifting_batch(ctx, dtype, y, x, n, nunits, stride, nsteps, iu.ctypes.data_as(i32), nc.ctypes.data_as(i32),
                                           sh.ctypes.data_as(i32), cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1, sch.norm2, tree,
                                           ntree, L, 1, None)]

    badl = dict(dtype=7, nsteps=17, nunits=0, L=-1)
    assert g(ctx=None, **badl) == g(y=None, **badl) == g(x=None, **badl) == "WL_EINVAL_ARG"
    assert g(**badl) == "WL_EINVAL_DTYPE"
    assert g(**{**badl, "dtype": 0}) == g(**{**badl, "dtype": 1, "nsteps": -1}) == "WL_EINVAL_SCHEME"
    assert g(nunits=0, L=-1) == g(n=0, L=-1) == g(stride=63, L=-1) == "WL_EDIMS"
    assert g(L=-1) == g(L=7) == "WL_EINVAL_L"                           # (y == x is the in-place call: no alias rule)
    assert g(tree=bt, ntree=63) == "WL_EINVAL_TREE"


def test_python_argument_errors_need_no_device(W):
    import torch

    def cpu(*shape, dtype=torch.float32):
        return torch.zeros(*reversed(shape), dtype=dtype).permute(*reversed(range(len(shape))))

    wt, sch = W.wavelet(W.WT.db4), LS.scheme(W, "cdf97")
    x = cpu(64, 3)
    for f in (W.wpt_batch, W.iwpt_batch):
        for bad in ("db4", None, 4, W.WT.db4):
            with pytest.raises(TypeError, match=f.__name__):
                f(x, bad)
        for shape in ((64,), (8, 8, 3)):
            with pytest.raises(TypeError, match=f.__name__ + " expects a len x B array"):
                f(cpu(*shape), wt)
        for w in (wt, sch):
            with pytest.raises(AssertionError, match="maxtransformlevels"):
                f(x, w, 7)
            with pytest.raises(AssertionError, match="maxtransformlevels"):
                f(x, w, -1)
        with pytest.raises(TypeError, match=f.__name__ + " is not defined for complex arrays"):
            f(cpu(64, 3, dtype=torch.complex64), wt)
        with W.complex_arrays():
            with pytest.raises(TypeError, match=f.__name__ + " is not defined for complex arrays"):
                f(cpu(64, 3, dtype=torch.complex64), wt)
            with pytest.raises(TypeError, match=f.__name__):
                f(x, wt, 3, y=cpu(64, 3, dtype=torch.complex64))
    assert W.wpt_batch.__name__ in W.__all__ and W.iwpt_batch.__name__ in W.__all__
    # valid arguments get as far as the device check, here without a device: no TypeError / AssertionError
    if not torch.cuda.is_available():
        for call in (lambda: W.wpt_batch(x, wt), lambda: W.iwpt_batch(x, sch, 3), lambda: W.wpt_batch(x, wt, W.maketree(64, 3, "dwt"))):
            with pytest.raises(W.HIPError):
                call()
