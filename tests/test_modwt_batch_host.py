"""modwt_batch / imodwt_batch (wl_modwt_batch, wl_imodwt_batch; W.modwt_batch / W.imodwt_batch): everything that can be checked
without a device.

- the two symbols in the header, in _lib.SIGNATURES with the prototype's arity and pointer / scalar positions, and in `nm -D` of
  both libraries; a C99 translation unit that references them compiles against the header;
- the status codes whose rules need no device, in the documented order (modwt_batch_cases.RULES_FWD / RULES_INV);
- the argument errors of the Python mirror, raised before any device call.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import modwt_batch_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "wavelets_mi355x.h")
SYMS = ("wl_modwt_batch", "wl_imodwt_batch")
C2CTYPES = {"wl_ctx *": C.c_void_p, "void *": C.c_void_p, "const void *": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64,
            "const double *": C.POINTER(C.c_double)}


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
    assert [n for _, n in _prototype("wl_modwt_batch")] == list(MC.BASE_FWD) + ["stream"]
    assert [n for _, n in _prototype("wl_imodwt_batch")] == list(MC.BASE_INV) + ["stream"]
    for path in _lib.LIB_PATHS.values():
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert set(SYMS) <= set(re.findall(r" T (wl_[a-z0-9_]+)", out)), path
    # the order of the status codes and the workspace rule are part of the header comment
    flat = " ".join(open(HDR).read().replace("\n *", " ").split())
    assert ("WL_EINVAL_ARG (NULL ctx / out / x / qmf), WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EDIMS (n < 1, nunits < 1, unit_stride < n, "
            "ldo < n, out_unit_stride < ldo * (L+1), a product that no int64 holds or nunits * stride >= 2^60), WL_EALIAS (the units of "
            "out and of x overlap), WL_EINVAL_SIZE (L > floor(log2 n)), WL_EINVAL_L (L < 1).") in flat
    assert "WL_EINVAL_FILTER, WL_EDIMS (as above, with ldw, xw_unit_stride and ncols), WL_EALIAS, WL_EINVAL_L (ncols < 1, ncols - 1 > 62)." in flat
    assert "Workspace: the LDS tier holds nothing." in flat and "option WL_MODWT_BATCH_GROUP lowers it" in flat
    assert "holds those 2 * G * n elements; groups change no bit." in flat


def test_a_c99_translation_unit_compiles_against_the_header(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "wavelets_mi355x.h"\n'
                   "int use(wl_ctx *c, void *o, const void *x, void *y, const double *q, void *s)\n"
                   "{ return wl_modwt_batch(c, WL_F32, o, 64, 192, x, 64, 3, 68, q, 8, 2, s)\n"
                   "       + wl_imodwt_batch(c, WL_F64, y, 64, o, 64, 192, 64, 3, 3, q, 8, s); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def test_status_codes_in_order_through_a_dummy_context(W):
    """every row breaks one rule and every later one; the argument rules run before the context is touched, so a block of zero
    bytes serves as the context"""
    lib = W._lib.load()
    ST = W._lib.STATUS
    bufp, bufq = (C.c_float * 16384)(), (C.c_float * 16384)()
    dummy = (C.c_char * 4096)()
    q = (C.c_double * 64)(*([0.5] * 64))
    named = {"CTX": C.cast(dummy, C.c_void_p), "P": C.cast(bufp, C.c_void_p), "Q": C.cast(bufq, C.c_void_p),
             "Q+32": C.c_void_p(C.addressof(bufq) + 32 * 4), "QMF": q}

    def call(fn, base, args):
        a = {**base, **args}
        return ST[fn(*[named.get(v, v) if isinstance(v, str) else v for v in a.values()], None)]

    seen = set()
    for fn, base, rules in ((lib.wl_modwt_batch, MC.BASE_FWD, MC.RULES_FWD), (lib.wl_imodwt_batch, MC.BASE_INV, MC.RULES_INV)):
        for status, args in MC.rows(rules):
            assert call(fn, base, args) == status, (fn.__name__, status, args)
            seen.add(status)
        # each rule alone as well
        for status, breakers in rules:
            for b in breakers:
                assert call(fn, base, b) == status, (fn.__name__, status, b)
    assert seen == {MC.ARG, MC.DTYPE, MC.FILTER, MC.EDIMS, MC.ALIAS, MC.SIZE, MC.EL}
    # a row is what its docstring says: the ALIAS rows of the forward call also carry a bad L
    assert (MC.ALIAS, dict(L=7, out="Q")) in MC.rows(MC.RULES_FWD)


def test_python_argument_errors_need_no_device(W):
    import torch

    def cpu(*shape, dtype=torch.float32):
        return torch.zeros(*reversed(shape), dtype=dtype).permute(*reversed(range(len(shape))))

    wt = W.wavelet(W.WT.db4)
    sch = W.wavelet(W.WT.cdf97, W.WT.Lifting)
    x, xw = cpu(100, 3), cpu(100, 4, 3)
    for f, a in ((W.modwt_batch, x), (W.imodwt_batch, xw)):
        for bad in ("db4", None, 4, W.WT.db4, sch):
            with pytest.raises(TypeError, match=f.__name__ + " is defined for OrthoFilter wavelets only"):
                f(a, bad)
        with pytest.raises(TypeError, match=f.__name__ + " is not defined for complex arrays"):
            f(a.to(torch.complex64), wt)
        with W.complex_arrays():
            with pytest.raises(TypeError, match=f.__name__ + " is not defined for complex arrays"):
                f(a.to(torch.complex64), wt)
        with pytest.raises(TypeError, match="expected a torch tensor"):
            f(np.zeros(tuple(a.shape)), wt)
    for shape in ((100,), (10, 10, 3)):
        with pytest.raises(TypeError, match="modwt_batch expects a len x B array"):
            W.modwt_batch(cpu(*shape), wt)
    for shape in ((100,), (100, 3)):
        with pytest.raises(TypeError, match="imodwt_batch expects an n x ncols x B array"):
            W.imodwt_batch(cpu(*shape), wt)
    assert W.maxmodwttransformlevels(100) == 6
    with pytest.raises(W.ArgumentError, match=re.escape("Too many transform levels (length(x) < 2^L)")):
        W.modwt_batch(x, wt, 7)
    for L in (0, -1):
        with pytest.raises(W.ArgumentError, match="L must be >= 1"):
            W.modwt_batch(x, wt, L)
    with pytest.raises(TypeError, match="modwt_batch is not defined for complex arrays"):
        W.modwt_batch(x, wt, 3, y=cpu(100, 4, 3, dtype=torch.complex64))
    assert W.modwt_batch.__name__ in W.__all__ and W.imodwt_batch.__name__ in W.__all__
    # valid arguments get as far as the device check, here without a device: no TypeError / ArgumentError
    if not torch.cuda.is_available():
        for call in (lambda: W.modwt_batch(x, wt), lambda: W.modwt_batch(x, wt, 6), lambda: W.imodwt_batch(xw, wt)):
            with pytest.raises(W.HIPError):
                call()


def test_the_shared_cases_are_what_the_gpu_tests_need():
    """the shape table holds the sizes at which the code takes another path: several units per workgroup with a remainder, both
    sides of the LDS cap, one vector apart, and a unit of 2^16 samples"""
    for dt in MC.DTYPES:
        sh = MC.shapes(dt)
        cap = MC.LDS_MAX[dt]
        assert 2 * cap * np.dtype(dt).itemsize == 65536
        assert [s[0] for s in sh["boundary"]] == [cap, cap + 16 // np.dtype(dt).itemsize]
        assert {(n, B) for n, B, _ in sh["packing"]} == {(64, 37), (64, 1), (100, 37), (100, 1)}
        assert {n for n, _, _ in sh["wrap"]} == {2, 3, 8, 12} and all(B == 5 for _, B, _ in sh["wrap"])
        assert all(1 <= L <= MC.maxlevels(n) for n, _, L in MC.all_shapes(dt))
    u = MC.units(12, 5, np.float32)
    assert u.shape == (5, 12) and len({r.tobytes() for r in u}) == 5
