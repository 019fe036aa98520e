"""The complex-valued entry points at the C boundary (include/wavelets_mi355x.h, section "complex-valued transforms") -- CPU only:
the six symbols are declared WL_API, bound in _lib.SIGNATURES with the arity of their prototypes and exported by both libraries,
and the header is still plain C99."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wavelets_mi355x.h")
SYMS = ("wl_complex_split", "wl_complex_merge", "wl_dwt_filter_complex", "wl_dwt_lifting_complex", "wl_wpt_filter_complex",
        "wl_wpt_lifting_complex")


def _prototypes():
    """name -> list of parameter declarations of every WL_API prototype (comments removed)"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"WL_API\s+int\s+(wl_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, re.S):
        out[m.group(1)] = [p.strip() for p in m.group(2).split(",")]
    return out


def test_symbols_declared_and_bound(W):
    protos = _prototypes()
    for s in SYMS:
        assert s in protos, s + " is not declared WL_API in the header"
        assert s in W._lib.SIGNATURES, s + " is missing from _lib.SIGNATURES"
        restype, argtypes = W._lib.SIGNATURES[s]
        assert len(argtypes) == len(protos[s]), (s, len(argtypes), protos[s])
        # context first, stream last, dtype second: the conventions of every transform entry point
        assert protos[s][0] == "wl_ctx *ctx" and protos[s][1] == "int dtype" and protos[s][-1] == "void *stream"


def test_pointer_and_scalar_positions_match(W):
    """every pointer parameter of the prototype is a pointer in the binding and every scalar a scalar"""
    import ctypes as C
    protos = _prototypes()
    for s in SYMS:
        for decl, ct in zip(protos[s], W._lib.SIGNATURES[s][1]):
            is_ptr = ct is C.c_void_p or hasattr(ct, "contents")
            assert ("*" in decl) == is_ptr, (s, decl, ct)
            if not is_ptr:
                want = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}[decl.split()[0]]
                assert ct is want, (s, decl, ct)


def test_both_libraries_export_them(W):
    for mode in ("exact", "fused"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", W._lib.LIB_PATHS[mode]]).decode()
        exported = set(re.findall(r" T (wl_[a-z0-9_]+)", out))
        assert set(SYMS) <= exported, (mode, set(SYMS) - exported)


def test_header_documents_the_status_order():
    txt = open(HEADER).read()
    sec = txt[txt.index("complex-valued transforms"):txt.index("introspection (tests / bench)")]
    flat = " ".join(sec.split()).replace("* ", "")
    assert ("WL_EINVAL_ARG (NULL ctx / y / x / dims / qmf), WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EDIMS (ndims outside 1..3, an extent or "
            "nunits < 1, unit_stride < prod(dims)), WL_EINVAL_L, WL_EINVAL_SIZE, WL_EALIAS (y == x)") in flat
    assert "WL_EINVAL_ARG, WL_EINVAL_DTYPE, WL_EINVAL_SCHEME, WL_EINVAL_CUBE, WL_EDIMS, WL_EINVAL_L, WL_EINVAL_SIZE" in flat


def test_header_still_compiles_as_c99():
    src = ('#include "wavelets_mi355x.h"\nint main(void){ return (wl_dwt_filter_complex == 0) + (wl_dwt_lifting_complex == 0) + '
           '(wl_wpt_filter_complex == 0) + (wl_wpt_lifting_complex == 0) + (wl_complex_split == 0) + (wl_complex_merge == 0); }\n')
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def test_complex_arrays_are_off_by_default(W):
    assert W.get_complex_arrays() is False
    with W.complex_arrays():
        assert W.get_complex_arrays() is True
    assert W.get_complex_arrays() is False


def test_complex_is_refused_outside_the_transforms(W):
    """no device needed: the rejection comes before anything touches the tensor's device"""
    import pytest
    import torch
    z = torch.zeros(16, dtype=torch.complex64)
    wt = W.wavelet(W.WT.db2)
    for name, call in (("denoise", lambda: W.denoise(z, wt)), ("threshold", lambda: W.threshold(z, W.HardTH(), 1.0)),
                       ("threshold_", lambda: W.threshold_(z, W.HardTH(), 1.0)), ("noisest", lambda: W.noisest(z, wt)),
                       ("modwt", lambda: W.modwt(z, wt, 2)), ("bestbasistree", lambda: W.bestbasistree(z, wt)),
                       ("coefentropy", lambda: W.coefentropy(z, W.ShannonEntropy())), ("dwtc", lambda: W.dwtc(z.reshape(8, 2), wt)),
                       ("denoise_batch", lambda: W.denoise_batch(z.reshape(8, 2), wt)),
                       ("noisest_batch", lambda: W.noisest_batch(z.reshape(8, 2), wt))):
        with pytest.raises(TypeError, match=name):
            call()
