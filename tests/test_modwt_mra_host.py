"""modwt_mra / modwt_mra_batch (wl_modwt_mra_batch; W.modwt_mra / W.modwt_mra_batch): everything that can be checked without a device.

- the symbol in the header, in _lib.SIGNATURES with the prototype's arity and pointer / scalar positions, and in `nm -D` of both
  libraries; a C99 translation unit that references it compiles against the header;
- the status codes whose rules need no device, in the documented order (modwt_mra_cases.RULES);
- the argument errors of the Python mirror, raised before any device call;
- the definition the device is held to, with the oracle alone: the columns of the reference analysis add up to the signal.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import modwt_mra_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "wavelets_mi355x.h")
SYM = "wl_modwt_mra_batch"
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


def test_symbol_in_header_signatures_and_both_libraries(W):
    from wavelets_jl_amd import _lib
    lib = _lib.load()
    proto = _prototype(SYM)
    assert SYM in _lib.SIGNATURES and _lib.SIGNATURES[SYM][0] is C.c_int
    argtypes = _lib.SIGNATURES[SYM][1]
    assert len(proto) == len(argtypes) == 14
    for k, ((ctype, name), at) in enumerate(zip(proto, argtypes)):
        assert C2CTYPES[ctype] is at, (k, name, ctype, at)
    assert hasattr(lib, SYM)
    assert [n for _, n in proto] == list(RC.BASE) + ["stream"]
    for path in _lib.LIB_PATHS.values():
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert SYM in set(re.findall(r" T (wl_[a-z0-9_]+)", out)), path
    assert lib.wl_version() == 100
    # the order of the status codes, the contract notes and the workspace rule are part of the header comment
    flat = " ".join(open(HDR).read().replace("\n *", " ").split())
    assert ("WL_EINVAL_ARG (NULL ctx / out / xw / qmf), WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EDIMS (n < 1, nunits < 1, ldo < n, ldw < n, "
            "a unit stride below ld * ncols, a product that no int64 holds or nunits * stride >= 2^60), WL_EALIAS (the byte ranges of out "
            "and xw overlap), WL_EINVAL_L (ncols < 1, ncols - 1 > 62).") in flat
    assert "the sign of a zero is not part of the contract" in flat and "propagates only what is in the column's own cascade" in flat
    assert '"k_modwt_mra_lds"' in flat and '"k_modwt_mra_step_b"' in flat and "holds 2 * G * ncols * n elements; groups change no bit." in flat


def test_a_c99_translation_unit_compiles_against_the_header(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "wavelets_mi355x.h"\n'
                   "int use(wl_ctx *c, void *o, const void *w, const double *q, void *s)\n"
                   "{ return wl_modwt_mra_batch(c, WL_F32, o, 64, 192, w, 64, 192, 64, 3, 3, q, 8, s); }\n")
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

    def call(args):
        a = {**RC.BASE, **args}
        return ST[lib.wl_modwt_mra_batch(*[named.get(v, v) if isinstance(v, str) else v for v in a.values()], None)]

    seen = set()
    for status, args in RC.rows(RC.RULES):
        assert call(args) == status, (status, args)
        seen.add(status)
    for status, breakers in RC.RULES:                    # each rule alone as well
        for b in breakers:
            assert call(b) == status, (status, b)
    assert seen == {RC.ARG, RC.DTYPE, RC.FILTER, RC.EDIMS, RC.ALIAS, RC.EL}
    assert [s for s, _ in RC.RULES] == [RC.ARG, RC.DTYPE, RC.FILTER, RC.EDIMS, RC.ALIAS, RC.EL]
    # a row is what its docstring says: the ALIAS rows also carry too many columns
    assert (RC.ALIAS, dict(ncols=64, out_unit_stride=4096, xw_unit_stride=4096, out="Q")) in RC.rows(RC.RULES)
    # out right behind the last element that xw's units reach is no overlap, one element earlier is (64 columns: the call that
    # passes the alias rule ends at WL_EINVAL_L, before it would touch the dummy context)
    end = 4096 + 63 * 64 + 64                            # (nunits - 1) * unit stride + (ncols - 1) * ld + n
    for off, want in ((end, RC.EL), (end - 1, RC.ALIAS)):
        assert call(dict(ncols=64, out_unit_stride=4096, xw_unit_stride=4096, out=C.c_void_p(C.addressof(bufq) + off * 4))) == want, off


def test_python_argument_errors_need_no_device(W):
    import torch

    def cpu(*shape, dtype=torch.float32):
        return torch.zeros(*reversed(shape), dtype=dtype).permute(*reversed(range(len(shape))))

    wt = W.wavelet(W.WT.db4)
    sch = W.wavelet(W.WT.cdf97, W.WT.Lifting)
    m, xw = cpu(100, 4), cpu(100, 4, 3)
    for f, a in ((W.modwt_mra, m), (W.modwt_mra_batch, xw)):
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
        assert f.__name__ in W.__all__ and getattr(W, f.__name__) is f
    for shape in ((100,), (100, 3)):
        with pytest.raises(TypeError, match="modwt_mra_batch expects an n x ncols x B array"):
            W.modwt_mra_batch(cpu(*shape), wt)
    for shape in ((100,), (100, 4, 3)):
        with pytest.raises(TypeError, match="modwt_mra expects a matrix"):
            W.modwt_mra(cpu(*shape), wt)
    with pytest.raises(W.DimensionMismatch, match="empty coefficient array"):
        W.modwt_mra_batch(cpu(100, 4, 3)[:, :0, :], wt)
    with pytest.raises(TypeError, match="modwt_mra_batch is not defined for complex arrays"):
        W.modwt_mra_batch(xw, wt, y=cpu(100, 4, 3, dtype=torch.complex64))
    # valid arguments get as far as the device check, here without a device: no CPU path
    if not torch.cuda.is_available():
        for call in (lambda: W.modwt_mra(m, wt), lambda: W.modwt_mra_batch(xw, wt), lambda: W.modwt_mra_batch(xw, wt, y=cpu(100, 4, 3))):
            with pytest.raises(W.HIPError):
                call()


DEFINITION_SHAPES = ((2, 1), (3, 1), (8, 3), (12, 3), (64, 6), (100, 6), (1000, 9), (8192, 13))
DEFINITION_BOUND = {np.float32: 4 * 8.2e-7, np.float64: 4 * 5.0e-12}


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.IDS)
def test_the_reference_analysis_adds_up_to_the_signal(W, oracle, dtype):
    """The definition, with the oracle alone: D_1 + ... + D_L + S_L = x for the orthogonal filters (batt2's table is not
    orthogonal: left out).  The columns are summed in Float64; the figure is max |sum - x| over haar / db2 / db4 / sym5 / coif6 and
    (n, L) in DEFINITION_SHAPES, on unit 0 of modwt_batch_cases.units.  Measured: 8.2e-7 (Float32, 8.12e-7 on the last run) and
    5.0e-12 (Float64, 4.98e-12).  The bound is 4 x those figures, a margin for other seeds.
    The same pass checks that the reference is what the device is documented to compute: every column comes back in the input's
    element type and a coefficient matrix with a single column is its own analysis."""
    worst = 0.0
    for fname in RC.ORTHOGONAL:
        q = W.wavelet(getattr(W.WT, fname)).qmf
        for n, L in DEFINITION_SHAPES:
            x = RC.units(n, 1, dtype)[0]
            ref = RC.reference(oracle, W, fname, n, 1, dtype, L)[0]
            assert ref.shape == (L + 1, n) and ref.dtype == dtype
            dev = float(np.abs(ref.astype(np.float64).sum(axis=0) - x.astype(np.float64)).max())
            assert dev <= DEFINITION_BOUND[dtype], (fname, n, L, dev)
            worst = max(worst, dev)
    print("max |sum of the columns - x| = %.3g (%s)" % (worst, np.dtype(dtype).name))
    one = RC.units(12, 1, dtype)
    assert np.array_equal(RC.mra_of(oracle, q, one), one)


def test_the_shared_cases_are_what_the_gpu_tests_need():
    """the shape table holds the sizes at which the code takes another path: several planes per workgroup with a remainder, both
    sides of the LDS cap, one vector apart, and a unit of 2^16 samples"""
    for dt in RC.DTYPES:
        sh = RC.shapes(dt)
        cap = RC.LDS_MAX[dt]
        assert 2 * cap * np.dtype(dt).itemsize == 65536
        assert [s[0] for s in sh["boundary"]] == [cap, cap + 16 // np.dtype(dt).itemsize]
        assert {(n, B) for n, B, _ in sh["packing"]} == {(64, 37), (64, 1), (100, 37), (100, 1)}
        assert {n for n, _, _ in sh["wrap"]} == {2, 3, 8, 12} and all(B == 5 for _, B, _ in sh["wrap"])
        assert sh["groups"] == [(1024, 5, 4), (cap + 64, 5, 2)] and sh["long"] == [(1 << 16, 2, 5)]
        # the packing shapes put planes of different depth into one workgroup: (L + 1) B planes are no multiple of a workgroup's
        assert all(((L + 1) * B) % 16 for _, B, L in sh["packing"])
    n, B, L = RC.DEEP
    assert (1 << (L - 1)) > 20 * n and RC.deep_coefficients(np.float32).shape == (B, L + 1, n)
