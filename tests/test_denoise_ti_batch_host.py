"""denoise_ti_batch (wl_denoise_ti_batch_filter, wl_denoise_ti_batch_lifting; W.denoise_ti_batch): everything that can be checked
without a device.

- the fixture (tests/denoise_ti_batch_cases.py over the units of tests/denoise_batch_cases.py), on the oracle's values: per unit the
  translation-invariant result with the unit's own sigma differs from the one with its neighbour's sigma and from the plain denoise,
  the sigmas of a batch are pairwise distinct, and transposed spin counts give different results (a mixed-up dimension shows);
- the two symbols in the header, _lib.SIGNATURES and `nm -D` of both libraries; the status codes in their documented order;
- the argument errors of the Python mirror, raised before any device call.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_batch_cases as DB
import denoise_ti_batch_cases as TB
import lifting_schemes as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("wl_denoise_ti_batch_filter", "wl_denoise_ti_batch_lifting")


# ---- the fixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ndim,B,nspin", TB.FILTER_CASES, ids=str)
def test_fixture_filter(oracle, W, n, ndim, B, nspin):
    for dt in TB.DTYPES:
        for wname, kind, L in TB.FILTER_COMBOS:
            TB.check_fixture(oracle, W, n, ndim, dt, B, nspin, wname, TB.level(oracle, n, L), kind)


@pytest.mark.parametrize("dtype", TB.DTYPES, ids=lambda d: d.__name__)
def test_fixture_lifting(oracle, W, dtype):
    """every pair the GPU test runs holds; the one pair DB.lifting_combos leaves out at (64, 1) fails there -- unit 2 keeps the same
    coefficients under its neighbour's hard threshold -- and nowhere else"""
    for n, ndim, B, nspin in TB.LIFTING_CASES:
        for sname, kind in DB.lifting_combos(n, ndim):
            TB.check_fixture(oracle, W, n, ndim, dtype, B, nspin, sname, DB.default_L(oracle, n), kind, lifting=True)
    assert DB.LIFTING_EXCEPT == {("twin_cdf97", "hard"): {(64, 1)}}
    with pytest.raises(AssertionError, match="unit 2: the neighbour"):
        TB.check_fixture(oracle, W, 64, 1, dtype, 5, (8,), "twin_cdf97", DB.default_L(oracle, 64), "hard", lifting=True)
    for n, ndim, B, nspin in TB.LIFTING_CASES[1:]:
        TB.check_fixture(oracle, W, n, ndim, dtype, B, nspin, "twin_cdf97", DB.default_L(oracle, n), "hard", lifting=True)


@pytest.mark.parametrize("dtype", TB.DTYPES, ids=lambda d: d.__name__)
def test_fixture_transposed_spin_counts_differ(oracle, W, dtype):
    for n, ndim, a, others in ((8, 2, (2, 3), [(3, 2)]), (64, 2, (2, 3), [(3, 2)]), (8, 3, (2, 1, 3), [(3, 1, 2), (1, 2, 3)])):
        L = DB.default_L(oracle, n)
        for wname, kind in (("sym5", "hard"), ("haar", "hard"), ("db2", "soft")):
            for i in range(3):
                ra = TB.ref_ti(oracle, W, n, ndim, dtype, i, wname, L, kind, a)
                for b in others:
                    assert not np.array_equal(ra, TB.ref_ti(oracle, W, n, ndim, dtype, i, wname, L, kind, b)), (n, ndim, wname, kind, i, a, b)


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_signatures_and_both_libraries(W):
    from wavelets_jl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "wavelets_mi355x.h")).read()
    lib = _lib.load()
    for s in SYMS:
        assert re.search(r"WL_API int %s\(" % s, hdr), s
        assert s in _lib.SIGNATURES and _lib.SIGNATURES[s][0] is C.c_int
        assert hasattr(lib, s)
        n_params = len(re.search(r"WL_API int %s\((.*?)\);" % s, hdr, re.S).group(1).split(","))
        assert n_params == len(_lib.SIGNATURES[s][1]), s
    # the batch form's arguments with nspin in front of the sigmas
    for s in SYMS:
        base = _lib.SIGNATURES[s.replace("_ti_batch_", "_batch_")][1]
        assert _lib.SIGNATURES[s][1] == base[:-3] + [_lib._i64p] + base[-3:], s
    for path in _lib.LIB_PATHS.values():
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert set(SYMS) <= set(re.findall(r" T (wl_[a-z0-9_]+)", out)), path
    # the order of the status codes, the workspace formula and the group option are part of the header comment
    flat = " ".join(hdr.split())
    assert ("WL_EINVAL_ARG (NULL ctx / y / x / dims / qmf / nspin, th outside 0..3, t_unit negative or NaN), * WL_EINVAL_DTYPE, "
            "WL_EINVAL_FILTER, WL_EINVAL_CUBE, WL_EDIMS") in flat
    assert "max(2 G N, min(G, nunits) * S without sigma_in) elements" in flat
    assert "WL_TI_BATCH_GROUP (0 = automatic) lowers G" in flat


def _filter_call(lib, ctx, y, x, ndims=2, dims=(12, 12, 1), nunits=2, stride=144, flen=4, L=3, th=0, t_unit=1.0, dtype=0, qmf=True, nspin=(2, 2, 1),
                 sig=None):
    q = (C.c_double * 64)(*([0.5] * 64))
    d = (C.c_int64 * 3)(*dims) if dims is not None else None
    ns = (C.c_int64 * 3)(*nspin) if nspin is not None else None
    return lib.wl_denoise_ti_batch_filter(ctx, dtype, y, x, ndims, d, nunits, stride, q if qmf else None, flen, L, th, t_unit, ns, sig, None, None)


def _lifting_call(lib, W, ctx, y, x, ndims=2, dims=(12, 12, 1), nunits=2, stride=144, nsteps=None, L=3, th=0, t_unit=1.0, dtype=0, nspin=(2, 2, 1),
                  sig=None):
    sch = LS.scheme(W, "cdf97")
    iu, nc, sh, cf = sch.flatten()
    i32 = C.POINTER(C.c_int32)
    d = (C.c_int64 * 3)(*dims) if dims is not None else None
    ns = (C.c_int64 * 3)(*nspin) if nspin is not None else None
    return lib.wl_denoise_ti_batch_lifting(ctx, dtype, y, x, ndims, d, nunits, stride, len(iu) if nsteps is None else nsteps, iu.ctypes.data_as(i32),
                                           nc.ctypes.data_as(i32), sh.ctypes.data_as(i32), cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1,
                                           sch.norm2, L, th, t_unit, ns, sig, None, None)


def test_status_codes_in_order_through_a_dummy_context(W):
    """one argument set per rule that breaks that rule and every later one; the argument rules run before the context is touched, so
    a block of zero bytes serves as the context.  y == x throughout: WL_EALIAS is the last rule of both entry points."""
    lib = W._lib.load()
    ST = W._lib.STATUS
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    dummy = C.cast((C.c_char * 4096)(), C.c_void_p)
    sig = (C.c_double * 4)()
    big = 1 << 40

    def rules(f, wavelet_bad, wavelet_status):
        bad = dict(dtype=7, dims=(8, 12, 1), nunits=0, L=-1, nspin=(0, 2, 1), **wavelet_bad)
        ok_wavelet = {k: v for k, v in bad.items() if k not in wavelet_bad}
        assert f(ctx=None, **bad) == f(y=None, **bad) == f(x=None, **bad) == f(**{**bad, "dims": None}) == "WL_EINVAL_ARG"
        assert f(**{**bad, "nspin": None}) == "WL_EINVAL_ARG"
        assert f(th=4, **bad) == f(th=-1, **bad) == f(t_unit=-1.0, **bad) == f(t_unit=float("nan"), **bad) == "WL_EINVAL_ARG"
        assert f(**bad) == "WL_EINVAL_DTYPE"
        assert f(**{**bad, "dtype": 0}) == f(**{**bad, "dtype": 1}) == wavelet_status
        assert f(**{**ok_wavelet, "dtype": 0}) == "WL_EINVAL_CUBE"
        assert f(ndims=3, dims=(12, 12, 8), nunits=0, L=-1, nspin=(0, 2, 1)) == "WL_EINVAL_CUBE"
        # WL_EDIMS: the rules of denoise_batch, then nspin
        assert f(nunits=0, L=-1) == f(stride=143, L=-1) == f(dims=(0, 0, 1), L=-1) == f(ndims=0, L=-1) == f(ndims=4, L=-1) == "WL_EDIMS"
        assert f(nspin=(0, 2, 1), L=-1) == f(nspin=(2, 0, 1), L=-1) == f(nspin=(2, -3, 1), L=-1) == "WL_EDIMS"
        assert f(ndims=3, dims=(12, 12, 12), stride=1728, nspin=(2, 2, 0), L=-1) == "WL_EDIMS"
        assert f(nspin=(2, 2, 0), L=2) == "WL_EALIAS"                          # (an entry beyond ndims is not read)
        # nunits * prod(nspin) beyond int64
        assert f(ndims=1, dims=(8, 1, 1), stride=8, nunits=big, nspin=(1 << 30, 1, 1), L=-1) == "WL_EDIMS"
        assert f(nunits=big, nspin=(1 << 12, 1 << 12, 1), L=-1) == "WL_EDIMS"
        assert f(nunits=1 << 20, nspin=(1 << 20, 1 << 20, 1), L=-1) == "WL_EINVAL_L"   # 2^60 planes: an int64 holds them
        assert f(L=-1) == "WL_EINVAL_L"
        assert f(L=3) == "WL_EINVAL_SIZE"                                      # 12 has no 2^3 factor
        assert f(ndims=1, dims=(7, 1, 1), stride=7, L=0, nspin=(3, 1, 1)) == "WL_EINVAL_SIZE"   # the estimate needs level 1: an even extent
        # the extent limits of the single translation-invariant call
        assert f(dims=(65536, 65536, 1), stride=1 << 32, L=2) == "WL_EINVAL_SIZE"
        assert f(ndims=3, dims=(1 << 20,) * 3, stride=1 << 60, L=2, nspin=(2, 2, 2)) == "WL_EINVAL_SIZE"
        assert f(dims=(65532, 65532, 1), stride=65532 * 65532, L=2) == "WL_EALIAS"
        assert f(L=2) == "WL_EALIAS"                                           # y == x, the last rule
        # (with sigma_in an odd extent passes the size rule at L = 0: the next rule answers)
        assert f(ndims=1, dims=(7, 1, 1), stride=7, L=0, nspin=(3, 1, 1), sig=sig) == "WL_EALIAS"

    def f(y=p, x=p, ctx=dummy, **kw):
        return ST[_filter_call(lib, ctx, y, x, **kw)]

    assert f(qmf=False, dtype=7, flen=1, dims=(8, 12, 1), nunits=0, L=-1) == "WL_EINVAL_ARG"
    rules(f, dict(flen=1), "WL_EINVAL_FILTER")
    assert f(flen=65, dims=(8, 12, 1)) == "WL_EINVAL_FILTER"

    def g(y=p, x=p, ctx=dummy, **kw):
        return ST[_lifting_call(lib, W, ctx, y, x, **kw)]

    rules(g, dict(nsteps=-1), "WL_EINVAL_SCHEME")
    assert g(nsteps=17, dims=(8, 12, 1)) == "WL_EINVAL_SCHEME"


# ---- the Python mirror: argument errors before any device call ------------------------------------------------------------------
def test_python_argument_errors_need_no_device(W):
    import torch

    def cpu(*shape):
        return torch.zeros(*reversed(shape)).permute(*reversed(range(len(shape))))

    assert "denoise_ti_batch" in W.__all__
    wt = W.wavelet(W.WT.sym5)
    # a unit that is no square / cube
    for shape in ((8, 4, 3), (8, 8, 4, 2), (8, 4, 8, 2), (4, 8, 8, 2)):
        with pytest.raises(W.ArgumentError, match="array must be square/cube"):
            W.denoise_ti_batch(cpu(*shape), wt)
    # what is not part of this call
    x = cpu(8, 8, 3)
    with pytest.raises(TypeError):
        W.denoise_ti_batch(x, None)
    for th in (W.BiggestTH(), W.PosTH(), W.NegTH()):
        with pytest.raises(TypeError):
            W.denoise_ti_batch(x, wt, dnt=W.VisuShrink(th, 1.0))
    # images and cubes: one nspin entry per unit dimension
    for bad in (4, (4,), (2, 2, 2), ()):
        with pytest.raises(W.ArgumentError, match="nspin"):
            W.denoise_ti_batch(x, wt, nspin=bad)
    with pytest.raises(W.ArgumentError, match="nspin"):
        W.denoise_ti_batch(cpu(8, 8, 8, 2), wt, nspin=(2, 2))
    with pytest.raises(W.ArgumentError, match="nspin"):
        W.denoise_ti_batch(x, wt, nspin=(2, 0))
    # a host sigma is validated before anything is uploaded
    with pytest.raises(AssertionError):
        W.denoise_ti_batch(x, wt, sigma=[0.1, -0.1, 0.2])
    with pytest.raises(AssertionError):
        W.denoise_ti_batch(x, wt, sigma=np.array([0.1, float("nan"), 0.2]))
    with pytest.raises(W.DimensionMismatch):
        W.denoise_ti_batch(x, wt, sigma=[0.1, 0.2])
    # denoise_batch keeps refusing the keyword: the translation-invariant batch is this function
    with pytest.raises(TypeError):
        W.denoise_batch(x, wt, TI=True)
    # valid arguments get as far as the device check, here without a device: no TypeError / ArgumentError / AssertionError
    if not torch.cuda.is_available():
        for call in (lambda: W.denoise_ti_batch(x, wt, sigma=[0.1, 0.2, 0.3]), lambda: W.denoise_ti_batch(x, wt, nspin=(2, 3)),
                     lambda: W.denoise_ti_batch(cpu(64, 2), wt, nspin=(2, 3, 4)), lambda: W.denoise_ti_batch(cpu(64, 2), wt, nspin=5),
                     lambda: W.denoise_ti_batch(cpu(64, 2), LS.scheme(W, "cdf97"))):
            with pytest.raises(W.HIPError):
                call()
