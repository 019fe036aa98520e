"""denoise_batch (wl_mad_batch, wl_denoise_batch_filter, wl_denoise_batch_lifting; W.denoise_batch / W.noisest_batch): everything
that can be checked without a device.

- the shared fixture (tests/denoise_batch_cases.py) separates "own sigma" from "somebody's sigma": per unit the share of zeroed
  coefficients lies strictly inside (0.2, 0.999), the sigmas of a batch are pairwise distinct and a neighbour's sigma changes the
  oracle's result;
- the premise of the one-transform sequence: detailrange(., 1) of the first column of the L-level transform is bit-equal to that of
  the level-1 transform;
- the three symbols in the header, _lib.SIGNATURES and `nm -D` of both libraries; the status codes whose rules need no device;
- the argument errors of the Python mirror, raised before any device call.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_batch_cases as DB
import lifting_schemes as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("wl_mad_batch", "wl_denoise_batch_filter", "wl_denoise_batch_lifting")
DTYPES = [np.float32, np.float64]


# ---- the fixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ndim,B,dtypes", DB.FILTER_SHAPES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_fixture_separates_own_sigma_from_somebody_elses(oracle, W, n, ndim, B, dtypes):
    """at the default L, for every wavelet and threshold kind the GPU test pairs at this shape"""
    L = DB.default_L(oracle, n)
    for dt in dtypes:
        for wname, kind in sorted({(w, k) for w, k, _ in DB.filter_combos(n, ndim)}):
            DB.check_fixture(oracle, W, n, ndim, np.dtype(dt).type, B, wname, L, kind)


def test_fixture_hard_threshold_at_every_shape_the_issue_lists(oracle, W):
    """sym5, db2 and haar with the hard threshold at the default L (the run the issue reports): shares and distinct sigmas
    everywhere; the neighbour's sigma changes the result everywhere except unit 0 of the 8 x 8 haar batch (DB.FILTER_EXCEPT)"""
    same = []
    for n, ndim, B, dtypes in DB.FILTER_SHAPES:
        for dt in dtypes:
            for wname in ("sym5", "db2", "haar"):
                try:
                    DB.check_fixture(oracle, W, n, ndim, np.dtype(dt).type, B, wname, DB.default_L(oracle, n), "hard")
                except AssertionError as e:
                    assert "neighbour" in str(e), e
                    same.append((n, ndim, dt, wname))
    assert same == [(8, 2, "float32", "haar"), (8, 2, "float64", "haar")], same
    assert DB.FILTER_EXCEPT == {("haar", "hard"): {(8, 2)}}


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_fixture_lifting(oracle, W, dtype):
    """every pair the GPU test runs at a shape holds there; the one pair left out of one shape (DB.LIFTING_EXCEPT) fails there, for
    the reason given, and nowhere else"""
    for n, ndim, B in DB.LIFTING_SHAPES:
        for sname, kind in DB.lifting_combos(n, ndim):
            DB.check_fixture(oracle, W, n, ndim, dtype, B, sname, DB.default_L(oracle, n), kind, lifting=True)
    assert DB.LIFTING_EXCEPT == {("twin_cdf97", "hard"): {(64, 1)}}
    with pytest.raises(AssertionError, match="neighbour"):
        DB.check_fixture(oracle, W, 64, 1, dtype, 5, "twin_cdf97", DB.default_L(oracle, 64), "hard", lifting=True)


# ---- the premise: level 1's detail range is final after level 1 ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n,ndim", [(64, 1), (16, 2), (8, 3)])
def test_level1_detail_range_is_final_after_level_1(oracle, W, n, ndim, dtype):
    x = DB.unit(1, n, ndim, dtype)
    lo, hi = int(round(n / 2 + 1)) - 1, n
    assert (lo, hi) == (n // 2, n)
    for wname, lifting in (("sym5", False), ("db2", False), ("cdf97", True)):
        fwd, _ = DB.transforms(oracle, W, wname, lifting)
        one = np.asfortranarray(fwd(x, 1)).reshape(-1, order="F")[lo:hi]
        for L in sorted({2, oracle.maxtransformlevels(n)}):
            deep = np.asfortranarray(fwd(x, L)).reshape(-1, order="F")[lo:hi]
            assert np.array_equal(one, deep), (wname, n, ndim, L)
        assert np.any(one != 0)


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
    for path in _lib.LIB_PATHS.values():
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert set(SYMS) <= set(re.findall(r" T (wl_[a-z0-9_]+)", out)), path
    # the order of the status codes and the workspace formula are part of the header comment
    flat = " ".join(hdr.split())
    assert "Workspace (wl_workspace_bytes_full does not cover it)" in flat
    assert "WL_EINVAL_ARG (NULL ctx / y / x / dims / qmf, th outside 0..3, t_unit negative or NaN), * WL_EINVAL_DTYPE, WL_EINVAL_FILTER, WL_EINVAL_CUBE, WL_EDIMS" in flat


def _filter_call(lib, ctx, y, x, ndims=2, dims=(12, 12, 1), nunits=2, stride=144, flen=4, L=3, th=0, t_unit=1.0, dtype=0, qmf=True, sig=None):
    q = (C.c_double * 64)(*([0.5] * 64))
    d = (C.c_int64 * 3)(*dims) if dims is not None else None
    return lib.wl_denoise_batch_filter(ctx, dtype, y, x, ndims, d, nunits, stride, q if qmf else None, flen, L, th, t_unit, sig, None, None)


def _lifting_call(lib, W, ctx, y, x, ndims=2, dims=(12, 12, 1), nunits=2, stride=144, nsteps=None, L=3, th=0, t_unit=1.0, dtype=0, sig=None):
    iu, nc, sh, cf = LS.scheme(W, "cdf97").flatten()
    sch = LS.scheme(W, "cdf97")
    i32 = C.POINTER(C.c_int32)
    d = (C.c_int64 * 3)(*dims) if dims is not None else None
    return lib.wl_denoise_batch_lifting(ctx, dtype, y, x, ndims, d, nunits, stride, len(iu) if nsteps is None else nsteps, iu.ctypes.data_as(i32),
                                        nc.ctypes.data_as(i32), sh.ctypes.data_as(i32), cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1,
                                        sch.norm2, L, th, t_unit, sig, None, None)


def test_status_codes_in_order_through_a_dummy_context(W):
    """one argument set per rule that breaks that rule and every later one; the argument rules run before the context is touched, so
    a block of zero bytes serves as the context"""
    lib = W._lib.load()
    ST = W._lib.STATUS
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    dummy = C.cast((C.c_char * 4096)(), C.c_void_p)
    sig = (C.c_double * 4)()
    bad = dict(dtype=7, flen=1, dims=(8, 12, 1), nunits=0, L=-1)

    def f(y=p, x=p, ctx=dummy, **kw):
        return ST[_filter_call(lib, ctx, y, x, **kw)]

    assert f(ctx=None, **bad) == f(y=None, **bad) == f(x=None, **bad) == f(qmf=False, **bad) == "WL_EINVAL_ARG"
    assert f(**{**bad, "dims": None}) == "WL_EINVAL_ARG"
    assert f(th=4, **bad) == f(th=-1, **bad) == f(t_unit=-1.0, **bad) == f(t_unit=float("nan"), **bad) == "WL_EINVAL_ARG"
    assert f(**bad) == "WL_EINVAL_DTYPE"
    assert f(**{**bad, "dtype": 0}) == f(**{**bad, "dtype": 1, "flen": 65}) == "WL_EINVAL_FILTER"
    assert f(dims=(8, 12, 1), nunits=0, L=-1) == "WL_EINVAL_CUBE"
    assert f(ndims=3, dims=(12, 12, 8), nunits=0, L=-1) == "WL_EINVAL_CUBE"
    assert f(nunits=0, L=-1) == f(stride=143, L=-1) == f(dims=(0, 0, 1), L=-1) == f(ndims=0, L=-1) == f(ndims=4, L=-1) == "WL_EDIMS"
    assert f(L=-1) == "WL_EINVAL_L"
    assert f(L=3) == "WL_EINVAL_SIZE"                                      # 12 has no 2^3 factor
    assert f(ndims=1, dims=(7, 1, 1), stride=7, L=0) == "WL_EINVAL_SIZE"   # the estimate needs level 1: an even extent
    assert f(L=2) == "WL_EALIAS"                                           # y == x, the last rule
    # (with sigma_in an odd extent passes the size rule at L = 0: the next rule answers)
    assert f(ndims=1, dims=(7, 1, 1), stride=7, L=0, sig=sig) == "WL_EALIAS"

    def g(y=p, x=p, ctx=dummy, **kw):
        return ST[_lifting_call(lib, W, ctx, y, x, **kw)]

    badl = dict(dtype=7, nsteps=-1, dims=(8, 12, 1), nunits=0, L=-1)
    assert g(ctx=None, **badl) == g(y=None, **badl) == g(x=None, **badl) == g(**{**badl, "dims": None}) == "WL_EINVAL_ARG"
    assert g(th=4, **badl) == g(t_unit=-0.5, **badl) == "WL_EINVAL_ARG"
    assert g(**badl) == "WL_EINVAL_DTYPE"
    assert g(**{**badl, "dtype": 0}) == g(**{**badl, "dtype": 1, "nsteps": 17}) == "WL_EINVAL_SCHEME"
    assert g(dims=(8, 12, 1), nunits=0, L=-1) == "WL_EINVAL_CUBE"
    assert g(nunits=0, L=-1) == g(stride=143, L=-1) == "WL_EDIMS"
    assert g(L=-1) == "WL_EINVAL_L"
    assert g(L=3) == g(ndims=1, dims=(7, 1, 1), stride=7, L=0) == "WL_EINVAL_SIZE"

    def m(y=p, n=8, nunits=2, stride=8, res=sig, dtype=0, ctx=dummy):
        return ST[lib.wl_mad_batch(ctx, dtype, y, n, nunits, stride, res, None)]

    assert m(ctx=None, dtype=7, n=0) == m(y=None, dtype=7, n=0) == m(res=None, dtype=7, n=0) == "WL_EINVAL_ARG"
    assert m(dtype=7, n=0) == "WL_EINVAL_DTYPE"
    assert m(n=0) == m(nunits=0) == m(stride=7) == "WL_EDIMS"
    assert m(n=1 << 31, stride=1 << 31) == "WL_EINVAL_SIZE"


# ---- the Python mirror: argument errors before any device call ------------------------------------------------------------------
def test_python_argument_errors_need_no_device(W):
    import torch

    def cpu(*shape):
        return torch.zeros(*reversed(shape)).permute(*reversed(range(len(shape))))

    wt = W.wavelet(W.WT.sym5)
    # a unit that is no square / cube
    for shape in ((8, 4, 3), (8, 8, 4, 2), (8, 4, 8, 2), (4, 8, 8, 2)):
        with pytest.raises(W.ArgumentError, match="array must be square/cube"):
            W.denoise_batch(cpu(*shape), wt)
        with pytest.raises(W.ArgumentError, match="array must be square/cube"):
            W.noisest_batch(cpu(*shape), wt)
    # what is not part of this call
    x = cpu(8, 8, 3)
    with pytest.raises(TypeError):
        W.denoise_batch(x, None)
    for th in (W.BiggestTH(), W.PosTH(), W.NegTH()):
        with pytest.raises(TypeError):
            W.denoise_batch(x, wt, dnt=W.VisuShrink(th, 1.0))
    with pytest.raises(TypeError):
        W.denoise_batch(x, wt, TI=True)
    # a host sigma is validated before anything is uploaded
    with pytest.raises(AssertionError):
        W.denoise_batch(x, wt, sigma=[0.1, -0.1, 0.2])
    with pytest.raises(AssertionError):
        W.denoise_batch(x, wt, sigma=np.array([0.1, float("nan"), 0.2]))
    with pytest.raises(W.DimensionMismatch):
        W.denoise_batch(x, wt, sigma=[0.1, 0.2])
    # valid arguments get as far as the device check, here without a device: no TypeError / ArgumentError / AssertionError
    if not torch.cuda.is_available():
        for call in (lambda: W.denoise_batch(x, wt, sigma=[0.1, 0.2, 0.3]), lambda: W.noisest_batch(x, wt),
                     lambda: W.denoise_batch(cpu(64, 2), LS.scheme(W, "cdf97"))):
            with pytest.raises(W.HIPError):
                call()
