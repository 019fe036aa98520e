"""wl_mad_batch, wl_denoise_batch_filter, wl_denoise_batch_lifting (W.denoise_batch / W.noisest_batch / W.mad_batch_) on the device.

Every value comparison is np.array_equal against the CPU oracle, unit by unit -- oracle.denoise(x_i, fwd, inv, L, kind, t_unit[,
sigma=]), oracle.noisest, oracle.mad -- and sigmas are compared as doubles with ==.  Inputs, case tables and the shared references:
tests/denoise_batch_cases.py; the conditions under which its fixture tells "own sigma" from "somebody's sigma" are asserted on the
oracle's values (DB.check_fixture) before a case looks at the device.
"""
import ctypes as C

import numpy as np
import pytest

import denoise_batch_cases as DB
import lifting_schemes as LS

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SENTINEL = 12345.0
LDS_MAX = {np.float32: 8192, np.float64: 4096}


# ---- helpers -------------------------------------------------------------------------------------------------------------
def _ctx(W, x):
    from wavelets_jl_amd import transforms as TR
    return TR._context(x.device)


def _f64p(t):
    return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double)) if t is not None else None


def _padded(W, torch, us, stride):
    """the units of a batch `stride` elements apart in one device buffer, the padding filled with the sentinel"""
    N = us[0].size
    host = np.full(stride * len(us), SENTINEL, dtype=us[0].dtype)
    for i, u in enumerate(us):
        host[i * stride:i * stride + N] = np.asfortranarray(u).reshape(-1, order="F")
    return torch.from_numpy(host).cuda(), host


def _units_of(host, shape, stride, B):
    N = int(np.prod(shape))
    return [host[i * stride:i * stride + N].reshape(shape, order="F") for i in range(B)], \
           np.concatenate([host[i * stride + N:(i + 1) * stride] for i in range(B)])


def _mad_batch(W, torch, vals, stride):
    """wl_mad_batch on B units of n values -> (results, overwritten units, padding, kernel name)"""
    B, n = len(vals), vals[0].size
    buf, _ = _padded(W, torch, vals, stride)
    res = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    h, st = _ctx(W, buf)
    rc = W._lib.load().wl_mad_batch(h, 0 if vals[0].dtype == np.float32 else 1, C.c_void_p(buf.data_ptr()), n, B, stride, _f64p(res), st)
    assert rc == 0, W._lib.STATUS.get(rc, rc)
    torch.cuda.synchronize()
    ys, pad = _units_of(buf.cpu().numpy(), (n,), stride, B)
    return res.cpu().numpy(), ys, pad, W.last_kernel()


def _check_mad(W, oracle, torch, vals, stride, want_kernel):
    res, ys, pad, k = _mad_batch(W, torch, vals, stride)
    tag = (vals[0].dtype.name, vals[0].size, len(vals), stride)
    assert k == want_kernel, tag + (k,)
    assert np.all(pad == SENTINEL), tag
    for i, v in enumerate(vals):
        e = oracle.mad(v)
        if np.isnan(e):
            assert np.isnan(res[i]), tag + (i,)
            continue
        assert res[i] == e, tag + (i, res[i], e)
        m = v.dtype.type(oracle.median(v))
        assert np.array_equal(ys[i], np.abs(v - m)), tag + (i,)
        d = W.to_device(v.copy())                            # device against device: the single-vector mad! of the library
        assert W.mad_(d) == res[i], tag + (i,)
        assert np.array_equal(W.to_host(d), ys[i]), tag + (i,)


def _vals(n, B, dtype, seed=0):
    r = np.random.default_rng(7000 + 31 * n + seed)
    return [(r.standard_normal(n) * (1 + i)).astype(dtype) + dtype(0.25 * i) for i in range(B)]


# ---- wl_mad_batch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n", [1, 2, 3, 64, 1000, 4096, 4097, 8192, 8193, 20000])
def test_mad_batch(gpu, W, oracle, n, dtype):
    import torch
    want = "k_mad_units_lds" if n <= LDS_MAX[dtype] else "k_mad_units_stream"
    for B in (1, 3, 70):
        vals = _vals(n, B, dtype)
        for stride in (n, n + 5):
            _check_mad(W, oracle, torch, vals, stride, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n", [1, 2, 3, 64, 1000])
def test_mad_batch_streaming_kernel_at_small_n(gpu, W, oracle, n, dtype):
    import torch
    W.set_option("WL_MAD_LDS_MAX", 0)
    for B in (1, 3, 70):
        vals = _vals(n, B, dtype, seed=1)
        for stride in (n, n + 5):
            _check_mad(W, oracle, torch, vals, stride, "k_mad_units_stream")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("lds_max", [None, 0], ids=["lds", "stream"])
def test_mad_batch_radix_prefix_stress(gpu, W, oracle, lds_max, dtype):
    """many ties, a constant unit (MAD exactly 0), mixed signed zeros, and one unit with a NaN whose result alone is NaN"""
    import torch
    if lds_max is not None:
        W.set_option("WL_MAD_LDS_MAX", lds_max)
    want = "k_mad_units_lds" if lds_max is None else "k_mad_units_stream"
    r = np.random.default_rng(77)
    for n in (7, 1000, 1001):
        ties = (np.round(r.standard_normal(n) * 4) / 4).astype(dtype)
        const = np.full(n, 1.75, dtype=dtype)
        zeros = np.where(r.random(n) < 0.5, 0.0, -0.0).astype(dtype)
        zeros2 = zeros.copy()
        zeros2[: n // 3] = r.standard_normal(n // 3).astype(dtype)
        nan = r.standard_normal(n).astype(dtype)
        nan[n // 2] = np.nan
        vals = [ties, const, zeros, nan, zeros2, (ties * 3).astype(dtype)]
        assert oracle.mad(const) == 0.0 and np.isnan(oracle.mad(nan))
        res, _, _, _ = _mad_batch(W, torch, vals, n + 3)
        assert np.isnan(res[3]) and not np.any(np.isnan(np.delete(res, 3)))
        _check_mad(W, oracle, torch, vals, n + 3, want)
        _check_mad(W, oracle, torch, vals, n, want)


def test_noisest_batch(gpu, W, oracle):
    import torch
    for n, ndim, B, dtype, wname in ((64, 1, 5, np.float32, "sym5"), (64, 2, 5, np.float64, "db2"), (8, 3, 3, np.float32, "haar")):
        s = W.noisest_batch(DB.to_batch(W, DB.units(n, ndim, dtype, B)), W.wavelet(getattr(W.WT, wname)))
        assert s.dtype == torch.float64 and tuple(s.shape) == (B,)
        assert s.cpu().tolist() == [DB.ref_sigma(oracle, W, n, ndim, dtype, i, wname) for i in range(B)]
    sch = LS.scheme(W, "cdf97")
    s = W.noisest_batch(DB.to_batch(W, DB.units(64, 2, np.float32, 3)), sch)
    assert s.cpu().tolist() == [DB.ref_sigma(oracle, W, 64, 2, np.float32, i, "cdf97", True) for i in range(3)]


# ---- denoise_batch, orthogonal filters ---------------------------------------------------------------------------------
TH = {"hard": "HardTH", "soft": "SoftTH", "semisoft": "SemiSoftTH", "stein": "SteinTH"}


def _dnt(W, kind, n):
    return W.VisuShrink(getattr(W, TH[kind])(), DB.t_unit(n))


def _check_batch(W, oracle, torch, n, ndim, dtype, B, wname, kind, L, lifting=False, inplace=False):
    Ld = DB.default_L(oracle, n)
    if L is None or L == Ld:
        DB.check_fixture(oracle, W, n, ndim, dtype, B, wname, Ld, kind, lifting)
    Lr = Ld if L is None else L
    us = DB.units(n, ndim, dtype, B)
    x = DB.to_batch(W, us)
    wt = LS.scheme(W, wname) if lifting else W.wavelet(getattr(W.WT, wname))
    y, sig = W.denoise_batch(x, wt, L, _dnt(W, kind, n), y=x if inplace else None, return_sigma=True)
    torch.cuda.synchronize()
    tag = (n, ndim, np.dtype(dtype).name, B, wname, kind, L, W.last_kernel())
    nd = n // 2
    want = "denoise_batch+" + ("k_mad_units_lds" if nd <= LDS_MAX[dtype] else "k_mad_units_stream")
    assert W.last_kernel() == want, tag
    assert sig.cpu().tolist() == [DB.ref_sigma(oracle, W, n, ndim, dtype, i, wname, lifting) for i in range(B)], tag
    got = W.to_host(y)
    for i in range(B):
        e = DB.ref_denoise(oracle, W, n, ndim, dtype, i, wname, Lr, kind, lifting)
        assert np.array_equal(got[..., i], e), tag + ("unit %d" % i, int((got[..., i] != e).sum()))
    if not inplace:
        assert np.array_equal(W.to_host(x), np.stack(us, axis=-1)), tag + ("x was modified",)


@pytest.mark.parametrize("n,ndim,B,dtypes", DB.FILTER_SHAPES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_denoise_batch_filter(gpu, W, oracle, n, ndim, B, dtypes):
    import torch
    for dt in dtypes:
        for wname, kind, L in DB.filter_combos(n, ndim):
            _check_batch(W, oracle, torch, n, ndim, np.dtype(dt).type, B, wname, kind, L)


def _abi_filter(W, torch, us, stride, wname, kind, L, sigma_in=None, y_is_x=False):
    """wl_denoise_batch_filter through the ABI with a unit stride of its own -> (units of y, padding of y, sigmas, status)"""
    shape, B = us[0].shape, len(us)
    xb, xh = _padded(W, torch, us, stride)
    yb = xb if y_is_x else torch.full_like(xb, SENTINEL)
    sg = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    q = np.ascontiguousarray(W.wavelet(getattr(W.WT, wname)).qmf, dtype=np.float64)
    h, st = _ctx(W, xb)
    dims = (C.c_int64 * 3)(*(list(shape) + [1] * (3 - len(shape))))
    rc = W._lib.load().wl_denoise_batch_filter(h, 0 if us[0].dtype == np.float32 else 1, C.c_void_p(yb.data_ptr()), C.c_void_p(xb.data_ptr()),
                                               len(shape), dims, B, stride, q.ctypes.data_as(C.POINTER(C.c_double)), len(q), L,
                                               DB.KINDS.index(kind), DB.t_unit(shape[0]), _f64p(sigma_in), _f64p(sg), st)
    torch.cuda.synchronize()
    if rc:
        return None, None, None, W._lib.STATUS[rc]
    assert np.array_equal(xb.cpu().numpy(), xh), "x was modified"
    ys, pad = _units_of(yb.cpu().numpy(), shape, stride, B)
    return ys, pad, sg.cpu().numpy(), "WL_OK"


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n,ndim,B", [(64, 1, 5), (8, 2, 5), (64, 2, 5), (8, 3, 3), (32, 3, 3)])
def test_unit_stride_and_padding(gpu, W, oracle, n, ndim, B, dtype):
    """unit_stride = N + 4 and N + 1 (unit bases off the 16-byte grid): the bits of the dense batch, the padding of y untouched"""
    import torch
    us = DB.units(n, ndim, dtype, B)
    N = us[0].size
    for wname, kind, L in (("sym5", "hard", None), ("db8", "soft", 1), ("haar", "stein", 0)):
        Lr = DB.default_L(oracle, n) if L is None else L
        for stride in (N + 4, N + 1):
            ys, pad, sg, rc = _abi_filter(W, torch, us, stride, wname, kind, Lr)
            tag = (n, ndim, dtype.__name__, wname, kind, L, stride)
            assert rc == "WL_OK", tag + (rc,)
            assert np.all(pad == SENTINEL), tag
            for i in range(B):
                assert sg[i] == DB.ref_sigma(oracle, W, n, ndim, dtype, i, wname), tag + (i,)
                assert np.array_equal(ys[i], DB.ref_denoise(oracle, W, n, ndim, dtype, i, wname, Lr, kind)), tag + (i,)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_groups_change_no_bit(gpu, W, oracle, dtype):
    """WL_TI_WS_CAP_MB = 1: the three 256 x 256 units (256 KiB / 512 KiB of coefficients each) run in several groups"""
    import torch
    W.set_option("WL_TI_WS_CAP_MB", 1)
    _check_batch(W, oracle, torch, 256, 2, dtype, 3, "sym5", "hard", None)
    _check_batch(W, oracle, torch, 256, 2, dtype, 3, "cdf97", "hard", None, lifting=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_a_group_of_several_units_and_a_shorter_last_group(gpu, W, oracle, dtype):
    """five 128 x 128 units under a cap of 1 MiB (Float32) / 2 MiB (Float64): a group of three units, then one of two, so the
    second group starts at unit 3 of x, y, sigma_in and sigma_out and its box is shorter than the buffers were carved for.
    Per unit the filter form needs 4.5 N elements (transform workspace 3.5 N, C N) and the lifting form 4 N, N = 16384: three
    units take 864 KiB / 768 KiB of Float32 (twice that of Float64) and fit, five (the first try) and four do not, so G = 3."""
    import torch
    n, B = 128, 5
    W.set_option("WL_TI_WS_CAP_MB", 1 if dtype is np.float32 else 2)
    _check_batch(W, oracle, torch, n, 2, dtype, B, "sym5", "hard", None)
    _check_batch(W, oracle, torch, n, 2, dtype, B, "db2", "soft", 0)           # (L = 0: the level-1 batch of the estimate, y a copy of x)
    _check_batch(W, oracle, torch, n, 2, dtype, B, "cdf97", "hard", None, lifting=True)
    # the caller's sigmas: unit 3 must get sigma_in[3], not the first entry again
    L = DB.default_L(oracle, n)
    sig = [0.03 + 0.045 * ((3 * i) % B) for i in range(B)]
    x = DB.to_batch(W, DB.units(n, 2, dtype, B))
    y, used = W.denoise_batch(x, W.wavelet(W.WT.sym5), L, _dnt(W, "hard", n), sigma=sig, return_sigma=True)
    torch.cuda.synchronize()
    assert used.cpu().tolist() == sig
    got = W.to_host(y)
    for i in range(B):
        assert np.array_equal(got[..., i], DB.ref_denoise(oracle, W, n, 2, dtype, i, "sym5", L, "hard", sigma=sig[i])), (dtype.__name__, i)


# ---- sigma supplied by the caller ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_sigma_from_the_caller(gpu, W, oracle, dtype):
    import torch
    for n, ndim, B, wname, kind, lifting in ((64, 1, 5, "sym5", "hard", False), (64, 2, 5, "db2", "soft", False), (8, 3, 3, "haar", "stein", False),
                                             (64, 2, 3, "cdf97", "hard", True)):
        L = DB.default_L(oracle, n)
        sig = [0.03 + 0.045 * ((3 * i) % B) for i in range(B)]
        wt = LS.scheme(W, wname) if lifting else W.wavelet(getattr(W.WT, wname))
        x = DB.to_batch(W, DB.units(n, ndim, dtype, B))
        exp = [DB.ref_denoise(oracle, W, n, ndim, dtype, i, wname, L, kind, lifting, sigma=sig[i]) for i in range(B)]
        assert not np.array_equal(exp[0], DB.ref_denoise(oracle, W, n, ndim, dtype, 0, wname, L, kind, lifting))
        for s in (sig, np.array(sig), torch.tensor(sig, dtype=torch.float64, device="cuda")):
            y, used = W.denoise_batch(x, wt, L, _dnt(W, kind, n), sigma=s, return_sigma=True)
            torch.cuda.synchronize()
            assert W.last_kernel() == "denoise_batch+sigma_in"
            assert used.cpu().tolist() == sig
            got = W.to_host(y)
            for i in range(B):
                assert np.array_equal(got[..., i], exp[i]), (n, ndim, dtype.__name__, wname, kind, i)
    before = W.last_kernel()
    with pytest.raises(AssertionError):
        W.denoise_batch(x, wt, L, _dnt(W, kind, n), sigma=[0.1, -0.2, 0.3])
    assert W.last_kernel() == before


# ---- lifting schemes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n,ndim,B", DB.LIFTING_SHAPES)
def test_denoise_batch_lifting(gpu, W, oracle, n, ndim, B, dtype):
    import torch
    for sname, kind in DB.lifting_combos(n, ndim):
        _check_batch(W, oracle, torch, n, ndim, dtype, B, sname, kind, None, lifting=True)
        _check_batch(W, oracle, torch, n, ndim, dtype, B, sname, kind, None, lifting=True, inplace=True)
    _check_batch(W, oracle, torch, n, ndim, dtype, B, "cdf97", "soft", 1, lifting=True)
    _check_batch(W, oracle, torch, n, ndim, dtype, B, "twin_cdf97", "hard", 0, lifting=True, inplace=True)
    _check_batch(W, oracle, torch, n, ndim, dtype, B, "db2", "stein", 0, lifting=True)


# ---- against the loop of single denoise calls ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,ndim,B,wname", [(512, 2, 16, "sym5"), (1 << 17, 1, 8, "db4")])
def test_equals_the_loop_of_single_calls(gpu, W, oracle, n, ndim, B, wname):
    import torch
    wt = W.wavelet(getattr(W.WT, wname))
    us = DB.units(n, ndim, np.float32, B)
    x = DB.to_batch(W, us)
    y = W.denoise_batch(x, wt)
    loop = torch.stack([W.denoise(W.to_device(np.array(u)), wt) for u in us], dim=-1)
    torch.cuda.synchronize()
    assert torch.equal(y, loop)
    got = W.to_host(y)
    for i in (1, B - 1):
        e = DB.ref_denoise(oracle, W, n, ndim, np.float32, i, wname, 6, "hard")
        assert np.array_equal(got[..., i], e), (n, ndim, i)


# ---- hipGraph ----------------------------------------------------------------------------------------------------------------
def test_hipgraph_capture_and_replay(gpu, W, oracle):
    """after one warm call that grows the workspace the call allocates nothing and synchronises nothing: captured with
    torch.cuda.graph, replayed on refilled input, compared with the oracle"""
    import torch
    n, ndim, B, dtype, wname = 64, 2, 5, np.float32, "sym5"
    wt = W.wavelet(W.WT.sym5)
    L = DB.default_L(oracle, n)
    us = DB.units(n, ndim, dtype, B)
    s = torch.cuda.Stream()
    x = DB.to_batch(W, [np.zeros_like(u) for u in us])
    y = W.similar(x)
    sg = None
    with torch.cuda.stream(s):
        W.denoise_batch(x, wt, L, y=y)                       # (warm call: code objects loaded, the workspace grown)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        _, sg = W.denoise_batch(x, wt, L, y=y, return_sigma=True)
    for order in ((0, 1, 2, 3, 4), (4, 3, 2, 1, 0)):
        x.copy_(DB.to_batch(W, [us[i] for i in order]))
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = W.to_host(y)
        assert sg.cpu().tolist() == [DB.ref_sigma(oracle, W, n, ndim, dtype, i, wname) for i in order]
        for k, i in enumerate(order):
            assert np.array_equal(got[..., k], DB.ref_denoise(oracle, W, n, ndim, dtype, i, wname, L, "hard")), (order, k)
    del graph


# ---- argument contract on a live context -----------------------------------------------------------------------------------------
def test_argument_contract(gpu, W, oracle):
    """one ABI call per status code, in the documented order; y == x is WL_EALIAS for the filter form and accepted for lifting"""
    import torch
    lib, ST = W._lib.load(), W._lib.STATUS
    us = DB.units(16, 2, np.float32, 2)
    xb, _ = _padded(W, torch, us, 256)
    yb = torch.zeros_like(xb)
    h, st = _ctx(W, xb)
    q = np.ascontiguousarray(W.wavelet(W.WT.db2).qmf, dtype=np.float64)
    qp = q.ctypes.data_as(C.POINTER(C.c_double))

    def f(y=yb, x=xb, dtype=0, ndims=2, dims=(16, 16, 1), B=2, stride=256, flen=4, L=2, th=0, t=DB.t_unit(16)):
        d = (C.c_int64 * 3)(*dims)
        return ST[lib.wl_denoise_batch_filter(h, dtype, C.c_void_p(y.data_ptr()), C.c_void_p(x.data_ptr()), ndims, d, B, stride, qp, flen, L, th, t,
                                              None, None, st)]

    assert f(th=4, dtype=9) == f(t=-1.0, dtype=9) == "WL_EINVAL_ARG"
    assert f(dtype=9, flen=1) == "WL_EINVAL_DTYPE"
    assert f(flen=1, dims=(16, 8, 1)) == "WL_EINVAL_FILTER"
    assert f(dims=(16, 8, 1), B=0) == "WL_EINVAL_CUBE"
    assert f(B=0, L=-1) == f(stride=255, L=-1) == "WL_EDIMS"
    assert f(L=-1, dims=(12, 12, 1), stride=144) == "WL_EINVAL_L"
    assert f(L=3, dims=(12, 12, 1), stride=144, y=xb) == "WL_EINVAL_SIZE"
    assert f(y=xb) == "WL_EALIAS"
    assert f() == "WL_OK"
    sch = LS.scheme(W, "cdf97")
    iu, nc, sh, cf = sch.flatten()
    i32 = C.POINTER(C.c_int32)

    def g(y=yb, x=xb, dtype=0, dims=(16, 16, 1), B=2, stride=256, nsteps=len(iu), L=2, th=0, t=DB.t_unit(16)):
        d = (C.c_int64 * 3)(*dims)
        return ST[lib.wl_denoise_batch_lifting(h, dtype, C.c_void_p(y.data_ptr()), C.c_void_p(x.data_ptr()), 2, d, B, stride, nsteps,
                                               iu.ctypes.data_as(i32), nc.ctypes.data_as(i32), sh.ctypes.data_as(i32),
                                               cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1, sch.norm2, L, th, t, None, None, st)]

    assert g(th=-1, dtype=9) == "WL_EINVAL_ARG"
    assert g(dtype=9, nsteps=17) == "WL_EINVAL_DTYPE"
    assert g(nsteps=17, dims=(16, 8, 1)) == "WL_EINVAL_SCHEME"
    assert g(dims=(16, 8, 1), B=0) == "WL_EINVAL_CUBE"
    assert g(B=0, L=-1) == "WL_EDIMS"
    assert g(L=-1, dims=(12, 12, 1), stride=144) == "WL_EINVAL_L"
    assert g(L=3, dims=(12, 12, 1), stride=144) == "WL_EINVAL_SIZE"
    assert g() == "WL_OK"
    torch.cuda.synchronize()
    out_of_place = yb.cpu().numpy().copy()
    assert g(y=xb) == "WL_OK"                               # in place: accepted, the same bits
    torch.cuda.synchronize()
    assert np.array_equal(xb.cpu().numpy(), out_of_place)
    e = DB.ref_denoise(oracle, W, 16, 2, np.float32, 1, "cdf97", 2, "hard", True)
    assert np.array_equal(out_of_place[256:512].reshape(16, 16, order="F"), e)
