"""wl_denoise_ti_batch_filter / wl_denoise_ti_batch_lifting (W.denoise_ti_batch) on the device.

Every value comparison is np.array_equal against the CPU oracle, unit by unit -- oracle.denoise(x_i, fwd, inv, L, kind, t_unit,
TI=True, nspin=..., sigma=...) with the unit's own oracle.noisest -- in the exact library, Float32 and Float64; sigmas are compared
as doubles with ==.  Inputs and case tables: tests/denoise_ti_batch_cases.py over the units of tests/denoise_batch_cases.py; the
conditions under which the fixture tells whose sigma was used are asserted on the oracle in tests/test_denoise_ti_batch_host.py.
"""
import ctypes as C

import numpy as np
import pytest

import denoise_batch_cases as DB
import denoise_ti_batch_cases as TB
import lifting_schemes as LS

pytestmark = pytest.mark.gpu

DTYPES = TB.DTYPES
SENTINEL = 12345.0
TH = {"hard": "HardTH", "soft": "SoftTH", "semisoft": "SemiSoftTH", "stein": "SteinTH"}


# ---- helpers -------------------------------------------------------------------------------------------------------------
def _ctx(W, x):
    from wavelets_jl_amd import transforms as TR
    return TR._context(x.device)


def _f64p(t):
    return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double)) if t is not None else None


def _dnt(W, kind, n):
    return W.VisuShrink(getattr(W, TH[kind])(), DB.t_unit(n))


def _wt(W, wname, lifting):
    return LS.scheme(W, wname) if lifting else W.wavelet(getattr(W.WT, wname))


def _run(W, torch, n, ndim, dtype, B, nspin, wname, kind, L, lifting=False, sigma=None):
    """W.denoise_ti_batch on the B units of the fixture -> (units of y on the host, sigmas used, kernel name); x must come back intact"""
    us = DB.units(n, ndim, dtype, B)
    x = DB.to_batch(W, us)
    y, sig = W.denoise_ti_batch(x, _wt(W, wname, lifting), L, _dnt(W, kind, n), nspin=nspin, sigma=sigma, return_sigma=True)
    torch.cuda.synchronize()
    assert np.array_equal(W.to_host(x), np.stack(us, axis=-1)), "x was modified"
    return W.to_host(y), sig.cpu().tolist(), W.last_kernel()


def _check(W, oracle, torch, n, ndim, dtype, B, nspin, wname, kind, L, lifting=False, opts=None):
    Lr = TB.level(oracle, n, L)
    for k, v in (opts or {}).items():
        W.set_option(k, v)
    got, sig, kernel = _run(W, torch, n, ndim, dtype, B, nspin, wname, kind, L, lifting)
    tag = (n, ndim, np.dtype(dtype).name, B, nspin, wname, kind, L, opts, kernel)
    assert kernel == "denoise_ti_units+k_mad_units_lds", tag
    assert sig == [DB.ref_sigma(oracle, W, n, ndim, dtype, i, wname, lifting) for i in range(B)], tag
    for i in range(B):
        e = TB.ref_ti(oracle, W, n, ndim, dtype, i, wname, Lr, kind, nspin, lifting)
        assert np.array_equal(got[..., i], e), tag + ("unit %d" % i, int((got[..., i] != e).sum()))
    return got


# ---- the tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ndim,B,nspin", TB.FILTER_CASES, ids=str)
def test_filter_cases(gpu, W, oracle, n, ndim, B, nspin):
    import torch
    for dt in DTYPES:
        for wname, kind, L in TB.FILTER_COMBOS:
            _check(W, oracle, torch, n, ndim, dt, B, nspin, wname, kind, L)


@pytest.mark.parametrize("n,ndim,B,nspin", TB.LIFTING_CASES, ids=str)
def test_lifting_cases(gpu, W, oracle, n, ndim, B, nspin):
    import torch
    for dt in DTYPES:
        for sname, kind in DB.lifting_combos(n, ndim):
            _check(W, oracle, torch, n, ndim, dt, B, nspin, sname, kind, None, lifting=True)


# ---- groups --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n,ndim,B,nspin,groups", [(64, 1, 5, (8,), (1, 5, 8, 16)), (8, 2, 5, (2, 3), (1, 5, 8, 16)), (1024, 1, 3, (3,), (4,))],
                         ids=str)
def test_groups_change_no_bit(gpu, W, oracle, n, ndim, B, nspin, groups, dtype):
    """WL_TI_BATCH_GROUP planes per group: 1; 5 -- groups begin inside a unit and hold parts of two units --; 8 -- exactly one unit of
    eight spins (six spins: a unit and a third) --; 16 -- several units and a shorter last group --; 4 with three spins -- the end of
    one unit, a whole unit in none, the start of the next.  Always against the ungrouped result and the oracle."""
    import torch
    for wname, kind, L, lifting in (("sym5", "hard", None, False), ("db8", "stein", 0, False), ("cdf97", "soft", None, True)):
        whole = _check(W, oracle, torch, n, ndim, dtype, B, nspin, wname, kind, L, lifting)
        for G in groups:
            part = _check(W, oracle, torch, n, ndim, dtype, B, nspin, wname, kind, L, lifting, opts={"WL_TI_BATCH_GROUP": G})
            assert np.array_equal(part, whole), (n, ndim, dtype.__name__, wname, G)
            W.clear_options()


def test_groups_under_the_workspace_cap(gpu, W, oracle):
    """WL_TI_WS_CAP_MB = 1 halves the 3 x 6 planes of 64 x 64 Float64 (32 KiB each, 5.5 planes' worth per plane held) into groups"""
    import torch
    _check(W, oracle, torch, 64, 2, np.float64, 3, (3, 2), "sym5", "hard", None, opts={"WL_TI_WS_CAP_MB": 1})


# ---- unit stride and padding through the ABI -----------------------------------------------------------------------------------
def _padded(torch, us, stride):
    N = us[0].size
    host = np.full(stride * len(us), SENTINEL, dtype=us[0].dtype)
    for i, u in enumerate(us):
        host[i * stride:i * stride + N] = np.asfortranarray(u).reshape(-1, order="F")
    return torch.from_numpy(host).cuda(), host


def _abi(W, torch, us, stride, nspin, wname, kind, L, lifting=False):
    """the entry point with a unit stride of its own -> (units of y, padding of y, sigmas)"""
    shape, B = us[0].shape, len(us)
    N = us[0].size
    xb, xh = _padded(torch, us, stride)
    yb = torch.full_like(xb, SENTINEL)
    sg = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    h, st = _ctx(W, xb)
    dims = (C.c_int64 * 3)(*(list(shape) + [1] * (3 - len(shape))))
    ns = (C.c_int64 * 3)(*(list(nspin) + [1] * (3 - len(nspin))))
    code = 0 if us[0].dtype == np.float32 else 1
    lib = W._lib.load()
    if lifting:
        sch = LS.scheme(W, wname)
        iu, nc, sh, cf = sch.flatten()
        i32 = C.POINTER(C.c_int32)
        rc = lib.wl_denoise_ti_batch_lifting(h, code, C.c_void_p(yb.data_ptr()), C.c_void_p(xb.data_ptr()), len(shape), dims, B, stride, len(iu),
                                             iu.ctypes.data_as(i32), nc.ctypes.data_as(i32), sh.ctypes.data_as(i32),
                                             cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1, sch.norm2, L, DB.KINDS.index(kind),
                                             DB.t_unit(shape[0]), ns, None, _f64p(sg), st)
    else:
        q = np.ascontiguousarray(W.wavelet(getattr(W.WT, wname)).qmf, dtype=np.float64)
        rc = lib.wl_denoise_ti_batch_filter(h, code, C.c_void_p(yb.data_ptr()), C.c_void_p(xb.data_ptr()), len(shape), dims, B, stride,
                                            q.ctypes.data_as(C.POINTER(C.c_double)), len(q), L, DB.KINDS.index(kind), DB.t_unit(shape[0]), ns,
                                            None, _f64p(sg), st)
    torch.cuda.synchronize()
    assert rc == 0, W._lib.STATUS.get(rc, rc)
    assert np.array_equal(xb.cpu().numpy(), xh), "x was modified"
    yh = yb.cpu().numpy()
    ys = [yh[i * stride:i * stride + N].reshape(shape, order="F") for i in range(B)]
    pad = np.concatenate([yh[i * stride + N:(i + 1) * stride] for i in range(B)])
    return ys, pad, sg.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n,ndim,B,nspin", [(64, 1, 5, (8,)), (8, 2, 5, (2, 3)), (8, 3, 3, (2, 1, 3))], ids=str)
def test_unit_stride_and_padding(gpu, W, oracle, n, ndim, B, nspin, dtype):
    """unit_stride = N + 4 and N + 1 (unit bases off the 16-byte grid): the bits of the dense batch, the padding of y untouched, x
    unmodified; whole and in groups of five planes"""
    import torch
    us = DB.units(n, ndim, dtype, B)
    N = us[0].size
    for wname, kind, L, lifting in (("sym5", "hard", None, False), ("db8", "stein", 0, False), ("cdf97", "hard", None, True)):
        Lr = TB.level(oracle, n, L)
        for stride in (N + 4, N + 1):
            for G in (0, 5):
                W.set_option("WL_TI_BATCH_GROUP", G)
                ys, pad, sg = _abi(W, torch, us, stride, nspin, wname, kind, Lr, lifting)
                tag = (n, ndim, dtype.__name__, wname, kind, L, stride, G)
                assert np.all(pad == SENTINEL), tag
                for i in range(B):
                    assert sg[i] == DB.ref_sigma(oracle, W, n, ndim, dtype, i, wname, lifting), tag + (i,)
                    assert np.array_equal(ys[i], TB.ref_ti(oracle, W, n, ndim, dtype, i, wname, Lr, kind, nspin, lifting)), tag + (i,)


# ---- sigma supplied by the caller ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_sigma_from_the_caller(gpu, W, oracle, dtype):
    import torch
    for n, ndim, B, nspin, wname, kind, lifting in ((64, 1, 5, (8,), "sym5", "hard", False), (8, 2, 5, (2, 3), "db2", "soft", False),
                                                    (8, 3, 3, (2, 1, 3), "cdf97", "hard", True)):
        L = DB.default_L(oracle, n)
        sig = [0.03 + 0.045 * ((3 * i) % B) for i in range(B)]
        exp = [TB.ref_ti(oracle, W, n, ndim, dtype, i, wname, L, kind, nspin, lifting, sigma=sig[i]) for i in range(B)]
        assert not np.array_equal(exp[0], TB.ref_ti(oracle, W, n, ndim, dtype, 0, wname, L, kind, nspin, lifting))
        for G in (0, 5):
            for s in (sig, np.array(sig), torch.tensor(sig, dtype=torch.float64, device="cuda")):
                W.set_option("WL_TI_BATCH_GROUP", G)
                got, used, kernel = _run(W, torch, n, ndim, dtype, B, nspin, wname, kind, L, lifting, sigma=s)
                assert kernel == "denoise_ti_units+sigma_in"
                assert used == sig
                for i in range(B):
                    assert np.array_equal(got[..., i], exp[i]), (n, ndim, dtype.__name__, wname, kind, G, i)
    # without sigma, what return_sigma gives back is noisest_batch
    x = DB.to_batch(W, DB.units(64, 2, dtype, 3))
    _, used = W.denoise_ti_batch(x, W.wavelet(W.WT.db2), nspin=(2, 2), return_sigma=True)
    assert torch.equal(used, W.noisest_batch(x, W.wavelet(W.WT.db2)))
    before = W.last_kernel()
    with pytest.raises(AssertionError):
        W.denoise_ti_batch(x, W.wavelet(W.WT.db2), sigma=[0.1, -0.2, 0.3])
    assert W.last_kernel() == before


# ---- a single spin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_a_single_spin_is_the_references_ti_branch(gpu, W, oracle, dtype):
    """nspin = (1,) and (1, 1): (0 + idwt(threshold!(dwt(x)))) * 1 -- the oracle's TI branch, where a -0.0 of the plain denoise comes
    back +0.0 -- at the default L and at L = 0"""
    import torch
    for n, ndim, B, nspin in ((64, 1, 5, (1,)), (8, 2, 5, (1, 1))):
        for wname, kind, L in (("sym5", "hard", None), ("db8", "stein", 0), ("haar", "soft", None)):
            got = _check(W, oracle, torch, n, ndim, dtype, B, nspin, wname, kind, L)
            assert not np.any(np.signbit(got) & (got == 0)), (n, ndim, wname)
        _check(W, oracle, torch, n, ndim, dtype, B, nspin, "cdf97", "hard", None, lifting=True)


# ---- against the loop of single translation-invariant calls -----------------------------------------------------------------------
@pytest.mark.parametrize("n,ndim,B,wname,nspin", [(64, 2, 16, "sym5", (4, 4)), (4096, 1, 8, "db4", (8,))], ids=str)
def test_equals_the_loop_of_single_calls(gpu, W, oracle, n, ndim, B, wname, nspin):
    """(the single Float32 image takes its virtual-shift, fused-threshold tier on the other side)"""
    import torch
    wt = W.wavelet(getattr(W.WT, wname))
    us = DB.units(n, ndim, np.float32, B)
    x = DB.to_batch(W, us)
    L = DB.default_L(oracle, n)
    dnt = _dnt(W, "hard", n)
    y = W.denoise_ti_batch(x, wt, L, dnt, nspin=nspin)
    loop = torch.stack([W.denoise(W.to_device(np.array(u)), wt, L, dnt, TI=True, nspin=nspin) for u in us], dim=-1)
    torch.cuda.synchronize()
    assert torch.equal(y, loop)
    got = W.to_host(y)
    for i in (1, B - 1):
        assert np.array_equal(got[..., i], TB.ref_ti(oracle, W, n, ndim, np.float32, i, wname, L, "hard", nspin)), (n, ndim, i)


# ---- hipGraph ----------------------------------------------------------------------------------------------------------------
def test_hipgraph_capture_and_replay(gpu, W, oracle):
    """after one warm call that grows the workspace the call allocates nothing and synchronises nothing: captured with
    torch.cuda.graph, replayed twice on refilled input, compared with the eager result and the oracle"""
    import torch
    n, ndim, B, dtype, wname, nspin = 8, 2, 5, np.float32, "sym5", (2, 3)
    wt = W.wavelet(W.WT.sym5)
    L = DB.default_L(oracle, n)
    us = DB.units(n, ndim, dtype, B)
    W.set_option("WL_TI_BATCH_GROUP", 5)                     # (groups that begin inside a unit, in the graph as well)
    s = torch.cuda.Stream()
    x = DB.to_batch(W, [np.zeros_like(u) for u in us])
    y = W.similar(x)
    with torch.cuda.stream(s):
        W.denoise_ti_batch(x, wt, L, nspin=nspin, y=y)       # (warm call: code objects loaded, the workspace grown)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        _, sg = W.denoise_ti_batch(x, wt, L, nspin=nspin, y=y, return_sigma=True)
    for order in ((0, 1, 2, 3, 4), (4, 3, 2, 1, 0)):
        x.copy_(DB.to_batch(W, [us[i] for i in order]))
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = W.to_host(y)
        assert sg.cpu().tolist() == [DB.ref_sigma(oracle, W, n, ndim, dtype, i, wname) for i in order]
        eager = W.denoise_ti_batch(x, wt, L, nspin=nspin)
        torch.cuda.synchronize()
        assert np.array_equal(got, W.to_host(eager)), order
        for k, i in enumerate(order):
            assert np.array_equal(got[..., k], TB.ref_ti(oracle, W, n, ndim, dtype, i, wname, L, "hard", nspin)), (order, k)
    del graph


# ---- argument contract on a live context -----------------------------------------------------------------------------------------
def test_argument_contract(gpu, W, oracle):
    """one ABI call per status code, in the documented order; y == x is WL_EALIAS for both entry points"""
    import torch
    lib, ST = W._lib.load(), W._lib.STATUS
    us = DB.units(16, 2, np.float32, 2)
    xb, _ = _padded(torch, us, 256)
    yb = torch.zeros_like(xb)
    h, st = _ctx(W, xb)
    q = np.ascontiguousarray(W.wavelet(W.WT.db2).qmf, dtype=np.float64)
    qp = q.ctypes.data_as(C.POINTER(C.c_double))

    def f(y=yb, x=xb, dtype=0, ndims=2, dims=(16, 16, 1), B=2, stride=256, flen=4, L=2, th=0, t=DB.t_unit(16), nspin=(2, 3, 1)):
        d = (C.c_int64 * 3)(*dims)
        ns = (C.c_int64 * 3)(*nspin) if nspin is not None else None
        return ST[lib.wl_denoise_ti_batch_filter(h, dtype, C.c_void_p(y.data_ptr()), C.c_void_p(x.data_ptr()), ndims, d, B, stride, qp, flen, L, th,
                                                 t, ns, None, None, st)]

    assert f(th=4, dtype=9) == f(t=-1.0, dtype=9) == f(nspin=None, dtype=9) == "WL_EINVAL_ARG"
    assert f(dtype=9, flen=1) == "WL_EINVAL_DTYPE"
    assert f(flen=1, dims=(16, 8, 1)) == "WL_EINVAL_FILTER"
    assert f(dims=(16, 8, 1), B=0) == "WL_EINVAL_CUBE"
    assert f(B=0, L=-1) == f(stride=255, L=-1) == f(nspin=(2, 0, 1), L=-1) == f(B=1 << 40, nspin=(1 << 12, 1 << 12, 1), L=-1) == "WL_EDIMS"
    assert f(L=-1, dims=(12, 12, 1), stride=144) == "WL_EINVAL_L"
    assert f(L=3, dims=(12, 12, 1), stride=144, y=xb) == "WL_EINVAL_SIZE"
    assert f(y=xb) == "WL_EALIAS"
    assert f() == "WL_OK"
    torch.cuda.synchronize()
    got = yb.cpu().numpy()
    for i in range(2):
        e = TB.ref_ti(oracle, W, 16, 2, np.float32, i, "db2", 2, "hard", (2, 3))
        assert np.array_equal(got[256 * i:256 * (i + 1)].reshape(16, 16, order="F"), e)
    sch = LS.scheme(W, "cdf97")
    iu, nc, sh, cf = sch.flatten()
    i32 = C.POINTER(C.c_int32)

    def g(y=yb, x=xb, dtype=0, dims=(16, 16, 1), B=2, stride=256, nsteps=len(iu), L=2, th=0, t=DB.t_unit(16), nspin=(2, 3, 1)):
        d = (C.c_int64 * 3)(*dims)
        ns = (C.c_int64 * 3)(*nspin) if nspin is not None else None
        return ST[lib.wl_denoise_ti_batch_lifting(h, dtype, C.c_void_p(y.data_ptr()), C.c_void_p(x.data_ptr()), 2, d, B, stride, nsteps,
                                                  iu.ctypes.data_as(i32), nc.ctypes.data_as(i32), sh.ctypes.data_as(i32),
                                                  cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1, sch.norm2, L, th, t, ns, None, None, st)]

    assert g(th=-1, dtype=9) == g(nspin=None, dtype=9) == "WL_EINVAL_ARG"
    assert g(dtype=9, nsteps=17) == "WL_EINVAL_DTYPE"
    assert g(nsteps=17, dims=(16, 8, 1)) == "WL_EINVAL_SCHEME"
    assert g(dims=(16, 8, 1), B=0) == "WL_EINVAL_CUBE"
    assert g(B=0, L=-1) == g(nspin=(0, 3, 1), L=-1) == "WL_EDIMS"
    assert g(L=-1, dims=(12, 12, 1), stride=144) == "WL_EINVAL_L"
    assert g(L=3, dims=(12, 12, 1), stride=144, y=xb) == "WL_EINVAL_SIZE"
    assert g(y=xb) == "WL_EALIAS"                           # x is re-read for every group of spins: no in-place form
    assert g() == "WL_OK"
    torch.cuda.synchronize()
    e = TB.ref_ti(oracle, W, 16, 2, np.float32, 1, "cdf97", 2, "hard", (2, 3), True)
    assert np.array_equal(yb.cpu().numpy()[256:512].reshape(16, 16, order="F"), e)


# ---- wl_last_kernel --------------------------------------------------------------------------------------------------------------
def test_last_kernel_names_the_batch_and_the_mad_tier(gpu, W, oracle):
    import torch
    n, ndim, B, nspin = 64, 1, 5, (8,)
    x = DB.to_batch(W, DB.units(n, ndim, np.float32, B))
    wt = W.wavelet(W.WT.sym5)
    whole = W.denoise_ti_batch(x, wt, nspin=nspin)
    assert W.last_kernel() == "denoise_ti_units+k_mad_units_lds"
    W.set_option("WL_MAD_LDS_MAX", 0)
    stream = W.denoise_ti_batch(x, wt, nspin=nspin)
    assert W.last_kernel() == "denoise_ti_units+k_mad_units_stream"
    assert torch.equal(whole, stream)
    W.denoise_ti_batch(x, wt, nspin=nspin, sigma=[0.1] * B)
    assert W.last_kernel() == "denoise_ti_units+sigma_in"
    e = TB.ref_ti(oracle, W, n, ndim, np.float32, 2, "sym5", DB.default_L(oracle, n), "hard", nspin)
    assert np.array_equal(W.to_host(whole)[..., 2], e)
