"""wl_dwt_lifting_batch (W.dwt_batch / W.idwt_batch with a GLS): a batch of square images through the 2-D lifting tiers, every
level one launch over all images.

Every comparison is np.array_equal against the oracle, image by image: oracle.dwt_lifting(x_i, scheme, L, fw); the inverse input
is the oracle's forward output.  Schemes come from tests/lifting_schemes.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

import lifting_schemes as LS
from conftest import rng_array

pytestmark = pytest.mark.gpu

SENT_X, SENT_Y, SENT_G = 7.0, -3.0, 123456.0


# ---- helpers -------------------------------------------------------------------------------------------------------------
def _images(n, nb, dtype, seed):
    return [rng_array((n, n), dtype, seed + i) for i in range(nb)]


def _to_batch(torch, gpu, imgs):
    """n x n x B column-major device tensor (image i = t[:, :, i])"""
    a = np.stack([np.ascontiguousarray(im.T) for im in imgs])              # [i][c][r]
    t = torch.from_numpy(a).to(gpu).permute(2, 1, 0)
    n = imgs[0].shape[0]
    assert t.stride() == (1, n, n * n)
    return t


def _from_batch(t):
    return [a.T for a in t.permute(2, 1, 0).contiguous().cpu().numpy()]


def _expected(oracle, imgs, sch, L, fw):
    return [oracle.dwt_lifting(a, sch, L, fw=fw) for a in imgs]


def _check_batch(W, oracle, torch, gpu, n, nb, L, sname, dtype, seed=1000, inplace=False):
    """forward and inverse of one case against the oracle; returns (forward kernel, inverse kernel)"""
    sch = LS.scheme(W, sname)
    xs = _images(n, nb, dtype, seed)
    fwd = _expected(oracle, xs, sch, L, True)
    kernels = []
    for fw, ins, exp in ((True, xs, fwd), (False, fwd, _expected(oracle, fwd, sch, L, False))):
        xb = _to_batch(torch, gpu, ins)
        f = W.dwt_batch if fw else W.idwt_batch
        yb = f(xb, sch, L, y=xb) if inplace else f(xb, sch, L)
        torch.cuda.synchronize()
        kernels.append(W.last_kernel())
        if inplace:
            assert yb.data_ptr() == xb.data_ptr()
        got = _from_batch(yb)
        for i in range(nb):
            assert np.array_equal(got[i], exp[i]), (sname, n, nb, L, dtype.__name__, "fw" if fw else "inv", "image %d" % i, kernels[-1])
        if not inplace:                                                      # the source of an out-of-place call is left alone
            back = _from_batch(xb)
            assert all(np.array_equal(back[i], ins[i]) for i in range(nb)), (sname, n, "source modified")
    return tuple(kernels)


def _single_kernel(W, torch, gpu, n, L, sname, dtype, fw):
    """W.last_kernel() after a single-image call of the same size, depth, scheme and direction"""
    sch = LS.scheme(W, sname)
    x = W.to_device(rng_array((n, n), dtype, 5))
    (W.dwt if fw else W.idwt)(x, sch, L)
    torch.cuda.synchronize()
    return W.last_kernel()


def _raw_call(W, gpu, yb, xb, n, nb, stride, sch, L, fw, dtype, dims=None, nsteps=None, dtype_code=None, ctx="ctx", ncoef=None):
    lib = W._lib.load()
    h, st = W.transforms._context(gpu)
    iu, nc, sh, cf = sch.flatten()
    if ncoef is not None:
        nc = np.asarray(ncoef, dtype=np.int32)
    d = None if dims == "null" else (C.c_int64 * 2)(*(dims if dims is not None else (n, n)))
    code = (0 if dtype == np.float32 else 1) if dtype_code is None else dtype_code
    i32 = C.POINTER(C.c_int32)
    return lib.wl_dwt_lifting_batch(h if ctx == "ctx" else ctx, code, C.c_void_p(yb) if yb is not None else None,
                                    C.c_void_p(xb) if xb is not None else None, d, nb, stride,
                                    len(iu) if nsteps is None else nsteps, iu.ctypes.data_as(i32), nc.ctypes.data_as(i32),
                                    sh.ctypes.data_as(i32), cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1, sch.norm2, L, fw, st)


# ---- every tier, table schemes -------------------------------------------------------------------------------------------
TIER_CASES = [
    # (scheme, n, images, L, dtype)
    ("cdf97", 4096, 2, 12, np.float32),          # fused level kernel (k_lift2d_fwd / _inv) down to the tiles and the tail
    ("db2", 1024, 3, 10, np.float32),            # tiles, two-level tiles
    ("cdf97", 2048, 2, 3, np.float32),
    ("haar", 256, 7, 8, np.float32),
    ("cdf97", 128, 9, 7, np.float32),            # tails
    ("cdf97", 64, 33, 6, np.float32),
    ("cdf97", 8, 5, 3, np.float32),
    ("cdf97", 2, 3, 1, np.float32),
    ("cdf97", 512, 5, 4, np.float64),
    ("db2", 256, 6, 8, np.float64),
    ("haar", 64, 9, 6, np.float64),
]


@pytest.mark.parametrize("sname,n,nb,L,dtype", TIER_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_every_tier_table_schemes(gpu, W, oracle, sname, n, nb, L, dtype):
    import torch
    kf, ki = _check_batch(W, oracle, torch, gpu, n, nb, L, sname, dtype)
    # dense, aligned batches take the tier of the single image -- never the two-pass or the one-thread-per-element route
    assert kf == _single_kernel(W, torch, gpu, n, L, sname, dtype, True), (kf, sname, n, L)
    assert ki == _single_kernel(W, torch, gpu, n, L, sname, dtype, False), (ki, sname, n, L)
    for k in (kf, ki):
        assert k != "k_lift_any" and not k.startswith("k_generic_lift"), (k, sname, n, L)


@pytest.mark.parametrize("sname,n,nb,L,dtype", [("cdf97", 96, 4, 5, np.float32), ("db2", 200, 3, 3, np.float32), ("cdf97", 1000, 2, 3, np.float32),
                                                ("cdf97", 96, 4, 5, np.float64)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_even_sizes_that_are_not_powers_of_two(gpu, W, oracle, sname, n, nb, L, dtype):
    import torch
    _check_batch(W, oracle, torch, gpu, n, nb, L, sname, dtype)


@pytest.mark.parametrize("sname", ["twin_cdf97", "twin_db2", "twin_haar"])
def test_shape_twins(gpu, W, oracle, sname):
    import torch
    kf, ki = _check_batch(W, oracle, torch, gpu, 256, 3, 8, sname, np.float32)
    assert kf == _single_kernel(W, torch, gpu, 256, 8, sname, np.float32, True) and kf == "k_lift2d_tile", kf
    assert ki == _single_kernel(W, torch, gpu, 256, 8, sname, np.float32, False) and ki == "k_lift2d_tile", ki


@pytest.mark.parametrize("sname", ["nc3", "shift5", "sixteen", "zero_steps"])
@pytest.mark.parametrize("n,nb,L", [(64, 6, 6), (256, 3, 3)])
def test_custom_schemes(gpu, W, oracle, sname, n, nb, L):
    """schemes of no known shape: the generic kernels with the images as the third extent"""
    import torch
    _check_batch(W, oracle, torch, gpu, n, nb, L, sname, np.float32)


# ---- degenerate ----------------------------------------------------------------------------------------------------------
def test_degenerate_cases(gpu, W, oracle):
    import torch
    sch = LS.scheme(W, "cdf97")
    # one image: the bits (and the kernel) of wl_dwt_lifting_oop
    for n, L in ((512, 9), (64, 6), (1000, 3)):
        a = rng_array((n, n), np.float32, 31)
        xb = _to_batch(torch, gpu, [a])
        yb = W.dwt_batch(xb, sch, L)
        kb = W.last_kernel()
        y1 = W.dwt(W.to_device(a), sch, L)
        assert kb == W.last_kernel()
        assert np.array_equal(_from_batch(yb)[0], W.to_host(y1)) and np.array_equal(W.to_host(y1), oracle.dwt_lifting(a, sch, L))
        xr = W.idwt_batch(yb, sch, L)
        kb = W.last_kernel()
        x1 = W.idwt(y1, sch, L)
        assert kb == W.last_kernel()
        assert np.array_equal(_from_batch(xr)[0], W.to_host(x1))
    # L = 0 copies
    xs = _images(64, 5, np.float32, 77)
    xb = _to_batch(torch, gpu, xs)
    for f in (W.dwt_batch, W.idwt_batch):
        yb = f(xb, sch, 0)
        assert yb.data_ptr() != xb.data_ptr() and all(np.array_equal(g, a) for g, a in zip(_from_batch(yb), xs))
    # partial depth
    _check_batch(W, oracle, torch, gpu, 1024, 2, 2, "cdf97", np.float32)


@pytest.mark.parametrize("n,nb", [(512, 4), (64, 8)])
def test_in_place(gpu, W, oracle, n, nb):
    """y == x: dwt!(y, scheme, L) of every image, both directions"""
    import torch
    _check_batch(W, oracle, torch, gpu, n, nb, W.maxtransformlevels(n), "cdf97", np.float32, inplace=True)
    _check_batch(W, oracle, torch, gpu, n, nb, 2, "cdf97", np.float32, inplace=True)


# ---- padded / misaligned image stride, guard bands -----------------------------------------------------------------------
@pytest.mark.parametrize("pad", [64, 10, 3])
@pytest.mark.parametrize("n,nb,L,sname,dtype", [(256, 3, 8, "cdf97", np.float32), (64, 5, 6, "cdf97", np.float32), (512, 2, 3, "db2", np.float32),
                                                (128, 3, 7, "cdf97", np.float64), (96, 3, 5, "cdf97", np.float32), (64, 4, 6, "nc3", np.float32),
                                                (256, 3, 0, "cdf97", np.float32)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_padded_image_stride_and_guard_bands(gpu, W, oracle, pad, n, nb, L, sname, dtype):
    """image_stride = n^2 + pad through ctypes (pad 3 breaks the 16-byte alignment of every second image); x and y sit inside larger
    allocations filled with a sentinel: results exact, padding in y untouched, nothing outside [0, nimages * image_stride) of y
    written, x untouched altogether"""
    import torch
    td = torch.float32 if dtype == np.float32 else torch.float64
    sch = LS.scheme(W, sname)
    stride = n * n + pad
    G = 4096 + 1                                                              # guard elements on either side (odd: unaligned base too)
    xs = _images(n, nb, dtype, 500)
    fwd = _expected(oracle, xs, sch, L, True)
    for fw, ins in ((1, xs), (0, fwd)):
        exp = _expected(oracle, ins, sch, L, bool(fw))
        for g0 in (4096, G):
            xa = torch.full((2 * g0 + nb * stride,), SENT_G, dtype=td, device=gpu)
            ya = torch.full((2 * g0 + nb * stride,), SENT_G, dtype=td, device=gpu)
            xa[g0:g0 + nb * stride] = SENT_X
            ya[g0:g0 + nb * stride] = SENT_Y
            for i, a in enumerate(ins):
                xa[g0 + i * stride:g0 + i * stride + n * n].copy_(torch.from_numpy(np.ascontiguousarray(a.T).ravel()))
            x_before = xa.clone()
            es = xa.element_size()
            rc = _raw_call(W, gpu, ya.data_ptr() + g0 * es, xa.data_ptr() + g0 * es, n, nb, stride, sch, L, fw, dtype)
            assert rc == 0, (rc, n, pad)
            torch.cuda.synchronize()
            yh = ya.cpu().numpy()
            assert torch.equal(xa, x_before), ("source modified", n, pad, fw)
            assert np.all(yh[:g0] == SENT_G) and np.all(yh[g0 + nb * stride:] == SENT_G), ("guard band written", n, pad, fw, g0, W.last_kernel())
            for i in range(nb):
                got = yh[g0 + i * stride:g0 + i * stride + n * n].reshape(n, n).T
                assert np.array_equal(got, exp[i]), (sname, n, pad, "fw" if fw else "inv", i, g0, W.last_kernel())
                assert np.all(yh[g0 + i * stride + n * n:g0 + (i + 1) * stride] == SENT_Y), ("padding written", n, pad, fw, i, W.last_kernel())


def test_guard_bands_in_place_padded(gpu, W, oracle):
    """the in-place batch (staged through the workspace) with a padded stride: padding and guard bands untouched"""
    import torch
    sch = LS.scheme(W, "cdf97")
    for n, nb, L, pad in ((256, 3, 8, 64), (256, 3, 8, 3), (64, 5, 6, 10)):
        stride, g0 = n * n + pad, 4096
        xs = _images(n, nb, np.float32, 900)
        for fw, ins in ((1, xs), (0, _expected(oracle, xs, sch, L, True))):
            exp = _expected(oracle, ins, sch, L, bool(fw))
            ya = torch.full((2 * g0 + nb * stride,), SENT_G, dtype=torch.float32, device=gpu)
            ya[g0:g0 + nb * stride] = SENT_Y
            for i, a in enumerate(ins):
                ya[g0 + i * stride:g0 + i * stride + n * n].copy_(torch.from_numpy(np.ascontiguousarray(a.T).ravel()))
            p = ya.data_ptr() + g0 * 4
            assert _raw_call(W, gpu, p, p, n, nb, stride, sch, L, fw, np.float32) == 0
            torch.cuda.synchronize()
            yh = ya.cpu().numpy()
            assert np.all(yh[:g0] == SENT_G) and np.all(yh[g0 + nb * stride:] == SENT_G)
            for i in range(nb):
                assert np.array_equal(yh[g0 + i * stride:g0 + i * stride + n * n].reshape(n, n).T, exp[i]), (n, pad, fw, i, W.last_kernel())
                assert np.all(yh[g0 + i * stride + n * n:g0 + (i + 1) * stride] == SENT_Y)


# ---- more than 65535 images ----------------------------------------------------------------------------------------------
def test_more_than_65535_images(gpu, W, oracle):
    import torch
    sch = LS.scheme(W, "cdf97")
    n, L, nb, distinct = 8, 3, 70000, 64
    xs = _images(n, distinct, np.float32, 4000)
    fwd = _expected(oracle, xs, sch, L, True)
    for fw, ins in ((True, xs), (False, fwd)):
        exp = np.stack([np.ascontiguousarray(e.T) for e in _expected(oracle, ins, sch, L, fw)])      # [k][c][r]
        base = torch.from_numpy(np.stack([np.ascontiguousarray(a.T) for a in ins])).to(gpu)
        reps = (nb + distinct - 1) // distinct
        xb = base.repeat(reps, 1, 1)[:nb].contiguous().permute(2, 1, 0)
        assert xb.shape == (n, n, nb) and xb.stride() == (1, n, n * n)
        yb = (W.dwt_batch if fw else W.idwt_batch)(xb, sch, L)
        torch.cuda.synchronize()
        got = yb.permute(2, 1, 0).contiguous()                                                         # [i][c][r]
        want = torch.from_numpy(exp).to(gpu).repeat(reps, 1, 1)[:nb]
        same = (got.view(torch.int32) == want.view(torch.int32)).reshape(nb, -1).all(dim=1)           # every image compared, bit for bit
        assert bool(same.all()), ("images that differ:", torch.nonzero(~same).flatten()[:8].tolist(), int((~same).sum()))


# ---- hipGraph, workspace -------------------------------------------------------------------------------------------------
def test_hipgraph_capture_and_replay_and_workspace(gpu, W, oracle):
    """once wl_workspace_bytes_full(dtype, 1, {nimages * image_stride}, L) is reserved the call allocates nothing (the workspace held
    is unchanged) and can be captured; replays on new data give the bits of a direct call"""
    import torch
    sch = LS.scheme(W, "cdf97")
    s = torch.cuda.Stream()
    for n, nb, L, inplace in ((256, 6, 8, False), (1024, 2, 10, False), (512, 3, 9, True), (200, 3, 3, False)):
        sets = [_images(n, nb, np.float32, 60 + 10 * k) for k in range(3)]
        xb = _to_batch(torch, gpu, sets[0]).clone(memory_format=torch.preserve_format)
        assert xb.stride() == (1, n, n * n)
        yb = xb if inplace else W.similar(xb)
        lib = W._lib.load()
        with torch.cuda.stream(s):
            h, _ = W.transforms._context(gpu)
            nbytes = lib.wl_workspace_bytes_full(0, 1, (C.c_int64 * 3)(nb * n * n, 1, 1), L)
            assert lib.wl_ctx_reserve(h, nbytes) == 0
            held = lib.wl_ctx_workspace_held(h)
            W.dwt_batch(xb, sch, L, y=yb)                    # (first call: code objects loaded)
            torch.cuda.synchronize()
            assert lib.wl_ctx_workspace_held(h) == held, (held, lib.wl_ctx_workspace_held(h))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            W.dwt_batch(xb, sch, L, y=yb)
        for k in (1, 2, 0):
            xb.copy_(_to_batch(torch, gpu, sets[k]))
            if not inplace:
                yb.zero_()
            graph.replay()
            torch.cuda.synchronize()
            got = _from_batch(yb)
            for i in range(nb):
                assert np.array_equal(got[i], oracle.dwt_lifting(sets[k][i], sch, L)), (n, nb, L, inplace, k, i)
        with torch.cuda.stream(s):
            assert lib.wl_ctx_workspace_held(h) == held
        del graph


# ---- argument contract ---------------------------------------------------------------------------------------------------
def test_argument_contract_on_the_device(gpu, W):
    """each status code, in the documented order: an argument set that breaks rule k and every later rule reports rule k"""
    import torch
    sch = LS.scheme(W, "cdf97")
    ST = W._lib.STATUS
    buf = torch.zeros(4 * 16 * 16 + 64, dtype=torch.float32, device=gpu)
    p = buf.data_ptr()

    def call(**kw):
        return ST[_raw_call(W, gpu, kw.pop("y", p), kw.pop("x", p), 16, kw.pop("nb", 2), kw.pop("stride", 256), sch, kw.pop("L", 2), 1,
                            np.float32, **kw)]

    assert call() == "WL_OK"
    bad_all = dict(dtype_code=7, dims=(8, 16), nb=0, L=-1, nsteps=-1)         # breaks every rule after the NULL checks
    assert call(ctx=None, **bad_all) == "WL_EINVAL_ARG"
    assert call(y=None, **bad_all) == "WL_EINVAL_ARG"
    assert call(x=None, **bad_all) == "WL_EINVAL_ARG"
    bad = dict(bad_all); bad["dims"] = "null"
    assert call(**bad) == "WL_EINVAL_ARG"
    assert call(**bad_all) == "WL_EINVAL_DTYPE"
    del bad_all["dtype_code"]
    assert call(**bad_all) == "WL_EINVAL_CUBE"                                 # the square rule before the extents
    bad_all["dims"] = (12, 12)                                                  # 12 has no 2^3 factor (rule 6), ...
    assert call(stride=256, **bad_all) == "WL_EDIMS"                           # nimages = 0
    bad_all["nb"] = 2
    assert call(stride=143, **bad_all) == "WL_EDIMS"                           # image_stride < 12 * 12
    assert call(dims=(0, 0), nb=2, L=-1, nsteps=-1) == "WL_EDIMS"
    assert call(dims=(-4, -4), nb=2, L=-1, nsteps=-1) == "WL_EDIMS"
    assert call(stride=256, **bad_all) == "WL_EINVAL_L"                        # L = -1
    bad_all["L"] = 3
    assert call(stride=256, **bad_all) == "WL_EINVAL_SIZE"
    assert call(dims=(16, 16), nsteps=-1) == "WL_EINVAL_SCHEME"
    assert call(dims=(16, 16), nsteps=17) == "WL_EINVAL_SCHEME"                # more than WL_MAX_STEPS
    assert call(dims=(16, 16), ncoef=[2, 0, 2, 2]) == "WL_EINVAL_SCHEME"
    assert call(dims=(16, 16), ncoef=[2, 4, 2, 2]) == "WL_EINVAL_SCHEME"       # more than WL_MAX_NCOEF
    torch.cuda.synchronize()
    assert call() == "WL_OK"


# ---- fused build ---------------------------------------------------------------------------------------------------------
def test_fused_build(gpu, W, oracle):
    """cdf97 512^2 x 3 Float32 L = 9 on the fused-arithmetic library: within DESIGN.md section 2's bound of the exact build"""
    import torch
    sch = LS.scheme(W, "cdf97")
    n, nb, L = 512, 3, 9
    xs = _images(n, nb, np.float32, 321)
    exact = _from_batch(W.dwt_batch(_to_batch(torch, gpu, xs), sch, L))
    assert all(np.array_equal(e, oracle.dwt_lifting(a, sch, L)) for e, a in zip(exact, xs))
    W.set_arithmetic("fused")
    try:
        assert W.get_arithmetic() == "fused"
        yb = W.dwt_batch(_to_batch(torch, gpu, xs), sch, L)
        fused = _from_batch(yb)
        xr = _from_batch(W.idwt_batch(yb, sch, L))
    finally:
        W.set_arithmetic("exact")
    for i in range(nb):
        e = exact[i].astype(np.float64)
        rel = np.linalg.norm(fused[i].astype(np.float64) - e) / np.linalg.norm(e)
        print("fused batch image %d: relative l2 error %.3e (bound %.3e)" % (i, rel, 1e-6 * math.sqrt(L)))
        assert rel <= 1e-6 * math.sqrt(L), (i, rel)
        rr = np.linalg.norm(xr[i].astype(np.float64) - xs[i]) / np.linalg.norm(xs[i].astype(np.float64))
        assert rr <= 1e-5, (i, rr)                                              # (round trip, tests/test_gpu_fused.py's bound)


# ---- it is a batch -------------------------------------------------------------------------------------------------------
def test_it_is_a_batch(gpu, W):
    """The one timed assertion: cdf9/7, Float32, 256 images of 256^2, L = 8.  Median of 10 batched calls against the median of 10
    rounds of 256 single wl_dwt_lifting_oop calls on the same images (host clock ending in a synchronise, both sides warmed up).
    Required: the batch at least 4x faster (a loop over the images gives 1x by construction; the filter path's measured ratios at the
    neighbouring shapes are 20x and 60x, profiles/r06_batch_of_images.md)."""
    import time
    import torch
    sch = LS.scheme(W, "cdf97")
    n, nb, L = 256, 256, 8
    lib = W._lib.load()
    h, st = W.transforms._context(gpu)
    xb = torch.randn(nb, n, n, dtype=torch.float32, device=gpu).permute(2, 1, 0)
    yb = W.similar(xb)
    W.reserve_workspace(xb, L, full=True)
    iu, nc, sh, cf = sch.flatten()
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    sargs = (len(iu), iu.ctypes.data_as(i32), nc.ctypes.data_as(i32), sh.ctypes.data_as(i32), cf.ctypes.data_as(f64), sch.norm1, sch.norm2, L, 1, st)
    d2, d3 = (C.c_int64 * 2)(n, n), (C.c_int64 * 3)(n, n, 1)
    xp, yp = xb.data_ptr(), yb.data_ptr()

    def batch():
        assert lib.wl_dwt_lifting_batch(h, 0, C.c_void_p(yp), C.c_void_p(xp), d2, nb, n * n, *sargs) == 0

    ptrs = [(C.c_void_p(yp + 4 * i * n * n), C.c_void_p(xp + 4 * i * n * n)) for i in range(nb)]

    def singles():
        for y, x in ptrs:
            rc = lib.wl_dwt_lifting_oop(h, 0, y, x, 2, d3, *sargs)
            assert rc == 0

    def median_ms(f):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    singles()
    torch.cuda.synchronize()
    ref = yb.clone()
    yb.zero_()
    batch()
    torch.cuda.synchronize()
    assert torch.equal(ref, yb)                                                 # the same bits as the 256 single calls
    tb, ts = median_ms(batch), median_ms(singles)
    print("lifting batch of images, cdf9/7 Float32 256 x 256^2 L=8: batch %.3f ms, 256 single calls %.3f ms, ratio %.1fx (kernel %s)"
          % (tb, ts, ts / tb, W.last_kernel()))
    assert ts / tb >= 4.0, (tb, ts, ts / tb)
