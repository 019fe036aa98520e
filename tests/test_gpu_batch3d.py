"""wl_dwt_filter_batch3 (W.dwt_batch / W.idwt_batch on an n0 x n1 x n2 x B tensor): a batch of independent 3-D filter-bank
transforms, every level of the one-launch 3-D tiers one launch over all volumes.

Every comparison is np.array_equal against the CPU oracle, volume by volume: oracle.dwt_filter(x_i, qmf, L, fw); the inverse input
is the oracle's forward output.  Every case asserts the tier it is meant for through W.last_kernel() (first forward level / last
inverse level), then runs again with WL_BATCH3_LOOP = 1 (the single-volume loops, volume after volume): same bits, and the
single-volume kernel names.  The shapes are the smallest that reach each tier.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import onepass3d_cases as CASES_3D
from conftest import rng_array

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
NVOL_MAX = 5

# options under which the small rows of tests/onepass3d_cases.py reach the one-pass kernels (as test_gpu_parity.py sets them)
ONE_PASS_OPTS = {"WL_3D_ONE_MIN": 0, "WL_3D_ONE_WAVES": 0, "WL_I3D_ONE_MIN": 0, "WL_I3D_ONE_MIN_LONG": 0, "WL_I3D_ONE_MIN_ANY": 0,
                 "WL_I3D_ONE_WAVES": 0, "WL_I3D_ONE_F64_FMAX": 8}


# ---- helpers -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _volumes(shape, dtype, nvol):
    """nvol volumes of one shape; the first k of them are the volumes of every smaller batch of that shape"""
    return tuple(rng_array(shape, dtype, 4000 + 17 * i + shape[0] + shape[2]) for i in range(nvol))


_REF = {}


def _reference(oracle, W, shape, dtype, nvol, fname, L):
    """-> (forward outputs, inverse outputs of those) per volume, computed once per (shape, dtype, filter, L) for NVOL_MAX volumes"""
    key = (shape, dtype, fname, L)
    have = _REF.get(key, ([], []))
    q = W.wavelet(getattr(W.WT, fname)).qmf
    xs = _volumes(shape, dtype, NVOL_MAX)
    while len(have[0]) < nvol:
        f = oracle.dwt_filter(xs[len(have[0])], q, L)
        have[0].append(f)
        have[1].append(oracle.dwt_filter(f, q, L, fw=False))
        _REF[key] = have
    return have[0][:nvol], have[1][:nvol]


def _to_batch(W, vols):
    t = W.to_device(np.stack(vols, axis=-1))
    n = vols[0].shape
    assert t.stride() == (1, n[0], n[0] * n[1], n[0] * n[1] * n[2])
    return t


def _run(W, torch, vols, wt, L, fw, opts):
    for k, v in opts.items():
        W.set_option(k, v)
    try:
        yb = (W.dwt_batch if fw else W.idwt_batch)(_to_batch(W, vols), wt, L)
        torch.cuda.synchronize()
        return W.to_host(yb), W.last_kernel()
    finally:
        W.clear_options()


def _check_case(W, oracle, shape, dtype, nvol, fname, L, kfw, kinv, opts=None, directions=(True, False)):
    """forward and inverse of one case: batched against the oracle and the tier asserted; looped against the batched bits"""
    import torch
    opts = dict(opts or {})
    wt = W.wavelet(getattr(W.WT, fname))
    xs = _volumes(shape, dtype, NVOL_MAX)[:nvol]
    fwd, inv = _reference(oracle, W, shape, dtype, nvol, fname, L)
    for fw in directions:
        ins, exp, want = (xs, fwd, kfw) if fw else (fwd, inv, kinv)
        tag = (shape, dtype.__name__, nvol, fname, L, "fw" if fw else "inv")
        got, k = _run(W, torch, ins, wt, L, fw, opts)
        assert k == want, tag + (k,)
        for i in range(nvol):
            assert np.array_equal(got[..., i], exp[i]), tag + ("volume %d" % i, k, int((got[..., i] != exp[i]).sum()))
        lopts = dict(opts)
        lopts["WL_BATCH3_LOOP"] = 1
        got1, k1 = _run(W, torch, ins, wt, L, fw, lopts)
        assert not k1.endswith("_batch"), tag + (k1,)
        if want.endswith("_batch"):
            assert k1 == want[:-len("_batch")], tag + (k1,)
        assert np.array_equal(got, got1), tag + ("batched != looped", k, k1, int((got != got1).sum()))


# ---- the tail tier: one workgroup per volume -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("shape,L", [((16, 16, 16), 4), ((8, 16, 8), 3)])
def test_tail_tier(gpu, W, oracle, shape, L, dtype):
    for nvol in (3, 5):
        for fname in ("haar", "db2", "db4", "sym5"):
            _check_case(W, oracle, shape, dtype, nvol, fname, L, "k_tail3_batch", "k_tail3_batch")


# ---- the LDS-block tier: the volume on blockIdx.y ------------------------------------------------------------------------
# (32,32,32) L = 2: level 2 (16^3) hands over to the tail; (64,32,32) L = 1; (44,28,36) L = 1: half-extents 22 x 14 x 18 are not
# multiples of the block edge P = 4, so the last block of every axis is the moved-back one (48 x 24 x 40 has half-extents that ARE
# multiples of 4 -- the nearest box whose are not, still admitted by level3_lds_ok and with a 16-byte volume size, is this one)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("shape,L,nvol", [((32, 32, 32), 2, 3), ((64, 32, 32), 1, 2), ((44, 28, 36), 1, 3)])
def test_lds_block_tier(gpu, W, oracle, shape, L, nvol, dtype):
    for fname in ("haar", "db2", "db4", "sym5"):
        _check_case(W, oracle, shape, dtype, nvol, fname, L, "k_level3_lds_batch", "k_level3_lds_batch")


# ---- the one-pass tier: the volume is the slowest-varying part of the workgroup index -------------------------------------
ONE_PASS_ROWS = [((256, 16, 16), 1), ((128, 32, 16), 1), ((72, 16, 16), 1), ((200, 24, 20), 1), ((128, 64, 64), 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("shape,L", ONE_PASS_ROWS)
def test_one_pass_tier(gpu, W, oracle, shape, L, dtype):
    assert (shape, L) in CASES_3D.FWD_CASES and (shape, L) in CASES_3D.INV_CASES
    tname = "float" if dtype == np.float32 else "double"
    for fname in ("db2", "db4"):
        assert CASES_3D.fwd_instance(tname, CASES_3D.TAPS[fname], shape[0]) and CASES_3D.inv_instance(tname, CASES_3D.TAPS[fname], shape[0])
        _check_case(W, oracle, shape, dtype, 3, fname, L, "k_fwd3d_one_batch", "k_inv3d_one_batch", ONE_PASS_OPTS)
    if dtype == np.float32:                                      # 10 taps: the forward kernel only, Float32 on 8-byte lanes
        assert CASES_3D.fwd_instance(tname, 10, shape[0])
        _check_case(W, oracle, shape, dtype, 3, "db5", L, "k_fwd3d_one_batch", None, ONE_PASS_OPTS, directions=(True,))


def test_one_pass_default_gate(gpu, W, oracle):
    """without options: 2 volumes of 128^3, db2 -- level 1 of both directions is the one-pass kernel, level 2 the LDS blocks,
    level 3 .. the tail: every level of the call one launch"""
    _check_case(W, oracle, (128, 128, 128), np.float32, 2, "db2", 4, "k_fwd3d_one_batch", "k_inv3d_one_batch")


# ---- levels no batched tier takes: volume after volume, inside a batch ------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_fallback_shapes_in_a_batch(gpu, W, oracle, dtype):
    import torch
    for shape, L, fname, nvol in (((20, 12, 28), 2, "db2", 2), ((32, 32, 32), 2, "db6", 2)):
        wt = W.wavelet(getattr(W.WT, fname))
        xs = _volumes(shape, dtype, NVOL_MAX)[:nvol]
        fwd, inv = _reference(oracle, W, shape, dtype, nvol, fname, L)
        for fw, ins, exp in ((True, xs, fwd), (False, fwd, inv)):
            got, k = _run(W, torch, ins, wt, L, fw, {})
            assert not k.endswith("_batch"), (shape, fname, k)
            # the kernel of the single-volume call of the same shape
            (W.dwt if fw else W.idwt)(W.to_device(ins[0]), wt, L)
            torch.cuda.synchronize()
            assert k == W.last_kernel(), (shape, fname, k, W.last_kernel())
            for i in range(nvol):
                assert np.array_equal(got[..., i], exp[i]), (shape, dtype.__name__, fname, fw, i, k)


# ---- padding, alignment, L = 0 (the C ABI: the Python wrapper only makes dense batches) ----------------------------------------
def _raw(W, gpu, yp, xp, dims, nvol, stride, q, L, fw, code=0, ctx="ctx", flen=None):
    lib = W._lib.load()
    h, st = W.transforms._context(gpu)
    d = None if dims is None else (C.c_int64 * 3)(*dims)
    qq = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
    return lib.wl_dwt_filter_batch3(h if ctx == "ctx" else ctx, code, None if yp is None else C.c_void_p(yp), None if xp is None else C.c_void_p(xp),
                                    d, nvol, stride, None if qq is None else qq.ctypes.data_as(C.POINTER(C.c_double)),
                                    (len(qq) if qq is not None else 0) if flen is None else flen, L, fw, st)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_padded_and_misaligned_strides(gpu, W, oracle, dtype):
    import torch
    SENT = -12345.0
    shape, nvol, fname = (32, 32, 32), 3, "db4"
    N = shape[0] * shape[1] * shape[2]
    q = W.wavelet(getattr(W.WT, fname)).qmf
    xs = _volumes(shape, dtype, NVOL_MAX)[:nvol]
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    code = 0 if dtype == np.float32 else 1
    for pad, L, fw, want in ((16, 2, 1, "k_level3_lds_batch"), (16, 2, 0, "k_level3_lds_batch"), (1, 2, 1, "k_level3_lds"), (1, 2, 0, "k_level3_lds"),
                             (16, 0, 1, "copy"), (1, 0, 0, "copy")):
        stride = N + pad
        fwd, inv = _reference(oracle, W, shape, dtype, nvol, fname, L) if L else (xs, xs)
        ins, exp = (xs, fwd) if fw else (fwd, inv)
        hx = np.full(nvol * stride, 7.0, dtype=dtype)
        for i in range(nvol):
            hx[i * stride:i * stride + N] = ins[i].ravel(order="F")
        xb = torch.from_numpy(hx).to(gpu)
        yb = torch.full((nvol * stride,), SENT, dtype=tdt, device=gpu)
        rc = _raw(W, gpu, yb.data_ptr(), xb.data_ptr(), shape, nvol, stride, q, L, fw, code)
        torch.cuda.synchronize()
        assert W._lib.STATUS[rc] == "WL_OK", rc
        assert W.last_kernel() == want, (pad, L, fw, W.last_kernel())
        hy = yb.cpu().numpy()
        for i in range(nvol):
            got = hy[i * stride:i * stride + N].reshape(shape, order="F")
            assert np.array_equal(got, exp[i]), (pad, L, fw, i)
            assert np.all(hy[i * stride + N:(i + 1) * stride] == dtype(SENT)), ("padding written", pad, L, fw, i)
        assert np.array_equal(xb.cpu().numpy(), hx), "source modified"


# ---- round trip, hipGraph ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_round_trip(gpu, W, dtype):
    """idwt_batch(dwt_batch(x)) == x to the project's round-trip bound (relative l2: Float32 1e-5, as smoke() and
    tests/test_gpu_fused.py; Float64 1e-13 sqrt(L)).  An orthogonal transform of L levels, three passes
    each, every output a sum of F <= 8 rounded products: about sqrt(6 L) F eps = 2e-6 (Float32) / 4e-15 (Float64) in l2."""
    import torch
    shape, nvol, L = (32, 32, 32), 4, 5
    wt = W.wavelet(W.WT.db4)
    xs = _volumes(shape, dtype, NVOL_MAX)[:nvol]
    xb = _to_batch(W, xs)
    yb = W.dwt_batch(xb, wt)                                     # default L: min over the extents of maxtransformlevels = 5
    assert W.last_kernel() == "k_level3_lds_batch"
    xr = W.to_host(W.idwt_batch(yb, wt))
    torch.cuda.synchronize()
    bound = 1e-5 if dtype == np.float32 else 1e-13 * math.sqrt(L)
    for i in range(nvol):
        rel = np.linalg.norm(xr[..., i].astype(np.float64) - xs[i]) / np.linalg.norm(xs[i].astype(np.float64))
        assert rel <= bound, (i, rel)
    assert np.array_equal(W.to_host(yb), W.to_host(W.dwt_batch(xb, wt, L)))


def test_hipgraph_capture_and_workspace(gpu, W, oracle):
    """once wl_workspace_bytes_full(dtype, 1, {nvolumes * volume_stride}, L) is reserved a batched call allocates nothing and can
    be captured; replays on new data give the bits of the eager call"""
    import torch
    s = torch.cuda.Stream()
    wt = W.wavelet(W.WT.db4)
    lib = W._lib.load()
    for shape, nvol, L, want in (((32, 32, 32), 4, 2, "k_level3_lds_batch"), ((16, 16, 16), 5, 4, "k_tail3_batch"), ((20, 12, 28), 2, 2, None)):
        N = shape[0] * shape[1] * shape[2]
        sets = [[rng_array(shape, np.float32, 900 + 10 * k + i) for i in range(nvol)] for k in range(3)]
        xb = _to_batch(W, sets[0])
        yb = W.similar(xb)
        with torch.cuda.stream(s):
            h, _ = W.transforms._context(gpu)
            nbytes = lib.wl_workspace_bytes_full(0, 1, (C.c_int64 * 3)(nvol * N, 1, 1), L)
            assert lib.wl_ctx_reserve(h, nbytes) == 0
            held = lib.wl_ctx_workspace_held(h)
            W.dwt_batch(xb, wt, L, y=yb)                        # (first call: code objects loaded)
            torch.cuda.synchronize()
            assert lib.wl_ctx_workspace_held(h) == held, (held, lib.wl_ctx_workspace_held(h))
            if want:
                assert W.last_kernel() == want
            eager = [W.to_host(W.dwt_batch(_to_batch(W, sets[k]), wt, L)) for k in range(3)]
            torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            W.dwt_batch(xb, wt, L, y=yb)
        for k in (1, 2, 0):
            xb.copy_(_to_batch(W, sets[k]))
            yb.zero_()
            graph.replay()
            torch.cuda.synchronize()
            got = W.to_host(yb)
            assert np.array_equal(got, eager[k]), (shape, k)
            for i in range(nvol):
                assert np.array_equal(got[..., i], oracle.dwt_filter(sets[k][i], wt.qmf, L)), (shape, k, i)
        with torch.cuda.stream(s):
            assert lib.wl_ctx_workspace_held(h) == held
        del graph


# ---- argument contract -----------------------------------------------------------------------------------------------------
def test_status_codes_in_order(gpu, W):
    """each status code, in the documented order: an argument set that breaks rule k and every later rule reports rule k"""
    import torch
    ST = W._lib.STATUS
    q = W.wavelet(W.WT.db2).qmf
    bx = torch.zeros(2 * 4096 + 64, dtype=torch.float32, device=gpu)
    by = torch.zeros(2 * 4096 + 64, dtype=torch.float32, device=gpu)
    px, py = bx.data_ptr(), by.data_ptr()

    def call(**kw):
        a = dict(y=py, x=px, dims=(16, 16, 16), nvol=2, stride=4096, q=q, L=2, fw=1, code=0, ctx="ctx", flen=None)
        a.update(kw)
        return ST[_raw(W, gpu, a["y"], a["x"], a["dims"], a["nvol"], a["stride"], a["q"], a["L"], a["fw"], a["code"], a["ctx"], a["flen"])]

    assert call() == "WL_OK"
    # breaks every rule after the NULL checks: dtype, filter length, extents, L, size, alias
    bad = dict(code=7, flen=1, dims=(12, 12, 0), L=-1, y=px)
    for null in (dict(ctx=None), dict(y=None), dict(x=None), dict(dims=None), dict(q=None)):
        assert call(**dict(bad, **null)) == "WL_EINVAL_ARG", null
    assert call(**bad) == "WL_EINVAL_DTYPE"
    del bad["code"]
    assert call(**bad) == "WL_EINVAL_FILTER"
    assert call(**dict(bad, flen=10 ** 6)) == "WL_EINVAL_FILTER"
    del bad["flen"]
    assert call(**bad) == "WL_EDIMS"                                          # an extent of 0
    bad["dims"] = (12, 12, 12)                                                # 12 has no 2^3 factor
    assert call(nvol=0, **bad) == "WL_EDIMS"
    assert call(stride=12 ** 3 - 1, **bad) == "WL_EDIMS"                      # volume_stride < the volume
    assert call(**bad) == "WL_EINVAL_L"
    bad["L"] = 3
    assert call(**bad) == "WL_EINVAL_SIZE"
    assert call(dims=(16, 16, 12), L=3, y=px) == "WL_EINVAL_SIZE"
    assert call(y=px) == "WL_EALIAS"
    torch.cuda.synchronize()
    assert call() == "WL_OK"


# ---- translation-invariant (and plain) denoise of a cube: the spins as a batch of volumes ------------------------------------
def _noisy_cube(n, dtype, seed):
    t = np.linspace(0.0, 1.0, n)
    s = np.sin(2 * np.pi * (1.5 * t + 0.2)) * (1.0 - t)
    clean = s[:, None, None] * s[None, :, None] * np.cos(3.0 * t)[None, None, :]
    return (clean + 0.05 * np.random.default_rng(seed).standard_normal((n, n, n))).astype(dtype)


def _oracle_denoise(oracle, x, wt, L, dnt, TI, nspin, sigma=None):
    kind = type(dnt.th).__name__[:-2].lower()
    fwd = lambda a, l: oracle.dwt_filter(a, wt.qmf, l)
    inv = lambda a, l: oracle.dwt_filter(a, wt.qmf, l, fw=False)
    return oracle.denoise(x, fwd, inv, L, kind, dnt.t, TI=TI, nspin=nspin, sigma=sigma)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_ti_denoise_of_cubes(gpu, W, oracle, dtype):
    """W.denoise(cube, TI=True, nspin=(a, b, c)) as one device-resident call (wl_denoise_ti_filter with ndims = 3): bit for bit the
    reference's per-spin sequence (denoising.jl:51-66) as restated by oracle.denoise"""
    cases = [
        # n, nspin, wavelet (None: the default, sym5), L, dnt (None: VisuShrink(n))
        (16, (2, 3, 2), None, 3, None),
        (32, (3, 2, 2), "db4", 2, W.VisuShrink(W.SoftTH(), 2.0)),
        (64, (2, 2, 2), "db2", 3, W.VisuShrink(W.HardTH(), 2.5)),
    ]
    for n, nspin, wname, L, dnt in cases:
        x = _noisy_cube(n, dtype, n)
        wt = W.DEFAULT_WAVELET if wname is None else W.wavelet(getattr(W.WT, wname))
        d = W.VisuShrink(n) if dnt is None else dnt
        kw = dict(L=L, TI=True, nspin=nspin)
        if dnt is not None:
            kw["dnt"] = dnt
        y = W.to_host(W.denoise(W.to_device(x), **kw) if wname is None else W.denoise(W.to_device(x), wt, **kw))
        assert W.last_kernel() == "denoise_ti_batch", (n, W.last_kernel())
        e = _oracle_denoise(oracle, x, wt, L, d, True, nspin)
        assert y.dtype == dtype and np.array_equal(y, e), (n, nspin, wname, L, int((y != e).sum()))
        assert not np.array_equal(y, x)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_ti_denoise_of_cubes_in_groups_and_edge_cases(gpu, W, oracle, dtype):
    x = _noisy_cube(32, dtype, 5)
    xd = W.to_device(x)
    wt = W.wavelet(W.WT.db4)
    # a 1 MiB cap: a spin of 32^3 holds about 74 k elements of workspace beside the 98 k fixed ones, so the 12 spins run in
    # groups of at most 2 (Float32: 6 groups; Float64: 12) -- the accumulation order across groups is the spin order
    e = _oracle_denoise(oracle, x, wt, 2, W.VisuShrink(32), True, (3, 2, 2))
    W.set_option("WL_TI_WS_CAP_MB", 1)
    y = W.to_host(W.denoise(xd, wt, L=2, TI=True, nspin=(3, 2, 2)))
    assert W.last_kernel() == "denoise_ti_batch"
    W.clear_options()
    assert np.array_equal(y, e), int((y != e).sum())
    assert np.array_equal(W.to_host(W.denoise(xd, wt, L=2, TI=True, nspin=(3, 2, 2))), e)
    # L = 0 (dwt / idwt are copies: every spin thresholds the shifted cube itself) with a custom estimate
    dnt = W.VisuShrink(W.HardTH(), 0.7)
    e0 = _oracle_denoise(oracle, x, wt, 0, dnt, True, (2, 2, 3), sigma=0.1)
    y0 = W.to_host(W.denoise(xd, wt, L=0, dnt=dnt, TI=True, nspin=(2, 2, 3), estnoise=lambda a, w: 0.1))
    assert W.last_kernel() == "denoise_ti_batch" and np.array_equal(y0, e0) and not np.array_equal(y0, x)
    # one spin of shift zero and the plain denoise: the reference's plain sequence, sigma kept on the device
    ep = _oracle_denoise(oracle, x, W.DEFAULT_WAVELET, 5, W.VisuShrink(32), False, None)
    y1 = W.to_host(W.denoise(xd, TI=True, nspin=(1, 1, 1)))
    assert W.last_kernel() == "denoise_one_spin", W.last_kernel()
    assert np.array_equal(y1, ep)
    y2 = W.to_host(W.denoise(xd))
    assert W.last_kernel() == "denoise_one_spin", W.last_kernel()
    assert np.array_equal(y2, ep)
    assert np.array_equal(W.to_host(xd), x)                      # denoise never modifies its input
    # a box that is not a cube: the reference's ArgumentError (denoising.jl:29)
    with pytest.raises(W.ArgumentError, match="square/cube"):
        W.denoise(W.to_device(rng_array((32, 32, 16), dtype, 1)), TI=True, nspin=(2, 2, 2))
