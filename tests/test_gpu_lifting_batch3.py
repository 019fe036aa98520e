"""wl_dwt_lifting_batch3 (W.dwt_batch / W.idwt_batch of an n x n x n x B tensor with a GLS) and the lifting TI denoise of cubes:
a batch of cubes through the 3-D lifting level loop, every launch of the single cube one launch over all volumes.

Every value comparison is np.array_equal against the CPU oracle, volume by volume: oracle.dwt_lifting(x_i, scheme, L, fw); the
inverse input is the oracle's forward output.  Schemes come from tests/lifting_schemes.py.  The shapes are the smallest that reach
each tier: k_tail_lift3d up to 32^3 (Float32) / 16^3 (Float64), the axis and short-line launches above that (and below with
WL_LIFT_TAIL3D = 0), the fused plane kernel from 128^3.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import lifting_schemes as LS
from conftest import rng_array

pytestmark = pytest.mark.gpu

BATCH = "k_lift_axis_stream+k_lift_short_lines_batch"
SINGLE = "k_lift_axis_stream+k_lift_short_lines"
NVOL_MAX = 5
SENT_X, SENT_Y, SENT_G = 7.0, -3.0, 123456.0


# ---- helpers -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _volumes(n, dtype):
    return tuple(rng_array((n, n, n), dtype, 7000 + 13 * i + n) for i in range(NVOL_MAX))


_REF = {}


def _reference(oracle, W, n, dtype, nvol, sname, L):
    """-> (forward outputs, inverse outputs of those) per volume; computed once per (n, dtype, scheme, L) and never modified"""
    key = (n, dtype, sname, L)
    have = _REF.setdefault(key, ([], []))
    sch = LS.scheme(W, sname)
    xs = _volumes(n, dtype)
    while len(have[0]) < nvol:
        f = oracle.dwt_lifting(xs[len(have[0])], sch, L)
        have[0].append(f)
        have[1].append(oracle.dwt_lifting(f, sch, L, fw=False))
    return have[0][:nvol], have[1][:nvol]


def _to_batch(W, vols):
    t = W.to_device(np.stack(vols, axis=-1))
    n = vols[0].shape[0]
    assert t.stride() == (1, n, n * n, n * n * n)
    return t


def _run(W, torch, vols, sch, L, fw, opts, inplace=False):
    for k, v in opts.items():
        W.set_option(k, v)
    try:
        xb = _to_batch(W, vols)
        f = W.dwt_batch if fw else W.idwt_batch
        yb = f(xb, sch, L, y=xb) if inplace else f(xb, sch, L)
        torch.cuda.synchronize()
        k = W.last_kernel()
        if inplace:
            assert yb.data_ptr() == xb.data_ptr()
        else:
            assert np.array_equal(W.to_host(xb), np.stack(vols, axis=-1)), "source modified"
        return W.to_host(yb), k
    finally:
        W.clear_options()


def _single_kernel(W, torch, n, L, sname, dtype, fw, opts=None):
    """W.last_kernel() after the single-cube call of the same size, depth, scheme and direction"""
    for k, v in (opts or {}).items():
        W.set_option(k, v)
    try:
        (W.dwt if fw else W.idwt)(W.to_device(_volumes(n, dtype)[0]), LS.scheme(W, sname), L)
        torch.cuda.synchronize()
        return W.last_kernel()
    finally:
        W.clear_options()


def _check_case(W, oracle, n, dtype, nvol, sname, L, want=BATCH, opts=None, directions=(True, False), inplace=(False,), loop=True):
    """forward and inverse of one case against the oracle, the kernel name asserted; then the volume-after-volume loop: same bits and
    the single-cube name"""
    import torch
    opts = dict(opts or {})
    sch = LS.scheme(W, sname)
    xs = _volumes(n, dtype)[:nvol]
    fwd, inv = _reference(oracle, W, n, dtype, nvol, sname, L)
    for fw in directions:
        ins, exp = (xs, fwd) if fw else (fwd, inv)
        for ip in inplace:
            tag = (n, dtype.__name__, nvol, sname, L, "fw" if fw else "inv", "in place" if ip else "out of place", sorted(opts.items()))
            got, k = _run(W, torch, ins, sch, L, fw, opts, ip)
            assert k == want, tag + (k,)
            for i in range(nvol):
                assert np.array_equal(got[..., i], exp[i]), tag + ("volume %d" % i, k, int((got[..., i] != exp[i]).sum()))
        if loop:
            lopts = dict(opts)
            lopts["WL_LIFT_BATCH3_LOOP"] = 1
            got1, k1 = _run(W, torch, ins, sch, L, fw, lopts)
            assert k1 == _single_kernel(W, torch, n, L, sname, dtype, fw, opts) and not k1.endswith("_batch"), tag + (k1,)
            if want == BATCH:
                assert k1 == SINGLE, tag + (k1,)
            assert np.array_equal(got, got1), tag + ("batched != looped", int((got != got1).sum()))


# ---- the tail tier: one workgroup per volume -----------------------------------------------------------------------------
@pytest.mark.parametrize("sname", ["cdf97", "db2", "haar", "twin_cdf97", "twin_db2", "twin_haar"])
@pytest.mark.parametrize("n,dtype", [(8, np.float32), (16, np.float32), (32, np.float32), (8, np.float64), (16, np.float64)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_tail_tier(gpu, W, oracle, n, dtype, sname):
    for L in (1, W.maxtransformlevels(n)):
        for nvol in (3, 5):
            _check_case(W, oracle, n, dtype, nvol, sname, L, inplace=(False, True))


# ---- the axis and short-line launches ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sname", ["cdf97", "twin_db2", "haar"])
@pytest.mark.parametrize("n,dtype,L,opts", [(64, np.float32, 2, {}), (32, np.float64, 2, {}), (8, np.float32, 3, {"WL_LIFT_TAIL3D": 0}),
                                            (16, np.float32, 4, {"WL_LIFT_TAIL3D": 0}), (16, np.float64, 4, {"WL_LIFT_TAIL3D": 0})],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_axis_and_short_line_tier(gpu, W, oracle, n, dtype, L, opts, sname):
    """64^3 / 32^3 (Float64): level 1 through the axis and short-line launches, level 2 in the tail (forward: the tail reads the
    approximation buffer of its volume; inverse: it writes the ping-pong slot of its volume).  With WL_LIFT_TAIL3D = 0 every level
    goes through those launches, down to side 2: the corner routing of every level is exercised from the second volume on."""
    _check_case(W, oracle, n, dtype, 3, sname, L, opts=opts)


def test_axis_tier_in_place(gpu, W, oracle):
    _check_case(W, oracle, 64, np.float32, 3, "cdf97", 2, inplace=(True,), loop=False)
    _check_case(W, oracle, 16, np.float32, 3, "db2", 4, opts={"WL_LIFT_TAIL3D": 0}, inplace=(True,), loop=False)


# ---- the fused plane kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "WL_NO_LIFT2D_FUSED"])
@pytest.mark.parametrize("sname,dtype,L", [("cdf97", np.float32, 1), ("cdf97", np.float32, 2), ("db2", np.float32, 2), ("cdf97", np.float64, 1)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_fused_plane_kernel(gpu, W, oracle, sname, dtype, L, fused):
    """128^3, 2 volumes: plane pass + k_lift2d_fwd / k_lift2d_inv over 256 planes (L = 2: the second level takes the approximation
    of its volume from / to the dense buffer); again through the row and short-line launches"""
    _check_case(W, oracle, 128, dtype, 2, sname, L, opts={} if fused else {"WL_NO_LIFT2D_FUSED": 1}, loop=fused)


def test_fused_plane_kernel_grid_split(gpu, W, oracle):
    """gridDim.y of k_lift2d_fwd / k_lift2d_inv holds 65535 planes; 520 volumes of 128^3 would be needed to pass it, so the split is
    exercised with the limit lowered (context option WL_LIFT2D_GRID_Y, read by the same code that splits at 65535): 3 volumes of
    128^3 = 384 planes with a limit of 300 go out as launches of 2 + 1 volumes, with a limit of 128 as three launches.  The split of
    the axis kernel (32768 planes) is covered by test_more_planes_than_a_grid_holds at its real size."""
    for gy in (300, 128):
        _check_case(W, oracle, 128, np.float32, 3, "cdf97", 2, opts={"WL_LIFT2D_GRID_Y": gy}, loop=False)


# ---- group and grid splits -----------------------------------------------------------------------------------------------
def _tiled_case(W, oracle, torch, gpu, nb, opts):
    """nb volumes of 8^3 Float32 cycling through 5 distinct cubes: the expectation is 5 oracle calls, tiled; compared on the device"""
    n, L, dtype = 8, 3, np.float32
    sch = LS.scheme(W, "cdf97")
    xs = _volumes(n, dtype)
    fwd, inv = _reference(oracle, W, n, dtype, NVOL_MAX, "cdf97", L)
    reps = (nb + NVOL_MAX - 1) // NVOL_MAX

    def dev(vols):                                                            # [i][k][j][r] on the device
        base = torch.from_numpy(np.stack([np.ascontiguousarray(v.transpose(2, 1, 0)) for v in vols])).to(gpu)
        return base.repeat(reps, 1, 1, 1)[:nb].contiguous()

    for k, v in opts.items():
        W.set_option(k, v)
    try:
        for fw, ins, exp in ((True, xs, fwd), (False, fwd, inv)):
            xb = dev(ins).permute(3, 2, 1, 0)
            assert xb.shape == (n, n, n, nb) and xb.stride() == (1, n, n * n, n * n * n)
            yb = (W.dwt_batch if fw else W.idwt_batch)(xb, sch, L)
            torch.cuda.synchronize()
            assert W.last_kernel() == BATCH
            got = yb.permute(3, 2, 1, 0).contiguous()
            same = (got.view(torch.int32) == dev(exp).view(torch.int32)).reshape(nb, -1).all(dim=1)
            assert bool(same.all()), ("fw" if fw else "inv", "volumes that differ:", torch.nonzero(~same).flatten()[:8].tolist(), int((~same).sum()))
    finally:
        W.clear_options()


def test_more_than_65535_volumes(gpu, W, oracle):
    """65540 volumes on the tail tier: a group of 65535 and one of 5"""
    import torch
    _tiled_case(W, oracle, torch, gpu, 65540, {})


def test_more_planes_than_a_grid_holds(gpu, W, oracle):
    """8200 volumes of 8^3 without the tail: 65600 planes in the row pass (k_lift_axis_stream splits blockIdx.y at 32768)"""
    import torch
    _tiled_case(W, oracle, torch, gpu, 8200, {"WL_LIFT_TAIL3D": 0})


# ---- what runs volume after volume inside a batch ------------------------------------------------------------------------
@pytest.mark.parametrize("sname,n,L", [("nc3", 16, 4), ("shift5", 16, 4), ("zero_steps", 16, 4), ("cdf97", 24, 3), ("cdf97", 4, 2)])
def test_fallbacks_inside_a_batch(gpu, W, oracle, sname, n, L):
    """unknown scheme shapes, a side that is no power of two and a side below 8: the bits of the oracle and the kernel of the
    single-cube call, no "_batch" """
    import torch
    for fw in (True, False):
        want = _single_kernel(W, torch, n, L, sname, np.float32, fw)
        assert not want.endswith("_batch")
        _check_case(W, oracle, n, np.float32, 3, sname, L, want=want, directions=(fw,), loop=False)


def test_forward_scheme_with_an_inverse_shape(gpu, W, oracle):
    """a user scheme whose forward step sequence is haar's inverse one (Update, Predict): match_shape knows it, k_tail_lift3d has no
    instance of that shape for that direction, so even an 8^3 batch goes through the axis and short-line launches and needs their
    workspace"""
    import torch
    WT = W.WT
    sch = W.GLS(([WT.make_lsstep(WT.Update, [0.55], 0), WT.make_lsstep(WT.Predict, [-0.9], 0)], 0.75, 1.35, "update_first"))
    assert LS.shape_id(sch, True) == 5 and LS.shape_id(sch, False) == 4
    xs = [rng_array((8, 8, 8), np.float32, 300 + i) for i in range(3)]
    fwd = [oracle.dwt_lifting(a, sch, 3) for a in xs]
    yb = W.dwt_batch(_to_batch(W, xs), sch, 3)
    torch.cuda.synchronize()
    assert W.last_kernel() == BATCH
    got = W.to_host(yb)
    assert all(np.array_equal(got[..., i], fwd[i]) for i in range(3))
    xr = W.to_host(W.idwt_batch(yb, sch, 3))
    assert W.last_kernel() == BATCH
    assert all(np.array_equal(xr[..., i], oracle.dwt_lifting(fwd[i], sch, 3, fw=False)) for i in range(3))


def test_path_1_runs_volume_after_volume(gpu, W, oracle):
    import torch
    sch = LS.scheme(W, "cdf97")
    xs = _volumes(16, np.float32)[:3]
    fwd, _ = _reference(oracle, W, 16, np.float32, 3, "cdf97", 4)
    W.set_kernel_path(1)
    try:
        yb = W.dwt_batch(_to_batch(W, xs), sch, 4)
        torch.cuda.synchronize()
        k = W.last_kernel()
        W.dwt(W.to_device(xs[0]), sch, 4)
        assert k == W.last_kernel() and not k.endswith("_batch"), k
    finally:
        W.set_kernel_path(0)
    got = W.to_host(yb)
    assert all(np.array_equal(got[..., i], fwd[i]) for i in range(3))


# ---- padded / misaligned volume stride, guard bands ----------------------------------------------------------------------
def _raw_call(W, gpu, yb, xb, n, nb, stride, sch, L, fw, dtype, dims=None, nsteps=None, dtype_code=None, ctx="ctx", ncoef=None):
    lib = W._lib.load()
    h, st = W.transforms._context(gpu)
    iu, nc, sh, cf = sch.flatten()
    if ncoef is not None:
        nc = np.asarray(ncoef, dtype=np.int32)
    d = None if dims == "null" else (C.c_int64 * 3)(*(dims if dims is not None else (n, n, n)))
    code = (0 if dtype == np.float32 else 1) if dtype_code is None else dtype_code
    i32 = C.POINTER(C.c_int32)
    return lib.wl_dwt_lifting_batch3(h if ctx == "ctx" else ctx, code, C.c_void_p(yb) if yb is not None else None,
                                     C.c_void_p(xb) if xb is not None else None, d, nb, stride,
                                     len(iu) if nsteps is None else nsteps, iu.ctypes.data_as(i32), nc.ctypes.data_as(i32),
                                     sh.ctypes.data_as(i32), cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1, sch.norm2, L, fw, st)


@pytest.mark.parametrize("inplace", [False, True], ids=["oop", "inplace"])
@pytest.mark.parametrize("n,L,pad,dtype,opts,want", [
    (8, 3, 16, np.float32, {}, BATCH),                                 # the tail tier with a padded stride
    (16, 4, 16, np.float32, {"WL_LIFT_TAIL3D": 0}, BATCH),             # the axis / short-line launches with a padded stride
    (64, 2, 16, np.float32, {}, BATCH),
    (16, 2, 16, np.float64, {}, BATCH),
    (8, 0, 16, np.float32, {}, "copy"),                                # L = 0 copies the volumes
    (8, 3, 1, np.float32, {}, None),                                   # stride N + 1: bases off 16 bytes, volume after volume
    (16, 4, 1, np.float64, {"WL_LIFT_TAIL3D": 0}, None),
], ids=lambda v: getattr(v, "__name__", str(v)))
def test_padded_volume_stride_and_guard_bands(gpu, W, oracle, n, L, pad, dtype, opts, want, inplace):
    """volume_stride = n^3 + pad through ctypes; x and y sit inside larger allocations filled with a sentinel: results exact, the
    padding between the volumes and the guard bands untouched, the source of an out-of-place call untouched altogether.  want = None:
    the kernel name of the single-cube call on the last volume's own (possibly misaligned) pointers, which never ends in "_batch"."""
    import torch
    td = torch.float32 if dtype == np.float32 else torch.float64
    sch = LS.scheme(W, "cdf97")
    N, nb, g0 = n * n * n, 3, 4096
    stride = N + pad
    xs = _volumes(n, dtype)[:nb]
    fwd, inv = (xs, xs) if L == 0 else _reference(oracle, W, n, dtype, nb, "cdf97", L)
    for k, v in opts.items():
        W.set_option(k, v)
    try:
        for fw, ins, exp in ((1, xs, fwd), (0, fwd, inv)):
            xa = torch.full((2 * g0 + nb * stride,), SENT_G, dtype=td, device=gpu)
            xa[g0:g0 + nb * stride] = SENT_Y if inplace else SENT_X
            for i, a in enumerate(ins):
                xa[g0 + i * stride:g0 + i * stride + N].copy_(torch.from_numpy(np.ascontiguousarray(a.transpose(2, 1, 0)).ravel()))
            if inplace:
                ya = xa
            else:
                ya = torch.full((2 * g0 + nb * stride,), SENT_G, dtype=td, device=gpu)
                ya[g0:g0 + nb * stride] = SENT_Y
            x_before = xa.clone()
            es = xa.element_size()
            rc = _raw_call(W, gpu, ya.data_ptr() + g0 * es, xa.data_ptr() + g0 * es, n, nb, stride, sch, L, fw, dtype)
            assert rc == 0, (rc, n, pad)
            torch.cuda.synchronize()
            kb = W.last_kernel()
            if want is None:
                iu, nc, sh, cf = sch.flatten()
                i32 = C.POINTER(C.c_int32)
                h, st = W.transforms._context(gpu)
                scratch = torch.zeros(N + 8, dtype=td, device=gpu)
                off = (g0 + (nb - 1) * stride) * es                             # the last volume: same base alignment for the scratch output
                rc1 = W._lib.load().wl_dwt_lifting_oop(h, 0 if dtype == np.float32 else 1, C.c_void_p(scratch.data_ptr() + off % 16),
                                                       C.c_void_p(xa.data_ptr() + off), 3, (C.c_int64 * 3)(n, n, n), len(iu),
                                                       iu.ctypes.data_as(i32), nc.ctypes.data_as(i32), sh.ctypes.data_as(i32),
                                                       cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1, sch.norm2, L, fw, st)
                assert rc1 == 0, rc1
                torch.cuda.synchronize()
                assert kb == W.last_kernel() and not kb.endswith("_batch"), (kb, W.last_kernel(), n, pad, fw)
            else:
                assert kb == want, (kb, n, pad, fw)
            yh = ya.cpu().numpy()
            if not inplace:
                assert torch.equal(xa, x_before), ("source modified", n, pad, fw)
            assert np.all(yh[:g0] == SENT_G) and np.all(yh[g0 + nb * stride:] == SENT_G), ("guard band written", n, pad, fw)
            for i in range(nb):
                got = yh[g0 + i * stride:g0 + i * stride + N].reshape(n, n, n).transpose(2, 1, 0)
                assert np.array_equal(got, exp[i]), (n, pad, "fw" if fw else "inv", i, W.last_kernel())
                assert np.all(yh[g0 + i * stride + N:g0 + (i + 1) * stride] == SENT_Y), ("padding written", n, pad, fw, i)
    finally:
        W.clear_options()


# ---- round trip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: d.__name__)
@pytest.mark.parametrize("sname,n,L", [("cdf97", 32, 5), ("cdf97", 64, 3), ("nc3", 16, 4)])
def test_round_trip(gpu, W, sname, n, L, dtype):
    """idwt_batch(dwt_batch(x)) against x, the project's bounds (tests/test_gpu_batch3d.py::test_round_trip): relative l2 <= 1e-5 for
    Float32, <= 1e-13 sqrt(L) for Float64 (the oracle alone stays at <= 9e-7 and <= 1.3e-15 for these schemes at 8^3 .. 128^3)"""
    sch = LS.scheme(W, sname)
    xs = _volumes(n, dtype)[:3]
    xr = W.to_host(W.idwt_batch(W.dwt_batch(_to_batch(W, xs), sch, L), sch, L))
    for i in range(3):
        rel = np.linalg.norm(xr[..., i].astype(np.float64) - xs[i]) / np.linalg.norm(xs[i].astype(np.float64))
        print("round trip %s %d^3 L=%d %s volume %d: relative l2 %.3e" % (sname, n, L, dtype.__name__, i, rel))
        assert rel <= (1e-5 if dtype == np.float32 else 1e-13 * math.sqrt(L)), (i, rel)


# ---- hipGraph, workspace -------------------------------------------------------------------------------------------------
def test_hipgraph_capture_and_replay_and_workspace(gpu, W, oracle):
    """once wl_workspace_bytes_full(dtype, 1, {nvolumes * volume_stride}, L) is reserved the call allocates nothing (the workspace held
    is unchanged) and can be captured; replays on new data give the bits of the eager call.  A tail case, an axis case and a
    volume-after-volume case."""
    import torch
    s = torch.cuda.Stream()
    lib = W._lib.load()
    for n, nb, L, sname, want in ((16, 4, 4, "cdf97", BATCH), (64, 3, 3, "cdf97", BATCH), (16, 3, 4, "nc3", None)):
        sch = LS.scheme(W, sname)
        sets = [[rng_array((n, n, n), np.float32, 90 + 10 * k + i) for i in range(nb)] for k in range(3)]
        xb = _to_batch(W, sets[0])
        yb = W.similar(xb)
        with torch.cuda.stream(s):
            h, _ = W.transforms._context(gpu)
            nbytes = lib.wl_workspace_bytes_full(0, 1, (C.c_int64 * 3)(nb * n * n * n, 1, 1), L)
            assert lib.wl_ctx_reserve(h, nbytes) == 0
            held = lib.wl_ctx_workspace_held(h)
            W.dwt_batch(xb, sch, L, y=yb)                    # (first call: code objects loaded)
            torch.cuda.synchronize()
            assert lib.wl_ctx_workspace_held(h) == held, (held, lib.wl_ctx_workspace_held(h))
            assert want is None or W.last_kernel() == want
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            W.dwt_batch(xb, sch, L, y=yb)
        for k in (1, 2, 0):
            xb.copy_(_to_batch(W, sets[k]))
            eager = W.to_host(W.dwt_batch(xb, sch, L))
            yb.zero_()
            graph.replay()
            torch.cuda.synchronize()
            got = W.to_host(yb)
            assert np.array_equal(got, eager), (n, nb, L, sname, k)
            for i in range(nb):
                assert np.array_equal(got[..., i], oracle.dwt_lifting(sets[k][i], sch, L)), (n, nb, L, sname, k, i)
        with torch.cuda.stream(s):
            assert lib.wl_ctx_workspace_held(h) == held
        del graph


# ---- argument contract ---------------------------------------------------------------------------------------------------
def test_argument_contract_on_the_device(gpu, W):
    """each status code, in the documented order: an argument set that breaks rule k and every later rule reports rule k"""
    import torch
    sch = LS.scheme(W, "cdf97")
    ST = W._lib.STATUS
    buf = torch.zeros(2 * 4096 + 64, dtype=torch.float32, device=gpu)
    p = buf.data_ptr()

    def call(**kw):
        return ST[_raw_call(W, gpu, kw.pop("y", p), kw.pop("x", p), 16, kw.pop("nb", 2), kw.pop("stride", 4096), sch, kw.pop("L", 2), 1,
                            np.float32, **kw)]

    assert call() == "WL_OK"
    bad_all = dict(dtype_code=7, dims=(8, 16, 16), nb=0, L=-1, nsteps=-1)     # breaks every rule after the NULL checks
    assert call(ctx=None, **bad_all) == "WL_EINVAL_ARG"
    assert call(y=None, **bad_all) == "WL_EINVAL_ARG"
    assert call(x=None, **bad_all) == "WL_EINVAL_ARG"
    bad = dict(bad_all); bad["dims"] = "null"
    assert call(**bad) == "WL_EINVAL_ARG"
    assert call(**bad_all) == "WL_EINVAL_DTYPE"
    del bad_all["dtype_code"]
    assert call(**bad_all) == "WL_EINVAL_CUBE"                                 # the cube rule before the extents
    bad = dict(bad_all); bad["dims"] = (16, 16, 8)
    assert call(**bad) == "WL_EINVAL_CUBE"
    bad_all["dims"] = (12, 12, 12)                                              # 12 has no 2^3 factor (rule 6), ...
    assert call(stride=4096, **bad_all) == "WL_EDIMS"                          # nvolumes = 0
    bad_all["nb"] = 2
    assert call(stride=1727, **bad_all) == "WL_EDIMS"                          # volume_stride < 12^3
    assert call(dims=(0, 0, 0), nb=2, L=-1, nsteps=-1) == "WL_EDIMS"
    assert call(dims=(-4, -4, -4), nb=2, L=-1, nsteps=-1) == "WL_EDIMS"
    assert call(stride=4096, **bad_all) == "WL_EINVAL_L"                       # L = -1
    bad_all["L"] = 3
    assert call(stride=4096, **bad_all) == "WL_EINVAL_SIZE"
    assert call(nsteps=-1) == "WL_EINVAL_SCHEME"
    assert call(nsteps=17) == "WL_EINVAL_SCHEME"                               # more than WL_MAX_STEPS
    assert call(ncoef=[2, 0, 2, 2]) == "WL_EINVAL_SCHEME"
    assert call(ncoef=[2, 4, 2, 2]) == "WL_EINVAL_SCHEME"                      # more than WL_MAX_NCOEF
    torch.cuda.synchronize()
    assert call() == "WL_OK"


def test_host_mirror_on_the_device(gpu, W):
    """a 4-D tensor that is no batch of cubes keeps raising TypeError with a GLS; one volume takes the single-cube kernels"""
    import torch
    sch = LS.scheme(W, "cdf97")
    with pytest.raises(TypeError, match="cubes only"):
        W.dwt_batch(torch.zeros(3, 8, 8, 2, device=gpu).permute(3, 2, 1, 0), sch, 1)
    a = _volumes(16, np.float32)[0]
    yb = W.dwt_batch(_to_batch(W, [a]), sch, 4)
    kb = W.last_kernel()
    y1 = W.dwt(W.to_device(a), sch, 4)
    assert kb == W.last_kernel() == SINGLE
    assert np.array_equal(W.to_host(yb)[..., 0], W.to_host(y1))


# ---- translation-invariant denoise of cubes ------------------------------------------------------------------------------
def _oracle_denoise(oracle, x, wt, L, dnt, nspin, sigma=None):
    kind = type(dnt.th).__name__[:-2].lower()
    fwd = lambda a, l: oracle.dwt_lifting(a, wt, l)
    inv = lambda a, l: oracle.dwt_lifting(a, wt, l, fw=False)
    return oracle.denoise(x, fwd, inv, L, kind, dnt.t, TI=True, nspin=nspin, sigma=sigma)


def _noisy_cube(n, dtype, seed):
    g = np.linspace(0.0, 1.0, n)
    clean = np.sin(6.0 * g)[:, None, None] * np.cos(4.0 * g)[None, :, None] + (g > 0.5)[None, None, :]
    return (clean + 0.1 * np.random.default_rng(seed).standard_normal((n, n, n))).astype(dtype)


DENOISE_CASES = [
    # (scheme, side, nspin, L, threshold)
    ("cdf97", 16, (2, 3, 2), 3, None),
    ("db2", 32, (3, 2, 2), 2, ("SoftTH", 2.0)),
    ("twin_cdf97", 64, (2, 2, 2), 3, ("SteinTH", 1.2)),
    ("nc3", 16, (2, 2, 2), 2, None),
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: d.__name__)
@pytest.mark.parametrize("sname,n,nspin,L,th", DENOISE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_denoise_ti_cube(gpu, W, oracle, sname, n, nspin, L, th, dtype):
    """denoise(x, wt::GLS; TI = true) of a cube: one device-resident call, the bits of the reference's sequence"""
    wt = LS.scheme(W, sname)
    x = _noisy_cube(n, dtype, n)
    dnt = W.VisuShrink(n) if th is None else W.VisuShrink(getattr(W, th[0])(), th[1])
    xd = W.to_device(x)
    y = W.to_host(W.denoise(xd, wt, L=L, dnt=dnt, TI=True, nspin=nspin))
    assert W.last_kernel() == "denoise_ti_lifting", W.last_kernel()
    assert np.array_equal(W.to_host(xd), x), "input modified"
    e = _oracle_denoise(oracle, x, wt, L, dnt, nspin)
    assert y.dtype == dtype and np.array_equal(y, e), (sname, n, nspin, L, int((y != e).sum()))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: d.__name__)
def test_denoise_ti_cube_in_groups_and_custom_estimator(gpu, W, oracle, dtype):
    wt = LS.scheme(W, "cdf97")
    n, nspin = 32, (3, 2, 2)
    x = _noisy_cube(n, dtype, 5)
    xd = W.to_device(x)
    dnt = W.VisuShrink(n)
    e = _oracle_denoise(oracle, x, wt, 2, dnt, nspin)
    # a 1 MiB cap: one spin of 32^3 needs 2 N for the shifted copy and its coefficients beside one cube's transform workspace of
    # 4 N (0.75 MiB in Float32), two spins 8.5 N: the 12 spins run one per group, accumulated across the groups in spin order
    # The call runs on a stream of its own, so on a context that holds nothing yet: what it holds afterwards is the need of one group,
    # at least that of one spin and less than that of two (the formulas of denoise_ti_lifting_impl, in elements).
    import torch
    N, es = n ** 3, np.dtype(dtype).itemsize
    vols = lambda B: 2 * (B * (N // 8) + 64) + 2 * B * N + 64
    need = lambda B: (max(vols(B), 4 * N + 192) + 2 * N * B + n + 64) * es
    assert need(2) > (1 << 20)
    W.set_option("WL_TI_WS_CAP_MB", 1)
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            h, _ = W.transforms._context(gpu)
            lib = W._lib.load()
            assert lib.wl_ctx_workspace_held(h) == 0
            y = W.to_host(W.denoise(xd, wt, L=2, TI=True, nspin=nspin))
            assert W.last_kernel() == "denoise_ti_lifting"
            held = lib.wl_ctx_workspace_held(h)
        assert need(1) <= held < need(2), (need(1), held, need(2))              # one spin per group: 12 groups
    finally:
        W.clear_options()
    assert np.array_equal(y, e), int((y != e).sum())
    y = W.to_host(W.denoise(xd, wt, L=2, TI=True, nspin=nspin))
    assert np.array_equal(y, e)
    # L = 0 (dwt and idwt are copies) with a custom estnoise
    y0 = W.to_host(W.denoise(xd, wt, L=0, TI=True, nspin=(2, 2, 2), estnoise=lambda a, w: 0.3))
    assert W.last_kernel() == "denoise_ti_lifting"
    assert np.array_equal(y0, _oracle_denoise(oracle, x, wt, 0, dnt, (2, 2, 2), sigma=0.3))
    assert np.array_equal(W.to_host(xd), x)


def test_denoise_ti_box_is_refused(gpu, W):
    wt = LS.scheme(W, "cdf97")
    with pytest.raises(W.ArgumentError, match="square/cube"):
        W.denoise(W.to_device(rng_array((32, 32, 16), np.float32, 1)), wt, L=2, TI=True, nspin=(2, 2, 2))
