"""modwt_batch / imodwt_batch on the device (wl_modwt_batch / wl_imodwt_batch, W.modwt_batch / W.imodwt_batch): a panel of vectors,
unit u in column u.  Every result is compared bit for bit (np.array_equal) with the CPU oracle's modwt / imodwt of each unit; the
inverse input is the oracle's forward output.  Every shape runs on both tiers -- the LDS kernel where the unit fits, and the
per-level kernels under WL_MODWT_FUSED = 0 -- and the two must give the same bits.  Shapes, units and references: modwt_batch_cases.
"""
import ctypes as C

import numpy as np
import pytest

import modwt_batch_cases as MC

pytestmark = pytest.mark.gpu

SENT = {np.float32: 0xFFC5A5A5, np.float64: 0xFFF85A5A5A5A5A5A}          # a NaN payload no transform produces
TIERS = (("lds", {}), ("step", {"WL_MODWT_FUSED": 0}))


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def filt(W, name):
    return W.wavelet(getattr(W.WT, name))


def panel(W, us):
    """(B, n) host units -> the n x B column-major device panel"""
    return W.to_device(np.ascontiguousarray(us.T))


def coefs(W, co):
    """(B, L + 1, n) host coefficients -> the n x (L + 1) x B column-major device tensor"""
    return W.to_device(np.ascontiguousarray(co.transpose(2, 1, 0)))


def units_of(W, y):
    """n x (L + 1) x B device tensor -> (B, L + 1, n) host"""
    import torch
    torch.cuda.synchronize()
    return np.ascontiguousarray(W.to_host(y).transpose(2, 1, 0))


def fits_lds(n, dtype):
    return n <= MC.LDS_MAX[dtype]


def check(W, oracle, fname, n, B, dtype, L, opts=None):
    """forward and inverse of one shape on both tiers against the oracle; returns {tier: (forward kernel, inverse kernel)}"""
    import torch
    wt = filt(W, fname)
    us = MC.units(n, B, dtype)
    ye = MC.forward(oracle, W, fname, n, B, dtype, L)
    xe = MC.inverse(oracle, W, fname, n, B, dtype, L)
    xd, cd = panel(W, us), coefs(W, ye)
    names = {}
    for tier, o in TIERS:
        with W.options(**{**o, **(opts or {})}):
            y = W.modwt_batch(xd, wt, L)
            kf = W.last_kernel()
            assert tuple(y.shape) == (n, L + 1, B) and W.is_julia_layout(y)
            got = units_of(W, y)
            assert np.array_equal(ibits(got), ibits(ye)), ("fwd", tier, fname, n, B, L, kf, int((ibits(got) != ibits(ye)).sum()))
            xr = W.imodwt_batch(cd, wt)
            ki = W.last_kernel()
            assert tuple(xr.shape) == (n, B) and W.is_julia_layout(xr)
            torch.cuda.synchronize()
            gx = np.ascontiguousarray(W.to_host(xr).T)
            assert np.array_equal(ibits(gx), ibits(xe)), ("inv", tier, fname, n, B, L, ki, int((ibits(gx) != ibits(xe)).sum()))
        want = ("k_modwt_lds", "k_imodwt_lds") if tier == "lds" and fits_lds(n, dtype) else ("k_modwt_step_b", "k_imodwt_step_b")
        assert (kf, ki) == want, (tier, n, kf, ki)
        names[tier] = (kf, ki)
    if fname in MC.ORTHOGONAL:          # the bound test_gpu_ext.py holds the single calls to
        tol = (1e-4 if dtype == np.float32 else 1e-10) * max(1.0, float(np.abs(us).max()))
        assert np.abs(xe.astype(np.float64) - us.astype(np.float64)).max() <= tol, (fname, n, L)
    return names


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_wrap_around_on_tiny_units(gpu, W, oracle, dtype):
    """n in {2, 3, 8, 12}: the tap reach 2^(j-1) (F - 1) goes round the unit several times for the long filters"""
    for n, B, L in MC.shapes(dtype)["wrap"]:
        for fname in MC.FILTERS:
            check(W, oracle, fname, n, B, dtype, L)


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_several_units_per_workgroup(gpu, W, oracle, dtype):
    """n = 64 and n = 100: a workgroup of the LDS tier takes several whole units, the last one fewer; and a batch of one"""
    for n, B, L in MC.shapes(dtype)["packing"]:
        for fname in MC.FILTERS:
            check(W, oracle, fname, n, B, dtype, L)


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_tier_boundary(gpu, W, oracle, dtype):
    """the longest unit of the LDS tier and one 16-byte vector more: the two sides take different tiers"""
    (n0, B, L), (n1, _, _) = MC.shapes(dtype)["boundary"]
    for fname in MC.FILTERS:
        below = check(W, oracle, fname, n0, B, dtype, L)
        above = check(W, oracle, fname, n1, B, dtype, L)
        assert below["lds"] == ("k_modwt_lds", "k_imodwt_lds") and above["lds"] == ("k_modwt_step_b", "k_imodwt_step_b")
        assert below["lds"] != above["lds"]


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_long_units(gpu, W, oracle, dtype):
    for n, B, L in MC.shapes(dtype)["long"]:
        for fname in MC.FILTERS:
            check(W, oracle, fname, n, B, dtype, L)


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_groups_change_no_bit(gpu, W, oracle, dtype):
    """five units in groups of two (WL_MODWT_BATCH_GROUP = 2): two full groups and a short one on the per-level tier"""
    for n, B, L in MC.shapes(dtype)["groups"]:
        for fname in MC.FILTERS:
            check(W, oracle, fname, n, B, dtype, L, opts={"WL_MODWT_BATCH_GROUP": 2})
            check(W, oracle, fname, n, B, dtype, L)


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_unaligned_and_padded_panels_write_nothing_else(gpu, W, oracle, dtype):
    """n in {129, 1000}, B = 3, unit_stride = n + 3, ldo = n + 1, out_unit_stride = ldo (L + 1) + 5, every buffer one element off a
    16-byte boundary: the padding rows, the padding between units and the guard bands keep the sentinel's bits"""
    import torch
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    idt = torch.int32 if dtype == np.float32 else torch.int64
    sent = np.array([SENT[dtype]], dtype=np.uint32 if dtype == np.float32 else np.uint64).view(np.int32 if dtype == np.float32 else np.int64)[0]
    G = 33                                                                # guard elements: the bases are odd
    for n, B in MC.UNALIGNED:
        L = min(3, MC.maxlevels(n))
        xs, ld = n + 3, n + 1
        ous = ld * (L + 1) + 5
        us = MC.units(n, B, dtype)
        for fname in MC.FILTERS:
            wt = filt(W, fname)
            ye = MC.forward(oracle, W, fname, n, B, dtype, L)
            xe = MC.inverse(oracle, W, fname, n, B, dtype, L)
            for tier, o in TIERS:
                xbuf = torch.full((G + B * xs + G,), int(sent), dtype=idt, device=gpu).view(tdt)
                xv = xbuf.as_strided((n, B), (1, xs), G)
                xv.copy_(panel(W, us))
                ybuf = torch.full((G + B * ous + G,), int(sent), dtype=idt, device=gpu).view(tdt)
                yv = ybuf.as_strided((n, L + 1, B), (1, ld, ous), G)
                with W.options(**o):
                    out = W.modwt_batch(xv, wt, L, y=yv)
                    assert out.data_ptr() == yv.data_ptr() == ybuf.data_ptr() + G * ybuf.element_size()
                    torch.cuda.synchronize()
                    h = ibits(ybuf.cpu().numpy())
                    body = h[G: G + B * ous].reshape(B, ous)
                    mats = body[:, : ld * (L + 1)].reshape(B, L + 1, ld)
                    assert np.array_equal(mats[:, :, :n], ibits(ye)), ("fwd", tier, fname, n)
                    rest = np.concatenate((h[:G], mats[:, :, n:].ravel(), body[:, ld * (L + 1):].ravel(), h[G + B * ous:]))
                    assert np.all(rest == SENT[dtype]), ("padding written", tier, fname, n)
                    # the inverse reads the padded coefficients where they are and writes a padded panel
                    rbuf = torch.full((G + B * xs + G,), int(sent), dtype=idt, device=gpu).view(tdt)
                    cv = ybuf.as_strided((n, L + 1, B), (1, ld, ous), G)
                    gx = W.imodwt_batch(cv, wt)                               # (the Python mirror passes these strides through)
                    torch.cuda.synchronize()
                    assert np.array_equal(ibits(W.to_host(gx).T), ibits(xe)), ("inv", tier, fname, n, "mirror")
                    lib = W._lib.load()
                    hctx, st = W.transforms._context(gpu)
                    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
                    rc = lib.wl_imodwt_batch(hctx, 0 if dtype == np.float32 else 1, C.c_void_p(rbuf.data_ptr() + G * rbuf.element_size()), xs,
                                             C.c_void_p(cv.data_ptr()), ld, ous, n, L + 1, B, q.ctypes.data_as(C.POINTER(C.c_double)), len(q), st)
                    assert rc == 0, rc
                    torch.cuda.synchronize()
                    r = ibits(rbuf.cpu().numpy())
                    rb = r[G: G + B * xs].reshape(B, xs)
                    assert np.array_equal(rb[:, :n], ibits(xe)), ("inv", tier, fname, n)
                    assert np.all(np.concatenate((r[:G], rb[:, n:].ravel(), r[G + B * xs:])) == SENT[dtype]), ("inverse padding written", tier, fname, n)
                    # ... and the coefficients and the source panel are what they were
                    assert np.array_equal(ibits(ybuf.cpu().numpy()), h)
                    assert np.array_equal(ibits(xbuf.cpu().numpy())[G: G + B * xs].reshape(B, xs)[:, :n], ibits(us))


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_the_batch_is_the_loop_of_single_calls(gpu, W, oracle, dtype):
    """one shape per tier: column u of the batch is W.modwt / W.imodwt of column u"""
    import torch
    wt = filt(W, "db4")
    for n, B, L in ((1000, 4, 5), (MC.LDS_MAX[dtype] + 1024, 3, 4)):
        xd = panel(W, MC.units(n, B, dtype))
        y = W.modwt_batch(xd, wt, L)
        assert W.last_kernel() == ("k_modwt_lds" if fits_lds(n, dtype) else "k_modwt_step_b")
        xr = W.imodwt_batch(y, wt)
        torch.cuda.synchronize()
        for u in range(B):
            yu = W.modwt(xd[:, u].contiguous(), wt, L)
            assert torch.equal(y[:, :, u].view(torch.int32 if dtype == np.float32 else torch.int64),
                               yu.view(torch.int32 if dtype == np.float32 else torch.int64)), (n, u)
            xu = W.imodwt(yu, wt)
            assert torch.equal(xr[:, u].view(torch.int32 if dtype == np.float32 else torch.int64),
                               xu.view(torch.int32 if dtype == np.float32 else torch.int64)), (n, u, "inv")


def test_layouts_of_the_python_mirror(gpu, W, oracle):
    """a row-major panel and an integer panel are copied once into the dense layout; a single column of coefficients is copied out"""
    import torch
    wt = filt(W, "db2")
    n, B, L = 100, 4, 3
    us = MC.units(n, B, np.float64)
    ye = MC.forward(oracle, W, "db2", n, B, np.float64, L)
    rowmajor = torch.from_numpy(np.ascontiguousarray(us.T)).to(gpu)          # strides (B, 1)
    assert not W.is_julia_layout(rowmajor)
    assert np.array_equal(units_of(W, W.modwt_batch(rowmajor, wt, L)), ye)
    ints = torch.arange(n * B, device=gpu).reshape(B, n).t()
    yi = units_of(W, W.modwt_batch(ints, wt, L))
    assert yi.dtype == np.float64
    for u in range(B):
        assert np.array_equal(yi[u].T, oracle.modwt(np.arange(u * n, (u + 1) * n, dtype=np.float64), wt.qmf, L))
    one = coefs(W, ye[:, L:, :])                                             # ncols = 1: the scaling column is the signal
    xr = W.imodwt_batch(one, wt)
    torch.cuda.synchronize()
    assert W.last_kernel() == "copy" and np.array_equal(W.to_host(xr).T, ye[:, L, :])
    assert np.array_equal(units_of(W, W.modwt_batch(panel(W, us), wt)), MC.forward(oracle, W, "db2", n, B, np.float64, 6))   # L = floor(log2 n)
    with pytest.raises(W.ArgumentError, match="Too many transform levels"):
        W.modwt_batch(panel(W, us), wt, 7)
    with pytest.raises(W.DimensionMismatch):
        W.modwt_batch(panel(W, us), wt, 3, y=W.similar(coefs(W, ye))[:, :3, :])


# ---- hipGraph ----------------------------------------------------------------------------------------------------------------------
def _hip():
    """the HIP runtime this process already uses"""
    for line in open("/proc/self/maps"):
        if "libamdhip64.so" in line:
            return C.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime loaded")


def test_hipgraph_capture_is_a_linear_chain_and_replays(gpu, W):
    """modwt_batch then imodwt_batch at 1024 x 16, L = 4, captured on one stream after a warm-up call has grown the workspace:
    replays on fresh input give the eager bits, on both tiers; the captured graph is a chain (every node has at most one
    predecessor and one successor, edges = nodes - 1)"""
    import torch
    n, B, L = 1024, 16, 4
    wt = filt(W, "db4")
    inputs = [np.asfortranarray(np.random.default_rng(s).standard_normal((n, B)).astype(np.float32)) for s in (1, 2, 3)]
    hip = _hip()
    for tier, o in TIERS:
        with W.options(**o):
            eager = []
            for a in inputs:
                ya = W.modwt_batch(W.to_device(a), wt, L)
                eager.append((W.to_host(ya), W.to_host(W.imodwt_batch(ya, wt))))
            x = W.to_device(inputs[0])
            y = torch.empty((B, L + 1, n), dtype=torch.float32, device=gpu).permute(2, 1, 0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                W.modwt_batch(x, wt, L, y=y)                                 # warm-up on the capture stream
                W.imodwt_batch(y, wt)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                W.modwt_batch(x, wt, L, y=y)
                xr = W.imodwt_batch(y, wt)
            for k in (1, 2):
                x.copy_(W.to_device(inputs[k]))
                y.zero_()
                xr.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert np.array_equal(ibits(W.to_host(y)), ibits(eager[k][0])), (tier, k)
                assert np.array_equal(ibits(W.to_host(xr)), ibits(eager[k][1])), (tier, k)
            del graph
            # the topology, through the runtime's own capture of the same two calls
            with torch.cuda.stream(s):
                hctx, _ = W.transforms._context(gpu)                             # the context of the capture stream: its workspace is grown
            lib = W._lib.load()
            q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
            qp = q.ctypes.data_as(C.POINTER(C.c_double))
            xo = torch.empty((B, n), dtype=torch.float32, device=gpu)
            st = C.c_void_p(s.cuda_stream)
            g = C.c_void_p()
            torch.cuda.synchronize()
            assert hip.hipStreamBeginCapture(st, 2) == 0                        # hipStreamCaptureModeRelaxed
            rc1 = lib.wl_modwt_batch(hctx, 0, C.c_void_p(y.data_ptr()), n, n * (L + 1), C.c_void_p(x.data_ptr()), n, B, n, qp, len(q), L, st)
            rc2 = lib.wl_imodwt_batch(hctx, 0, C.c_void_p(xo.data_ptr()), n, C.c_void_p(y.data_ptr()), n, n * (L + 1), n, L + 1, B, qp, len(q), st)
            assert hip.hipStreamEndCapture(st, C.byref(g)) == 0 and (rc1, rc2) == (0, 0)
            nn, ne = C.c_size_t(0), C.c_size_t(0)
            assert hip.hipGraphGetNodes(g, None, C.byref(nn)) == 0 and hip.hipGraphGetEdges(g, None, None, C.byref(ne)) == 0
            want = 2 if tier == "lds" else 2 * L
            assert nn.value == want and ne.value == want - 1, (tier, nn.value, ne.value)
            src, dst = (C.c_void_p * ne.value)(), (C.c_void_p * ne.value)()
            assert hip.hipGraphGetEdges(g, src, dst, C.byref(ne)) == 0
            assert len(set(src)) == len(set(dst)) == ne.value, "a node with two successors or two predecessors"
            assert hip.hipGraphDestroy(g) == 0
