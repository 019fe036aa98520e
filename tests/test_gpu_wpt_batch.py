"""Batched wavelet packet transforms on the device (wl_wpt_filter_batch / wl_wpt_lifting_batch, W.wpt_batch / W.iwpt_batch): nunits
signals that share one tree, unit i at element offset i * unit_stride.  Every result is compared bit for bit (np.array_equal) with
the CPU oracle's packet transform of each unit; the inverse input is the oracle's forward output.  Every buffer sits between guard
bands and a padded batch carries a sentinel in its padding: both are read back after the call.  Batches with many units repeat
PERIOD distinct columns, so the oracle runs PERIOD times and its answer is tiled."""
import ctypes as C

import numpy as np
import pytest

import lifting_schemes as LS

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements on either side of a buffer (a multiple of 16 bytes for both element types)
SENT = -7.25                    # what guard bands and padding hold
PERIOD = 7
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
CODE = {np.float32: 0, np.float64: 1}
ST = {"WL_EINVAL_L": -2, "WL_EALIAS": -3, "WL_EDIMS": -4, "WL_EINVAL_TREE": -6, "WL_EINVAL_SCHEME": -7, "WL_EINVAL_DTYPE": -8,
      "WL_EINVAL_FILTER": -9, "WL_EINVAL_ARG": -10}


def TS(dtype):
    """wpt_tile_samples: what one workgroup of the packet kernels holds"""
    return 16384 // np.dtype(dtype).itemsize


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def columns(n, B, dtype, seed):
    """(B, n): PERIOD distinct seeded columns, repeated"""
    d = np.random.default_rng(seed).standard_normal((min(B, PERIOD), n)).astype(dtype)
    return d[np.arange(B) % d.shape[0]]


def full_tree(W, n, tree):
    return W.maketree(n, int(tree), "full") if isinstance(tree, (int, np.integer)) else tree


def expect(W, oracle, wt, us, tree, fw):
    """the oracle's transform of every distinct column of `us`, tiled"""
    B, n = us.shape
    t = np.ascontiguousarray(full_tree(W, n, tree), dtype=np.uint8)
    k = min(B, PERIOD)
    if isinstance(wt, W.OrthoFilter):
        d = [oracle.wpt_filter(np.ascontiguousarray(us[i]), wt.qmf, t.copy(), fw=fw) for i in range(k)]
    else:
        d = [oracle.wpt_lifting(np.ascontiguousarray(us[i]), wt, t.copy(), fw=fw) for i in range(k)]
    return np.stack(d)[np.arange(B) % k]


def random_tree(W, n, depth, seed, p=0.6):
    rs = np.random.default_rng(seed)
    nn = 2 ** W.maxtransformlevels(n) - 1
    t = np.zeros(nn, dtype=np.uint8)
    t[0] = 1
    for i in range(1, min(nn, 2 ** depth - 1)):
        t[i] = 1 if (t[(i + 1) // 2 - 1] and rs.random() < p) else 0
    return t


def lopsided_tree(W, n, depth, p=0.6):
    """a seeded random valid tree whose left and right subtrees differ below both children of the root"""
    for seed in range(1000):
        t = random_tree(W, n, depth, seed, p)
        if t[1] and t[2] and not np.array_equal(t[3:5], t[5:7]):
            return t
    raise AssertionError("no lopsided tree found")


def padded(torch, gpu, us, S, off=0):
    B, n = us.shape
    base = GUARD + off
    buf = np.full(base + B * S + GUARD, SENT, dtype=us.dtype)
    buf[base: base + B * S].reshape(B, S)[:, :n] = us
    return torch.from_numpy(buf).to(gpu), base


def unpack(torch, buf, base, B, n, S):
    """(units (B, n), True when every guard / padding element still holds the sentinel)"""
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    if S == n:
        out = h[base: base + B * n].reshape(B, n).copy()
        rest = np.concatenate((h[:base], h[base + B * n:]))
    else:
        body = h[base: base + B * S].reshape(B, S)
        out = body[:, :n].copy()
        rest = np.concatenate((h[:base], body[:, n:].ravel(), h[base + B * S:]))
    return out, bool(np.all(rest == h.dtype.type(SENT)))


def ptr(buf, base):
    return C.c_void_p(buf.data_ptr() + base * buf.element_size())


def raw_call(W, h, st, wt, dtype, y, x, n, B, S, tree, fw):
    lib = W._lib.load()
    if isinstance(tree, (int, np.integer)):
        tp, nt, L = None, 0, int(tree)
    else:
        tree = np.ascontiguousarray(tree, dtype=np.uint8)
        tp, nt, L = tree.ctypes.data_as(C.POINTER(C.c_uint8)), len(tree), 0
    if isinstance(wt, W.OrthoFilter):
        q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
        return lib.wl_wpt_filter_batch(h, CODE[dtype], y, x, n, B, S, q.ctypes.data_as(C.POINTER(C.c_double)), len(q), tp, nt, L,
                                       1 if fw else 0, st)
    iu, nc, sh, cf = wt.flatten()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    return lib.wl_wpt_lifting_batch(h, CODE[dtype], y, x, n, B, S, len(iu), ip(iu), ip(nc), ip(sh), cf.ctypes.data_as(C.POINTER(C.c_double)),
                                    wt.norm1, wt.norm2, tp, nt, L, 1 if fw else 0, st)


def run(W, torch, gpu, wt, us, tree, fw, S=None, off=0, inplace=False):
    """one batch call on guarded (and, for S > n, padded) buffers -> the units of y; the guards, the padding and (out of place) the
    source are checked here"""
    B, n = us.shape
    S = n if S is None else S
    xb, base = padded(torch, gpu, us, S, off)
    yb = xb if inplace else padded(torch, gpu, np.full_like(us, SENT), S, off)[0]
    h, st = W.transforms._context(xb.device)
    rc = raw_call(W, h, st, wt, us.dtype.type, ptr(yb, base), ptr(xb, base), n, B, S, tree, fw)
    assert rc == 0, (rc, n, B, S)
    got, clean = unpack(torch, yb, base, B, n, S)
    assert clean, ("guard bands / padding written", n, B, S, off)
    if not inplace:
        src, sclean = unpack(torch, xb, base, B, n, S)
        assert sclean and np.array_equal(ibits(src), ibits(us)), ("source changed", n, B, S)
    return got


def check(W, torch, gpu, oracle, wt, n, B, dtype, tree, seed, S=None, off=0, inplace=False, kernel=None):
    """forward and inverse of one case against the oracle; returns the kernel names"""
    us = columns(n, B, dtype, seed)
    ye = expect(W, oracle, wt, us, tree, True)
    y = run(W, torch, gpu, wt, us, tree, True, S, off, inplace)
    kf = W.last_kernel()
    assert np.array_equal(y, ye), ("fwd", n, B, dtype.__name__, S, off, kf, int((ibits(y) != ibits(ye)).sum()))
    xe = expect(W, oracle, wt, ye, tree, False)
    xr = run(W, torch, gpu, wt, ye, tree, False, S, off, inplace)
    ki = W.last_kernel()
    assert np.array_equal(xr, xe), ("inv", n, B, dtype.__name__, S, off, ki, int((ibits(xr) != ibits(xe)).sum()))
    if kernel is not None:
        assert kf.startswith(kernel[0]) and ki.startswith(kernel[1]), (n, B, kf, ki)
    return kf, ki


def filt(W, name):
    return W.wavelet(getattr(W.WT, name))


# ---- several units per tail workgroup ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [2, 4, 16, 256, 1024])
def test_several_units_per_tail_workgroup(gpu, W, oracle, dtype, n):
    """n < TS: a workgroup of k_wpt_*_tail takes TS / n whole units; the last one takes what is left.  (n = 2 in Float32 is shorter
    than a 16-byte vector: the single-unit plan has no packet kernel for it and the batch follows that plan.)"""
    import torch
    upw = TS(dtype) // n
    Lmax = W.maxtransformlevels(n)
    packet = n * np.dtype(dtype).itemsize >= 16
    for B in (1, 3, upw - 1, upw, upw + 1, 2 * upw + 1):
        for depth in sorted({Lmax, 1}):
            for fname in ("haar", "db2", "db4", "sym5"):
                kf, ki = check(W, torch, gpu, oracle, filt(W, fname), n, B, dtype, depth, 31 * n + B)
                if packet:
                    assert (kf, ki) == ("k_wpt_fwd_tail", "k_wpt_inv_tail"), (n, B, depth, fname, kf, ki)


# ---- one unit per workgroup and the fused passes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_passes_then_tail(gpu, W, oracle, dtype):
    """n >= TS: the tiles of all units in one k_wpt_fwd_multi / k_wpt_inv_multi launch, then the tail on one unit's chunks.  The
    forward plan fuses 3 depths at 8 TS, 2 + 2 (Float32) / 3 + 2 (Float64) at 2^16, 2 at 8 TS with depth 2, and 1 depth where a
    partially split tree starts at 2 TS (a fully split single depth there is the streaming line kernel, then the tail)."""
    import torch
    ts = TS(dtype)
    for n in (ts, 2 * ts, 8 * ts, 1 << 16):
        Lmax = W.maxtransformlevels(n)
        for B in (1, 3):
            for depth in (Lmax, 2):
                kf, ki = check(W, torch, gpu, oracle, filt(W, "db4"), n, B, dtype, depth, n + B)
                if n >= 8 * ts:
                    assert (kf, ki) == ("k_wpt_fwd_multi", "k_wpt_inv_multi"), (n, B, depth, kf, ki)
                elif n == ts:
                    assert (kf, ki) == ("k_wpt_fwd_tail", "k_wpt_inv_tail"), (n, B, depth, kf, ki)
            check(W, torch, gpu, oracle, filt(W, "haar"), n, B, dtype, Lmax, n + B + 1)
    kf, ki = check(W, torch, gpu, oracle, filt(W, "db4"), 2 * ts, 3, dtype, W.maketree(2 * ts, 5, "dwt"), 77)
    # (the inverse takes the deep depths in the tail; depth 0 alone, fully split, is the streaming line kernel)
    assert (kf, ki) == ("k_wpt_fwd_multi", "k_wpt_inv_tail"), (kf, ki)


# ---- one partially split tree shared by all units --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_shared_partial_trees(gpu, W, oracle, dtype):
    """the node bits are indexed by the segment INSIDE the unit: unit i >= 1 takes the bits of unit 0 (a random tree with distinct
    left / right subtrees would show a global segment index).  Units 0, 2 and 4 hold the same column and must give the same bits."""
    import torch
    B = 5
    for n in (256, 8 * TS(dtype)):
        Lmax = W.maxtransformlevels(n)
        root = np.zeros(2 ** Lmax - 1, dtype=np.uint8)
        root[0] = 1
        trees = [W.maketree(n, Lmax, "dwt"), W.maketree(n, 3, "dwt"), lopsided_tree(W, n, Lmax), lopsided_tree(W, n, 6, 0.45), root,
                 np.zeros(2 ** Lmax - 1, dtype=np.uint8)]
        for ti, tree in enumerate(trees):
            two = np.random.default_rng(n + ti).standard_normal((2, n)).astype(dtype)
            us = two[np.arange(B) % 2]
            for wt in (filt(W, "db4"), filt(W, "haar"), LS.scheme(W, "cdf97")):
                for fw in (True, False):
                    ye = expect(W, oracle, wt, us[:2], tree, fw)[np.arange(B) % 2]
                    y = run(W, torch, gpu, wt, us, tree, fw, inplace=not isinstance(wt, W.OrthoFilter))
                    assert np.array_equal(ibits(y[2]), ibits(y[0])) and np.array_equal(ibits(y[4]), ibits(y[0])), (n, ti, fw)
                    assert np.array_equal(y, ye), (n, ti, fw, W.last_kernel())
            if not tree[0]:
                assert W.last_kernel() == "copy"


# ---- lengths that are no power of two ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_non_power_of_two_lengths(gpu, W, oracle, dtype):
    """n = 40: the per-depth kernels only (unit = third extent); 3 TS and 6 TS: a fused pass first, the per-depth kernels below"""
    import torch
    ts = TS(dtype)
    for n in (40, 3 * ts, 6 * ts):
        Lmax = W.maxtransformlevels(n)
        for fname in ("db4", "haar"):
            kf, ki = check(W, torch, gpu, oracle, filt(W, fname), n, 3, dtype, Lmax, n)
            if n == 40:
                assert "generic" in kf and "generic" in ki, (kf, ki)
        check(W, torch, gpu, oracle, filt(W, "db4"), n, 3, dtype, random_tree(W, n, Lmax, 9), n + 1)
        check(W, torch, gpu, oracle, LS.scheme(W, "cdf97"), n, 3, dtype, Lmax, n + 2, inplace=True)


# ---- strides and misaligned views ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_strides_and_views(gpu, W, oracle, dtype):
    """unit_stride n (dense), n + 4 (16-byte aligned unit bases for both types), n + 2 (Float64 only), n + 1 (neither): aligned
    batches take the packet kernels, the others the per-depth kernels; so does a view that starts one element off the grid"""
    import torch
    es = np.dtype(dtype).itemsize
    for n in (16, 1024, 2 * TS(dtype)):
        Lmax = W.maxtransformlevels(n)
        for pad in (0, 4, 2, 1):
            for off in (0, 1):
                for tree in (Lmax, W.maketree(n, min(Lmax, 4), "dwt")):
                    kf, ki = check(W, torch, gpu, oracle, filt(W, "db4"), n, 3, dtype, tree, n + pad, S=n + pad, off=off)
                    aligned = off == 0 and ((n + pad) * es) % 16 == 0
                    assert kf.startswith("k_wpt_fwd") == aligned and ki.startswith("k_wpt_inv") == aligned, (n, pad, off, kf, ki)


# ---- filters the packet kernels do not take -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fallback_filters(gpu, W, oracle, dtype):
    """db6 (12 taps) and the 23-tap Battle filter: one launch of the line / per-depth kernels per depth over all units"""
    import torch
    batt = [f for f in (filt(W, "batt2"), filt(W, "batt4"), filt(W, "batt6")) if len(f.qmf) == 23]
    assert len(batt) == 1
    for wt in (filt(W, "db6"), batt[0]):
        for n in (64, 2048):
            for pad in (0, 4):
                for tree in (W.maxtransformlevels(n), random_tree(W, n, 5, 3)):
                    kf, ki = check(W, torch, gpu, oracle, wt, n, 3, dtype, tree, n + pad, S=n + pad)
                    assert not kf.startswith("k_wpt") and not ki.startswith("k_wpt"), (kf, ki)
    # the per-depth family on request: wl_ctx_set_path(ctx, 1)
    W.set_kernel_path(1)
    try:
        kf, ki = check(W, torch, gpu, oracle, filt(W, "db4"), 1024, 3, dtype, 10, 5)
        assert "generic" in kf and "generic" in ki, (kf, ki)
    finally:
        W.set_kernel_path(0)


# ---- lifting -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lifting(gpu, W, oracle, dtype):
    """cdf9/7, haar, db2 and a user scheme; in place (y == x) and out of place (x unchanged: checked in run()); dense batches (fully
    split depths on the fused line kernels over all segments of all units) and padded ones (per-depth passes, unit = third extent)"""
    import torch
    for sname in ("cdf97", "haar", "db2", "nc3"):
        sch = LS.scheme(W, sname)
        for n in (64, 8192):
            Lmax = W.maxtransformlevels(n)
            for pad in (0, 4, 1):
                for tree in (Lmax, 3, W.maketree(n, 4, "dwt"), random_tree(W, n, 6, 11)):
                    for inplace in (True, False):
                        check(W, torch, gpu, oracle, sch, n, 3, dtype, tree, n + pad, S=n + pad, inplace=inplace)
    check(W, torch, gpu, oracle, LS.scheme(W, "cdf97"), 256, 2 * PERIOD + 3, dtype, 8, 1)
    assert not W.last_kernel().startswith("k_generic"), W.last_kernel()


# ---- groups ----------------------------------------------------------------------------------------------------------------------------------
def test_groups_change_no_bit(gpu, W, oracle):
    import torch
    for dtype in DTYPES:
        for n in (256, 2 * TS(dtype)):
            Lmax = W.maxtransformlevels(n)
            with W.options(WL_WPT_BATCH_GROUP=2):
                for wt in (filt(W, "db4"), LS.scheme(W, "cdf97")):
                    for tree in (Lmax, random_tree(W, n, 6, 2)):
                        for pad in (0, 4):
                            check(W, torch, gpu, oracle, wt, n, 5, dtype, tree, n, S=n + pad, inplace=not isinstance(wt, W.OrthoFilter))
    # a work buffer cap of 1 MiB: 40 units of 8192 Float32 (1.25 MiB) run in two groups
    with W.options(WL_TI_WS_CAP_MB=1):
        check(W, torch, gpu, oracle, filt(W, "db4"), 8192, 40, np.float32, 13, 4)
    # one real crossing of the default group size: 65537 units of 16 (4 MiB)
    check(W, torch, gpu, oracle, filt(W, "db4"), 16, 65537, np.float32, 4, 8)
    check(W, torch, gpu, oracle, LS.scheme(W, "cdf97"), 16, 65537, np.float32, 4, 8, inplace=True)


# ---- device against device ---------------------------------------------------------------------------------------------------------------------
def _batch_vs_loop(W, torch, seed, ncases):
    rs = np.random.default_rng(seed)
    names = ("haar", "db2", "db4", "sym5", "db6")
    worst = []
    for _ in range(ncases):
        dtype = DTYPES[int(rs.integers(2))]
        n = int(2 ** rs.integers(1, 17)) * (3 if rs.random() < 0.2 else 1)
        B = int(rs.integers(1, 9)) if n > 4096 else int(rs.integers(1, 70))
        Lmax = W.maxtransformlevels(n)
        depth = int(rs.integers(0, Lmax + 1))
        fname = names[int(rs.integers(len(names)))]
        wt = filt(W, fname)
        tree = depth if rs.random() < 0.6 else random_tree(W, n, max(depth, 1), int(rs.integers(1 << 30)))
        xh = np.asfortranarray(rs.standard_normal((n, B)).astype(dtype))
        x = W.to_device(xh)
        for f, f1 in ((W.wpt_batch, W.wpt_), (W.iwpt_batch, W.iwpt_)):
            yb = f(x, wt, tree)
            kb = W.last_kernel()
            ref = W.similar(x)
            for i in range(B):
                f1(ref[:, i], x[:, i], wt, tree)
            k1 = W.last_kernel()
            torch.cuda.synchronize()
            same = np.array_equal(ibits(W.to_host(yb)), ibits(W.to_host(ref)))
            assert kb == k1, (n, B, depth, fname, kb, k1)
            if not same:
                worst.append((n, B, depth, fname, dtype.__name__, kb))
    return worst


def test_batch_equals_the_loop_of_single_calls(gpu, W):
    """seeded random (n, B, depth or tree, filter, dtype): the batch equals B calls of wpt_ / iwpt_ as integer bit patterns, and
    wl_last_kernel names the single-unit call's kernel: the plan is the single unit's, every launch is over all units (the single
    transform is the batch of one of the same kernel instances), there is no loop over the units to fall back on"""
    import torch
    assert _batch_vs_loop(W, torch, 20261, 40) == []


def test_batch_equals_the_loop_in_the_fused_library(gpu, W):
    """the same under W.set_arithmetic("fused"): the plan is the single unit's and batch and single call run the same kernel
    instances, so the bits match there too (orthogonal filters; a lifting batch hands nseg * nunits lines to the line kernels, whose
    choice of tier depends on the line count: test_lifting_in_the_fused_library holds it to the oracle)"""
    import torch
    with W.arithmetic("fused"):
        assert _batch_vs_loop(W, torch, 20262, 24) == []
    assert W.get_arithmetic() == "exact"


def _fused_close(y, ref, depths):
    """the tolerances of tests/test_gpu_fused.py, per unit"""
    f64 = ref.dtype == np.float64
    for u in range(ref.shape[0]):
        a, b = y[u].astype(np.float64), ref[u].astype(np.float64)
        rel = np.linalg.norm(a - b) / np.linalg.norm(b)
        assert rel <= (1e-13 if f64 else 1e-6) * np.sqrt(max(depths, 1)), (u, rel)
        if not f64:
            assert np.abs(a - b).max() <= 1e-5 * max(1.0, np.abs(b).max()), (u, np.abs(a - b).max())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lifting_in_the_fused_library(gpu, W, oracle, dtype):
    """Lifting batches under W.set_arithmetic("fused").  A dense batch hands nseg * nunits lines to the fused line kernels, whose tier
    depends on the line count (the LDS tail takes more samples from 32 lines on), and a padded batch takes the per-depth passes, so
    the plan is not the single unit's and the fused bits need not be the loop's.  These cases -- every lifting batch: cdf9/7, db2 and a
    user scheme, 3 and 40 units of 64 and 8192 samples, dense and padded, full and dwt-shaped trees, in place and out of place, and
    the complex lifting packet transform, whose two planes are one such batch -- are held to the oracle with the fused library's
    tolerances (relative L2 <= 1e-6 sqrt(depths) Float32 with max error <= 1e-5 max(1, |ref|), 1e-13 sqrt(depths) Float64)."""
    import torch
    with W.arithmetic("fused"):
        for sname in ("cdf97", "db2", "nc3"):
            sch = LS.scheme(W, sname)
            for n, B in ((64, 3), (64, 40), (8192, 3), (8192, 40)):
                Lmax = W.maxtransformlevels(n)
                for pad in (0, 4):
                    for tree, depths in ((Lmax, Lmax), (W.maketree(n, 4, "dwt"), 4)):
                        us = columns(n, B, dtype, n + B + pad)
                        for fw in (True, False):
                            ref = expect(W, oracle, sch, us, tree, fw)
                            for inplace in (True, False):
                                _fused_close(run(W, torch, gpu, sch, us, tree, fw, S=n + pad, inplace=inplace), ref, depths)
        # the complex packet transform with a lifting scheme: its two planes are one batch of two units
        sch = LS.scheme(W, "cdf97")
        cdt = torch.complex64 if dtype == np.float32 else torch.complex128
        with W.complex_arrays():
            for n in (64, 4096):
                L = W.maxtransformlevels(n)
                us = columns(n, 2, dtype, n + 5)
                z = torch.complex(W.to_device(us[0].copy()), W.to_device(us[1].copy()))
                assert z.dtype == cdt
                for f, fw in ((W.wpt, True), (W.iwpt, False)):
                    zh = W.to_host(f(z, sch, L))
                    _fused_close(np.stack([zh.real, zh.imag]).astype(dtype), expect(W, oracle, sch, us, L, fw), L)
    assert W.get_arithmetic() == "exact"


# ---- host mirror -------------------------------------------------------------------------------------------------------------------------------
def test_python_mirror(gpu, W, oracle):
    import torch
    n, B = 512, 6
    xh = np.asfortranarray(np.random.default_rng(3).standard_normal((n, B)).astype(np.float32))
    x = W.to_device(xh)
    wt, sch = filt(W, "db4"), LS.scheme(W, "cdf97")
    tree = W.maketree(n, 5, "dwt")
    for t in (None, 4, tree):
        tt = W.maxtransformlevels(n) if t is None else t
        y = W.wpt_batch(x, wt, t)
        assert np.array_equal(W.to_host(y).T, expect(W, oracle, wt, xh.T, tt, True))
        assert np.array_equal(W.to_host(W.iwpt_batch(y, wt, t)).T, expect(W, oracle, wt, W.to_host(y).T, tt, False))
        z = W.wpt_batch(x, sch, t)
        assert z.data_ptr() != x.data_ptr() and np.array_equal(W.to_host(x), xh)
        assert np.array_equal(W.to_host(z).T, expect(W, oracle, sch, xh.T, tt, True))
        w = x.clone()
        assert W.wpt_batch(w, sch, t, y=w) is w and np.array_equal(W.to_host(w), W.to_host(z))       # y = x: in place
    out = W.similar(x)
    assert W.wpt_batch(x, wt, 3, y=out) is out
    with pytest.raises(W.ArgumentError, match="in array is out array"):
        W.wpt_batch(x, wt, 3, y=x)
    with pytest.raises(W.DimensionMismatch):
        W.wpt_batch(x, wt, 3, y=W.similar(x[:, :3]))
    with pytest.raises(TypeError):
        W.wpt_batch(x, wt, 3, y=W.similar(x, dtype=torch.float64))
    with pytest.raises(W.ArgumentError):
        W.wpt_batch(x, wt, 3, y=torch.empty((n, B), dtype=torch.float32, device=gpu))               # row-major: not Julia layout
    with pytest.raises(TypeError, match="wpt_batch"):
        W.wpt_batch(x[:, 0], wt)
    with pytest.raises(AssertionError):
        W.wpt_batch(x, wt, 10)
    with pytest.raises(TypeError):
        W.iwpt_batch(x, "db4")
    with W.complex_arrays():
        with pytest.raises(TypeError, match="wpt_batch"):
            W.wpt_batch(torch.zeros((8, 2), dtype=torch.complex64, device=gpu).t().contiguous().t(), wt)


# ---- hipGraph ----------------------------------------------------------------------------------------------------------------------------------
def test_hipgraph_capture_and_replay(gpu, W):
    """the full-tree form captured on one stream after a warm call has grown the workspace, replayed on new data of the same shape"""
    import torch
    n, B = 4096, 12
    wt = filt(W, "db4")
    inputs = [np.asfortranarray(np.random.default_rng(s).standard_normal((n, B)).astype(np.float32)) for s in (1, 2, 3)]
    eager = [W.to_host(W.wpt_batch(W.to_device(a), wt, 12)) for a in inputs]
    x = W.to_device(inputs[0])
    y = W.similar(x)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        W.wpt_batch(x, wt, 12, y=y)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        W.wpt_batch(x, wt, 12, y=y)
    for k in (1, 2):
        x.copy_(W.to_device(inputs[k]))
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ibits(W.to_host(y)), ibits(eager[k])), k
    del graph


# ---- status codes and the workspace rule ---------------------------------------------------------------------------------------------------
def test_status_codes_in_order(gpu, W):
    import torch
    lib = W._lib.load()
    n, B, S = 64, 3, 68
    us = columns(n, B, np.float32, 1)
    xb, base = padded(torch, gpu, us, S)
    yb, _ = padded(torch, gpu, np.full_like(us, SENT), S)
    h, st = W.transforms._context(xb.device)
    q = np.ascontiguousarray(filt(W, "db2").qmf, dtype=np.float64)
    qp = q.ctypes.data_as(C.POINTER(C.c_double))
    sch = LS.scheme(W, "cdf97")
    iu, nc, sh, cf = sch.flatten()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    bad = np.zeros(63, dtype=np.uint8)
    bad[1] = 1                                                          # a child without its parent
    badp = bad.ctypes.data_as(C.POINTER(C.c_uint8))
    X, Y, null = ptr(xb, base), ptr(yb, base), C.c_void_p(None)

    def f(ctx=h, y=Y, x=X, dtype=0, n=n, B=B, S=S, q_=qp, flen=4, tree=None, nt=0, L=2):
        return lib.wl_wpt_filter_batch(ctx, dtype, y, x, n, B, S, q_, flen, tree, nt, L, 1, st)

    def g(ctx=h, y=Y, x=X, dtype=0, n=n, B=B, S=S, nsteps=len(iu), tree=None, nt=0, L=2):
        return lib.wl_wpt_lifting_batch(ctx, dtype, y, x, n, B, S, nsteps, ip(iu), ip(nc), ip(sh), cf.ctypes.data_as(C.POINTER(C.c_double)),
                                        sch.norm1, sch.norm2, tree, nt, L, 1, st)

    assert f(ctx=null) == f(y=null) == f(x=null) == f(q_=None) == ST["WL_EINVAL_ARG"]
    assert g(ctx=null) == g(y=null) == g(x=null) == ST["WL_EINVAL_ARG"]
    assert f(dtype=2) == g(dtype=-1) == ST["WL_EINVAL_DTYPE"]
    assert f(flen=1) == f(flen=65) == ST["WL_EINVAL_FILTER"]
    assert g(nsteps=17) == ST["WL_EINVAL_SCHEME"]
    assert f(n=0) == f(B=0) == f(S=63) == g(n=0) == g(B=0) == g(S=63) == ST["WL_EDIMS"]
    assert f(y=X) == ST["WL_EALIAS"]
    assert f(L=-1) == f(L=7) == g(L=-1) == g(L=7) == ST["WL_EINVAL_L"]
    assert f(tree=badp, nt=63) == g(tree=badp, nt=63) == f(tree=badp, nt=62) == ST["WL_EINVAL_TREE"]
    # the order: an earlier rule wins over every later one
    assert f(y=null, dtype=2, flen=1, B=0, L=-1) == ST["WL_EINVAL_ARG"]
    assert f(dtype=2, flen=1, B=0, y=X, L=-1) == ST["WL_EINVAL_DTYPE"]
    assert f(flen=1, B=0, y=X, L=-1) == ST["WL_EINVAL_FILTER"]
    assert f(B=0, y=X, L=-1) == ST["WL_EDIMS"]
    assert f(y=X, L=-1) == f(y=X, tree=badp, nt=63) == ST["WL_EALIAS"]
    assert g(dtype=2, nsteps=17, B=0, L=-1) == ST["WL_EINVAL_DTYPE"]
    assert g(nsteps=17, B=0, L=-1) == ST["WL_EINVAL_SCHEME"]
    assert g(B=0, L=-1) == ST["WL_EDIMS"]
    # nothing was written by any failed call; depth 0 copies the units and nothing else
    got, clean = unpack(torch, yb, base, B, n, S)
    assert clean and np.all(got == np.float32(SENT))
    assert f(L=0) == 0
    got, clean = unpack(torch, yb, base, B, n, S)
    assert clean and np.array_equal(ibits(got), ibits(us)) and W.last_kernel() == "copy"


def test_reserved_workspace_is_enough(gpu, W, oracle):
    """nothing is allocated once wl_workspace_bytes_full(dtype, 1, {nunits * unit_stride}, L) bytes are held"""
    import torch
    lib = W._lib.load()
    n, B, S = 8192, 6, 8196
    h, st = W.transforms._context(gpu)
    need = lib.wl_workspace_bytes_full(0, 1, (C.c_int64 * 1)(B * S), 13)
    assert lib.wl_ctx_reserve(h, need) == 0
    held = W.workspace_held()
    for wt in (filt(W, "db4"), LS.scheme(W, "cdf97"), filt(W, "db6")):
        for tree in (13, random_tree(W, n, 8, 1)):
            check(W, torch, gpu, oracle, wt, n, B, np.float32, tree, 9, S=S)
            assert W.workspace_held() == held
