"""Complex-valued dwt / idwt / wpt on the device (wl_*_complex): re(y) = transform(re(x)), im(y) = transform(im(x)).

Expected values come from the existing REAL entry points applied to the two components and are compared as integer bit patterns
(exact equality); one case per parametrisation is also compared with the CPU oracle on the two components, bit-exact as the
parity tests are (-0.0 == +0.0 accepted there).  Inputs are seeded normal values with exact zeros and negative zeros planted.
Every buffer handed to the ABI sits between guard bands of a sentinel, and the padding between units is sentinel too: all of it
is compared bit for bit after the call."""
import ctypes as C

import numpy as np
import pytest

import lifting_schemes as LS

pytestmark = pytest.mark.gpu

GUARD = 8                      # complex elements of guard band on either side (keeps the base 16-byte aligned)
CDT = {np.float32: np.complex64, np.float64: np.complex128}
IDT = {np.float32: np.int32, np.float64: np.int64}
CODE = {np.float32: 0, np.float64: 1}
SENT = complex(-12345.678, 9876.5)
FILTERS = ("haar", "db2", "db4", "sym5", "db8")


@pytest.fixture(autouse=True)
def _complex_arrays_on(W):
    """the Python mirror takes complex tensors only after W.set_complex_arrays(True) (off by default: the package's earlier
    behaviour); the C entry points need no switch"""
    with W.complex_arrays():
        yield


def bits(a, rdt):
    return np.ascontiguousarray(a).view(rdt).view(IDT[rdt])


def units(nunits, N, rdt, seed):
    """(nunits, N) complex: seeded normal values, exact zeros and negative zeros planted in both components"""
    r = np.random.default_rng(seed)
    a = (r.standard_normal((nunits, N)) + 1j * r.standard_normal((nunits, N))).astype(CDT[rdt])
    for u in range(nunits):
        a[u, (3 * u) % N] = complex(0.0, 0.0)
        a[u, (3 * u + 1) % N] = complex(-0.0, 1.5)
        a[u, (5 * u + N // 2) % N] = complex(-2.5, -0.0)
    return a


def ctx(W, t):
    from wavelets_jl_amd import transforms as TR
    return TR._context(t.device)


def padded(torch, gpu, us, S, rdt, offset=0):
    """device buffer [guard + offset | unit 0 .. | padding .. | guard] of sentinels with the units in place; returns (buffer, first
    element index of unit 0)"""
    nunits, N = us.shape
    base = GUARD + offset
    buf = np.full(base + nunits * S + GUARD, SENT, dtype=CDT[rdt])
    for u in range(nunits):
        buf[base + u * S: base + u * S + N] = us[u]
    return torch.from_numpy(buf).to(gpu), base


def unpack(torch, buf, base, nunits, N, S, rdt):
    """(units (nunits, N), True when every guard / padding element still holds the sentinel's bits)"""
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    mask = np.ones(h.shape, dtype=bool)
    out = np.empty((nunits, N), dtype=h.dtype)
    for u in range(nunits):
        out[u] = h[base + u * S: base + u * S + N]
        mask[base + u * S: base + u * S + N] = False
    clean = np.array_equal(bits(h[mask], rdt), bits(np.full(int(mask.sum()), SENT, dtype=h.dtype), rdt))
    return out, clean


def ptr(buf, base):
    return C.c_void_p(buf.data_ptr() + base * buf.element_size())


def dims3(shape):
    return (C.c_int64 * 3)(*(list(shape) + [1] * (3 - len(shape))))


def call_complex(W, torch, gpu, wt, us, shape, L, fw, S, rdt, inplace=False):
    """wl_dwt_filter_complex / wl_dwt_lifting_complex on padded buffers; returns the units of y"""
    nunits, N = us.shape
    xb, base = padded(torch, gpu, us, S, rdt)
    yb = xb if inplace else padded(torch, gpu, np.full_like(us, SENT), S, rdt)[0]
    h, st = ctx(W, xb)
    lib = W._lib.load()
    if isinstance(wt, W.OrthoFilter):
        q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
        rc = lib.wl_dwt_filter_complex(h, CODE[rdt], ptr(yb, base), ptr(xb, base), len(shape), dims3(shape), nunits, S,
                                       q.ctypes.data_as(C.POINTER(C.c_double)), len(q), L, 1 if fw else 0, st)
    else:
        iu, nc, sh, cf = wt.flatten()
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        rc = lib.wl_dwt_lifting_complex(h, CODE[rdt], ptr(yb, base), ptr(xb, base), len(shape), dims3(shape), nunits, S, len(iu), ip(iu),
                                        ip(nc), ip(sh), cf.ctypes.data_as(C.POINTER(C.c_double)), wt.norm1, wt.norm2, L, 1 if fw else 0, st)
    assert rc == 0, W._lib.STATUS.get(rc, rc)
    got, clean = unpack(torch, yb, base, nunits, N, S, rdt)
    assert clean, "guard band or padding between units of y was written"
    if not inplace:
        xs, xclean = unpack(torch, xb, base, nunits, N, S, rdt)
        assert xclean and np.array_equal(bits(xs, rdt), bits(us, rdt)), "x was modified"
    return got


def real_transform(W, torch, wt, comp, shape, L, fw):
    """the existing real entry point on one component (flat column-major, N values) -> flat column-major result"""
    x = W.to_device(np.ascontiguousarray(comp).reshape(shape, order="F"))
    y = (W.dwt if fw else W.idwt)(x, wt, L)
    torch.cuda.synchronize()
    return W.to_host(y).reshape(-1, order="F")


def expect_bits(W, torch, wt, us, shape, L, fw, rdt):
    e = np.empty(us.shape, dtype=us.dtype)
    for u in range(us.shape[0]):
        e[u].real = real_transform(W, torch, wt, us[u].real, shape, L, fw)
        e[u].imag = real_transform(W, torch, wt, us[u].imag, shape, L, fw)
    return e


# ---- split / merge alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rdt", [np.float32, np.float64], ids=["c64", "c128"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 1023, 1024, 1025, 2050])
def test_split_merge(gpu, W, rdt, n):
    """planes == real / imag, merge(split(z)) == z, nothing outside the units and planes written; aligned bases (vector path) and a
    base one element off (element path), one and three units, three unit strides"""
    import torch
    lib = W._lib.load()
    E = 16 // np.dtype(rdt).itemsize
    for nunits in (1, 3):
        for S in (n, n + 1, n + 3):
            for off in (0, 1):
                us = units(nunits, n, rdt, 100 * n + 10 * nunits + off)
                zb, base = padded(torch, gpu, us, S, rdt, offset=off)
                ps = (n + E - 1) // E * E + (3 if off else 0)               # planes of their own stride; off: odd stride, odd base
                pbase = 2 * GUARD + off
                sent_r = np.float64(SENT.real).astype(rdt)
                planes = torch.from_numpy(np.full(pbase + 2 * nunits * ps + 2 * GUARD, sent_r, dtype=rdt)).to(gpu)
                h, st = ctx(W, zb)
                rc = lib.wl_complex_split(h, CODE[rdt], ptr(planes, pbase), ps, ptr(zb, base), n, nunits, S, st)
                assert rc == 0
                torch.cuda.synchronize()
                ph = planes.cpu().numpy()
                pmask = np.ones(ph.shape, dtype=bool)
                for u in range(nunits):
                    for c, comp in enumerate((us[u].real, us[u].imag)):
                        lo = pbase + (2 * u + c) * ps
                        assert np.array_equal(bits(ph[lo:lo + n], rdt), bits(comp, rdt)), (n, nunits, S, off, u, c)
                        pmask[lo:lo + n] = False
                assert np.array_equal(bits(ph[pmask], rdt), bits(np.full(int(pmask.sum()), sent_r, dtype=rdt), rdt)), (n, nunits, S, off)
                ob, _ = padded(torch, gpu, np.full_like(us, SENT), S, rdt, offset=off)
                rc = lib.wl_complex_merge(h, CODE[rdt], ptr(ob, base), ptr(planes, pbase), ps, n, nunits, S, st)
                assert rc == 0
                got, clean = unpack(torch, ob, base, nunits, n, S, rdt)
                assert clean, (n, nunits, S, off)
                assert np.array_equal(bits(got, rdt), bits(us, rdt)), (n, nunits, S, off)
                _, zclean = unpack(torch, zb, base, nunits, n, S, rdt)
                assert zclean


def test_split_merge_host_mirror(gpu, W):
    import torch
    for rdt in (np.float32, np.float64):
        a = units(1, 6 * 10, rdt, 7)[0].reshape((6, 10), order="F")
        z = W.to_device(a)
        p = W.complex_split(z)
        assert tuple(p.shape) == (6, 10, 2) and W.is_julia_layout(p)
        ph = W.to_host(p)
        assert np.array_equal(bits(ph[..., 0], rdt), bits(a.real, rdt)) and np.array_equal(bits(ph[..., 1], rdt), bits(a.imag, rdt))
        back = W.complex_merge(p)
        assert back.dtype == z.dtype and np.array_equal(bits(W.to_host(back), rdt), bits(a, rdt))
    with pytest.raises(TypeError):
        W.complex_split(torch.zeros(4, device=gpu))


# ---- filter dwt / idwt ---------------------------------------------------------------------------------------------------------------
FILTER_SHAPES = [((2,), 1), ((6,), 1), ((40,), 3), ((2050,), 1), ((4096,), 12),
                 ((4, 6), 1), ((8, 8), 3), ((64, 64), 6), ((130, 66), 1),
                 ((4, 2, 6), 1), ((16, 16, 16), 4), ((32, 16, 8), 3)]


@pytest.mark.parametrize("rdt", [np.float32, np.float64], ids=["c64", "c128"])
@pytest.mark.parametrize("shape,L", FILTER_SHAPES, ids=["x".join(map(str, s)) + "_L%d" % l for s, l in FILTER_SHAPES])
def test_filter_dwt_idwt(gpu, W, oracle, rdt, shape, L):
    import torch
    N = int(np.prod(shape))
    for k, name in enumerate(FILTERS):
        wt = W.wavelet(getattr(W.WT, name))
        for nunits, S in ((1, N), (3, N + 1)):
            us = units(nunits, N, rdt, 1000 * k + N + nunits)
            for fw in (True, False):
                got = call_complex(W, torch, gpu, wt, us, shape, L, fw, S, rdt)
                kern = W.last_kernel()
                assert kern not in ("none", "copy") and "cplx" not in kern, kern      # the inner transform's kernel is what is reported
                want = expect_bits(W, torch, wt, us, shape, L, fw, rdt)
                assert np.array_equal(bits(got, rdt), bits(want, rdt)), (name, nunits, fw)
        if k == 2:                                                   # db4, the last unit of the batch of three, against the CPU oracle
            for comp, g in ((us[2].real, got[2].real), (us[2].imag, got[2].imag)):
                e = oracle.dwt_filter(np.ascontiguousarray(comp).reshape(shape, order="F"), wt.qmf, L, fw=False)
                assert np.array_equal(g.reshape(shape, order="F"), e)


# ---- lifting ---------------------------------------------------------------------------------------------------------------------------
LIFT_SHAPES = [(2,), (40,), (4096,), (8, 8), (64, 64), (8, 8, 8), (32, 32, 32)]


@pytest.mark.parametrize("rdt", [np.float32, np.float64], ids=["c64", "c128"])
@pytest.mark.parametrize("shape", LIFT_SHAPES, ids=["x".join(map(str, s)) for s in LIFT_SHAPES])
def test_lifting_dwt_idwt(gpu, W, oracle, rdt, shape):
    import torch
    N = int(np.prod(shape))
    L = W.maxtransformlevels(shape[0])
    names = ["cdf97", "haar", "db2"] + (["nc3"] if shape in ((40,), (64, 64), (8, 8, 8)) else [])   # nc3: a user scheme, the fallback tier
    for k, name in enumerate(names):
        sch = LS.scheme(W, name)
        for nunits, S in ((1, N), (3, N + 1)):
            us = units(nunits, N, rdt, 2000 * k + N + nunits)
            for fw in (True, False):
                want = expect_bits(W, torch, sch, us, shape, L, fw, rdt)
                for inplace in (False, True):
                    got = call_complex(W, torch, gpu, sch, us, shape, L, fw, S, rdt, inplace=inplace)
                    assert np.array_equal(bits(got, rdt), bits(want, rdt)), (name, nunits, fw, inplace)
        if k == 0:                                                   # cdf9/7, inverse, last unit, against the CPU oracle
            for comp, g in ((us[2].real, got[2].real), (us[2].imag, got[2].imag)):
                e = oracle.dwt_lifting(np.ascontiguousarray(comp).reshape(shape, order="F"), sch, L, fw=False)
                assert np.array_equal(g.reshape(shape, order="F"), e)


# ---- wavelet packets --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rdt", [np.float32, np.float64], ids=["c64", "c128"])
@pytest.mark.parametrize("n", [64, 4096])
def test_wpt_iwpt(gpu, W, oracle, rdt, n):
    import torch
    Lmax = W.maxtransformlevels(n)
    z = units(1, n, rdt, n)[0]
    zd = W.to_device(z)
    for wt in (W.wavelet(W.WT.db4), W.wavelet(W.WT.cdf97, W.WT.Lifting)):
        for tree in (1, 3, Lmax, W.maketree(n, 3, "dwt"), W.maketree(n, Lmax, "dwt")):
            for f in (W.wpt, W.iwpt):
                y = f(zd, wt, tree)
                assert y.dtype == zd.dtype and tuple(y.shape) == (n,)
                yr, yi = f(W.to_device(z.real.copy()), wt, tree), f(W.to_device(z.imag.copy()), wt, tree)
                torch.cuda.synchronize()
                yh = W.to_host(y)
                assert np.array_equal(bits(yh.real.copy(), rdt), bits(W.to_host(yr), rdt)), (type(wt).__name__, tree if isinstance(tree, int) else "dwt")
                assert np.array_equal(bits(yh.imag.copy(), rdt), bits(W.to_host(yi), rdt)), (type(wt).__name__, tree if isinstance(tree, int) else "dwt")
        # the partially split tree against the CPU oracle
        tree = W.maketree(n, 3, "dwt")
        yh = W.to_host(W.wpt(zd, wt, tree))
        orc = oracle.wpt_filter if isinstance(wt, W.OrthoFilter) else oracle.wpt_lifting
        arg = wt.qmf if isinstance(wt, W.OrthoFilter) else wt
        assert np.array_equal(yh.real, orc(z.real.copy(), arg, tree)) and np.array_equal(yh.imag, orc(z.imag.copy(), arg, tree))
    # in-place forms: wpt_(y, x, filter, L) and wpt_(y, scheme, L)
    y = W.similar(zd)
    W.wpt_(y, zd, W.wavelet(W.WT.db4), 3)
    assert np.array_equal(bits(W.to_host(y), rdt), bits(W.to_host(W.wpt(zd, W.wavelet(W.WT.db4), 3)), rdt))
    sch = W.wavelet(W.WT.cdf97, W.WT.Lifting)
    y.copy_(zd)
    W.iwpt_(y, sch, 3)
    assert np.array_equal(bits(W.to_host(y), rdt), bits(W.to_host(W.iwpt(zd, sch, 3)), rdt))


# ---- round trip ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rdt,bound", [(np.float32, 1e-5), (np.float64, 1e-12)], ids=["c64", "c128"])
def test_round_trip(gpu, W, rdt, bound):
    """idwt(dwt(z)) against z within the bound of the real round-trip tests (relative L2: 1e-5 Float32, 1e-12 Float64)"""
    import torch
    for shape in ((4096,), (64, 64), (16, 16, 16)):
        z = units(1, int(np.prod(shape)), rdt, 5)[0].reshape(shape, order="F")
        zd = W.to_device(z)
        for wt in (W.wavelet(W.WT.db4), W.wavelet(W.WT.cdf97, W.WT.Lifting)):
            back = W.idwt(W.dwt(zd, wt), wt)
            rel = float(torch.linalg.vector_norm((back - zd).to(torch.complex128))) / float(torch.linalg.vector_norm(zd.to(torch.complex128)))
            assert rel < bound, (shape, type(wt).__name__, rel)


# ---- status codes ----------------------------------------------------------------------------------------------------------------------
def test_status_codes(gpu, W):
    """one call per code, in the documented order; none of them writes y"""
    import torch
    lib, ST = W._lib.load(), {v: k for k, v in W._lib.STATUS.items()}
    rdt = np.float32
    us = units(2, 64, rdt, 1)
    xb, base = padded(torch, gpu, us, 65, rdt)
    yb, _ = padded(torch, gpu, np.full_like(us, SENT), 65, rdt)
    h, st = ctx(W, xb)
    q = np.ascontiguousarray(W.wavelet(W.WT.db2).qmf, dtype=np.float64)
    qp = q.ctypes.data_as(C.POINTER(C.c_double))
    sch = W.wavelet(W.WT.cdf97, W.WT.Lifting)
    iu, nc, sh, cf = sch.flatten()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))

    def filt(y=None, x=None, dtype=0, ndims=2, dims=(8, 8, 1), nunits=2, S=65, flen=4, L=2, q_=qp):
        return lib.wl_dwt_filter_complex(h, dtype, ptr(yb, base) if y is None else y, ptr(xb, base) if x is None else x, ndims,
                                         (C.c_int64 * 3)(*dims), nunits, S, q_, flen, L, 1, st)

    def lift(y=None, x=None, dtype=0, ndims=2, dims=(8, 8, 1), nunits=2, S=65, L=2, nsteps=len(iu)):
        return lib.wl_dwt_lifting_complex(h, dtype, ptr(yb, base) if y is None else y, ptr(xb, base) if x is None else x, ndims,
                                          (C.c_int64 * 3)(*dims), nunits, S, nsteps, ip(iu), ip(nc), ip(sh),
                                          cf.ctypes.data_as(C.POINTER(C.c_double)), sch.norm1, sch.norm2, L, 1, st)

    null = C.c_void_p(None)
    assert filt(y=null) == ST["WL_EINVAL_ARG"] and filt(x=null) == ST["WL_EINVAL_ARG"] and filt(q_=None) == ST["WL_EINVAL_ARG"]
    assert lift(y=null) == ST["WL_EINVAL_ARG"]
    assert filt(dtype=2) == ST["WL_EINVAL_DTYPE"] and lift(dtype=-1) == ST["WL_EINVAL_DTYPE"]
    assert filt(flen=1) == ST["WL_EINVAL_FILTER"] and filt(flen=65) == ST["WL_EINVAL_FILTER"]      # what the real call rejects
    assert lift(nsteps=17) == ST["WL_EINVAL_SCHEME"]
    assert lift(dims=(8, 4, 1), S=65) == ST["WL_EINVAL_CUBE"]                                      # non-square lifting image
    assert filt(dims=(8, 4, 1), L=1) == 0                                                          # (filters take any box)
    assert filt(nunits=0) == ST["WL_EDIMS"] and lift(nunits=0) == ST["WL_EDIMS"]
    assert filt(S=63) == ST["WL_EDIMS"] and lift(S=63) == ST["WL_EDIMS"]                           # unit_stride < prod(dims)
    assert filt(ndims=4) == ST["WL_EDIMS"] and filt(dims=(8, 0, 1)) == ST["WL_EDIMS"]
    assert filt(L=-1) == ST["WL_EINVAL_L"] and lift(L=-1) == ST["WL_EINVAL_L"]
    assert filt(L=4) == ST["WL_EINVAL_SIZE"] and lift(L=4) == ST["WL_EINVAL_SIZE"]                 # missing 2^L factor
    assert filt(y=ptr(xb, base)) == ST["WL_EALIAS"]                                                # y == x, filters only
    # the order: an earlier rule wins over every later one
    assert filt(dtype=2, flen=1, nunits=0, L=-1) == ST["WL_EINVAL_DTYPE"]
    assert filt(flen=1, nunits=0, L=-1) == ST["WL_EINVAL_FILTER"]
    assert filt(nunits=0, L=-1, y=ptr(xb, base)) == ST["WL_EDIMS"]
    assert filt(L=-1, y=ptr(xb, base)) == ST["WL_EINVAL_L"] and filt(L=4, y=ptr(xb, base)) == ST["WL_EINVAL_SIZE"]
    assert lift(dims=(8, 4, 1), nunits=0, L=-1) == ST["WL_EINVAL_CUBE"] and lift(nsteps=17, dims=(8, 4, 1)) == ST["WL_EINVAL_SCHEME"]
    # wpt: the L range of the full tree, an invalid tree, y == x
    one = lambda y, x, tree, nt, L: lib.wl_wpt_filter_complex(h, 0, y, x, 64, qp, 4, tree, nt, L, 1, st)
    bad = np.zeros(63, dtype=np.uint8); bad[1] = 1                                                 # a child without its parent
    assert one(ptr(yb, base), ptr(xb, base), None, 0, 7) == ST["WL_EINVAL_L"]
    assert one(ptr(yb, base), ptr(xb, base), bad.ctypes.data_as(C.POINTER(C.c_uint8)), 63, 0) == ST["WL_EINVAL_TREE"]
    assert one(ptr(xb, base), ptr(xb, base), None, 0, 1) == ST["WL_EALIAS"]
    # L = 0 copies the units and nothing else
    fresh, _ = padded(torch, gpu, np.full_like(us, SENT), 65, rdt)
    assert lib.wl_dwt_filter_complex(h, 0, ptr(fresh, base), ptr(xb, base), 2, (C.c_int64 * 3)(8, 8, 1), 2, 65, qp, 4, 0, 1, st) == 0
    got, clean = unpack(torch, fresh, base, 2, 64, 65, rdt)
    assert clean and np.array_equal(bits(got, rdt), bits(us, rdt))


def test_failed_calls_write_nothing(gpu, W):
    import torch
    lib = W._lib.load()
    rdt = np.float32
    us = units(2, 64, rdt, 2)
    xb, base = padded(torch, gpu, us, 65, rdt)
    yb, _ = padded(torch, gpu, np.full_like(us, SENT), 65, rdt)
    h, st = ctx(W, xb)
    q = np.ascontiguousarray(W.wavelet(W.WT.db2).qmf, dtype=np.float64)
    for kw in (dict(nunits=0), dict(S=63), dict(L=-1), dict(L=4), dict(flen=1), dict(dtype=2)):
        a = dict(dtype=0, nunits=2, S=65, flen=4, L=2)
        a.update(kw)
        rc = lib.wl_dwt_filter_complex(h, a["dtype"], ptr(yb, base), ptr(xb, base), 2, (C.c_int64 * 3)(8, 8, 1), a["nunits"], a["S"],
                                       q.ctypes.data_as(C.POINTER(C.c_double)), a["flen"], a["L"], 1, st)
        assert rc < 0
    got, clean = unpack(torch, yb, base, 2, 64, 65, rdt)
    assert clean and np.array_equal(bits(got, rdt), bits(np.full_like(us, SENT), rdt))


# ---- groups -----------------------------------------------------------------------------------------------------------------------------
def test_groups_change_no_bit(gpu, W):
    """8 units of 64 x 64 under a cap of 1 MiB run in more than one group (one group of 8 would hold about 1.4 MiB); same bits"""
    import torch
    rdt = np.float32
    us = units(8, 64 * 64, rdt, 3)
    for wt in (W.wavelet(W.WT.db4), W.wavelet(W.WT.cdf97, W.WT.Lifting)):
        one = call_complex(W, torch, gpu, wt, us, (64, 64), 3, True, 64 * 64 + 2, rdt)
        with W.options(WL_TI_WS_CAP_MB=1):
            many = call_complex(W, torch, gpu, wt, us, (64, 64), 3, True, 64 * 64 + 2, rdt)
        assert np.array_equal(bits(one, rdt), bits(many, rdt))
        assert np.array_equal(bits(one, rdt), bits(expect_bits(W, torch, wt, us, (64, 64), 3, True, rdt), rdt))


# ---- the fused library ----------------------------------------------------------------------------------------------------------------
def test_fused_library(gpu, W):
    """W.set_arithmetic("fused"): the complex transform equals the fused real transform of the components bit for bit.

    In the fused build the real entry points do not agree bit for bit among themselves: the single-image call and the batched call
    take different kernels, which contract different products (measured on 64 x 64 db4, L = 4, six planes: the two differ in the last
    bit of some coefficients; the figure is printed below).  "The fused real transform of the components" is therefore the call the
    complex entry point is defined to make -- wl_dwt_filter_batch on the 2 * nunits component planes -- and that comparison is exact;
    against the single-image transform the fused mode's own tolerance applies (relative L2 <= 1e-6 sqrt(L))."""
    import torch
    rdt = np.float32
    us = units(3, 64 * 64, rdt, 4)
    wt = W.wavelet(W.WT.db4)
    planes = np.stack([c for u in us for c in (u.real.reshape((64, 64), order="F"), u.imag.reshape((64, 64), order="F"))], axis=-1)
    with W.arithmetic("fused"):
        for fw in (True, False):
            got = call_complex(W, torch, gpu, wt, us, (64, 64), 4, fw, 64 * 64 + 1, rdt)
            yb = (W.dwt_batch if fw else W.idwt_batch)(W.to_device(planes), wt, 4)
            torch.cuda.synchronize()
            ybh = W.to_host(yb)
            want = np.empty_like(us)
            for u in range(3):
                want[u].real = ybh[..., 2 * u].reshape(-1, order="F")
                want[u].imag = ybh[..., 2 * u + 1].reshape(-1, order="F")
            assert np.array_equal(bits(got, rdt), bits(want, rdt)), fw
            single = expect_bits(W, torch, wt, us, (64, 64), 4, fw, rdt)
            print("fused, fw=%d: %d of %d values of the real batch transform differ from the real single-image transform"
                  % (fw, int((bits(want, rdt) != bits(single, rdt)).sum()), want.size * 2))
            assert np.linalg.norm(got - single) / np.linalg.norm(single) <= 1e-6 * 2.0
    assert W.get_arithmetic() == "exact"


# ---- hipGraph ---------------------------------------------------------------------------------------------------------------------------
def test_hipgraph_capture_and_replay(gpu, W):
    """one wl_dwt_filter_complex call (64 x 64, db4) captured on a single stream after a warm call has grown the workspace, replayed
    twice on changed input, compared with the eager result"""
    import torch
    rdt = np.float32
    wt = W.wavelet(W.WT.db4)
    inputs = [units(1, 64 * 64, rdt, s)[0].reshape((64, 64), order="F") for s in (11, 12, 13)]
    eager = [W.to_host(W.dwt(W.to_device(a), wt, 4)) for a in inputs]
    x = W.to_device(inputs[0])
    y = W.similar(x)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        W.dwt_(y, x, wt, 4)                                    # (warm call: code objects loaded, the workspace grown)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        W.dwt_(y, x, wt, 4)
    for k in (1, 2):
        x.copy_(W.to_device(inputs[k]))
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(W.to_host(y), rdt), bits(eager[k], rdt)), k
    del graph


# ---- host mirror ------------------------------------------------------------------------------------------------------------------------
def test_complex_arrays_are_opt_in(gpu, W):
    """off: a complex tensor raises TypeError in the transforms as it did before; on: it is transformed; the block restores the setting"""
    import torch
    wt = W.wavelet(W.WT.db2)
    z = W.to_device(units(1, 32, np.float64, 1)[0])
    with W.complex_arrays(False):
        assert not W.get_complex_arrays()
        for call in (lambda: W.dwt(z, wt, 1), lambda: W.idwt(z, wt, 1), lambda: W.wpt(z, wt, 1), lambda: W.dwt_(W.similar(z), z, wt, 1),
                     lambda: W.dwt_batch(z.reshape(4, 4, 2), wt, 1)):
            with pytest.raises(TypeError, match="set_complex_arrays"):
                call()
    assert W.get_complex_arrays()
    assert W.dwt(z, wt, 1).dtype == torch.complex128


@pytest.mark.parametrize("rdt", [np.float32, np.float64], ids=["c64", "c128"])
def test_host_mirror(gpu, W, rdt):
    import torch
    cdt = torch.complex64 if rdt == np.float32 else torch.complex128
    filt, sch = W.wavelet(W.WT.db4), W.wavelet(W.WT.cdf97, W.WT.Lifting)

    def same(y, x, f):
        assert y.dtype == cdt and tuple(y.shape) == tuple(x.shape)
        want = torch.complex(f(x.real.contiguous()), f(x.imag.contiguous()))
        assert torch.equal(torch.view_as_real(y.contiguous()).view(torch.int32 if rdt == np.float32 else torch.int64),
                           torch.view_as_real(want.contiguous()).view(torch.int32 if rdt == np.float32 else torch.int64))

    v = W.to_device(units(1, 256, rdt, 1)[0])
    m = W.to_device(units(1, 32 * 32, rdt, 2)[0].reshape((32, 32), order="F"))
    for wt in (filt, sch):
        for x in (v, m):
            for L in (None, 2):
                y = W.dwt(x, wt, L)
                same(y, x, lambda r: W.dwt(W.julia_layout(r.reshape(x.shape)), wt, L))
                same(W.idwt(y, wt, L), y, lambda r: W.idwt(W.julia_layout(r.reshape(y.shape)), wt, L))
        same(W.wpt(v, wt, 3), v, lambda r: W.wpt(r, wt, 3))
        same(W.iwpt(v, wt), v, lambda r: W.iwpt(r, wt))
    # in-place forms
    y = W.similar(m)
    W.dwt_(y, m, filt, 2)
    same(y, m, lambda r: W.dwt(W.julia_layout(r.reshape(m.shape)), filt, 2))
    y.copy_(m)
    W.idwt_(y, sch, 2)
    same(y, m, lambda r: W.idwt(W.julia_layout(r.reshape(m.shape)), sch, 2))
    with pytest.raises(W.ArgumentError, match="in array is out array"):
        W.dwt_(m, m, filt, 1)
    with pytest.raises(W.ArgumentError, match="power of 2"):
        W.dwt(v, filt, 9)
    with pytest.raises(W.ArgumentError, match="square/cube"):
        W.dwt(W.to_device(units(1, 128, rdt, 3)[0].reshape((8, 16), order="F")), sch, 1)
    with pytest.raises(TypeError):
        W.dwt_(W.similar(m, torch.float32 if rdt == np.float32 else torch.float64), m, filt, 1)      # mixed element types
    # a batch of images and a batch of volumes
    for shape, wts in (((16, 16, 3), (filt, sch)), ((8, 8, 8, 2), (filt, sch)), ((8, 4, 3), (filt,))):
        b = W.to_device(units(1, int(np.prod(shape)), rdt, 4)[0].reshape(shape, order="F"))
        for wt in wts:
            yb = W.dwt_batch(b, wt, 1)
            assert yb.dtype == cdt and tuple(yb.shape) == shape
            re = W.dwt_batch(W.julia_layout(b.real), wt, 1)
            im = W.dwt_batch(W.julia_layout(b.imag), wt, 1)
            torch.cuda.synchronize()
            yh = W.to_host(yb)
            assert np.array_equal(bits(yh.real.copy(), rdt), bits(W.to_host(re), rdt))
            assert np.array_equal(bits(yh.imag.copy(), rdt), bits(W.to_host(im), rdt))
            back = W.to_host(W.idwt_batch(yb, wt, 1))
            assert np.allclose(back, W.to_host(b), rtol=0, atol=1e-4 if rdt == np.float32 else 1e-11)
    # a complex tensor that is not dense column-major gets the treatment of _prep_in: a column-major copy
    rowmajor = torch.from_numpy(np.ascontiguousarray(W.to_host(m))).to(gpu)
    assert not W.is_julia_layout(rowmajor)
    assert torch.equal(W.dwt(rowmajor, filt, 2), W.dwt(m, filt, 2))
    # everything else refuses complex tensors by name
    for name, call in (("denoise", lambda: W.denoise(v, filt)), ("threshold", lambda: W.threshold(v, W.HardTH(), 1.0)),
                       ("modwt", lambda: W.modwt(v, filt, 2)), ("bestbasistree", lambda: W.bestbasistree(v, filt)),
                       ("noisest", lambda: W.noisest(v, filt)), ("dwtc", lambda: W.dwtc(m, filt))):
        with pytest.raises(TypeError, match=name):
            call()
