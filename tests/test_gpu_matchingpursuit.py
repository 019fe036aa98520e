"""matchingpursuit / findmaxabs on the device (wl_findmaxabs, wl_mp_select, wl_mp_residual, wl_matchingpursuit_filter).

* findmaxabs against the reference's loop: every length at which the launch plan changes, ties inside and across workgroups,
  NaN / Inf / signed zeros, an unaligned base, and the whole set again under WL_MP_MAX_BLOCKS = 1 and 3;
* the fast path against the shared case table (matchingpursuit_cases.py) in the exact library: y and r bit for bit, niter equal,
  nrm within DESIGN.md section 11's bound, sentinels around y, r and x untouched, x unchanged;
* the generic form: equal to the fast path with f / ft built from W.dwt / W.idwt, and bit for bit the numpy loop on an integer
  dictionary of the reference's own test shape;
* ft -> wl_findmaxabs -> wl_mp_select captured into a hipGraph and replayed on two inputs;
* both libraries: x - f(y) = r elementwise to niter x the one-transform tolerance of tests/test_gpu_fused.py x max|x|.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import matchingpursuit_cases as MC

pytestmark = pytest.mark.gpu

GUARD = 3                                                    # sentinel elements on either side (an odd count: the arrays are unaligned)
SENTINEL = -777.25
TORCH = {np.float32: "float32", np.float64: "float64"}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- findmaxabs --------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 257, 4097, (1 << 20) + 3)


def _patterns(n, dtype):
    """name -> vector; the last workgroup boundary of the default plan is far below n - 2 for the two long lengths"""
    nan, inf = float("nan"), float("inf")
    base = (np.random.default_rng(7 * n + 1).standard_normal(n) * 1.5).astype(dtype)
    out = {"random": base.copy()}

    def put(name, pairs, fill=None):
        v = base.copy() if fill is None else np.full(n, fill, dtype=dtype)
        for i, val in pairs:
            v[i % n] = val
        out[name] = v

    put("max_last", [(n - 1, 100.0)])
    put("max_first", [(0, -100.0)])
    put("neg_before_pos", [(n // 3, -50.0), (n - 1 - n // 4, 50.0)])
    put("all_equal", [], fill=2.5)
    put("all_equal_neg", [], fill=-2.5)
    put("two_equal_maxima", [(n // 4 + 1, 77.0), (n - 2, 77.0), (n // 2, -77.0)])
    put("zeros_with_negative_zero", [(n // 2, -0.0)], fill=0.0)
    put("nan_first", [(0, nan)])
    put("nan_elsewhere", [(n // 2, nan), (n - 1, nan)])
    put("all_nan", [], fill=nan)
    put("nan_first_inf_later", [(0, nan), (n - 1, inf)])
    put("inf", [(n // 3, -inf), (n - 1 - n // 4, inf)])
    put("inf_last", [(n - 1, inf)])
    return out


@functools.lru_cache(maxsize=None)
def _findmaxabs_set(dtype):
    """(length, name, vector, expected index by the reference's loop), computed once and shared by the three grid caps"""
    return tuple((n, name, v, MC.findmaxabs(v)) for n in LENGTHS for name, v in _patterns(n, dtype).items())


@pytest.mark.parametrize("cap", (None, 1, 3), ids=("default", "blocks1", "blocks3"))
@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_findmaxabs_is_the_references_loop(W, gpu, dtype, cap):
    import torch
    if cap is not None:
        W.set_option("WL_MP_MAX_BLOCKS", cap)
    wrong = []
    for n, name, v, want in _findmaxabs_set(dtype):
        buf = torch.full((n + 1,), SENTINEL, dtype=getattr(torch, TORCH[dtype]), device=gpu)
        hv = torch.from_numpy(v).to(gpu)
        for off in (0, 1):                                   # off = 1: a base one element past a 16-byte boundary
            d = hv if off == 0 else buf[1:]
            if off:
                d.copy_(hv)
            got = W.findmaxabs(d)
            if got != want:
                wrong.append((n, name, off, got, want))
        assert float(buf[0]) == SENTINEL
    assert not wrong, wrong[:10]
    # expectations the table must contain, whatever the random values are
    exp = {(n, name): want for n, name, _, want in _findmaxabs_set(dtype)}
    n = LENGTHS[-1]
    assert exp[(n, "all_equal")] == 0 and exp[(n, "all_nan")] == 0 and exp[(n, "nan_first")] == 0 and exp[(n, "zeros_with_negative_zero")] == 0
    assert exp[(n, "two_equal_maxima")] == n // 4 + 1 and exp[(n, "neg_before_pos")] == n // 3 and exp[(n, "inf")] == n // 3
    assert exp[(n, "max_last")] == n - 1 and exp[(n, "nan_first_inf_later")] == 0 and exp[(n, "nan_elsewhere")] not in (n // 2, n - 1)


def test_findmaxabs_launch_plan(W, gpu):
    """one launch up to 4096 elements, partials and a fold beyond"""
    import torch
    W.findmaxabs(torch.ones(4096, device=gpu))
    assert W.last_kernel() == "k_mp_absmax_fold"
    W.findmaxabs(torch.ones(4097, device=gpu))
    assert W.last_kernel() == "k_mp_absmax_part"


# ---- the fast path against the case table ---------------------------------------------------------------------------------------
def _guarded(torch, gpu, dtype, n, fill=None):
    """a tensor of n elements between GUARD sentinels; returns (whole buffer, the view)"""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=getattr(torch, TORCH[dtype]), device=gpu)
    view = buf[GUARD:GUARD + n]
    if fill is not None:
        view.copy_(torch.from_numpy(np.array(fill)).to(gpu))
    return buf, view


def _guards_intact(buf):
    h = buf.cpu().numpy()
    return bool((h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all())


def _abi_pursuit(W, torch, gpu, case, ref, dtype):
    """wl_matchingpursuit_filter on guarded y and r; returns (y, r, niter, nrm) as host values"""
    n, bases = case[0], case[1]
    ws, Ls = MC.filters(W, bases), MC.levels(W, bases, n)
    ybuf, y = _guarded(torch, gpu, dtype, n * len(ws))
    rbuf, r = _guarded(torch, gpu, dtype, n, ref["x"])
    q = np.ascontiguousarray(np.concatenate([np.asarray(w.qmf, dtype=np.float64) for w in ws]))
    fl = np.array([len(w.qmf) for w in ws], dtype=np.int32)
    la = np.array(Ls, dtype=np.int32)
    niter, nrm = C.c_int64(-1), C.c_double(-1.0)
    h, st = W.transforms._context(gpu)
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rc = W._lib.load().wl_matchingpursuit_filter(h, 0 if dtype == np.float32 else 1, C.c_void_p(y.data_ptr()), C.c_void_p(r.data_ptr()), n, len(ws),
                                                 q.ctypes.data_as(f64), fl.ctypes.data_as(i32), la.ctypes.data_as(i32), ref["tol"], ref["nmax"],
                                                 C.byref(niter), C.byref(nrm), st)
    assert rc == 0, W._lib.STATUS[rc]
    torch.cuda.synchronize()
    assert _guards_intact(ybuf) and _guards_intact(rbuf), "a sentinel around y or r was overwritten"
    return y.cpu().numpy(), r.cpu().numpy(), niter.value, nrm.value


def _check_norm(got, ref, dtype):
    assert abs(got - ref["nrm"]) <= MC.norm_bound(ref["nrm"], dtype), (got, ref["nrm"])


@pytest.mark.parametrize("case", MC.CASES, ids=MC.CASE_IDS)
@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_fast_path_is_the_reference_loop(W, oracle, gpu, dtype, case):
    import torch
    assert W.get_arithmetic() == "exact"
    ref = MC.reference(oracle, W, case, dtype)
    n, bases = case[0], case[1]
    y, r, niter, nrm = _abi_pursuit(W, torch, gpu, case, ref, dtype)
    print("niter %d (reference %d), nrm %.17g (reference %.17g)" % (niter, ref["niter"], nrm, ref["nrm"]))
    assert niter == ref["niter"]
    assert same_bits(y, ref["y"]), np.flatnonzero(bits(y) != bits(ref["y"]))[:8]
    assert same_bits(r, ref["r"]), np.flatnonzero(bits(r) != bits(ref["r"]))[:8]
    _check_norm(nrm, ref, dtype)
    assert W.last_kernel().startswith("matchingpursuit+")
    # the Python form: x between sentinels and unchanged, the residual into a guarded tensor, the same bits
    xbuf, x = _guarded(torch, gpu, dtype, n, ref["x"])
    resbuf, res = _guarded(torch, gpu, dtype, n)
    Ls = MC.levels(W, bases, n)
    y2, niter2, nrm2 = W.matchingpursuit(x, MC.filters(W, bases), ref["tol"], ref["nmax"], L=Ls, residual=res, info=True)
    assert _guards_intact(xbuf) and _guards_intact(resbuf)
    assert same_bits(x.cpu().numpy(), ref["x"]), "x was modified"
    assert niter2 == niter and nrm2 == nrm and same_bits(y2.cpu().numpy(), y) and same_bits(res.cpu().numpy(), r)


def test_fast_path_with_a_capped_grid_and_default_levels(W, oracle, gpu):
    """WL_MP_MAX_BLOCKS = 3 on a few thousand elements runs the grid-stride loops and the multi-partial folds: the same y, r and
    niter (the cap changes the order of the norm's Float64 sum only); L defaults to maxtransformlevels(n) per base"""
    import torch
    for case in ((4096, "haar+db4", "gauss", ("after", 7), 40), (4096, "dirac+db4", "tie", 1e-3, 5)):
        for dtype in MC.DTYPES:
            ref = MC.reference(oracle, W, case, dtype)
            x = torch.from_numpy(ref["x"].copy()).to(gpu)
            with W.options(WL_MP_MAX_BLOCKS=3):
                y, niter, nrm = W.matchingpursuit(x, MC.filters(W, case[1]), ref["tol"], ref["nmax"], L=MC.levels(W, case[1], 4096), info=True)
            assert niter == ref["niter"] and same_bits(y.cpu().numpy(), ref["y"])
            _check_norm(nrm, ref, dtype)
    ref = MC.reference(oracle, W, (4096, "haar+db4", "gauss", ("after", 7), 40), np.float32)
    wts = MC.filters(W, "haar+db4")
    x = torch.from_numpy(ref["x"].copy()).to(gpu)
    assert same_bits(W.matchingpursuit(x, wts, ref["tol"], 40).cpu().numpy(), ref["y"])          # L = None: 12 levels each
    one = W.matchingpursuit(x, wts[1], 1e-3, 5)                                                    # one OrthoFilter, not a sequence
    assert same_bits(one.cpu().numpy(), W.matchingpursuit(x, [wts[1]], 1e-3, 5, L=12).cpu().numpy()) and one.numel() == 4096


# ---- the generic form ---------------------------------------------------------------------------------------------------------
GENERIC_CASES = ((8, "haar+db4", "gauss", 1e-3, -1), (64, "db2+sym5+db10@L2", "gauss", 1e-3, 5), (64, "dirac+db4", "atoms", ("after", 2), 40),
                 (64, "mixedL", "tie", 1e-3, 5), (1000, "haar@L3", "gauss", 1e-3, 5), (4096, "haar+db4", "gauss", ("after", 7), 40))


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_generic_form_over_dwt_and_idwt_equals_the_fast_path(W, oracle, gpu, dtype):
    """f is the literal sum over the bases, so equality is == (the sign of a zero is not part of the contract)"""
    import torch
    assert set(GENERIC_CASES) <= set(MC.CASES)
    for case in GENERIC_CASES:
        n, bases = case[0], case[1]
        ref = MC.reference(oracle, W, case, dtype)
        ws, Ls = MC.filters(W, bases), MC.levels(W, bases, n)

        def ft(r):
            return torch.cat([W.dwt(r, w, L) for w, L in zip(ws, Ls)])

        def f(c):
            out = W.idwt(c[:n].clone(), ws[0], Ls[0])
            for k in range(1, len(ws)):
                out = out + W.idwt(c[k * n:(k + 1) * n].clone(), ws[k], Ls[k])
            return out

        x = torch.from_numpy(ref["x"].copy()).to(gpu)
        res = torch.empty_like(x)
        y, niter, nrm = W.matchingpursuit(x, f, ft, ref["tol"], ref["nmax"], residual=res, info=True)
        assert niter == ref["niter"], case
        assert np.array_equal(y.cpu().numpy(), ref["y"]) and np.array_equal(res.cpu().numpy(), ref["r"]), case
        _check_norm(nrm, ref, dtype)
        assert same_bits(x.cpu().numpy(), ref["x"])
        rf = torch.empty_like(x)
        yf = W.matchingpursuit(x, ws, ref["tol"], ref["nmax"], L=Ls, residual=rf)
        assert torch.equal(yf, y) and torch.equal(rf, res), case


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_generic_form_on_an_integer_dictionary(W, gpu, dtype):
    """the reference's own test shape (test/threshold.jl:39-45) with M = 16, N = 64: entries in -2..2 and an integer y0 keep every
    product and sum an integer below 2^24, exact in both element types, so the numpy loop is the expected result bit for bit"""
    import torch
    M, N, nmax, tol = 16, 64, 3, 0.1
    rng = np.random.default_rng(5)
    A = rng.integers(-2, 3, size=(M, N))
    y0 = np.zeros(N, dtype=np.int64)
    y0[rng.choice(N, 5, replace=False)] = rng.integers(-2, 3, size=5)
    x = A @ y0
    # the loop in exact integers, and the bound that makes the floating-point loop exact
    r, y, it, peak = x.copy(), np.zeros(N, dtype=np.int64), 0, int(np.abs(x).max())
    while math.sqrt(float((r * r).sum())) > tol and it < nmax:
        ftr = A.T @ r
        i = MC.findmaxabs(ftr.astype(np.float64))
        aphi = A[:, i] * ftr[i]
        r = r - aphi
        y[i] += ftr[i]
        it += 1
        peak = max(peak, int(np.abs(ftr).max()), int(np.abs(aphi).max()), int(np.abs(r).max()), int(np.abs(y).max()))
    assert it == nmax and peak < (1 << 24) and M * 4 * peak < (1 << 53), (it, peak)
    Ad = torch.from_numpy(A.astype(dtype)).to(gpu)
    At = Ad.t().contiguous()
    xd = torch.from_numpy(x.astype(dtype)).to(gpu)
    res = torch.empty_like(xd)
    yd, niter, nrm = W.matchingpursuit(xd, lambda c: torch.mv(Ad, c), lambda v: torch.mv(At, v), tol, nmax, residual=res, info=True)
    assert niter == it
    assert same_bits(yd.cpu().numpy(), y.astype(dtype)) and same_bits(res.cpu().numpy(), r.astype(dtype))
    assert same_bits(xd.cpu().numpy(), x.astype(dtype))
    want = math.sqrt(float((r * r).sum()))
    assert abs(nrm - want) <= MC.norm_bound(want, dtype)
    assert yd.numel() == N and res.numel() == M


# ---- capture --------------------------------------------------------------------------------------------------------------------
def test_select_chain_is_capturable(W, oracle, gpu):
    """ft -> wl_findmaxabs -> wl_mp_select captured into a hipGraph (partials and fold: 8192 coefficients) and replayed"""
    import torch
    from wavelets_jl_amd import pursuit as P
    n, L, wt = 8192, 13, W.wavelet(W.WT.db4)
    inputs = [np.random.default_rng(40 + k).standard_normal(n).astype(np.float32) for k in range(3)]
    x = torch.from_numpy(inputs[0]).to(gpu)
    ftr, y, spat = torch.empty_like(x), torch.zeros_like(x), torch.zeros_like(x)
    idx = torch.zeros(1, dtype=torch.int64, device=gpu)
    s = torch.cuda.Stream()

    def chain():
        W.dwt_oop_(ftr, x, wt, L)
        P._findmaxabs_dev(ftr, idx)
        P._select_dev(spat, y, ftr, idx)

    with torch.cuda.stream(s):
        W.reserve_workspace(x, L, full=True)
        chain()                                              # (first call: code objects loaded, the workspace of stream s held)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        chain()
    for k in (1, 2):
        x.copy_(torch.from_numpy(inputs[k]).to(gpu))
        y.zero_()
        spat.zero_()
        graph.replay()
        torch.cuda.synchronize()
        e = oracle.dwt_filter(inputs[k], wt.qmf, L)
        i = MC.findmaxabs(e)
        want = np.zeros(n, dtype=np.float32)
        want[i] = e[i]
        assert int(idx.item()) == i and same_bits(y.cpu().numpy(), want) and same_bits(spat.cpu().numpy(), want), k
    del graph


# ---- both libraries: x - f(y) = r -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("exact", "fused"))
@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_residual_identity_in_both_libraries(W, oracle, gpu, dtype, mode):
    """No equality with the oracle is claimed for the fused library (an arg-max may flip).  For every case x - f(y) = r holds
    elementwise, f built from W.idwt: within niter x (the tolerance tests/test_gpu_fused.py applies to one transform of that
    depth: 1e-5 elementwise for Float32, 1e-13 sqrt(L) for Float64) x max|x|."""
    import torch
    worst = 0.0
    with W.arithmetic(mode):
        for case in MC.CASES:
            n, bases = case[0], case[1]
            ref = MC.reference(oracle, W, case, dtype)
            ws, Ls = MC.filters(W, bases), MC.levels(W, bases, n)
            x = torch.from_numpy(ref["x"].copy()).to(gpu)
            res = torch.empty_like(x)
            y, niter, nrm = W.matchingpursuit(x, ws, ref["tol"], ref["nmax"], L=Ls, residual=res, info=True)
            assert 0 <= niter <= ref["cap"] and y.numel() == n * len(ws)
            fy = np.zeros(n, dtype=np.float64)
            for k, (w, L) in enumerate(zip(ws, Ls)):
                fy += W.idwt(y[k * n:(k + 1) * n].clone(), w, L).cpu().numpy().astype(np.float64)
            one = 1e-5 if dtype == np.float32 else 1e-13 * math.sqrt(max(max(Ls), 1))
            bound = max(niter, 1) * one * float(np.abs(ref["x"]).max())
            dev = float(np.abs(ref["x"].astype(np.float64) - fy - res.cpu().numpy().astype(np.float64)).max())
            worst = max(worst, dev / bound)
            assert dev <= bound, (case, niter, dev, bound)
            rn = float(np.linalg.norm(res.cpu().numpy().astype(np.float64)))
            assert abs(nrm - rn) <= 4 * MC.norm_bound(rn, dtype) + 1e-300, (case, nrm, rn)
    print("largest |x - f(y) - r| / bound = %.3g (%s, %s)" % (worst, mode, np.dtype(dtype).name))
    assert W.get_arithmetic() == "exact"
