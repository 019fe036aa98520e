"""wpt2 / iwpt2 on the device against the definition (wpt2_cases.wpt2_ref: a recursion over the oracle's one-level 2-D dwt).

* every case of wpt2_cases (8 shapes x 5 filters x 2 element types x 5 trees), forward and inverse, bit for bit, under four
  WL_WPT2_TAIL_MAX settings -- the default (the tail takes nodes of up to 256 elements), 4096 (the most its LDS buffers hold), 16
  and 1 (level passes only) -- with wl_last_kernel naming the kernel each setting must end on;
* the full-tree entry point == the tree entry point with maketree2(.., "full"); the dwt-shaped tree == W.dwt, device against device;
* guard bands around x and y (with and without the workspace plane in use, on and off the 16-byte grid): x is unchanged, nothing
  outside y is written;
* NaN / Inf / signed zeros propagate as in the oracle;
* hipGraph capture and replay of the full-tree form;
* the fused-arithmetic library within 1e-6 sqrt(L) (Float32) / 1e-13 sqrt(L) (Float64) of the definition in the 2-norm.
"""
import math

import numpy as np
import pytest

import wpt2_cases as WC

pytestmark = pytest.mark.gpu

SETTINGS = (None, 4096, 16, 1)
TAIL_DEFAULT, TAIL_CAP = 256, 4096


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def effective_depth(tree, L):
    for d in range(L, 0, -1):
        if tree[WC.depth_base(d - 1):WC.depth_base(d)].any():
            return d
    return 0


def expected_kernel(shape, depth, setting, fw):
    """the kernel of the last launch: depths 0 .. P - 1 are level passes, the tail takes the rest from the first depth whose
    nodes hold at most TAIL_MAX elements"""
    if depth == 0:
        return "copy"
    tmax = TAIL_DEFAULT if setting is None else max(1, min(setting, TAIL_CAP))
    dt = 0
    while dt < depth and (shape[0] >> dt) * (shape[1] >> dt) > tmax:
        dt += 1
    tail = dt < depth
    if fw:
        return "k_wpt2_tail" if tail else "k_wpt2_level"
    return "k_wpt2_level" if dt > 0 else "k_wpt2_tail"


def apply_setting(W, setting):
    W.clear_options()
    if setting is not None:
        W.set_option("WL_WPT2_TAIL_MAX", setting)


@pytest.mark.parametrize("dtype", WC.DTYPES, ids=WC.IDS)
@pytest.mark.parametrize("shape", WC.SHAPES, ids=WC.SHAPE_IDS)
def test_every_case_is_the_recursion_bit_for_bit(W, oracle, gpu, shape, dtype):
    import torch
    assert W.get_arithmetic() == "exact"
    n0, n1, L = shape
    seen = set()
    for fname in WC.FILTERS:
        wt = W.wavelet(getattr(W.WT, fname))
        for kind in WC.TREES:
            ref = WC.reference(oracle, W, (n0, n1), L, fname, dtype, kind)
            tree = np.array(ref["tree"])
            depth = effective_depth(tree, L)
            x, ye = W.to_device(ref["x"]), W.to_device(ref["y"])
            for setting in SETTINGS:
                apply_setting(W, setting)
                y = W.wpt2(x, wt, tree)
                kf = W.last_kernel()
                xr = W.iwpt2(ye, wt, tree)
                ki = W.last_kernel()
                torch.cuda.synchronize()
                label = (shape, fname, kind, setting)
                assert np.array_equal(bits(W.to_host(y)), bits(ref["y"])), ("wpt2", label, kf)
                assert np.array_equal(bits(W.to_host(xr)), bits(ref["xr"])), ("iwpt2", label, ki)
                assert kf == expected_kernel((n0, n1), depth, setting, True), (label, kf)
                assert ki == expected_kernel((n0, n1), depth, setting, False), (label, ki)
                seen.update((kf, ki))
            assert np.array_equal(W.to_host(x), ref["x"])                # the input is only read
    assert {"k_wpt2_level", "k_wpt2_tail"} <= seen, seen


@pytest.mark.parametrize("dtype", WC.DTYPES, ids=WC.IDS)
def test_full_entry_point_and_dwt_shaped_tree(W, oracle, gpu, dtype):
    """wl_wpt2_filter_full == wl_wpt2_filter with maketree2(.., "full") at every depth 0 .. L; the dwt-shaped tree == W.dwt /
    W.idwt, device against device; wpt2_ / iwpt2_ write into the caller's y; None is maxtransformlevels"""
    import torch
    for n0, n1, L in WC.SHAPES:
        for fname in ("haar", "db4", "batt6"):
            wt = W.wavelet(getattr(W.WT, fname))
            x = W.to_device(WC.image((n0, n1), dtype, seed=3))
            for setting in SETTINGS:
                apply_setting(W, setting)
                for l in range(L + 1):
                    full = W.maketree2(n0, n1, l, "full")
                    a, b = W.wpt2(x, wt, l), W.wpt2(x, wt, full)
                    assert torch.equal(a, b), ("wpt2", n0, n1, l, fname, setting)
                    assert W.last_kernel() == expected_kernel((n0, n1), l, setting, True)
                    assert torch.equal(W.iwpt2(a, wt, l), W.iwpt2(a, wt, full)), ("iwpt2", n0, n1, l, fname, setting)
                    if l == 0:
                        assert torch.equal(a, x) and a.data_ptr() != x.data_ptr()
                dwt_tree = W.maketree2(n0, n1, L, "dwt")
                y = W.wpt2(x, wt, dwt_tree)
                assert torch.equal(y, W.dwt(x, wt, L)), ("dwt", n0, n1, L, fname, setting)
                assert torch.equal(W.iwpt2(y, wt, dwt_tree), W.idwt(y, wt, L)), ("idwt", n0, n1, L, fname, setting)
            W.clear_options()
            if L == WC.maxlevels(n0, n1):
                assert torch.equal(W.wpt2(x, wt), W.wpt2(x, wt, L))
            out = W.similar(x)
            assert W.wpt2_(out, x, wt, L) is out and torch.equal(out, W.wpt2(x, wt, L))
            back = W.similar(x)
            assert W.iwpt2_(back, out, wt, L) is back and torch.equal(back, W.iwpt2(out, wt, L))
            with pytest.raises(W.ArgumentError, match="in array is out array"):
                W.wpt2_(x, x, wt, L)
    # a root-clear tree and an empty tree are copies
    x = W.to_device(WC.image((16, 4), dtype))
    wt = W.wavelet(W.WT.db4)
    for t in (np.zeros(5, dtype=np.uint8), np.zeros(0, dtype=np.uint8), np.zeros(5, dtype=bool)):
        assert torch.equal(W.wpt2(x, wt, t), x) and W.last_kernel() == "copy"


CANARY = 1024


def _guarded(torch, gpu, dtype, n, misalign):
    """[canary | x | canary | y | canary] in one buffer; returns the buffer and the offsets of x and y"""
    td = torch.float32 if dtype == np.float32 else torch.float64
    buf = torch.full((3 * CANARY + 2 * n + 2 * misalign,), -7.25, dtype=td, device=gpu)
    ox = CANARY + misalign
    oy = ox + n + CANARY + misalign
    return buf, ox, oy


GUARD_CASES = (
    # (shape, L, filter, dtype, WL_WPT2_TAIL_MAX): level passes through the workspace plane and the tail; level passes only; tiles
    # clipped at node and image edges; a filter longer than the nodes; the tail alone
    ((256, 128), 4, "db4", np.float32, 4096),
    ((256, 128), 4, "db4", np.float32, 1),
    ((200, 120), 3, "sym5", np.float64, 16),
    ((24, 40), 3, "batt6", np.float32, 1),
    ((64, 64), 6, "db8", np.float64, None),
    ((64, 64), 6, "db8", np.float64, 4096),
)


@pytest.mark.parametrize("misalign", [0, 1])
def test_guard_bands(W, oracle, gpu, misalign):
    import torch
    for (n0, n1), L, fname, dtype, setting in GUARD_CASES:
        for kind in ("full", "rand1"):
            ref = WC.reference(oracle, W, (n0, n1), L, fname, dtype, kind)
            tree = np.array(ref["tree"])
            arg = L if kind == "full" else tree
            wt = W.wavelet(getattr(W.WT, fname))
            n = n0 * n1
            for src, want, f in ((ref["x"], ref["y"], W.wpt2_), (ref["y"], ref["xr"], W.iwpt2_)):
                buf, ox, oy = _guarded(torch, gpu, dtype, n, misalign)
                xv = buf[ox:ox + n].view(n1, n0).t()
                yv = buf[oy:oy + n].view(n1, n0).t()
                xv.copy_(W.to_device(src))
                before = buf.clone()
                apply_setting(W, setting)
                f(yv, xv, wt, arg)
                torch.cuda.synchronize()
                label = (f.__name__, n0, n1, L, fname, kind, setting, misalign)
                keep = torch.ones(buf.numel(), dtype=torch.bool, device=gpu)
                keep[oy:oy + n] = False
                assert torch.equal(buf[keep], before[keep]), label       # x and every canary are as they were
                assert np.array_equal(bits(W.to_host(yv)), bits(want)), label


@pytest.mark.parametrize("dtype", WC.DTYPES, ids=WC.IDS)
def test_nan_inf_and_signed_zeros_propagate_as_in_the_oracle(W, oracle, gpu, dtype):
    """zeros of both signs scattered over the image and filling its lower right quadrant; a NaN, or a +Inf and a -Inf far enough
    apart to stay infinite, in the upper left corner"""
    seen = {"nan": 0, "inf": 0, "-0": 0, "+0": 0}
    for n0, n1, L, special in ((8, 8, 3, "nan"), (24, 40, 3, "nan"), (64, 64, 3, "inf"), (200, 120, 3, "nan")):
        x = WC.image((n0, n1), dtype, seed=5)
        x[::3, ::5] = 0.0
        x[1::4, 2::3] = -0.0
        x[n0 // 2:, n1 // 2:] = 0.0
        x[n0 // 2 + 1::2, n1 // 2:] = -0.0
        if special == "nan":
            x[0, 0] = np.nan
        else:
            x[0, 0], x[20, 20] = np.inf, -np.inf
        for fname in ("haar", "db4"):
            wt = W.wavelet(getattr(W.WT, fname))
            q = wt.qmf
            for kind in ("full", "rand2"):
                tree = WC.make_tree(n0, n1, L, kind)
                ye = WC.wpt2_ref(oracle, x, q, tree, L, True)
                xe = WC.wpt2_ref(oracle, ye, q, tree, L, False)
                for want in (ye, xe):
                    zero = want == 0
                    seen["nan"] += int(np.isnan(want).sum())
                    seen["inf"] += int(np.isinf(want).sum())
                    seen["-0"] += int(np.signbit(want[zero]).sum())
                    seen["+0"] += int((~np.signbit(want[zero])).sum())
                for setting in SETTINGS:
                    apply_setting(W, setting)
                    for got, want in ((W.to_host(W.wpt2(W.to_device(x), wt, tree)), ye), (W.to_host(W.iwpt2(W.to_device(ye), wt, tree)), xe)):
                        label = (n0, n1, fname, kind, setting)
                        nan = np.isnan(want)
                        assert np.array_equal(np.isnan(got), nan), label
                        # everything that is not a NaN bit for bit: infinities and the signs of zeros included
                        assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), label
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("shape", ((64, 64, 6), (256, 128, 4)), ids=("64x64-L6", "256x128-L4"))
def test_hipgraph_capture_and_replay(W, gpu, shape):
    """the full-tree form captured on one stream after a warm call has grown the workspace, replayed on new data of the same shape"""
    import torch
    n0, n1, L = shape
    wt = W.wavelet(W.WT.db4)
    inputs = [WC.image((n0, n1), np.float32, seed=s) for s in (1, 2, 3)]
    for fw in (True, False):
        f, f_ = (W.wpt2, W.wpt2_) if fw else (W.iwpt2, W.iwpt2_)
        eager = [W.to_host(f(W.to_device(a), wt, L)) for a in inputs]
        x = W.to_device(inputs[0])
        y = W.similar(x)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            f_(y, x, wt, L)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            f_(y, x, wt, L)
        for k in (1, 2):
            x.copy_(W.to_device(inputs[k]))
            y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(bits(W.to_host(y)), bits(eager[k])), (shape, fw, k)
        del graph


@pytest.mark.parametrize("dtype", WC.DTYPES, ids=WC.IDS)
def test_fused_library_within_the_bounds_of_one_transform(W, oracle, gpu, dtype):
    """libwavelets_mi355x_fma.so: ||got - ref||_2 / ||ref||_2 <= 1e-6 sqrt(L) (Float32), 1e-13 sqrt(L) (Float64)"""
    rel = 1e-6 if dtype == np.float32 else 1e-13
    worst = 0.0
    with W.arithmetic("fused"):
        for n0, n1, L in WC.SHAPES:
            for fname in WC.FILTERS:
                wt = W.wavelet(getattr(W.WT, fname))
                for kind in ("full", "rand1"):
                    ref = WC.reference(oracle, W, (n0, n1), L, fname, dtype, kind)
                    tree = np.array(ref["tree"])
                    for setting in SETTINGS:
                        apply_setting(W, setting)
                        for got, want in ((W.to_host(W.wpt2(W.to_device(ref["x"]), wt, tree)), ref["y"]),
                                          (W.to_host(W.iwpt2(W.to_device(ref["y"]), wt, tree)), ref["xr"])):
                            w64 = want.astype(np.float64)
                            err = float(np.linalg.norm(got.astype(np.float64) - w64) / np.linalg.norm(w64))
                            worst = max(worst, err / (rel * math.sqrt(L)))
                            assert err <= rel * math.sqrt(L), (n0, n1, L, fname, kind, setting, err)
    print("largest error / bound = %.3g (%s)" % (worst, np.dtype(dtype).name))
    assert W.get_arithmetic() == "exact"
