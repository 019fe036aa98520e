"""User-defined lifting schemes on the device (tests/lifting_schemes.py): schemes of no known shape -- 3-coefficient steps,
shifts beyond +-1 up to the int32 limits, 0 / 1 / 5 / 16 steps -- and the table schemes with one field changed, through every
entry point, against the oracle with identical bit patterns.  None of them may reach a shape-specialised kernel.

Where they go (wl_lift.hip lifting_lines_fast, wl_api.hip wl_lifting_box): 1-D lines of <= 2048 samples and batches of >= 32
lines of <= 16384 (Float32) / 8192 (Float64) samples take the LDS tail k_tail_lift; longer lines, squares and cubes the generic
one-thread-per-element kernels."""
import numpy as np
import pytest

import lifting_schemes as LS
from conftest import rng_array

pytestmark = pytest.mark.gpu

CUSTOM = sorted(LS.CUSTOM)
NEAR = sorted(LS.NEAR_MISSES)
LARGE = sorted(LS.LARGE_SHIFTS)
UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def dev(W, a):
    return W.to_device(a)


def host(W, t):
    import torch
    torch.cuda.synchronize()
    return W.to_host(t)


def same_bits(y, e):
    return y.dtype == e.dtype and y.shape == e.shape and np.array_equal(y, e) and np.array_equal(y.view(UINT[y.dtype]), e.view(UINT[e.dtype]))


def _not_specialised(W, ctx):
    k = W.last_kernel()
    assert not any(k == s or k.startswith(s + "+") or k.startswith(s + "_") for s in LS.SPECIALISED_KERNELS), (ctx, k)
    return k


def _depths(x, W):
    Lmax = W.maxtransformlevels(x)
    return sorted({1, max(1, Lmax // 2), Lmax} - {0}) if Lmax else []


def _dwt_all_ways(W, oracle, sch, x, L, kernel, ctx):
    """forward and inverse, out of place and in place, against the oracle bit for bit; `kernel` is the tier that must run
    (a prefix of W.last_kernel())"""
    ye = oracle.dwt_lifting(x, sch, L)
    y = host(W, W.dwt(dev(W, x), sch, L))
    k = _not_specialised(W, ctx + ("fwd",))
    assert k.startswith(kernel), (ctx, "fwd", k)
    assert same_bits(y, ye), (ctx, "fwd", int((y != ye).sum()))
    t = dev(W, x)
    W.dwt_(t, sch, L)
    assert same_bits(host(W, t), ye), (ctx, "fwd in place")
    xe = oracle.dwt_lifting(ye, sch, L, fw=False)
    xr = host(W, W.idwt(dev(W, ye), sch, L))
    k = _not_specialised(W, ctx + ("inv",))
    assert k.startswith(kernel), (ctx, "inv", k)
    assert same_bits(xr, xe), (ctx, "inv", int((xr != xe).sum()))
    t = dev(W, ye)
    W.idwt_(t, sch, L)
    assert same_bits(host(W, t), xe), (ctx, "inv in place")
    return ye


# ---- twins: the shape-specialised kernel families with coefficients they were not written around -------------------------
# (shape, dtype, L, options, forward kernel, inverse kernel): what W.last_kernel() must contain (None: any specialised kernel)
TWIN_TIERS = [
    ((1 << 16,), np.float32, 16, {}, "k_lift1d_fwd3", None),
    ((1 << 16,), np.float64, 2, {}, "k_lift1d_stream", "k_lift1d_stream"),
    ((2100,), np.float32, 1, {}, "k_lift1d_gtile", "k_lift1d_gtile"),
    ((2048,), np.float32, 11, {}, "k_tail_lift_reg", "k_tail_lift_reg_inv"),
    ((256, 256), np.float32, 2, {}, "k_lift2d_tile", "k_lift2d_tile"),
    ((128, 128), np.float32, 1, {}, "k_lift2d_tile", "k_tail_lift2d_lds"),
    ((512, 512), np.float32, 1, {"WL_LIFT_TILE": 0}, "k_lift2d_fwd", "k_lift2d_inv"),
    ((512, 512), np.float64, 1, {"WL_LIFT_TILE": 0, "WL_NO_LIFT2D_FUSED": 1}, "k_lift_axis_stream", "k_lift_axis_stream"),
    ((250, 250), np.float32, 1, {}, "k_lift2d_gtile", "k_lift2d_gtile"),
    ((128, 128, 128), np.float32, 2, {}, "k_lift_short_lines", None),
    ((10, 10, 10), np.float64, 1, {}, "k_lift_any", "k_lift_any"),
]


@pytest.mark.parametrize("name", sorted(LS.TWINS))
def test_twins_on_every_specialised_family(gpu, W, oracle, name):
    """a twin runs on the kernels of its shape (cdf9/7: IDs 0 / 1, db2: 2 / 3, haar: 4 / 5) and gives the oracle's bits there"""
    sch = LS.scheme(W, name)
    assert LS.shape_id(sch) in (0, 2, 4) and LS.shape_id(sch, fw=False) == LS.shape_id(sch) + 1
    seen = set()
    for shape, dtype, L, opts, kf, ki in TWIN_TIERS:
        x = rng_array(shape, dtype, sum(shape) + len(name))
        ye = oracle.dwt_lifting(x, sch, L)
        xe = oracle.dwt_lifting(ye, sch, L, fw=False)
        with W.options(**opts):
            y = host(W, W.dwt(dev(W, x), sch, L))
            k1 = W.last_kernel()
            xr = host(W, W.idwt(dev(W, ye), sch, L))
            k2 = W.last_kernel()
        assert kf in k1 and (ki is None or ki in k2), (name, shape, L, k1, k2)
        assert any(k2.startswith(s) for s in LS.SPECIALISED_KERNELS), (name, shape, L, k2)
        assert same_bits(y, ye), (name, shape, L, k1, int((y != ye).sum()))
        assert same_bits(xr, xe), (name, shape, L, k2, int((xr != xe).sum()))
        seen |= {k1, k2}
    print(name, sorted(seen))


# ---- reversed twins: a forward pass with an inverse shape (and the other way round) -----------------------------------------
# (shape, dtype, L, options, entry point, prefix W.last_kernel() must have, substring it must not have)
REVERSED_TIERS = [
    # one level, not streamable (2100 % 8 != 0), above the 2048-sample tail: k_lift1d_gtile exists for its own direction only
    ((2100,), np.float32, 1, {}, "dwt", "k_generic_lift", "k_lift1d_gtile"),
    ((2100, 3), np.float32, 1, {}, "dwtc", "k_generic_lift", "k_lift1d_gtile"),
    # the all-shapes families keep them
    ((1 << 16,), np.float64, 2, {}, "dwt", "k_lift1d_stream", None),
    ((512, 512), np.float64, 1, {"WL_LIFT_TILE": 0, "WL_NO_LIFT2D_FUSED": 1}, "dwt", "k_lift_axis_stream", None),
    # direction-bound and guarded: the 2-D any-size tile, the any-axis pass
    ((250, 250), np.float32, 1, {}, "dwt", "k_generic_lift", "k_lift2d_gtile"),
    ((10, 10, 10), np.float64, 1, {}, "dwt", "", "k_lift_any"),
]


@pytest.mark.parametrize("tier", REVERSED_TIERS, ids=lambda t: "%s-%s-%s" % ("x".join(map(str, t[0])), np.dtype(t[1]).name, t[4]))
@pytest.mark.parametrize("name", sorted(LS.REVERSED_TWINS))
def test_reversed_twins_stay_off_the_direction_bound_kernels(gpu, W, oracle, name, tier):
    """forward and inverse, out of place and in place, the oracle's bits; a kernel family instantiated for the shapes of its own
    direction only must not take a scheme whose steps have the other direction's shape (it would run another shape's steps)"""
    shape, dtype, L, opts, entry, prefix, banned = tier
    sch = LS.scheme(W, name)
    assert LS.shape_id(sch) in (1, 3, 5) and LS.shape_id(sch, fw=False) == LS.shape_id(sch) - 1
    x = rng_array(shape, dtype, sum(shape) + len(name))
    cols = entry == "dwtc"
    ye = oracle.dwtc_lifting(x, sch, L) if cols else oracle.dwt_lifting(x, sch, L)
    xe = oracle.dwtc_lifting(ye, sch, L, fw=False) if cols else oracle.dwt_lifting(ye, sch, L, fw=False)
    fwd, inv = (W.dwtc, W.idwtc) if cols else (W.dwt, W.idwt)
    with W.options(**opts):
        y = host(W, fwd(dev(W, x), sch, L))
        k1 = W.last_kernel()
        xr = host(W, inv(dev(W, ye), sch, L))
        k2 = W.last_kernel()
        if cols:
            yi, xi = dev(W, np.zeros_like(x)), dev(W, np.zeros_like(x))
            W.dwtc_(yi, dev(W, x), sch, L)
            W.idwtc_(xi, dev(W, ye), sch, L)
        else:
            yi, xi = dev(W, x), dev(W, ye)
            W.dwt_(yi, sch, L)
            W.idwt_(xi, sch, L)
        yi, xi = host(W, yi), host(W, xi)
    print(name, shape, np.dtype(dtype).name, k1, k2, int((y != ye).sum()), int((xr != xe).sum()))
    for k in (k1, k2):
        assert k.startswith(prefix) and (banned is None or banned not in k), (name, shape, k1, k2)
    assert same_bits(y, ye), (name, shape, "fwd", k1, int((y != ye).sum()))
    assert same_bits(xr, xe), (name, shape, "inv", k2, int((xr != xe).sum()))
    assert same_bits(yi, ye), (name, shape, "fwd in place")
    assert same_bits(xi, xe), (name, shape, "inv in place")


# ---- 1-D lines: the LDS tail (<= 2048 samples) and the generic kernels ------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", CUSTOM)
def test_custom_scheme_lines(gpu, W, oracle, name, dtype):
    sch = LS.scheme(W, name)
    # tiny lines at full depth: nc + |shift| > half, every element is a boundary element and operand indices wrap many times
    for n in (2, 4, 6, 8, 12):
        x = rng_array((n,), dtype, n + 3)
        _dwt_all_ways(W, oracle, sch, x, W.maxtransformlevels(n), "k_tail_lift", (name, n))
    for n, kernel in ((2048, "k_tail_lift"), (8192, "k_generic_lift")):
        x = rng_array((n,), dtype, n + len(name))
        for L in _depths(x, W):
            _dwt_all_ways(W, oracle, sch, x, L, kernel, (name, n, L))


@pytest.mark.parametrize("name", NEAR)
def test_near_miss_scheme_lines(gpu, W, oracle, name):
    """one field away from a known shape: match_shape must not accept it (a specialised kernel would apply the known shape's
    step types / counts / shifts to these coefficients)"""
    sch = LS.scheme(W, name)
    assert LS.shape_id(sch) == -1 and LS.shape_id(sch, fw=False) == -1
    for n, dtype, kernel in ((1024, np.float32, "k_tail_lift"), (4096, np.float64, "k_generic_lift"), (8, np.float32, "k_tail_lift")):
        x = rng_array((n,), dtype, n + 1)
        for L in _depths(x, W):
            _dwt_all_ways(W, oracle, sch, x, L, kernel, (name, n, L))
    x = rng_array((64, 64), np.float32, 64)
    for L in (1, 6):
        _dwt_all_ways(W, oracle, sch, x, L, "k_generic_lift", (name, "64x64", L))


# ---- batched columns: the batched tail (>= 32 lines) and the generic kernels ----------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_custom_scheme_columns(gpu, W, oracle, dtype):
    cap = 16384 if dtype == np.float32 else 8192
    for name in CUSTOM:
        sch = LS.scheme(W, name)
        for shape, kernel in (((1024, 32), "k_tail_lift"), ((cap, 32), "k_tail_lift"), ((2 * cap, 32), "k_generic_lift"), ((64, 40), "k_tail_lift")):
            if shape[0] == cap and name not in ("sixteen", "mix", "nc3"):
                continue
            xb = rng_array(shape, dtype, shape[0] % 997 + len(name))
            for L in _depths(rng_array((shape[0],), dtype, 0), W):
                ye = oracle.dwtc_lifting(xb, sch, L)
                y = host(W, W.dwtc(dev(W, xb), sch, L))
                k = _not_specialised(W, (name, shape, L))
                assert k.startswith(kernel), (name, shape, L, k)
                assert same_bits(y, ye), (name, shape, L, "fwd")
                yd = dev(W, np.zeros_like(xb))
                W.dwtc_(yd, dev(W, xb), sch, L)
                assert same_bits(host(W, yd), ye), (name, shape, L, "fwd into y")
                xe = oracle.dwtc_lifting(ye, sch, L, fw=False)
                xr = host(W, W.idwtc(dev(W, ye), sch, L))
                assert W.last_kernel().startswith(kernel), (name, shape, L, W.last_kernel())
                assert same_bits(xr, xe), (name, shape, L, "inv")


# ---- squares and cubes: the generic kernels --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_custom_scheme_2d_3d(gpu, W, oracle, dtype):
    for name in CUSTOM:
        sch = LS.scheme(W, name)
        for shape in ((128, 128), (4, 4), (16, 16, 16), (2, 2, 2)):
            x = rng_array(shape, dtype, sum(shape) + len(name))
            for L in _depths(x, W):
                _dwt_all_ways(W, oracle, sch, x, L, "k_generic_lift", (name, shape, L))


# ---- wavelet packets and translation-invariant denoising ------------------------------------------------------------------
def test_custom_scheme_wpt(gpu, W, oracle):
    n = 1024
    rs = np.random.default_rng(31)
    part = np.zeros(n - 1, dtype=np.uint8)
    part[0] = 1
    for i in range(1, len(part)):
        part[i] = 1 if (part[(i + 1) // 2 - 1] and rs.random() < 0.6) else 0
    for dtype in (np.float32, np.float64):
        x = rng_array((n,), dtype, 17)
        for name in CUSTOM + NEAR[::6]:
            sch = LS.scheme(W, name)
            for tree in (W.maketree(n, 10, "full"), W.maketree(n, 3, "full"), part):
                ye = oracle.wpt_lifting(x, sch, tree)
                y = host(W, W.wpt(dev(W, x), sch, tree))
                _not_specialised(W, (name, "wpt"))
                assert same_bits(y, ye), (name, dtype, "wpt", int(np.asarray(tree).sum()))
                xe = oracle.wpt_lifting(ye, sch, tree, fw=False)
                xr = host(W, W.iwpt(dev(W, ye), sch, tree))
                _not_specialised(W, (name, "iwpt"))
                assert same_bits(xr, xe), (name, dtype, "iwpt", int(np.asarray(tree).sum()))
            t = dev(W, x)
            W.wpt_(t, sch, 4)
            assert same_bits(host(W, t), oracle.wpt_lifting(x, sch, W.maketree(n, 4, "full"))), (name, dtype, "wpt in place")


def _oracle_denoise(oracle, x, sch, L, dnt, nspin):
    fwd = lambda a, l: oracle.dwt_lifting(a, sch, l)
    inv = lambda a, l: oracle.dwt_lifting(a, sch, l, fw=False)
    return oracle.denoise(x, fwd, inv, L, type(dnt.th).__name__[:-2].lower(), dnt.t, TI=True, nspin=nspin)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_custom_scheme_denoise_ti(gpu, W, oracle, dtype):
    r = np.random.default_rng(8)
    v = (np.sin(np.linspace(0, 20, 1024)) + 0.1 * r.standard_normal(1024)).astype(dtype)
    a = (np.outer(np.sin(np.linspace(0, 6, 64)), np.cos(np.linspace(0, 4, 64))) + 0.1 * r.standard_normal((64, 64))).astype(dtype)
    for name in ("nc3", "shift5", "wide", "zero_steps", "sixteen", "mix", "near_cdf97_shiftplus1", "near_db2_type1"):
        sch = LS.scheme(W, name)
        for x, nsp, L in ((v, (5,), 6), (a, (3, 2), 4)):
            dnt = W.VisuShrink(x.shape[0])
            e = _oracle_denoise(oracle, x, sch, L, dnt, nsp)
            y = host(W, W.denoise(W.to_device(x), sch, L=L, dnt=dnt, TI=True, nspin=nsp))
            assert W.last_kernel() == "denoise_ti_lifting", W.last_kernel()
            assert np.array_equal(y, e), (name, x.shape, nsp, L)


# ---- shifts up to the int32 limits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LARGE)
def test_large_shifts_on_tail_and_generic(gpu, W, oracle, name):
    """+-(2^20 + 3), +-(2^31 - 1) and -2^31: the tail tier and the generic tier wrap in int64 exactly as the reference's mod1"""
    sch = LS.scheme(W, name)
    for dtype in (np.float32, np.float64):
        for n, kernel in ((2, "k_tail_lift"), (12, "k_tail_lift"), (2048, "k_tail_lift"), (8192, "k_generic_lift")):
            x = rng_array((n,), dtype, n + 5)
            for L in _depths(x, W):
                _dwt_all_ways(W, oracle, sch, x, L, kernel, (name, n, L))
        xb = rng_array((256, 32), dtype, 6)
        ye = oracle.dwtc_lifting(xb, sch, 8)
        assert same_bits(host(W, W.dwtc(dev(W, xb), sch, 8)), ye) and W.last_kernel() == "k_tail_lift"
        x = rng_array((32, 32), dtype, 7)
        _dwt_all_ways(W, oracle, sch, x, 5, "k_generic_lift", (name, "32x32"))


# ---- the scheme contract ----------------------------------------------------------------------------------------------------
def _bad_schemes(W):
    WT = W.WT
    ok = WT.make_lsstep(WT.Predict, [0.25], 0)
    return {
        "nc0": W.GLS(([WT.make_lsstep(WT.Predict, [], 0)], 1.0, 1.0, "nc0")),
        "nc4": W.GLS(([ok, WT.make_lsstep(WT.Update, [0.1, 0.2, 0.3, 0.4], 0)], 1.0, 1.0, "nc4")),
        "17 steps": W.GLS(([WT.make_lsstep((WT.Predict, WT.Update)[i % 2], [0.05], 0) for i in range(17)], 1.0, 1.0, "s17")),
    }


def test_scheme_contract_refused_before_any_write(gpu, W):
    """nc = 0, nc = 4 and 17 steps: WL_EINVAL_SCHEME -> ArgumentError from every lifting entry point, the destination untouched"""
    x = rng_array((256,), np.float32, 1)
    m = rng_array((64, 64), np.float32, 2)
    for tag, sch in _bad_schemes(W).items():
        for call in (lambda t: W.dwt(t, sch, 3), lambda t: W.idwt(t, sch, 3), lambda t: W.wpt(t, sch, 3), lambda t: W.iwpt(t, sch, 3),
                     lambda t: W.denoise(t, sch, L=3), lambda t: W.denoise(t, sch, L=3, TI=True, nspin=4)):
            t = dev(W, x)
            with pytest.raises(W.ArgumentError):
                call(t)
            assert same_bits(host(W, t), x), tag
        t = dev(W, x)
        with pytest.raises(W.ArgumentError):
            W.dwt_(t, sch, 3)
        assert same_bits(host(W, t), x), (tag, "dwt_")
        t = dev(W, x)
        with pytest.raises(W.ArgumentError):
            W.idwt_(t, sch, 3)
        assert same_bits(host(W, t), x), (tag, "idwt_")
        y0 = rng_array((64, 64), np.float32, 3)
        yd, md = dev(W, y0), dev(W, m)
        with pytest.raises(W.ArgumentError):
            W.dwtc_(yd, md, sch, 2)
        assert same_bits(host(W, yd), y0) and same_bits(host(W, md), m), (tag, "dwtc_")
        with pytest.raises(W.ArgumentError):
            W.dwtc(md, sch, 2)
        with pytest.raises(W.ArgumentError):
            W.denoise(md, sch, L=2, TI=True, nspin=(2, 2))
        assert same_bits(host(W, md), m), tag


def test_shift_outside_int32_raises_before_any_launch(gpu, W, oracle):
    """a shift that does not fit the ABI's int32 is refused in Python (numpy's OverflowError in GLS.flatten), never wrapped"""
    x = rng_array((64,), np.float32, 4)
    for sh in (2 ** 31, -2 ** 31 - 1, 2 ** 40):
        sch = W.GLS(([W.WT.make_lsstep(W.WT.Predict, [0.25], sh)], 1.0, 1.0, "too wide"))
        W.dwt(dev(W, x), W.wavelet(W.WT.db2), 1)
        before = W.last_kernel()
        t = dev(W, x)
        with pytest.raises(OverflowError):
            W.dwt(t, sch, 2)
        with pytest.raises(OverflowError):
            W.dwt_(t, sch, 2)
        assert W.last_kernel() == before and same_bits(host(W, t), x), sh


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_step_scheme_is_split_and_normalise(gpu, W, oracle, dtype):
    """0 steps is a valid scheme: each level only splits and scales (s * norm1, d * norm2)"""
    sch = LS.scheme(W, "zero_steps")
    x = rng_array((16,), dtype, 5)
    y = host(W, W.dwt(dev(W, x), sch, 1))
    n1, n2 = dtype(sch.norm1), dtype(sch.norm2)
    assert same_bits(y, np.concatenate([x[0::2] * n1, x[1::2] * n2]))
    assert same_bits(y, oracle.dwt_lifting(x, sch, 1))


# ---- against Float64: the oracle and the table entries are sane ----------------------------------------------------------
@pytest.mark.parametrize("group", ["custom", "large_shifts"])
def test_float32_device_against_float64_oracle(gpu, W, oracle, group):
    """the Float32 device result against the Float64 oracle on the same inputs: relative L2 error <= 1e-5 * sqrt(L) (Float32
    rounding ~6e-8 per operation; a wrong oracle or a table entry that blows up exceeds it by orders of magnitude)"""
    for name in (CUSTOM if group == "custom" else LARGE):
        sch = LS.scheme(W, name)
        for shape in ((2048,), (8192,), (64, 64), (8, 8, 8)):
            x = rng_array(shape, np.float64, 11)
            L = W.maxtransformlevels(x)
            e = oracle.dwt_lifting(x, sch, L)
            y = host(W, W.dwt(dev(W, x.astype(np.float32)), sch, L)).astype(np.float64)
            rel = np.linalg.norm(y - e) / np.linalg.norm(e)
            assert rel <= 1e-5 * np.sqrt(L), (name, shape, L, rel)
            xr = host(W, W.idwt(dev(W, e.astype(np.float32)), sch, L)).astype(np.float64)
            assert np.linalg.norm(xr - x) / np.linalg.norm(x) <= 1e-5 * np.sqrt(L), (name, shape, L, "inv")
