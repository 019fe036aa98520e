"""threshold_batch_ on the device (wl_threshold_batch / wl_threshold_biggest_batch, W.threshold_batch_ / W.threshold_batch): every unit
of a batch thresholded with its own t or m, in place, the units a stride apart inside one buffer between sentinel guard bands.

Every comparison is one of integer bit patterns over the WHOLE buffer: the units against the CPU oracle's threshold of each unit
(oracle.threshold(unit, kind, t_u) / oracle.threshold(unit, "biggest", m=m_u)) and against the loop of the single device call
W.threshold_ over the units; the padding between the units and the guard bands against the sentinel they were filled with.
BiggestTH runs on every tier (forced through options, W.last_kernel() names it).  Units that hold NaN are compared with the single
call alone: it orders NaN above every finite magnitude and compares nothing against a NaN cut, the oracle's sort does not.
Units, layouts and references: threshold_batch_cases.
"""
import numpy as np
import pytest

import threshold_batch_cases as TC

pytestmark = pytest.mark.gpu
ibits = TC.ibits


def TH(W, kind):
    return {"hard": W.HardTH, "soft": W.SoftTH, "semisoft": W.SemiSoftTH, "stein": W.SteinTH, "pos": W.PosTH, "neg": W.NegTH,
            "biggest": W.BiggestTH}[kind]()


def device_batch(us, stride, dtype):
    """(flat device buffer, its n x B strided view): unit u in column u"""
    import torch
    B, n = us.shape
    buf = torch.from_numpy(TC.layout(us, stride, dtype)).cuda()
    return buf, torch.as_strided(buf, (n, B), (1, stride), TC.GUARD)


def same_buffer(buf, want_units, stride, dtype, what):
    import torch
    torch.cuda.synchronize()
    got, want = ibits(buf.cpu().numpy()), ibits(TC.layout(want_units, stride, dtype))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "first differing elements (buffer index)", bad[:8].tolist(), "of", got.size)


_single = {}


def single(W, unit, kind, t):
    """the single device call on one unit (host result), remembered: threshold_(unit, TH, t)"""
    import torch
    key = (unit.dtype.str, unit.tobytes(), kind, repr(t))
    if key not in _single:
        d = W.to_device(unit.copy())
        W.threshold_(d, TH(W, kind), t) if t is not None else W.threshold_(d, TH(W, kind))
        torch.cuda.synchronize()
        _single[key] = W.to_host(d).copy()
    return _single[key]


# ---- the element-wise kinds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TC.DTYPES, ids=TC.IDS)
@pytest.mark.parametrize("kind", TC.KINDS)
def test_elementwise_kinds(gpu, W, oracle, kind, dtype):
    """n in {1, 3, 5, 1023, 1025} and both sides of the wave-per-unit limit x B in {1, 3} x three strides; a scalar t as int and as
    float, and one t per unit (a 0 among them)"""
    import torch
    takes_t = kind not in ("pos", "neg")
    for n in TC.EW_N:
        for B in TC.EW_B:
            us = TC.units(n, B + 1, dtype)[1:]        # (unit 0 continuous: Stein with t = 0 divides 0 by 0 at an exact zero)
            per_unit = [0.0, 0.625, 1.25][:B]
            variants = [("int", 1, [1] * B), ("float", 0.75, [0.75] * B), ("tensor", torch.tensor(per_unit, dtype=torch.float64).cuda(), per_unit)]
            if dtype == np.float32:     # Float32 thresholds: the arithmetic stays in the element type
                variants.append(("tensor32", torch.tensor(per_unit, dtype=torch.float32).cuda(), [np.float32(v) for v in per_unit]))
            if not takes_t:
                variants = [("none", None, [None] * B)]
            for stride in TC.strides(n):
                for name, t, tu in variants:
                    want = np.stack([oracle.threshold(us[u], kind, tu[u]) for u in range(B)])
                    loop = np.stack([single(W, us[u], kind, tu[u]) for u in range(B)])
                    assert np.array_equal(ibits(loop), ibits(want)), (kind, n, B, name)
                    buf, x = device_batch(us, stride, dtype)
                    r = W.threshold_batch_(x, TH(W, kind), t) if takes_t else W.threshold_batch_(x, TH(W, kind))
                    assert r is x and W.last_kernel() == TC.ew_kernel(n, B, stride, name.startswith("tensor")), (kind, n, B, stride, name)
                    same_buffer(buf, want, stride, dtype, (kind, n, B, stride, name))


def test_unit_of_any_shape_and_the_copying_form(gpu, W, oracle):
    """a unit is everything in front of the last dimension; threshold_batch leaves its argument alone"""
    import torch
    a = np.random.default_rng(3).standard_normal((6, 5, 4, 3)).astype(np.float32)
    t = [0.5, 0.0, 1.5]
    x = W.to_device(a)
    y = W.threshold_batch(x, W.SoftTH(), torch.tensor(t, dtype=torch.float64).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(W.to_host(x), a)
    for u in range(3):
        want = oracle.threshold(np.ascontiguousarray(a[..., u].transpose(2, 1, 0).reshape(-1)), "soft", t[u])
        assert np.array_equal(ibits(np.ascontiguousarray(W.to_host(y)[..., u].transpose(2, 1, 0).reshape(-1))), ibits(want))
    with pytest.raises(W.ArgumentError, match="works in place"):
        W.threshold_batch_(W.to_device(a).permute(1, 0, 2, 3), W.HardTH(), 1.0)


# ---- BiggestTH -----------------------------------------------------------------------------------------------------------------
def biggest_check(W, oracle, us, dtype, tier, ms, stride, nan_units=(), opts=None):
    """one batch call on `tier` with m (an int, or a list of one m per unit -> a device tensor) against the oracle and the loop"""
    import torch
    B, n = us.shape
    kernel, o = TC.TIERS[tier]
    mu = [ms] * B if isinstance(ms, int) else list(ms)
    clamp = [min(max(m, 0), n) for m in mu]
    loop = np.stack([single(W, us[u], "biggest", clamp[u]) for u in range(B)])
    for u in range(B):
        if u not in nan_units:
            want = oracle.threshold(us[u], "biggest", m=clamp[u])
            assert np.array_equal(ibits(loop[u]), ibits(want)), ("single call against the oracle", n, u, clamp[u])
    buf, x = device_batch(us, stride, dtype)
    with W.options(**{**o, **(opts or {})}):
        W.threshold_batch_(x, W.BiggestTH(), ms if isinstance(ms, int) else torch.tensor(mu, dtype=torch.int64).cuda())
        assert W.last_kernel() == kernel, (tier, n, B, W.last_kernel())
    same_buffer(buf, loop, stride, dtype, (tier, n, B, stride, ms))


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=TC.IDS)
@pytest.mark.parametrize("tier", list(TC.TIERS))
def test_biggest_every_tier(gpu, W, oracle, tier, dtype):
    """n in {1, 2, 3, 63, 64, 65, 100} x B in {1, 3, 5} x three strides x m in {0, 1, n/2, n-1, n, n+5} and one m per unit
    (0, n, n + 1 and a negative one among them)"""
    for n in TC.BIG_N:
        for B in TC.BIG_B:
            us = TC.units(n, B, dtype)
            for stride in TC.strides(n):
                for m in TC.scalar_ms(n):
                    biggest_check(W, oracle, us, dtype, tier, m, stride)
                biggest_check(W, oracle, us, dtype, tier, TC.unit_ms(n, B), stride)


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=TC.IDS)
def test_lds_boundary_takes_two_kernels_by_default(gpu, W, oracle, dtype):
    """the longest unit of the LDS tier and four elements more: different kernels without any option, the same bits on every tier"""
    cap = TC.LDS_MAX[dtype]
    seen = {}
    for n in (cap, cap + 4):
        us = TC.units(n, 3, dtype)
        buf, x = device_batch(us, n + 1, dtype)
        W.threshold_batch_(x, W.BiggestTH(), n // 3)
        seen[n] = W.last_kernel()
        same_buffer(buf, np.stack([oracle.threshold(u, "biggest", m=n // 3) for u in us]), n + 1, dtype, ("default", n))
        for tier in (("lds",) if n == cap else ()) + ("stream", "split"):
            biggest_check(W, oracle, us, dtype, tier, [n // 2, 7, n - 1], n + 1)
    assert seen == {cap: "k_thbig_lds", cap + 4: "k_thbig_stream"}


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=TC.IDS)
def test_split_tier_cut_inside_a_run_of_ties_across_chunks(gpu, W, oracle, dtype):
    """5000 elements in chunks of 2048 (two full chunks and a partial one), 3800 equal magnitudes from the first chunk into the last:
    the cut is taken through the run so that the last cleared tie falls in each of the three chunks, and on both ends of the run"""
    n = 5000
    us = np.stack([TC.split_run_unit(dtype), TC.units(n, 1, dtype)[0], TC.split_run_unit(dtype)[::-1]])
    # cleared = n - m: 300 entries are smaller than the run, so n - m - 300 ties go: 0, 1, into chunk 0, chunk 1, chunk 2, all of them
    for m in (n - 300, n - 301, n - 300 - 1000, n - 300 - 1148, n - 300 - 1149, n - 300 - 2500, n - 300 - 3500, n - 300 - 3799, n - 300 - 3800, 10):
        biggest_check(W, oracle, us, dtype, "split", m, n + 1, opts={"WL_THB_CHUNK": 2048})
    biggest_check(W, oracle, us, dtype, "split", [n - 300 - 2500, 17, n - 300 - 3000], n + 3, opts={"WL_THB_CHUNK": 2048})
    biggest_check(W, oracle, us, dtype, "stream", [n - 300 - 2500, 17, n - 300 - 3000], n + 3)


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=TC.IDS)
@pytest.mark.parametrize("tier", list(TC.TIERS))
def test_ties_and_signed_zeros(gpu, W, oracle, tier, dtype):
    """units drawn from {-2, -1, -0.0, +0.0, 1, 2} and a unit of all-equal values, m across the whole range: the cleared ties are
    exactly the lowest-indexed ones, a surviving -0.0 keeps its sign bit, a cleared one becomes +0"""
    n = 100
    us = TC.tie_units(n, dtype)
    neg0 = ibits(np.array([-0.0], dtype))[0]
    kept_neg0 = 0
    for m in range(0, n + 1):
        for u in range(3):      # the loop result is what the buffer is compared with: hold it to the index-order rule first
            got = single(W, us[u], "biggest", m)
            assert np.array_equal(ibits(got), ibits(TC.biggest_ref(us[u], m))), (u, m)
            kept_neg0 += int((ibits(got) == neg0).sum())
        biggest_check(W, oracle, us, dtype, tier, m, n + 1)
    assert kept_neg0 > 0
    biggest_check(W, oracle, us, dtype, tier, [40, 70, 33], n + 3)


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=TC.IDS)
@pytest.mark.parametrize("tier", list(TC.TIERS))
def test_nonfinite_values(gpu, W, oracle, tier, dtype):
    """+-Inf and subnormals against the oracle and the single call; units that hold NaN against the single call alone"""
    n = 100
    us = TC.nonfinite_units(n, dtype)
    for m in (0, 1, 2, 3, 4, 5, 50, 90, 94, 97, 99, 100):
        biggest_check(W, oracle, us, dtype, tier, m, n + 1, nan_units=(2, 3))
    biggest_check(W, oracle, us, dtype, tier, [3, 0, 2, 96], n + 3, nan_units=(2, 3))


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=TC.IDS)
def test_groups_change_no_bit(gpu, W, oracle, dtype):
    """the split tier under a workspace cap of zero: one unit per group"""
    n = 1000
    us = TC.units(n, 5, dtype)
    for ms in (n // 10, [0, n, n + 1, -3, n // 2]):
        biggest_check(W, oracle, us, dtype, "split", ms, n + 1, opts={"WL_TI_WS_CAP_MB": 0})
        biggest_check(W, oracle, us, dtype, "split", ms, n + 1)


@pytest.mark.parametrize("tier", ("lds", "split"))
def test_hipgraph_dwt_biggest_idwt(gpu, W, tier):
    """dwt_batch -> threshold_batch_(BiggestTH, m on the device) -> idwt_batch captured into one graph after a warm call, replayed on
    two inputs and two contents of m: the bits of the eager sequence"""
    import torch
    wt = W.wavelet(W.WT.db2)
    n0, B, L = 64, 4, 3
    inputs = [np.random.default_rng(s).standard_normal((n0, n0, B)).astype(np.float32) for s in (1, 2)]
    mvals = [[400, 0, 4096, 17], [5, 4000, 1, 2048]]
    with W.options(**TC.TIERS[tier][1]):
        def run(x, m, c, out):
            W.dwt_batch(x, wt, L, y=c)
            W.threshold_batch_(c, W.BiggestTH(), m)
            W.idwt_batch(c, wt, L, y=out)

        eager = {}
        for i, a in enumerate(inputs):
            for j, mv in enumerate(mvals):
                x = W.to_device(a)
                c, out = W.similar(x), W.similar(x)
                run(x, torch.tensor(mv, dtype=torch.int64).cuda(), c, out)
                torch.cuda.synchronize()
                eager[i, j] = W.to_host(out).copy()
        assert not np.array_equal(eager[0, 0], eager[0, 1])
        x = W.to_device(inputs[0])
        c, out = W.similar(x), W.similar(x)
        m = torch.tensor(mvals[0], dtype=torch.int64).cuda()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            run(x, m, c, out)                                 # the context of stream s, its workspace grown
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            run(x, m, c, out)
        for i, j in ((1, 1), (0, 1), (1, 0), (0, 0)):
            x.copy_(W.to_device(inputs[i]))
            m.copy_(torch.tensor(mvals[j], dtype=torch.int64))
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(ibits(W.to_host(out)), ibits(eager[i, j])), (tier, i, j)
        del graph


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=TC.IDS)
def test_fused_library_same_bits(gpu, W, oracle, dtype):
    """the opt-in fused-arithmetic build: a select has nothing to contract, and Hard / Pos / Neg only compare"""
    import torch
    n, B = 100, 3
    us = TC.units(n, B, dtype)
    W.set_arithmetic("fused")
    try:
        for tier in TC.TIERS:
            kernel, o = TC.TIERS[tier]
            buf, x = device_batch(us, n + 1, dtype)
            with W.options(**o):
                W.threshold_batch_(x, W.BiggestTH(), torch.tensor([10, 50, 99], dtype=torch.int64).cuda())
                assert W.last_kernel() == kernel
            same_buffer(buf, np.stack([oracle.threshold(us[u], "biggest", m=m) for u, m in enumerate((10, 50, 99))]), n + 1, dtype, ("fused", tier))
        for kind, t in (("hard", [0.0, 0.5, 1.25]), ("pos", None), ("neg", None)):
            buf, x = device_batch(us, n + 1, dtype)
            if t is None:
                W.threshold_batch_(x, TH(W, kind))
            else:
                W.threshold_batch_(x, TH(W, kind), torch.tensor(t, dtype=torch.float64).cuda())
            want = np.stack([oracle.threshold(us[u], kind, None if t is None else t[u]) for u in range(B)])
            same_buffer(buf, want, n + 1, dtype, ("fused", kind))
    finally:
        W.set_arithmetic("exact")
