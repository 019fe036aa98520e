"""Shared by tests/test_gpu_threshold_batch.py and tests/test_threshold_batch_host.py: the units, layouts, thresholds and references
of threshold_batch_ (wl_threshold_batch / wl_threshold_biggest_batch), and the status rules of the two entry points.

A batch lives in one flat buffer: GUARD sentinel elements, then B units of n elements `stride` apart, the padding between and behind
the units filled with the sentinel, then GUARD sentinel elements.  The expected buffer is built the same way from the expected
units, so one comparison of integer bit patterns covers the units, the padding and the guard bands.

RULES_EW / RULES_BIG: the status codes in the documented order -- (status, [breaker, ...]) as in modwt_batch_cases.
"""
import numpy as np

DTYPES = (np.float32, np.float64)
IDS = ("f32", "f64")
LDS_MAX = {np.float32: 8192, np.float64: 4096}             # mad_lds_max: the longest unit whose keys fit in LDS
SENT = {np.float32: 0xFFC5A5A5, np.float64: 0xFFF85A5A5A5A5A5A}          # a NaN payload no threshold produces
GUARD = 8                                                   # elements; keeps the first unit 16-byte aligned
KINDS = ("hard", "soft", "semisoft", "stein", "pos", "neg")
EW_N, EW_B = (1, 3, 5, 256, 257, 1023, 1025), (1, 3)            # (256: the longest unit that gets a wave instead of a workgroup row)
WAVE_MAX = 256
BIG_N, BIG_B = (1, 2, 3, 63, 64, 65, 100), (1, 3, 5)
# options that force a tier of the BiggestTH batch whatever n and nunits are; the split tier with 64-element chunks
TIERS = {
    "lds": ("k_thbig_lds", {}),
    "stream": ("k_thbig_stream", {"WL_THB_LDS_MAX": 0, "WL_THB_SPLIT_N": 1 << 62}),
    "split": ("k_thbig_split", {"WL_THB_LDS_MAX": 0, "WL_THB_SPLIT_N": 1, "WL_THB_SPLIT_UNITS": 1 << 40, "WL_THB_CHUNK": 64}),
}


def ew_kernel(n, B, stride, per_unit):
    """the kernel of the element-wise call: short units of a batch take a wave each, unless the batch is one dense array with one
    threshold (then it is thresholded as a single unit)"""
    one_unit = B == 1 or (stride == n and not per_unit)
    return "k_threshold_batch_wave" if n <= WAVE_MAX and not one_unit else "k_threshold_batch"


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def strides(n):
    """dense; bases of the units >= 1 off the 16-byte grid; and a third"""
    return (n, n + 1, n + 3)


def units(n, B, dtype, seed=0):
    """(B, n): even units quantised to quarters (equal magnitudes of both signs and zeros everywhere), odd units continuous.  The
    first B rows of a larger batch with the same seed and n"""
    r = np.random.default_rng(1000 * seed + n)
    u = r.standard_normal((8, n))
    u[0::2] = np.round(u[0::2] * 4) / 4
    return np.ascontiguousarray(u[:B].astype(dtype))


def tie_units(n, dtype, seed=0):
    """(3, n): draws from {-2, -1, -0.0, +0.0, 1, 2} -- the cut lands inside a long run of equal magnitudes for most m -- twice, and
    a unit of all-equal values"""
    r = np.random.default_rng(77 + seed)
    vals = np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0])
    u = np.stack([vals[r.integers(0, 6, n)], vals[r.integers(0, 6, n)], np.full(n, -1.5)])
    return np.ascontiguousarray(u.astype(dtype))


def nonfinite_units(n, dtype):
    """(4, n): rows 0-1 hold +-Inf and subnormals (no NaN: the oracle orders them), rows 2-3 also hold NaNs of both signs"""
    assert n >= 12
    r = np.random.default_rng(5)
    tiny = np.finfo(dtype).tiny
    u = r.standard_normal((4, n)).astype(dtype)
    for k in range(4):
        idx = r.permutation(n)
        u[k, idx[:3]] = [np.inf, -np.inf, np.inf]
        u[k, idx[3:9]] = (np.array([0.25, -0.5, 0.75, -0.25, 0.5, 1e-3]) * tiny).astype(dtype)
        if k >= 2:
            u[k, idx[9:12]] = [np.nan, -np.nan, np.nan]
    return u


def split_run_unit(dtype, n=5000):
    """the unit of the split-tier case: magnitudes 1 (signs mixed) on [900, 4700) -- a run of ties that starts in the first 2048-element
    chunk, covers the second and ends in the partial third one -- larger magnitudes in front, smaller ones behind"""
    r = np.random.default_rng(9)
    u = np.empty(n)
    u[:900] = 2 + r.random(900)
    u[900:4700] = np.where(r.random(3800) < 0.5, -1.0, 1.0)
    u[4700:] = 0.5 * r.random(n - 4700)
    return u.astype(dtype)


def biggest_ref(u, m):
    """threshold!(u, BiggestTH(), m) with the tie rule of the device calls, for units without NaN: the n - m entries of smallest
    magnitude go, equal magnitudes lower index first"""
    u = np.array(u, copy=True)
    m = min(max(int(m), 0), u.size)
    order = np.argsort(np.abs(u.astype(np.float64)), kind="stable")
    u[order[:u.size - m]] = 0
    return u


def layout(us, stride, dtype):
    """the flat host buffer of the (B, n) units `us`"""
    B, n = us.shape
    buf = np.full(2 * GUARD + B * stride, SENT[dtype], dtype=ibits(np.zeros(1, dtype)).dtype).view(dtype)
    for u in range(B):
        buf[GUARD + u * stride:GUARD + u * stride + n] = us[u]
    return buf


def scalar_ms(n):
    return sorted({0, 1, n // 2, n - 1, n, n + 5})


def unit_ms(n, B):
    """one m per unit, all different where n allows: 0, n, one above n, one negative, and values inside"""
    return [0, n, n + 1, -3, n // 2][:B] if B > 1 else [n // 2]


# ---- the status rules -------------------------------------------------------------------------------------------------------
ARG, DTYPE, EDIMS = "WL_EINVAL_ARG", "WL_EINVAL_DTYPE", "WL_EDIMS"
# a valid call: three units of 64 elements 68 apart in a buffer P of 16384 elements that the runner supplies
BASE_EW = dict(ctx="CTX", dtype=0, x="P", n=64, nunits=3, unit_stride=68, th=0, t=1.0, t_dev=None, t_is_f64=1)
RULES_EW = [
    (ARG, [dict(ctx=None), dict(x=None)]),
    (DTYPE, [dict(dtype=7), dict(dtype=-1)]),
    (EDIMS, [dict(n=0), dict(nunits=0), dict(unit_stride=63), dict(nunits=1 << 40, unit_stride=1 << 40), dict(nunits=1 << 30, unit_stride=1 << 30)]),
    (ARG, [dict(th=6), dict(th=-1), dict(t=-1.0), dict(t=float("nan")), dict(th=3, t=-0.5)]),
]
BASE_BIG = dict(ctx="CTX", dtype=0, x="P", n=64, nunits=3, unit_stride=68, m=5, m_dev=None)
RULES_BIG = [
    (ARG, [dict(ctx=None), dict(x=None)]),
    (DTYPE, [dict(dtype=7), dict(dtype=-1)]),
    (EDIMS, [dict(n=0), dict(nunits=0), dict(unit_stride=63), dict(nunits=1 << 40, unit_stride=1 << 40), dict(nunits=1 << 30, unit_stride=1 << 30)]),
    (ARG, [dict(m=-1)]),
]


def rows(rules):
    """(status, arguments): each breaker with the first breaker of every later rule"""
    out = []
    for i, (status, breakers) in enumerate(rules):
        for b in breakers:
            args = {}
            for _, later in reversed(rules[i + 1:]):
                args.update(later[0])
            args.update(b)
            out.append((status, args))
    return out
