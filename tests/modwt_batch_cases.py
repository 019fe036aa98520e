"""Shared inputs of the modwt_batch tests (test_modwt_batch_host.py, test_gpu_modwt_batch.py, test_gpu_modwt_batch_fused.py).

Unit i of a panel is `default_rng(1000 * n + i).standard_normal(n)` cast to the element type: every unit is a different signal, so
a result computed from a neighbour's samples shows.  The references are the oracle's modwt / imodwt of each unit, computed once
per (n, B, dtype, filter, L) and shared: callers must not modify what they get.

SHAPES lists every (n, B, L) the GPU tests run, by the property it is there for.  LDS_MAX is the longest unit of the LDS tier
(2 * n * sizeof(T) <= 64 KB).

RULES_FWD / RULES_INV: the status codes of wl_modwt_batch / wl_imodwt_batch in the documented order -- (status, [breaker, ...]),
a breaker being the arguments that break that rule; the tests combine a breaker with one breaker of every later rule.
"""
import numpy as np

FILTERS = ("haar", "db2", "db4", "sym5", "coif6", "batt2")
ORTHOGONAL = ("haar", "db2", "db4", "sym5", "coif6")          # the Battle tables are not orthogonal: imodwt is only the adjoint there
DTYPES = (np.float32, np.float64)
IDS = ("f32", "f64")
LDS_MAX = {np.float32: 8192, np.float64: 4096}


def maxlevels(n):
    return int(n).bit_length() - 1


def _levels(n):
    return sorted({1, maxlevels(n)})


def shapes(dtype):
    cap = LDS_MAX[dtype]
    above = cap + 16 // np.dtype(dtype).itemsize               # one 16-byte vector above the cap
    return {
        # the tap reach 2^(j-1) (F-1) exceeds n several times over for the long filters
        "wrap": [(n, 5, L) for n in (2, 3, 8, 12) for L in _levels(n)],
        # several units per workgroup and a remainder; one unit
        "packing": [(n, B, L) for n in (64, 100) for B in (37, 1) for L in (maxlevels(n),)],
        # a workgroup per unit, then the last LDS size and the first per-level size
        "boundary": [(cap, 3, 3), (above, 3, 3)],
        "long": [(1 << 16, 2, 5)],
        # the graph test's shape, and B = 5 for groups of two
        "groups": [(1024, 5, 4), (cap + 64, 5, 2)],
    }


UNALIGNED = [(129, 3), (1000, 3)]                              # with unit_stride = n + 3, ldo = n + 1, out_unit_stride = ldo (L+1) + 5


def all_shapes(dtype):
    return [s for group in shapes(dtype).values() for s in group]


def units(n, B, dtype):
    """(B, n): unit i in row i"""
    return np.stack([np.random.default_rng(1000 * n + i).standard_normal(n).astype(dtype) for i in range(B)])


_FWD, _INV = {}, {}


def forward(oracle, W, fname, n, B, dtype, L):
    """(B, L + 1, n): [u, j] is column j of oracle.modwt(unit u)"""
    key = (fname, n, B, np.dtype(dtype).name, L)
    if key not in _FWD:
        q = W.wavelet(getattr(W.WT, fname)).qmf
        us = units(n, B, dtype)
        ref = np.stack([np.ascontiguousarray(oracle.modwt(us[u], q, L).T) for u in range(B)])
        ref.setflags(write=False)
        _FWD[key] = ref
    return _FWD[key]


def inverse(oracle, W, fname, n, B, dtype, L):
    """(B, n): oracle.imodwt of the oracle's coefficients of unit u"""
    key = (fname, n, B, np.dtype(dtype).name, L)
    if key not in _INV:
        q = W.wavelet(getattr(W.WT, fname)).qmf
        co = forward(oracle, W, fname, n, B, dtype, L)
        ref = np.stack([oracle.imodwt(np.ascontiguousarray(co[u].T), q) for u in range(B)])
        ref.setflags(write=False)
        _INV[key] = ref
    return _INV[key]


# ---- status codes ---------------------------------------------------------------------------------------------------------------
ARG, DTYPE, FILTER, EDIMS, ALIAS, SIZE, EL = ("WL_EINVAL_ARG", "WL_EINVAL_DTYPE", "WL_EINVAL_FILTER", "WL_EDIMS", "WL_EALIAS",
                                              "WL_EINVAL_SIZE", "WL_EINVAL_L")
# a valid call: two units of 64 samples, db2, L = 2 (P and Q are two distinct buffers of 16384 elements that the runner supplies; the
# units of out are 512 apart, so that a row with L = 7 still meets the extent rule)
BASE_FWD = dict(ctx="CTX", dtype=0, out="P", ldo=64, out_unit_stride=512, x="Q", n=64, nunits=2, unit_stride=64, qmf="QMF", flen=4, L=2)
RULES_FWD = [
    (ARG, [dict(ctx=None), dict(out=None), dict(x=None), dict(qmf=None)]),
    (DTYPE, [dict(dtype=7), dict(dtype=-1)]),
    (FILTER, [dict(flen=0), dict(flen=65)]),
    (EDIMS, [dict(n=0), dict(nunits=0), dict(unit_stride=63), dict(ldo=63), dict(out_unit_stride=191),
             dict(nunits=1 << 40, unit_stride=1 << 40), dict(ldo=1 << 62, out_unit_stride=1 << 62)]),
    (ALIAS, [dict(out="Q"), dict(out="Q+32")]),
    (SIZE, [dict(L=7)]),
    (EL, [dict(L=0), dict(L=-1)]),
]
BASE_INV = dict(ctx="CTX", dtype=0, x="P", unit_stride=64, xw="Q", ldw=64, xw_unit_stride=192, n=64, ncols=3, nunits=2, qmf="QMF", flen=4)
RULES_INV = [
    (ARG, [dict(ctx=None), dict(x=None), dict(xw=None), dict(qmf=None)]),
    (DTYPE, [dict(dtype=7), dict(dtype=-1)]),
    (FILTER, [dict(flen=0), dict(flen=65)]),
    (EDIMS, [dict(n=0), dict(nunits=0), dict(unit_stride=63), dict(ldw=63), dict(xw_unit_stride=191),
             dict(nunits=1 << 40, xw_unit_stride=1 << 40), dict(ldw=1 << 62, xw_unit_stride=1 << 62)]),
    (ALIAS, [dict(x="Q"), dict(x="Q+32")]),
    (EL, [dict(ncols=64, xw_unit_stride=4096), dict(ncols=0)]),      # (ncols = 0 alone: no extent rule sees a matrix without columns)
]


def rows(rules):
    """(status, arguments): each breaker with the first breaker of every later rule (the earlier rule's value stands where two rules
    need the same argument; SIZE and EL both need L, so a row keeps the first of them it meets)"""
    out = []
    for i, (status, breakers) in enumerate(rules):
        for b in breakers:
            args = {}
            for _, later in reversed(rules[i + 1:]):
                args.update(later[0])
            args.update(b)
            out.append((status, args))
    return out
