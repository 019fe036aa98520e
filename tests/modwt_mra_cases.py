"""Shared inputs of the modwt_mra tests (test_modwt_mra_host.py, test_gpu_modwt_mra.py, test_gpu_modwt_mra_fused.py).

The units are modwt_batch_cases.units and the coefficients modwt_batch_cases.forward (the oracle's modwt of each unit).  The reference
multiresolution analysis is the definition itself: column c of unit u is oracle.imodwt of that unit's coefficient matrix with every
column but c set to +0.  It is computed once per (filter, n, B, dtype, L) and shared: callers must not modify what they get.

SHAPES lists every (n, B, L) the GPU tests run, by the property it is there for (see shapes()).

RULES: the status codes of wl_modwt_mra_batch in the documented order -- (status, [breaker, ...]) as in modwt_batch_cases.
"""
import numpy as np

import modwt_batch_cases as MC

FILTERS, ORTHOGONAL, DTYPES, IDS, LDS_MAX = MC.FILTERS, MC.ORTHOGONAL, MC.DTYPES, MC.IDS, MC.LDS_MAX
maxlevels, units, forward, rows = MC.maxlevels, MC.units, MC.forward, MC.rows


def shapes(dtype):
    cap = LDS_MAX[dtype]
    above = cap + 16 // np.dtype(dtype).itemsize               # one 16-byte vector above the cap
    return {
        # the tap reach 2^(j-1) (F-1) exceeds n several times over for the long filters
        "wrap": [(n, 5, L) for n in (2, 3, 8, 12) for L in sorted({1, maxlevels(n)})],
        # several planes per workgroup, a remainder, and a last workgroup whose planes start at different levels; one unit
        "packing": [(n, B, maxlevels(n)) for n in (64, 100) for B in (37, 1)],
        # a workgroup per plane, then the last LDS size and the first per-level size
        "boundary": [(cap, 3, 3), (above, 3, 3)],
        "long": [(1 << 16, 2, 5)],
        # the graph test's shape, and B = 5 for groups of two
        "groups": [(1024, 5, 4), (cap + 64, 5, 2)],
    }


DEEP = (3, 5, 7)                   # n = 3 with ncols = 8: strides up to 64, many times n (coefficients: random, no modwt has that many levels)
UNALIGNED = [(129, 3), (1000, 3)]  # with ldw = n + 1, ldo = n + 3 and unit strides ld * ncols + 5


_REF = {}


def mra_of(oracle, q, co):
    """(ncols, n) coefficients of one unit, row j = column j -> (ncols, n): row c = imodwt of the matrix with every other column +0"""
    ncols, n = co.shape
    out = np.empty_like(co)
    for c in range(ncols):
        z = np.zeros((n, ncols), dtype=co.dtype)
        z[:, c] = co[c]
        out[c] = oracle.imodwt(z, q)
    return out


def reference(oracle, W, fname, n, B, dtype, L):
    """(B, L + 1, n): [u, c] is column c of the multiresolution analysis of unit u"""
    key = (fname, n, B, np.dtype(dtype).name, L)
    if key not in _REF:
        q = W.wavelet(getattr(W.WT, fname)).qmf
        co = forward(oracle, W, fname, n, B, dtype, L)
        ref = np.stack([mra_of(oracle, q, co[u]) for u in range(B)])
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def deep_coefficients(dtype):
    """(B, ncols, n) random coefficients for DEEP"""
    n, B, L = DEEP
    return np.random.default_rng(77).standard_normal((B, L + 1, n)).astype(dtype)


# ---- status codes ---------------------------------------------------------------------------------------------------------------
ARG, DTYPE, FILTER, EDIMS, ALIAS, EL = MC.ARG, MC.DTYPE, MC.FILTER, MC.EDIMS, MC.ALIAS, MC.EL
# a valid call: two units of 64 samples, three columns, db2 (P and Q are two distinct buffers of 16384 elements that the runner supplies)
BASE = dict(ctx="CTX", dtype=0, out="P", ldo=64, out_unit_stride=192, xw="Q", ldw=64, xw_unit_stride=192, n=64, ncols=3, nunits=2, qmf="QMF",
            flen=4)
RULES = [
    (ARG, [dict(ctx=None), dict(out=None), dict(xw=None), dict(qmf=None)]),
    (DTYPE, [dict(dtype=7), dict(dtype=-1)]),
    (FILTER, [dict(flen=0), dict(flen=65)]),
    (EDIMS, [dict(n=0), dict(nunits=0), dict(ldo=63), dict(ldw=63), dict(out_unit_stride=191), dict(xw_unit_stride=191),
             dict(nunits=1 << 40, out_unit_stride=1 << 40, xw_unit_stride=1 << 40), dict(ldo=1 << 62, out_unit_stride=1 << 62),
             dict(ldw=1 << 62, xw_unit_stride=1 << 62)]),
    (ALIAS, [dict(out="Q"), dict(out="Q+32")]),
    (EL, [dict(ncols=64, out_unit_stride=4096, xw_unit_stride=4096), dict(ncols=0)]),     # (ncols = 0 alone: no extent rule sees a matrix without columns)
]
