"""Case tables and shared oracle references of the denoise_ti_batch tests (test_denoise_ti_batch_host.py,
test_gpu_denoise_ti_batch.py).  The units are those of tests/denoise_batch_cases.py (DB.unit); every reference is
oracle.denoise(unit, fwd, inv, L, kind, t_unit(n), TI=True, nspin=..., sigma=...), unit by unit, computed once per key and shared
(callers must not modify what they get).
"""
import numpy as np

import denoise_batch_cases as DB

# (n, ndim, B, nspin): the smallest shapes at which each rule of the shift / threshold / accumulate kernels can go wrong
FILTER_CASES = [
    (64, 1, 5, (8,)),          # baseline signal batch
    (64, 1, 3, (70,)),         # more spins than samples: the shift wraps
    (512, 1, 2, (300,)),       # more than 256 spins per unit: the accumulate's shift table is walked in chunks
    (1024, 1, 3, (3,)),        # a spin count that is no power of two
    (8, 2, 5, (2, 3)),         # asymmetric nspin, dimension order
    (64, 2, 3, (3, 2)),        # asymmetric nspin, dimension order
    (16, 2, 3, (8, 8)),        # the default spins on an image
    (8, 3, 3, (2, 1, 3)),      # asymmetric nspin on a cube
    (16, 3, 2, (2, 2, 2)),     # cube batch
]
# (wavelet, threshold kind, L; None = the default min(maxtransformlevels, 6)) at every case
FILTER_COMBOS = [("sym5", "hard", None), ("db2", "soft", None), ("haar", "semisoft", 1), ("db8", "stein", 0), ("haar", "hard", None),
                 ("db2", "hard", 1)]
# lifting: DB.lifting_combos(n, ndim) at the default L
LIFTING_CASES = [(64, 1, 5, (8,)), (16, 2, 3, (2, 3)), (8, 3, 3, (2, 1, 3))]
DTYPES = [np.float32, np.float64]

_TI = {}


def level(oracle, n, L):
    return DB.default_L(oracle, n) if L is None else L


def ref_ti(oracle, W, n, ndim, dtype, i, wname, L, kind, nspin, lifting=False, sigma=None):
    """the oracle's translation-invariant denoise of unit i (L: a number); sigma = None: the unit's own estimate"""
    key = (n, ndim, np.dtype(dtype).name, i, wname, L, kind, tuple(nspin), lifting, sigma)
    if key not in _TI:
        fwd, inv = DB.transforms(oracle, W, wname, lifting)
        s = DB.ref_sigma(oracle, W, n, ndim, dtype, i, wname, lifting) if sigma is None else sigma
        r = oracle.denoise(DB.unit(i, n, ndim, dtype), fwd, inv, L, kind, DB.t_unit(n), TI=True, nspin=tuple(nspin), sigma=s)
        r.setflags(write=False)
        _TI[key] = r
    return _TI[key]


def check_fixture(oracle, W, n, ndim, dtype, B, nspin, wname, L, kind, lifting=False):
    """what lets a batch tell whose sigma a unit was thresholded with, and that the spins were summed at all -- on the oracle's values"""
    tag = (n, ndim, np.dtype(dtype).name, B, tuple(nspin), wname, L, kind)
    sig = [DB.ref_sigma(oracle, W, n, ndim, dtype, i, wname, lifting) for i in range(B)]
    assert len(set(sig)) == B, tag + ("sigmas not pairwise distinct", sig)
    for i in range(B):
        own = ref_ti(oracle, W, n, ndim, dtype, i, wname, L, kind, nspin, lifting)
        other = ref_ti(oracle, W, n, ndim, dtype, i, wname, L, kind, nspin, lifting, sigma=sig[(i + 1) % B])
        assert not np.array_equal(own, other), tag + ("unit %d: the neighbour's sigma gives the same result" % i,)
        plain = DB.ref_denoise(oracle, W, n, ndim, dtype, i, wname, L, kind, lifting)
        assert not np.array_equal(own, plain), tag + ("unit %d: the plain denoise gives the same result" % i,)
