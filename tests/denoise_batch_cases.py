"""Shared inputs and oracle references of the denoise_batch tests (test_denoise_batch_host.py, test_gpu_denoise_batch.py).

Unit i of side n (a signal of n samples, an n x n image, an n^3 cube) is
    sum over the axes k of sin(2 pi (k + 1) x_k)  +  a step of height 1 at x_0 > 0.5  +  0.05 (i + 1) * standard normal noise
with x_k = (0 .. n-1) / n on every axis and the noise drawn from default_rng(9000 + 17 i + n), cast to the element type: the units
of a batch differ in their noise level, so every unit has its own sigma and a result computed with a neighbour's sigma differs.

Every reference is the CPU oracle, unit by unit, computed once per case and shared (callers must not modify what they get).
"""
import functools
import math

import numpy as np

import lifting_schemes as LS

KINDS = ("hard", "soft", "semisoft", "stein")

# The filter cases of the GPU test: (n, ndim, B, element types).  32768 Float32 / 16384 Float64 samples: the detail range is longer
# than the LDS limit of the per-unit MAD (8192 / 4096), so the streaming kernel runs without an option.
FILTER_SHAPES = [(64, 1, 5, ("float32", "float64")), (1024, 1, 3, ("float32", "float64")), (32768, 1, 3, ("float32",)),
                 (16384, 1, 3, ("float64",)), (8, 2, 5, ("float32", "float64")), (64, 2, 5, ("float32", "float64")),
                 (256, 2, 3, ("float32", "float64")), (8, 3, 3, ("float32", "float64")), (32, 3, 3, ("float32", "float64"))]
# ... and what runs at every one of them: (wavelet, threshold kind, L; None = the default min(maxtransformlevels, 6)).  Every
# wavelet, every kind and every L of {0, 1, default} at every shape, not their full product (864 oracle denoises).
FILTER_COMBOS = [("sym5", "hard", None), ("db2", "soft", None), ("haar", "semisoft", None), ("db8", "stein", None),
                 ("db2", "hard", 1), ("haar", "stein", 0), ("sym5", "semisoft", 1), ("db8", "soft", 0), ("haar", "hard", None),
                 ("haar", "hard", 1)]
# The one place where the fixture cannot carry a combination: with haar the 64 coefficients of unit 0 of the 8 x 8 batch have none
# between its own hard threshold and its neighbour's, so there the hard threshold could not tell whose sigma was used (the kinds that
# shrink the survivors by t can, at every shape).  test_denoise_batch_host.py pins that this is the only such shape.
FILTER_EXCEPT = {("haar", "hard"): {(8, 2)}}
# lifting: (scheme of tests/lifting_schemes.py, threshold kind) at the default L.  With twin_cdf97 unit 2 of the 64-sample batch
# keeps the same coefficients under its neighbour's hard threshold: that pair runs at the other three shapes.
LIFTING_COMBOS = [("cdf97", "hard"), ("db2", "soft"), ("haar", "semisoft"), ("twin_cdf97", "stein"), ("twin_cdf97", "hard"), ("haar", "hard")]
LIFTING_EXCEPT = {("twin_cdf97", "hard"): {(64, 1)}}
LIFTING_SHAPES = [(64, 1, 5), (64, 2, 3), (8, 3, 3), (64, 3, 2)]


def filter_combos(n, ndim):
    return [c for c in FILTER_COMBOS if (n, ndim) not in FILTER_EXCEPT.get(c[:2], ())]


def lifting_combos(n, ndim):
    return [c for c in LIFTING_COMBOS if (n, ndim) not in LIFTING_EXCEPT.get(c, ())]


@functools.lru_cache(maxsize=None)
def unit(i, n, ndim, dtype):
    g = np.arange(n, dtype=np.float64) / n
    axes = np.meshgrid(*([g] * ndim), indexing="ij")
    clean = sum(np.sin(2 * np.pi * (k + 1) * axes[k]) for k in range(ndim)) + (axes[0] > 0.5)
    noise = np.random.default_rng(9000 + 17 * i + n).standard_normal((n,) * ndim)
    a = (clean + 0.05 * (i + 1) * noise).astype(dtype)
    a.setflags(write=False)
    return a


def units(n, ndim, dtype, B):
    return [unit(i, n, ndim, dtype) for i in range(B)]


def default_L(oracle, n):
    return min(oracle.maxtransformlevels(n), 6)


def t_unit(n):
    return math.sqrt(2 * math.log(n))          # VisuShrink(n).t


def transforms(oracle, W, wname, lifting=False):
    """(fwd(a, L), inv(a, L)) of the oracle for a wavelet name: an orthogonal filter of W.WT, or a scheme of tests/lifting_schemes.py"""
    if lifting:
        sch = LS.scheme(W, wname)
        return (lambda a, l: oracle.dwt_lifting(a, sch, l)), (lambda a, l: oracle.dwt_lifting(a, sch, l, fw=False))
    q = W.wavelet(getattr(W.WT, wname)).qmf
    return (lambda a, l: oracle.dwt_filter(a, q, l)), (lambda a, l: oracle.dwt_filter(a, q, l, fw=False))


_SIGMA = {}
_DENOISE = {}


def ref_sigma(oracle, W, n, ndim, dtype, i, wname, lifting=False):
    key = (n, ndim, np.dtype(dtype).name, i, wname, lifting)
    if key not in _SIGMA:
        fwd, _ = transforms(oracle, W, wname, lifting)
        _SIGMA[key] = oracle.noisest(unit(i, n, ndim, dtype), fwd)
    return _SIGMA[key]


def ref_denoise(oracle, W, n, ndim, dtype, i, wname, L, kind, lifting=False, sigma=None):
    """oracle.denoise of unit i with t_unit = sqrt(2 ln n); sigma = None: the unit's own estimate"""
    key = (n, ndim, np.dtype(dtype).name, i, wname, L, kind, lifting, sigma)
    if key not in _DENOISE:
        fwd, inv = transforms(oracle, W, wname, lifting)
        s = ref_sigma(oracle, W, n, ndim, dtype, i, wname, lifting) if sigma is None else sigma
        r = oracle.denoise(unit(i, n, ndim, dtype), fwd, inv, L, kind, t_unit(n), sigma=s)
        r.setflags(write=False)
        _DENOISE[key] = r
    return _DENOISE[key]


def zero_share(oracle, W, n, ndim, dtype, i, wname, L, lifting=False):
    """share of the coefficients of unit i that the hard threshold with the unit's own sigma zeroes"""
    fwd, _ = transforms(oracle, W, wname, lifting)
    c = fwd(unit(i, n, ndim, dtype), L)
    t = ref_sigma(oracle, W, n, ndim, dtype, i, wname, lifting) * t_unit(n)
    return float(np.mean(oracle.threshold(c, "hard", t) == 0))


def check_fixture(oracle, W, n, ndim, dtype, B, wname, L, kind="hard", lifting=False):
    """the conditions under which a batch separates "own sigma" from "somebody's sigma", asserted on the oracle's values"""
    tag = (n, ndim, np.dtype(dtype).name, B, wname, L, kind)
    sig = [ref_sigma(oracle, W, n, ndim, dtype, i, wname, lifting) for i in range(B)]
    assert len(set(sig)) == B, tag + ("sigmas not pairwise distinct", sig)
    for i in range(B):
        z = zero_share(oracle, W, n, ndim, dtype, i, wname, L, lifting)
        assert 0.2 < z < 0.999, tag + ("unit %d: share of zeroed coefficients %.4f" % (i, z),)
        if B > 1:
            own = ref_denoise(oracle, W, n, ndim, dtype, i, wname, L, kind, lifting)
            other = ref_denoise(oracle, W, n, ndim, dtype, i, wname, L, kind, lifting, sigma=sig[(i + 1) % B])
            assert not np.array_equal(own, other), tag + ("unit %d: the neighbour's sigma gives the same result" % i,)


def to_batch(W, us):
    """units stacked along a new last axis, column-major on the device: unit i at element offset i * prod(unit shape)"""
    return W.to_device(np.stack(us, axis=-1))
