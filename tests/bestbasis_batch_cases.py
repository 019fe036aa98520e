"""Shared inputs of the bestbasistree_batch tests (test_bestbasis_batch_host.py, test_gpu_bestbasis_batch.py).

Unit i of n samples is drawn with default_rng(100 + i):
    i % 5 == 4   standard normal noise
    otherwise    testfunction(n, ("Doppler", "Blocks", "Bumps", "HeaviSine")[i % 5]) + 0.05 (i // 5 + 1) * standard normal noise
cast to the element type: neighbouring units are different signals, so their best bases differ and a result computed with a
neighbour's tree (or a neighbour's norm) shows.  Under Shannon entropy the 7 units of a batch have at least 6 distinct best bases at
n in {64, 320, 1024, 8192} with haar and db4 in both element types, and at least 98.4 % of every unit's nodes decide by more than
the error bound of the accuracy contract (the worst case is Float32 haar at 8192); test_bestbasis_batch_host.py holds the generator
to the weaker conditions MIN_DISTINCT and MIN_CERTAIN below.  Under log energy most units keep only the root (2-3 distinct trees from 320 samples on).

Every reference is computed once per case and shared: callers must not modify what they get.
"""
import functools

import numpy as np

import bestbasis_ref as R

KINDS = ("Doppler", "Blocks", "Bumps", "HeaviSine")
MIN_DISTINCT = 4        # distinct Shannon best bases among the 7 units of a batch (at least)
MIN_CERTAIN = 0.97      # share of a unit's nodes that decide by more than the contract's error bound (more than)
CHECK_N = (64, 320, 1024, 8192)
CHECK_FILTERS = ("haar", "db4")
CHECK_B = 7


@functools.lru_cache(maxsize=None)
def unit(i, n, dtype):
    from wavelets_jl_amd import testfunction
    noise = np.random.default_rng(100 + i).standard_normal(n)
    a = noise if i % 5 == 4 else testfunction(n, KINDS[i % 5]) + 0.05 * (i // 5 + 1) * noise
    a = a.astype(dtype)
    a.setflags(write=False)
    return a


def units(n, dtype, B):
    """(B, n): unit i in row i"""
    return np.stack([unit(i, n, np.dtype(dtype).name) for i in range(B)])


_EXACT = {}


def exact(oracle, W, i, n, fname, dtype, code):
    """bestbasis_ref.Exact of unit i (the oracle's packet content of every depth, exact entropies and their error bounds)"""
    key = (i, n, fname, np.dtype(dtype).name, code)
    if key not in _EXACT:
        wt = W.wavelet(getattr(W.WT, fname))
        x = np.array(unit(i, n, np.dtype(dtype).name))
        _EXACT[key] = R.Exact(R.depth_contents(oracle, x, wt.qmf, R.maxtransformlevels(n)), code)
    return _EXACT[key]


def distinct(trees):
    """number of different trees among the rows / list entries"""
    return len({np.asarray(t, dtype=np.uint8).tobytes() for t in trees})
