"""Best-basis search, CPU side: the two host forms of tests/bestbasis_ref.py agree away from near-ties, the scalar coefentropy
formulas (entropy.jl:15-30), the argument checks that run before the device, and the new ABI symbols in the header, in
_lib.SIGNATURES and in the built library."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bestbasis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wl_coefentropy", "wl_bestbasistree_filter")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("code", [0, 1])
@pytest.mark.parametrize("fname,n,kind", [("db4", 1024, "Doppler"), ("haar", 256, "Blocks"), ("sym5", 320, "HeaviSine"),
                                          ("db8", 512, "Bumps")])
def test_exact_and_reference_order_agree_away_from_ties(W, oracle, dtype, code, fname, n, kind):
    rng = np.random.default_rng(n)
    x = (W.testfunction(n, kind) + 0.05 * rng.standard_normal(n)).astype(dtype)
    wt = W.wavelet(getattr(W.WT, fname))
    cont = R.depth_contents(oracle, x, wt.qmf, R.maxtransformlevels(n))
    # the reference-order form carries the reference's own error, ~n eps(T) sum|term|: near-ties at that scale may go either way
    ex = R.Exact(cont, code, tol=4 * n * float(np.finfo(dtype).eps))
    for tree in (W.maketree(n), W.maketree(n, 2), R.random_tree(rng, n)):
        want, certain = ex.decide(tree)
        got = R.bestbasistree_reference_order(cont, code, tree)
        assert R.isvalidtree(n, got) and R.isvalidtree(n, want)
        assert certain.mean() > 0.9
        assert np.array_equal(got[certain], want[certain])


def test_depth_contents_are_the_packet_transform(W, oracle):
    """depth d of the helper is wpt(x, wt, maketree(n, d, :full)), bit for bit (the reference's own per-node dwt! levels)"""
    rng = np.random.default_rng(2)
    for dtype in (np.float32, np.float64):
        x = rng.standard_normal(320).astype(dtype)
        wt = W.wavelet(W.WT.db4)
        cont = R.depth_contents(oracle, x, wt.qmf, 6)
        for d in range(7):
            assert np.array_equal(cont[d], oracle.wpt_filter(x, wt.qmf, W.maketree(320, d)))


def test_exact_tree_is_not_trivial_on_the_gpu_test_signals(W, oracle):
    """the GPU tree test asserts that nearly every node is certain and, for Shannon, a best tree that is neither empty nor full"""
    n = 2 ** 14
    for kind in ("Doppler", "Blocks"):
        for fname in ("db4", "sym5", "db8"):
            for dtype in (np.float32, np.float64):
                rng = np.random.default_rng(0 + n)
                x = (W.testfunction(n, kind) + 0.05 * rng.standard_normal(n)).astype(dtype)
                wt = W.wavelet(getattr(W.WT, fname))
                cont = R.depth_contents(oracle, x, wt.qmf, R.maxtransformlevels(n))
                for code in (0, 1):
                    t, certain = R.Exact(cont, code).decide(W.maketree(n))
                    assert certain.mean() > 0.99, (kind, fname, dtype, code, certain.mean())
                    if code == 0:        # (log energy keeps the root here: its entropy grows with every split of these signals)
                        assert 1 < t.sum() < len(t), (kind, fname, dtype, code, t.sum())


def test_scalar_coefentropy(W):
    sh, le = W.ShannonEntropy(), W.LogEnergyEntropy()
    for et in (sh, le):
        for zero in (0.0, np.float32(0.0), -0.0):
            v = W.coefentropy(zero, et, 1.0 if not isinstance(zero, np.float32) else np.float32(1))
            assert v == 0 and math.copysign(1, v) < 0                    # s == 0 contributes -zero(T)
    x, nrm = 0.3, 2.0
    s = (x / nrm) ** 2
    assert W.coefentropy(x, sh, nrm) == -s * math.log(s)
    assert W.coefentropy(x, le, nrm) == -math.log(s)
    xf, nf = np.float32(0.3), np.float32(2.0)
    v = W.coefentropy(xf, sh, nf)
    assert isinstance(v, np.float32)
    q = np.float32(xf / nf)
    sf = np.float32(q * q)
    assert v == np.float32(-sf * np.log(sf))
    assert W.coefentropy(xf, le, nf) == np.float32(-np.log(sf))
    with pytest.raises(TypeError):
        W.coefentropy(0.3, sh)                                           # a scalar needs nrm
    with pytest.raises(TypeError):
        W.coefentropy(0.3, "ShannonEntropy", 1.0)


def test_reference_order_sums_start_from_positive_zero():
    z = np.zeros(8, np.float32)
    v = R.coefentropy_T(z, 0, np.float32(1))
    assert v == 0 and math.copysign(1, v) > 0                            # zero(T) + (-0.0) + ... == +0.0
    assert R.coefentropy_T(np.ones(4, np.float64), 0, 0.0) == 0.0         # nrm == 0: early return


def test_argument_checks_before_the_device(W):
    x = np.zeros(64)
    with pytest.raises(TypeError):
        W.bestbasistree(x, W.wavelet(W.WT.cdf97, W.WT.Lifting))           # GLS: a MethodError in the reference
    with pytest.raises(TypeError):
        W.bestbasistree(x, W.wavelet(W.WT.db4), None, "shannon")
    with pytest.raises(TypeError):
        W.bestbasistree(x, W.wavelet(W.WT.db4))                            # a host array: there is no CPU path


def test_new_symbols_in_header_signatures_and_library(W):
    hdr = open(os.path.join(ROOT, "include", "wavelets_mi355x.h")).read()
    assert re.search(r"enum wl_entropy \{ WL_ENTROPY_SHANNON = 0, WL_ENTROPY_LOGENERGY = 1 \}", hdr)
    for s in NEW_SYMBOLS:
        assert re.search(r"WL_API int %s\(" % s, hdr), s
        assert s in W._lib.SIGNATURES, s
    nm = subprocess.run(["nm", "-D", "--defined-only", W._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (\w+)$", nm, re.M))
    assert set(NEW_SYMBOLS) <= exported
    lib = W._lib.load()
    assert all(getattr(lib, s) for s in NEW_SYMBOLS)
