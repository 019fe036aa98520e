"""Device bestbasistree / coefentropy (wl_bestbasistree_filter, wl_coefentropy) against the host restatement in
tests/bestbasis_ref.py, under the accuracy contract of DESIGN.md section 11: node coefficients bit-identical to wpt, node entropies
within TOL * sum|term| of the exact entropy of those coefficients, the tree equal on every node whose own and whose ancestors'
decision margins exceed the bound, always a valid tree, deterministic bytes."""
import math

import numpy as np
import pytest
import torch

import bestbasis_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
ENTS = ["ShannonEntropy", "LogEnergyEntropy"]
FAST_FILTERS = ["haar", "db2", "coif2", "db4", "sym5"]        # even, <= 10 taps: the packet kernels
FALLBACK_FILTERS = ["db8", "coif6", "batt2"]                   # 16, 18 and 23 (odd) taps: the per-depth generic kernels
_CONTENTS = {}


def _et(W, name):
    return getattr(W, name)()


def _signal(n, dtype, seed=0, kind="noise"):
    rng = np.random.default_rng(seed + n)
    if kind == "noise":
        return rng.standard_normal(n).astype(dtype)
    from wavelets_jl_amd import testfunction
    x = testfunction(n, kind) + 0.05 * rng.standard_normal(n)
    return x.astype(dtype)


def _contents(oracle, W, n, fname, dtype, kind="noise"):
    key = (n, fname, dtype, kind)
    if key not in _CONTENTS:
        x = _signal(n, dtype, kind=kind)
        wt = W.wavelet(getattr(W.WT, fname))
        _CONTENTS[key] = (x, wt, R.depth_contents(oracle, x, wt.qmf, R.maxtransformlevels(n)))
    return _CONTENTS[key]


# ---- coefentropy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("et", ENTS)
@pytest.mark.parametrize("n", [1, 7, 1000, 2 ** 16, 2 ** 22 + 6])
def test_coefentropy_within_contract(W, gpu, dtype, et, n):
    x = _signal(n, dtype, seed=3)
    code = 0 if et == "ShannonEntropy" else 1
    xd = W.to_device(x)
    T = np.dtype(dtype).type
    # nrm given: the terms are those of the exact form exactly
    nrm = R.exact_nrm(x) * T(1.5)
    got = W.coefentropy(xd, _et(W, et), float(nrm))
    t = R.exact_terms(x, nrm, code)
    ref, bound = math.fsum(t.tolist()), R.TOL[dtype] * float(np.abs(t).sum())
    assert abs(got - ref) <= bound + abs(ref) * float(np.finfo(dtype).eps), (got, ref, bound)
    assert float(T(got)) == got                                     # rounded to the element type
    # nrm defaulted: the device's norm may sit one ulp from the host's exactly rounded one
    nrm = R.exact_nrm(x)
    got = W.coefentropy(xd, _et(W, et))
    t = R.exact_terms(x, nrm, code)
    ref = math.fsum(t.tolist())
    bound = R.TOL[dtype] * float(np.abs(t).sum()) + R.nrm_ulp_effect(x, nrm, code) + abs(ref) * float(np.finfo(dtype).eps)
    assert abs(got - ref) <= bound, (got, ref, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("et", ENTS)
def test_coefentropy_zero_norm_zero_input_and_bad_norm(W, gpu, dtype, et):
    x = W.to_device(_signal(1000, dtype))
    assert W.coefentropy(x, _et(W, et), 0.0) == 0.0                 # nrm == 0: the reference's early return
    z = W.to_device(np.zeros(4096, dtype))
    v = W.coefentropy(z, _et(W, et))
    assert v == 0.0 and math.copysign(1, v) > 0
    assert W.coefentropy(z, _et(W, et), 1.0) == 0.0                 # every s == 0 term is -0.0, the sum +0.0
    with pytest.raises(W.ArgumentError):
        W.coefentropy(x, _et(W, et), -1.0)
    with pytest.raises(TypeError):
        W.coefentropy(x, "shannon")


# ---- node entropies ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("et", ENTS)
@pytest.mark.parametrize("fname", FAST_FILTERS + FALLBACK_FILTERS)
@pytest.mark.parametrize("n", [64, 320, 1000, 1024, 2 ** 16, 2 ** 20])
def test_node_entropy_every_node(W, gpu, oracle, dtype, et, fname, n):
    x, wt, cont = _contents(oracle, W, n, fname, dtype)
    code = 0 if et == "ShannonEntropy" else 1
    ex = R.Exact(cont, code)
    tree, ent = W.bestbasistree(W.to_device(x), wt, None, _et(W, et), return_entropy=True)
    ent = ent.cpu().numpy()
    assert ent.shape == ex.ent.shape
    bad = np.abs(ent - ex.ent) > ex.err
    assert not bad.any(), (np.flatnonzero(bad)[:10], ent[bad][:5], ex.ent[bad][:5], ex.err[bad][:5])
    ref_tree, certain = ex.decide(W.maketree(n))
    assert R.isvalidtree(n, tree)
    assert np.array_equal(tree[certain], ref_tree[certain])


# ---- trees --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("et", ENTS)
@pytest.mark.parametrize("kind", ["Doppler", "Blocks"])
@pytest.mark.parametrize("fname", ["db4", "sym5", "db8"])
def test_tree_matches_on_certain_nodes(W, gpu, oracle, dtype, et, kind, fname):
    n = 2 ** 14
    x, wt, cont = _contents(oracle, W, n, fname, dtype, kind)
    code = 0 if et == "ShannonEntropy" else 1
    ex = R.Exact(cont, code)
    xd = W.to_device(x)
    Lmax = R.maxtransformlevels(n)
    rng = np.random.default_rng(7)
    trees = [None, Lmax - 3, R.random_tree(rng, n), R.random_tree(rng, n, 0.9), np.zeros(2 ** Lmax - 1, np.uint8)]
    trees[-1][0] = 0
    for tr in trees:
        tin = W.maketree(n) if tr is None else (W.maketree(n, tr) if isinstance(tr, int) else tr)
        got = W.bestbasistree(xd, wt, tr, _et(W, et))
        want, certain = ex.decide(tin)
        assert got.dtype == np.uint8 and R.isvalidtree(n, got)
        assert np.array_equal(got[certain], want[certain])
        assert not np.any(got & ~tin.astype(bool))                # a subtree of the input tree
        if tr is None:
            # not vacuous: nearly every node is decided with margin, and the best tree is neither trivial nor the full tree
            assert certain.mean() > 0.99, certain.mean()
            if et == "ShannonEntropy":     # (log energy keeps the root on these signals: tests/test_bestbasis_host.py)
                assert 1 < got.sum() < len(got)
    got = W.bestbasistree(xd, wt, trees[-1], _et(W, et))
    assert not got.any()                                          # tree[1] == false: all false


@pytest.mark.parametrize("n", [1024, 320])
def test_reference_best_basis_case(W, gpu, n):
    """test/threshold.jl "Best basis": sine, db4, iwpt(wpt(x, wt, tree), wt, tree) ≈ x"""
    wt = W.wavelet(W.WT.db4)
    x = np.sin(4 * np.linspace(0, 2 * np.pi - np.finfo(float).eps, n))
    xd = W.to_device(x)
    tree = W.bestbasistree(xd, wt)
    assert R.isvalidtree(n, tree) and tree[0] == 1
    xr = W.to_host(W.iwpt(W.wpt(xd, wt, tree), wt, tree))
    assert np.allclose(xr, x, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_inputs(W, gpu, oracle, dtype):
    n = 1024
    wt = W.wavelet(W.WT.db4)
    rng = np.random.default_rng(1)
    for et in ENTS:
        x = _signal(n, dtype)
        x[17] = np.nan
        xd = W.to_device(x)
        assert np.array_equal(W.bestbasistree(xd, wt, None, _et(W, et)), W.maketree(n))        # NaN: the input tree comes back
        t = R.random_tree(rng, n)
        assert np.array_equal(W.bestbasistree(xd, wt, t, _et(W, et)), t)
        assert np.array_equal(W.bestbasistree(xd, wt, 4, _et(W, et)), W.maketree(n, 4))
        z = W.to_device(np.zeros(n, dtype))
        tz, ez = W.bestbasistree(z, wt, None, _et(W, et), return_entropy=True)
        assert not tz.any() and not ez.cpu().numpy().any()                                   # exact zeros: ties do not split
        imp = np.zeros(n, dtype)
        imp[100] = 1
        cont = R.depth_contents(oracle, imp, wt.qmf, R.maxtransformlevels(n))
        ex = R.Exact(cont, 0 if et == "ShannonEntropy" else 1)
        got, ent = W.bestbasistree(W.to_device(imp), wt, None, _et(W, et), return_entropy=True)
        assert not np.any(np.abs(ent.cpu().numpy() - ex.ent) > ex.err)
        want, certain = ex.decide(W.maketree(n))
        assert R.isvalidtree(n, got) and np.array_equal(got[certain], want[certain])


@pytest.mark.parametrize("dtype", DTYPES)
def test_deterministic(W, gpu, dtype):
    n = 2 ** 18 + 2 ** 10
    x = W.to_device(_signal(n, dtype))
    wt = W.wavelet(W.WT.sym5)
    a, ea = W.bestbasistree(x, wt, None, W.ShannonEntropy(), return_entropy=True)
    b, eb = W.bestbasistree(x, wt, None, W.ShannonEntropy(), return_entropy=True)
    assert np.array_equal(a, b)
    assert ea.cpu().numpy().tobytes() == eb.cpu().numpy().tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fname", ["haar", "db4", "sym5"])
def test_generic_path_agrees(W, gpu, dtype, fname):
    n = 2 ** 16
    x = W.to_device(_signal(n, dtype, kind="Doppler"))
    wt = W.wavelet(getattr(W.WT, fname))
    a, ea = W.bestbasistree(x, wt, None, W.ShannonEntropy(), return_entropy=True)
    W.set_kernel_path(1)
    try:
        b, eb = W.bestbasistree(x, wt, None, W.ShannonEntropy(), return_entropy=True)
    finally:
        W.set_kernel_path(0)
    # the packet content is bit-identical on both paths, so are the entropies and the tree
    assert np.array_equal(a, b)
    assert ea.cpu().numpy().tobytes() == eb.cpu().numpy().tobytes()


def test_large_float32_db4(W, gpu):
    n = 2 ** 24
    rng = np.random.default_rng(5)
    x = (W.testfunction(n, "Doppler") + 0.05 * rng.standard_normal(n)).astype(np.float32)
    xd = W.to_device(x)
    wt = W.wavelet(W.WT.db4)
    Lmax = R.maxtransformlevels(n)
    cont = [x] + [W.to_host(W.wpt(xd, wt, d)) for d in range(1, Lmax + 1)]        # wpt is bit-exact (tests/test_gpu_parity.py)
    ex = R.Exact(cont, 0)
    tree, ent = W.bestbasistree(xd, wt, None, W.ShannonEntropy(), return_entropy=True)
    ent = ent.cpu().numpy()
    assert not np.any(np.abs(ent - ex.ent) > ex.err)
    want, certain = ex.decide(W.maketree(n))
    assert certain.mean() > 0.99
    assert R.isvalidtree(n, tree) and np.array_equal(tree[certain], want[certain])


def test_argument_contract(W, gpu):
    x = W.to_device(_signal(1024, np.float64))
    wt = W.wavelet(W.WT.db4)
    with pytest.raises(TypeError):
        W.bestbasistree(x, W.wavelet(W.WT.cdf97, W.WT.Lifting))               # GLS: no best-basis search in the reference
    with pytest.raises(TypeError):
        W.bestbasistree(W.to_device(np.zeros((64, 64))), wt)                 # matrices
    with pytest.raises(TypeError):
        W.bestbasistree(x, "db4")
    with pytest.raises(W.ArgumentError):
        W.bestbasistree(x, wt, np.ones(7, np.uint8))                         # wrong length
    bad = W.maketree(1024, 3)
    bad[1] = 0
    with pytest.raises(W.ArgumentError):
        W.bestbasistree(x, wt, bad)                                           # a child under an unset node
    with pytest.raises(AssertionError):
        W.bestbasistree(x, wt, 11)                                            # maketree's assertion
    with pytest.raises(W.ArgumentError):
        W.bestbasistree(W.to_device(_signal(1001, np.float64)), wt)          # maxtransformlevels == 0
