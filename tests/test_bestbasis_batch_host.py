"""bestbasistree_batch and per-unit trees for wpt_batch (wl_bestbasistree_filter_batch, wl_wpt_filter_batch_trees;
W.bestbasistree_batch, W.wpt_batch / W.iwpt_batch with a tensor of trees): everything that can be checked without a device.

- the two symbols in the header, in _lib.SIGNATURES with the prototype's arity and pointer / scalar positions, and in `nm -D` of
  both libraries; a C99 translation unit that references them compiles against the header;
- the status codes whose rules need no device, in the documented order;
- the argument errors of the Python mirror, raised before any device call;
- the shared generator (bestbasis_batch_cases.py) gives batches whose units have different best bases that decide clearly.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bestbasis_batch_cases as BC
import bestbasis_ref as R
import lifting_schemes as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "wavelets_mi355x.h")
SYMS = ("wl_bestbasistree_filter_batch", "wl_wpt_filter_batch_trees")
# (device pointers -- trees_out, node_entropy, trees -- are bound as addresses)
C2CTYPES = {"wl_ctx *": (C.c_void_p,), "void *": (C.c_void_p,), "const void *": (C.c_void_p,), "int": (C.c_int,), "int64_t": (C.c_int64,),
            "const double *": (C.POINTER(C.c_double),), "const uint8_t *": (C.POINTER(C.c_uint8), C.c_void_p), "uint8_t *": (C.c_void_p,),
            "double *": (C.c_void_p,)}


def _prototype(sym):
    hdr = open(HDR).read()
    params = re.search(r"WL_API int %s\((.*?)\);" % sym, hdr, re.S).group(1)
    out = []
    for p in params.split(","):
        p = " ".join(p.split())
        m = re.match(r"(.*?)(\w+)$", p)
        out.append((m.group(1).strip(), m.group(2)))
    return out


def test_symbols_in_header_signatures_and_both_libraries(W):
    from wavelets_jl_amd import _lib
    lib = _lib.load()
    for s in SYMS:
        proto = _prototype(s)
        assert s in _lib.SIGNATURES and _lib.SIGNATURES[s][0] is C.c_int
        argtypes = _lib.SIGNATURES[s][1]
        assert len(proto) == len(argtypes), s
        for k, ((ctype, name), at) in enumerate(zip(proto, argtypes)):
            assert at in C2CTYPES[ctype], (s, k, name, ctype, at)
        assert hasattr(lib, s)
    names = [n for _, n in _prototype("wl_bestbasistree_filter_batch")]
    assert names == ["ctx", "dtype", "x", "n", "nunits", "unit_stride", "qmf", "flen", "tree", "ntree", "L", "et", "trees_out", "tree_stride",
                     "node_entropy", "entropy_stride", "stream"]
    names = [n for _, n in _prototype("wl_wpt_filter_batch_trees")]
    assert names == ["ctx", "dtype", "y", "x", "n", "nunits", "unit_stride", "qmf", "flen", "trees", "tree_stride", "L", "fw", "stream"]
    # the host tree of the search is a host pointer, the per-unit trees of the transform are an address
    assert _lib.SIGNATURES[SYMS[0]][1][8] is C.POINTER(C.c_uint8) and _lib.SIGNATURES[SYMS[1]][1][9] is C.c_void_p
    for path in _lib.LIB_PATHS.values():
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert set(SYMS) <= set(re.findall(r" T (wl_[a-z0-9_]+)", out)), path
    # the order of the status codes, the closure rule and the workspace formula are part of the header comment
    flat = " ".join(open(HDR).read().split())
    assert ("WL_EINVAL_ARG (NULL ctx / x / qmf / trees_out, unknown et), WL_EINVAL_DTYPE, WL_EINVAL_FILTER, * WL_EDIMS (n < 1, nunits < 1, "
            "unit_stride < n, tree_stride < ntree, entropy_stride < ntree + 2^(Lmax-1), products >= 2^61), * WL_EINVAL_SIZE (odd n), "
            "WL_EINVAL_L (tree == NULL), WL_EINVAL_TREE.") in flat
    assert "an INVALID tree means its largest valid subtree" in flat
    assert "wl_bestbasistree_filter is G = 1 of the same formula" in flat
    assert "DESIGN.md section 15" in flat


def test_a_c99_translation_unit_compiles_against_the_header(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "wavelets_mi355x.h"\n'
                   "int use(wl_ctx *c, void *y, const void *x, const double *q, const uint8_t *t, uint8_t *o, double *e, void *s)\n"
                   "{ return wl_bestbasistree_filter_batch(c, WL_F32, x, 64, 3, 68, q, 8, t, 63, 0, WL_ENTROPY_SHANNON, o, 66, e, 95, s)\n"
                   "       + wl_bestbasistree_filter_batch(c, WL_F64, x, 64, 3, 64, q, 8, (const uint8_t *)0, 0, 6, WL_ENTROPY_LOGENERGY, o, 63,\n"
                   "                                       (double *)0, 0, s)\n"
                   "       + wl_wpt_filter_batch_trees(c, WL_F64, y, x, 64, 3, 64, q, 8, o, 63, 6, 1, s); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def test_status_codes_in_order_through_a_dummy_context(W):
    """one argument set per rule that breaks that rule and every later one; the argument rules run before the context is touched, so
    a block of zero bytes serves as the context (and host memory as the device buffers: nothing is launched)"""
    lib = W._lib.load()
    ST = W._lib.STATUS
    buf, buf2 = (C.c_float * 4096)(), (C.c_float * 4096)()
    p, p2 = C.cast(buf, C.c_void_p), C.cast(buf2, C.c_void_p)
    dummy = C.cast((C.c_char * 4096)(), C.c_void_p)
    q = (C.c_double * 64)(*([0.5] * 64))
    u8 = C.POINTER(C.c_uint8)
    bad_tree = np.zeros(63, dtype=np.uint8)
    bad_tree[1] = 1
    bt = bad_tree.ctypes.data_as(u8)
    good_tree = np.ones(63, dtype=np.uint8)
    gt = good_tree.ctypes.data_as(u8)

    def f(ctx=dummy, x=p, dtype=0, n=64, nunits=2, stride=64, qmf=True, flen=4, tree=None, ntree=63, L=2, et=0, out=p2, tstride=63,
          ent=None, estride=95):
        return ST[lib.wl_bestbasistree_filter_batch(ctx, dtype, x, n, nunits, stride, q if qmf else None, flen, tree, ntree, L, et, out, tstride,
                                                    ent, estride, None)]

    # n = 63 is odd (WL_EINVAL_SIZE) and shorter than nothing else; with it every stride rule passes, so WL_EDIMS needs nunits = 0
    bad = dict(dtype=7, flen=1, nunits=0, n=63, stride=63, L=-1)
    assert f(ctx=None, **bad) == f(x=None, **bad) == f(qmf=False, **bad) == f(out=None, **bad) == "WL_EINVAL_ARG"
    assert f(et=2, **bad) == f(et=-1, **bad) == "WL_EINVAL_ARG"
    assert f(**bad) == "WL_EINVAL_DTYPE"
    assert f(**{**bad, "dtype": 0}) == f(**{**bad, "dtype": 1, "flen": 65}) == "WL_EINVAL_FILTER"
    assert f(**{**bad, "dtype": 0, "flen": 4}) == "WL_EDIMS"
    assert f(n=0, L=-1) == f(stride=63, L=-1) == f(nunits=1 << 40, stride=1 << 40, L=-1) == "WL_EDIMS"
    assert f(tstride=62, L=-1) == f(ent=p, estride=94, L=-1) == f(tstride=62, tree=bt) == "WL_EDIMS"
    assert f(n=63, stride=63, L=-1) == f(n=63, stride=63, tree=bt) == f(n=1, stride=1, L=0) == "WL_EINVAL_SIZE"
    assert f(L=-1) == f(L=7) == f(L=-1, ent=p) == "WL_EINVAL_L"
    assert f(tree=bt, L=-1) == f(tree=gt, ntree=62) == f(tree=gt, ntree=0) == "WL_EINVAL_TREE"       # (L is ignored with a tree)

    def g(ctx=dummy, y=p, x=p, dtype=0, n=64, nunits=2, stride=64, qmf=True, flen=4, trees=p2, tstride=63, L=2):
        return ST[lib.wl_wpt_filter_batch_trees(ctx, dtype, y, x, n, nunits, stride, q if qmf else None, flen, trees, tstride, L, 1, None)]

    bad = dict(dtype=7, flen=1, nunits=0, L=-1)                          # (y == x as well: every later rule is broken)
    assert g(ctx=None, **bad) == g(y=None, **bad) == g(x=None, **bad) == g(qmf=False, **bad) == g(trees=None, **bad) == "WL_EINVAL_ARG"
    assert g(**bad) == "WL_EINVAL_DTYPE"
    assert g(**{**bad, "dtype": 0}) == g(**{**bad, "dtype": 1, "flen": 65}) == "WL_EINVAL_FILTER"
    assert g(nunits=0, L=-1) == g(n=0, L=-1) == g(stride=63, L=-1) == g(nunits=1 << 40, stride=1 << 40, L=-1) == g(tstride=62, L=-1) == "WL_EDIMS"
    assert g(L=-1) == g(L=7) == "WL_EALIAS"
    assert g(y=p2, trees=p, L=-1) == g(y=p2, trees=p, L=7) == "WL_EINVAL_L"


def test_python_argument_errors_need_no_device(W):
    import torch

    def cpu(*shape, dtype=torch.float32):
        return torch.zeros(*reversed(shape), dtype=dtype).permute(*reversed(range(len(shape))))

    wt, sch = W.wavelet(W.WT.db4), LS.scheme(W, "cdf97")
    x = cpu(64, 3)
    f = W.bestbasistree_batch
    for bad in (sch, "db4", None):
        with pytest.raises(TypeError, match="bestbasistree_batch"):
            f(x, bad)
    for shape in ((64,), (8, 8, 3)):
        with pytest.raises(TypeError, match="bestbasistree_batch expects a len x B array"):
            f(cpu(*shape), wt)
    with pytest.raises(TypeError, match="bestbasistree_batch is not defined for complex arrays"):
        f(cpu(64, 3, dtype=torch.complex64), wt)
    with W.complex_arrays():
        with pytest.raises(TypeError, match="bestbasistree_batch is not defined for complex arrays"):
            f(cpu(64, 3, dtype=torch.complex64), wt)
    with pytest.raises(TypeError, match="ShannonEntropy"):
        f(x, wt, None, "shannon")
    for L in (7, -1):
        with pytest.raises(AssertionError, match="maxtransformlevels"):
            f(x, wt, L)
    trees = torch.zeros(3, 63, dtype=torch.uint8).t()
    for g in (W.wpt_batch, W.iwpt_batch):
        with pytest.raises(TypeError, match=g.__name__ + " with one tree per unit is defined for orthogonal filters only"):
            g(x, sch, trees)
        with pytest.raises(TypeError, match=g.__name__ + ": a tensor of trees must be uint8 or bool"):
            g(x, wt, trees.to(torch.int32))
        for shape in ((63,), (62, 3), (63, 2), (3, 63)):
            with pytest.raises(AssertionError, match=g.__name__ + ": trees must have shape"):
                g(x, wt, torch.zeros(*shape, dtype=torch.uint8))
        with pytest.raises(TypeError, match=g.__name__ + " expects a len x B array"):
            g(cpu(64), wt, trees)
        with pytest.raises(TypeError, match=g.__name__ + ": L bounds a tensor of per-unit trees only"):
            g(x, wt, 3, L=2)
    assert "bestbasistree_batch" in W.__all__
    # valid arguments get as far as the device check, here without a device: no TypeError / AssertionError
    if not torch.cuda.is_available():
        for call in (lambda: f(x, wt), lambda: f(x, wt, 3, W.LogEnergyEntropy(), return_entropy=True), lambda: f(x, wt, W.maketree(64, 3, "dwt")),
                     lambda: W.wpt_batch(x, wt, trees), lambda: W.iwpt_batch(x, wt, trees.to(torch.bool), L=3)):
            with pytest.raises(W.HIPError):
                call()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("fname", BC.CHECK_FILTERS)
@pytest.mark.parametrize("n", BC.CHECK_N)
def test_the_generator_gives_distinct_and_certain_best_bases(W, oracle, dtype, fname, n):
    """the two conditions the GPU tests rest on, through the host restatement: the units of a batch have different Shannon best
    bases (a neighbour's tree would show) and nearly every node decides by more than the contract's error bound (so the device's
    tree is pinned on nearly every node)"""
    full = W.maketree(n)
    trees, shares = [], []
    for i in range(BC.CHECK_B):
        ex = BC.exact(oracle, W, i, n, fname, dtype, 0)
        tree, certain = ex.decide(full)
        assert R.isvalidtree(n, tree)
        trees.append(tree)
        shares.append(float(certain.mean()))
    assert BC.distinct(trees) >= BC.MIN_DISTINCT, (n, fname, BC.distinct(trees))
    assert min(shares) > BC.MIN_CERTAIN, (n, fname, shares)
