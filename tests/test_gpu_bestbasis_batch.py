"""The batched best-basis search and the packet transforms with one tree per unit on the device (wl_bestbasistree_filter_batch,
wl_wpt_filter_batch_trees; W.bestbasistree_batch, W.wpt_batch / W.iwpt_batch with a tensor of trees).

- batch = loop: tree bytes and node-entropy bit patterns of every unit equal W.bestbasistree of that unit alone;
- independent of the code under test: entropies within the contract's bound of the host restatement (tests/bestbasis_ref.py on the
  oracle's packet content), the tree equal to the exact decision on every certain node, always a valid tree;
- wpt_batch / iwpt_batch with per-unit trees: np.array_equal with the CPU oracle's packet transform of each unit with its own tree.
Every buffer -- signals, trees, entropies -- sits between guard bands of a sentinel and a padded batch carries the sentinel in its
padding; all of them are read back after the call.  The inputs are those of tests/bestbasis_batch_cases.py: neighbouring units
have different best bases, so a unit computed with a neighbour's tree, norm or entropies differs."""
import ctypes as C
import math

import numpy as np
import pytest

import bestbasis_batch_cases as BC
import bestbasis_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements on either side of a buffer (a multiple of 16 bytes for every element type used)
SENT = -7.25                    # what guard bands and padding of the floating-point buffers hold
TSENT = 0xA5                    # ... and those of the tree bytes
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
CODE = {np.float32: 0, np.float64: 1}
ENTS = ["ShannonEntropy", "LogEnergyEntropy"]
PACKET_FILTERS = ["haar", "db4", "sym5"]       # even, <= 10 taps: the packet kernels
FALLBACK_FILTERS = ["db8", "batt2"]            # 16 and 11 (odd) taps: the per-depth kernels
BS = (1, 3, 7, 67)
ST = {"WL_EINVAL_SIZE": -1, "WL_EINVAL_L": -2, "WL_EALIAS": -3, "WL_EDIMS": -4, "WL_EINVAL_TREE": -6, "WL_EINVAL_DTYPE": -8,
      "WL_EINVAL_FILTER": -9, "WL_EINVAL_ARG": -10}


def strides(n, ntree):
    """(unit stride, tree stride, entropy stride - its minimum): dense, padded and aligned, misaligned (the transform then takes the
    per-depth kernels; the search copies a padded batch into dense buffers and runs the dense plan either way)"""
    return [(n, ntree, 0), (n + 4, ntree + 3, 5), (n + 1, ntree, 0)]


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def filt(W, name):
    return W.wavelet(getattr(W.WT, name))


def sentinel(dtype):
    return np.uint8(TSENT) if np.dtype(dtype) == np.uint8 else np.dtype(dtype).type(SENT)


def padded(torch, gpu, rows, S):
    """rows (B, m) -> a device buffer [guard | B units of stride S | guard], everything else the sentinel; (buffer, offset of unit 0)"""
    B, m = rows.shape
    buf = np.full(GUARD + B * S + GUARD, sentinel(rows.dtype), dtype=rows.dtype)
    buf[GUARD: GUARD + B * S].reshape(B, S)[:, :m] = rows
    return torch.from_numpy(buf).to(gpu), GUARD


def blank(torch, gpu, B, m, S, dtype):
    return padded(torch, gpu, np.full((B, m), sentinel(dtype), dtype=dtype), S)


def unpack(torch, buf, base, B, m, S):
    """(units (B, m), True when every guard / padding element still holds the sentinel)"""
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    body = h[base: base + B * S].reshape(B, S)
    rest = np.concatenate((h[:base], body[:, m:].ravel(), h[base + B * S:]))
    return body[:, :m].copy(), bool(np.all(rest == sentinel(h.dtype)))


def ptr(buf, base):
    return C.c_void_p(buf.data_ptr() + base * buf.element_size())


def sizes(n):
    Lmax = R.maxtransformlevels(n)
    ntree = 2 ** Lmax - 1
    return Lmax, ntree, ntree + 2 ** (Lmax - 1)


def search(W, torch, gpu, wt, us, et, tree=None, S=None, TSR=None, ES=None, want_ent=True):
    """one wl_bestbasistree_filter_batch call on guarded buffers -> (trees (B, ntree), entropies (B, nent) or None); the guards, the
    padding and the source are checked here.  tree: None / an integer depth / one host tree."""
    B, n = us.shape
    Lmax, ntree, nent = sizes(n)
    S, TSR, ES = S or n, TSR or ntree, ES or nent
    xb, base = padded(torch, gpu, us, S)
    tb, _ = blank(torch, gpu, B, ntree, TSR, np.uint8)
    eb = blank(torch, gpu, B, nent, ES, np.float64)[0] if want_ent else None
    h, st = W.transforms._context(xb.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    if tree is None or isinstance(tree, (int, np.integer)):
        tp, nt, L = None, 0, Lmax if tree is None else int(tree)
    else:
        tree = np.ascontiguousarray(tree, dtype=np.uint8)
        tp, nt, L = tree.ctypes.data_as(C.POINTER(C.c_uint8)), len(tree), 0
    rc = W._lib.load().wl_bestbasistree_filter_batch(h, CODE[us.dtype.type], ptr(xb, base), n, B, S, q.ctypes.data_as(C.POINTER(C.c_double)),
                                                     len(q), tp, nt, L, getattr(W, et).code, ptr(tb, base), TSR,
                                                     ptr(eb, base) if want_ent else None, ES, st)
    assert rc == 0, (rc, n, B, S, TSR, ES)
    trees, tclean = unpack(torch, tb, base, B, ntree, TSR)
    assert tclean, ("guard bands / padding of the trees written", n, B, TSR)
    ent = None
    if want_ent:
        ent, eclean = unpack(torch, eb, base, B, nent, ES)
        assert eclean, ("guard bands / padding of the entropies written", n, B, ES)
    src, sclean = unpack(torch, xb, base, B, n, S)
    assert sclean and np.array_equal(ibits(src), ibits(us)), ("source changed", n, B, S)
    assert set(np.unique(trees)) <= {0, 1}
    return trees, ent


def transform(W, torch, gpu, wt, us, trees, fw, S=None, TSR=None, L=None):
    """one wl_wpt_filter_batch_trees call on guarded buffers -> the units of y; guards, padding, source and trees are checked"""
    B, n = us.shape
    Lmax, ntree, _ = sizes(n)
    S, TSR = S or n, TSR or ntree
    xb, base = padded(torch, gpu, us, S)
    yb, _ = blank(torch, gpu, B, n, S, us.dtype)
    tb, _ = padded(torch, gpu, np.ascontiguousarray(trees, dtype=np.uint8), TSR)
    h, st = W.transforms._context(xb.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    rc = W._lib.load().wl_wpt_filter_batch_trees(h, CODE[us.dtype.type], ptr(yb, base), ptr(xb, base), n, B, S,
                                                 q.ctypes.data_as(C.POINTER(C.c_double)), len(q), ptr(tb, base), TSR, Lmax if L is None else L,
                                                 1 if fw else 0, st)
    assert rc == 0, (rc, n, B, S, TSR)
    got, clean = unpack(torch, yb, base, B, n, S)
    assert clean, ("guard bands / padding written", n, B, S)
    src, sclean = unpack(torch, xb, base, B, n, S)
    assert sclean and np.array_equal(ibits(src), ibits(us)), ("source changed", n, B, S)
    tr, tclean = unpack(torch, tb, base, B, ntree, TSR)
    assert tclean and np.array_equal(tr, trees), ("trees changed", n, B, TSR)
    return got


_LOOP = {}


def loop(W, us, fname, et, tree=None, key=None):
    """W.bestbasistree of every unit alone -> (trees, entropies); computed once per unit and case (unit i is the same in every B)"""
    B, n = us.shape
    wt = filt(W, fname)
    trees, ents = [], []
    for i in range(B):
        k = (i, n, us.dtype.name, fname, et, key)
        if key is None or k not in _LOOP:
            t, e = W.bestbasistree(W.to_device(us[i]), wt, tree, getattr(W, et)(), return_entropy=True)
            v = (np.array(t), e.cpu().numpy())
            if key is None:
                trees.append(v[0]); ents.append(v[1])
                continue
            _LOOP[k] = v
        trees.append(_LOOP[k][0]); ents.append(_LOOP[k][1])
    return np.stack(trees), np.stack(ents)


def same(trees, ent, lt, le, what):
    assert np.array_equal(trees, lt), (what, "trees", np.argwhere(trees != lt)[:5].tolist())
    assert np.array_equal(ent.view(np.uint64), le.view(np.uint64)), (what, "entropies", np.argwhere(ent.view(np.uint64) != le.view(np.uint64))[:5].tolist())


# ---- batch = loop ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("et", ENTS)
@pytest.mark.parametrize("n", [64, 320, 1000, 1024])
def test_batch_is_the_loop_bit_for_bit(gpu, W, dtype, et, n):
    """every small-group tier of the reduction (segments of 1024 ... 2 samples, non-power-of-two bottoms at 320 and 1000), several
    whole units per tail workgroup with a short last workgroup (no B divides TS / n), padded and misaligned batches, the packet
    kernels and the per-depth fallbacks"""
    import torch
    _, ntree, nent = sizes(n)
    all_us = BC.units(n, dtype, max(BS))
    for fname in PACKET_FILTERS + FALLBACK_FILTERS:
        lt, le = loop(W, all_us, fname, et, key="full")
        for B in BS:
            for S, TSR, epad in strides(n, ntree):
                trees, ent = search(W, torch, gpu, filt(W, fname), all_us[:B], et, S=S, TSR=TSR, ES=nent + epad)
                same(trees, ent, lt[:B], le[:B], (n, fname, B, S, TSR))
    # without node_entropy the entropies live in the workspace: the same trees
    trees, _ = search(W, torch, gpu, filt(W, "db4"), all_us[:7], et, S=n + 4, want_ent=False)
    assert np.array_equal(trees, loop(W, all_us[:7], "db4", et, key="full")[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("et", ENTS)
@pytest.mark.parametrize("n", [8192, 2 ** 14])
def test_batch_is_the_loop_beyond_one_workgroup(gpu, W, dtype, et, n):
    """n > TS: the fused multi kernels over all units then the tail on each unit's chunks; segments of 4096 samples and more take
    the 256-lane pieces and the fold of 2 (8192) and 4 (2^14) pieces"""
    import torch
    _, ntree, nent = sizes(n)
    us = BC.units(n, dtype, 3)
    for fname in ("db4", "db8"):
        lt, le = loop(W, us, fname, et, key="full")
        for S, TSR, epad in strides(n, ntree):
            trees, ent = search(W, torch, gpu, filt(W, fname), us, et, S=S, TSR=TSR, ES=nent + epad)
            same(trees, ent, lt, le, (n, fname, S, TSR))


# ---- independent of the code under test -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fname", BC.CHECK_FILTERS)
@pytest.mark.parametrize("n", [320, 1024, 8192])
def test_entropies_and_trees_against_the_host_restatement(gpu, W, oracle, dtype, fname, n):
    import torch
    B = BC.CHECK_B
    us = BC.units(n, dtype, B)
    trees, ent = search(W, torch, gpu, filt(W, fname), us, "ShannonEntropy", S=n + 4)
    full = W.maketree(n)
    shares = []
    for i in range(B):
        ex = BC.exact(oracle, W, i, n, fname, dtype, 0)
        bad = np.abs(ent[i] - ex.ent) > ex.err
        assert not bad.any(), (i, np.flatnonzero(bad)[:10], ent[i][bad][:5], ex.ent[bad][:5], ex.err[bad][:5])
        ref_tree, certain = ex.decide(full)
        assert R.isvalidtree(n, trees[i]), i
        assert np.array_equal(trees[i][certain], ref_tree[certain]), i
        shares.append(float(certain.mean()))
    assert BC.distinct(trees) >= BC.MIN_DISTINCT, BC.distinct(trees)
    assert min(shares) > BC.MIN_CERTAIN, shares


# ---- input trees ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [320, 1024])
def test_input_trees(gpu, W, dtype, n):
    import torch
    Lmax, ntree, nent = sizes(n)
    us = BC.units(n, dtype, 7)
    wt = filt(W, "db4")
    rng = np.random.default_rng(n)
    for et in ENTS:
        # a full tree of a depth below Lmax: nothing at depth >= L is set, and it is the loop
        for L in (Lmax - 2, 1, 0):
            trees, ent = search(W, torch, gpu, wt, us, et, tree=L, S=n + 4, TSR=ntree + 3)
            lt, le = loop(W, us, "db4", et, tree=L)
            same(trees, ent, lt, le, (n, et, "L", L))
            assert not trees[:, 2 ** L - 1:].any()
        # one random partial host tree shared by all units: every result is a subtree of it
        shared = R.random_tree(rng, n, 0.8)
        trees, ent = search(W, torch, gpu, wt, us, et, tree=shared)
        lt, le = loop(W, us, "db4", et, tree=shared)
        same(trees, ent, lt, le, (n, et, "shared"))
        assert not trees[:, shared == 0].any()
        assert all(R.isvalidtree(n, t) for t in trees)
        # an unset root: nothing splits
        noroot = shared.copy()
        noroot[:] = 0
        trees, _ = search(W, torch, gpu, wt, us, et, tree=noroot)
        assert not trees.any()
    # a NaN unit among finite ones returns the input tree (every comparison with NaN is false: every node of the tree stays split);
    # an all-zero unit has norm 0, every entropy exactly 0 and nothing splits; the neighbours are those of the clean batch
    clean, cent = search(W, torch, gpu, wt, us, "ShannonEntropy", S=n + 4)
    odd = us.copy()
    odd[2, n // 3] = np.nan
    odd[4, :] = 0
    for tree, tin in ((None, W.maketree(n)), (Lmax - 1, W.maketree(n, Lmax - 1)), (shared, shared)):
        base, bent = (clean, cent) if tree is None else search(W, torch, gpu, wt, us, "ShannonEntropy", tree=tree, S=n + 4)
        trees, ent = search(W, torch, gpu, wt, odd, "ShannonEntropy", tree=tree, S=n + 4)
        assert np.array_equal(trees[2], tin) and np.isnan(ent[2]).all()
        assert not trees[4].any() and not ent[4].any() and not np.signbit(ent[4]).any()
        keep = [0, 1, 3, 5, 6]
        assert np.array_equal(trees[keep], base[keep]) and np.array_equal(ent[keep].view(np.uint64), bent[keep].view(np.uint64))


# ---- wpt_batch / iwpt_batch with one tree per unit -----------------------------------------------------------------------------------------
def closure(tree, L=None):
    """the largest valid subtree (a node counts iff it and every ancestor is set), cut at depth L"""
    t = np.asarray(tree).astype(bool).copy()
    if L is not None:
        t[2 ** L - 1:] = False
    for k in range(1, len(t)):
        t[k] &= t[(k - 1) // 2]
    return t.astype(np.uint8)


def unit_trees(n, B, seed):
    """seeded random valid trees, neighbours different (unit u: split probability 0.5 + 0.07 (u % 7))"""
    rng = np.random.default_rng(seed)
    out = [R.random_tree(rng, n, 0.5 + 0.07 * (u % 7)) for u in range(B)]
    for u in range(1, B):
        while np.array_equal(out[u], out[u - 1]):
            out[u] = R.random_tree(rng, n, 0.5 + 0.07 * (u % 7))
    return np.stack(out)


_ORACLE = {}


def expect(oracle, wt, us, trees, fw, key=None):
    """the oracle's packet transform of every unit with its own tree (cached per unit where the caller names the case)"""
    out = []
    for i in range(len(us)):
        k = (key, i, us.shape[1], us.dtype.name, fw)
        if key is None or k not in _ORACLE:
            v = oracle.wpt_filter(np.ascontiguousarray(us[i]), wt.qmf, np.ascontiguousarray(trees[i], dtype=np.uint8).copy(), fw=fw)
            if key is None:
                out.append(v)
                continue
            _ORACLE[k] = v
        out.append(_ORACLE[k])
    return np.stack(out)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [64, 320, 1000, 1024])
def test_packet_transforms_with_per_unit_trees(gpu, W, oracle, dtype, n):
    """forward, inverse and round trip against the oracle, unit by unit: the trees of the search and random trees that differ between
    neighbouring units (a unit transformed with a neighbour's tree differs); the same B / stride / filter grid as the search"""
    import torch
    Lmax, ntree, _ = sizes(n)
    all_us = BC.units(n, dtype, max(BS))
    rt = unit_trees(n, max(BS), n)
    assert not any(np.array_equal(rt[u], rt[u - 1]) for u in range(1, len(rt)))
    for fname in PACKET_FILTERS + FALLBACK_FILTERS:
        wt = filt(W, fname)
        found, _ = search(W, torch, gpu, wt, all_us, "ShannonEntropy", want_ent=False)
        for kind, trees in (("search", found), ("random", rt)):
            ye = expect(oracle, wt, all_us, trees, True, key=(fname, kind))
            xe = expect(oracle, wt, ye, trees, False, key=(fname, kind))
            for B in BS:
                for S, TSR, _ in strides(n, ntree):
                    y = transform(W, torch, gpu, wt, all_us[:B], trees[:B], True, S=S, TSR=TSR)
                    assert np.array_equal(ibits(y), ibits(ye[:B])), ("fwd", n, fname, kind, B, S, TSR, W.last_kernel())
                    x = transform(W, torch, gpu, wt, ye[:B], trees[:B], False, S=S, TSR=TSR)
                    assert np.array_equal(ibits(x), ibits(xe[:B])), ("inv", n, fname, kind, B, S, TSR, W.last_kernel())
            # round trip (the oracle's values are the device's, bit for bit): rounding only, ~ eps * depths * filter length, for the
            # orthogonal filters (batt2 is a truncated filter: its bank does not reconstruct exactly)
            if fname != "batt2":
                tol = 1e-4 if dtype == np.float32 else 1e-10
                assert np.abs(xe.astype(np.float64) - all_us).max() <= tol * np.abs(all_us).max(), (n, fname, kind)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [8192, 2 ** 14])
def test_packet_transforms_with_per_unit_trees_beyond_one_workgroup(gpu, W, oracle, dtype, n):
    import torch
    _, ntree, _ = sizes(n)
    us = BC.units(n, dtype, 3)
    rt = unit_trees(n, 3, n)
    for fname in ("db4", "db8"):
        wt = filt(W, fname)
        found, _ = search(W, torch, gpu, wt, us, "ShannonEntropy", want_ent=False)
        for kind, trees in (("search", found), ("random", rt)):
            ye = expect(oracle, wt, us, trees, True, key=(fname, kind))
            xe = expect(oracle, wt, ye, trees, False, key=(fname, kind))
            for S, TSR, _ in strides(n, ntree):
                y = transform(W, torch, gpu, wt, us, trees, True, S=S, TSR=TSR)
                kf = W.last_kernel()
                assert np.array_equal(ibits(y), ibits(ye)), ("fwd", n, fname, kind, S, kf)
                x = transform(W, torch, gpu, wt, ye, trees, False, S=S, TSR=TSR)
                assert np.array_equal(ibits(x), ibits(xe)), ("inv", n, fname, kind, S, W.last_kernel())
                if fname == "db4" and S != n + 1:
                    assert kf == "k_wpt_fwd_multi", kf


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_invalid_trees_depth_bound_and_kernel_path(gpu, W, oracle, dtype):
    """a node set under an unset parent does not count (the tree means its largest valid subtree); nodes at depth >= L are ignored;
    wl_ctx_set_path(ctx, 1) gives the same bits"""
    import torch
    for n in (1024, 8192, 320):
        Lmax, ntree, _ = sizes(n)
        us = BC.units(n, dtype, 3)
        wt = filt(W, "db4")
        trees = unit_trees(n, 3, 5 * n)
        bad = trees.copy()
        bad[0, 1] = 0                      # unit 0: the left child of the root unset, its descendants left as they were
        bad[1, 0] = 0                      # unit 1: the root unset under a populated tree: the unit is copied
        bad[1, 1] = 1
        bad[2, 2] = 0
        bad[2, 5:7] = 1                    # unit 2: both children of the unset right child set
        assert not R.isvalidtree(n, bad[2]) and not R.isvalidtree(n, bad[1])
        closed = np.stack([closure(t) for t in bad])
        assert not closed[1].any()
        ye = expect(oracle, wt, us, closed, True)
        for S in (n, n + 1):
            y = transform(W, torch, gpu, wt, us, bad, True, S=S)
            assert np.array_equal(ibits(y), ibits(ye)), (n, S)
            assert np.array_equal(ibits(y[1]), ibits(us[1]))
            x = transform(W, torch, gpu, wt, ye, bad, False, S=S)
            assert np.array_equal(ibits(x), ibits(expect(oracle, wt, ye, closed, False))), (n, S)
        for L in (0, 1, Lmax - 2):
            cut = np.stack([closure(t, L) for t in trees])
            yl = expect(oracle, wt, us, cut, True)
            assert np.array_equal(ibits(transform(W, torch, gpu, wt, us, trees, True, L=L, S=n + 4)), ibits(yl)), (n, L)
            assert np.array_equal(ibits(transform(W, torch, gpu, wt, yl, trees, False, L=L, S=n + 4)),
                                  ibits(expect(oracle, wt, yl, cut, False))), (n, L)
        yv = expect(oracle, wt, us, trees, True)
        W.set_kernel_path(1)
        try:
            assert np.array_equal(ibits(transform(W, torch, gpu, wt, us, trees, True)), ibits(yv)), n
            assert not W.last_kernel().startswith("k_wpt")
            assert np.array_equal(ibits(transform(W, torch, gpu, wt, yv, trees, False)), ibits(expect(oracle, wt, yv, trees, False))), n
            t1, e1 = search(W, torch, gpu, wt, us, "ShannonEntropy")
        finally:
            W.set_kernel_path(0)
        t0, e0 = search(W, torch, gpu, wt, us, "ShannonEntropy")
        same(t1, e1, t0, e0, (n, "path 1"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_groups_change_no_bit(gpu, W, oracle, dtype):
    """five units in groups of two (WL_WPT_BATCH_GROUP = 2): two full groups and a short one, both entry points"""
    import torch
    for n in (1024, 8192):
        _, ntree, nent = sizes(n)
        us = BC.units(n, dtype, 5)
        wt = filt(W, "db4")
        shared = R.random_tree(np.random.default_rng(3), n, 0.85)
        t0, e0 = search(W, torch, gpu, wt, us, "ShannonEntropy", S=n + 4, TSR=ntree + 3, ES=nent + 5)
        s0, f0 = search(W, torch, gpu, wt, us, "LogEnergyEntropy", tree=shared)
        rt = unit_trees(n, 5, 7 * n)
        ye = expect(oracle, wt, us, rt, True)
        W.set_option("WL_WPT_BATCH_GROUP", 2)
        t1, e1 = search(W, torch, gpu, wt, us, "ShannonEntropy", S=n + 4, TSR=ntree + 3, ES=nent + 5)
        s1, f1 = search(W, torch, gpu, wt, us, "LogEnergyEntropy", tree=shared)
        y = transform(W, torch, gpu, wt, us, rt, True, S=n + 4, TSR=ntree + 3)
        x = transform(W, torch, gpu, wt, ye, rt, False, S=n + 4, TSR=ntree + 3)
        W.clear_options()
        same(t1, e1, t0, e0, (n, "groups"))
        same(s1, f1, s0, f0, (n, "groups, shared tree"))
        same(t0, e0, *loop(W, us, "db4", "ShannonEntropy", key="full"), (n, "loop"))
        assert np.array_equal(ibits(y), ibits(ye)) and np.array_equal(ibits(x), ibits(expect(oracle, wt, ye, rt, False))), n


# ---- the Python mirror ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_python_mirror(gpu, W, oracle, dtype):
    import torch
    n, B = 1024, 7
    Lmax, ntree, nent = sizes(n)
    us = BC.units(n, dtype, B)
    wt = filt(W, "sym5")
    x = W.to_device(np.asfortranarray(us.T))
    for et in ENTS:
        lt, le = loop(W, us, "sym5", et, key="full")
        trees, ent = W.bestbasistree_batch(x, wt, None, getattr(W, et)(), return_entropy=True)
        assert trees.dtype == torch.uint8 and trees.device == x.device and tuple(trees.shape) == (ntree, B) and trees.stride(0) == 1
        assert ent.dtype == torch.float64 and tuple(ent.shape) == (nent, B)
        same(trees.cpu().numpy().T, np.ascontiguousarray(ent.cpu().numpy().T), lt, le, et)
    trees = W.bestbasistree_batch(x, wt)
    assert isinstance(trees, torch.Tensor) and np.array_equal(trees.cpu().numpy().T, loop(W, us, "sym5", "ShannonEntropy", key="full")[0])
    t3 = W.bestbasistree_batch(x, wt, 3).cpu().numpy().T
    assert np.array_equal(t3, loop(W, us, "sym5", "ShannonEntropy", tree=3)[0])
    shared = R.random_tree(np.random.default_rng(1), n, 0.8)
    assert np.array_equal(W.bestbasistree_batch(x, wt, shared.astype(bool)).cpu().numpy().T, loop(W, us, "sym5", "ShannonEntropy", tree=shared)[0])
    # the trees go straight into wpt_batch / iwpt_batch, as uint8 or bool, column-major or not
    th = trees.cpu().numpy().T
    ye = expect(oracle, wt, us, th, True)
    for tr in (trees, trees.to(torch.bool), trees.t().contiguous().t().contiguous()):
        y = W.wpt_batch(x, wt, tr)
        assert np.array_equal(ibits(W.to_host(y).T), ibits(ye))
        xr = W.iwpt_batch(y, wt, tr)
        assert np.array_equal(ibits(W.to_host(xr).T), ibits(expect(oracle, wt, ye, th, False)))
    # a broadcast view (every column the tree of unit 0, stride 0 between columns) is materialised, not read past its one column
    one = trees[:, :1].expand(ntree, B)
    assert one.stride(1) == 0
    yb = W.wpt_batch(x, wt, one)
    assert np.array_equal(ibits(W.to_host(yb).T), ibits(expect(oracle, wt, us, np.repeat(th[:1], B, axis=0), True)))
    y2 = W.wpt_batch(x, wt, trees, L=2)
    assert np.array_equal(ibits(W.to_host(y2).T), ibits(expect(oracle, wt, us, np.stack([closure(t, 2) for t in th]), True)))
    with pytest.raises(W.ArgumentError, match="in array is out array"):
        W.wpt_batch(x, wt, trees, y=x)
    with pytest.raises(AssertionError, match="trees must have shape"):
        W.wpt_batch(x, wt, trees[:, :3])
    with pytest.raises(TypeError, match="orthogonal filters only"):
        W.wpt_batch(x, W.wavelet(W.WT.cdf97, W.WT.Lifting), trees)
    with pytest.raises(W.ArgumentError):
        W.wpt_batch(x, wt, trees, L=Lmax + 1)
    with pytest.raises(W.ArgumentError):
        W.bestbasistree_batch(W.to_device(np.zeros((63, 2), dtype)), wt)      # odd length: WL_EINVAL_SIZE


# ---- hipGraph ----------------------------------------------------------------------------------------------------------------------------------
def test_hipgraph_capture_and_replay(gpu, W):
    """search + wpt_batch(trees) captured in one graph on one stream (full input tree; a warm call has grown the workspace), replayed
    twice on new inputs: the bits of the eager calls"""
    import torch
    n, B = 4096, 12
    wt = filt(W, "db4")
    base = BC.units(n, np.float32, B)
    inputs = [np.asfortranarray((np.roll(base, k, axis=0) * (1 + k)).T) for k in range(3)]
    eager = []
    for a in inputs:
        t = W.bestbasistree_batch(W.to_device(a), wt)
        eager.append((t.cpu().numpy(), W.to_host(W.wpt_batch(W.to_device(a), wt, t))))
    assert not np.array_equal(eager[0][0], eager[1][0])
    x = W.to_device(inputs[0])
    y = W.similar(x)
    s = torch.cuda.Stream()
    _, ntree, nent = sizes(n)
    trees = torch.zeros((B, ntree), dtype=torch.uint8, device=gpu).t()
    lib = W._lib.load()
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    qp = q.ctypes.data_as(C.POINTER(C.c_double))

    def pipeline():
        h, st = W.transforms._context(x.device)
        assert lib.wl_bestbasistree_filter_batch(h, 0, C.c_void_p(x.data_ptr()), n, B, n, qp, len(q), None, 0, 12, 0, C.c_void_p(trees.data_ptr()),
                                                 ntree, None, 0, st) == 0
        W.wpt_batch(x, wt, trees, y=y)

    with torch.cuda.stream(s):
        pipeline()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        pipeline()
    for k in (1, 2):
        x.copy_(W.to_device(inputs[k]))
        y.zero_()
        trees.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(trees.cpu().numpy(), eager[k][0]), k
        assert np.array_equal(ibits(W.to_host(y)), ibits(eager[k][1])), k
    del graph


# ---- the fused library -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_library(gpu, W, oracle, dtype):
    """search: batch = loop bit for bit in the fused library too (the single search is the batch of one of the same instances); wpt
    with per-unit trees: within the fused tolerances of test_gpu_fused.py against the Float64 oracle"""
    import torch
    f64 = dtype == np.float64
    with W.arithmetic("fused"):
        for n, fnames, B in ((64, PACKET_FILTERS, 67), (1024, PACKET_FILTERS + ["db8"], 7), (8192, ["db4"], 3)):
            Lmax, ntree, nent = sizes(n)
            us = BC.units(n, dtype, B)
            for fname in fnames:
                wt = filt(W, fname)
                for et in ENTS:
                    lt, le = loop(W, us, fname, et)
                    for S, TSR in ((n, ntree), (n + 4, ntree + 3)):
                        trees, ent = search(W, torch, gpu, wt, us, et, S=S, TSR=TSR)
                        same(trees, ent, lt, le, ("fused", n, fname, et, S))
                trees, _ = search(W, torch, gpu, wt, us, "ShannonEntropy", want_ent=False)
                ref = expect(oracle, wt, us.astype(np.float64), trees, True)
                y = transform(W, torch, gpu, wt, us, trees, True, S=n + 4)
                xr = transform(W, torch, gpu, wt, y, trees, False, S=n + 4)
                for i in range(B):
                    if trees[i, 0]:
                        rel = np.linalg.norm(y[i].astype(np.float64) - ref[i]) / np.linalg.norm(ref[i])
                        assert rel <= (1e-13 if f64 else 1e-6) * math.sqrt(Lmax), (n, fname, i, rel)
                        if not f64:
                            assert np.abs(y[i] - ref[i]).max() <= 1e-5 * max(1.0, np.abs(ref[i]).max()), (n, fname, i)
                    else:
                        assert np.array_equal(ibits(y[i]), ibits(us[i]))
                assert np.abs(xr.astype(np.float64) - us).max() <= (1e-12 if f64 else 1e-5) * max(1.0, np.abs(us).max()), (n, fname)
    assert W.get_arithmetic() == "exact"


# ---- status codes --------------------------------------------------------------------------------------------------------------------------
def test_status_codes_on_a_live_context(gpu, W):
    """the documented order with a real context, and nothing is written by a failed call"""
    import torch
    lib = W._lib.load()
    n, B, S = 64, 3, 68
    _, ntree, nent = sizes(n)
    us = BC.units(n, np.float32, B)
    xb, base = padded(torch, gpu, us, S)
    yb, _ = blank(torch, gpu, B, n, S, np.float32)
    tb, _ = blank(torch, gpu, B, ntree, ntree, np.uint8)
    h, st = W.transforms._context(xb.device)
    q = np.ascontiguousarray(filt(W, "db2").qmf, dtype=np.float64)
    qp = q.ctypes.data_as(C.POINTER(C.c_double))
    bad = np.zeros(63, dtype=np.uint8)
    bad[1] = 1
    badp = bad.ctypes.data_as(C.POINTER(C.c_uint8))
    X, Y, TR, null = ptr(xb, base), ptr(yb, base), ptr(tb, base), C.c_void_p(None)

    def f(ctx=h, x=X, dtype=0, n=n, B=B, S=S, q_=qp, flen=4, tree=None, nt=0, L=2, et=0, out=TR, ts=ntree):
        return lib.wl_bestbasistree_filter_batch(ctx, dtype, x, n, B, S, q_, flen, tree, nt, L, et, out, ts, None, 0, st)

    def g(ctx=h, y=Y, x=X, dtype=0, n=n, B=B, S=S, q_=qp, flen=4, trees=TR, ts=ntree, L=2):
        return lib.wl_wpt_filter_batch_trees(ctx, dtype, y, x, n, B, S, q_, flen, trees, ts, L, 1, st)

    assert f(ctx=null) == f(x=null) == f(q_=None) == f(out=null) == f(et=2) == ST["WL_EINVAL_ARG"]
    assert f(dtype=2) == g(dtype=-1) == ST["WL_EINVAL_DTYPE"]
    assert f(flen=1) == g(flen=65) == ST["WL_EINVAL_FILTER"]
    assert f(n=0) == f(B=0) == f(S=63) == f(ts=62) == g(n=0) == g(B=0) == g(S=63) == g(ts=62) == ST["WL_EDIMS"]
    assert f(n=63, S=63) == ST["WL_EINVAL_SIZE"]
    assert g(y=X) == ST["WL_EALIAS"]
    assert f(L=-1) == f(L=7) == g(L=-1) == g(L=7) == ST["WL_EINVAL_L"]
    assert f(tree=badp, nt=63) == f(tree=badp, nt=62) == ST["WL_EINVAL_TREE"]
    assert f(et=2, dtype=2, flen=1, B=0, L=-1) == ST["WL_EINVAL_ARG"] and f(dtype=2, flen=1, B=0, L=-1) == ST["WL_EINVAL_DTYPE"]
    assert f(flen=1, B=0, L=-1) == ST["WL_EINVAL_FILTER"] and f(ts=62, L=-1) == ST["WL_EDIMS"]
    assert g(trees=null, dtype=2) == ST["WL_EINVAL_ARG"] and g(B=0, y=X, L=-1) == ST["WL_EDIMS"] and g(y=X, L=-1) == ST["WL_EALIAS"]
    got, clean = unpack(torch, yb, base, B, n, S)
    assert clean and np.all(got == np.float32(SENT))
    tr, clean = unpack(torch, tb, base, B, ntree, ntree)
    assert clean and np.all(tr == TSENT)
