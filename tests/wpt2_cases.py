"""Shared cases of wpt2 / iwpt2 (needs no GPU): the definition of the 2-D wavelet packet transform as a recursion over the oracle's
one-level 2-D dwt of a copied block, the quadtree helpers restated, and the table of cases the host and GPU tests run.

The node at depth d with block coordinates (bi, bj), 0 <= bi, bj < 2^d, is the sub-block of rows bi n0 / 2^d ... and columns
bj n1 / 2^d ... of the n0 x n1 image.  Splitting a node replaces the block by its one-level dwt, periodic within the block; the
four quadrants [[ss, sd], [ds, dd]] are the children c = ci + 2 cj (ci = 1: the lower half of dimension 0, cj = 1: the right half
of dimension 1).  The tree is a uint8 vector in breadth-first order: node k has the children 4k + 1 + c, depth d starts at
(4^d - 1) / 3 and the index inside a depth is the Morton code of (bi, bj) with bi in the even bits.
"""
import numpy as np

DTYPES = (np.float32, np.float64)
IDS = ("f32", "f64")

# (n0, n1, L): what it hits
SHAPES = (
    (2, 2, 1),          # smallest possible
    (8, 8, 3),          # 1 x 1 leaves
    (16, 4, 2),         # non-square, 2-wide nodes
    (24, 40, 3),        # not powers of two, odd 3 x 5 leaves
    (64, 64, 6),        # deepest power-of-two case
    (96, 32, 5),        # non-square, deep
    (256, 128, 4),      # several tiles per node in the level kernel
    (200, 120, 3),      # tiles that straddle node and image edges
)
SHAPE_IDS = tuple("%dx%d-L%d" % s for s in SHAPES)
# haar (2 taps), db4 (8), sym5 (10), db8 (16) and the 59-tap Battle-Lemarie filter: taps far longer than the node
FILTERS = ("haar", "db4", "sym5", "db8", "batt6")
TREES = ("full", "dwt", "rand1", "rand2", "root")


def tree_size(L):
    """nodes of a quadtree of depth bound L"""
    return (4 ** L - 1) // 3


def depth_base(d):
    """index of the first node of depth d"""
    return (4 ** d - 1) // 3


def morton(bi, bj):
    """bi in the even bits, bj in the odd bits"""
    code, bit = 0, 0
    while (bi >> bit) or (bj >> bit):
        code |= ((bi >> bit) & 1) << (2 * bit) | ((bj >> bit) & 1) << (2 * bit + 1)
        bit += 1
    return code


def node_index(d, bi, bj):
    return depth_base(d) + morton(bi, bj)


def node_coords(k):
    """(d, bi, bj) of node k, by walking up: node k is child c = (k - 1) % 4 of node (k - 1) // 4"""
    path = []
    while k > 0:
        path.append((k - 1) % 4)
        k = (k - 1) // 4
    bi = bj = 0
    for c in reversed(path):
        bi, bj = 2 * bi + (c & 1), 2 * bj + (c >> 1)
    return len(path), bi, bj


def maxlevels(n0, n1):
    L = 0
    while n0 % (2 ** (L + 1)) == 0 and n1 % (2 ** (L + 1)) == 0:
        L += 1
    return L


def maketree2(n0, n1, L, kind):
    assert 0 <= L <= maxlevels(n0, n1)
    b = np.zeros(tree_size(L), dtype=np.uint8)
    if kind == "full":
        b[:] = 1
    elif kind == "dwt":
        for d in range(L):
            b[depth_base(d)] = 1        # child 0 of child 0 of ...: Morton code 0 of every depth
    else:
        raise ValueError(kind)
    return b


def isvalidtree2(shape, tree):
    n0, n1 = shape
    L = 0
    while tree_size(L) < len(tree):
        L += 1
    if tree_size(L) != len(tree) or n0 % 2 ** L or n1 % 2 ** L:
        return False
    return all(not tree[k] or tree[(k - 1) // 4] for k in range(1, len(tree)))


def random_tree(L, seed, p=0.6):
    """a valid tree: the root splits, every other node splits with probability p if its parent does"""
    rng = np.random.default_rng(seed)
    b = np.zeros(tree_size(L), dtype=np.uint8)
    if L > 0:
        b[0] = 1
    for k in range(1, len(b)):
        b[k] = 1 if b[(k - 1) // 4] and rng.random() < p else 0
    return b


def make_tree(n0, n1, L, kind):
    if kind in ("full", "dwt"):
        return maketree2(n0, n1, L, kind)
    if kind == "root":
        b = np.zeros(tree_size(L), dtype=np.uint8)
        b[0] = 1
        return b
    return random_tree(L, 1000 * n0 + 10 * n1 + int(kind[-1]))


def wpt2_ref(oracle, x, qmf, tree, L, fw=True):
    """the normative statement: the recursion over the unchanged oracle"""
    n0, n1 = x.shape
    y = np.array(x, copy=True)
    contiguous = np.ascontiguousarray

    def run(k, d, r0, c0):                     # y starts as a copy of x
        if d >= L or not tree[k]: return
        m0, m1 = n0 >> d, n1 >> d
        if fw:  y[r0:r0+m0, c0:c0+m1] = oracle.dwt_filter(contiguous(y[r0:r0+m0, c0:c0+m1]), qmf, 1)
        for c in range(4): run(4*k+1+c, d+1, r0 + (c & 1)*(m0//2), c0 + (c >> 1)*(m1//2))
        if not fw: y[r0:r0+m0, c0:c0+m1] = oracle.dwt_filter(contiguous(y[r0:r0+m0, c0:c0+m1]), qmf, 1, fw=False)

    run(0, 0, 0, 0)
    return y


def qmf_of(W, name):
    return W.wavelet(getattr(W.WT, name)).qmf


def image(shape, dtype, seed=0):
    n0, n1 = shape
    return np.random.default_rng(7919 * n0 + 31 * n1 + seed).standard_normal((n0, n1)).astype(dtype)


_CACHE = {}


def reference(oracle, W, shape, L, fname, dtype, kind):
    """{x, tree, y = wpt2(x), xr = iwpt2(y)} of a case, computed once and shared (callers must not write to the arrays)"""
    key = (shape, L, fname, np.dtype(dtype).name, kind)
    if key not in _CACHE:
        x = image(shape, dtype)
        tree = make_tree(shape[0], shape[1], L, kind)
        q = qmf_of(W, fname)
        y = wpt2_ref(oracle, x, q, tree, L, True)
        xr = wpt2_ref(oracle, y, q, tree, L, False)
        for a in (x, tree, y, xr):
            a.setflags(write=False)
        _CACHE[key] = dict(x=x, tree=tree, y=y, xr=xr)
    return _CACHE[key]
