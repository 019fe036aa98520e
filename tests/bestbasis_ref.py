"""Host restatement of the reference's best-basis search (src/Threshold/entropy.jl:15-133), in two forms.

exact            node coefficients of every depth from the oracle (one dwt level per segment: oracle.dwtc_filter on the depth's
                 segments as columns, which is what the reference's per-node `dwt!(dtmp, dx, wt, 1)` computes), s = (x / nrm)^2 in
                 T as the reference computes it, terms in Float64, one math.fsum per node; the decision in Float64 with a margin
                 and an error bound per node.  This is what the device's accuracy contract is stated against.
reference order  T arithmetic throughout, sequential sums from zero(T), nrm = norm(y) in T and the recursive bestsubtree_entropy
                 transcribed literally -- what the reference itself returns, up to its own log and BLAS norm.
"""
import math

import numpy as np

TOL = {np.float32: 4e-7, np.float64: 1e-12}     # contract: |device - exact| <= TOL * sum|term| (+ the effect of nrm's last ulp)


def maxtransformlevels(n):
    if n <= 1:
        return 0
    L = 0
    while n % (2 ** (L + 1)) == 0:
        L += 1
    return L


def depth_contents(oracle, x, qmf, Lmax):
    """[content of depth 0, 1, ..., Lmax] of the full packet decomposition, each in x's dtype (bit-identical to wpt(x, wt, d))"""
    out = [np.ascontiguousarray(x)]
    n = len(x)
    for d in range(Lmax):
        nj, nseg = n >> d, 1 << d
        cols = out[-1].reshape(nseg, nj).T                     # column s = segment s
        nxt = oracle.dwtc_filter(cols, qmf, 1)
        out.append(np.ascontiguousarray(nxt.T).reshape(-1))
    return out


def exact_nrm(x):
    """the contract's norm: T(sqrt(Float64 sum of squares)), here with an exactly rounded sum"""
    T = x.dtype.type
    return T(math.sqrt(math.fsum((x.astype(np.float64) ** 2).tolist())))


def s_values(c, nrm):
    T = c.dtype.type
    q = (c / T(nrm)).astype(T)
    return (q * q).astype(T)


def exact_terms(c, nrm, code):
    """Float64 terms of the T coefficients c (s == 0 -> -0.0), nrm == 0 -> all zero"""
    if nrm == 0:
        return np.zeros(len(c))
    s = s_values(c, nrm).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ls = np.log(s)
        t = -s * ls if code == 0 else -ls
    t[s == 0] = -0.0
    return t


def nrm_ulp_effect(c, nrm, code):
    """how far one ulp of nrm moves the node's entropy (the device's nrm may be one ulp off a host-computed one)"""
    if nrm == 0:
        return 0.0
    T = c.dtype.type
    s = s_values(c, nrm).astype(np.float64)
    d = 2.0 * float(np.finfo(T).eps) * 1.01
    with np.errstate(divide="ignore", invalid="ignore"):
        e = d * s * (np.abs(np.log(s)) + 1.0) if code == 0 else np.where(s > 0, d, 0.0)
    return float(np.nansum(e))


class Exact:
    """entr_bf / entr_af (Float64), their error bounds and the exact-arithmetic tree of the reference's algorithm.  Per node the sum
    is math.fsum (exactly rounded) on depths of at most 256 nodes, a Float64 numpy sum below them (segments short enough that its
    error is far under the bound)."""

    def __init__(self, contents, code, nrm=None, tol=None):
        x = contents[0]
        self.T = x.dtype.type
        n = len(x)
        self.Lmax = Lmax = len(contents) - 1
        self.ntree = ntree = 2 ** Lmax - 1
        self.naf = naf = 2 ** (Lmax - 1)
        self.nrm = exact_nrm(x) if nrm is None else self.T(nrm)
        tol = TOL[self.T] if tol is None else tol
        ent, err = [], []
        for d in range(Lmax + 1):
            nseg = 2 ** d if d < Lmax else naf
            c = contents[d].reshape(nseg, -1)
            t = exact_terms(contents[d], self.nrm, code).reshape(nseg, -1)
            if nseg <= 256:
                ent.append(np.array([math.fsum(r.tolist()) + 0.0 for r in t]))
            else:
                ent.append(t.sum(axis=1) + 0.0)
            eff = np.array([nrm_ulp_effect(r, self.nrm, code) for r in c]) if nseg <= 256 else nrm_ulp_effect_rows(c, self.nrm, code)
            err.append(tol * np.abs(t).sum(axis=1) + eff)
        self.ent, self.err = np.concatenate(ent), np.concatenate(err)
        self.bf, self.af = self.ent[:ntree], self.ent[ntree:]

    def decide(self, tree):
        """(tree, certain): the reference's tree in exact arithmetic, and per node whether it and every ancestor decide by more than
        the error bound (a certain-path node must come out the same from the device)"""
        ntree, Lmax, bf = self.ntree, self.Lmax, self.bf
        best, cs, ebest, ecs = np.zeros(ntree), np.zeros(ntree), np.zeros(ntree), np.zeros(ntree)
        for d in range(Lmax - 1, -1, -1):                        # 0-based node k = 2^d - 1 + j; children 2k+1, 2k+2
            k = np.arange(2 ** d - 1, 2 ** (d + 1) - 1)
            if d == Lmax - 1:
                cs[k], ecs[k] = self.af, self.err[ntree:]
            else:
                cs[k] = best[2 * k + 1] + best[2 * k + 2]
                ecs[k] = ebest[2 * k + 1] + ebest[2 * k + 2]
            b = np.where(cs[k] < bf[k], cs[k], bf[k])
            b = np.where(np.isnan(cs[k]), cs[k], b)
            best[k] = np.where(np.isnan(bf[k]), bf[k], b)
            ebest[k] = np.maximum(self.err[k], ecs[k])
        with np.errstate(invalid="ignore"):
            split = ~(bf <= cs)
            margin_ok = np.abs(bf - cs) > (self.err[:ntree] + ecs)
        tree = np.asarray(tree).astype(bool)
        out = tree & split
        certain = margin_ok.copy()
        for d in range(1, Lmax):
            k = np.arange(2 ** d - 1, 2 ** (d + 1) - 1)
            out[k] &= out[(k - 1) // 2]
            certain[k] &= certain[(k - 1) // 2]
        return out.astype(np.uint8), certain


def nrm_ulp_effect_rows(c, nrm, code):
    if nrm == 0:
        return np.zeros(c.shape[0])
    T = c.dtype.type
    s = s_values(c.reshape(-1), nrm).astype(np.float64).reshape(c.shape)
    d = 2.0 * float(np.finfo(T).eps) * 1.01
    with np.errstate(divide="ignore", invalid="ignore"):
        e = d * s * (np.abs(np.log(s)) + 1.0) if code == 0 else np.where(s > 0, d, 0.0)
    return np.nansum(e, axis=1)


def jl_min(a, b):
    """Julia's min for floats: NaN propagates"""
    if a != a:
        return a
    if b != b:
        return b
    if b < a or (math.copysign(1, b) < 0 < math.copysign(1, a) and a == b):
        return b
    return a


# ---- reference order -------------------------------------------------------------------------------------------------------------
def coefentropy_T(c, code, nrm):
    """coefentropy(x::AbstractArray{T}, et, nrm) literally: terms in T, a sequential sum from zero(T)"""
    T = c.dtype.type
    nrm = T(nrm)
    if nrm == 0:
        return T(0)
    s = s_values(c, nrm)
    with np.errstate(divide="ignore", invalid="ignore"):
        ls = np.log(s).astype(T)
        t = (-s * ls).astype(T) if code == 0 else (-ls).astype(T)
    t[s == 0] = T(-0.0)
    if len(t) == 0:
        return T(0)
    return T(np.cumsum(t, dtype=T)[-1] + T(0))


def bestbasistree_reference_order(contents, code, tree):
    """entropy.jl:47-111 in T arithmetic, bestsubtree_entropy recursive as written"""
    x = contents[0]
    T = x.dtype.type
    n = len(x)
    Lmax = len(contents) - 1
    ntree, naf = 2 ** Lmax - 1, 2 ** (Lmax - 1)
    nrm = T(np.linalg.norm(x))
    entr_bf = []
    for d in range(Lmax):
        nj = n >> d
        for s in range(2 ** d):
            entr_bf.append(coefentropy_T(contents[d][s * nj:(s + 1) * nj], code, nrm))
    ncoef = n // naf
    entr_af = [coefentropy_T(contents[Lmax][i * ncoef:(i + 1) * ncoef], code, nrm) for i in range(naf)]

    def bestsubtree_entropy(i):                                # 1-based, as in the reference
        if ntree < (i << 1):
            sm = entr_af[i - naf]
        else:
            sm = bestsubtree_entropy(i << 1)
            sm = T(sm + bestsubtree_entropy((i << 1) + 1))
        return jl_min(entr_bf[i - 1], sm)

    tree = np.asarray(tree).astype(bool)
    best = np.zeros(ntree, dtype=bool)
    for i in range(1, ntree + 1):
        if (i > 1 and not best[(i >> 1) - 1]) or not tree[i - 1]:
            best[i - 1] = False
        else:
            best[i - 1] = not (entr_bf[i - 1] <= bestsubtree_entropy(i))
    return best.astype(np.uint8)


def isvalidtree(n, b):
    ns = maxtransformlevels(n)
    if len(b) != 2 ** ns - 1:
        return False
    b = np.asarray(b).astype(bool)
    k = np.arange(1, len(b))
    return not np.any(b[k] & ~b[(k - 1) // 2])


def random_tree(rng, n, p=0.7):
    """a random valid tree: each child of a split node splits with probability p"""
    Lmax = maxtransformlevels(n)
    t = np.zeros(2 ** Lmax - 1, dtype=np.uint8)
    t[0] = 1
    for k in range(1, len(t)):
        t[k] = 1 if (t[(k - 1) // 2] and rng.random() < p) else 0
    return t
