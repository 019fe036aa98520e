"""Shared cases of matchingpursuit (needs no GPU): the reference loop of src/Threshold/basis_functions.jl:8-55 over a union of
orthonormal wavelet bases, built from oracle.dwt_filter and numpy, and the table of cases the host and GPU tests run.

    r = x;  y = zeros(T, N);  it = 0;  cap = (nmax == -1 ? N : nmax)
    while nrm(r) > tol && it < cap
        ftr = ft(r);  i = findmaxabs(ftr);  aphi = f(ftr[i] e_i);  r = T(r - aphi);  y[i] = T(y[i] + ftr[i]);  it += 1

findmaxabs is the reference's loop written out; r - aphi and y[i] += are done in T.  The one thing the device is allowed to do
differently is nrm (T(sqrt(Float64 sum of squares)), about 1 ulp of T from the exact norm).  Here every
iteration's norm is computed with math.fsum and asserted to be farther from tol than that bound -- 1 ulp of Float32, 1e-12
relative for Float64 -- so the iteration at which the loop ends is the same under either norm.  A case's tol is either given or
placed halfway between the norms of two consecutive iterations of a probe run (tol = ("after", k): the loop ends after k atoms).
"""
import functools
import math

import numpy as np

DTYPES = (np.float32, np.float64)
IDS = ("f32", "f64")

# name -> ((wavelet, L or None = maxtransformlevels), ...)
BASES = {
    "haar": (("haar", None),),
    "db4": (("db4", None),),
    "haar+db4": (("haar", None), ("db4", None)),
    "dirac+db4": (("db1", 0), ("db4", None)),            # spikes + wavelets
    "db2+sym5+db10@L2": (("db2", 2), ("sym5", 2), ("db10", 2)),
    "mixedL": (("haar", 1), ("db4", 3), ("db2", 2)),
    "haar@L3": (("haar", 3),),
    "haar@L3+db4@L2": (("haar", 3), ("db4", 2)),
}

# (n, bases, signal, tol, nmax); tol: a number, ("after", k) = between the norms after k - 1 and k atoms, "above" = above nrm(x)
_TABLE = (
    (2, "haar", "gauss", 1e-3, -1),
    (2, "haar", "gauss", 1e-3, 1),
    (8, "haar", "gauss", 1e-3, -1),
    (8, "db4", "gauss", 1e-3, -1),
    (8, "haar+db4", "gauss", 1e-3, -1),
    (8, "dirac+db4", "tie", 1e-3, -1),
    (8, "mixedL", "tie", 1e-3, 5),
    (8, "haar+db4", "atoms", ("after", 3), -1),
    (64, "haar", "gauss", 1e-3, 0),
    (64, "haar", "gauss", 1e-3, 1),
    (64, "db4", "gauss", 1e-3, 5),
    (64, "haar+db4", "atoms", ("after", 3), 40),
    (64, "dirac+db4", "atoms", ("after", 2), 40),
    (64, "dirac+db4", "tie", 1e-3, 5),
    (64, "db2+sym5+db10@L2", "gauss", 1e-3, 5),
    (64, "db2+sym5+db10@L2", "atoms", ("after", 3), 40),
    (64, "db2+sym5+db10@L2", "tie", 1e-3, 1),
    (64, "mixedL", "gauss", ("after", 4), 40),
    (64, "mixedL", "tie", 1e-3, 5),
    (64, "db4", "gauss", "above", -1),
    (1000, "haar@L3", "gauss", 1e-3, 5),
    (1000, "haar@L3+db4@L2", "atoms", ("after", 3), 40),
    (1000, "haar@L3+db4@L2", "tie", 1e-3, 1),
    (1000, "mixedL", "gauss", ("after", 6), 40),
    (4096, "haar", "gauss", 1e-3, 5),
    (4096, "db4", "atoms", ("after", 3), 40),
    (4096, "haar+db4", "gauss", ("after", 7), 40),
    (4096, "dirac+db4", "tie", 1e-3, 5),
    (4096, "haar+db4", "gauss", "above", 5),
    (65536, "haar+db4", "gauss", 1e-3, 4),
    (65536, "db4", "atoms", 1e-3, 4),
)


def case_id(c):
    n, bases, signal, tol, nmax = c
    t = tol if isinstance(tol, str) else ("after%d" % tol[1] if isinstance(tol, tuple) else "%g" % tol)
    return "n%d-%s-%s-tol_%s-nmax%d" % (n, bases, signal, t, nmax)


CASES = _TABLE
CASE_IDS = tuple(case_id(c) for c in CASES)


def findmaxabs(v):
    """basis_functions.jl:45-55, 0-based"""
    a = np.abs(v).tolist()
    m, k = a[0], 0
    for i, ai in enumerate(a):
        if ai > m:
            k, m = i, ai
    return k


def norm_exact(r):
    """sqrt of the exactly summed squares (Float32 squares are exact in Float64; Float64 squares are rounded once each)"""
    return math.sqrt(math.fsum(float(v) * float(v) for v in r.tolist()))


def norm_bound(nrm, dtype):
    """DESIGN.md section 11's bound on |device nrm - exact nrm|"""
    return float(np.spacing(np.float32(nrm))) if dtype == np.float32 else 1e-12 * nrm


def levels(W, bases, n):
    return [W.maxtransformlevels(n) if L is None else L for _, L in BASES[bases]]


def filters(W, bases):
    return [W.wavelet(getattr(W.WT, name)) for name, _ in BASES[bases]]


def _xf(oracle, v, q, L, fw):
    return v.copy() if L == 0 else oracle.dwt_filter(v, q, L, fw=fw)


def analysis(oracle, W, bases, r):
    """ft(r): the forward transforms of every base, concatenated"""
    n = len(r)
    return np.concatenate([_xf(oracle, r, w.qmf, L, True) for w, L in zip(filters(W, bases), levels(W, bases, n))])


def atom(oracle, W, bases, n, i, c, dtype):
    """f(c e_i): the inverse transform of the one block that holds the spike"""
    k, p = divmod(i, n)
    spat = np.zeros(n, dtype=dtype)
    spat[p] = c
    return _xf(oracle, spat, filters(W, bases)[k].qmf, levels(W, bases, n)[k], False)


def synthesis(oracle, W, bases, y):
    """f(y): the literal sum over the bases, in Float64 (for the identity x - f(y) = r)"""
    ws = filters(W, bases)
    n = len(y) // len(ws)
    out = np.zeros(n, dtype=np.float64)
    for k, (w, L) in enumerate(zip(ws, levels(W, bases, n))):
        out += _xf(oracle, np.ascontiguousarray(y[k * n:(k + 1) * n], dtype=np.float64), w.qmf, L, False)
    return out


def signal(oracle, W, n, bases, kind, dtype):
    K = len(BASES[bases])
    if kind == "gauss":
        return np.random.default_rng(1000 + n + K).standard_normal(n).astype(dtype)
    if kind == "tie":
        x = np.zeros(n, dtype=dtype)                         # integer-valued: e_0 + e_{n/2}
        x[0] = x[n // 2] = 1
        return x
    assert kind == "atoms"
    x = np.zeros(n, dtype=np.float64)
    for j, amp in enumerate((4.0, -2.0, 1.0)):               # three atoms from different bases (as far as there are that many)
        x += atom(oracle, W, bases, n, (j % K) * n + (5 * j + 3) % n, amp, np.float64)
    return x.astype(dtype)


def pursue(oracle, W, bases, x, tol, cap):
    """the reference loop; returns (y, r, niter, norms) with norms[k] = the exact norm the test before atom k saw (the last one
    is the norm the loop ended on, or the norm behind the last atom when the cap ended it)"""
    dtype = x.dtype.type
    n = len(x)
    N = n * len(BASES[bases])
    r, y = x.copy(), np.zeros(N, dtype=dtype)
    norms, ties = [norm_exact(r)], []
    it = 0
    while float(dtype(norms[-1])) > tol and it < cap:
        ftr = analysis(oracle, W, bases, r)
        i = findmaxabs(ftr)
        ties.append(int(np.count_nonzero(np.abs(ftr) == abs(ftr[i]))))
        aphi = atom(oracle, W, bases, n, i, ftr[i], dtype)
        r = (r - aphi).astype(dtype)
        y[i] = dtype(y[i] + ftr[i])
        it += 1
        norms.append(norm_exact(r))
    return y, r, it, norms, ties


@functools.lru_cache(maxsize=None)
def _reference(oracle, W, case, dtype):
    n, bases, kind, tol, nmax = case
    x = signal(oracle, W, n, bases, kind, dtype)
    N = n * len(BASES[bases])
    cap = N if nmax == -1 else nmax
    if tol == "above":
        tol = float("%.3g" % (1.5 * norm_exact(x)))
    elif isinstance(tol, tuple):
        k = tol[1]
        probe = pursue(oracle, W, bases, x, 1e-30, k)[3]
        assert len(probe) == k + 1 and probe[k] < probe[k - 1], (case, probe)
        tol = float("%.3g" % (0.5 * (probe[k - 1] + probe[k])))
    y, r, it, norms, ties = pursue(oracle, W, bases, x, tol, cap)
    # the condition on tol: no norm the loop tested is within the bound of tol
    for v in norms:
        assert abs(v - tol) > norm_bound(v, dtype), (case, dtype, v, tol)
    if kind == "tie":
        assert it >= 1 and ties[0] >= 2, (case, ties)
    return dict(x=x, y=y, r=r, niter=it, nrm=norms[-1], norms=tuple(norms), ties=tuple(ties), tol=tol, nmax=nmax, cap=cap,
                ended_by_norm=not float(dtype(norms[-1])) > tol)


def reference(oracle, W, case, dtype):
    """the shared, cached reference of a case (arrays are read-only)"""
    ref = _reference(oracle, W, case, dtype)
    for k in ("x", "y", "r"):
        ref[k].setflags(write=False)
    return ref
