"""matchingpursuit / findmaxabs (wl_findmaxabs, wl_mp_select, wl_mp_residual, wl_matchingpursuit_filter): everything that can be
checked without a device.

- the four symbols in the header, in _lib.SIGNATURES with the prototypes' arity and pointer / scalar positions, and in `nm -D` of
  both libraries; a C99 translation unit that references them compiles against the header;
- every status code in the documented order, through a block of zero bytes as the context (the argument rules run before the
  context is touched);
- the AssertionErrors and TypeErrors of the Python mirror, raised before any device call; the names in __all__;
- the shared case builder's own conditions: the ties exist, every tol keeps its margin, and for a single orthonormal basis y
  after m atoms holds the m largest coefficients of dwt(x).
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import matchingpursuit_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "wavelets_mi355x.h")
SYMS = {"wl_findmaxabs": 6, "wl_mp_select": 9, "wl_mp_residual": 10, "wl_matchingpursuit_filter": 14}
C2CTYPES = {"wl_ctx *": C.c_void_p, "void *": C.c_void_p, "const void *": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64, "double": C.c_double,
            "const double *": C.POINTER(C.c_double), "double *": C.POINTER(C.c_double), "const int *": C.POINTER(C.c_int32),
            "int64_t *": C.POINTER(C.c_int64)}
# (idx_dev is a device address on the Python side, the host outputs of wl_matchingpursuit_filter are typed pointers)
DEVICE_ADDRESSES = {("wl_findmaxabs", "idx_dev"), ("wl_mp_select", "idx_dev"), ("wl_mp_residual", "idx_dev")}


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
    for sym, arity in SYMS.items():
        proto = _prototype(sym)
        assert sym in _lib.SIGNATURES and _lib.SIGNATURES[sym][0] is C.c_int
        argtypes = _lib.SIGNATURES[sym][1]
        assert len(proto) == len(argtypes) == arity, sym
        for k, ((ctype, name), at) in enumerate(zip(proto, argtypes)):
            want = C.c_void_p if (sym, name) in DEVICE_ADDRESSES else C2CTYPES[ctype]
            assert want is at, (sym, k, name, ctype, at)
        assert proto[-1] == ("void *", "stream") and hasattr(lib, sym)
        # none of them takes a batch of units (tests/test_batch_limits_host.py goes by these parameter names)
        assert not {n for _, n in proto} & {"nunits", "nimages", "nvolumes", "ns", "nsignals"}
    for path in _lib.LIB_PATHS.values():
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert set(SYMS) <= set(re.findall(r" T (wl_[a-z0-9_]+)", out)), path
    assert lib.wl_version() == 100
    assert len(_lib.STATUS) == 14                            # no status code was added
    flat = " ".join(open(HDR).read().replace("\n *", " ").split())
    assert ("WL_EINVAL_ARG (NULL ctx / y / r / qmfs / flens / Ls / niter / nrm, nbases < 1, !(tol > 0), nmax < -1), WL_EINVAL_DTYPE, "
            "WL_EINVAL_FILTER (any flens[k]), WL_EDIMS (n < 1, nbases * n beyond 2^60), WL_EALIAS (the byte ranges of y and r overlap), "
            "then base by base what wl_dwt_filter returns") in flat
    assert "Synchronises `stream` (the norm is a host scalar" in flat and "the sign of a zero is not part of the contract" in flat
    assert '"WL_MP_MAX_BLOCKS"' in flat and "ONE 24-byte read-back" in flat


def test_a_c99_translation_unit_compiles_against_the_header(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "wavelets_mi355x.h"\n'
                   "int use(wl_ctx *c, void *y, void *r, void *sp, const double *q, const int *fl, const int *Ls, int64_t *idx, int64_t *ni,\n"
                   "        double *nrm, void *s)\n"
                   "{ return wl_findmaxabs(c, WL_F32, r, 64, idx, s) + wl_mp_select(c, WL_F32, sp, 64, y, r, 128, idx, s)\n"
                   "       + wl_mp_residual(c, WL_F64, r, y, 64, sp, 64, idx, nrm, s)\n"
                   "       + wl_matchingpursuit_filter(c, WL_F32, y, r, 64, 2, q, fl, Ls, 0.1, -1, ni, nrm, s); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


ARG, DTYPE, FILTER, EDIMS, ALIAS, EL, ESIZE = ("WL_EINVAL_ARG", "WL_EINVAL_DTYPE", "WL_EINVAL_FILTER", "WL_EDIMS", "WL_EALIAS", "WL_EINVAL_L",
                                               "WL_EINVAL_SIZE")


def test_status_codes_in_order_through_a_dummy_context(W):
    """a row breaks one rule and every later one and must return the status of the rule it names; each rule alone as well"""
    lib = W._lib.load()
    ST = W._lib.STATUS
    bufy, bufr, bufs = (C.c_double * 4096)(), (C.c_double * 4096)(), (C.c_double * 4096)()
    dummy = (C.c_char * 4096)()
    q = (C.c_double * 128)(*([0.5] * 128))
    fl, badfl = (C.c_int32 * 2)(2, 8), (C.c_int32 * 2)(2, 65)
    Ls, negL, bigL = (C.c_int32 * 2)(1, 3), (C.c_int32 * 2)(1, -1), (C.c_int32 * 2)(1, 7)
    ni, nrm, idx = C.c_int64(), C.c_double(), C.c_int64()
    named = {"CTX": C.cast(dummy, C.c_void_p), "Y": C.cast(bufy, C.c_void_p), "R": C.cast(bufr, C.c_void_p), "S": C.cast(bufs, C.c_void_p),
             "QMF": q, "FL": fl, "BADFL": badfl, "LS": Ls, "NEGL": negL, "BIGL": bigL, "NI": C.byref(ni), "NRM": C.byref(nrm),
             "IDX": C.cast(C.pointer(idx), C.c_void_p), "Y+32": C.c_void_p(C.addressof(bufy) + 32 * 4)}

    def run(sym, base, rules):
        def call(args):
            a = {**base, **args}
            return ST[getattr(lib, sym)(*[named.get(v, v) if isinstance(v, str) else v for v in a.values()], None)]
        order = [s for s, _ in rules]
        for k, (status, breakers) in enumerate(rules):
            later = {}
            for _, bs in rules[k + 1:]:
                later.update(bs[0])
            for b in breakers:
                assert call(b) == status, (sym, status, b)                       # the rule alone
                assert call({**later, **b}) == status, (sym, status, b, later)   # ... and with every later rule broken too
        return order

    mp = dict(ctx="CTX", dtype=0, y="Y", r="R", n=64, nbases=2, qmfs="QMF", flens="FL", Ls="LS", tol=0.1, nmax=-1, niter="NI", nrm="NRM")
    rules = [
        (ARG, [dict(ctx=None), dict(y=None), dict(r=None), dict(qmfs=None), dict(flens=None), dict(Ls=None), dict(niter=None), dict(nrm=None),
               dict(nbases=0), dict(tol=0.0), dict(tol=-1.0), dict(tol=float("nan")), dict(nmax=-2)]),
        (DTYPE, [dict(dtype=2), dict(dtype=-1)]),
        (FILTER, [dict(flens="BADFL")]),
        (EDIMS, [dict(n=0), dict(n=-8), dict(n=1 << 60)]),
        (ALIAS, [dict(r="Y"), dict(r="Y+32")]),
        (EL, [dict(Ls="NEGL")]),
    ]
    assert run("wl_matchingpursuit_filter", mp, rules) == [ARG, DTYPE, FILTER, EDIMS, ALIAS, EL]
    # the size rule of wl_dwt_filter, base by base: 64 has no factor 2^7
    assert ST[lib.wl_matchingpursuit_filter(named["CTX"], 0, named["Y"], named["R"], 64, 2, q, fl, bigL, 0.1, -1, C.byref(ni), C.byref(nrm),
                                            None)] == ESIZE
    # r right behind y's nbases * n elements is no overlap (the call then ends at the level rule, before it would touch the context)
    for off, want in ((2 * 64, EL), (2 * 64 - 1, ALIAS)):
        assert ST[lib.wl_matchingpursuit_filter(named["CTX"], 0, named["Y"], C.c_void_p(C.addressof(bufy) + off * 4), 64, 2, q, fl, negL, 0.1, -1,
                                                C.byref(ni), C.byref(nrm), None)] == want, off

    fm = dict(ctx="CTX", dtype=0, v="R", len=64, idx_dev="IDX")
    assert run("wl_findmaxabs", fm, [(ARG, [dict(ctx=None), dict(v=None), dict(idx_dev=None)]), (DTYPE, [dict(dtype=5)]),
                                     (EDIMS, [dict(len=0), dict(len=-3)])]) == [ARG, DTYPE, EDIMS]
    sel = dict(ctx="CTX", dtype=1, spat="S", n=64, y="Y", ftr="R", ncoef=128, idx_dev="IDX")
    assert run("wl_mp_select", sel, [(ARG, [dict(ctx=None), dict(spat=None), dict(y=None), dict(ftr=None), dict(idx_dev=None)]),
                                     (DTYPE, [dict(dtype=2)]), (EDIMS, [dict(n=0), dict(ncoef=100), dict(ncoef=0)])]) == [ARG, DTYPE, EDIMS]
    res = dict(ctx="CTX", dtype=0, r="R", aphi="Y", n=64, spat="S", spat_len=64, idx_dev="IDX", nrm="NRM")
    assert run("wl_mp_residual", res, [(ARG, [dict(ctx=None), dict(r=None), dict(nrm=None), dict(idx_dev=None)]), (DTYPE, [dict(dtype=2)]),
                                       (EDIMS, [dict(n=0), dict(spat_len=32), dict(spat_len=0)])]) == [ARG, DTYPE, EDIMS]


def test_python_argument_errors_need_no_device(W):
    import torch
    wt, sch = W.wavelet(W.WT.db4), W.wavelet(W.WT.cdf97, W.WT.Lifting)
    x = torch.zeros(64)
    for name in ("matchingpursuit", "findmaxabs"):
        assert name in W.__all__ and callable(getattr(W, name))
    # the reference's @assert nmax >= -1 and @assert tol > 0, in both forms, before anything touches a device
    ident = lambda v: v
    for args in ((wt,), ([wt, wt],), (ident, ident)):
        with pytest.raises(AssertionError):
            W.matchingpursuit(x, *args, 0.1, -2)
        for tol in (0.0, -0.5):
            with pytest.raises(AssertionError):
                W.matchingpursuit(x, *args, tol)
        with pytest.raises(AssertionError):
            W.matchingpursuit(x, *args, tol=0.1, nmax=-7)
    for bad in ("db4", None, 4, sch, [], [wt, sch], [wt, "haar"]):
        with pytest.raises(TypeError, match="matchingpursuit takes one OrthoFilter or a sequence of them"):
            W.matchingpursuit(x, bad, 0.1)
    with pytest.raises(TypeError, match="f and ft must be callables"):
        W.matchingpursuit(x, ident, 3, 0.1)
    with pytest.raises(TypeError, match="tol is required"):
        W.matchingpursuit(x, wt)
    with pytest.raises(TypeError, match="unexpected or repeated argument"):
        W.matchingpursuit(x, wt, 0.1, oop=True)
    with pytest.raises(TypeError, match="unexpected or repeated argument"):
        W.matchingpursuit(x, ident, ident, 0.1, L=2)
    for f, a in ((W.matchingpursuit, (wt, 0.1)), (W.matchingpursuit, (ident, ident, 0.1)), (W.findmaxabs, ())):
        with pytest.raises(TypeError, match=f.__name__ + " is not defined for complex arrays"):
            f(x.to(torch.complex64), *a)
        with W.complex_arrays():
            with pytest.raises(TypeError, match=f.__name__ + " is not defined for complex arrays"):
                f(x.to(torch.complex64), *a)
        with pytest.raises(TypeError, match="expected a torch tensor"):
            f(np.zeros(64), *a)
    # valid arguments get as far as the device check, here without a device: no CPU path
    if not torch.cuda.is_available():
        for call in (lambda: W.matchingpursuit(x, wt, 0.1), lambda: W.matchingpursuit(x, [wt, wt], 0.1, L=[1, 2]),
                     lambda: W.matchingpursuit(x, ident, ident, 0.1), lambda: W.findmaxabs(x)):
            with pytest.raises(W.HIPError):
                call()


def test_findmaxabs_of_the_case_builder_is_the_references_loop():
    f = MC.findmaxabs
    nan, inf = float("nan"), float("inf")
    assert f(np.array([0.0, 0.0, -0.0])) == 0 and f(np.array([3.0, -3.0, 3.0])) == 0 and f(np.array([1.0, -3.0, 3.0])) == 1
    assert f(np.array([nan, 5.0, 7.0])) == 0 and f(np.array([1.0, nan, 7.0, nan])) == 2 and f(np.array([nan, nan])) == 0
    assert f(np.array([1.0, -inf, inf])) == 1 and f(np.array([2.0], dtype=np.float32)) == 0


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_the_case_table_keeps_its_conditions(W, oracle, dtype):
    """building a reference asserts the tol margins and the ties (matchingpursuit_cases._reference); here the table itself: what it
    must cover, how each loop ended, and the identity x - f(y) = r that every case satisfies"""
    refs = {c: MC.reference(oracle, W, c, dtype) for c in MC.CASES}
    assert {c[0] for c in MC.CASES} == {2, 8, 64, 1000, 4096, 65536}
    assert {c[1] for c in MC.CASES} >= {"haar", "db4", "haar+db4", "dirac+db4", "db2+sym5+db10@L2", "mixedL"}
    assert {c[2] for c in MC.CASES} == {"gauss", "atoms", "tie"}
    assert {c[4] for c in MC.CASES} >= {0, 1, 5, -1} and all(c[0] <= 8 for c in MC.CASES if c[4] == -1 and c[3] != "above")
    assert all(c[4] == 4 for c in MC.CASES if c[0] == 65536)
    assert all(MC.levels(W, c[1], 1000) and max(MC.levels(W, c[1], 1000)) <= 3 for c in MC.CASES if c[0] == 1000)
    assert MC.levels(W, "dirac+db4", 64) == [0, 6] and MC.levels(W, "db2+sym5+db10@L2", 64) == [2, 2, 2] and len(set(MC.levels(W, "mixedL", 64))) == 3
    for c, ref in refs.items():
        n, bases, kind, tol, nmax = c
        if tol == "above":
            assert ref["niter"] == 0 and ref["ended_by_norm"] and not ref["y"].any() and np.array_equal(ref["r"], ref["x"]), c
        elif isinstance(tol, tuple):
            assert ref["niter"] == tol[1] < ref["cap"] and ref["ended_by_norm"], c          # the norm test ended it, before the cap
        elif nmax >= 0:
            assert ref["niter"] == nmax or (ref["niter"] < nmax and ref["ended_by_norm"]), c   # the cap ended it, or an exact zero residual
        if kind == "tie":
            assert ref["ties"][0] >= 2 and np.array_equal(ref["x"], np.round(ref["x"])), c
        assert np.count_nonzero(ref["y"]) <= ref["niter"]
        # x - f(y) = r up to the roundings of niter atoms
        eps = np.finfo(dtype).eps
        fy = MC.synthesis(oracle, W, bases, ref["y"])
        scale = max(1.0, float(np.abs(ref["x"]).max()))
        assert np.abs(ref["x"].astype(np.float64) - fy - ref["r"]).max() <= 64 * eps * max(1, ref["niter"]) * scale, c
    assert any(r["ended_by_norm"] and r["niter"] > 0 for r in refs.values()) and any(r["niter"] == 0 for r in refs.values())


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=MC.IDS)
def test_one_orthonormal_basis_keeps_the_largest_coefficients(W, oracle, dtype):
    """for a single orthonormal basis the atoms are orthogonal: y after m atoms holds the m largest coefficients of dwt(x), to
    1e-6 / 1e-13 x sqrt(L) relative to the largest coefficient"""
    rel = 1e-6 if dtype == np.float32 else 1e-13
    seen = 0
    for c in MC.CASES:
        n, bases, kind, tol, nmax = c
        if len(MC.BASES[bases]) != 1 or kind != "gauss":
            continue
        ref = MC.reference(oracle, W, c, dtype)
        m = ref["niter"]
        if m == 0:
            continue
        L = MC.levels(W, bases, n)[0]
        coef = MC.analysis(oracle, W, bases, ref["x"]).astype(np.float64)
        order = np.argsort(-np.abs(coef), kind="stable")[:m]
        want = np.zeros_like(coef)
        want[order] = coef[order]
        assert set(np.flatnonzero(ref["y"]).tolist()) == set(order.tolist()), c
        assert np.abs(ref["y"] - want).max() <= rel * math.sqrt(L) * np.abs(coef).max(), c
        seen += 1
    assert seen >= 4

