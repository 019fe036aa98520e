"""Subnormals, overflow, NaN, Inf and signed zeros through every transform tier (tests/special_values_cases.py: the input classes, one
recipe per kernel name that W.last_kernel() can report, the comparison).

Per recipe and element type, with the recipe's options set once: every class forward on the class input and inverse on the oracle's
forward output (`zeros`: on the zeros input itself, at the recipe's depth Lz), W.last_kernel() is the recipe's kernel, and the result
equals the oracle's: NaN masks equal, everything else bit for bit, signs of zeros included (SV.mismatch).  A kernel whose result
differs from the oracle's in the sign of zeros alone is recorded; only an inverse (or modwt_mra) call of a kernel in
SV.ZERO_SIGN_FREE is let off, and the last test holds the record against that table.

A second pass runs `straddle` and `zeros` with W.set_kernel_path(1): the generic kernels back every fallback.

The fused library (W.set_arithmetic("fused")) promises less (DESIGN.md "Special values"), on the same recipes:
    nan_corner, nan_last, inf_pair   NaN masks equal; outside them the Inf values equal and the finite values within the bounds of
                                     test_gpu_fused.py (Float32: relative L2 <= 1e-6 sqrt(L) and max |d| <= 1e-5 max(1, |ref|_inf);
                                     Float64: relative L2 <= 1e-13 sqrt(L)), against the oracle of the same element type
    zeros                            forward calls of the filter recipes at one level: as the exact library with zero_sign = False, bit
                                     for bit (every chain there is a single non-zero product).  The inverse calls (an approximation
                                     and a detail term meet in one chain), the lifting recipes (an update step sums two non-zero
                                     neighbours) and the deeper recipes (level 2 works on a blob): a zero is a zero of either sign and
                                     a non-zero a non-zero within the bounds above -- a sum of two non-zero products rounds once
                                     instead of twice, and a few results per case are one unit in the last place off
    deep                             every recipe, at its depth Lz (1 unless its kernels are multi-level ones; modwt: its own L):
                                     |got - want| <= B q, q the smallest subnormal.
        B, derived from the chain and not from any run: in the subnormal range every rounding moves a value by at most q / 2.  One
        pass computes an output from R roundings in the exact library (a filter of F taps: F products and F - 1 sums; a lifting
        scheme: two per coefficient and one per step and two for the normalisation) and from no more in the fused one, so the two
        differ by at most R q after the pass -- q / 2 each, R roundings on either side.  A later pass multiplies what it is handed by
        at most its gain G (a filter: sum |taps|; a scheme: the product over its steps of 1 + sum |coefficients|, times the larger
        normalisation factor; modwt: both filters, 4 F - 1 roundings, taps / sqrt 2).  P = d Lz passes (d transformed dimensions;
        inverse passes have the same taps; a coefficient that leaves the chain earlier has met fewer): B = R (1 + G + ... + G^(P-1)).
        The largest B here is below 2^19; a tier that flushes misses by about tiny = 2^23 q (Float32) or 2^52 q.
`overflow` and `straddle` are not run on the fused library: one rounding in place of two moves an overflow and a rounding boundary.
"""
import math

import numpy as np
import pytest

import special_values_cases as SV

pytestmark = pytest.mark.gpu

CASES = SV.recipe_cases()
ZERO_SIGN_DIFFERED = {}          # kernel name -> did any zero of its results differ in sign from the oracle's, in any class
RAN = set()                      # ids of the exact-library cases that ran to their end (the bookkeeping test needs all of them)


def _dev(W, a):
    return W.to_device(np.array(a))


def _host(W, t):
    import torch
    torch.cuda.synchronize()
    return W.to_host(t)


def _calls(r, ref):
    e = SV.ENTRIES[r.entry]
    x, fwd, inv_in, inv, dir_in, dir_out = ref
    out = [("fwd", x, fwd, e.fwd_gpu, r.kfwd)]
    if e.inv_gpu is not None:
        out.append(("inv", inv_in, inv, e.inv_gpu, r.kinv))
        if dir_in is not None:           # (inf_pair: the Inf planted in the approximation band, SV.direct_inverse_input)
            out.append(("inv_direct", dir_in, dir_out, e.inv_gpu, r.kinv))
    return out


def run_exact(W, oracle, r, dtype, classes, pin=True):
    """-> the list of what went wrong for one recipe and element type on the exact library (empty: nothing)"""
    bad = []
    for wname in r.wavelets:
        wt = SV.wavelet(W, r.entry, wname)
        for cls in classes:
            if (r.name, cls) in SV.SKIPS:
                continue
            L = SV.depth(r, cls)
            for tag, src, want, fn, kexp in _calls(r, SV.reference(oracle, W, r, dtype, wname, cls)):
                got = _host(W, fn(W, wt, _dev(W, src), L))
                k = W.last_kernel()
                where = (wname, cls, tag, k)
                if pin and kexp is not None and k != kexp:
                    bad.append(where + ("ran on another kernel than %s" % kexp,))
                m = SV.mismatch(got, want, True)
                if m is None:
                    ZERO_SIGN_DIFFERED.setdefault(k, False)
                elif SV.mismatch(got, want, False) is None:
                    ZERO_SIGN_DIFFERED[k] = True
                    if k not in SV.ZERO_SIGN_FREE or not (tag.startswith("inv") or SV.ENTRIES[r.entry].synthesis):
                        bad.append(where + ("signs of zeros: " + m,))
                else:
                    ZERO_SIGN_DIFFERED.setdefault(k, False)
                    bad.append(where + (SV.mismatch(got, want, False),))
    return bad


@pytest.mark.parametrize("rd", CASES, ids=SV.case_id)
def test_every_class_on_the_recipes_kernel(gpu, W, oracle, rd):
    r, dtype = rd
    with W.options(**r.opts):
        bad = run_exact(W, oracle, r, dtype, tuple(SV.CLASSES))
    assert not bad, bad
    RAN.add(SV.case_id(rd))


@pytest.mark.parametrize("rd", CASES, ids=SV.case_id)
def test_generic_kernels(gpu, W, oracle, rd):
    r, dtype = rd
    try:
        W.set_kernel_path(1)
        with W.options(**r.opts):
            bad = run_exact(W, oracle, r, dtype, SV.GENERIC_CLASSES, pin=False)
    finally:
        W.set_kernel_path(0)
    assert not bad, bad
    RAN.add("generic-" + SV.case_id(rd))


# ---- the fused library -----------------------------------------------------------------------------------------------------------
def _fused_finite(got, want, L):
    """the bounds of test_gpu_fused.py on the finite values (None: met)"""
    fin = np.isfinite(want)
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    if w.size == 0:
        return None
    nw = np.linalg.norm(w)
    rel = np.linalg.norm(g - w) / nw if nw > 0 else float(np.abs(g - w).max())
    if want.dtype == np.float64:
        return None if rel <= 1e-13 * math.sqrt(max(L, 1)) else "relative L2 %.3g" % rel
    if rel > 1e-6 * math.sqrt(max(L, 1)):
        return "relative L2 %.3g" % rel
    d = float(np.abs(g - w).max())
    return None if d <= 1e-5 * max(1.0, float(np.abs(w).max())) else "max |d| %.3g" % d


def _fused_nonfinite(got, want, L):
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return "NaN masks differ at %d places" % int((gn != wn).sum())
    if not (np.array_equal(got == np.inf, want == np.inf) and np.array_equal(got == -np.inf, want == -np.inf)):
        return "Inf values differ"
    return _fused_finite(got, want, L)


def _fused_zeros(got, want, L, bitwise):
    if bitwise:
        return SV.mismatch(got, want, False)
    if not np.isfinite(got).all() or not np.array_equal(got == 0, want == 0):
        return "%d zeros became non-zero or the other way round" % int(((got == 0) != (want == 0)).sum())
    return _fused_finite(got, want, L)


def deep_bound(r, wt, L):
    """B of the docstring for a transform of depth L, in units of the smallest subnormal"""
    e = SV.ENTRIES[r.entry]
    if e.lifting:
        iu, nc, sh, cf = wt.flatten()
        R, G, at = 2 + len(nc), max(abs(wt.norm1), abs(wt.norm2)), 0
        for n in nc:
            R += 2 * int(n)
            G *= 1 + float(np.abs(cf[at:at + int(n)]).sum())
            at += int(n)
    elif r.entry.startswith("modwt"):    # (imodwt and the analysis sum both filters: 2 F products, 2 F - 1 sums; taps / sqrt 2)
        R, G = 4 * len(wt.qmf) - 1, float(np.abs(wt.qmf).sum()) / math.sqrt(2)
    else:
        R, G = 2 * len(wt.qmf) - 1, float(np.abs(wt.qmf).sum())
    d = {"dwt": len(r.shape), "dwt_lifting": len(r.shape), "dwtc": 1, "wpt": 1, "wpt_lifting": 1, "dwt_batch": len(r.shape) - 1,
         "dwt_batch_lifting": len(r.shape) - 1, "modwt": 1, "modwt_batch": 1, "modwt_mra": 1}[r.entry]
    return R * sum(G ** p for p in range(d * L))


def run_fused(W, oracle, r, dtype):
    """-> the list of what went wrong for one recipe and element type on the fused library (the caller has selected it)"""
    bad = []
    q = float(np.finfo(dtype).smallest_subnormal)
    assert W.get_arithmetic() == "fused"
    with W.options(**r.opts):
        for wname in r.wavelets:
            wt = SV.wavelet(W, r.entry, wname)
            for cls in SV.FUSED_CLASSES:
                if (r.name, cls) in SV.SKIPS:
                    continue
                L = r.Lz if cls == "deep" else SV.depth(r, cls)
                for tag, src, want, fn, kexp in _calls(r, SV.reference(oracle, W, r, dtype, wname, cls, L)):
                    got = _host(W, fn(W, wt, _dev(W, src), L))
                    k = W.last_kernel()
                    if cls == "deep":
                        B = deep_bound(r, wt, L)
                        assert B < 2 ** 19, (r.name, wname, B)
                        d = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) / q
                        m = None if (np.isfinite(got).all() and d <= B) else "off by %.4g q, bound %.4g q" % (d, B)
                    elif cls == "zeros":
                        m = _fused_zeros(got, want, L, bitwise=(tag == "fwd" and L == 1 and not SV.ENTRIES[r.entry].lifting))
                    else:
                        m = _fused_nonfinite(got, want, L)
                    if m is not None:
                        bad.append((wname, cls, tag, k, m))
    return bad


@pytest.fixture(scope="module")
def fused(gpu, W):
    """the fused library for the tests that ask for it, once (a switch retires every context of the library being left)"""
    W.set_arithmetic("fused")
    yield W
    W.set_arithmetic("exact")


@pytest.mark.parametrize("rd", CASES, ids=SV.case_id)
def test_fused_library(fused, oracle, rd):
    bad = run_fused(fused, oracle, *rd)
    assert not bad, bad


# ---- the signs of zeros, tier by tier --------------------------------------------------------------------------------------------
def test_zero_sign_table_is_exact():
    """In the manner of a strict expected failure: every kernel of SV.ZERO_SIGN_FREE did give a zero of another sign than the oracle's
    somewhere (the table keeps no tier that has become exact), and no other kernel did."""
    want = {SV.case_id(rd) for rd in CASES}
    want |= {"generic-" + c for c in want}
    if not want <= RAN:
        pytest.skip("needs the whole module: %d of %d cases ran to their end" % (len(RAN & want), len(want)))
    differed = {k for k, v in ZERO_SIGN_DIFFERED.items() if v}
    assert differed == set(SV.ZERO_SIGN_FREE), {"differed but not in the table": sorted(differed - set(SV.ZERO_SIGN_FREE)),
                                                "in the table but exact": sorted(set(SV.ZERO_SIGN_FREE) - differed)}
