"""Pursuit -- host-side mirror of src/Threshold/basis_functions.jl: matchingpursuit and findmaxabs.

    y = matchingpursuit(x, [wavelet(WT.haar), wavelet(WT.db4)], 0.1)        # a union of orthonormal wavelet bases, on the device
    y = matchingpursuit(x, f, ft, 0.1)                                      # the reference's generic form, f / ft on device tensors

The loop (basis_functions.jl:8-44), with T the element type:

    r = x;  y = zeros(T, N);  it = 0;  cap = (nmax == -1 ? N : nmax)
    while nrm(r) > tol && it < cap
        ftr = ft(r);  i = findmaxabs(ftr);  aphi = f(ftr[i] e_i);  r = T(r - aphi);  y[i] = T(y[i] + ftr[i]);  it += 1

Everything but nrm(r) is the reference bit for bit; the norm follows DESIGN.md section 11 (Float64 sum of squares in a fixed
order, rounded to T: about 1 ulp of T from BLAS nrm2) and only gates termination.  The host reads one norm back per atom.
The reference's `oop` / `N` arguments (out-of-place f / ft with caller-provided buffers) are not mirrored: f and ft return tensors.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import util as Util
from .transforms import _check, _context, _dtype_code, _f64p, _i32p, _prep_in, _reject_complex
from .wt import OrthoFilter


def _vector(x, fname: str) -> torch.Tensor:
    x = _prep_in(x)
    if x.dim() != 1:
        raise TypeError(f"{fname} is defined for vectors only")
    return x


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _findmaxabs_dev(v: torch.Tensor, idx: torch.Tensor):
    """idx[0] = findmaxabs(v), on the device (wl_findmaxabs: enqueues only)"""
    h, st = _context(v.device)
    _check(_lib.load().wl_findmaxabs(h, _dtype_code(v), _vp(v), int(v.numel()), _vp(idx), st), h)


def _select_dev(spat: torch.Tensor, y: torch.Tensor, ftr: torch.Tensor, idx: torch.Tensor):
    """spat[i % len(spat)] = ftr[i]; y[i] += ftr[i] with i = idx[0] (wl_mp_select: enqueues only)"""
    h, st = _context(y.device)
    _check(_lib.load().wl_mp_select(h, _dtype_code(y), _vp(spat), int(spat.numel()), _vp(y), _vp(ftr), int(y.numel()), _vp(idx), st), h)


def _residual_dev(r: torch.Tensor, aphi=None, spat=None, idx=None) -> float:
    """r -= aphi (when given), the spike of spat cleared (when given), nrm(r) returned (wl_mp_residual: synchronises the stream)"""
    h, st = _context(r.device)
    out = C.c_double()
    _check(_lib.load().wl_mp_residual(h, _dtype_code(r), _vp(r), _vp(aphi), int(r.numel()), _vp(spat), int(spat.numel()) if spat is not None else 0,
                                      _vp(idx) if spat is not None else None, C.byref(out), st), h)
    return out.value


def findmaxabs(v) -> int:
    """findmaxabs(v) (basis_functions.jl:45-55) of a device vector as a 0-based Python int: the first index whose magnitude is
    strictly greater than every earlier one (v[0] NaN gives 0, a NaN elsewhere never wins, ties keep the first)."""
    _reject_complex(v, "findmaxabs")
    v = _vector(v, "findmaxabs")
    if v.numel() < 1:
        raise ValueError("findmaxabs of an empty vector")
    idx = torch.zeros(1, dtype=torch.int64, device=v.device)
    _findmaxabs_dev(v, idx)
    return int(idx.item())


def _residual_buffer(x: torch.Tensor, residual) -> torch.Tensor:
    """the vector the loop works on: a copy of x, in `residual` when the caller gave one"""
    if residual is None:
        return x.clone()
    if not isinstance(residual, torch.Tensor):
        raise TypeError("residual must be a torch tensor")
    if residual.dtype != x.dtype or residual.device != x.device or tuple(residual.shape) != tuple(x.shape) or not residual.is_contiguous():
        raise TypeError("residual must be a contiguous tensor of x's shape, element type and device")
    residual.copy_(x)
    return residual


def _bases(wts):
    ws = [wts] if isinstance(wts, OrthoFilter) else (list(wts) if isinstance(wts, (list, tuple)) else None)
    if not ws or not all(isinstance(w, OrthoFilter) for w in ws):
        raise TypeError("matchingpursuit takes one OrthoFilter or a sequence of them, or the callables f and ft "
                        "(lifting schemes run through the generic form)")
    return ws


def _levels(L, nbases: int, n: int):
    if L is None:
        return [Util.maxtransformlevels(n)] * nbases
    if isinstance(L, (int, np.integer)) and not isinstance(L, bool):
        return [int(L)] * nbases
    Ls = [int(v) for v in L]
    if len(Ls) != nbases:
        raise ValueError("L must be one integer or one per base")
    return Ls


def _pursuit_filter(x, wts, tol, nmax, L, residual, info):
    ws = _bases(wts)
    assert nmax >= -1
    assert tol > 0
    x = _vector(x, "matchingpursuit")
    n = int(x.numel())
    Ls = _levels(L, len(ws), n)
    r = _residual_buffer(x, residual)
    y = torch.empty(len(ws) * n, dtype=x.dtype, device=x.device)
    q = np.ascontiguousarray(np.concatenate([np.asarray(w.qmf, dtype=np.float64) for w in ws]))
    fl = np.array([len(w.qmf) for w in ws], dtype=np.int32)
    la = np.array(Ls, dtype=np.int32)
    niter, nrm = C.c_int64(), C.c_double()
    h, st = _context(x.device)
    _check(_lib.load().wl_matchingpursuit_filter(h, _dtype_code(x), _vp(y), _vp(r), n, len(ws), _f64p(q), _i32p(fl), _i32p(la), float(tol), int(nmax),
                                                 C.byref(niter), C.byref(nrm), st), h)
    return (y, niter.value, nrm.value) if info else y


def _pursuit_generic(x, f, ft, tol, nmax, residual, info):
    if not callable(f) or not callable(ft):
        raise TypeError("matchingpursuit(x, f, ft, tol): f and ft must be callables on device tensors")
    assert nmax >= -1
    assert tol > 0
    x = _vector(x, "matchingpursuit")
    m = int(x.numel())
    r = _residual_buffer(x, residual)

    def coefficients(v):
        c = ft(v)
        if not isinstance(c, torch.Tensor) or c.dim() != 1 or c.dtype != x.dtype or c.device != x.device or c.numel() < 1:
            raise TypeError("ft must return a non-empty device vector of x's element type")
        return c.contiguous()

    ftr = coefficients(r)                                   # (length(ft(x)) sizes y, basis_functions.jl:15; reused by the first atom)
    N = int(ftr.numel())
    y = torch.zeros(N, dtype=x.dtype, device=x.device)
    spat = torch.zeros(N, dtype=x.dtype, device=x.device)
    idx = torch.zeros(1, dtype=torch.int64, device=x.device)
    cap = N if nmax == -1 else int(nmax)
    nrm = _residual_dev(r)
    it = 0
    while nrm > tol and it < cap:
        if it > 0:
            ftr = coefficients(r)
            if int(ftr.numel()) != N:
                raise TypeError("ft changed the length of its result")
        _findmaxabs_dev(ftr, idx)
        _select_dev(spat, y, ftr, idx)
        aphi = f(spat)
        if not isinstance(aphi, torch.Tensor) or aphi.dtype != x.dtype or aphi.device != x.device or tuple(aphi.shape) != (m,):
            raise TypeError("f must return a device vector of x's length and element type")
        aphi = aphi.contiguous()
        if N == m:
            nrm = _residual_dev(r, aphi, spat, idx)
        else:                                               # (wl_mp_residual clears a spike in a vector of r's length only)
            nrm = _residual_dev(r, aphi)
            spat.index_fill_(0, idx, 0)
        it += 1
    return (y, it, nrm) if info else y


def matchingpursuit(x, *args, **kw):
    """matchingpursuit(x, wts, tol, nmax=-1, L=None, residual=None, info=False)
    matchingpursuit(x, f, ft, tol, nmax=-1, residual=None, info=False)            (basis_functions.jl:8-44)

    Greedy pursuit of a device vector x: a sparse y with ||x - f(y)|| <= tol approximately, one atom per iteration, at most nmax
    atoms (-1: len(y)).

    * wts: one OrthoFilter or a sequence of K of them -- the dictionary is the union of the K orthonormal wavelet bases, y has
      K n coefficients, block k being in the basis of dwt(., wts[k], L[k]) (L: one int or one per base, default
      maxtransformlevels(n); L = 0 is the Dirac basis).  The whole loop runs in the library (wl_matchingpursuit_filter).
    * f, ft: callables on device tensors (f: N coefficients -> signal, ft: its transpose), e.g. a dense dictionary through
      torch.mv, or lifting transforms.  The same loop in Python over wl_findmaxabs / wl_mp_select / wl_mp_residual.  The
      reference's `oop` / `N` arguments are not mirrored.

    x is never modified (the reference's `r = x` overwrites it; here the loop works on a copy).  residual=: a tensor that receives
    the final residual.  info=True: returns (y, niter, nrm).  nmax < -1 and tol <= 0 raise AssertionError, as the reference's
    @assert.  Float32 / Float64 vectors only; there is no CPU path."""
    _reject_complex(x, "matchingpursuit")
    if not args:
        raise TypeError("matchingpursuit(x, wts, tol, ...) or matchingpursuit(x, f, ft, tol, ...)")
    generic = callable(args[0]) and not isinstance(args[0], OrthoFilter)
    names = ("f", "ft", "tol", "nmax") if generic else ("wts", "tol", "nmax", "L")
    if len(args) > len(names):
        raise TypeError("matchingpursuit: too many positional arguments")
    a = dict(zip(names, args))
    for k, v in kw.items():
        if k not in names + ("residual", "info") or k in a:
            raise TypeError(f"matchingpursuit: unexpected or repeated argument {k!r}")
        a[k] = v
    if "tol" not in a or (generic and "ft" not in a):
        raise TypeError("matchingpursuit: tol is required" if "tol" not in a else "matchingpursuit(x, f, ft, tol): ft is required")
    nmax, residual, info = a.get("nmax", -1), a.get("residual"), bool(a.get("info", False))
    if generic:
        return _pursuit_generic(x, a["f"], a["ft"], a["tol"], nmax, residual, info)
    return _pursuit_filter(x, a["wts"], a["tol"], nmax, a.get("L"), residual, info)
