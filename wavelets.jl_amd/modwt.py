"""Maximal-overlap DWT -- host-side mirror of src/Transforms/transforms_maximal_overlap.jl
(modwt :47-63, imodwt :99-107) and maxmodwttransformlevels (src/Util/non_dyadic.jl:24-25).

`modwt(x, wt, L)` returns the n x (L+1) coefficient matrix as a column-major device tensor (each
level's coefficients are one contiguous column; the scaling coefficients are the last column),
`imodwt(xw, wt)` inverts it; `modwt_batch` / `imodwt_batch` do the same for every column of a len x B panel in one call;
`modwt_mra` / `modwt_mra_batch` turn coefficients into the multiresolution analysis (details D_1 .. D_L and smooth S_L).  The
compute is libwavelets_mi355x.so (wl_modwt / wl_imodwt / wl_modwt_batch / wl_imodwt_batch / wl_modwt_mra_batch); there is
no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from .transforms import (ArgumentError, DimensionMismatch, HIPError, _check, _context, _dtype_code, _f64p, _prep_in, _reject_complex,
                         julia_layout)
from .wt import OrthoFilter


def maxmodwttransformlevels(x) -> int:
    """floor(Int, log2(length(x))) -- length of an array, or the integer itself"""
    n = int(x.numel()) if isinstance(x, torch.Tensor) else (int(np.asarray(x).size) if hasattr(x, "__len__") else int(x))
    if n < 1:
        raise ArgumentError("maxmodwttransformlevels of an empty array (DomainError in the reference)")
    return int(_lib.load().wl_maxmodwttransformlevels(n))


def modwt(x, wt: OrthoFilter, L: Optional[int] = None) -> torch.Tensor:
    """modwt(x::AbstractVector, wt::OrthoFilter, L=maxmodwttransformlevels(x)) -> n x (L+1)"""
    _reject_complex(x, "modwt")
    if not isinstance(wt, OrthoFilter):
        raise TypeError("modwt is defined for OrthoFilter wavelets only (MethodError in the reference)")
    x = _prep_in(x)
    if x.dim() != 1:
        raise TypeError("modwt expects a vector (MethodError in the reference)")
    n = int(x.numel())
    if n < 1:
        raise ArgumentError("modwt of an empty vector")
    L = maxmodwttransformlevels(n) if L is None else int(L)
    if L > maxmodwttransformlevels(n):
        raise ArgumentError("Too many transform levels (length(x) < 2^L)")
    if L < 1:
        raise ArgumentError("L must be >= 1")
    out = torch.empty((L + 1, n), dtype=x.dtype, device=x.device).t()       # column-major n x (L+1)
    h, st = _context(x.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    rc = _lib.load().wl_modwt(h, _dtype_code(x), C.c_void_p(out.data_ptr()), n, C.c_void_p(x.data_ptr()), n,
                              _f64p(q), len(q), L, st)
    _check(rc, h)
    return out


def imodwt(xw, wt: OrthoFilter) -> torch.Tensor:
    """imodwt(xw::Matrix, wt::OrthoFilter): inverse of modwt(x, wt, size(xw, 2) - 1)"""
    _reject_complex(xw, "imodwt")
    if not isinstance(wt, OrthoFilter):
        raise TypeError("imodwt is defined for OrthoFilter wavelets only (MethodError in the reference)")
    if not isinstance(xw, torch.Tensor) or xw.device.type != "cuda":
        raise HIPError("expected a torch tensor resident on an MI355X device; there is no CPU path")
    if xw.dim() != 2:
        raise TypeError("imodwt expects a matrix (MethodError in the reference)")
    xw = julia_layout(xw)
    n, ncols = int(xw.shape[0]), int(xw.shape[1])
    if n < 1 or ncols < 1:
        raise DimensionMismatch("empty coefficient matrix")
    x = torch.empty(n, dtype=xw.dtype, device=xw.device)
    h, st = _context(xw.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    rc = _lib.load().wl_imodwt(h, _dtype_code(xw), C.c_void_p(x.data_ptr()), C.c_void_p(xw.data_ptr()), n, n, ncols,
                               _f64p(q), len(q), st)
    _check(rc, h)
    return x


# ---- a panel of vectors in one call (wl_modwt_batch / wl_imodwt_batch) ---------------------------------
def _batch_in(x) -> torch.Tensor:
    """what _prep_in checks, without its copy into the dense layout: the batch calls take strides"""
    if not isinstance(x, torch.Tensor):
        raise TypeError("expected a torch tensor resident on an MI355X device (use to_device(array)); there is no CPU path")
    if x.device.type != "cuda":
        raise HIPError("tensor is not on a HIP device; there is no CPU path")
    if not x.dtype.is_floating_point:
        x = x.to(torch.float64)            # Int -> Float, as the single calls do
    _dtype_code(x)
    return x


def _panel_strides(x: torch.Tensor):
    """(x, unit_stride) of a len x B panel: x itself when its columns are contiguous and unit_stride elements apart, else its
    dense column-major copy"""
    n, nb = int(x.shape[0]), int(x.shape[1])
    if (n == 1 or x.stride(0) == 1) and (nb == 1 or x.stride(1) >= n):
        return x, (int(x.stride(1)) if nb > 1 else n)
    return julia_layout(x), n


def _coef_strides(w: torch.Tensor):
    """(ld, unit_stride) of an n x ncols x B coefficient tensor when its layout is expressible that way, else None"""
    n, nc, nb = (int(v) for v in w.shape)
    if n > 1 and w.stride(0) != 1:
        return None
    ld = int(w.stride(1)) if nc > 1 else n
    us = int(w.stride(2)) if nb > 1 else ld * nc
    return (ld, us) if ld >= n and us >= ld * nc else None


def modwt_batch(x, wt: OrthoFilter, L: Optional[int] = None, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """modwt of every column of a len x B panel in one call: the n x (L+1) x B tensor whose [:, :, u] is modwt(x[:, u], wt, L), bit
    for bit.  Columns that are contiguous and a fixed number of elements apart (a padded or sliced panel) are taken in place; any
    other layout is copied once.  y: an n x (L+1) x B result tensor, dense or padded (stride 1 along the first dimension)."""
    _reject_complex(x, "modwt_batch")
    _reject_complex(y, "modwt_batch")
    if not isinstance(wt, OrthoFilter):
        raise TypeError("modwt_batch is defined for OrthoFilter wavelets only (MethodError in the reference)")
    if isinstance(x, torch.Tensor):                          # (the shape and level rules before anything touches the device)
        if x.dim() != 2:
            raise TypeError("modwt_batch expects a len x B array (unit i = x[:, i])")
        n, nb = int(x.shape[0]), int(x.shape[1])
        if n < 1 or nb < 1:
            raise ArgumentError("modwt_batch of an empty panel")
        L = maxmodwttransformlevels(n) if L is None else int(L)
        if L > maxmodwttransformlevels(n):
            raise ArgumentError("Too many transform levels (length(x) < 2^L)")
        if L < 1:
            raise ArgumentError("L must be >= 1")
    x = _batch_in(x)
    x, xs = _panel_strides(x)
    if y is None:
        y = torch.empty((nb, L + 1, n), dtype=x.dtype, device=x.device).permute(2, 1, 0)        # column-major n x (L+1) x B
    else:
        y = _batch_in(y)
        if tuple(y.shape) != (n, L + 1, nb):
            raise DimensionMismatch(f"modwt_batch: y must have shape (n, L + 1, B) = {(n, L + 1, nb)}, got {tuple(y.shape)}")
        if y.dtype != x.dtype or y.device != x.device:
            raise TypeError("x and y must have the same element type and device")
        if _coef_strides(y) is None:
            raise ArgumentError("modwt_batch: y must be column-major (stride 1 along n, columns >= n apart, units >= ld * (L + 1) apart)")
    ldo, ous = _coef_strides(y)
    h, st = _context(x.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    rc = _lib.load().wl_modwt_batch(h, _dtype_code(x), C.c_void_p(y.data_ptr()), ldo, ous, C.c_void_p(x.data_ptr()), n, nb, xs,
                                    _f64p(q), len(q), L, st)
    _check(rc, h)
    return y


def imodwt_batch(xw, wt: OrthoFilter) -> torch.Tensor:
    """imodwt of every n x ncols slice xw[:, :, u] in one call: the n x B panel whose column u is imodwt(xw[:, :, u], wt), bit for
    bit.  A padded column-major xw (what modwt_batch fills) is taken in place."""
    _reject_complex(xw, "imodwt_batch")
    if not isinstance(wt, OrthoFilter):
        raise TypeError("imodwt_batch is defined for OrthoFilter wavelets only (MethodError in the reference)")
    if isinstance(xw, torch.Tensor):
        if xw.dim() != 3:
            raise TypeError("imodwt_batch expects an n x ncols x B array (unit i = xw[:, :, i])")
        if min(int(v) for v in xw.shape) < 1:
            raise DimensionMismatch("empty coefficient array")
    xw = _batch_in(xw)
    if _coef_strides(xw) is None:
        xw = julia_layout(xw)
    ldw, ws = _coef_strides(xw)
    n, ncols, nb = (int(v) for v in xw.shape)
    x = torch.empty((nb, n), dtype=xw.dtype, device=xw.device).t()                               # column-major n x B
    h, st = _context(xw.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    rc = _lib.load().wl_imodwt_batch(h, _dtype_code(xw), C.c_void_p(x.data_ptr()), n, C.c_void_p(xw.data_ptr()), ldw, ws, n, ncols, nb,
                                     _f64p(q), len(q), st)
    _check(rc, h)
    return x


# ---- multiresolution analysis (wl_modwt_mra_batch) --------------------------------------------------------
def _mra(name, xw, wt, y, dim, what):
    _reject_complex(xw, name)
    _reject_complex(y, name)
    if not isinstance(wt, OrthoFilter):
        raise TypeError(name + " is defined for OrthoFilter wavelets only (MethodError in the reference)")
    if isinstance(xw, torch.Tensor):                         # (the shape rules before anything touches the device)
        if xw.dim() != dim:
            raise TypeError(f"{name} expects {what}")
        if min(int(v) for v in xw.shape) < 1:
            raise DimensionMismatch("empty coefficient array")
    xw = _batch_in(xw)
    if dim == 2:                                             # one matrix: a batch of one unit
        xw = xw.unsqueeze(2)
    if _coef_strides(xw) is None:
        xw = julia_layout(xw)
    ldw, ws = _coef_strides(xw)
    n, ncols, nb = (int(v) for v in xw.shape)
    if y is None:
        y = torch.empty((nb, ncols, n), dtype=xw.dtype, device=xw.device).permute(2, 1, 0)      # column-major n x ncols x B
    else:
        y = _batch_in(y)
        if tuple(y.shape) != (n, ncols, nb):
            raise DimensionMismatch(f"{name}: y must have the shape of xw, {(n, ncols, nb)}, got {tuple(y.shape)}")
        if y.dtype != xw.dtype or y.device != xw.device:
            raise TypeError("xw and y must have the same element type and device")
        if _coef_strides(y) is None:
            raise ArgumentError(name + ": y must be column-major (stride 1 along n, columns >= n apart, units >= ld * ncols apart)")
    ldo, ous = _coef_strides(y)
    h, st = _context(xw.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    rc = _lib.load().wl_modwt_mra_batch(h, _dtype_code(xw), C.c_void_p(y.data_ptr()), ldo, ous, C.c_void_p(xw.data_ptr()), ldw, ws, n, ncols, nb,
                                        _f64p(q), len(q), st)
    _check(rc, h)
    return y[:, :, 0] if dim == 2 else y


def modwt_mra_batch(xw, wt: OrthoFilter, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MODWT multiresolution analysis of every n x ncols slice xw[:, :, u] (what modwt_batch returns) in one call: the n x ncols x B
    tensor whose [:, c, u] is imodwt of xw[:, :, u] with every column but c set to zero -- the details D_1 .. D_L in columns
    0 .. L-1 and the smooth S_L in column L = ncols - 1, aligned with x and adding up to it.  Equal (==) to that loop for finite
    input.  A padded column-major xw is taken in place, any other layout is copied once.  y: an n x ncols x B result tensor,
    dense or padded (stride 1 along the first dimension), not overlapping xw."""
    return _mra("modwt_mra_batch", xw, wt, y, 3, "an n x ncols x B array (unit i = xw[:, :, i])")


def modwt_mra(xw, wt: OrthoFilter) -> torch.Tensor:
    """MODWT multiresolution analysis of one n x ncols coefficient matrix (what modwt returns): n x ncols, columns D_1 .. D_L, S_L --
    modwt_mra_batch of a batch of one"""
    return _mra("modwt_mra", xw, wt, None, 2, "a matrix (MethodError in the reference)")
