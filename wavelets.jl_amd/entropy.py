"""Entropy -- host-side mirror of src/Threshold/entropy.jl: the entropy measures, coefentropy and bestbasistree, the best-basis
search of a wavelet packet tree (`tree = bestbasistree(x, wt); y = wpt(x, wt, tree)`).

On a device tensor both run on the device (wl_coefentropy, wl_bestbasistree_filter; bestbasistree_batch: every column of a
len x B array in one chain of launches, the trees staying on the device for wpt_batch -- wl_bestbasistree_filter_batch); the packet content of every node is
bit-identical to wpt's, the entropies follow the accuracy contract of DESIGN.md section 11 (Float64 log and sums, deterministic).
coefentropy of a single coefficient is host arithmetic in the coefficient's type, as in the reference (entropy.jl:15-30).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from . import util as Util
from .transforms import ArgumentError, _check, _context, _dtype_code, _f64p, _prep_in, _reject_complex, _tree_arg
from .wt import OrthoFilter


# ---- entropy measures (entropy.jl:6-8) -------------------------------------------------------------
class Entropy:
    code = None

    def __repr__(self):
        return type(self).__name__ + "()"


class ShannonEntropy(Entropy):
    """Coifman-Wickerhauser: -s log s"""
    code = 0


class LogEnergyEntropy(Entropy):
    """-log s"""
    code = 1


def _et_code(et) -> int:
    if not isinstance(et, Entropy) or et.code is None:
        raise TypeError(f"et must be ShannonEntropy() or LogEnergyEntropy(), got {et!r}")
    return et.code


def _scalar_entropy(x, code, nrm):
    # coefentropy(x::T, et, nrm::T) (entropy.jl:15-30): s = (x / nrm)^2 in T, s == 0 contributes -0.0
    if isinstance(x, np.float32):
        ty = np.float32
    elif isinstance(x, (float, int, np.floating, np.integer)) and not isinstance(x, bool):
        ty = np.float64
    else:
        raise TypeError("coefentropy takes a device tensor or a real scalar")
    xv, nv = ty(x), ty(nrm)
    q = ty(xv / nv)
    s = ty(q * q)
    if s == 0:
        return ty(-0.0)
    ls = ty(np.log(s))
    return ty(-s * ls) if code == 0 else ty(-ls)


def coefentropy(x, et, nrm=None):
    """coefentropy(x, et[, nrm]) (entropy.jl:15-40).  x: a device tensor (nrm defaults to norm(x)) or a real scalar (nrm required).
    The tensor form returns a Python float holding a value of the element type."""
    _reject_complex(x, "coefentropy")
    code = _et_code(et)
    if not isinstance(x, torch.Tensor):
        if nrm is None:
            raise TypeError("coefentropy(x::Real, et, nrm): nrm is required for a scalar")
        return _scalar_entropy(x, code, nrm)
    x = _prep_in(x)
    h, st = _context(x.device)
    out = C.c_double()
    have = nrm is not None
    _check(_lib.load().wl_coefentropy(h, _dtype_code(x), C.c_void_p(x.data_ptr()), int(x.numel()), code, 1 if have else 0,
                                      float(nrm) if have else 0.0, C.byref(out), st), h)
    return out.value


def bestbasistree(y, wt, L_or_tree=None, et=ShannonEntropy(), *, return_entropy=False):
    """bestbasistree(y, wt[, L | tree][, et]) (entropy.jl:43-111): the best subtree (uint8 per node, like maketree) of the input
    tree (default and integer L: maketree(n, L, :full)).  OrthoFilter wavelets on a device vector only: GLS has no best-basis search
    in the reference (a MethodError there), matrices none either.  return_entropy=True also returns the Float64 device tensor
    [entr_bf ; entr_af] of the node entropies the decision used."""
    _reject_complex(y, "bestbasistree")
    if not isinstance(wt, OrthoFilter):
        raise TypeError("bestbasistree is defined for OrthoFilter wavelets only (the reference has no method for %s)" % type(wt).__name__)
    code = _et_code(et)
    y = _prep_in(y)
    if y.dim() != 1:
        raise TypeError("bestbasistree is defined for vectors only")
    n = int(y.numel())
    Lmax = Util.maxtransformlevels(n)
    tree = _tree_arg(n, L_or_tree)
    if not isinstance(tree, np.ndarray):
        tree = Util.maketree(n, int(tree), "full")
    out = np.zeros(len(tree), dtype=np.uint8)
    ent = None
    if return_entropy and Lmax > 0:
        ent = torch.empty(len(tree) + (1 << (Lmax - 1)), dtype=torch.float64, device=y.device)
    h, st = _context(y.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    u8 = C.POINTER(C.c_uint8)
    rc = _lib.load().wl_bestbasistree_filter(h, _dtype_code(y), C.c_void_p(y.data_ptr()), n, _f64p(q), len(q),
                                             tree.ctypes.data_as(u8), len(tree), code, out.ctypes.data_as(u8),
                                             C.cast(C.c_void_p(ent.data_ptr()), C.POINTER(C.c_double)) if ent is not None else None, st)
    _check(rc, h)
    return (out, ent) if return_entropy else out


def bestbasistree_batch(x, wt, L_or_tree=None, et=ShannonEntropy(), *, return_entropy=False):
    """bestbasistree of every column of a len x B device array (unit u = x[:, u]) in one chain of launches over all columns
    (wl_bestbasistree_filter_batch): a torch.uint8 DEVICE tensor of shape (ntree, B), column u being unit u's tree -- bit for bit
    `bestbasistree(x[:, u], wt, L_or_tree, et)` -- which wpt_batch / iwpt_batch take as their tree argument.  Nothing synchronises.
    L_or_tree: None / an integer L (maketree(n, L, :full)) or ONE host tree shared by all columns.  return_entropy=True also returns
    the Float64 device tensor (ntree + 2^(Lmax-1), B) of the node entropies [entr_bf ; entr_af] of every column."""
    _reject_complex(x, "bestbasistree_batch")
    if not isinstance(wt, OrthoFilter):
        raise TypeError("bestbasistree_batch is defined for OrthoFilter wavelets only (the reference has no method for %s)" % type(wt).__name__)
    code = _et_code(et)
    if isinstance(x, torch.Tensor) and x.dim() != 2:
        raise TypeError("bestbasistree_batch expects a len x B array (unit u = x[:, u])")
    if isinstance(x, torch.Tensor):
        tree = _tree_arg(int(x.shape[0]), L_or_tree)         # (maketree's assertion on a bad depth, before anything touches the device)
    x = _prep_in(x, maxdim=2)
    n, nb = (int(v) for v in x.shape)
    Lmax = Util.maxtransformlevels(n)
    ntree = (1 << Lmax) - 1
    if isinstance(tree, np.ndarray):
        tp, nt, L = tree.ctypes.data_as(C.POINTER(C.c_uint8)), len(tree), 0
    else:
        tp, nt, L = None, ntree, int(tree)
    # (column-major like x: column u is contiguous, ntree bytes from column u - 1)
    out = torch.empty((nb, ntree), dtype=torch.uint8, device=x.device).t()
    ent = None
    nent = ntree + (1 << (Lmax - 1)) if Lmax > 0 else 0
    if return_entropy:
        ent = torch.empty((nb, nent), dtype=torch.float64, device=x.device).t()
    h, st = _context(x.device)
    q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
    rc = _lib.load().wl_bestbasistree_filter_batch(h, _dtype_code(x), C.c_void_p(x.data_ptr()), n, nb, n, _f64p(q), len(q), tp, nt, L, code,
                                                   C.c_void_p(out.data_ptr()), ntree,
                                                   C.c_void_p(ent.data_ptr()) if ent is not None and nent else None, nent, st)
    _check(rc, h)
    return (out, ent) if return_entropy else out
