"""Threshold -- host-side mirror of src/Threshold/threshold_main.jl (threshold!/threshold, the THType
singletons) and src/Threshold/denoising.jl (VisuShrink, denoise, noisest, mad!), the main in-package
caller of the transform path.  Julia's `f!` is spelled `f_`.

Everything runs on the device through libwavelets_mi355x.so (wl_threshold, wl_threshold_biggest,
wl_threshold_batch, wl_threshold_biggest_batch, wl_mad, wl_circshift, wl_arrayadd, wl_rmul + the
dwt/idwt entry points); the only host scalars are
the ones the reference also has on the host (the noise estimate sigma and the threshold t).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from . import util as Util
from . import wt as WT
from .transforms import (ArgumentError, DimensionMismatch, HIPError, _check, _check_pair, _context, _dims, _dtype_code, _prep_in, _reject_complex, _i32p, _f64p,
                         dwt, dwt_oop_, idwt, idwt_, idwt_oop_, is_julia_layout, julia_layout, similar)
from .wt import GLS, OrthoFilter, wavelet


# ---- threshold types (threshold_main.jl:8-17) --------------------------------------------------
class THType:
    code = None

    def __repr__(self):
        return type(self).__name__ + "()"


class HardTH(THType):
    code = 0


class SoftTH(THType):
    code = 1


class SemiSoftTH(THType):
    code = 2


class SteinTH(THType):
    code = 3


class PosTH(THType):
    code = 4


class NegTH(THType):
    code = 5


class BiggestTH(THType):
    code = -1


DEFAULT_TH = HardTH()


def _dev_array(x) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise HIPError("expected a torch tensor resident on an MI355X device (use to_device(array)); there is no CPU path")
    _dtype_code(x)
    if not (x.is_contiguous() or is_julia_layout(x)):
        raise ArgumentError("array must be dense (Julia layout or C-contiguous)")
    return x


def _t_is_f64(x: torch.Tensor, t) -> int:
    """the type Julia's promotion computes `x[i] op t` in: Float64 for a Python float / np.float64 threshold,
    the element type for integers and for thresholds that already have the element type"""
    if isinstance(t, (bool, int, np.integer)):
        return 0
    if isinstance(t, np.floating):
        return 0 if (t.dtype == np.float32 and x.dtype == torch.float32) else 1
    return 1


def threshold_(x, TH: THType, t=None):
    """threshold!(x, TH, t) / threshold!(x, BiggestTH(), m) / threshold!(x, PosTH()|NegTH()) -- in place"""
    _reject_complex(x, "threshold_")
    x = _dev_array(x)
    lib = _lib.load()
    h, st = _context(x.device)
    n = int(x.numel())
    if isinstance(TH, BiggestTH):
        if t is None or int(t) != t:
            raise TypeError("threshold!(x, BiggestTH(), m::Int)")
        if int(t) < 0:
            raise AssertionError("m >= 0")
        _check(lib.wl_threshold_biggest(h, _dtype_code(x), C.c_void_p(x.data_ptr()), n, int(t), st), h)
        return x
    if isinstance(TH, (PosTH, NegTH)):
        if t is not None:
            raise TypeError("threshold!(x, PosTH()/NegTH()) takes no threshold (MethodError in the reference)")
        _check(lib.wl_threshold(h, _dtype_code(x), C.c_void_p(x.data_ptr()), n, TH.code, 0.0, 0, st), h)
        return x
    if not isinstance(TH, THType) or TH.code is None:
        raise TypeError("unknown threshold type")
    if t is None:
        raise TypeError("threshold!(x, TH, t): t is required (MethodError in the reference)")
    if not float(t) >= 0:
        raise AssertionError("t >= 0")
    _check(lib.wl_threshold(h, _dtype_code(x), C.c_void_p(x.data_ptr()), n, TH.code, float(t), _t_is_f64(x, t), st), h)
    return x


def threshold(x, TH: THType, t=None):
    """threshold(x, TH[, t]): the non-in-place form (threshold_main.jl:120-127)"""
    _reject_complex(x, "threshold")
    x = _dev_array(x)
    y = similar(x)
    y.copy_(x)
    return threshold_(y, TH, t)


# ---- threshold! of a batch: per-unit thresholds and the best m-term approximation on the device ----------
def _batch_units(x: torch.Tensor):
    """(n, B, unit_stride) of a tensor whose last dimension is the batch, or None when its layout is not a batch of column-major
    units a fixed number of elements apart"""
    nb = int(x.shape[-1])
    unit = tuple(int(s) for s in x.shape[:-1])
    n = int(np.prod(unit)) if unit else 1
    if n > 1 and not is_julia_layout(x[..., 0]):
        return None
    us = int(x.stride(-1)) if nb > 1 else n
    return (n, nb, us) if us >= n else None


def threshold_batch_(x, TH: THType, t=None):
    """threshold!(x[.., u], TH, t_u) for every unit of a batch, in place, in one call (wl_threshold_batch /
    wl_threshold_biggest_batch): x is column-major with the batch as its last dimension, a unit is everything in front of it (any
    shape); units may be padded apart (the stride of the last dimension), the padding is never touched.
    t: a Python number -- one threshold for all units, int versus float choosing the arithmetic type as in threshold_ -- or a 1-D
    device tensor of B entries, one per unit: Float64 for HardTH / SoftTH / SemiSoftTH / SteinTH (a Float32 tensor with Float32
    data: the arithmetic stays in Float32), Int64 for BiggestTH (the m of the best m-term approximation; entries are clamped to
    [0, n] on the device).  Host numbers are validated as threshold_ does; device entries are not (no synchronisation): a negative
    or NaN threshold yields what the reference's arithmetic yields without its assertion.  Same bits as the loop of threshold_ over
    the units; nothing synchronises, a captured graph may hold the call."""
    _reject_complex(x, "threshold_batch_")
    if not isinstance(TH, THType) or TH.code is None:
        raise TypeError("unknown threshold type")
    big = isinstance(TH, BiggestTH)
    tens = isinstance(t, torch.Tensor)
    if big:
        if t is None or (tens and t.dtype != torch.int64) or (not tens and int(t) != t):
            raise TypeError("threshold!(x, BiggestTH(), m::Int): m is an integer or an Int64 tensor of one m per unit")
        if not tens and int(t) < 0:
            raise AssertionError("m >= 0")
    elif isinstance(TH, (PosTH, NegTH)):
        if t is not None:
            raise TypeError("threshold!(x, PosTH()/NegTH()) takes no threshold (MethodError in the reference)")
    else:
        if t is None:
            raise TypeError("threshold!(x, TH, t): t is required (MethodError in the reference)")
        if tens and t.dtype not in (torch.float64, torch.float32):
            raise TypeError("per-unit thresholds are a Float64 tensor (Float32 with Float32 data)")
        if not tens and not float(t) >= 0:
            raise AssertionError("t >= 0")
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise HIPError("expected a torch tensor resident on an MI355X device (use to_device(array)); there is no CPU path")
    _dtype_code(x)
    if x.dim() < 1 or int(x.numel()) == 0:
        raise DimensionMismatch("threshold_batch_ expects a non-empty array whose last dimension is the batch")
    lay = _batch_units(x)
    if lay is None:
        raise ArgumentError("threshold_batch_ works in place: units must be column-major and a fixed stride >= their length apart")
    n, nb, us = lay
    tdev, is64 = None, 1
    if tens:
        if t.device != x.device or t.dim() != 1 or int(t.numel()) != nb:
            raise ArgumentError("the per-unit tensor must be 1-D with B entries on x's device")
        if t.dtype == torch.float32:
            if x.dtype != torch.float32:
                raise TypeError("Float32 thresholds go with Float32 data")
            tdev, is64 = t.to(torch.float64), 0
        else:
            tdev = t.contiguous()
    lib = _lib.load()
    h, st = _context(x.device)
    if big:
        rc = lib.wl_threshold_biggest_batch(h, _dtype_code(x), C.c_void_p(x.data_ptr()), n, nb, us, 0 if tens else int(t),
                                            C.c_void_p(tdev.data_ptr()) if tens else None, st)
    else:
        tv = 0.0 if (tens or t is None) else float(t)
        if not tens and t is not None:
            is64 = _t_is_f64(x, t)
        rc = lib.wl_threshold_batch(h, _dtype_code(x), C.c_void_p(x.data_ptr()), n, nb, us, TH.code, tv,
                                    C.c_void_p(tdev.data_ptr()) if tens else None, is64, st)
    _check(rc, h)
    return x


def threshold_batch(x, TH: THType, t=None):
    """threshold_batch_ on a dense column-major copy of x"""
    _reject_complex(x, "threshold_batch")
    if isinstance(x, torch.Tensor) and x.device.type == "cuda" and x.dim() >= 1:
        y = similar(x)
        y.copy_(x)
        x = y
    return threshold_batch_(x, TH, t)


# ---- denoising (denoising.jl) -------------------------------------------------------------------
class DNFT:
    pass


class VisuShrink(DNFT):
    """VisuShrink(th, t) / VisuShrink(n): t = sqrt(2*log(n)) for noise level sigma = 1"""

    def __init__(self, *args):
        if len(args) == 1:
            self.th, self.t = DEFAULT_TH, math.sqrt(2 * math.log(int(args[0])))
        elif len(args) == 2:
            self.th, self.t = args[0], float(args[1])
        else:
            raise TypeError("VisuShrink(th, t) or VisuShrink(n)")


DEFAULT_WAVELET = wavelet(WT.sym5, WT.Filter)
_DEFAULT = object()


def mad_(y) -> float:
    """mad!(y): median absolute deviation; y is overwritten by abs.(y .- median(y)) (denoising.jl:103-110)"""
    _reject_complex(y, "mad_")
    y = _dev_array(y)
    h, st = _context(y.device)
    out = C.c_double()
    _check(_lib.load().wl_mad(h, _dtype_code(y), C.c_void_p(y.data_ptr()), int(y.numel()), C.byref(out), st), h)
    return out.value


def median(v) -> float:
    _reject_complex(v, "median")
    v = _dev_array(v)
    h, st = _context(v.device)
    out = C.c_double()
    vv = v if v.is_contiguous() else julia_layout(v)
    _check(_lib.load().wl_median(h, _dtype_code(vv), C.c_void_p(vv.data_ptr()), int(vv.numel()), C.byref(out), st), h)
    return out.value


def noisest(x, wt=_DEFAULT, L: int = 1) -> float:
    """noisest(x, wt=DEFAULT_WAVELET, L=1) (denoising.jl:92-101): MAD of the level-L detail range / 0.6745.
    `y[detailrange(y, L)]` is linear indexing with size(y, 1), as in the reference."""
    _reject_complex(x, "noisest")
    wt = DEFAULT_WAVELET if wt is _DEFAULT else wt
    x = _prep_in(x)
    y = x if wt is None else dwt(x, wt, L)
    n1 = int(y.shape[0])
    r = Util.detailrange(n1, L)            # round(Int, n/2^L + 1) : round(Int, n/2^(L-1)), ties to even (non_dyadic.jl:7)
    flat = y.t().reshape(-1) if y.dim() == 2 else (y.permute(2, 1, 0).reshape(-1) if y.dim() == 3 else y)
    dr = flat[r.start - 1:r.stop - 1].clone()
    return mad_(dr) / 0.6745


def nspin2circ(nspin, i: int):
    """shift vector of spin number i (1-based), first dimension fastest (denoising.jl:112-121)"""
    nsp = (int(nspin),) if not hasattr(nspin, "__len__") else tuple(int(s) for s in nspin)
    rem, c = int(i) - 1, []
    for d in nsp:
        c.append(rem % d)
        rem //= d
    return c


def circshift(a, shift) -> torch.Tensor:
    """b[i] = a[i - shift] along every dimension (Util.circshift! / Base.circshift)"""
    a = _prep_in(a)
    sh = [int(shift)] if not hasattr(shift, "__len__") else [int(s) for s in shift]
    if len(sh) > a.dim():
        raise DimensionMismatch("more shifts than dimensions")
    sh = sh + [0] * (3 - len(sh))
    b = similar(a)
    h, st = _context(a.device)
    _check(_lib.load().wl_circshift(h, _dtype_code(a), C.c_void_p(b.data_ptr()), C.c_void_p(a.data_ptr()), a.dim(),
                                    _dims(a), (C.c_int64 * 3)(*sh), st), h)
    return b


def _arrayadd_(y, z):
    if y.numel() != z.numel():
        raise DimensionMismatch("lengths must be equal")
    h, st = _context(y.device)
    _check(_lib.load().wl_arrayadd(h, _dtype_code(y), C.c_void_p(y.data_ptr()), C.c_void_p(z.data_ptr()), int(y.numel()), st), h)
    return y


def _rmul_(y, s: float):
    h, st = _context(y.device)
    _check(_lib.load().wl_rmul(h, _dtype_code(y), C.c_void_p(y.data_ptr()), int(y.numel()), float(s), st), h)
    return y


def denoise(x, wt=_DEFAULT, L: Optional[int] = None, dnt: Optional[DNFT] = None, estnoise=noisest, TI: bool = False,
            nspin: Union[int, Sequence[int], None] = None) -> torch.Tensor:
    """denoise(x, wt=DEFAULT_WAVELET; L=min(maxtransformlevels(x),6), dnt=VisuShrink(size(x,1)), estnoise=noisest,
    TI=false, nspin=8 per dimension) -- denoising.jl:21-81.  wt=None is the reference's `nothing`."""
    _reject_complex(x, "denoise")
    wt = DEFAULT_WAVELET if wt is _DEFAULT else wt
    x = _prep_in(x)
    L = min(Util.maxtransformlevels(x), 6) if L is None else int(L)
    dnt = VisuShrink(int(x.shape[0])) if dnt is None else dnt
    nspin = tuple(8 for _ in range(x.dim())) if nspin is None else nspin
    if not Util.iscube(x):
        raise ArgumentError("array must be square/cube")
    nsp = (int(nspin),) if not hasattr(nspin, "__len__") else tuple(int(s) for s in nspin)
    # fast path only where it is the reference's own branch: threshold!(xt, th, t) exists for Hard / Soft / Semisoft / Stein
    # (codes 0..3; Pos / Neg take no t and raise in the loop below exactly as the reference's MethodError does); matrices need
    # one nspin entry per dimension (anything else goes through nspin2circ / circshift in the loop below, as in the reference)
    # The plain (not translation-invariant) denoise of an orthogonal filter takes the same device-resident call with ONE spin
    # of shift zero: y = (0 + idwt(threshold!(dwt(x)))) * 1 -- the same bits (a -0.0 may come back as +0.0), and the noise
    # estimate never leaves the device (the reference's order needs sigma on the host between noisest and threshold!).
    one_spin = (not TI) and estnoise is noisest and wt is not None
    if one_spin:
        nsp = tuple(1 for _ in range(x.dim()))
    if ((TI or one_spin) and isinstance(wt, OrthoFilter) and (x.dim() == 1 or (x.dim() == 2 and len(nsp) == 2) or (x.dim() == 3 and len(nsp) == 3))
            and isinstance(dnt.th, THType) and dnt.th.code is not None and 0 <= dnt.th.code <= 3):
        # the translation-invariant branch for orthogonal filters, vectors, square matrices and cubes: one device-resident batch
        # (wl_denoise_ti_filter) -- all spins transformed / thresholded / inverted together, the noise estimate consumed on
        # the device, nothing allocated per spin, no host synchronisation.  Same arithmetic in the same order as the loop below.
        sig = -1.0 if estnoise is noisest else float(estnoise(x, wt))
        if estnoise is not noisest and not (sig >= 0 and sig * float(dnt.t) >= 0):
            raise AssertionError("t >= 0")               # (@assert t >= 0 in threshold!, threshold_main.jl:24, t = sigma * dnt.t: NaN
            #                                              fails it, +Inf passes -- everything is thresholded -- as in the reference)
        y = similar(x)
        h, st = _context(x.device)
        q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
        # vectors: prod(nspin) spins shifted by 0 .. pns-1 whatever nspin's length (denoising.jl:38-42)
        nsl = [int(np.prod(nsp))] if x.dim() == 1 else list(nsp)
        nsv = (C.c_int64 * 3)(*(nsl + [1] * (3 - len(nsl))))
        rc = _lib.load().wl_denoise_ti_filter(h, _dtype_code(x), C.c_void_p(y.data_ptr()), C.c_void_p(x.data_ptr()), x.dim(), _dims(x),
                                              q.ctypes.data_as(C.POINTER(C.c_double)), len(q), int(L), dnt.th.code, float(dnt.t), nsv,
                                              sig, st)
        if _lib.STATUS.get(rc) != "WL_ENOMEM":
            _check(rc, h)
            return y
        # (no room for the batch's workspace -- about ws + 2 N prod(nspin) elements, 5.5 N for one spin: the reference's own
        #  sequence below runs the same device kernels one spin at a time and needs only the transform's two buffers)
    if (TI and isinstance(wt, GLS) and (x.dim() == 1 or (x.dim() == 2 and len(nsp) == 2) or (x.dim() == 3 and len(nsp) == 3))
            and isinstance(dnt.th, THType) and dnt.th.code is not None and 0 <= dnt.th.code <= 3):
        # the same device-resident batch for a lifting scheme (wl_denoise_ti_lifting, round 4): shifted signals as one
        # batched-lines transform, shifted images one batched 2-D and shifted cubes one batched 3-D lifting transform per group of
        # spins; sigma never leaves the device
        sig = -1.0 if estnoise is noisest else float(estnoise(x, wt))
        if estnoise is not noisest and not (sig >= 0 and sig * float(dnt.t) >= 0):
            raise AssertionError("t >= 0")
        y = similar(x)
        h, st = _context(x.device)
        iu, nc, sh, cf = wt.flatten()
        nsl = [int(np.prod(nsp))] if x.dim() == 1 else list(nsp)
        nsv = (C.c_int64 * 3)(*(nsl + [1] * (3 - len(nsl))))
        rc = _lib.load().wl_denoise_ti_lifting(h, _dtype_code(x), C.c_void_p(y.data_ptr()), C.c_void_p(x.data_ptr()), x.dim(), _dims(x),
                                               len(iu), _i32p(iu), _i32p(nc), _i32p(sh), _f64p(cf), wt.norm1, wt.norm2,
                                               int(L), dnt.th.code, float(dnt.t), nsv, sig, st)
        if _lib.STATUS.get(rc) != "WL_ENOMEM":
            _check(rc, h)
            return y
        # (as above: the per-spin loop below needs far less memory than the batch)
    sigma = estnoise(x, wt)
    t = sigma * dnt.t
    if TI:
        if wt is None:
            raise RuntimeError("TI not supported with wt=nothing")
        pns = int(np.prod(nsp))
        y = similar(x)
        y.zero_()
        xt = similar(x)
        for i in range(1, pns + 1):
            shift = [i - 1] if x.dim() == 1 else nspin2circ(nsp, i)      # (denoising.jl:40-42 / :52-53)
            z = circshift(x, shift)
            dwt_oop_(xt, z, wt, L)
            threshold_(xt, dnt.th, t)
            idwt_oop_(z, xt, wt, L)
            _arrayadd_(y, circshift(z, [-s for s in shift]))
        return _rmul_(y, 1 / pns)
    if wt is None:
        y = similar(x)
        y.copy_(x)
        return threshold_(y, dnt.th, t)
    y = dwt(x, wt, L)
    threshold_(y, dnt.th, t)
    if isinstance(wt, GLS):
        return idwt_(y, wt, L)
    return idwt(y, wt, L)


# ---- a batch of independent units: per-unit noise estimates and thresholds on the device ------------
def mad_batch_(y) -> torch.Tensor:
    """mad!(y[:, i]) for every column of an n x B matrix (column-major) in one launch (wl_mad_batch): a Float64 device tensor of B
    values; y is overwritten by the absolute deviations of its columns.  No host synchronisation."""
    _reject_complex(y, "mad_batch_")
    y = _dev_array(y)
    if y.dim() != 2 or not is_julia_layout(y):
        raise ArgumentError("mad_batch_ expects a dense column-major n x B matrix")
    n, nb = int(y.shape[0]), int(y.shape[1])
    out = torch.empty(nb, dtype=torch.float64, device=y.device)
    h, st = _context(y.device)
    _check(_lib.load().wl_mad_batch(h, _dtype_code(y), C.c_void_p(y.data_ptr()), n, nb, n, C.cast(C.c_void_p(out.data_ptr()), _lib._f64p), st), h)
    return out


def _batch_unit_shape(x, what: str):
    """(unit shape, B) of a len x B / n x n x B / n x n x n x B batch; the reference's own errors for what a unit may be"""
    if not isinstance(x, torch.Tensor):
        raise TypeError("expected a torch tensor resident on an MI355X device (use to_device(array)); there is no CPU path")
    if x.dim() not in (2, 3, 4):
        raise DimensionMismatch(what + " expects a len x B matrix (signals), an n x n x B array (images) or an n x n x n x B array (cubes)")
    unit = tuple(int(s) for s in x.shape[:-1])
    if any(s != unit[0] for s in unit):
        raise ArgumentError("array must be square/cube")               # iscube(x) (denoising.jl:29)
    return unit, int(x.shape[-1])


def _batch_transform(x, wt, L):
    from .transforms import dwtc, dwt_batch
    return dwtc(x, wt, L) if x.dim() == 2 else dwt_batch(x, wt, L)


def noisest_batch(x, wt=_DEFAULT, L: int = 1) -> torch.Tensor:
    """noisest(x[.., i], wt, L) for every unit of a batch (x: len x B, n x n x B or n x n x n x B): a Float64 device tensor of B
    sigmas.  One batched transform, the detail range of every unit's first column gathered into an nd x B matrix, one wl_mad_batch,
    one division by 0.6745 -- nothing synchronises with the host."""
    _reject_complex(x, "noisest_batch")
    wt = DEFAULT_WAVELET if wt is _DEFAULT else wt
    if wt is not None and not isinstance(wt, (OrthoFilter, GLS)):
        raise TypeError("wt must be an OrthoFilter, a GLS or None")
    _batch_unit_shape(x, "noisest_batch")
    x = _prep_in(x, maxdim=4)
    y = x if wt is None else _batch_transform(x, wt, int(L))
    r = Util.detailrange(int(y.shape[0]), int(L))
    first = y[(slice(r.start - 1, r.stop - 1),) + (0,) * (y.dim() - 2) + (slice(None),)]
    dr = similar(first)
    dr.copy_(first)
    return mad_batch_(dr) / 0.6745


def denoise_batch(x, wt=_DEFAULT, L: Optional[int] = None, dnt: Optional[DNFT] = None, sigma=None, y=None, return_sigma: bool = False):
    """denoise(x[.., i], wt; L, dnt) of every unit of a batch in one call: x is len x B (signals), n x n x B (square images) or
    n x n x n x B (cubes), column-major.  Defaults as denoise: L = min(maxtransformlevels(unit), 6), dnt = VisuShrink(size(x, 1)).
    Every unit gets its OWN sigma = noisest(unit, wt) and threshold, estimated and applied on the device (wl_denoise_batch_filter /
    wl_denoise_batch_lifting): the same bits as the loop of denoise over the units, without its per-unit launches.
    sigma: per-unit noise levels instead of the estimate -- a host sequence / array (validated: every entry >= 0, else
    AssertionError; uploaded) or a Float64 device tensor of B values (not validated).  y: the output (lifting schemes: may be x).
    return_sigma: also return the Float64 device tensor of the B sigmas used.
    Not part of this call (TypeError): wt=None, BiggestTH / PosTH / NegTH, and the TI keyword: translation-invariant denoising of a
    batch is denoise_ti_batch."""
    return _denoise_units("denoise_batch", x, wt, L, dnt, sigma, y, return_sigma)


def denoise_ti_batch(x, wt=_DEFAULT, L: Optional[int] = None, dnt: Optional[DNFT] = None, nspin: Union[int, Sequence[int], None] = None,
                     sigma=None, y=None, return_sigma: bool = False):
    """denoise(x[.., i], wt; L, dnt, TI=true, nspin) of every unit of a batch in one call (wl_denoise_ti_batch_filter /
    wl_denoise_ti_batch_lifting): x, L, dnt, sigma, y and return_sigma as denoise_batch, except that y must not be x.  Every unit gets
    its OWN sigma = noisest(unit, wt), estimated from the unshifted unit on the device; the shifted copies of all units are transformed,
    thresholded and inverted as batches, un-shifted and summed in spin order: the same bits as the loop of denoise(unit, wt, TI=True)
    over the units, without its per-unit launches.
    nspin: 8 per unit dimension by default; for signals an int or any tuple, whose product is the number of spins (shifts 0 .. prod - 1);
    for images and cubes one entry per unit dimension (ArgumentError otherwise).
    Not part of this call (TypeError): wt=None, BiggestTH / PosTH / NegTH."""
    return _denoise_units("denoise_ti_batch", x, wt, L, dnt, sigma, y, return_sigma, ti=True, nspin=nspin)


def _denoise_units(what, x, wt, L, dnt, sigma, y, return_sigma, ti=False, nspin=None):
    """the body denoise_batch and denoise_ti_batch (ti: with nspin) share: validation before any device call, then one ABI call"""
    _reject_complex(x, what)
    wt = DEFAULT_WAVELET if wt is _DEFAULT else wt
    if not isinstance(wt, (OrthoFilter, GLS)):
        raise TypeError(what + " is defined for orthogonal filters and lifting schemes (wt=None is not part of it)")
    unit, nb = _batch_unit_shape(x, what)
    L = min(Util.maxtransformlevels(unit[0]), 6) if L is None else int(L)
    dnt = VisuShrink(int(x.shape[0])) if dnt is None else dnt
    if not isinstance(dnt, DNFT) or not isinstance(dnt.th, THType) or dnt.th.code is None or not 0 <= dnt.th.code <= 3:
        raise TypeError(what + " thresholds with HardTH, SoftTH, SemiSoftTH or SteinTH (threshold!(x, TH, t)); "
                        "BiggestTH / PosTH / NegTH are not part of it")
    if not float(dnt.t) >= 0:
        raise AssertionError("t >= 0")
    spins = []
    if ti:
        nspin = tuple(8 for _ in unit) if nspin is None else nspin
        nsp = (int(nspin),) if not hasattr(nspin, "__len__") else tuple(int(s) for s in nspin)
        if len(unit) == 1:
            nsp = (int(np.prod(nsp)),)                       # vectors: prod(nspin) spins shifted by 0 .. pns-1 (denoising.jl:38-42)
        if len(nsp) != len(unit):
            raise ArgumentError("nspin must have one entry per unit dimension")
        if any(s < 1 for s in nsp):
            raise ArgumentError("nspin must be positive")
        spins = [(C.c_int64 * 3)(*(list(nsp) + [1] * (3 - len(nsp))))]
    sig_host = None
    if sigma is not None and not isinstance(sigma, torch.Tensor):
        sig_host = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).reshape(-1))
        if sig_host.size != nb:
            raise DimensionMismatch("sigma must have one entry per unit")
        if not bool(np.all(sig_host >= 0)):
            raise AssertionError("t >= 0")                   # (@assert t >= 0 in threshold!, t = sigma * dnt.t: NaN fails it too)
    x = _prep_in(x, maxdim=4)
    y = similar(x) if y is None else y
    _check_pair(y, x)
    if sigma is not None:
        sig_dev = torch.from_numpy(sig_host).to(x.device) if sig_host is not None else sigma
        if sig_dev.device != x.device or sig_dev.dtype != torch.float64 or sig_dev.numel() != nb or not sig_dev.is_contiguous():
            raise ArgumentError("sigma must be a contiguous Float64 tensor of B values on x's device")
    else:
        sig_dev = None
    sig_out = torch.empty(nb, dtype=torch.float64, device=x.device) if return_sigma else None
    f64 = lambda t: C.cast(C.c_void_p(t.data_ptr()), _lib._f64p) if t is not None else None
    lib = _lib.load()
    h, st = _context(x.device)
    dims = (C.c_int64 * 3)(*(list(unit) + [1] * (3 - len(unit))))
    nunit = int(np.prod(unit))
    tail = spins + [f64(sig_dev), f64(sig_out), st]          # (the translation-invariant entry points take nspin in front of the sigmas)
    if isinstance(wt, GLS):
        iu, nc, sh, cf = wt.flatten()
        fn = lib.wl_denoise_ti_batch_lifting if ti else lib.wl_denoise_batch_lifting
        rc = fn(h, _dtype_code(x), C.c_void_p(y.data_ptr()), C.c_void_p(x.data_ptr()), len(unit), dims, nb, nunit,
                len(iu), _i32p(iu), _i32p(nc), _i32p(sh), _f64p(cf), wt.norm1, wt.norm2, L, dnt.th.code, float(dnt.t), *tail)
    else:
        q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
        fn = lib.wl_denoise_ti_batch_filter if ti else lib.wl_denoise_batch_filter
        rc = fn(h, _dtype_code(x), C.c_void_p(y.data_ptr()), C.c_void_p(x.data_ptr()), len(unit), dims, nb, nunit,
                _f64p(q), len(q), L, dnt.th.code, float(dnt.t), *tail)
    _check(rc, h)
    return (y, sig_out) if return_sigma else y
