"""Special values through every transform tier: the shared inputs, recipes and comparison of test_special_values_host.py (CPU) and
test_gpu_special_values.py (GPU).  Plain data and numpy; the library and the oracle are handed in by the callers.

INPUT CLASSES (CLASSES; each a function of (shape, dtype, seed) built from conftest.rng_array's normals) and what the oracle's
output must contain for a (recipe, class) pair to test anything (CONDITIONS, checked on the CPU per recipe and element type):

    straddle    normals * 4 tiny (a power of two: exact)       >= 5 % non-zero subnormals and >= 5 % normal values
    deep        normals * tiny / 64                            every non-zero output subnormal, < 50 % exact zeros
    overflow    unit normals, two clusters of +-2^(maxexp-1)   >= 1 Inf, >= 1 NaN, >= 50 % finite (every input finite)
    nan_corner  normals, NaN at index (0, ..., 0)              0 < NaN count < 50 %
    nan_last    normals, NaN at the last index (wraps)         as above
    inf_pair    normals, +Inf at n/4 and -Inf at 3n/4          >= 1 +Inf and >= 1 -Inf (NaN allowed)
    zeros       zeros with coin-flip signs, the upper half of  >= 25 % exact zeros; under haar, forward, zeros of both signs
                every axis all -0.0, three non-zero samples

overflow: one pass of an orthonormal filter has sum |taps| < 2, so entries of 2^(maxexp-1) cannot overflow in it: the first Inf needs
two passes over a same-sign cluster (haar: three), the first Inf - Inf one more.  A 2-D or 3-D recipe therefore runs L = 2 and a 1-D
one L = 4 where its tier allows it; the recipes with fewer passes and the modwt recipes (taps / sqrt 2) are in SKIPS.  The lifting
schemes overflow in their first predict step.  An inverse call whose input is the forward output turns every Inf into NaN (taps of
both signs meet it), so for that call `overflow` and `inf_pair` ask for a non-finite value only, and `inf_pair` has a second inverse
call on an input that keeps its Inf values (direct_inverse_input), held to the full condition; the NaN classes' condition is
taken at L = 1, where it is stated; `zeros` runs at the recipe's Lz, the smallest depth at which the named kernels run.

RECIPES: one row per kernel name that the transform entry points report through W.last_kernel(): the entry point, the options that
force the tier (copied from the per-tier tests of test_gpu_parity.py, test_gpu_lifting_schemes.py, test_gpu_modwt_batch.py,
test_gpu_batch3d.py, test_gpu_lifting_batch3.py; a composite name such as "k_lift_axis_stream+lines" is a tier's name like any other), the smallest shape of those tests at which the tier runs, the depth, the wavelets, and the kernel the forward
and the inverse call must report (None: that direction is compared but its tier is another row's).  The forward name is the kernel
of level 1, the inverse name the kernel of level 1 too (the last one launched).

ELSEWHERE: kernel names whose special values are tested by the test named there.  NOT_KERNELS: literals of the same spelling in the
sources that are no kernel name.  ZERO_SIGN_FREE: the kernels whose zero results may carry either sign (DESIGN.md "Special values").
"""
from collections import namedtuple

import numpy as np

from conftest import rng_array

F32, F64 = "float32", "float64"
BOTH = (F32, F64)


# ---- input classes ---------------------------------------------------------------------------------------------------------------
def _tiny(dtype):
    return np.finfo(dtype).tiny


def straddle(shape, dtype, seed):
    return rng_array(shape, dtype, seed) * np.dtype(dtype).type(4 * _tiny(dtype))


def deep(shape, dtype, seed):
    return rng_array(shape, dtype, seed) * np.dtype(dtype).type(_tiny(dtype) / 64)


def _cluster(shape, num, den):
    """the slices of a cluster of 2 .. 32 entries per axis (a power of two, at most a quarter of the axis; one entry on an axis shorter
    than 8: the units of a batch) that starts near num / den of every axis, on a multiple of its edge"""
    out = []
    for s in shape:
        e = 1 << (min(32, s // 4).bit_length() - 1) if s >= 8 else 1
        lo = min((s * num // den) // e * e, s - e)
        out.append(slice(lo, lo + e))
    return tuple(out)


def overflow(shape, dtype, seed):
    x = rng_array(shape, dtype, seed)
    big = np.dtype(dtype).type(2.0) ** (np.finfo(dtype).maxexp - 1)
    x[_cluster(shape, 1, 4)] = big
    x[_cluster(shape, 5, 8)] = -big
    assert np.isfinite(x).all()
    return x


def nan_corner(shape, dtype, seed):
    x = rng_array(shape, dtype, seed)
    x[(0,) * len(shape)] = np.nan
    return x


def nan_last(shape, dtype, seed):
    x = rng_array(shape, dtype, seed)
    x[tuple(s - 1 for s in shape)] = np.nan
    return x


def inf_pair(shape, dtype, seed):
    x = rng_array(shape, dtype, seed)
    x[tuple(s // 4 for s in shape)] = np.inf
    x[tuple(3 * s // 4 for s in shape)] = -np.inf
    return x


def zeros(shape, dtype, seed):
    r = np.random.default_rng(seed)
    x = np.where(r.random(shape) < 0.5, -0.0, 0.0).astype(dtype)
    x[tuple(slice(s // 2, None) for s in shape)] = -0.0
    x[tuple(s // 4 for s in shape)] = 1.5
    x[tuple(max(s // 2 - 1, 0) for s in shape)] = -0.75
    x[tuple(3 * s // 4 for s in shape)] = 2.25                   # inside the -0.0 block
    return x


CLASSES = {"straddle": straddle, "deep": deep, "overflow": overflow, "nan_corner": nan_corner, "nan_last": nan_last,
           "inf_pair": inf_pair, "zeros": zeros}
FUSED_CLASSES = ("nan_corner", "nan_last", "inf_pair", "zeros", "deep")      # (deep: at the recipe's depth Lz)
GENERIC_CLASSES = ("straddle", "zeros")


def _counts(out):
    a = np.abs(out)
    fin = np.isfinite(out)
    return {"n": out.size, "nan": int(np.isnan(out).sum()), "pinf": int((out == np.inf).sum()), "ninf": int((out == -np.inf).sum()),
            "zero": int((out == 0).sum()), "negzero": int(((out == 0) & np.signbit(out)).sum()),
            "sub": int((fin & (a > 0) & (a < _tiny(out.dtype))).sum()), "normal": int((fin & (a >= _tiny(out.dtype))).sum()),
            "finite": int(fin.sum())}


def condition(cls, out, forward, haar, direct=False):
    """None where the oracle's output `out` has what class `cls` is there for, else what is missing.  An inverse call whose input is
    the forward output meets every Inf of it with taps of both signs, and what comes out is NaN (on a small array with a long filter,
    everywhere): there `overflow` and `inf_pair` ask for a non-finite value, the Inf itself being in the input (the forward
    condition), and a second inverse input (direct: direct_inverse_input) is held to the class's full condition.  `forward` is false for the synthesis of modwt_mra as well: no chain of an up-sampling pass ends in -0."""
    c = _counts(out)
    n = c["n"]
    if not forward and not direct and cls in ("overflow", "inf_pair"):
        return None if c["n"] - c["finite"] >= 1 else c
    if cls == "straddle":
        ok = c["sub"] >= 0.05 * n and c["normal"] >= 0.05 * n
    elif cls == "deep":
        ok = c["normal"] == 0 and c["finite"] == n and c["zero"] < 0.5 * n
    elif cls == "overflow":
        ok = c["pinf"] + c["ninf"] >= 1 and c["nan"] >= 1 and c["finite"] >= 0.5 * n
    elif cls in ("nan_corner", "nan_last"):
        ok = 0 < c["nan"] < 0.5 * n
    elif cls == "inf_pair":
        ok = c["pinf"] >= 1 and c["ninf"] >= 1
    else:
        ok = c["zero"] >= 0.25 * n and (not (forward and haar) or 0 < c["negzero"] < c["zero"])
    return None if ok else c


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def mismatch(got, want, zero_sign=True):
    """None, or what differs: the NaN masks must be equal, and everything outside them bit for bit -- infinities, subnormals and
    (zero_sign) the signs of zeros.  Without zero_sign a zero may have either sign, but it must be a zero.  NaN payloads and NaN
    signs are never compared (the host's and the GPU's default NaN differ)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape / dtype %s %s against %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        bad = np.argwhere(gn != wn)
        return "NaN masks differ at %d places (got %d NaN, want %d), first %s" % (len(bad), int(gn.sum()), int(wn.sum()), bad[0].tolist())
    diff = (bits(got) != bits(want)) & ~wn
    if not zero_sign:
        diff &= ~((got == 0) & (want == 0))
    if diff.any():
        bad = np.argwhere(diff)
        i = tuple(bad[0])
        return "%d values differ, first at %s: got %r (0x%x), want %r (0x%x)" % (len(bad), list(i), got[i], int(bits(got)[i]), want[i],
                                                                               int(bits(want)[i]))
    return None


def compare(got, want, zero_sign=True):
    m = mismatch(got, want, zero_sign)
    assert m is None, m


# ---- entry points ----------------------------------------------------------------------------------------------------------------
# fwd_ref / inv_ref: the oracle on host arrays; fwd_gpu / inv_gpu: the library on device tensors.  The batch entries hold their units
# on the last axis, and the oracle takes them one by one.
def _units(fn, a):
    return np.stack([fn(np.ascontiguousarray(a[..., u])) for u in range(a.shape[-1])], axis=-1)


def _tree(W, n, L):
    return W.maketree(n, L, "full")


def _mra_unit(o, q, co):
    """(n, ncols) coefficients -> (n, ncols): column c = imodwt of the matrix with every other column +0 (modwt_mra_cases.mra_of)"""
    out = np.empty_like(co)
    for c in range(co.shape[1]):
        z = np.zeros_like(co)
        z[:, c] = co[:, c]
        out[:, c] = o.imodwt(z, q)
    return out


Entry = namedtuple("Entry", "lifting fwd_ref inv_ref fwd_gpu inv_gpu synthesis", defaults=(False,))
ENTRIES = {
    "dwt": Entry(False, lambda o, W, wt, x, L: o.dwt_filter(x, wt.qmf, L), lambda o, W, wt, y, L: o.dwt_filter(y, wt.qmf, L, fw=False),
                 lambda W, wt, x, L: W.dwt(x, wt, L), lambda W, wt, y, L: W.idwt(y, wt, L)),
    "dwt_lifting": Entry(True, lambda o, W, wt, x, L: o.dwt_lifting(x, wt, L), lambda o, W, wt, y, L: o.dwt_lifting(y, wt, L, fw=False),
                         lambda W, wt, x, L: W.dwt(x, wt, L), lambda W, wt, y, L: W.idwt(y, wt, L)),
    "dwtc": Entry(False, lambda o, W, wt, x, L: o.dwtc_filter(x, wt.qmf, L), lambda o, W, wt, y, L: o.dwtc_filter(y, wt.qmf, L, fw=False),
                  lambda W, wt, x, L: W.dwtc(x, wt, L), lambda W, wt, y, L: W.idwtc(y, wt, L)),
    "wpt": Entry(False, lambda o, W, wt, x, L: o.wpt_filter(x, wt.qmf, _tree(W, len(x), L)),
                 lambda o, W, wt, y, L: o.wpt_filter(y, wt.qmf, _tree(W, len(y), L), fw=False),
                 lambda W, wt, x, L: W.wpt(x, wt, _tree(W, x.shape[0], L)), lambda W, wt, y, L: W.iwpt(y, wt, _tree(W, y.shape[0], L))),
    "wpt_lifting": Entry(True, lambda o, W, wt, x, L: o.wpt_lifting(x, wt, _tree(W, len(x), L)),
                         lambda o, W, wt, y, L: o.wpt_lifting(y, wt, _tree(W, len(y), L), fw=False),
                         lambda W, wt, x, L: W.wpt(x, wt, _tree(W, x.shape[0], L)), lambda W, wt, y, L: W.iwpt(y, wt, _tree(W, y.shape[0], L))),
    "modwt": Entry(False, lambda o, W, wt, x, L: o.modwt(x, wt.qmf, L), lambda o, W, wt, y, L: o.imodwt(y, wt.qmf),
                   lambda W, wt, x, L: W.modwt(x, wt, L), lambda W, wt, y, L: W.imodwt(y, wt)),
    "modwt_batch": Entry(False, lambda o, W, wt, x, L: _units(lambda u: o.modwt(u, wt.qmf, L), x),
                         lambda o, W, wt, y, L: _units(lambda u: o.imodwt(u, wt.qmf), y),
                         lambda W, wt, x, L: W.modwt_batch(x, wt, L), lambda W, wt, y, L: W.imodwt_batch(y, wt)),
    # (the analysis of a coefficient tensor n x (L + 1) x B: one direction only)
    "modwt_mra": Entry(False, lambda o, W, wt, x, L: _units(lambda u: _mra_unit(o, wt.qmf, u), x), None,
                       lambda W, wt, x, L: W.modwt_mra_batch(x, wt), None, True),
    "dwt_batch_lifting": Entry(True, lambda o, W, wt, x, L: _units(lambda u: o.dwt_lifting(u, wt, L), x),
                               lambda o, W, wt, y, L: _units(lambda u: o.dwt_lifting(u, wt, L, fw=False), y),
                               lambda W, wt, x, L: W.dwt_batch(x, wt, L), lambda W, wt, y, L: W.idwt_batch(y, wt, L)),
    "dwt_batch": Entry(False, lambda o, W, wt, x, L: _units(lambda u: o.dwt_filter(u, wt.qmf, L), x),
                       lambda o, W, wt, y, L: _units(lambda u: o.dwt_filter(u, wt.qmf, L, fw=False), y),
                       lambda W, wt, x, L: W.dwt_batch(x, wt, L), lambda W, wt, y, L: W.idwt_batch(y, wt, L)),
}


def wavelet(W, entry, name):
    return W.wavelet(getattr(W.WT, name), W.WT.Lifting) if ENTRIES[entry].lifting else W.wavelet(getattr(W.WT, name))


# ---- recipes ---------------------------------------------------------------------------------------------------------------------
# Lz: the depth of the `zeros` class -- the smallest at which the named kernels run (1 unless they are multi-level kernels), so that a
# zero of another sign is the named kernel's and not the doing of the tier below it
Recipe = namedtuple("Recipe", "name entry opts shape L wavelets kfwd kinv dtypes note Lz")


def R(name, entry, opts, shape, L, wavelets, kfwd, kinv, dtypes=BOTH, note="", Lz=1):
    return Recipe(name, entry, dict(opts), tuple(shape), L, tuple(wavelets), kfwd, kinv, tuple(dtypes), note, Lz)


def depth(r, cls):
    return r.Lz if cls == "zeros" else r.L


NO_TILES = {"WL_M2D_MAX": 128, "WL_TILE": 0, "WL_TILEB": 0}
ONE_PASS_3D = {"WL_3D_ONE_MIN": 0, "WL_3D_ONE_WAVES": 0, "WL_I3D_ONE_MIN": 0, "WL_I3D_ONE_MIN_LONG": 0, "WL_I3D_ONE_MIN_ANY": 0,
               "WL_I3D_ONE_WAVES": 0, "WL_I3D_ONE_F64_FMAX": 8}
INV_LONG = {"WL_INVLONG2D_MIN_ROWS": 256, "WL_INVLONG_FMIN": 8, "WL_INVLONG_SHORT_MIN": 0, "WL_INV_PAIR": 0, "WL_TILE_INV": 0,
            "WL_TILE_INV_LONG": 0}

RECIPES = (
    # ---- wl_fwd.hip / wl_inv.hip: 2-D ----
    R("pair", "dwt", {"WL_LDS_PAIR_MIN": 0, "WL_PAIR_WG_PER_CU": 0, **NO_TILES}, (512, 96), 2, ("db4", "haar"), "k_fwd2d_pair", None, (F32,),
      Lz=2),
    R("inv_pair", "dwt", {"WL_INV_PAIR_MIN": 0, "WL_TILE_INV": 0}, (1024, 96), 2, ("db4", "haar"), None, "k_inv2d_pair", (F32,),
      "1024 rows: the kernel's smallest strip", Lz=2),
    R("pair_tile", "dwt", {"WL_FUSE4": 1, "WL_LDS_PAIR_MIN": 0, "WL_TILEB_MIN": 0, "WL_PAIR_WG_PER_CU": 0, "WL_TILE": 0, "WL_M2D_MAX": 64,
                           "WL_TILEB_MAX": 128}, (512, 512), 4, ("db4",), "k_fwd2d_pair_tile", None, (F32,),
      "opt-in; L = 4: the launch is four levels", Lz=4),
    R("lds", "dwt", {"WL_FUSE2": 0, "WL_INV_PAIR": 0, "WL_TILE_INV": 0, **NO_TILES}, (272, 64), 2, ("db4", "haar"), "k_fwd2d_lds",
      "k_inv2d_stream", (F32,)),
    R("lds64", "dwt", {"WL_LDS_PAIR_MIN64": 1 << 62, "WL_PAIR_WG_PER_CU": 0, "WL_WAVES_PER_CU": 0, "WL_WAVES_MIN": 0, "WL_TILE_INV": 0,
                       **NO_TILES}, (256, 160), 2, ("db4", "haar"), "k_fwd2d_lds64", "k_inv2d_stream", (F64,)),
    R("pair64", "dwt", {"WL_LDS_PAIR_MIN64": 0, "WL_PAIR_WG_PER_CU": 0, "WL_WAVES_PER_CU": 0, "WL_WAVES_MIN": 0, **NO_TILES}, (256, 160), 2,
      ("db4", "sym5"), "k_fwd2d_pair64", None, (F64,), Lz=2),
    R("stream2", "dwt", {"WL_FUSE2_MIN": 0, "WL_LDS2D": 0, **NO_TILES}, (528, 96), 2, ("db4", "haar"), "k_fwd2d_stream2", None, (F32,), Lz=2),
    R("stream", "dwt", {"WL_LDS2D": 0, "WL_FUSE2": 0, "WL_TILE_INV": 0, **NO_TILES}, (528, 96), 2, ("db4", "db2"), "k_fwd2d_stream",
      "k_inv2d_stream"),
    R("tile", "dwt", {"WL_TILE_MAX": 2048, "WL_TILEB": 0, "WL_LDS2D_MIN_ROWS": 1 << 20}, (192, 320), 2, ("db4", "haar"), "k_fwd2d_tile",
      "k_inv2d_tile2", Lz=2),
    R("tileB", "dwt", {"WL_TILEB_MIN": 0, "WL_LDS2D_MIN_ROWS": 1 << 20, "WL_LDS_PAIR_MIN": 1 << 62}, (128, 128), 2, ("db4", "sym5"),
      "k_fwd2d_tileB", None, (F32,), Lz=2),
    R("multi2d", "dwt", {"WL_TILE": 0, "WL_TILEB": 0}, (128, 128), 2, ("db4", "haar"), "k_fwd2d_multi", None),
    R("tail2", "dwt", {"WL_NO_MULTI2D": 1}, (64, 64), 2, ("db4", "haar"), "k_tail2_fwd", "k_tail2_inv"),
    R("tail", "dwt", {"WL_NO_MULTI2D": 1, "WL_TAIL2": 0}, (64, 32), 2, ("db2", "haar"), "k_tail_fwd", "k_tail_inv"),
    R("lds_long", "dwt", {"WL_LONG2D_MIN_ROWS": 256, "WL_TILE_LONG": 0, **INV_LONG}, (256, 96), 2, ("db6", "db10"), "k_fwd2d_lds_long",
      "k_inv2d_lds_long", (F32,)),
    R("inv_lds_long64", "dwt", INV_LONG, (256, 96), 2, ("db4", "db8"), None, "k_inv2d_lds_long", (F64,)),
    R("long_lines", "dwt", {}, (520, 96), 2, ("db6", "sym8"), "k_long_lines", "k_long_lines"),
    R("vl_lines", "dwt", {}, (520, 96), 1, ("batt2",), "k_vl_lines", "k_vl_lines", BOTH, "L = 1: 260 rows is no shape of the kernel"),
    R("gtile", "dwt", {}, (260, 132), 2, ("db4", "haar"), "k_fwd2d_gtile", "k_inv2d_gtile"),
    R("inv_dim2", "dwt", {"WL_NO_INV2D": 1, "WL_INV_PAIR": 0, "WL_TILE_INV": 0}, (512, 96), 2, ("db4", "haar"), None, "k_inv_dim2_stream"),
    # ---- 1-D ----
    R("multi1d", "dwt", {}, (16384,), 4, ("db4", "haar"), "k_fwd1d_multi", "k_inv1d_stream2", Lz=2),
    R("stream1d", "dwt", {}, (8200,), 3, ("db4", "haar"), "k_fwd1d_stream", "k_inv1d_stream"),
    R("tail2_1d", "dwt", {}, (512,), 4, ("db4", "haar"), "k_tail2_fwd", "k_tail2_inv"),
    R("long_lines_1d", "dwt", {}, (8192,), 4, ("db6",), "k_long_lines", "k_long_lines"),
    R("dwtc_multi", "dwtc", {}, (1024, 33), 4, ("db4", "haar"), "k_fwd1d_multi", None),
    R("dwtc_tail2", "dwtc", {}, (256, 37), 4, ("db4", "haar"), "k_tail2_fwd", "k_tail2_inv"),
    # ---- wl_axis.hip and the 3-D tiers ----
    R("tail3", "dwt", {}, (16, 16, 16), 2, ("db2", "haar"), "k_tail3", "k_tail3"),
    R("level3", "dwt", {"WL_3D_ONE_MIN_ANY": 1 << 40, "WL_I3D_ONE_MIN_ANY": 1 << 40}, (16, 16, 32), 2, ("db2", "haar"), "k_level3_lds",
      "k_level3_lds"),
    R("one3d", "dwt", ONE_PASS_3D, (72, 16, 16), 2, ("db4", "haar"), "k_fwd3d_one", "k_inv3d_one"),
    R("axis3d", "dwt", {"WL_3D_ONE": 0, "WL_I3D_ONE": 0, "WL_LEVEL3": 0}, (64, 16, 32), 2, ("db4", "haar"), "k_fwd_axis_stream",
      "k_inv_axis_stream"),
    R("any3d", "dwt", {"WL_LEVEL3": 0, "WL_3D_ONE": 0, "WL_I3D_ONE": 0}, (60, 36, 20), 2, ("db4", "haar"), "k_fwd_any", "k_inv_any"),
    R("generic3d", "dwt", {"WL_ANYAXIS": 0, "WL_LEVEL3": 0, "WL_3D_ONE": 0, "WL_I3D_ONE": 0}, (60, 36, 20), 2, ("db4", "haar"),
      "k_generic_fwd_filter", "k_generic_inv_filter"),
    # ---- wl_batch3d.hip and the batch of images ----
    R("tail3_batch", "dwt_batch", {}, (16, 16, 16, 3), 2, ("db2", "haar"), "k_tail3_batch", "k_tail3_batch"),
    R("level3_batch", "dwt_batch", {}, (44, 28, 36, 2), 2, ("db4", "haar"), "k_level3_lds_batch", "k_level3_lds_batch"),
    R("one3d_batch", "dwt_batch", ONE_PASS_3D, (72, 16, 16, 2), 2, ("db4", "haar"), "k_fwd3d_one_batch", "k_inv3d_one_batch"),
    R("images", "dwt_batch", {}, (256, 96, 3), 2, ("db4", "haar"), "k_fwd2d_lds", "k_inv2d_stream", (F32,)),
    R("images_long", "dwt_batch", {"WL_INVLONG2D_MIN_ROWS": 256, "WL_INVLONG_SHORT_MIN": 0}, (256, 96, 3), 1, ("db10",), None,
      "k_inv2d_lds_long", (F32,), "L = 1 as in test_batched_planes_lds_exchange_inverse"),
    # ---- wl_lift.hip ----
    R("lift_stream", "dwt_lifting", {}, (8192,), 1, ("cdf97", "db2"), "k_lift1d_stream", "k_lift1d_stream"),
    R("lift_3level", "dwt_lifting", {}, (32768,), 3, ("cdf97", "haar"), "k_lift1d_fwd3", "k_lift1d_inv3", BOTH, "L = 3: the launch is three levels", Lz=3),
    R("lift_gtile1d", "dwt_lifting", {}, (2100,), 1, ("cdf97", "db2"), "k_lift1d_gtile", "k_lift1d_gtile"),
    R("lift_regtail", "dwt_lifting", {}, (256,), 2, ("cdf97", "haar"), "k_tail_lift_reg", "k_tail_lift_reg_inv", Lz=2),
    R("lift_tail", "dwt_lifting", {"WL_LIFT_REGTAIL": 0}, (2048,), 2, ("cdf97", "db2"), "k_tail_lift", "k_tail_lift"),
    R("lift2d_fused", "dwt_lifting", {"WL_LIFT_TILE": 0}, (256, 256), 1, ("cdf97", "haar"), "k_lift2d_fwd", "k_lift2d_inv"),
    R("lift2d_tile", "dwt_lifting", {}, (192, 192), 1, ("cdf97", "db2"), "k_lift2d_tile", "k_lift2d_tile"),
    R("lift2d_gtile", "dwt_lifting", {}, (100, 100), 1, ("cdf97", "haar"), "k_lift2d_gtile", "k_lift2d_gtile"),
    R("lift2d_ldstail", "dwt_lifting", {}, (64, 64), 2, ("cdf97", "db2"), "k_tail_lift2d_lds", None),
    R("lift2d_ldstail_inv", "dwt_lifting", {}, (128, 128), 1, ("cdf97", "haar"), None, "k_tail_lift2d_lds", (F32,)),
    R("lift2d_stream", "dwt_lifting", {"WL_LIFT_TILE": 0, "WL_NO_LIFT2D_FUSED": 1}, (512, 512), 1, ("cdf97", "haar"),
      "k_lift_axis_stream+lines", "k_lift_axis_stream+lines", BOTH, "k_lift_axis_stream along dimension 2, k_lift1d_stream along dimension 1"),
    R("lift3d", "dwt_lifting", {"WL_LIFT_TAIL3D": 0}, (32, 32, 32), 1, ("cdf97", "haar"), "k_lift_axis_stream+k_lift_short_lines",
      "k_lift_axis_stream+k_lift_short_lines", BOTH, "without the tail every level goes through the axis and short-line launches"),
    R("lift3d_batch", "dwt_batch_lifting", {"WL_LIFT_TAIL3D": 0}, (16, 16, 16, 3), 2, ("cdf97", "db2"),
      "k_lift_axis_stream+k_lift_short_lines_batch", "k_lift_axis_stream+k_lift_short_lines_batch"),
    R("lift_generic", "dwt_lifting", {"WL_LIFT_GTILE": 0}, (100, 100), 1, ("cdf97", "db2"), "k_generic_lift_fwd", "k_generic_lift_inv"),
    R("lift_any", "dwt_lifting", {}, (36, 36, 36), 1, ("cdf97", "haar"), "k_lift_any", "k_lift_any"),
    # ---- the packet part of wl_api.hip ----
    R("wpt_tail", "wpt", {}, (256,), 4, ("db2", "haar"), "k_wpt_fwd_tail", "k_wpt_inv_tail"),
    R("wpt_multi", "wpt", {}, (16384,), 4, ("db4", "haar"), "k_wpt_fwd_multi", "k_wpt_inv_multi", Lz=2),
    R("wpt_lines", "wpt", {}, (16384,), 1, ("db4", "haar"), "k_fwd1d_stream", "k_inv1d_stream", BOTH, "a lone fully split depth is a line level"),
    R("wpt_generic", "wpt", {"WL_WPT_FAST": 0}, (256,), 4, ("db2", "haar"), "k_generic_filter_wpt", "k_generic_filter_wpt"),
    R("wpt_lift", "wpt_lifting", {}, (16384,), 2, ("cdf97", "haar"), "k_lift1d_stream", "k_lift1d_stream"),
    R("wpt_lift_generic", "wpt_lifting", {"WL_WPT_FAST": 0}, (256,), 2, ("cdf97", "haar"), "k_generic_lift_wpt", "k_generic_lift_wpt"),
    # ---- wl_modwt.hip ----
    R("modwt", "modwt", {}, (1000,), 3, ("db4", "haar"), "k_modwt_step", "k_imodwt_step", Lz=3),
    R("modwt_lds", "modwt_batch", {}, (100, 5), 3, ("db4", "haar"), "k_modwt_lds", "k_imodwt_lds", Lz=3),
    R("modwt_step_b", "modwt_batch", {"WL_MODWT_FUSED": 0}, (100, 5), 3, ("db4", "haar"), "k_modwt_step_b", "k_imodwt_step_b", Lz=3),
    R("mra_lds", "modwt_mra", {}, (100, 4, 3), 3, ("db4", "haar"), "k_modwt_mra_lds", None, Lz=3),
    R("mra_step_b", "modwt_mra", {"WL_MODWT_FUSED": 0}, (100, 4, 3), 3, ("db4", "haar"), "k_modwt_mra_step_b", None, Lz=3),
)

# (recipe, class) pairs that cannot meet their class's condition: at most one class per recipe, at most 10 % of all pairs
_FEW_PASSES = "fewer than three passes over the cluster: no Inf - Inf"
_MODWT = "taps / sqrt 2, sum |taps| < 1.2: entries of 2^(maxexp-1) stay finite at these depths"
SKIPS = {
    ("vl_lines", "overflow"): _FEW_PASSES, ("stream1d", "overflow"): _FEW_PASSES,
    ("images_long", "overflow"): _FEW_PASSES, ("wpt_lines", "overflow"): _FEW_PASSES,
    ("modwt", "overflow"): _MODWT, ("modwt_lds", "overflow"): _MODWT, ("modwt_step_b", "overflow"): _MODWT,
    ("mra_lds", "overflow"): _MODWT, ("mra_step_b", "overflow"): _MODWT,
}

# kernel names whose special-value behaviour another test covers
ELSEWHERE = {
    "k_threshold": "test_gpu_threshold_batch.py::test_special_values",
    "k_threshold_batch": "test_gpu_threshold_batch.py::test_special_values",
    "k_threshold_batch_wave": "test_gpu_threshold_batch.py::test_special_values",
    "k_thbig_lds": "test_gpu_threshold_batch.py::test_special_values",
    "k_thbig_stream": "test_gpu_threshold_batch.py::test_special_values",
    "k_thbig_split": "test_gpu_threshold_batch.py::test_special_values",
    "k_mad_units_lds": "test_gpu_denoise_batch.py",
    "k_mad_units_stream": "test_gpu_denoise_batch.py",
    "k_mp_absmax_part": "test_gpu_matchingpursuit.py",
    "k_mp_absmax_fold": "test_gpu_matchingpursuit.py",
    "k_mp_select": "test_gpu_matchingpursuit.py",
    "k_mp_residual_part": "test_gpu_matchingpursuit.py",
    "k_entropy_seg": "test_gpu_bestbasis.py",
    "k_wpt2_tail": "test_gpu_wpt2.py",
    "k_wpt2_level": "test_gpu_wpt2.py",
}
# literals of the same spelling that are no kernel name
NOT_KERNELS = {"k_wpt": "the prefix wpt_impl compares the running name with (strncmp), never reported"}

# kernels whose zero results may carry either sign: {name: the zero terms of the reference's chain that the kernel omits}
# Every inverse filter-bank kernel evaluates the closed form of wl_internal.h, x[o] = S[o] + D[o] with S and D summed over the taps
# that meet a coefficient.  The reference's filtup! runs its shift register over the up-sampled sequence: its chain starts as 0 + ...
# and carries a tap * 0 term for every inserted zero.  Those terms change no value and no non-zero sum; they turn a result of -0 into
# +0.  modwt_mra drops the h * 0 terms of the columns it sets to +0.  Only the inverse calls of a name that
# serves both directions are let off.
_CLOSED = "closed form S[o] + D[o]%s: no leading 0 + and no tap * 0 terms of the up-sampled zeros"
ZERO_SIGN_FREE = {
    "k_inv1d_stream": _CLOSED % "",
    "k_inv1d_stream2": _CLOSED % ", both levels",
    "k_inv2d_stream": _CLOSED % " along both dimensions",
    "k_inv_dim2_stream": _CLOSED % " (and k_inv1d_stream for dimension 1)",
    "k_inv2d_pair": _CLOSED % ", both levels",
    "k_inv2d_tile2": _CLOSED % " (window_inv), both levels",
    "k_inv2d_gtile": _CLOSED % " (window_inv)",
    "k_tail_inv": _CLOSED % ", every level of the tail",
    "k_tail2_inv": _CLOSED % " (window_inv), every level of the tail",
    "k_tail3": _CLOSED % " (window_inv) in its inverse levels",
    "k_tail3_batch": _CLOSED % " (window_inv) in its inverse levels",
    "k_level3_lds": _CLOSED % " (window_inv) in its inverse launch",
    "k_level3_lds_batch": _CLOSED % " (window_inv) in its inverse launch",
    "k_inv3d_one": _CLOSED % " (window_inv) along the three dimensions",
    "k_inv3d_one_batch": _CLOSED % " (window_inv) along the three dimensions",
    "k_inv_axis_stream": _CLOSED % " along the strided axes (and k_short_lines along dimension 1)",
    "k_inv_any": _CLOSED % " (window_inv)",
    "k_generic_inv_filter": _CLOSED % ": S starts on its first product",
    "k_wpt_inv_tail": _CLOSED % " (window_inv) at every depth",
    "k_wpt_inv_multi": _CLOSED % " (window_inv) at every depth",
    "k_generic_filter_wpt": _CLOSED % " in its inverse passes (k_generic_inv_filter)",
    "k_modwt_mra_lds": "drops the h * 0 terms of the columns the definition sets to +0",
    "k_modwt_mra_step_b": "drops the h * 0 terms of the columns the definition sets to +0",
}


def recipe_cases():
    """(recipe, dtype name) for every row and element type"""
    return [(r, d) for r in RECIPES for d in r.dtypes]


def case_id(rd):
    return "%s-%s" % (rd[0].name, "f32" if rd[1] == F32 else "f64")


def kernel_names():
    return {k for r in RECIPES for k in (r.kfwd, r.kinv) if k}


def inv_shape(r, L):
    """the shape of the inverse call's input"""
    if r.entry == "modwt":
        return r.shape + (L + 1,)
    if r.entry == "modwt_batch":
        return (r.shape[0], L + 1, r.shape[1])
    return r.shape


_SEED = {c: 11 + 7 * i for i, c in enumerate(CLASSES)}


def class_input(r, dtype, cls):
    return CLASSES[cls](r.shape, np.dtype(dtype), _SEED[cls] + sum(r.shape))


def reference_one_level(oracle, W, r, dtype, wname, cls):
    """-> (fwd, inv) of the class input at L = 1 (modwt_mra: the recipe's own columns): where the nan classes' condition is stated"""
    e = ENTRIES[r.entry]
    wt = wavelet(W, r.entry, wname)
    with np.errstate(all="ignore"):
        fwd = e.fwd_ref(oracle, W, wt, class_input(r, dtype, cls), 1)
        return fwd, (e.inv_ref(oracle, W, wt, fwd, 1) if e.inv_ref is not None else None)


def direct_inverse_input(r, dtype, cls, L):
    """A second inverse input for `inf_pair`, whose Inf the inverse of a forward output turns into NaN, planted so that the inverse
    itself keeps it: normals with +Inf at a quarter and -Inf at three quarters of the deepest approximation band of every axis -- one
    sub-band, so the two meet at most where their supports overlap.  (`overflow` has no such input: a synthesis pass scales a
    same-sign block of the approximation band by 1 / sqrt 2 and sums at most half the taps per output, so finite clusters of
    2^(maxexp-1) stay finite in every inverse; an Inf of an inverse output can only come from its input.)"""
    shape, dt = inv_shape(r, L), np.dtype(dtype)
    x = rng_array(shape, dt, _SEED[cls] + 2 + sum(shape))
    lo = tuple(min(s - 1, (s >> L) // 4) for s in shape)
    hi = tuple(min(s - 1, max(3 * (s >> L) // 4, a + 1)) for s, a in zip(shape, lo))
    x[lo], x[hi] = np.inf, -np.inf
    return x


DIRECT_CLASSES = ("inf_pair",)
_REF = {}


def reference(oracle, W, r, dtype, wname, cls, L=None):
    """-> (x, fwd, inv_in, inv, dir_in, dir_out): the class input, the oracle's forward output, the inverse call's input (the forward
    output; for `zeros` a zeros input of that shape), the oracle's inverse output (None for an entry with one direction), and for
    DIRECT_CLASSES the second inverse input (direct_inverse_input) with its inverse output (else None).  Computed once per key and
    shared: callers must not modify what they get.  L: another depth than the class's own (depth(r, cls))."""
    L = depth(r, cls) if L is None else L
    key = (r.name, dtype, wname, cls, L)
    if key not in _REF:
        e = ENTRIES[r.entry]
        wt = wavelet(W, r.entry, wname)
        dt = np.dtype(dtype)
        x = class_input(r, dtype, cls)
        with np.errstate(all="ignore"):
            fwd = e.fwd_ref(oracle, W, wt, x, L)
            inv_in = inv = dir_in = dir_out = None
            if e.inv_ref is not None and cls in DIRECT_CLASSES:
                dir_in = direct_inverse_input(r, dtype, cls, L)
                dir_out = e.inv_ref(oracle, W, wt, dir_in, L)
            if e.inv_ref is not None:
                if cls == "zeros":       # (the zeros input itself; modwt: one of the coefficient array's shape)
                    inv_in = x if inv_shape(r, L) == r.shape else zeros(inv_shape(r, L), dt, _SEED[cls] + 1 + sum(r.shape))
                else:
                    inv_in = fwd
                inv = e.inv_ref(oracle, W, wt, inv_in, L)
        for a in (x, fwd, inv_in, inv, dir_in, dir_out):
            if a is not None:
                a.setflags(write=False)
        _REF[key] = (x, fwd, inv_in, inv, dir_in, dir_out)
    return _REF[key]
