"""Case table of user-defined lifting schemes (GLS built from the user's own steps, as W.GLS((steps, norm1, norm2, name)) takes
them) and the kernel tier each one must reach.

The shape-specialised lifting kernels are picked by match_shape (wl_lift_shapes.h) from the step types, coefficient counts and
shifts of the direction-adjusted scheme; the coefficients and norms stay run-time data.  SHAPES restates the Shape<ID>
specialisations of wl_lift_shapes.h (test_lifting_schemes.py parses the header and fails when the two drift apart), so that a
test can state which tier a scheme must take:

- TWINS have the step sequence of cdf9/7, db2 and haar/db1 but other coefficients (c1 != +-c2 in every 2-coefficient step,
  none equal to a table coefficient) and other norms: they run on the shape-specialised kernels, where a swapped operand order
  or a wrong coefficient index would show (every cdf9/7 step has two equal coefficients).
- REVERSED_TWINS are the twins with their step lists read backwards: their FORWARD step sequence has an inverse shape (IDs 1 / 3 / 5)
  and their inverse a forward one.  Only the kernel families instantiated for every shape in both directions (k_lift1d_stream,
  k_lift_axis_stream, k_lift_short_lines) may take them; every direction-bound family must leave them to the generic kernels.
- CUSTOM schemes match no known shape: 3-coefficient steps, shifts beyond +-1 (operand indices that wrap more than once),
  0, 1, 5 and 16 steps.  They run on the LDS tails and the generic kernels.
- NEAR_MISSES are the table schemes with exactly one field changed; match_shape must not accept them.
- LARGE_SHIFTS use shifts up to the int32 limits (the C ABI takes any int32 shift).

Coefficients are small enough that a full-depth Float32 transform of the test inputs stays far from overflow (checked on the
Float64 oracle by test_lifting_schemes.py).
"""
import numpy as np

# wl_lift_shapes.h, Shape<ID>::S: (is_update, nc, shift) per step in direction-adjusted order (make_scheme: the table order
# forward, reversed for the inverse)
SHAPES = {
    0: ((1, 2, 0), (0, 2, 1), (1, 2, 0), (0, 2, 1)),     # cdf9/7 forward
    1: ((0, 2, 1), (1, 2, 0), (0, 2, 1), (1, 2, 0)),     # cdf9/7 inverse
    2: ((0, 1, 0), (1, 2, 1), (0, 1, -1)),               # db2 forward
    3: ((0, 1, -1), (1, 2, 1), (0, 1, 0)),               # db2 inverse
    4: ((0, 1, 0), (1, 1, 0)),                           # haar/db1 forward
    5: ((1, 1, 0), (0, 1, 0)),                           # haar/db1 inverse
}

# the kernels match_shape can send a scheme to (W.last_kernel() names); a scheme of no known shape never reaches them
SPECIALISED_KERNELS = ("k_lift1d_fwd3", "k_lift1d_inv3", "k_lift1d_stream", "k_lift1d_gtile", "k_tail_lift_reg", "k_tail_lift_reg_inv",
                       "k_lift2d", "k_lift2d_tile", "k_lift2d_gtile", "k_tail_lift2d_reg", "k_tail_lift2d_lds", "k_lift_axis_stream",
                       "k_lift_short_lines", "k_tail_lift3d", "k_lift_any")

# the reference's table schemes (wt_tables.json) these are measured against
REFERENCE = ("cdf97", "db2", "haar", "db1")

# ---- schemes: name -> (steps, norm1, norm2); a step is ("P" | "U", coefficients, shift) in table order ----------------------
TWINS = {
    # cdf9/7's shape; every pair keeps the table pair's sum (so the transform stays as well conditioned) with c1 != +-c2
    "twin_cdf97": ((("U", (1.9, 1.2722686841208), 0), ("P", (0.0831, 0.02286023714582988), 1),
                    ("U", (-1.05, -0.715822151062786), 0), ("P", (-0.61, -0.2770137040876931), 1)), 1.13, 0.885),
    "twin_db2": ((("P", (-1.6180339887498949,), 0), ("U", (-0.105, 0.4710254037844386), 1), ("P", (0.9,), -1)), 0.55, 1.85),
    "twin_haar": ((("P", (-0.9,), 0), ("U", (0.55,), 0)), 0.75, 1.35),
}

# the table scheme each twin copies the shape of
TWIN_OF = {"twin_cdf97": "cdf97", "twin_db2": "db2", "twin_haar": "haar"}

# the twins read backwards (same coefficients and norms): a user's scheme whose forward pass has the shape of an inverse pass
REVERSED_TWINS = {"rev_" + name: (steps[::-1], n1, n2) for name, (steps, n1, n2) in TWINS.items()}

_SIXTEEN = tuple((("P", "U")[i % 2], ((0.11, -0.07, 0.05)[: 1 + i % 3] if i % 4 < 2 else (-0.09, 0.06, 0.13)[: 1 + i % 3]),
                  (-2, -1, 0, 1, 2, 3)[i % 6]) for i in range(16))

CUSTOM = {
    "nc3": ((("P", (0.21, -0.47, 0.13), 1), ("U", (-0.17, 0.29, 0.08), 0), ("P", (0.06, -0.11, 0.27), -1)), 1.21, 0.79),
    "shift2": ((("P", (0.37, -0.19), 2), ("U", (0.23,), -2)), 0.93, 1.07),
    "shift3": ((("U", (-0.31,), 3), ("P", (0.14, 0.41), -3)), 1.05, 0.96),
    "shift5": ((("P", (0.12, -0.26, 0.33), 5), ("U", (-0.22,), -5), ("P", (0.18,), 2)), 0.97, 1.03),
    "wide": ((("P", (0.27,), 37), ("U", (-0.19, 0.34), -41), ("P", (0.07, 0.15, -0.09), 300), ("U", (0.2,), 70001)), 1.04, 0.94),
    "zero_steps": ((), 1.07, 0.91),
    "one_update": ((("U", (0.29, -0.13), 1),), 1.1, 0.9),
    "one_predict": ((("P", (-0.44,), -1),), 0.8, 1.2),
    "five": ((("P", (0.3,), 0), ("U", (-0.2, 0.1), 1), ("P", (0.15, -0.05, 0.2), -1), ("U", (0.25,), 2), ("P", (-0.12, 0.09), -2)),
             1.02, 0.98),
    "sixteen": (_SIXTEEN, 1.01, 0.99),
    "mix": ((("U", (0.16, -0.23, 0.31), -3), ("P", (0.22,), 2), ("U", (-0.14, 0.08), 37), ("P", (0.05, 0.12, -0.17), -5),
             ("U", (0.26,), 3), ("P", (-0.18, 0.07), -2), ("U", (0.09, -0.04, 0.11), 0)), 0.96, 1.06),
}


def _tbl(name):
    """table steps of a reference scheme, as (type, coefs, shift) tuples"""
    c = {
        "cdf97": ((("U", (1.5861343420604, 1.5861343420604), 0), ("P", (0.05298011857291494, 0.05298011857291494), 1),
                   ("U", (-0.882911075531393, -0.882911075531393), 0), ("P", (-0.44350685204384654, -0.44350685204384654), 1)),
                  1.1496043988603355, 0.8698644516247099),
        "db2": ((("P", (-1.7320508075688772,), 0), ("U", (-0.0669872981077807, 0.4330127018922193), 1), ("P", (1.0,), -1)),
                0.5176380902050414, 1.9318516525781364),
        "haar": ((("P", (-1.0,), 0), ("U", (0.5,), 0)), 0.7071067811865475, 1.4142135623730951),
    }
    return c[name]


def _flip(st):
    return ("U" if st[0] == "P" else "P",) + tuple(st[1:])


def _near_misses():
    out = {}
    for ref in ("cdf97", "db2", "haar"):
        steps, n1, n2 = _tbl(ref)
        steps = list(steps)
        for k in range(len(steps)):
            t, c, s = steps[k]
            mods = {"type%d" % k: _flip(steps[k]), "ncplus%d" % k: (t, c + (c[-1] * 0.5,), s), "shiftplus%d" % k: (t, c, s + 1),
                    "shiftminus%d" % k: (t, c, s - 1)}
            if len(c) > 1:
                mods["ncminus%d" % k] = (t, c[:1], s)
            if ref == "cdf97" and t == "U":
                # (cdf9/7's Update pairs of +-1.6 / -0.9 turned into Predicts amplify ~10x per level: growth 1e10 at 2^14, a
                # round trip good to 1e-6 only -- the Predict steps flipped cover the type field)
                del mods["type%d" % k]
            for tag, st in mods.items():
                out["near_%s_%s" % (ref, tag)] = (tuple(steps[:k]) + (st,) + tuple(steps[k + 1:]), n1, n2)
        out["near_%s_added" % ref] = (tuple(steps) + (("U" if steps[-1][0] == "P" else "P", (0.125,), 0),), n1, n2)
        out["near_%s_dropped" % ref] = (tuple(steps[:-1]), n1, n2)
    return out


NEAR_MISSES = _near_misses()

# shifts up to the int32 limits: every operand index of every element wraps (reached only after the tail tier's wrap was made
# int64 -- with `int j0 = j - shift` and a wrap loop the tail could spin ~2^31 times per element)
LARGE_SHIFTS = {
    "shift_2p20": ((("P", (0.31, -0.17), 2 ** 20 + 3), ("U", (0.23,), -(2 ** 20 + 3)), ("P", (0.11, 0.07, -0.05), 1)), 1.03, 0.95),
    "shift_int32": ((("P", (0.19, -0.08, 0.14), 2 ** 31 - 1), ("U", (-0.21, 0.12), -(2 ** 31 - 1)), ("P", (0.17,), -2 ** 31),
                     ("U", (0.06, 0.1, -0.13), 2 ** 31 - 1)), 0.98, 1.04),
}

ALL = {**TWINS, **CUSTOM, **NEAR_MISSES, **LARGE_SHIFTS}


def spec(name):
    if name in ALL:
        return ALL[name]
    if name in REVERSED_TWINS:
        return REVERSED_TWINS[name]
    return _tbl("haar" if name == "db1" else name)


def scheme(W, name):
    """the GLS of a table entry (or of a reference scheme by its WT name), built the way a user builds one"""
    if name in REFERENCE:
        return W.wavelet(getattr(W.WT, name), W.WT.Lifting)
    steps, n1, n2 = spec(name)
    WT = W.WT
    st = [WT.make_lsstep(WT.Predict if t == "P" else WT.Update, list(c), s) for t, c, s in steps]
    return W.GLS((st, n1, n2, name))


def steps_of(sch):
    """(is_update, nc, shift) per step of a GLS in table order"""
    return tuple((1 if type(s.steptype).__name__ == "UpdateStep" else 0, len(s.param.coef), int(s.param.shift)) for s in sch.step)


def shape_id(sch, fw=True):
    """match_shape (wl_lift_shapes.h) restated: the ID of the known shape the direction-adjusted scheme has, or -1"""
    seq = steps_of(sch)
    if not fw:
        seq = seq[::-1]
    for i in sorted(SHAPES):
        if SHAPES[i] == seq:
            return i
    return -1
