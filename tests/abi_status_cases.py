"""The order of the status codes of the C ABI entry points that no other test pins (test_abi_status.py runs this table).

Every entry is (symbol, base, rules):

- base: the arguments of a valid, small call in the prototype's order -- 64 samples, an 8 x 8 image, two units, db2, cdf9/7,
  L = 2 -- as (name, value) pairs.  A value in capitals names something the runner supplies: CTX the context, B0 / B1 two distinct
  data buffers (16 KiB each: more than any base set describes), RES a HOST array of doubles, DRES a data buffer for doubles,
  QMF the db2 filter, NSTEPS / IU / NC / SH / CF / NORM1 / NORM2 the flattened cdf9/7 scheme, BADNC a coefficient-count array
  whose first entry is 0, TREE the HOST tree of a 2-level dwt of 64 samples, BADTREE one with a node set below an unset node,
  TREEOUT a HOST array of 63 bytes.  A tuple of integers is an int64 array.
- rules: in the order the entry point applies them, (status, [breaker, ...]).  A breaker is a dict of arguments that breaks that
  rule.  A row of the table is one breaker together with the first breaker of EVERY LATER rule (where two rules need the same
  argument the earlier rule's value stands), so that a rule checked out of order returns another status.  SCOPE marks where the entry
  point makes the context's device current: the rules behind it need a live context (rows marked live), the rules before it run
  on a block of zero bytes.

No row describes more data than the buffers hold, except the rows of wl_mad_batch's n >= 2^31 rule, which the host test sees
first.  The oversize rules of wl_denoise_ti_* (a side of 2^20 / more than 65535 columns) come behind the scope and have no row.

The statuses are what the library returned before the entry points were rewritten over wl_entry.h, checked against a reading
of that source.
"""
SCOPE = "SCOPE"

ARG, DTYPE, FILTER, EDIMS, EL, SIZE, ALIAS, CUBE, TREE_, SCHEME = (
    "WL_EINVAL_ARG", "WL_EINVAL_DTYPE", "WL_EINVAL_FILTER", "WL_EDIMS", "WL_EINVAL_L", "WL_EINVAL_SIZE", "WL_EALIAS", "WL_EINVAL_CUBE",
    "WL_EINVAL_TREE", "WL_EINVAL_SCHEME")

_SCH = [("nsteps", "NSTEPS"), ("step_is_update", "IU"), ("step_ncoef", "NC"), ("step_shift", "SH"), ("coefs_flat", "CF"),
        ("norm1", "NORM1"), ("norm2", "NORM2")]
# makescheme's rules, in its order
_SCH_RULES = [(SCHEME, [dict(nsteps=17), dict(nsteps=-1)]),
              (ARG, [dict(step_is_update=None), dict(step_ncoef=None), dict(step_shift=None), dict(coefs_flat=None)]),
              (SCHEME, [dict(step_ncoef="BADNC")])]


def _nulls(*names):
    return (ARG, [{n: None} for n in names])


_DT = (DTYPE, [dict(dtype=7), dict(dtype=-1)])
_FL = (FILTER, [dict(flen=1), dict(flen=65)])
_FL1 = (FILTER, [dict(flen=0), dict(flen=65)])

_DWTC = [("len", 64), ("nsignals", 2), ("ld", 64)]
_DWTC_RULES = [(EDIMS, [dict(len=0), dict(nsignals=0), dict(ld=63)]), (EL, [dict(L=-1)]), (SIZE, [dict(L=7)])]
# check_box behind the pointer rules: dims == NULL, ndims, an extent below 1, L, the power-of-two rule
_BOX_RULES = [_nulls("dims"), (EDIMS, [dict(ndims=0), dict(ndims=4), dict(dims=(0, 0))]), (EL, [dict(L=-1)]), (SIZE, [dict(L=4)])]
_TI_HEAD = [("ctx", "CTX"), ("dtype", 0), ("y", "B0"), ("x", "B1"), ("ndims", 2), ("dims", (8, 8))]
_TI_TAIL = [("L", 2), ("th", 0), ("t_unit", 1.0), ("nspin", (2, 2)), ("sigma_host", -1.0), ("stream", None)]
_TI_RULES = [(ARG, [dict(th=4), dict(th=-1)]), (ARG, [dict(sigma_host=float("nan")), dict(sigma_host=float("inf"), t_unit=0.0)]),
             (EDIMS, [dict(dims=(0, 0)), dict(nspin=(0, 1))]), (CUBE, [dict(dims=(8, 4))]), (EL, [dict(L=-1)]), (SIZE, [dict(L=4)]),
             (ALIAS, [dict(y="B1")]), (ARG, [dict(t_unit=-1.0)])]

ENTRIES = [
    ("wl_dwt_filter",
     [("ctx", "CTX"), ("dtype", 0), ("y", "B0"), ("x", "B1"), ("ndims", 1), ("dims", (64,)), ("qmf", "QMF"), ("flen", 4), ("L", 2),
      ("fw", 1), ("stream", None)],
     [_nulls("ctx", "y", "x", "qmf"), _DT, _FL, _nulls("dims"), (EDIMS, [dict(ndims=0), dict(ndims=4), dict(dims=(0,))]),
      (EL, [dict(L=-1)]), (SIZE, [dict(L=7), dict(dims=(62,))]), (ALIAS, [dict(y="B1")]), SCOPE]),
    ("wl_dwt_lifting",
     [("ctx", "CTX"), ("dtype", 1), ("y", "B0"), ("ndims", 2), ("dims", (8, 8))] + _SCH + [("L", 2), ("fw", 1), ("stream", None)],
     [_nulls("ctx", "y"), _DT, (CUBE, [dict(ndims=2, dims=(8, 4))])] + _BOX_RULES + [SCOPE] + _SCH_RULES),
    ("wl_dwt_lifting_oop",
     [("ctx", "CTX"), ("dtype", 0), ("y", "B0"), ("x", "B1"), ("ndims", 2), ("dims", (8, 8))] + _SCH + [("L", 2), ("fw", 0), ("stream", None)],
     [_nulls("ctx", "y", "x"), _DT, (CUBE, [dict(ndims=2, dims=(8, 4)), dict(ndims=3, dims=(8, 8, 4))])] + _BOX_RULES + [SCOPE] + _SCH_RULES),
    ("wl_dwtc_filter",
     [("ctx", "CTX"), ("dtype", 0), ("y", "B0"), ("x", "B1")] + _DWTC + [("qmf", "QMF"), ("flen", 4), ("L", 2), ("fw", 1), ("stream", None)],
     [_nulls("ctx", "y", "x", "qmf"), _DT, _FL] + _DWTC_RULES + [(ALIAS, [dict(y="B1")]), SCOPE]),
    ("wl_dwtc_lifting",
     [("ctx", "CTX"), ("dtype", 0), ("y", "B0")] + _DWTC + _SCH + [("L", 2), ("fw", 1), ("stream", None)],
     [_nulls("ctx", "y"), _DT] + _DWTC_RULES + [SCOPE] + _SCH_RULES),
    ("wl_dwtc_lifting_oop",
     [("ctx", "CTX"), ("dtype", 1), ("y", "B0"), ("x", "B1")] + _DWTC + _SCH + [("L", 2), ("fw", 0), ("stream", None)],
     [_nulls("ctx", "y", "x"), _DT] + _DWTC_RULES + [SCOPE] + _SCH_RULES),
    ("wl_wpt_filter",
     [("ctx", "CTX"), ("dtype", 0), ("y", "B0"), ("x", "B1"), ("n", 64), ("qmf", "QMF"), ("flen", 4), ("tree", "TREE"), ("ntree", 63),
      ("fw", 1), ("stream", None)],
     [_nulls("ctx", "y", "x", "qmf", "tree"), _DT, _FL, (EDIMS, [dict(n=0)]), (ALIAS, [dict(y="B1")]),
      (TREE_, [dict(tree="BADTREE"), dict(ntree=62), dict(tree=None, ntree=0)]), SCOPE]),
    ("wl_wpt_lifting",
     [("ctx", "CTX"), ("dtype", 0), ("y", "B0"), ("n", 64)] + _SCH + [("tree", "TREE"), ("ntree", 63), ("fw", 1), ("stream", None)],
     [_nulls("ctx", "y", "tree"), _DT, (EDIMS, [dict(n=0)]), (TREE_, [dict(tree="BADTREE"), dict(ntree=62)]), SCOPE] + _SCH_RULES),
    ("wl_wpt_filter_full",
     [("ctx", "CTX"), ("dtype", 1), ("y", "B0"), ("x", "B1"), ("n", 64), ("qmf", "QMF"), ("flen", 4), ("L", 2), ("fw", 1), ("stream", None)],
     [_nulls("ctx", "y", "x", "qmf"), _DT, _FL, (EDIMS, [dict(n=0)]), (ALIAS, [dict(y="B1")]), (EL, [dict(L=-1), dict(L=7)]), SCOPE]),
    ("wl_wpt_lifting_full",
     [("ctx", "CTX"), ("dtype", 0), ("y", "B0"), ("n", 64)] + _SCH + [("L", 2), ("fw", 0), ("stream", None)],
     [_nulls("ctx", "y"), _DT, (EDIMS, [dict(n=0)]), (EL, [dict(L=-1), dict(L=7)]), SCOPE] + _SCH_RULES),
    ("wl_dwt_filter_batch",
     [("ctx", "CTX"), ("dtype", 0), ("y", "B0"), ("x", "B1"), ("dims", (8, 8)), ("nimages", 2), ("image_stride", 64), ("qmf", "QMF"),
      ("flen", 4), ("L", 2), ("fw", 1), ("stream", None)],
     [_nulls("ctx", "y", "x", "dims", "qmf"), _DT, _FL,
      (EDIMS, [dict(nimages=0), dict(dims=(0, 8)), dict(dims=(8, 0)), dict(image_stride=63)]), (EL, [dict(L=-1)]),
      (SIZE, [dict(L=4), dict(dims=(8, 4), L=3)]), (ALIAS, [dict(y="B1")]), SCOPE]),
    ("wl_dwt_lifting_batch",
     [("ctx", "CTX"), ("dtype", 0), ("y", "B0"), ("x", "B1"), ("dims", (8, 8)), ("nimages", 2), ("image_stride", 64)] + _SCH +
     [("L", 2), ("fw", 1), ("stream", None)],
     [_nulls("ctx", "y", "x", "dims"), _DT, (CUBE, [dict(dims=(8, 4))]), (EDIMS, [dict(nimages=0), dict(dims=(0, 0)), dict(image_stride=63)]),
      (EL, [dict(L=-1)]), (SIZE, [dict(L=4)])] + _SCH_RULES + [SCOPE]),
    ("wl_bestbasistree_filter",
     [("ctx", "CTX"), ("dtype", 0), ("x", "B1"), ("n", 64), ("qmf", "QMF"), ("flen", 4), ("tree", "TREE"), ("ntree", 63), ("et", 0),
      ("tree_out", "TREEOUT"), ("node_entropy", None), ("stream", None)],
     [_nulls("ctx", "x", "qmf", "tree", "tree_out"), _DT, (ARG, [dict(et=2), dict(et=-1)]), _FL, (EDIMS, [dict(n=0)]),
      (SIZE, [dict(n=63), dict(n=1)]), (TREE_, [dict(tree="BADTREE"), dict(ntree=62)]), SCOPE]),
    ("wl_complex_split",
     [("ctx", "CTX"), ("dtype", 0), ("planes", "B0"), ("plane_stride", 64), ("z", "B1"), ("n", 64), ("nunits", 2), ("unit_stride", 64),
      ("stream", None)],
     [_nulls("ctx", "planes", "z"), _DT, (EDIMS, [dict(n=0), dict(nunits=0), dict(unit_stride=63), dict(plane_stride=63)]), SCOPE]),
    ("wl_complex_merge",
     [("ctx", "CTX"), ("dtype", 1), ("z", "B0"), ("planes", "B1"), ("plane_stride", 64), ("n", 64), ("nunits", 2), ("unit_stride", 64),
      ("stream", None)],
     [_nulls("ctx", "z", "planes"), _DT, (EDIMS, [dict(n=0), dict(nunits=0), dict(unit_stride=63), dict(plane_stride=63)]), SCOPE]),
    # ---- wl_modwt.hip, wl_ext.hip: the older entry points enter the scope right behind ctx and dtype (ext_enter, wl_entry.h) ----
    ("wl_modwt",
     [("ctx", "CTX"), ("dtype", 0), ("out", "B0"), ("ldo", 64), ("x", "B1"), ("n", 64), ("qmf", "QMF"), ("flen", 4), ("L", 2), ("stream", None)],
     [_nulls("ctx"), _DT, SCOPE, _nulls("out", "x", "qmf"), _FL1, (EDIMS, [dict(n=0), dict(ldo=63)]), (SIZE, [dict(L=7)]),
      (EL, [dict(L=0), dict(L=-1)])]),
    ("wl_imodwt",
     [("ctx", "CTX"), ("dtype", 0), ("x", "B0"), ("xw", "B1"), ("ldw", 64), ("n", 64), ("ncols", 3), ("qmf", "QMF"), ("flen", 4),
      ("stream", None)],
     [_nulls("ctx"), _DT, SCOPE, _nulls("x", "xw", "qmf"), _FL1, (EDIMS, [dict(n=0), dict(ncols=0), dict(ldw=63)])]),
    ("wl_threshold",
     [("ctx", "CTX"), ("dtype", 0), ("x", "B0"), ("n", 64), ("th", 0), ("t", 1.0), ("t_is_f64", 0), ("stream", None)],
     [_nulls("ctx"), _DT, SCOPE, _nulls("x"), (ARG, [dict(th=6), dict(th=-1)]), (ARG, [dict(t=-1.0), dict(t=float("nan"))])]),
    ("wl_threshold_biggest",
     [("ctx", "CTX"), ("dtype", 0), ("x", "B0"), ("n", 64), ("m", 8), ("stream", None)],
     [_nulls("ctx"), _DT, SCOPE, (ARG, [dict(x=None), dict(m=-1)])]),
    ("wl_median",
     [("ctx", "CTX"), ("dtype", 0), ("v", "B0"), ("n", 64), ("result", "RES"), ("stream", None)],
     [_nulls("ctx"), _DT, SCOPE, _nulls("v", "result"), (EDIMS, [dict(n=0)])]),
    ("wl_mad",
     [("ctx", "CTX"), ("dtype", 1), ("y", "B0"), ("n", 64), ("result", "RES"), ("stream", None)],
     [_nulls("ctx"), _DT, SCOPE, _nulls("y", "result"), (EDIMS, [dict(n=0)])]),
    ("wl_mad_batch",
     [("ctx", "CTX"), ("dtype", 0), ("y", "B0"), ("n", 64), ("nunits", 2), ("stride", 64), ("result", "DRES"), ("stream", None)],
     [_nulls("ctx", "y", "result"), _DT, (EDIMS, [dict(n=0), dict(nunits=0), dict(stride=63)]), (SIZE, [dict(n=1 << 31, stride=1 << 31)]),
      SCOPE]),
    ("wl_denoise_ti_filter",
     _TI_HEAD + [("qmf", "QMF"), ("flen", 4)] + _TI_TAIL,
     [_nulls("ctx"), _DT, SCOPE, _nulls("y", "x", "dims", "qmf", "nspin"), (EDIMS, [dict(ndims=0), dict(ndims=4)]), _FL] + _TI_RULES),
    ("wl_denoise_ti_lifting",
     _TI_HEAD + _SCH + _TI_TAIL,
     [_nulls("ctx"), _DT, SCOPE, _nulls("y", "x", "dims", "nspin"), (EDIMS, [dict(ndims=0), dict(ndims=4)])] + _TI_RULES + _SCH_RULES),
    ("wl_circshift",
     [("ctx", "CTX"), ("dtype", 0), ("b", "B0"), ("a", "B1"), ("ndims", 2), ("dims", (8, 8)), ("shift", (1, 2)), ("stream", None)],
     [_nulls("ctx"), _DT, SCOPE, _nulls("b", "a", "dims", "shift"), (EDIMS, [dict(ndims=0), dict(ndims=4)]), (ALIAS, [dict(b="B1")]),
      (EDIMS, [dict(dims=(8, -1))])]),
    ("wl_arrayadd",
     [("ctx", "CTX"), ("dtype", 0), ("y", "B0"), ("z", "B1"), ("n", 64), ("stream", None)],
     [_nulls("ctx"), _DT, SCOPE, (ARG, [dict(y=None), dict(z=None)])]),
    ("wl_rmul",
     [("ctx", "CTX"), ("dtype", 1), ("y", "B0"), ("n", 64), ("s", 0.5), ("stream", None)],
     [_nulls("ctx"), _DT, SCOPE, _nulls("y")]),
]


def rows():
    """[(id, symbol, [argument values in the prototype's order], status, live)]: one per breaker of every rule"""
    out = []
    for sym, base, rules in ENTRIES:
        names = [n for n, _ in base]
        live = False
        for k, rule in enumerate(rules):
            if rule == SCOPE:
                live = True
                continue
            status, breakers = rule
            later = {}
            for r in reversed(rules[k + 1:]):
                if r != SCOPE:
                    later.update(r[1][0])
            for j, br in enumerate(breakers):
                args = dict(base)
                args.update(later)
                args.update(br)
                assert set(br) <= set(names) and set(later) <= set(names), (sym, br)
                out.append(("%s-%d.%d-%s" % (sym, k, j, status), sym, [args[n] for n in names], status, live))
    return out
