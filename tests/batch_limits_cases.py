"""Shared by tests/test_batch_limits_host.py and tests/test_gpu_batch_limits.py: one row per place where a batched entry point splits
its units into several launches, groups or grid-stride sweeps, each with a batch just large enough to run the code behind the limit.

Inputs.  A batch has D = 61 distinct units, default_rng(seed + k).standard_normal(m), and unit u of the batch is distinct[u % 61];
per-unit parameters (thresholds, m, sigmas, trees) have period P = 7.  61 is coprime to 65535, 32767, 2^20, 65535 / 4 and to every
units-per-workgroup count of the LDS tiers (powers of two); 7 is coprime to all of them but 32767 = 7 * 31 * 151, the group of the
complex batches, which take no per-unit parameter.  So the unit behind every boundary differs from the unit that an offset wrong
by one group, launch or sweep would read (test_batch_limits_host.py asserts both).

References.  `unit_ref(row, oracle, W, ins)` is the reference of ONE unit: the CPU oracle's result for that unit with that unit's
parameters (for the best-basis search: the single device call, as test_gpu_bestbasis_batch.py does).  `build(row, oracle, W, B)`
runs it on the 61 distinct units -- 61 x 7 combinations where the call takes per-unit parameters -- and describes every buffer
of the call as (table, index, stride): unit u of the buffer is table[index[u]], `stride` elements from unit u - 1, everything
else (padding, rows behind n of a padded column, guard bands) a sentinel no call produces.  `tiled_host` / the GPU test's gather
expand that to the flat buffer.  test_batch_limits_host.py checks the expansion against the plain loop over the units.

LIMIT RULES restated from the launchers (wl_entry.h group_size / for_groups, wl_modwt.hip modwt_lds_shape, wl_select.h ext_blocks):
`crossing(row, cu)` returns (what runs over the limit, the limit) for a row, and the host test asserts the first exceeds the second.
"""
import numpy as np

import threshold_batch_cases as TC

D, P = 61, 7
GUARD = 64                                      # elements on either side of every buffer (keeps unit 0 16-byte aligned)
PAD = 3                                         # the padded variant: unit stride = unit length + 3
DT = {"f32": np.float32, "f64": np.float64}
SENT = {np.dtype(np.float32): TC.SENT[np.float32], np.dtype(np.float64): TC.SENT[np.float64], np.dtype(np.uint8): 0xA5,
        np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A}
IBITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64, np.dtype(np.uint8): np.uint8, np.dtype(np.int64): np.uint64}
CU_HOST = 256                                   # the host test's compute-unit count (an MI355X)


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view(IBITS[a.dtype])


def sentinel(dtype, shape):
    """an array of the sentinel's bit pattern"""
    dt = np.dtype(dtype)
    return np.full(shape, SENT[dt], dtype=IBITS[dt]).view(dt)


# ---- the launch rules, restated -----------------------------------------------------------------------------------------------
def group_size(nunits, limit, lower=0, limit_first=True, cap=8192 << 20, nbytes=lambda g: 0):
    G = nunits
    if limit_first and G > limit:
        G = limit
    if 1 <= lower < G:
        G = lower
    while G > 1 and nbytes(G) > cap:
        G = (G + 1) // 2
    return min(G, limit)


def ext_blocks(n, per_thread, cu):
    return max(1, min((n + 256 * per_thread - 1) // (256 * per_thread), cu * 16))


def modwt_lds_shape(n, nunits, vec, itemsize, cu):
    """(threads, grid, units per workgroup) of the LDS tier of the modwt family"""
    items = n // (16 // itemsize) if vec else n
    threads = min(max((items + 63) // 64 * 64, 256), 1024)
    upw = min(threads // items if items < threads else 1, nunits)
    grid = min((nunits + upw - 1) // upw, cu * 8)
    return threads, grid, upw


# ---- rows -----------------------------------------------------------------------------------------------------------------------
ROWS = []


def row(id, fn, kind, site, rule, nunits, dtype="f32", pad=0, opts=None, kernel=None, zero_sign=True, **kw):
    """nunits: a number, or a function of the compute-unit count (the grid-stride rows).  kernel: what wl_last_kernel names after the
    call (None: the call names no kernel -- wl_complex_split / wl_complex_merge).  zero_sign: compare
    bit patterns as they are; False: -0 == +0 (the rule of the call's own GPU test)."""
    ROWS.append(dict(id=id, fn=fn, kind=kind, site=site, rule=rule, nunits=nunits, dtype=dtype, pad=pad, opts=opts or {}, kernel=kernel,
                     zero_sign=zero_sign, **kw))


def both(id, *a, kernel=None, kernel_padded=None, aligned=False, **kw):
    """the dense row and the one with unit stride = unit length + 3 (kernel_padded: the unit bases leave the 16-byte grid there and
    some calls take another tier); aligned: also a row with unit stride = unit length + 4, which keeps the bases on that grid and
    the call on the dense row's tier"""
    row(id, *a, kernel=kernel, **kw)
    row(id + "-padded", *a, pad=PAD, kernel=kernel_padded or kernel, **kw)
    if aligned:
        row(id + "-padded4", *a, pad=4, kernel=kernel, **kw)


G16 = ("group", 65535)
B16 = 65535 + 5

# -- wl_api.hip: for_groups(.., 65535, ..) of the image / volume batches, copy_units
both("dwt_batch-8x8", "wl_dwt_filter_batch", "dwt_box", "wl_api.hip:dwt_filter_batch_impl", G16, 70000, dims=(8, 8), L=2, wname="db2",
     kernel="k_fwd_any")
both("idwt_batch-8x8", "wl_dwt_filter_batch", "dwt_box", "wl_api.hip:dwt_filter_batch_impl", G16, 70000, dims=(8, 8), L=2, wname="db2", fw=0,
     dtype="f64", kernel="k_inv_any")
both("dwt_batch3-4x4x4", "wl_dwt_filter_batch3", "dwt_box", "wl_api.hip:dwt_filter_batch3_impl", G16, B16, dims=(4, 4, 4), L=2, wname="haar",
     kernel="k_tail3_batch", kernel_padded="k_tail3", aligned=True)
both("dwt_batch3-copy", "wl_dwt_filter_batch3", "dwt_box", "wl_api.hip:copy_units", G16, B16, dims=(4, 4, 4), L=0, wname="haar", kernel="copy")
both("lifting_batch-8x8", "wl_dwt_lifting_batch", "lift_box", "wl_api.hip:wl_dwt_lifting_batch", G16, B16, dims=(8, 8), L=2, wname="cdf97",
     kernel="k_lift_axis_stream+lines")
row("lifting_batch3-8x8x8", "wl_dwt_lifting_batch3", "lift_box", "wl_api.hip:lifting_batch3_impl", G16, B16, dims=(8, 8, 8), L=2, wname="cdf97",
    inplace=True, kernel="k_lift_axis_stream+k_lift_short_lines_batch")
# -- the column batches: one box of len x nsignals and no split in the entry point.  65535 is what a kernel with the column in the
#    grid's second dimension would hold; the tail kernels these shapes take have one workgroup per column in the grid's x
COLS = ("columns", 65535)
both("dwtc_filter-64", "wl_dwtc_filter", "dwtc", "wl_api.hip:wl_dwtc_filter", COLS, 70000, n=64, L=3, wname="db2", kernel="k_tail2_fwd")
both("dwtc_lifting-64", "wl_dwtc_lifting", "dwtc", "wl_api.hip:wl_dwtc_lifting", COLS, 70000, n=64, L=3, wname="cdf97", lifting=True, inplace=True,
     kernel="k_tail_lift_reg", kernel_padded="k_lift_any", aligned=True)
both("dwtc_lifting_oop-64", "wl_dwtc_lifting_oop", "dwtc", "wl_api.hip:wl_dwtc_lifting_oop", COLS, 70000, n=64, L=3, wname="cdf97", lifting=True,
     dtype="f64", kernel="k_tail_lift_reg", kernel_padded="k_lift_any")
# -- wl_ext.hip: group_reserve(.., 65535, ..) of the denoise batches
both("denoise_filter-64", "wl_denoise_batch_filter", "denoise", "wl_ext.hip:denoise_batch_filter_impl", G16, B16, dims=(64,), L=3, wname="db2",
     th="hard", sigma_out=True, kernel="denoise_batch+k_mad_units_lds", zero_sign=False)
row("denoise_filter-64-sigma_in", "wl_denoise_batch_filter", "denoise", "wl_ext.hip:denoise_batch_filter_impl (sigma_in + u0, sigma_out + u0)",
    G16, B16, dims=(64,), L=3, wname="db2", th="soft", sigma_in=True, sigma_out=True, kernel="denoise_batch+sigma_in", zero_sign=False)
row("denoise_filter-64-L0", "wl_denoise_batch_filter", "denoise", "wl_ext.hip:denoise_batch_filter_impl (L = 0)", G16, B16, dims=(64,), L=0,
    wname="db2", th="hard", sigma_out=True, kernel="denoise_batch+k_mad_units_lds", zero_sign=False, dtype="f64")
both("denoise_filter-4x4", "wl_denoise_batch_filter", "denoise", "wl_ext.hip:denoise_batch_filter_impl", G16, B16, dims=(4, 4), L=2, wname="haar",
     th="soft", sigma_out=True, kernel="denoise_batch+k_mad_units_lds", zero_sign=False)
both("denoise_lifting-64", "wl_denoise_batch_lifting", "denoise", "wl_ext.hip:denoise_batch_lifting_impl", G16, B16, dims=(64,), L=3, wname="cdf97",
     lifting=True, th="hard", sigma_out=True, kernel="denoise_batch+k_mad_units_lds", zero_sign=False)
row("denoise_lifting-64-sigma_in", "wl_denoise_batch_lifting", "denoise", "wl_ext.hip:denoise_batch_lifting_impl (sigma_in + u0, sigma_out + u0)",
    G16, B16, dims=(64,), L=3, wname="cdf97", lifting=True, th="soft", sigma_in=True, sigma_out=True, kernel="denoise_batch+sigma_in",
    zero_sign=False)
row("denoise_lifting-64-L0", "wl_denoise_batch_lifting", "denoise", "wl_ext.hip:denoise_batch_lifting_impl (L = 0)", G16, B16, dims=(64,), L=0,
    wname="cdf97", lifting=True, th="hard", sigma_out=True, kernel="denoise_batch+k_mad_units_lds", zero_sign=False)
row("denoise_lifting-4x4", "wl_denoise_batch_lifting", "denoise", "wl_ext.hip:denoise_batch_lifting_impl", G16, B16, dims=(4, 4), L=2,
    wname="haar", lifting=True, th="soft", sigma_out=True, kernel="denoise_batch+k_mad_units_lds", zero_sign=False)
# -- wl_ext.hip: denoise_ti_batch_run: planes = units * spins in groups of at most 65535, cut into groups of even size.  9001 units of 8
#    spins are 72008 planes in two groups of 36004: the boundary falls inside unit 4500 (with 9000 units it would fall between two units)
both("denoise_ti_filter-planes", "wl_denoise_ti_batch_filter", "denoise", "wl_ext.hip:denoise_ti_batch_run (planes)", ("planes", 65535), 9001,
     dims=(16,), L=2, wname="db2", th="hard", nspin=(8,), sigma_out=True, kernel="denoise_ti_units+k_mad_units_lds", zero_sign=False)
row("denoise_ti_filter-units", "wl_denoise_ti_batch_filter", "denoise", "wl_ext.hip:denoise_ti_batch_run (units of the estimate)", ("planes", 65535),
    B16, dims=(16,), L=2, wname="db2", th="soft", nspin=(1,), sigma_out=True, kernel="denoise_ti_units+k_mad_units_lds", zero_sign=False)
row("denoise_ti_filter-units-sigma_in", "wl_denoise_ti_batch_filter", "denoise", "wl_ext.hip:denoise_ti_batch_run (sigma_in)", ("planes", 65535),
    B16, dims=(16,), L=2, wname="db2", th="hard", nspin=(1,), sigma_in=True, sigma_out=True, kernel="denoise_ti_units+sigma_in", zero_sign=False,
    dtype="f64")
# -- wl_select.h: ext_blocks clamps a grid over the elements of all planes of a group to cu_count * 16 workgroups, the rest by a grid-stride
#    loop that finds its plane (and the plane's unit, for sigma) by division: 36004 planes of 128 samples are 4501 workgroups of
#    k_ti_shift_units (four samples per thread) and of k_threshold_planes
row("denoise_ti_filter-planes-128", "wl_denoise_ti_batch_filter", "denoise", "wl_ext.hip:denoise_ti_batch_run (ext_blocks over a group's planes)",
    ("blocks", 16), 9001, dims=(128,), L=3, wname="db2", th="soft", nspin=(8,), sigma_out=True, kernel="denoise_ti_units+k_mad_units_lds",
    zero_sign=False)
both("denoise_ti_lifting-planes", "wl_denoise_ti_batch_lifting", "denoise", "wl_ext.hip:denoise_ti_batch_run (planes)", ("planes", 65535), 9001,
     dims=(16,), L=2, wname="cdf97", lifting=True, th="hard", nspin=(8,), sigma_out=True, kernel="denoise_ti_units+k_mad_units_lds",
     zero_sign=False)
row("denoise_ti_lifting-units", "wl_denoise_ti_batch_lifting", "denoise", "wl_ext.hip:denoise_ti_batch_run (units of the estimate)",
    ("planes", 65535), B16, dims=(16,), L=2, wname="cdf97", lifting=True, th="soft", nspin=(1,), sigma_out=True,
    kernel="denoise_ti_units+k_mad_units_lds", zero_sign=False)
# -- wl_api.hip: group_size(.., 65535, WL_WPT_BATCH_GROUP, ..) of the packet and best-basis batches
both("wpt_filter_batch-64", "wl_wpt_filter_batch", "wpt", "wl_api.hip:wpt_batch_impl", G16, B16, n=64, wname="db4", tree="partial",
     kernel="k_wpt_fwd_tail", kernel_padded="k_generic_filter_wpt", aligned=True)
row("iwpt_filter_batch-64", "wl_wpt_filter_batch", "wpt", "wl_api.hip:wpt_batch_impl", G16, B16, n=64, wname="db4", tree="partial", fw=0, dtype="f64",
    kernel="k_wpt_inv_tail")
both("wpt_lifting_batch-64", "wl_wpt_lifting_batch", "wpt", "wl_api.hip:wpt_batch_impl", G16, B16, n=64, wname="cdf97", lifting=True,
     tree="partial", inplace=True, kernel="k_tail_lift_reg", kernel_padded="k_generic_lift_wpt")     # (any padding: the generic kernels)
both("wpt_filter_batch_trees-64", "wl_wpt_filter_batch_trees", "wpt", "wl_api.hip:wpt_batch_impl (utrees + u0 * utstride)", G16, B16, n=64,
     wname="db4", tree="per-unit", kernel="k_wpt_fwd_tail", kernel_padded="k_generic_filter_wpt", aligned=True)
both("bestbasistree_batch-64", "wl_bestbasistree_filter_batch", "bestbasis", "wl_api.hip:bestbasis_batch_impl", G16, B16, n=64, wname="db4",
     et="ShannonEntropy", kernel="k_entropy_seg")
# -- wl_api.hip: group_reserve(.., 32767, ..) of the complex batches; wl_complex.hip: the u0 += 65535 loops of split and merge
both("dwt_filter_complex-16", "wl_dwt_filter_complex", "cdwt", "wl_api.hip:dwt_filter_complex_impl", ("group", 32767), 32767 + 5, n=16, L=2,
     wname="db2", kernel="k_tail2_fwd")
both("dwt_lifting_complex-16", "wl_dwt_lifting_complex", "cdwt", "wl_api.hip:dwt_lifting_complex_impl", ("group", 32767), 32767 + 5, n=16, L=2,
     wname="cdf97", lifting=True, dtype="f64", kernel="k_tail_lift_reg")
row("dwt_filter_complex-copy", "wl_dwt_filter_complex", "cdwt", "wl_api.hip:copy_units", G16, B16, n=16, L=0, wname="db2", kernel="copy")
both("complex_split-16", "wl_complex_split", "csplit", "wl_complex.hip:complex_split", G16, B16, n=16)
both("complex_merge-16", "wl_complex_merge", "cmerge", "wl_complex.hip:complex_merge", G16, B16, n=16, dtype="f64")
# -- wl_modwt.hip, per-level tier (WL_MODWT_FUSED = 0): group_size(.., 65535, ..); 65535 / ncols for the analysis
STEP = {"WL_MODWT_FUSED": 0}
both("modwt_batch-step", "wl_modwt_batch", "modwt", "wl_modwt.hip:modwt_batch_impl", G16, B16, n=8, L=3, wname="db2", opts=STEP,
     kernel="k_modwt_step_b", aligned=True)
both("imodwt_batch-step", "wl_imodwt_batch", "imodwt", "wl_modwt.hip:imodwt_batch_impl", G16, B16, n=8, ncols=4, wname="db2", opts=STEP,
     kernel="k_imodwt_step_b", aligned=True)
both("modwt_mra_batch-step", "wl_modwt_mra_batch", "mra", "wl_modwt.hip:modwt_mra_batch_impl", ("group", 65535 // 4), 65535 // 4 + 5, n=8, ncols=4,
     wname="db2", opts=STEP, kernel="k_modwt_mra_step_b", zero_sign=False, aligned=True)
# -- wl_modwt.hip, LDS tier: the grid is clamped to cu_count * 8 workgroups of upw units, the rest by a grid-stride loop.  n = 8: many
#    units per workgroup (128 with 16-byte accesses, 32 element-wise); n = 1024 dense / 256 padded: one unit per workgroup
SWEEP = ("sweep", None)


def _lds_units(n, vec, planes=1, itemsize=4):
    """one full sweep of the clamped grid, one more workgroup and five units (in planes for the analysis)"""
    def f(cu):
        upw = modwt_lds_shape(n, 1 << 40, vec, itemsize, cu)[2]
        return (cu * 8 * upw + upw + 5 + planes - 1) // planes + 1
    return f


for _n, _np, _tag in ((8, 8, "many"), (1024, 256, "one")):
    row("modwt_batch-lds-" + _tag, "wl_modwt_batch", "modwt", "wl_modwt.hip:modwt_lds_shape / k_modwt_lds", SWEEP, _lds_units(_n, True), n=_n, L=3,
        wname="db2", kernel="k_modwt_lds")
    row("modwt_batch-lds-%s-padded" % _tag, "wl_modwt_batch", "modwt", "wl_modwt.hip:modwt_lds_shape / k_modwt_lds", SWEEP, _lds_units(_np, False),
        n=_np, L=3, wname="db2", kernel="k_modwt_lds", pad=PAD)
    row("imodwt_batch-lds-" + _tag, "wl_imodwt_batch", "imodwt", "wl_modwt.hip:modwt_lds_shape / k_imodwt_lds", SWEEP, _lds_units(_n, True), n=_n,
        ncols=4, wname="db2", kernel="k_imodwt_lds")
    row("imodwt_batch-lds-%s-padded" % _tag, "wl_imodwt_batch", "imodwt", "wl_modwt.hip:modwt_lds_shape / k_imodwt_lds", SWEEP,
        _lds_units(_np, False), n=_np, ncols=4, wname="db2", kernel="k_imodwt_lds", pad=PAD)
    row("modwt_mra_batch-lds-" + _tag, "wl_modwt_mra_batch", "mra", "wl_modwt.hip:modwt_lds_shape / k_modwt_mra_lds", SWEEP,
        _lds_units(_n, True, planes=4), n=_n, ncols=4, wname="db2", kernel="k_modwt_mra_lds", zero_sign=False)
    row("modwt_mra_batch-lds-%s-padded" % _tag, "wl_modwt_mra_batch", "mra", "wl_modwt.hip:modwt_lds_shape / k_modwt_mra_lds", SWEEP,
        _lds_units(_np, False, planes=4), n=_np, ncols=4, wname="db2", kernel="k_modwt_mra_lds", zero_sign=False, pad=PAD)
# -- wl_thbatch.hip: k_threshold_batch, the unit in gridDim.y (u0 += 65535; units of more than 256 elements); the grid's x clamped so that
#    bx * nb stays below cu_count * 64
TH_T = (0.0, 0.3, 0.6, 0.9, 1.2, 1.5, 2.0)
row("threshold_batch-hard", "wl_threshold_batch", "threshold", "wl_thbatch.hip:threshold_batch_impl (t_dev + u0)", ("launch", 65535), B16, n=257,
    th="hard", kernel="k_threshold_batch", pad=PAD)
row("threshold_batch-soft", "wl_threshold_batch", "threshold", "wl_thbatch.hip:threshold_batch_impl (t_dev + u0)", ("launch", 65535), B16, n=257,
    th="soft", kernel="k_threshold_batch")
# -- wl_thbatch.hip / wl_ext.hip: 2^20 units per launch of the workgroup-per-unit kernels (u0 += 1 << 20)
M20 = ("launch", 1 << 20)
B20 = (1 << 20) + 5
for _dt in ("f32", "f64"):
    both("biggest-lds-" + _dt, "wl_threshold_biggest_batch", "biggest", "wl_thbatch.hip:biggest_batch_impl (md + u0) / k_thbig_lds", M20, B20,
         n=4, dtype=_dt, kernel="k_thbig_lds", ms=(0, 1, 2, 3, 4, 5, -1))
    both("biggest-stream-" + _dt, "wl_threshold_biggest_batch", "biggest", "wl_thbatch.hip:biggest_batch_impl (md + u0) / k_thbig_stream", M20,
         B20, n=4, dtype=_dt, kernel="k_thbig_stream", ms=(0, 1, 2, 3, 4, 5, -1), opts={"WL_THB_LDS_MAX": 0})
    both("mad_batch-lds-" + _dt, "wl_mad_batch", "mad", "wl_ext.hip:mad_units (result + u0) / k_mad_units_lds", M20, B20, n=4, dtype=_dt,
         kernel="k_mad_units_lds")
    both("mad_batch-stream-" + _dt, "wl_mad_batch", "mad", "wl_ext.hip:mad_units (result + u0) / k_mad_units_stream", M20, B20, n=4, dtype=_dt,
         kernel="k_mad_units_stream", opts={"WL_MAD_LDS_MAX": 0})
# -- wl_thbatch.hip: the split tier's group_reserve(.., 65535, ..)
both("biggest-split", "wl_threshold_biggest_batch", "biggest", "wl_thbatch.hip:biggest_batch_impl (split tier, md + u0)", G16, B16, n=128,
     kernel="k_thbig_split", ms=(0, 1, 17, 64, 100, 128, 200),
     opts={"WL_THB_LDS_MAX": 0, "WL_THB_SPLIT_N": 64, "WL_THB_SPLIT_UNITS": 1 << 20, "WL_THB_CHUNK": 64})

BY_ID = {r["id"]: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

# limits that no cheap input crosses, and batched ABI functions that have no launch limit at all
UNREACHED = {
    "wl_thbatch.hip:threshold_batch_impl (k_threshold_batch_wave, u0 += 1 << 30)":
        "2^30 units of at least one element each: 4 GiB of Float32 and minutes of oracle tiling; the loop body is the one of the "
        "65535-unit loop behind it, which threshold_batch-hard / -soft run",
    "wl_ext.hip:denoise_ti_batch_run (sigma_in chunk of 65535 * 256 units)":
        "16.7 million units: the shifted planes of one pass alone exceed the device-data budget of a test by two orders of magnitude",
    "wl_ext.hip:ti_shift / ti_accumulate (gy > 65535 clamp of the single-call TI shift)":
        "needs more than 65535 * 8 columns per spin: an image of 65535 columns is refused (WL_EINVAL_SIZE) and a cube reaches it only "
        "from 725 per side, 1.5 GB per copy",
    "wl_shard_range": "host arithmetic on (nunits, rank, world): no launch, covered by tests/test_sharding_gloo.py and tests/test_abi.py",
}


def units_of(r, cu=CU_HOST):
    return int(r["nunits"](cu)) if callable(r["nunits"]) else int(r["nunits"])


def unit_len(r):
    return int(np.prod(r["dims"])) if "dims" in r else int(r["n"])


def is_vec(r):
    """16-byte accesses of the modwt family: every extent and stride a multiple of 16 bytes (the bases are, by GUARD)"""
    e = 16 // np.dtype(DT[r["dtype"]]).itemsize
    return r["n"] % e == 0 and r["pad"] % e == 0


def crossing(r, cu=CU_HOST):
    """(what the batch puts on the limited dimension, the limit): the first must exceed the second"""
    what, lim = r["rule"]
    B = units_of(r, cu)
    if what in ("group", "launch", "columns"):
        return B, lim
    if what == "planes":
        return B * int(np.prod(r["nspin"])), lim
    if what == "blocks":                                      # workgroups of 256 threads, four samples each, over one even group of planes
        planes = B * int(np.prod(r["nspin"]))
        group = -(-planes // -(-planes // 65535))
        return -(-(group * unit_len(r) // 4) // 256), cu * lim
    if what == "sweep":
        planes = B * (r["ncols"] if r["kind"] == "mra" else 1)
        _, grid, upw = modwt_lds_shape(r["n"], planes, is_vec(r), np.dtype(DT[r["dtype"]]).itemsize, cu)
        assert grid == cu * 8
        return planes, grid * upw
    raise KeyError(what)


# ---- inputs and references ---------------------------------------------------------------------------------------------------------
def distinct(m, dtype, seed):
    return np.stack([np.random.default_rng(seed + k).standard_normal(m) for k in range(D)]).astype(dtype)


def seed_of(r):
    return 1000 + 100 * [x["id"] for x in ROWS].index(r["id"])


def _wavelet(W, r):
    if r.get("lifting") or r["kind"] == "lift_box":
        return W.wavelet(getattr(W.WT, r["wname"]), W.WT.Lifting)
    return W.wavelet(getattr(W.WT, r["wname"]))


def _transform(oracle, wt, W):
    if isinstance(wt, W.OrthoFilter):
        return (lambda a, l: oracle.dwt_filter(a, wt.qmf, l)), (lambda a, l: oracle.dwt_filter(a, wt.qmf, l, fw=False))
    return (lambda a, l: oracle.dwt_lifting(a, wt, l)), (lambda a, l: oracle.dwt_lifting(a, wt, l, fw=False))


def _box(flat, dims):
    return np.ascontiguousarray(flat.reshape(dims, order="F"))


def _flat(a):
    return np.asfortranarray(a).reshape(-1, order="F")


def shared_tree(n):
    """one valid partial tree of an n-sample signal: the root and its left child split, then the left-left and the right child's left"""
    import bestbasis_ref as R
    nn = 2 ** R.maxtransformlevels(n) - 1
    t = np.zeros(nn, dtype=np.uint8)
    t[[0, 1, 3, 2, 5]] = 1
    return t


def unit_trees(n):
    """P valid trees, pairwise different"""
    import bestbasis_ref as R
    rng = np.random.default_rng(4242)
    out = []
    while len(out) < P:
        t = R.random_tree(rng, n, 0.5 + 0.07 * len(out))
        if not any(np.array_equal(t, o) for o in out):
            out.append(t)
    return np.stack(out)


def params_of(r):
    """{name: (P, k) table} of the per-unit parameters of a row (period P)"""
    k = r["kind"]
    if k == "threshold":
        return {"t": np.array(TH_T, dtype=np.float64).reshape(P, 1)}
    if k == "biggest":
        return {"m": np.array(r["ms"], dtype=np.int64).reshape(P, 1)}
    if k == "denoise" and r.get("sigma_in"):
        return {"sigma_in": np.array([0.05, 0.1, 0.2, 0.35, 0.5, 0.8, 1.25], dtype=np.float64).reshape(P, 1)}
    if k == "wpt" and r["tree"] == "per-unit":
        return {"trees": unit_trees(r["n"])}
    return {}


def inputs_of(r):
    """{name: (D, m) table} of the distinct input units of a row"""
    dt, k, s = DT[r["dtype"]], r["kind"], seed_of(r)
    if k in ("imodwt", "mra"):
        return {"xw": distinct(r["ncols"] * r["n"], dt, s)}
    if k in ("cdwt", "csplit"):
        return {"z": distinct(2 * r["n"], dt, s)}                  # (re, im) interleaved
    if k == "cmerge":
        return {"planes": distinct(2 * r["n"], dt, s)}             # re plane, im plane
    return {"x": distinct(unit_len(r), dt, s)}


def unit_ref(r, oracle, W, ins, par):
    """the reference of one unit: ins / par hold that unit's input rows and parameter rows; -> {name: 1-D array}"""
    k = r["kind"]
    dt = DT[r["dtype"]]
    if k in ("dwt_box", "lift_box"):
        wt = _wavelet(W, r)
        fwd, inv = _transform(oracle, wt, W)
        return {"y": _flat((fwd if r.get("fw", 1) else inv)(_box(ins["x"], r["dims"]), r["L"]))}
    if k == "dwtc":
        fwd, inv = _transform(oracle, _wavelet(W, r), W)
        return {"y": (fwd if r.get("fw", 1) else inv)(np.ascontiguousarray(ins["x"]), r["L"])}
    if k == "modwt":
        return {"out": np.ascontiguousarray(oracle.modwt(np.ascontiguousarray(ins["x"]), _wavelet(W, r).qmf, r["L"]).T).reshape(-1)}
    if k == "imodwt":
        co = ins["xw"].reshape(r["ncols"], r["n"])
        return {"x": oracle.imodwt(np.ascontiguousarray(co.T), _wavelet(W, r).qmf)}
    if k == "mra":
        import modwt_mra_cases as RC
        return {"out": RC.mra_of(oracle, _wavelet(W, r).qmf, np.ascontiguousarray(ins["xw"].reshape(r["ncols"], r["n"]))).reshape(-1)}
    if k == "threshold":
        return {"x": oracle.threshold(np.ascontiguousarray(ins["x"]), r["th"], float(par["t"][0]))}
    if k == "biggest":
        n = ins["x"].size
        return {"x": oracle.threshold(np.ascontiguousarray(ins["x"]), "biggest", m=min(max(int(par["m"][0]), 0), n))}
    if k == "mad":
        v = np.ascontiguousarray(ins["x"])
        med = v.dtype.type(oracle.median(v))
        return {"x": np.abs(v - med), "result": np.array([oracle.mad(v)], dtype=np.float64)}
    if k == "denoise":
        wt = _wavelet(W, r)
        fwd, inv = _transform(oracle, wt, W)
        x = _box(ins["x"], r["dims"])
        sig = float(par["sigma_in"][0]) if "sigma_in" in par else oracle.noisest(x, fwd)
        kw = dict(TI=True, nspin=tuple(r["nspin"])) if "nspin" in r else {}
        y = oracle.denoise(x, fwd, inv, r["L"], r["th"], t_unit(r), sigma=sig, **kw)
        return {"y": _flat(y), "sigma_out": np.array([sig], dtype=np.float64)}
    if k == "wpt":
        wt = _wavelet(W, r)
        tree = par["trees"] if "trees" in par else shared_tree(r["n"])
        f = oracle.wpt_lifting if r.get("lifting") else oracle.wpt_filter
        return {"y": f(np.ascontiguousarray(ins["x"]), wt if r.get("lifting") else wt.qmf, np.ascontiguousarray(tree).copy(), fw=bool(r.get("fw", 1)))}
    if k == "bestbasis":
        t, e = W.bestbasistree(W.to_device(np.ascontiguousarray(ins["x"])), _wavelet(W, r), None, getattr(W, r["et"])(), return_entropy=True)
        return {"trees_out": np.array(t, dtype=np.uint8), "node_entropy": e.cpu().numpy()}
    if k == "cdwt":
        z = ins["z"]
        if r["L"] == 0:
            return {"y": z.copy()}
        fwd, inv = _transform(oracle, _wavelet(W, r), W)
        f = fwd if r.get("fw", 1) else inv
        y = np.empty_like(z)
        y[0::2] = f(np.ascontiguousarray(z[0::2]), r["L"])
        y[1::2] = f(np.ascontiguousarray(z[1::2]), r["L"])
        return {"y": y}
    if k == "csplit":
        return {"planes": np.concatenate((ins["z"][0::2], ins["z"][1::2]))}
    if k == "cmerge":
        n = r["n"]
        z = np.empty(2 * n, dtype=dt)
        z[0::2], z[1::2] = ins["planes"][:n], ins["planes"][n:]
        return {"z": z}
    raise KeyError(k)


def t_unit(r):
    """dnt.t of the denoise rows.  The units are white noise: VisuShrink's sqrt(2 ln n) would zero nearly every coefficient and the
    results of most units would be the same zeros; 0.75 sigma keeps about half of them, so every unit has a result of its own"""
    return 0.75


def embed(table, cols, n, ld):
    """(K, cols * n) -> (K, cols * ld): every column in a leading dimension of ld, the rows behind n the sentinel"""
    if ld == n:
        return table
    K = table.shape[0]
    out = sentinel(table.dtype, (K, cols, ld))
    out[:, :, :n] = table.reshape(K, cols, n)
    return out.reshape(K, cols * ld)


def layout(r, name, table):
    """(table as it lies in memory, unit stride) of the buffer `name` of row r: a unit of a padded row is PAD elements further from
    the last, and the columns of a coefficient matrix / the planes of a complex unit have a leading dimension of their own there"""
    k, pad = r["kind"], r["pad"]
    m = table.shape[1]
    if name in ("t", "m", "sigma_in", "sigma_out", "result"):
        return table, m                                             # one value per unit, dense by the ABI
    if name in ("trees", "trees_out", "node_entropy"):
        return table, m + pad                                       # tree_stride / entropy_stride
    if (k, name) in (("modwt", "out"), ("imodwt", "xw"), ("mra", "xw"), ("mra", "out")):
        cols = r["L"] + 1 if k == "modwt" else r["ncols"]
        ld = r["n"] + pad
        return embed(table, cols, r["n"], ld), cols * ld + pad
    if (k, name) in (("csplit", "planes"), ("cmerge", "planes")):
        ps = r["n"] + (4 if pad else 0)                             # plane_stride (a multiple of 16 bytes either way)
        return embed(table, 2, r["n"], ps), 2 * ps
    if (k, name) in (("cdwt", "z"), ("cdwt", "y"), ("csplit", "z"), ("cmerge", "z")):
        return table, m + 2 * pad                                   # unit_stride counts complex values
    return table, m + pad


def build(r, oracle, W, B=None, cu=CU_HOST):
    """{name: dict(table, index, stride, role)} of every buffer of the call with B units (default: the row's), role in "in" (read
    only), "out" (written: table = expected), "inout" (in place: table_in = the input, table = expected), "param" """
    B = units_of(r, cu) if B is None else B
    ins, par = inputs_of(r), params_of(r)
    u = np.arange(B)
    iu, ip = u % D, u % P
    combos = [(a, b) for a in range(D) for b in range(P)] if par else [(a, 0) for a in range(D)]
    ic = iu * P + ip if par else iu
    refs = [unit_ref(r, oracle, W, {k: v[a] for k, v in ins.items()}, {k: v[b] for k, v in par.items()}) for a, b in combos]
    out = {}
    for name, tab in par.items():
        t, s = layout(r, name, tab)
        out[name] = dict(table=t, index=ip, stride=s, role="param")
    for name, tab in ins.items():
        t, s = layout(r, name, tab)
        out[name] = dict(table=t, index=iu, stride=s, role="in")
    for name in refs[0]:
        tab = np.stack([np.asarray(x[name]) for x in refs])
        t, s = layout(r, name, tab)
        if name in out:                                           # in place
            out[name] = dict(table=t, index=ic, stride=s, role="inout", table_in=out[name]["table"], index_in=out[name]["index"])
        else:
            out[name] = dict(table=t, index=ic, stride=s, role="out")
    if r.get("inplace"):                                          # y is x
        y = out.pop("y")
        out["x"] = dict(table=y["table"], index=y["index"], stride=y["stride"], role="inout", table_in=out["x"]["table"],
                        index_in=out["x"]["index"])
    return out


def tiled_host(table, index, stride):
    """the flat buffer [guard | unit 0 .. | unit B-1 .. | guard]: unit u = table[index[u]] at GUARD + u * stride, the rest the sentinel"""
    B, m = len(index), table.shape[1]
    buf = sentinel(table.dtype, 2 * GUARD + B * stride)
    buf[GUARD:GUARD + B * stride].reshape(B, stride)[:, :m] = table[index]
    return buf


def plain_loop(r, oracle, W, B):
    """{name: flat expected buffer} by the plain loop over the B units: unit u with its own input and parameters, one oracle call each"""
    ins, par = inputs_of(r), params_of(r)
    bufs = {}
    for u in range(B):
        ref = unit_ref(r, oracle, W, {k: v[u % D] for k, v in ins.items()}, {k: v[u % P] for k, v in par.items()})
        if r.get("inplace"):
            ref = {"x": ref["y"]}
        for name, val in ref.items():
            t, s = layout(r, name, np.asarray(val).reshape(1, -1))
            if name not in bufs:
                bufs[name] = (sentinel(t.dtype, 2 * GUARD + B * s), s)
            bufs[name][0][GUARD + u * s:GUARD + u * s + t.shape[1]] = t[0]
    return {k: v[0] for k, v in bufs.items()}
