"""Every batched entry point with a batch that crosses a launch limit of its host code: the 65535 (32767 complex) units of a group,
the 2^20 units of a launch of the workgroup-per-unit kernels, the 65535 units of k_threshold_batch's grid, and the clamped grids of
the LDS tier of the modwt family with their grid-stride loop over units.  One test per row of tests/batch_limits_cases.py.

A row's buffers are built on the device by gather from the 61 distinct units (and the 7 distinct per-unit parameters) and so is
the expected content of every buffer the call writes -- the CPU oracle's result for each distinct unit, tiled -- with a sentinel in
the guard bands, the padding between units and the rows behind n of a padded column.  One comparison of integer bit patterns per
buffer therefore covers the units, the padding and the guards; the buffers the call only reads are compared with their own
content from before the call.  Rows of calls whose own tests compare by value (the denoise batches, the multiresolution analysis:
the sign of a zero is not part of their contract) map -0 to +0 on both sides first.  All calls go through ctypes on the context
of the Python mirror: the mirror has no unit strides for most of them, and one way of calling keeps the rows alike.
"""
import ctypes as C

import numpy as np
import pytest

import batch_limits_cases as BL

pytestmark = pytest.mark.gpu

CODE = {"f32": 0, "f64": 1}
TH = {"hard": 0, "soft": 1, "semisoft": 2, "stein": 3}


def tiled_device(torch, table, index, stride):
    """BL.tiled_host on the device"""
    B, m = len(index), table.shape[1]
    fill = int(np.array([BL.SENT[table.dtype]], dtype=BL.IBITS[table.dtype]).view({1: np.uint8, 4: np.int32, 8: np.int64}[table.dtype.itemsize])[0])
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8,
           np.dtype(np.int64): torch.int64}[table.dtype]
    idt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[table.dtype.itemsize]
    buf = torch.full((2 * BL.GUARD + B * stride,), fill, dtype=idt, device="cuda").view(tdt)
    t = torch.from_numpy(np.ascontiguousarray(table)).cuda()
    i = torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).cuda()
    buf[BL.GUARD:BL.GUARD + B * stride].view(B, stride)[:, :m] = t[i]
    return buf


def as_int(torch, t):
    return t.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


def first_differences(torch, got, want, stride):
    bad = torch.nonzero(as_int(torch, got) != as_int(torch, want)).flatten()[:6].cpu().tolist()
    return [("unit", (i - BL.GUARD) // stride, "element", (i - BL.GUARD) % stride) if i >= BL.GUARD else ("guard", i) for i in bad]


def same(torch, got, want, zero_sign):
    if not zero_sign and got.dtype.is_floating_point:       # by value: -0 == +0; every other pattern, the sentinel's included, as it is
        z = torch.zeros((), dtype=got.dtype, device=got.device)
        got, want = torch.where(got == 0, z, got), torch.where(want == 0, z, want)
    return torch.equal(as_int(torch, got), as_int(torch, want))


def ptr(t):
    return C.c_void_p(t.data_ptr() + BL.GUARD * t.element_size()) if t is not None else None


def f64p(t):
    return C.cast(ptr(t), C.POINTER(C.c_double)) if t is not None else None


def dims3(d):
    return (C.c_int64 * 3)(*(list(d) + [1] * (3 - len(d))))


def wavelet_args(W, r):
    """the filter or scheme arguments of the ABI, and what keeps them alive"""
    wt = BL._wavelet(W, r)
    if isinstance(wt, W.OrthoFilter):
        q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
        return [q.ctypes.data_as(C.POINTER(C.c_double)), len(q)], q
    iu, nc, sh, cf = wt.flatten()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    return [len(iu), ip(iu), ip(nc), ip(sh), cf.ctypes.data_as(C.POINTER(C.c_double)), wt.norm1, wt.norm2], (iu, nc, sh, cf)


def call(W, r, B, d, s, h, st):
    """the ABI call of row r on the device buffers d (by name; strides s)"""
    lib = W._lib.load()
    fn, k, code = getattr(lib, r["fn"]), r["kind"], CODE[r["dtype"]]
    wa, keep = wavelet_args(W, r) if "wname" in r else ([], None)
    fw = int(r.get("fw", 1))
    x = d.get("x")
    y = x if r.get("inplace") else d.get("y")
    if k in ("dwt_box", "lift_box"):
        return fn(h, code, ptr(y), ptr(x), dims3(r["dims"]), B, s["x"], *wa, r["L"], fw, st)
    if k == "dwtc":
        if r["fn"] == "wl_dwtc_lifting":
            return fn(h, code, ptr(x), r["n"], B, s["x"], *wa, r["L"], fw, st)
        return fn(h, code, ptr(y), ptr(x), r["n"], B, s["x"], *wa, r["L"], fw, st)
    if k == "modwt":
        ld = r["n"] + r["pad"]
        return fn(h, code, ptr(d["out"]), ld, s["out"], ptr(x), r["n"], B, s["x"], *wa, r["L"], st)
    if k == "imodwt":
        ld = r["n"] + r["pad"]
        return fn(h, code, ptr(x), s["x"], ptr(d["xw"]), ld, s["xw"], r["n"], r["ncols"], B, *wa, st)
    if k == "mra":
        ld = r["n"] + r["pad"]
        return fn(h, code, ptr(d["out"]), ld, s["out"], ptr(d["xw"]), ld, s["xw"], r["n"], r["ncols"], B, *wa, st)
    if k == "threshold":
        return fn(h, code, ptr(x), r["n"], B, s["x"], TH[r["th"]], 0.0, ptr(d["t"]), 1, st)
    if k == "biggest":
        return fn(h, code, ptr(x), r["n"], B, s["x"], 0, ptr(d["m"]), st)
    if k == "mad":
        return fn(h, code, ptr(x), r["n"], B, s["x"], f64p(d["result"]), st)
    if k == "denoise":
        spins = [dims3(r["nspin"])] if "nspin" in r else []
        return fn(h, code, ptr(y), ptr(x), len(r["dims"]), dims3(r["dims"]), B, s["x"], *wa, r["L"], TH[r["th"]], BL.t_unit(r), *spins,
                  f64p(d.get("sigma_in")), f64p(d.get("sigma_out")), st)
    if k == "wpt":
        if r["tree"] == "per-unit":
            import bestbasis_ref as R
            return fn(h, code, ptr(y), ptr(x), r["n"], B, s["x"], *wa, ptr(d["trees"]), s["trees"], R.maxtransformlevels(r["n"]), fw, st)
        tree = BL.shared_tree(r["n"])
        return fn(h, code, ptr(y), ptr(x), r["n"], B, s["x"], *wa, tree.ctypes.data_as(C.POINTER(C.c_uint8)), len(tree), 0, fw, st)
    if k == "bestbasis":
        import bestbasis_ref as R
        return fn(h, code, ptr(x), r["n"], B, s["x"], *wa, None, 0, R.maxtransformlevels(r["n"]), getattr(W, r["et"]).code, ptr(d["trees_out"]),
                  s["trees_out"], ptr(d["node_entropy"]), s["node_entropy"], st)
    if k == "cdwt":
        return fn(h, code, ptr(d["y"]), ptr(d["z"]), 1, dims3((r["n"],)), B, s["z"] // 2, *wa, r["L"], fw, st)
    if k == "csplit":
        return fn(h, code, ptr(d["planes"]), s["planes"] // 2, ptr(d["z"]), r["n"], B, s["z"] // 2, st)
    if k == "cmerge":
        return fn(h, code, ptr(d["z"]), ptr(d["planes"]), s["planes"] // 2, r["n"], B, s["z"] // 2, st)
    raise KeyError(k)


@pytest.mark.parametrize("rid", [r["id"] for r in BL.ROWS])
def test_batch_past_its_launch_limit(gpu, W, oracle, rid):
    """status 0, the kernel of the tier the row is there for, the bits of the tiled oracle results in every written buffer (padding
    and guard bands included), every read-only buffer unchanged"""
    import torch
    r = BL.BY_ID[rid]
    cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    B = BL.units_of(r, cu)
    over, limit = BL.crossing(r, cu)
    assert over > limit, (rid, over, limit)
    bufs = BL.build(r, oracle, W, B, cu)
    d, s, before = {}, {}, {}
    for name, b in bufs.items():
        s[name] = b["stride"]
        if b["role"] == "out":
            d[name] = tiled_device(torch, BL.sentinel(b["table"].dtype, (1, b["table"].shape[1])), np.zeros(B, dtype=np.int64), b["stride"])
        elif b["role"] == "inout":
            d[name] = tiled_device(torch, b["table_in"], b["index_in"], b["stride"])
        else:
            d[name] = tiled_device(torch, b["table"], b["index"], b["stride"])
            before[name] = d[name].clone()
    h, st = W.transforms._context(gpu)
    with W.options(**r["opts"]):
        rc = call(W, r, B, d, s, h, st)
        kernel = W.last_kernel()
    torch.cuda.synchronize()
    print(rid, "units", B, "over", over, "limit", limit, "kernel", kernel)
    assert rc == 0, (rid, W._lib.STATUS.get(rc, rc))
    assert r["kernel"] is None or kernel == r["kernel"], (rid, kernel)
    for name, b in bufs.items():
        if name in before:
            assert same(torch, d[name], before[name], True), (rid, name, "a read-only buffer was written", first_differences(torch, d[name], before[name], b["stride"]))
            continue
        want = tiled_device(torch, b["table"], b["index"], b["stride"])
        assert same(torch, d[name], want, r["zero_sign"]), (rid, name, kernel, B, first_differences(torch, d[name], want, b["stride"]))
        del want
