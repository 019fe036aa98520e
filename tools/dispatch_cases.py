"""Which kernels does every level of the filter-bank dispatchers (filter_fwd_levels, filter_inv_levels) launch?  (GPU box)

One call per case, a fill of a marker tensor between the calls and `call k: label` on stdout: the protocol of
tools/count_launches.py.  Run it under a kernel trace alone and reduce it with the instances kept:

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/dispatch_cases.py > calls.txt
    python tools/count_launches.py <dir> calls.txt --instances > table.md

Two builds of the library dispatch alike when their tables are identical (profiles/dispatch_refactor.md).  A case the package
rejects prints its exception in the label, so both tables keep the same rows.  `--list` prints the labels without a GPU call.
"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavelets_jl_amd as W

F32, F64 = torch.float32, torch.float64
LIST_ONLY = "--list" in sys.argv[1:]
_k = 0
_mark = None


def jl(shape, dtype, misalign=0):
    """Julia-layout array; misalign = 1: one element off the 16-byte grid, as tests/test_gpu_robustness.py makes them"""
    if LIST_ONLY:
        return None
    n = 1
    for s in shape:
        n *= s
    t = torch.randn(n + 64, dtype=dtype, device="cuda")[misalign:misalign + n].view(*reversed(shape))
    return t.permute(*reversed(range(len(shape)))) if len(shape) > 1 else t


def call(label, fn):
    global _k, _mark
    if not LIST_ONLY:
        if _mark is None:
            _mark = torch.zeros(1024, device="cuda")
        torch.cuda.synchronize()
        _mark.fill_(float(_k))
        torch.cuda.synchronize()
        try:
            fn()
        except (W.DimensionMismatch, W.ArgumentError, TypeError) as e:     # an argument the package rejects: the row stays and says so
            label += " (%s)" % type(e).__name__                            # (a HIP error ends the run)
        torch.cuda.synchronize()
    print("call %d: %s" % (_k, label), flush=True)
    _k += 1


def depth(shape, nt):
    L = 0
    while all(s % (2 << L) == 0 for s in shape[:nt]):
        L += 1
    return L


def levels(shape, nt, which=(1, 2, 3, 0)):
    full = depth(shape, nt)
    return sorted({min(L, full) if L else full for L in which} - {0})


def both(label, shape, dtype, wname, L, misalign=0, nt=None):
    """dwt and idwt (dwtc / idwtc when only axis 0 of a matrix is transformed) of one array"""
    wt = W.wavelet(getattr(W.WT, wname))
    x = jl(shape, dtype, misalign)
    y = None if LIST_ONLY else (jl(shape, dtype, misalign) if misalign else W.similar(x))
    tag = "%s %s %s L=%d%s" % (label, "f32" if dtype == F32 else "f64", wname, L, " misaligned" if misalign else "")
    if nt == 1 and len(shape) == 2:
        call("dwtc " + tag, lambda: W.dwtc_(y, x, wt, L))
        call("idwtc " + tag, lambda: W.idwtc_(y, x, wt, L))
    else:
        call("dwt " + tag, lambda: W.dwt_oop_(y, x, wt, L))
        call("idwt " + tag, lambda: W.idwt_oop_(y, x, wt, L))


def squares():
    for dtype in (F32, F64):
        for wname in ("haar", "db2", "db4", "sym5", "db6", "db8", "db10", "coif8", "batt2", "batt6"):
            top = 2048 if wname in ("coif8", "batt2", "batt6") else (8192 if dtype == F32 else 4096)
            n = 8
            while n <= top:
                for L in levels((n, n), 2):
                    both("%d^2" % n, (n, n), dtype, wname, L)
                n *= 2
    both("8192^2", (8192, 8192), F64, "db4", 13)


def rectangles():
    for shape in ((2048, 1024), (1024, 2048), (4096, 2048), (2048, 4096), (1536, 1536), (768, 512), (1080, 1920), (1000, 1000), (7680, 4320),
                  (96, 96), (100, 60), (6, 10)):
        for dtype in (F32, F64):
            for wname in ("haar", "db4", "sym5", "db8"):
                for L in levels(shape, 2):
                    both("%dx%d" % shape, shape, dtype, wname, L)


def lines_and_columns():
    for dtype in (F32, F64):
        for wname in ("haar", "db4", "sym5", "db8"):
            for lg in (3, 6, 9, 10, 12, 13, 16, 20, 22, 24):
                for L in levels((1 << lg,), 1, (1, 2, 0)):
                    both("2^%d" % lg, (1 << lg,), dtype, wname, L)
            both("10^6", (1000000,), dtype, wname, 3)
            for shape in ((512, 32), (4096, 64), (65536, 64), (1024, 2048)):
                for L in levels(shape, 1, (1, 0)):
                    both("%dx%d columns" % shape, shape, dtype, wname, L, nt=1)
        # a leading dimension larger than the column length (a whole number of 16-byte vectors more, and an odd pitch), short and long
        # columns, few and many of them
        for wname in ("db4", "db8"):
            for n, ns, ld in ((4096, 64, 4104), (4096, 33, 4099), (1 << 16, 16, (1 << 16) + 8), (512, 48, 520), (1 << 20, 2, (1 << 20) + 4)):
                for fw in (1, 0):
                    call("%s %dx%d ld=%d %s %s L=%d" % ("dwtc" if fw else "idwtc", n, ns, ld, "f32" if dtype == F32 else "f64", wname, depth((n,), 1)),
                         lambda: pitched_columns(n, ns, ld, dtype, wname, depth((n,), 1), fw))


def pitched_columns(n, ns, ld, dtype, wname, L, fw):
    """wl_dwtc_filter through the raw ABI, as tests/test_gpu_robustness.py calls it: the host mirror only passes dense matrices"""
    import ctypes as C
    import numpy as np
    from wavelets_jl_amd import transforms as TR
    xs = torch.as_strided(torch.randn(ld * ns + 64, dtype=dtype, device="cuda"), (n, ns), (1, ld))
    ys = torch.as_strided(torch.empty(ld * ns + 64, dtype=dtype, device="cuda"), (n, ns), (1, ld))
    h, st = TR._context(xs.device)
    q = np.ascontiguousarray(W.wavelet(getattr(W.WT, wname)).qmf, dtype=np.float64)
    rc = W._lib.load().wl_dwtc_filter(h, TR._dtype_code(xs), C.c_void_p(ys.data_ptr()), C.c_void_p(xs.data_ptr()), n, ns, ld,
                                      q.ctypes.data_as(C.POINTER(C.c_double)), len(q), L, fw, st)
    if rc:
        raise RuntimeError("wl_dwtc_filter returned %d" % rc)


def volumes():
    for dtype in (F32, F64):
        for wname in ("haar", "db4", "db5", "db6"):             # 2, 8, 10 and 12 taps
            for shape in ((8,) * 3, (16,) * 3, (32,) * 3, (64,) * 3, (128,) * 3, (256,) * 3, (48, 40, 24)):
                for L in levels(shape, 3, (1, 0)):
                    both("%dx%dx%d" % shape, shape, dtype, wname, L)


def plane_batches():
    db4 = W.wavelet(W.WT.db4)
    for nb, n in ((64, 256), (8, 512), (4, 2048), (2, 4096)):
        for dtype in (F32, F64):
            x = jl((n, n, nb), dtype)
            y = None if LIST_ONLY else W.similar(x)
            for L in levels((n, n), 2, (2, 0)):
                call("dwt_batch %d x %d^2 %s L=%d" % (nb, n, dtype, L), lambda: W.dwt_batch(x, db4, L, y=y))
                call("idwt_batch %d x %d^2 %s L=%d" % (nb, n, dtype, L), lambda: W.idwt_batch(x, db4, L, y=y))
    for n, spins in ((256, (4, 4)), (2048, (8, 8))):
        x = jl((n, n), F32)
        for th in (W.HardTH(), W.SoftTH()):
            call("denoise TI %d^2 %dx%d spins %s" % (n, spins[0], spins[1], type(th).__name__),
                 lambda: W.denoise(x, dnt=W.VisuShrink(th, 3.0), TI=True, nspin=spins))


def misaligned():
    for dtype in (F32, F64):
        for shape in ((256, 256), (1024, 1024), (4096, 4096), (1 << 16,)):
            both("x".join(map(str, shape)), shape, dtype, "db4", depth(shape, len(shape)), misalign=1)


# every option that switches a tier of either dispatcher, in dispatch order (forward, then inverse, then the tiers they share)
SWITCHES = (("WL_PAIR_BATCH", 0), ("WL_TILEB", 0), ("WL_TILEB_TALL", 0), ("WL_TILE", 0), ("WL_TILE_LONG", 0), ("WL_NO_MULTI2D", 1), ("WL_TAIL3", 0),
            ("WL_TAIL2", 0), ("WL_LONG_TAIL", 0), ("WL_NO_MULTI", 1), ("WL_LDS2D", 0), ("WL_FUSE2", 0), ("WL_FUSE4", 1), ("WL_LONG2D", 0),
            ("WL_NO_INVTAIL", 1), ("WL_INVLONG2D", 0), ("WL_INV_PAIR", 0), ("WL_TILE_INV", 0), ("WL_TILE_INV_LONG", 0), ("WL_NO_INV1D2", 1),
            ("WL_NO_INV2D", 1), ("WL_INV2D_PPL", 4), ("WL_NO_LONGF", 1), ("WL_NO_FAST3D", 1), ("WL_NO_INVFAST", 1), ("WL_GTILE", 0), ("WL_ANYAXIS", 0))
OPTION_SHAPES = ((64, 64), (256, 256), (1024, 1024), (2048, 2048), (4096, 4096), (8192, 8192), (1 << 16,), (1 << 22,), (64, 64, 64))


def option_shapes(tag):
    for shape in OPTION_SHAPES:
        for dtype in (F32, F64):
            for wname in ("db4", "db8"):
                both(tag + " " + "x".join(map(str, shape)), shape, dtype, wname, depth(shape, len(shape)))


def options_one_at_a_time():
    for key, val in SWITCHES:
        W.set_option(key, val)
        option_shapes("[%s=%d]" % (key, val))
        W.clear_options()
    W.set_kernel_path(1)
    option_shapes("[path=1]")
    W.set_kernel_path(0)


def options_cumulative():
    for key, val in SWITCHES:
        if key in ("WL_FUSE4", "WL_INV2D_PPL", "WL_TILEB_TALL"):     # (these pick a variant, they turn no tier off)
            continue
        W.set_option(key, val)
        option_shapes("[.. %s=%d]" % (key, val))
    W.clear_options()


if __name__ == "__main__":
    for part in (squares, rectangles, lines_and_columns, volumes, plane_batches, misaligned, options_one_at_a_time, options_cumulative):
        part()
    if not LIST_ONLY:
        torch.cuda.synchronize()
        _mark.fill_(float(_k))
        torch.cuda.synchronize()
