"""Batched packet transform against the loop of single calls (GPU box).  Markdown rows.

    python tools/time_wpt_batch.py [--parent OTHER_LIB.so] [--reps R] [batch] [single]

batch    one wl_wpt_filter_batch / wl_wpt_lifting_batch call over B units of n samples against B calls of wl_wpt_filter_full /
         wl_wpt_lifting_full, the two alternating round by round, timed with device events on inputs that rotate through ROT buffer
         sets (cache-cold: together they exceed the last-level cache).  With --parent the loop runs in that library (a build
         without the batch entry points: the baseline a user runs today), otherwise in the product library.
single   the single-unit wpt rows of tools/time_wpt.py (2^22 depth 6, 2^18 full depth, the dwt-shaped tree at 2^22) on the product
         library and on --parent, interleaved, with the parent measured twice (two contexts) for the run-to-run spread.
Algorithmic GB/s = 2 * n * B * sizeof(T) per call."""
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavelets_jl_amd as W
from wavelets_jl_amd import _lib

ROT = 4
vp = C.c_void_p


def load(path):
    lib = C.CDLL(path)
    for nm, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, nm):
            fn = getattr(lib, nm)
            fn.restype, fn.argtypes = res, args
    return lib


def new_ctx(lib):
    h = vp()
    assert lib.wl_ctx_create(0, C.byref(h)) == 0
    return h


def stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


class Wavelet:
    def __init__(self, wt):
        self.wt = wt
        if isinstance(wt, W.OrthoFilter):
            self.q = np.ascontiguousarray(wt.qmf, dtype=np.float64)
        else:
            self.iu, self.nc, self.sh, self.cf = wt.flatten()

    def batch(self, lib, h, y, x, n, B, L, fw=1):
        if isinstance(self.wt, W.OrthoFilter):
            return lib.wl_wpt_filter_batch(h, 0, vp(y), vp(x), n, B, n, self.q.ctypes.data_as(C.POINTER(C.c_double)), len(self.q), None, 0, L, fw,
                                           stream())
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        return lib.wl_wpt_lifting_batch(h, 0, vp(y), vp(x), n, B, n, len(self.iu), ip(self.iu), ip(self.nc), ip(self.sh),
                                        self.cf.ctypes.data_as(C.POINTER(C.c_double)), self.wt.norm1, self.wt.norm2, None, 0, L, fw, stream())

    def single(self, lib, h, y, x, n, L, fw=1):
        """wpt!(y, x, filter, L) / wpt!(y, scheme, L) (in place on y: the copy of x is not part of the call, as in the reference)"""
        if isinstance(self.wt, W.OrthoFilter):
            return lib.wl_wpt_filter_full(h, 0, vp(y), vp(x), n, self.q.ctypes.data_as(C.POINTER(C.c_double)), len(self.q), L, fw, stream())
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        return lib.wl_wpt_lifting_full(h, 0, vp(y), n, len(self.iu), ip(self.iu), ip(self.nc), ip(self.sh),
                                       self.cf.ctypes.data_as(C.POINTER(C.c_double)), self.wt.norm1, self.wt.norm2, L, fw, stream())


def batch_table(lib, plib, reps):
    db4, cdf = Wavelet(W.wavelet(W.WT.db4)), Wavelet(W.wavelet(W.WT.cdf97, W.WT.Lifting))
    h, ph = new_ctx(lib), new_ctx(plib)
    print("| B x n | wavelet | depth | batch us | kernel | batch GB/s | loop of B single calls us | loop kernel | loop / batch |")
    print("|---|---|---|---|---|---|---|---|---|")
    cases = []
    for B, n in ((65536, 256), (4096, 1024), (1024, 4096), (64, 1 << 16), (16, 1 << 20)):
        Lmax = n.bit_length() - 1
        cases += [(B, n, db4, "db4", Lmax), (B, n, db4, "db4", 3)]
        if (B, n) in ((4096, 1024), (64, 1 << 16)):
            cases.append((B, n, cdf, "cdf9/7", Lmax))
    for B, n, wv, name, L in cases:
        xs = [torch.randn(B * n, dtype=torch.float32, device="cuda") for _ in range(ROT)]
        ys = [torch.randn(B * n, dtype=torch.float32, device="cuda") for _ in range(ROT)]
        es = 4
        lib.wl_ctx_reserve(h, lib.wl_workspace_bytes_full(0, 1, (C.c_int64 * 1)(B * n), L))
        plib.wl_ctx_reserve(ph, plib.wl_workspace_bytes_full(0, 1, (C.c_int64 * 1)(n), L))
        k = [0]

        def fb():
            i = k[0] % ROT; k[0] += 1
            assert wv.batch(lib, h, ys[i].data_ptr(), xs[i].data_ptr(), n, B, L) == 0

        def fl():
            i = k[0] % ROT; k[0] += 1
            yp, xp = ys[i].data_ptr(), xs[i].data_ptr()
            for u in range(B):
                wv.single(plib, ph, yp + u * n * es, xp + u * n * es, n, L)

        fb(); fl()
        tb, tl = [], []
        nloop = max(2, min(reps, 200000 // B))
        for r in range(reps):
            tb.append(timed(fb))
            if r < nloop:
                tl.append(timed(fl))
        kb = lib.wl_last_kernel(h).decode()
        kl = plib.wl_last_kernel(ph).decode()
        mb, ml = statistics.median(tb), statistics.median(tl)
        print(f"| {B} x {n} | {name} | {L} | {mb:.1f} | {kb} | {2 * n * B * es / mb / 1e3:.0f} | {ml:.1f} | {kl} | {ml / mb:.1f} |", flush=True)
        del xs, ys
    print(f"(medians of {reps} batch calls; the loop: min(reps, 200000 / B) rounds, at least 2; {ROT} rotating buffer sets)")


def single_table(lib, plib, reps):
    db4 = Wavelet(W.wavelet(W.WT.db4))
    hs = {"new": (lib, new_ctx(lib)), "parent": (plib, new_ctx(plib)), "parent again": (plib, new_ctx(plib))}
    print("| case (db4, f32) | new us | parent us | parent again us | spread (parent vs itself) | new - parent |")
    print("|---|---|---|---|---|---|")
    n22 = 1 << 22
    for label, n, L, tree in (("wpt 2^22 depth 6", n22, 6, None), ("wpt 2^18 full depth", 1 << 18, 18, None),
                              ("wpt 2^22 dwt-shaped tree, depth 22", n22, 0, W.maketree(n22, 22, "dwt"))):
        xs = [torch.randn(n, dtype=torch.float32, device="cuda") for _ in range(ROT)]
        y = torch.empty_like(xs[0])
        t8 = None if tree is None else np.ascontiguousarray(tree, dtype=np.uint8)
        qp = db4.q.ctypes.data_as(C.POINTER(C.c_double))
        k = [0]

        def call(l, h):
            i = k[0] % ROT; k[0] += 1
            if t8 is None:
                rc = l.wl_wpt_filter_full(h, 0, vp(y.data_ptr()), vp(xs[i].data_ptr()), n, qp, len(db4.q), L, 1, stream())
            else:
                rc = l.wl_wpt_filter(h, 0, vp(y.data_ptr()), vp(xs[i].data_ptr()), n, qp, len(db4.q), t8.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     len(t8), 1, stream())
            assert rc == 0

        t = {name: [] for name in hs}
        for name, (l, h) in hs.items():
            l.wl_ctx_reserve(h, l.wl_workspace_bytes_full(0, 1, (C.c_int64 * 1)(n), 22))
            for _ in range(10):
                call(l, h)
        order = list(hs.items())
        for r in range(reps):
            for name, (l, h) in order[r % 3:] + order[:r % 3]:      # (the build that goes first rotates round by round)
                t[name].append(timed(lambda: call(l, h)))
        m = {name: statistics.median(v) for name, v in t.items()}
        print(f"| {label} | {m['new']:.1f} | {m['parent']:.1f} | {m['parent again']:.1f} | {abs(m['parent'] - m['parent again']):.1f} | "
              f"{m['new'] - m['parent']:+.1f} |", flush=True)
    print(f"(medians of {reps} calls per build, the three interleaved call by call, the first of a round rotating; {ROT} rotating inputs)")


if __name__ == "__main__":
    args = sys.argv[1:]
    parent, reps = None, 20
    if "--parent" in args:
        parent = args[args.index("--parent") + 1]
    if "--reps" in args:
        reps = int(args[args.index("--reps") + 1])
    lib = load(_lib.LIB_PATH)
    plib = load(parent) if parent else lib
    print("product library:", _lib.LIB_PATH, "| loop / parent library:", parent or "(the same)")
    if "single" in args:
        single_table(lib, plib, max(reps, 60))
    if "batch" in args or "single" not in args:
        batch_table(lib, plib, reps)
