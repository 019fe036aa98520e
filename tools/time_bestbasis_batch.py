"""Batched best-basis search against the loop of single searches (GPU box).  Markdown, written to profiles/bestbasis_batch.md with
--write (the resource table of that file is kept: everything from the line "## Timings" on is replaced).

    python tools/time_bestbasis_batch.py [--parent OTHER_LIB.so] [--reps R] [--write [--out FILE]]

batch     one wl_bestbasistree_filter_batch call over B units of n samples (full input tree, trees left on the device),
          synchronising after the call, against the loop of B wl_bestbasistree_filter calls (each returns its tree to the host and
          synchronises).  With --parent the loop runs in that library (a build without the batch entry points: what a user runs
          today), otherwise in the product library.  Wall-clock medians of R repetitions (the loops too) on inputs that rotate
          through rot(bytes) buffer sets: as many as it takes for the sets together to exceed the 256 MiB last-level cache, so
          that a set has been evicted before its turn comes again.
pipeline  search + wl_wpt_filter_batch_trees on the same batch, one synchronisation, against the loop of bestbasistree + wpt.
single    wl_wpt_filter at 2^22 with the dwt-shaped depth-9 tree and wl_bestbasistree_filter at 2^20 on the product library and on
          --parent, interleaved, the parent measured twice (two contexts) for its run-to-run spread.
Float32 db4 Shannon throughout."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import wavelets_jl_amd as W
from wavelets_jl_amd import _lib

LLC = 256 << 20


def rot(set_bytes):
    """input sets to rotate through: together more than the last-level cache (and at least 4)"""
    return max(4, (LLC + (32 << 20)) // set_bytes + 1)


vp = C.c_void_p
u8p = C.POINTER(C.c_uint8)
OUT = []


def emit(s=""):
    print(s, flush=True)
    OUT.append(s)


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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def batch_table(lib, plib, reps):
    q = np.ascontiguousarray(W.wavelet(W.WT.db4).qmf, dtype=np.float64)
    qp = q.ctypes.data_as(C.POINTER(C.c_double))
    h, ph = new_ctx(lib), new_ctx(plib)
    emit("| B x n | batch search us | padded batch (unit_stride n + 4) us | loop of B searches us | loop / batch | search + wpt_batch(trees) us | "
         "loop of search + wpt us | loop / pipeline |")
    emit("|---|---|---|---|---|---|---|---|")
    for B, n in ((4096, 1024), (64, 1 << 16), (16, 1 << 20)):
        Lmax = n.bit_length() - 1
        ntree = n - 1
        ROT = rot(4 * B * n)
        xs = [torch.randn(B * (n + 4), dtype=torch.float32, device="cuda") for _ in range(ROT)]
        y = torch.empty(B * n, dtype=torch.float32, device="cuda")
        trees = torch.zeros(B * ntree, dtype=torch.uint8, device="cuda")
        full = np.ones(ntree, dtype=np.uint8)
        host = np.zeros(ntree, dtype=np.uint8)
        k = [0]

        def search(S=n):
            i = k[0] % ROT
            assert lib.wl_bestbasistree_filter_batch(h, 0, vp(xs[i].data_ptr()), n, B, S, qp, len(q), None, 0, Lmax, 0, vp(trees.data_ptr()), ntree,
                                                     None, 0, stream()) == 0

        def fb():
            search(); k[0] += 1

        def fpad():                                          # the search copies a padded batch into dense buffers first
            search(n + 4); k[0] += 1

        def fp():
            i = k[0] % ROT
            search()
            assert lib.wl_wpt_filter_batch_trees(h, 0, vp(y.data_ptr()), vp(xs[i].data_ptr()), n, B, n, qp, len(q), vp(trees.data_ptr()), ntree, Lmax,
                                                 1, stream()) == 0
            k[0] += 1

        def fl(with_wpt):
            i = k[0] % ROT; k[0] += 1
            xp = xs[i].data_ptr()
            for u in range(B):
                assert plib.wl_bestbasistree_filter(ph, 0, vp(xp + 4 * u * n), n, qp, len(q), full.ctypes.data_as(u8p), ntree, 0,
                                                    host.ctypes.data_as(u8p), None, stream()) == 0
                if with_wpt:
                    assert plib.wl_wpt_filter(ph, 0, vp(y.data_ptr() + 4 * u * n), vp(xp + 4 * u * n), n, qp, len(q), host.ctypes.data_as(u8p), ntree,
                                              1, stream()) == 0

        fb(); fpad(); fp(); fl(True)
        nloop = reps
        tb = [wall(fb) for _ in range(reps)]
        tpad = [wall(fpad) for _ in range(reps)]
        tp = [wall(fp) for _ in range(reps)]
        tl = [wall(lambda: fl(False)) for _ in range(nloop)]
        tlp = [wall(lambda: fl(True)) for _ in range(nloop)]
        mb, mp, ml, mlp = (statistics.median(v) for v in (tb, tp, tl, tlp))
        emit(f"| {B} x {n} | {mb:.0f} | {statistics.median(tpad):.0f} | {ml:.0f} | {ml / mb:.1f} | {mp:.0f} | {mlp:.0f} | {mlp / mp:.1f} |")
        del xs, y, trees
    emit(f"(wall-clock medians of {reps} repetitions of each column, a batch call or a whole loop followed by one synchronisation; "
         f"the inputs rotate through sets that together exceed {LLC >> 20} MiB)")


def single_table(lib, plib, reps):
    q = np.ascontiguousarray(W.wavelet(W.WT.db4).qmf, dtype=np.float64)
    qp = q.ctypes.data_as(C.POINTER(C.c_double))
    hs = {"new": (lib, new_ctx(lib)), "parent": (plib, new_ctx(plib)), "parent again": (plib, new_ctx(plib))}
    emit("| case (db4, f32) | new us | parent us | parent again us | spread (parent vs itself) | new - parent |")
    emit("|---|---|---|---|---|---|")
    n22, n20 = 1 << 22, 1 << 20
    t9 = np.ascontiguousarray(W.maketree(n22, 9, "dwt"), dtype=np.uint8)
    full = np.ones(n20 - 1, dtype=np.uint8)
    host = np.zeros(n20 - 1, dtype=np.uint8)
    for label, n in (("wpt 2^22, dwt-shaped depth-9 tree (device events)", n22), ("bestbasistree 2^20 (wall clock, synchronises)", n20)):
        ROT = rot(4 * n)
        xs = [torch.randn(n, dtype=torch.float32, device="cuda") for _ in range(ROT)]
        y = torch.empty_like(xs[0])
        k = [0]

        def call(l, hh):
            i = k[0] % ROT; k[0] += 1
            if n == n22:
                rc = l.wl_wpt_filter(hh, 0, vp(y.data_ptr()), vp(xs[i].data_ptr()), n, qp, len(q), t9.ctypes.data_as(u8p), len(t9), 1, stream())
            else:
                rc = l.wl_bestbasistree_filter(hh, 0, vp(xs[i].data_ptr()), n, qp, len(q), full.ctypes.data_as(u8p), len(full), 0,
                                               host.ctypes.data_as(u8p), None, stream())
            assert rc == 0

        def timed(fn):
            if n != n22:
                return wall(fn)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) * 1e3

        t = {name: [] for name in hs}
        for name, (l, hh) in hs.items():
            for _ in range(10):
                call(l, hh)
        order = list(hs.items())
        for r in range(reps):
            for name, (l, hh) in order[r % 3:] + order[:r % 3]:      # (the build that goes first rotates round by round)
                t[name].append(timed(lambda: call(l, hh)))
        m = {name: statistics.median(v) for name, v in t.items()}
        emit(f"| {label} | {m['new']:.1f} | {m['parent']:.1f} | {m['parent again']:.1f} | {abs(m['parent'] - m['parent again']):.1f} | "
             f"{m['new'] - m['parent']:+.1f} |")
    emit(f"(medians of {reps} calls per build, the three interleaved call by call, the first of a round rotating; "
         f"inputs rotating through more than {LLC >> 20} MiB)")


if __name__ == "__main__":
    args = sys.argv[1:]
    parent, reps = None, 20
    if "--parent" in args:
        parent = args[args.index("--parent") + 1]
    if "--reps" in args:
        reps = int(args[args.index("--reps") + 1])
    lib = load(_lib.LIB_PATH)
    plib = load(parent) if parent else lib
    emit("## Timings")
    emit()
    emit("`python tools/time_bestbasis_batch.py --parent <library of the parent commit>` on one MI355X; Float32 db4, Shannon entropy, full input")
    emit("tree.  Loop and single-call baselines ran in " + ("the parent commit's library." if parent else "the product library itself."))
    emit()
    batch_table(lib, plib, reps)
    emit()
    emit("### Single calls: the cost of the extension")
    emit()
    single_table(lib, plib, max(reps, 60))
    if "--write" in args:
        path = os.path.join(ROOT, "profiles", "bestbasis_batch.md")
        head = open(path).read().split("## Timings")[0] if os.path.exists(path) else ""
        if "--out" in args:                                  # (another place for the same file)
            path = args[args.index("--out") + 1]
        open(path, "w").write(head + "\n".join(OUT) + "\n")
