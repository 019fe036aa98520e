"""Device timings of the 2-D packet transforms (wpt2 / iwpt2): python tools/time_wpt2.py  (GPU box).  Markdown rows.

Every timed call runs on the next of a ring of (x, y) pairs whose footprint exceeds the 256 MiB last-level cache, so no call
finds its input resident; times are medians of device-event intervals, with the quartiles as the in-run spread.

The comparator is the best loop a caller can write without wpt2: per depth, gather the 4^d nodes into an m0 x m1 x 4^d array,
dwt_batch(., wt, 1), scatter back (the inverse: the depths upwards with idwt_batch).  It uses nothing this transform added.
"""
import os, sys, statistics
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavelets_jl_amd as W

RING_BYTES = 320 << 20
REPS = 24


def ring(n0, n1, dtype=torch.float32):
    per = 2 * n0 * n1 * torch.empty((), dtype=dtype).element_size()
    k = max(3, -(-RING_BYTES // per))
    g = torch.Generator(device="cuda").manual_seed(n0 + n1)
    return [(torch.randn((n1, n0), generator=g, dtype=dtype, device="cuda").t(), torch.empty((n1, n0), dtype=dtype, device="cuda").t())
            for _ in range(k)]


def t_us(fn, pairs, reps=REPS, warm=4):
    """fn(y, x) on the ring's pairs in rotation: (median, lower quartile, upper quartile) in microseconds"""
    k = len(pairs)
    for i in range(warm):
        fn(pairs[i % k][1], pairs[i % k][0])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (a, b) in enumerate(ev):
        y, x = pairs[(warm + i) % k][1], pairs[(warm + i) % k][0]
        a.record(); fn(y, x); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return statistics.median(ts), ts[len(ts) // 4], ts[(3 * len(ts)) // 4]


def nodes_view(a, d):
    """the n0 x n1 image as (i, j, bi, bj): element (i, j) of node (bi, bj) of depth d"""
    n0, n1 = a.shape
    nb = 1 << d
    return a.view(nb, n0 >> d, nb, n1 >> d).permute(1, 3, 0, 2)


def loop_transform(y, x, wt, L, fw):
    """the caller's loop: one gather, one batched single-level transform and one scatter per depth"""
    n0, n1 = x.shape
    cur = x
    for d in (range(L) if fw else range(L - 1, -1, -1)):
        nb = 1 << d
        batch = nodes_view(cur, d).reshape(n0 >> d, n1 >> d, nb * nb)
        out = (W.dwt_batch if fw else W.idwt_batch)(batch, wt, 1)
        nodes_view(y, d).copy_(out.view(n0 >> d, n1 >> d, nb, nb))
        cur = y
    return y


def fmt(t):
    return "%.1f (%.1f .. %.1f)" % t


def main():
    db4 = W.wavelet(W.WT.db4)
    print("| Float32 db4 | wpt2 us | kernel | iwpt2 us | kernel | loop wpt2 us | loop iwpt2 us |")
    print("|---|---|---|---|---|---|---|")
    for n0, n1, L in ((512, 512, 4), (2048, 2048, 3), (2048, 2048, 6), (8192, 8192, 2), (1080, 1920, 3)):
        pairs = ring(n0, n1)
        tf = t_us(lambda y, x: W.wpt2_(y, x, db4, L), pairs); kf = W.last_kernel()
        ti = t_us(lambda y, x: W.iwpt2_(y, x, db4, L), pairs); ki = W.last_kernel()
        lf = t_us(lambda y, x: loop_transform(y, x, db4, L, True), pairs, reps=20)
        li = t_us(lambda y, x: loop_transform(y, x, db4, L, False), pairs, reps=20)
        print(f"| {n0} x {n1} L{L} | {fmt(tf)} | {kf} | {fmt(ti)} | {ki} | {fmt(lf)} | {fmt(li)} |")
        del pairs
        torch.cuda.empty_cache()

    # one level pass over the whole image against its data floor of 2 n0 n1 sizeof(T) bytes (depth 0 alone, tail off)
    print()
    print("| one level pass, Float32 db4 | fwd us | GB/s | inv us | GB/s |")
    print("|---|---|---|---|---|")
    W.set_option("WL_WPT2_TAIL_MAX", 1)
    for n0, n1 in ((2048, 2048), (8192, 8192), (1080, 1920)):
        pairs = ring(n0, n1)
        tf = t_us(lambda y, x: W.wpt2_(y, x, db4, 1), pairs)
        ti = t_us(lambda y, x: W.iwpt2_(y, x, db4, 1), pairs)
        gb = 2 * n0 * n1 * 4 / 1e3
        print(f"| {n0} x {n1} | {fmt(tf)} | {gb / tf[0]:.0f} | {fmt(ti)} | {gb / ti[0]:.0f} |")
        del pairs
        torch.cuda.empty_cache()
    W.clear_options()

    # the largest node the tail takes: a shallow tree (the tail takes one depth at most) and a deep one (up to five)
    pairs = ring(2048, 2048)
    for L in (6, 9):
        print()
        print(f"| WL_WPT2_TAIL_MAX, 2048 x 2048 L{L} Float32 db4 | level passes + depths in the tail | wpt2 us | iwpt2 us |")
        print("|---|---|---|---|")
        for tmax in (1, 64, 256, 1024, 4096):
            W.set_option("WL_WPT2_TAIL_MAX", tmax)
            d = 0
            while d < L and (2048 >> d) ** 2 > tmax:
                d += 1
            tf = t_us(lambda y, x: W.wpt2_(y, x, db4, L), pairs)
            ti = t_us(lambda y, x: W.iwpt2_(y, x, db4, L), pairs)
            print(f"| {tmax} | {d} + {L - d} | {fmt(tf)} | {fmt(ti)} |")
    W.clear_options()


if __name__ == "__main__":
    main()
