"""Batch of images: one batched chain of launches against B single transforms (GPU box).  Markdown rows.

    python tools/time_batch.py            orthogonal filter (db4): wl_dwt_filter_batch
    python tools/time_batch.py lifting    lifting scheme (cdf9/7): wl_dwt_lifting_batch, forward and inverse
    python tools/time_batch.py launches   one call of every lifting configuration, a torch fill between them: run it under
                                          `rocprofv3 --kernel-trace` and count the library's kernels between the fills
                                          (tools/count_launches.py)
"""
import os, sys, statistics
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavelets_jl_amd as W


def t_us(fn, reps=20):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def filter_table():
    db4 = W.wavelet(W.WT.db4)
    print("| images | L | batch us | kernel | B single calls us | speed-up | batch GB/s (algorithmic) | idwt batch us |")
    print("|---|---|---|---|---|---|---|---|")
    for n, nb, L in ((2048, 64, 4), (2048, 64, 11), (1024, 64, 4), (1024, 256, 10), (512, 256, 4), (512, 1024, 9), (256, 1024, 8)):
        xb = torch.randn(nb, n, n, dtype=torch.float32, device="cuda").permute(2, 1, 0)
        yb = W.similar(xb)
        zb = W.similar(xb)
        fb = lambda: W.dwt_batch(xb, db4, L, y=yb)
        tb = t_us(fb)
        kb = W.last_kernel()
        ti = t_us(lambda: W.idwt_batch(yb, db4, L, y=zb))
        ys = W.similar(xb[:, :, 0])
        def fs():
            for i in range(nb):
                W.dwt_oop_(ys, xb[:, :, i], db4, L)
        ts = t_us(fs, reps=5)
        gb = 2 * xb.numel() * 4 / tb / 1e3
        print(f"| {nb} x {n}^2 | {L} | {tb:.1f} | {kb} | {ts:.1f} | {ts / tb:.2f} | {gb:.0f} | {ti:.1f} |")


LIFTING_CASES = ((2048, 64, 4), (2048, 64, 11), (1024, 256, 10), (512, 1024, 9), (256, 1024, 8), (64, 4096, 6))


def lifting_table():
    cdf = W.wavelet(W.WT.cdf97, W.WT.Lifting)
    print("| images | L | batch us | kernel | B single calls us | speed-up | batch GB/s (algorithmic) | idwt batch us | idwt kernel | B single idwt calls us | idwt speed-up |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for n, nb, L in LIFTING_CASES:
        xb = torch.randn(nb, n, n, dtype=torch.float32, device="cuda").permute(2, 1, 0)
        yb = W.similar(xb)
        zb = W.similar(xb)
        W.reserve_workspace(xb, L, full=True)
        tb = t_us(lambda: W.dwt_batch(xb, cdf, L, y=yb))
        kb = W.last_kernel()
        ti = t_us(lambda: W.idwt_batch(yb, cdf, L, y=zb))
        ki = W.last_kernel()
        ys = W.similar(xb[:, :, 0])
        def fs():
            for i in range(nb):
                W.dwt_oop_(ys, xb[:, :, i], cdf, L)
        def fi():
            for i in range(nb):
                W.idwt_oop_(ys, yb[:, :, i], cdf, L)
        ts = t_us(fs, reps=5)
        tis = t_us(fi, reps=5)
        gb = 2 * xb.numel() * 4 / tb / 1e3
        print(f"| {nb} x {n}^2 | {L} | {tb:.1f} | {kb} | {ts:.1f} | {ts / tb:.2f} | {gb:.0f} | {ti:.1f} | {ki} | {tis:.1f} | {tis / ti:.2f} |", flush=True)


def lifting_launches():
    """one call per configuration, separated by fills of a marker tensor: the kernel trace holds, between fill k and fill k + 1, the
    launches of call k (printed here in the same order)"""
    cdf = W.wavelet(W.WT.cdf97, W.WT.Lifting)
    mark = torch.zeros(1024, device="cuda")
    k = 0
    for n, nb, L in LIFTING_CASES:
        small = max(2, nb // 4)
        xb = torch.randn(nb, n, n, dtype=torch.float32, device="cuda").permute(2, 1, 0)
        yb = W.similar(xb)
        W.reserve_workspace(xb, L, full=True)
        xs, ys = xb[:, :, :small], W.similar(xb[:, :, :small])
        x1, y1 = xb[:, :, 0], W.similar(xb[:, :, 0])
        for label, f in ((f"{nb} x {n}^2 L={L} dwt", lambda: W.dwt_batch(xb, cdf, L, y=yb)),
                         (f"{small} x {n}^2 L={L} dwt", lambda: W.dwt_batch(xs, cdf, L, y=ys)),
                         (f"1 x {n}^2 L={L} dwt (single)", lambda: W.dwt_oop_(y1, x1, cdf, L)),
                         (f"{nb} x {n}^2 L={L} idwt", lambda: W.idwt_batch(xb, cdf, L, y=yb)),
                         (f"{small} x {n}^2 L={L} idwt", lambda: W.idwt_batch(xs, cdf, L, y=ys)),
                         (f"1 x {n}^2 L={L} idwt (single)", lambda: W.idwt_oop_(y1, x1, cdf, L))):
            torch.cuda.synchronize()
            mark.fill_(float(k))
            torch.cuda.synchronize()
            f()
            torch.cuda.synchronize()
            print(f"call {k}: {label}", flush=True)
            k += 1
    mark.fill_(float(k))
    torch.cuda.synchronize()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "filter"
    {"filter": filter_table, "lifting": lifting_table, "launches": lifting_launches}[mode]()
