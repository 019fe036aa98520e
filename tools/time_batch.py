"""Batch of images: one batched chain of launches against B single transforms (GPU box).  Markdown rows.

    python tools/time_batch.py            orthogonal filter (db4): wl_dwt_filter_batch
    python tools/time_batch.py lifting    lifting scheme (cdf9/7): wl_dwt_lifting_batch, forward and inverse
    python tools/time_batch.py launches   one call of every lifting configuration, a torch fill between them: run it under
                                          `rocprofv3 --kernel-trace` and count the library's kernels between the fills
                                          (tools/count_launches.py)
    python tools/time_batch.py volumes    batch of volumes (db4, Float32, full depth): wl_dwt_filter_batch3 against the same number
                                          of single wl_dwt_filter calls, forward and inverse, rotating inputs
    python tools/time_batch.py denoise3d  W.denoise(cube, TI=True) with the default 8 x 8 x 8 spins, host wall time
    python tools/time_batch.py lifting_volumes    batch of cubes (cdf9/7, Float32, full depth): wl_dwt_lifting_batch3 against the same
                                          number of single wl_dwt_lifting_oop calls, forward and inverse, rotating inputs
    python tools/time_batch.py lifting_denoise3d  W.denoise(cube, cdf9/7 scheme, TI=True) with the default 8 x 8 x 8 spins, host wall time
    python tools/time_batch.py denoise_batch [reps [case ...]]   one W.denoise_batch call against the loop of single W.denoise calls
                                          over the units, host wall time, the two alternating; on a build without denoise_batch the
                                          loop alone (the baseline a user runs today)
    python tools/time_batch.py denoise_batch_launches   one batched call at two unit counts and the loop over the units, a torch
                                          fill between them (the inputs and warm calls of a case get an interval of their own), the
                                          timed cases and three 16-tap ones: run it under `rocprofv3 --kernel-trace` and count
                                          with `tools/count_launches.py <dir> calls.txt --all`
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


def t_stats(fns, reps=20):
    """median, min and max (us) of `reps` timed calls that rotate through `fns` (the same call on different inputs)"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for k, (a, b) in enumerate(ev):
        a.record(); fns[k % len(fns)](); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return statistics.median(ts), ts[0], ts[-1]


def volumes_table():
    db4 = W.wavelet(W.WT.db4)
    print("| volumes | L | direction | batch us (min .. max) | kernel | single calls in a loop us (min .. max) | speed-up |")
    print("|---|---|---|---|---|---|---|")
    for n, nb in ((32, 512), (64, 512), (128, 64)):
        L = W.maxtransformlevels(n)
        xs = [torch.randn(nb, n, n, n, dtype=torch.float32, device="cuda").permute(3, 2, 1, 0) for _ in range(3)]
        yb = W.similar(xs[0])
        cs = [W.dwt_batch(x, db4, L) for x in xs]                # coefficients: the inputs of the inverse
        y1 = W.similar(xs[0][..., 0])
        for name, fb, f1, ins in (("dwt", W.dwt_batch, W.dwt_oop_, xs), ("idwt", W.idwt_batch, W.idwt_oop_, cs)):
            batch = [(lambda x=x: fb(x, db4, L, y=yb)) for x in ins]
            def loop(x):
                for i in range(nb):
                    f1(y1, x[..., i], db4, L)
            singles = [(lambda x=x: loop(x)) for x in ins]
            tb = t_stats(batch, 21)
            kb = W.last_kernel()
            ts = t_stats(singles, 21)
            print(f"| {nb} x {n}^3 | {L} | {name} | {tb[0]:.1f} ({tb[1]:.1f} .. {tb[2]:.1f}) | {kb} | {ts[0]:.1f} ({ts[1]:.1f} .. {ts[2]:.1f}) | "
                  f"{ts[0] / tb[0]:.2f} |", flush=True)


def lifting_volumes_table():
    """runs on any build of the package: one without the batched transform of cubes (dwt_batch raises TypeError) fills the loop
    columns only"""
    cdf = W.wavelet(W.WT.cdf97, W.WT.Lifting)
    print("| volumes | L | direction | batch us (min .. max) | kernel | single calls in a loop us (min .. max) | speed-up |")
    print("|---|---|---|---|---|---|---|")
    for n, nb in ((32, 512), (64, 64), (128, 8)):
        L = W.maxtransformlevels(n)
        xs = [torch.randn(nb, n, n, n, dtype=torch.float32, device="cuda").permute(3, 2, 1, 0) for _ in range(3)]
        yb = W.similar(xs[0])
        y1 = W.similar(xs[0][..., 0])
        try:
            cs = [W.dwt_batch(x, cdf, L) for x in xs]            # coefficients: the inputs of the inverse
            have_batch = True
        except TypeError:
            cs = [W.similar(x) for x in xs]
            for c, x in zip(cs, xs):
                for i in range(nb):
                    W.dwt_oop_(c[..., i], x[..., i], cdf, L)
            have_batch = False
        for name, fb, f1, ins in (("dwt", W.dwt_batch, W.dwt_oop_, xs), ("idwt", W.idwt_batch, W.idwt_oop_, cs)):
            batch = [(lambda x=x: fb(x, cdf, L, y=yb)) for x in ins]
            def loop(x):
                for i in range(nb):
                    f1(y1, x[..., i], cdf, L)
            singles = [(lambda x=x: loop(x)) for x in ins]
            tb, kb = (t_stats(batch, 21), W.last_kernel()) if have_batch else (None, "-")
            ts = t_stats(singles, 21)
            bt = f"{tb[0]:.1f} ({tb[1]:.1f} .. {tb[2]:.1f})" if tb else "-"
            sp = f"{ts[0] / tb[0]:.2f}" if tb else "-"
            print(f"| {nb} x {n}^3 | {L} | {name} | {bt} | {kb} | {ts[0]:.1f} ({ts[1]:.1f} .. {ts[2]:.1f}) | {sp} |", flush=True)


def denoise3d_table(wt=None, cubes=((32, 7), (64, 7), (128, 5)), label="sym5"):
    """host wall time of the whole call (a synchronise before and after), median of `reps`; runs on any build of the package, so the
    same script times the per-spin host loop of an older build"""
    import time
    print("| cube | median ms (min .. max) | reps | kernel |")
    print("|---|---|---|---|")
    kw = {} if wt is None else {"wt": wt}
    for n, reps in cubes:
        xs = [W.to_device((torch.randn(n, n, n) * 0.05 + torch.linspace(0, 1, n)[:, None, None]).numpy().astype("float32")) for _ in range(2)]
        W.denoise(xs[0], TI=True, **kw)
        torch.cuda.synchronize()
        ts = []
        for k in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            W.denoise(xs[k % 2], TI=True, **kw)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        print(f"| {n}^3 Float32, {label}, L = {min(W.maxtransformlevels(n), 6)}, 512 spins | {statistics.median(ts):.2f} ({ts[0]:.2f} .. {ts[-1]:.2f}) | {reps} | "
              f"{W.last_kernel()} |", flush=True)


DENOISE_BATCH_CASES = (("1024 x 256^2 sym5", (256, 256, 1024), "sym5", False), ("64 x 2048^2 sym5", (2048, 2048, 64), "sym5", False),
                       ("4096 x 2^14 db4", (1 << 14, 4096), "db4", False), ("65536 x 2^10 db4", (1 << 10, 65536), "db4", False),
                       ("512 x 32^3 sym5", (32, 32, 32, 512), "sym5", False), ("256 x 256^2 cdf9/7 lifting", (256, 256, 256), "cdf97", True),
                       # few, very long units: the detail range (2^19 values) is past the LDS limit, the streaming MAD runs
                       ("8 x 2^20 db4", (1 << 20, 8), "db4", False))


def denoise_batch_table(reps=21, cases=None):
    """medians of `reps` repetitions on three rotating inputs, min .. max beside them: host wall time around a final synchronise,
    the batched call and the loop alternating in one run"""
    import time
    have_batch = hasattr(W, "denoise_batch")
    print("| batch (Float32) | denoise_batch ms (min .. max) | kernel | loop of W.denoise ms (min .. max) | speed-up |")
    print("|---|---|---|---|---|")
    for k, (label, shape, wname, lifting) in enumerate(DENOISE_BATCH_CASES):
        if cases and k not in cases:
            continue
        wt = W.wavelet(getattr(W.WT, wname), W.WT.Lifting) if lifting else W.wavelet(getattr(W.WT, wname))
        nb = shape[-1]
        ramp = torch.linspace(0, 1, shape[0], device="cuda").reshape((shape[0],) + (1,) * (len(shape) - 1))
        xs = [W.julia_layout(ramp + 0.05 * torch.randn(*shape, device="cuda")) for _ in range(3)]
        y = W.similar(xs[0])

        def loop(x):
            for i in range(x.shape[-1]):
                W.denoise(x[..., i], wt)

        def wall(f, x):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(x)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        batch = (lambda x: W.denoise_batch(x, wt, y=y)) if have_batch else None
        kb = "-"
        if have_batch:
            batch(xs[0])
            kb = W.last_kernel()
        loop(xs[0][..., :min(nb, 8)])
        tb, tl = [], []
        for r in range(reps):
            if have_batch:
                tb.append(wall(batch, xs[r % 3]))
            tl.append(wall(loop, xs[r % 3]))
        tb.sort(); tl.sort()
        bt = f"{statistics.median(tb):.3f} ({tb[0]:.3f} .. {tb[-1]:.3f})" if tb else "-"
        sp = f"{statistics.median(tl) / statistics.median(tb):.1f}" if tb else "-"
        print(f"| {label} | {bt} | {kb} | {statistics.median(tl):.3f} ({tl[0]:.3f} .. {tl[-1]:.3f}) | {sp} |", flush=True)
        del xs, y


def denoise_batch_launches():
    """the batched call at B = 8 and B = 32 units (the launch count must not depend on B) and the loop of W.denoise over 8 units"""
    mark = torch.zeros(1024, device="cuda")
    k = 0
    # (db8: 16 taps, the long-filter family that the batched level loops run unit after unit on images and cubes)
    extra = (("32 x 2^10 db8", (1 << 10, 32), "db8", False), ("32 x 64^2 db8", (64, 64, 32), "db8", False), ("32 x 32^3 db8", (32, 32, 32, 32), "db8", False))
    for label, shape, wname, lifting in DENOISE_BATCH_CASES + extra:
        wt = W.wavelet(getattr(W.WT, wname), W.WT.Lifting) if lifting else W.wavelet(getattr(W.WT, wname))
        torch.cuda.synchronize()
        mark.fill_(float(k))                                 # (the inputs and the warm calls of a case get an interval of their own)
        torch.cuda.synchronize()
        x = W.julia_layout(torch.randn(*shape[:-1], 32, device="cuda"))
        x8 = W.julia_layout(x[..., :8])
        y, y8 = W.similar(x), W.similar(x8)
        W.denoise_batch(x, wt, y=y)
        W.denoise(x8[..., 0], wt)
        torch.cuda.synchronize()
        print(f"call {k}: (inputs and warm calls, {label.split(' x ', 1)[1]})", flush=True)
        k += 1

        def loop():
            for i in range(8):
                W.denoise(x8[..., i], wt)

        unit = label.split(" x ", 1)[1]
        for lab, f in ((f"denoise_batch 32 x {unit}", lambda: W.denoise_batch(x, wt, y=y)), (f"denoise_batch 8 x {unit}", lambda: W.denoise_batch(x8, wt, y=y8)),
                       (f"loop of 8 W.denoise, {unit}", loop)):
            torch.cuda.synchronize()
            mark.fill_(float(k))
            torch.cuda.synchronize()
            f()
            torch.cuda.synchronize()
            print(f"call {k}: {lab}", flush=True)
            k += 1
    mark.fill_(float(k))
    torch.cuda.synchronize()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "filter"
    if mode == "denoise_batch":
        denoise_batch_table(int(sys.argv[2]) if len(sys.argv) > 2 else 21, [int(a) for a in sys.argv[3:]])
        sys.exit(0)
    if mode == "denoise_batch_launches":
        denoise_batch_launches()
        sys.exit(0)
    {"filter": filter_table, "lifting": lifting_table, "launches": lifting_launches, "volumes": volumes_table,
     "denoise3d": denoise3d_table, "lifting_volumes": lifting_volumes_table,
     "lifting_denoise3d": lambda: denoise3d_table(W.wavelet(W.WT.cdf97, W.WT.Lifting), ((32, 5), (64, 5)), "cdf9/7 (lifting)")}[mode]()
