"""Translation-invariant denoise of a batch: one W.denoise_ti_batch call against the loop of W.denoise(unit, wt, TI=True, nspin=...)
over the units (GPU box).  Markdown rows.

    python tools/time_ti_batch.py [table [reps [loop_units [case ...]]]]
        Float32, default L and threshold: medians of `reps` (20) repetitions on three rotating inputs, min .. max beside them, host
        wall time around a final synchronise, the batched call and the loop alternating in one run.  The loop is the protocol of
        `tools/time_batch.py denoise_batch`.  loop_units (0 = all): the loop runs over the first loop_units units only and its time
        is scaled by units / loop_units -- the loop is launch bound and linear in the units, and over 65536 units one pass takes
        seconds; the column says when a row was scaled.
    python tools/time_ti_batch.py launches
        one batched call at 32 and at 8 units and the loop over 8 units, a torch fill between them: run it under
        `rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/time_ti_batch.py launches > calls.txt` and count with
        `python tools/count_launches.py trace calls.txt --all`
    python tools/time_ti_batch.py batch_only case [reps]
        the batched call of one case alone, `reps` (5) times after a warm call: the run to put under
        `rocprofv3 --kernel-trace --stats` for the kernel times of that case
"""
import os, sys, statistics, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavelets_jl_amd as W

# (label, batch shape with the units last, wavelet, lifting, nspin)
CASES = (("65536 x 64 sym5, 8 spins", (64, 65536), "sym5", False, (8,)),
         ("4096 x 1024 sym5, 8 spins", (1024, 4096), "sym5", False, (8,)),
         ("1024 x 64^2 sym5, 8 x 8 spins", (64, 64, 1024), "sym5", False, (8, 8)),
         ("256 x 256^2 sym5, 8 x 8 spins", (256, 256, 256), "sym5", False, (8, 8)),
         ("64 x 32^3 sym5, 2 x 2 x 2 spins", (32, 32, 32, 64), "sym5", False, (2, 2, 2)),
         ("1024 x 64^2 cdf9/7 lifting, 8 x 8 spins", (64, 64, 1024), "cdf97", True, (8, 8)),
         ("16 x 64^2 sym5, 8 x 8 spins", (64, 64, 16), "sym5", False, (8, 8)),
         ("16 x 1024 sym5, 8 spins", (1024, 16), "sym5", False, (8,)))


def _wt(wname, lifting):
    return W.wavelet(getattr(W.WT, wname), W.WT.Lifting) if lifting else W.wavelet(getattr(W.WT, wname))


def _inputs(shape, count):
    ramp = torch.linspace(0, 1, shape[0], device="cuda").reshape((shape[0],) + (1,) * (len(shape) - 1))
    return [W.julia_layout(ramp + 0.05 * torch.randn(*shape, device="cuda")) for _ in range(count)]


def table(reps=20, loop_units=0, cases=None):
    print("| batch (Float32) | denoise_ti_batch ms (min .. max) | kernel | loop of W.denoise(TI=True) ms (min .. max) | loop measured over | loop / batch |")
    print("|---|---|---|---|---|---|")
    for k, (label, shape, wname, lifting, nspin) in enumerate(CASES):
        if cases and k not in cases:
            continue
        wt = _wt(wname, lifting)
        nb = shape[-1]
        nl = nb if loop_units <= 0 else min(nb, loop_units)
        xs = _inputs(shape, 3)
        y = W.similar(xs[0])

        def loop(x):
            for i in range(nl):
                W.denoise(x[..., i], wt, TI=True, nspin=nspin)

        def batch(x):
            W.denoise_ti_batch(x, wt, nspin=nspin, y=y)

        def wall(f, x):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(x)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        batch(xs[0])
        kb = W.last_kernel()
        for i in range(min(nb, 8)):
            W.denoise(xs[0][..., i], wt, TI=True, nspin=nspin)
        tb, tl = [], []
        for r in range(reps):
            tb.append(wall(batch, xs[r % 3]))
            tl.append(wall(loop, xs[r % 3]) * nb / nl)
        tb.sort(); tl.sort()
        over = "all units" if nl == nb else f"{nl} units, scaled by {nb // nl}"
        print(f"| {label} | {statistics.median(tb):.3f} ({tb[0]:.3f} .. {tb[-1]:.3f}) | {kb} | {statistics.median(tl):.3f} ({tl[0]:.3f} .. {tl[-1]:.3f}) | "
              f"{over} | {statistics.median(tl) / statistics.median(tb):.1f} |", flush=True)
        del xs, y


def launches():
    mark = torch.zeros(1024, device="cuda")
    k = 0
    for label, shape, wname, lifting, nspin in CASES[:6]:
        wt = _wt(wname, lifting)
        unit = label.split(" x ", 1)[1]
        torch.cuda.synchronize()
        mark.fill_(float(k))                                 # (the inputs and the warm calls of a case get an interval of their own)
        torch.cuda.synchronize()
        x = _inputs(shape[:-1] + (32,), 1)[0]
        x8 = W.julia_layout(x[..., :8])
        y, y8 = W.similar(x), W.similar(x8)
        W.denoise_ti_batch(x, wt, nspin=nspin, y=y)
        W.denoise(x8[..., 0], wt, TI=True, nspin=nspin)
        torch.cuda.synchronize()
        print(f"call {k}: (inputs and warm calls, {unit})", flush=True)
        k += 1

        def loop():
            for i in range(8):
                W.denoise(x8[..., i], wt, TI=True, nspin=nspin)

        for lab, f in ((f"denoise_ti_batch 32 x {unit}", lambda: W.denoise_ti_batch(x, wt, nspin=nspin, y=y)),
                       (f"denoise_ti_batch 8 x {unit}", lambda: W.denoise_ti_batch(x8, wt, nspin=nspin, y=y8)),
                       (f"loop of 8 W.denoise(TI=True), {unit}", loop)):
            torch.cuda.synchronize()
            mark.fill_(float(k))
            torch.cuda.synchronize()
            f()
            torch.cuda.synchronize()
            print(f"call {k}: {lab}", flush=True)
            k += 1
    mark.fill_(float(k))
    torch.cuda.synchronize()


def batch_only(case, reps=5):
    label, shape, wname, lifting, nspin = CASES[case]
    wt = _wt(wname, lifting)
    x = _inputs(shape, 1)[0]
    y = W.similar(x)
    for _ in range(reps + 1):
        W.denoise_ti_batch(x, wt, nspin=nspin, y=y)
    torch.cuda.synchronize()
    print(label, W.last_kernel())


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "table"
    if mode == "launches":
        launches()
    elif mode == "batch_only":
        batch_only(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    else:
        a = [int(v) for v in sys.argv[2:]]
        table(a[0] if a else 20, a[1] if len(a) > 1 else 0, a[2:])
