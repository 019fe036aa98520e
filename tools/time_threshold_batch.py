"""threshold_batch_ against what it replaces (GPU box).  Markdown tables; profiles/threshold_batch.md holds a run.

    python tools/time_threshold_batch.py rows [reps [loop_units]]
        BiggestTH with m = n / 10, Float32: one W.threshold_batch_ call against the loop of W.threshold_(unit, BiggestTH(), m) over the
        units.  Medians of `reps` (20) repetitions, min .. max beside them, host wall time around a final synchronise, the batched
        call and the loop alternating in one run.  The call works in place, so every repetition starts from a fresh copy of one of
        three rotating inputs (the copy is outside the timed window).  loop_units (256; 0 = all): the loop runs over the first
        loop_units units only and its time is scaled by units / loop_units -- it is one host round trip per unit and linear in the
        units; the column says when a row was scaled.
    python tools/time_threshold_batch.py cross [reps]
        the stream tier against the split tier (chunks of 16384 and of 65536 elements), forced through options, over n = 2^14 .. 2^22
        and B in {1, 16, 256}: where the default of WL_THB_SPLIT_N / WL_THB_SPLIT_UNITS comes from
    python tools/time_threshold_batch.py ew [reps]
        HardTH with one threshold per unit against W.threshold_ on the whole dense array with one threshold (the same bytes: the floor)
    python tools/time_threshold_batch.py all [reps]
"""
import os, sys, statistics, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavelets_jl_amd as W

ROWS = (("65536 x 64", (64, 65536)), ("4096 x 1024", (1024, 4096)), ("1024 x 256^2", (256, 256, 1024)), ("64 x 2048^2", (2048, 2048, 64)),
        ("16 x 2^20", (1 << 20, 16)))
EW = (("65536 x 64", (64, 65536)), ("4096 x 1024", (1024, 4096)), ("1024 x 256^2", (256, 256, 1024)), ("64 x 2048^2", (2048, 2048, 64)))
STREAM = {"WL_THB_LDS_MAX": 0, "WL_THB_SPLIT_N": 1 << 62}
SPLIT = {"WL_THB_LDS_MAX": 0, "WL_THB_SPLIT_N": 1, "WL_THB_SPLIT_UNITS": 1 << 40}


def _inputs(shape, count):
    return [W.julia_layout(torch.randn(*shape, device="cuda")) for _ in range(count)]


def _wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _fmt(ts):
    ts = sorted(ts)
    return f"{statistics.median(ts):.3f} ({ts[0]:.3f} .. {ts[-1]:.3f})"


def rows(reps=20, loop_units=256):
    print("| batch (Float32), BiggestTH, m = n / 10 | threshold_batch_ ms (min .. max) | kernel | loop of W.threshold_ ms (min .. max) | "
          "loop measured over | loop / batch |")
    print("|---|---|---|---|---|---|")
    for label, shape in ROWS:
        nb = shape[-1]
        n = 1
        for s in shape[:-1]:
            n *= s
        m = n // 10
        nl = nb if loop_units <= 0 else min(nb, loop_units)
        xs = _inputs(shape, 3)
        work = W.similar(xs[0])
        flat = work.reshape(-1) if work.dim() == 1 else torch.as_strided(work, (n, nb), (1, n))
        big = W.BiggestTH()

        def batch():
            W.threshold_batch_(work, big, m)

        def loop():
            for i in range(nl):
                W.threshold_(flat[:, i], big, m)

        work.copy_(xs[0]); batch(); kb = W.last_kernel()
        work.copy_(xs[0]); W.threshold_(flat[:, 0], big, m)
        tb, tl = [], []
        for r in range(reps):
            work.copy_(xs[r % 3]); tb.append(_wall(batch))
            work.copy_(xs[r % 3]); tl.append(_wall(loop) * nb / nl)
        over = "all units" if nl == nb else f"{nl} units, scaled by {nb // nl}"
        print(f"| {label} | {_fmt(tb)} | {kb} | {_fmt(tl)} | {over} | {statistics.median(tl) / statistics.median(tb):.1f} |", flush=True)
        del xs, work, flat


def cross(reps=20):
    print("| n | B | k_thbig_stream ms (min .. max) | k_thbig_split, chunk 16384, ms | k_thbig_split, chunk 65536, ms | stream / best split |")
    print("|---|---|---|---|---|---|")
    big = W.BiggestTH()
    for nb in (1, 16, 256):
        for e in range(14, 23):
            n = 1 << e
            xs = _inputs((n, nb), 3)
            work = W.similar(xs[0])
            res = []
            for opts, want in ((STREAM, "k_thbig_stream"), ({**SPLIT, "WL_THB_CHUNK": 16384}, "k_thbig_split"),
                               ({**SPLIT, "WL_THB_CHUNK": 65536}, "k_thbig_split")):
                with W.options(**opts):
                    work.copy_(xs[0]); W.threshold_batch_(work, big, n // 10)
                    assert W.last_kernel() == want, W.last_kernel()
                    ts = []
                    for r in range(reps):
                        work.copy_(xs[r % 3]); ts.append(_wall(lambda: W.threshold_batch_(work, big, n // 10)))
                    res.append(ts)
            best = min(statistics.median(res[1]), statistics.median(res[2]))
            print(f"| 2^{e} | {nb} | {_fmt(res[0])} | {_fmt(res[1])} | {_fmt(res[2])} | {statistics.median(res[0]) / best:.2f} |", flush=True)
            del xs, work


def ew(reps=20):
    print("| batch (Float32), HardTH | threshold_batch_, one t per unit, ms (min .. max) | W.threshold_ on the dense array, one t, ms (min .. max) | "
          "batch / dense | GB/s of the batch call (read + write) |")
    print("|---|---|---|---|---|")
    for label, shape in EW:
        nb = shape[-1]
        xs = _inputs(shape, 3)
        work = W.similar(xs[0])
        t = (0.5 + torch.rand(nb, device="cuda", dtype=torch.float64))
        hard = W.HardTH()
        work.copy_(xs[0]); W.threshold_batch_(work, hard, t); W.threshold_(work, hard, 1.0)
        tb, td = [], []
        for r in range(reps):
            work.copy_(xs[r % 3]); tb.append(_wall(lambda: W.threshold_batch_(work, hard, t)))
            work.copy_(xs[r % 3]); td.append(_wall(lambda: W.threshold_(work, hard, 1.0)))
        gbs = 2 * work.numel() * 4 / (statistics.median(tb) * 1e-3) / 1e9
        print(f"| {label} | {_fmt(tb)} | {_fmt(td)} | {statistics.median(tb) / statistics.median(td):.2f} | {gbs:.0f} |", flush=True)
        del xs, work


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("time_threshold_batch.py needs a HIP device: a timing without one says nothing")
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    W._lib.load()
    if what in ("rows", "all"):
        rows(reps, int(sys.argv[3]) if len(sys.argv) > 3 else 256)
        print()
    if what in ("cross", "all"):
        cross(reps)
        print()
    if what in ("ew", "all"):
        ew(reps)
