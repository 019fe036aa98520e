"""MODWT multiresolution analysis of a batch: W.modwt_mra_batch against what a user writes without it (GPU box).  Markdown rows.

    python tools/time_modwt_mra.py [reps]        every row, each in a child process of its own under `timeout`; stops at the first
                                                 row that fails
    python tools/time_modwt_mra.py row K [reps]  row K alone

Rows: Float32 db4, coefficients from W.modwt_batch of standard normal units.  Per row, alternating in one run on three rotating sets
of buffers (each set is larger than the 256 MB Infinity Cache for the large rows, so a call finds none of its data there):
  mra     W.modwt_mra_batch(xw, wt, y=y) as dispatched (the LDS tier where the unit fits);
  levels  the same call under WL_MODWT_FUSED = 0 (the per-level tier), where both tiers apply;
  loop    (a) the loop a user writes today, on the same build: for every column zero a scratch tensor, copy the column in, run
          W.imodwt_batch.
Times are device-event medians in microseconds, min .. max beside them.  Before timing, the row checks that mra == loop on the
device (torch.equal: by value) and that the two tiers give the same bytes.
"""
import os, statistics, subprocess, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import wavelets_jl_amd as W

ROWS = ((64, 65536, 6), (1024, 4096, 10), (8192, 512, 13), (1 << 20, 16, 8))        # (n, B, L)
HEADER = ("| units x n (L) | mra us (min .. max) | kernel | per-level tier us (min .. max) | loop of imodwt_batch us (min .. max) | loop / mra | "
          "per-level / mra | mra GB/s (algorithmic) |\n|---|---|---|---|---|---|---|---|")
ROW_TIMEOUT = 240


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record()
    return a, b


def fmt(ts):
    ts = sorted(ts)
    return f"{statistics.median(ts):.1f} ({ts[0]:.1f} .. {ts[-1]:.1f})"


def row(k, reps):
    n, B, L = ROWS[k]
    wt = W.wavelet(W.WT.db4)
    sets = []
    for s in range(3):
        x = torch.randn(B, n, dtype=torch.float32, device="cuda").t()
        xw = W.modwt_batch(x, wt, L)
        sets.append((xw, W.similar(xw), W.similar(xw), torch.empty((B, n), dtype=torch.float32, device="cuda").t()))
        del x
    both = 2 * n * 4 <= 65536

    def mra(s):
        W.modwt_mra_batch(s[0], wt, y=s[1])

    def levels(s):
        with W.options(WL_MODWT_FUSED=0):
            W.modwt_mra_batch(s[0], wt, y=s[1])

    def loop(s, keep=None):
        xw, _, z, _ = s
        for c in range(L + 1):
            z.zero_()
            z[:, c, :].copy_(xw[:, c, :])
            col = W.imodwt_batch(z, wt)
            if keep is not None:
                keep[:, c, :].copy_(col)

    # results first: the call is the loop, and the tiers agree
    s0 = sets[0]
    mra(s0)
    kernel = W.last_kernel()
    want = W.similar(s0[0])
    loop(s0, want)
    torch.cuda.synchronize()
    assert torch.equal(s0[1], want), "modwt_mra_batch differs from the loop of imodwt_batch"
    if both:
        first = s0[1].clone()
        levels(s0)
        assert W.last_kernel() == "k_modwt_mra_step_b"
        torch.cuda.synchronize()
        assert torch.equal(first.view(torch.int32), s0[1].view(torch.int32)), "the two tiers differ"
        del first
    del want
    for s in sets:                                        # warm every buffer set on every path
        mra(s); loop(s)
        if both:
            levels(s)
    torch.cuda.synchronize()
    ev = {"mra": [], "levels": [], "loop": []}
    for r in range(reps):
        s = sets[r % 3]
        ev["mra"].append(timed(lambda: mra(s)))
        if both:
            ev["levels"].append(timed(lambda: levels(s)))
        ev["loop"].append(timed(lambda: loop(s)))
    torch.cuda.synchronize()
    t = {name: [a.elapsed_time(b) * 1e3 for a, b in pairs] for name, pairs in ev.items()}
    m = statistics.median(t["mra"])
    lv = fmt(t["levels"]) if both else "-"
    ratio = f"{statistics.median(t['levels']) / m:.2f}" if both else "-"
    gbs = 2 * n * (L + 1) * B * 4 / m / 1e3                # every coefficient read once, every result written once
    print(f"| {B} x {n} ({L}) | {fmt(t['mra'])} | {kernel} | {lv} | {fmt(t['loop'])} | {statistics.median(t['loop']) / m:.2f} | {ratio} | {gbs:.0f} |",
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "row":
        row(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 21)
        sys.exit(0)
    reps = sys.argv[1] if len(sys.argv) > 1 else "21"
    print(HEADER, flush=True)
    for k in range(len(ROWS)):
        rc = subprocess.call(["timeout", "-k", "10", str(ROW_TIMEOUT), sys.executable, os.path.abspath(__file__), "row", str(k), reps])
        if rc:
            sys.exit(f"row {k} ended with status {rc}: nothing more is started on the device")
