"""Device timings of the best-basis search: python tools/time_bestbasis.py [--profile]  (GPU box).  Markdown rows.

Each case is the median of 20 calls, cache-cold (a 512 MiB buffer is rewritten between calls, twice the MI355X's last-level
cache), wall time from the call to its return -- bestbasistree synchronises once to hand back the tree, so this is what a caller
waits for.  The floor next to it is wpt(x, wt, Lmax) at the same size, timed the same way (call + synchronisation): the packet work
of every depth that the search cannot avoid.  --profile runs one call of each case (for rocprofv3 --kernel-trace --stats).
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavelets_jl_amd as W

PROFILE = "--profile" in sys.argv
REPS = 1 if PROFILE else 20
flush = torch.empty(128 << 20, dtype=torch.float32, device="cuda")


def t_us(fn):
    ts = []
    for _ in range(REPS + (0 if PROFILE else 2)):
        flush.fill_(1.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts[-REPS:])


print("| n | dtype | wavelet | bestbasistree us | wpt(x, wt, Lmax) us | ratio |")
print("|---|---|---|---|---|---|")
rng = np.random.default_rng(11)
for pw in (20, 22, 24):
    n = 1 << pw
    base = W.testfunction(n, "Doppler") + 0.05 * rng.standard_normal(n)
    for dt in (np.float32, np.float64):
        x = W.to_device(base.astype(dt))
        tree = W.maketree(n)
        for name in ("haar", "db4", "sym5"):
            wt = W.wavelet(getattr(W.WT, name))
            W.bestbasistree(x, wt, tree)                     # grows the workspace once
            tb = t_us(lambda: W.bestbasistree(x, wt, tree))
            tw = t_us(lambda: W.wpt(x, wt, pw))
            print(f"| 2^{pw} | {np.dtype(dt).name} | {name} | {tb:.0f} | {tw:.0f} | {tb / tw:.2f} |", flush=True)
