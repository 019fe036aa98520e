"""matchingpursuit over wavelet bases: wl_matchingpursuit_filter against what a user writes without it (GPU box).  Markdown rows.

    python tools/time_matchingpursuit.py [reps]        every row, each in a child process of its own under `timeout`; stops at the
                                                       first row that fails
    python tools/time_matchingpursuit.py row K [reps]  row K alone

Rows: Float32 standard normal signals of n samples, 64 atoms (tol far below any norm the loop reaches, nmax = 64), the bases at
their maximal depth.  Per row, alternating in one run on three rotating inputs:
  (a) fused    W.matchingpursuit(x, wts, tol, 64): the loop inside the library (wl_matchingpursuit_filter);
  (b) generic  W.matchingpursuit(x, f, ft, tol, 64) with f / ft over W.dwt_oop_ / W.idwt_oop_: the Python loop over the primitives;
  (c) today    the loop a user writes today on the same build: the transforms, torch.argmax(torch.abs(.)).item(), `r -= aphi` and
               torch.linalg.vector_norm(r).item();
  (d) floor    the K forward transforms and one inverse per atom alone, launched from Python, one synchronisation at the end.
Times are host wall time around the call, which ends synchronised, divided by the 64 atoms: median (min .. max) in milliseconds per
atom.  Before timing, the row checks that (a), (b) and (c) select the same atoms.
"""
import os, statistics, subprocess, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import wavelets_jl_amd as W

ATOMS = 64
TOL = 1e-20
ROWS = tuple((n, names) for n in (1 << 12, 1 << 16, 1 << 20) for names in (("db4",), ("haar", "db4", "sym5")))
HEADER = ("| n | bases | (a) fused ms/atom (min .. max) | (b) generic ms/atom | (c) today's loop ms/atom | (d) transforms alone ms/atom | (c) / (a) | "
          "(a) - (d) ms/atom | kernel |\n|---|---|---|---|---|---|---|---|---|")
ROW_TIMEOUT = 240


def fmt(ts):
    ts = sorted(ts)
    return f"{statistics.median(ts):.4f} ({ts[0]:.4f} .. {ts[-1]:.4f})"


def row(k, reps):
    n, names = ROWS[k]
    ws = [W.wavelet(getattr(W.WT, nm)) for nm in names]
    K, L = len(ws), W.maxtransformlevels(n)
    xs = [torch.randn(n, dtype=torch.float32, device="cuda") for _ in range(3)]
    ftr = torch.empty(K * n, dtype=torch.float32, device="cuda")
    aphi, spat = torch.empty_like(xs[0]), torch.zeros_like(xs[0])

    def ft(r):
        for j, w in enumerate(ws):
            W.dwt_oop_(ftr[j * n:(j + 1) * n], r, w, L)
        return ftr

    def fused(x):
        return W.matchingpursuit(x, ws, TOL, ATOMS)

    def f_generic(c):
        out = torch.zeros_like(aphi)
        for j, w in enumerate(ws):
            out += W.idwt(c[j * n:(j + 1) * n], w, L)
        return out

    def generic(x):
        return W.matchingpursuit(x, f_generic, ft, TOL, ATOMS)

    def today(x):
        r = x.clone()
        y = torch.zeros(K * n, dtype=torch.float32, device="cuda")
        for _ in range(ATOMS):
            if not torch.linalg.vector_norm(r).item() > TOL:
                break
            c = ft(r)
            i = torch.argmax(torch.abs(c)).item()
            j, p = divmod(i, n)
            spat[p] = c[i]
            W.idwt_oop_(aphi, spat, ws[j], L)
            spat[p] = 0
            r -= aphi
            y[i] += c[i]
        torch.cuda.synchronize()
        return y

    def floor(x):
        for _ in range(ATOMS):
            ft(x)
            W.idwt_oop_(aphi, spat, ws[0], L)
        torch.cuda.synchronize()

    # results first: the three loops pick the same atoms (torch.argmax promises no tie rule; random input has no ties)
    ya = fused(xs[0])
    kernel = W.last_kernel()
    yb, yc = generic(xs[0]), today(xs[0])
    torch.cuda.synchronize()
    assert torch.equal(ya != 0, yc != 0) and torch.equal(ya != 0, yb != 0), "the loops selected different atoms"
    for x in xs:
        fused(x); generic(x); today(x); floor(x)
    t = {"a": [], "b": [], "c": [], "d": []}
    for r in range(reps):
        x = xs[r % 3]
        for name, fn in (("a", fused), ("b", generic), ("c", today), ("d", floor)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(x)
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / ATOMS)
    ma, mc, md = (statistics.median(t[v]) for v in "acd")
    print(f"| {n} | {' + '.join(names)} | {fmt(t['a'])} | {fmt(t['b'])} | {fmt(t['c'])} | {fmt(t['d'])} | {mc / ma:.2f} | {ma - md:.4f} | {kernel} |",
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
