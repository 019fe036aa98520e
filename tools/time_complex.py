"""Complex transforms against the real batch transform of the same two planes (GPU box).  Markdown rows.

    python tools/time_complex.py [reps]

One complex array (ComplexF32) per call: wl_dwt_filter_complex / wl_dwt_lifting_complex, forward and inverse, beside the inner call
alone -- wl_dwt_filter_batch / wl_dwt_lifting_batch (images) or their batch3 forms (volumes) on the two planar component planes --
which shows what the split and the merge pass cost.  Medians of `reps` (default 20) device-event timings, cache-cold: every
repetition takes the next of three input / output sets (768 MiB per side at these sizes, above the 256 MiB of last-level cache), the
two variants alternating.
"""
import os, sys, statistics
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wavelets_jl_amd as W

SETS = 3


def medians(fns, reps):
    """fns: callables taking the set index; alternated, each timed `reps` times with device events; medians in microseconds"""
    for f in fns:
        for k in range(SETS):
            f(k)
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for i, f in enumerate(fns):
            a, b = ev[i][r]
            a.record(); f(r % SETS); b.record()
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) for a, b in e) * 1e3 for e in ev]


def colmajor(shape, dtype):
    t = torch.randn(tuple(reversed(shape)), dtype=dtype, device="cuda")
    return t.permute(*reversed(range(len(shape))))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    W.set_complex_arrays(True)
    print("| array (ComplexF32) | wavelet | direction | complex us | kernel | real batch of the 2 planes us | split + merge us (difference) | ratio |")
    print("|---|---|---|---|---|---|---|---|")
    for shape in ((4096, 4096), (256, 256, 256)):
        for wname, wt in (("db4", W.wavelet(W.WT.db4)), ("cdf9/7", W.wavelet(W.WT.cdf97, W.WT.Lifting))):
            L = W.maxtransformlevels(shape[0])
            zs = [colmajor(shape, torch.complex64) for _ in range(SETS)]
            ys = [W.similar(z) for z in zs]
            ps = [colmajor(shape + (2,), torch.float32) for _ in range(SETS)]
            qs = [W.similar(p) for p in ps]
            for fw in (True, False):
                cplx = (W.dwt_oop_ if fw else W.idwt_oop_)
                real = (W.dwt_batch if fw else W.idwt_batch)
                tc, tr = medians([lambda k: cplx(ys[k], zs[k], wt, L), lambda k: real(ps[k], wt, L, y=qs[k])], reps)
                cplx(ys[0], zs[0], wt, L)
                kern = W.last_kernel()
                name = "x".join(map(str, shape))
                print(f"| {name} | {wname} | {'dwt' if fw else 'idwt'} | {tc:.1f} | {kern} | {tr:.1f} | {tc - tr:.1f} | {tc / tr:.2f} |", flush=True)
            del zs, ys, ps, qs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
